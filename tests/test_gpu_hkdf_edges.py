"""GPU: HKDF-SHA256 (k_hkdf_sha256, padding by sha::tail) at every length where one-lane SHA-256 with
hand-rolled padding can go wrong, against `hkdf_ref` of tests/hkdf_cases.py (hmac / hashlib).

The tables are those of tests/hkdf_cases.py; tests/test_hkdf_cases.py proves on the CPU that they put every
hash of the kernel on both sides of the padding seams 55 | 56 and 63 | 0 and through 1, 2 and 3 blocks:
* info lengths 0..191 as one ragged batch with L = 96 (r = 1 hashes info || 01, r = 2, 3 splice T(r-1) in
  front through word_over), and twelve of them again as one shared string (info_off NULL);
* IKM lengths 1..128 with all-zero, all-ones and random rows; salts None..200 with the switch to a hashed
  key at 64 | 65, and the zero-padding identities of RFC 2104;
* output lengths around one and two T blocks and at 8160, through the C ABI into a prefilled buffer with a
  guard behind it; n = 1, 255, 256, 257 (one workgroup is 256 lanes); one 1000-byte info.
Bar: byte-exact.  Each test is a handful of small launches.
"""
import ctypes as ct

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import hkdf_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu

FILL, GUARD = 0xA5, 64


@pytest.fixture(scope="module")
def kdf():
    from qrkem.handshake import KeyDerivation
    return KeyDerivation(device=0)


def _rows(rows):
    return np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), -1)


def _want(salt, ikm_rows, infos, L):
    infos = [infos] * len(ikm_rows) if isinstance(infos, bytes) else infos
    return _rows([K.hkdf_ref(salt, k, i, L) for k, i in zip(ikm_rows, infos)])


def _derive(kdf, salt, ikm_rows, infos, L):
    out = kdf.derive(torch.from_numpy(_rows(ikm_rows).copy()).cuda(), infos, L, salt=salt)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _differ(got, want):
    w = np.nonzero((got != want).any(axis=1))[0]
    return f"{len(w)} of {len(want)} rows differ, first: {w[:8].tolist()}"


def _abi(kdf, ikm_rows, infos, L, salt=None):
    """qrk_hkdf_sha256_batch into an okm buffer of n L + GUARD bytes prefilled with FILL: (rc, buffer)."""
    from qrkem._native import LIB
    from qrkem.handshake import PackedInfos, _ptr
    n = len(ikm_rows)
    ikm = torch.from_numpy(_rows(ikm_rows).copy()).cuda()
    inf = PackedInfos(infos, n, 0)
    okm = torch.full((n * max(L, 1) + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    salt_t = torch.from_numpy(np.frombuffer(salt, np.uint8).copy()).cuda() if salt else None
    stream = ct.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    rc = LIB.qrk_hkdf_sha256_batch(kdf._ctx, n, _ptr(ikm), ikm.shape[1], _ptr(salt_t), len(salt) if salt else 0,
                                   _ptr(inf.data), _ptr(inf.off), inf.length, _ptr(okm), L, stream)
    torch.cuda.synchronize()
    return rc, okm.cpu().numpy()


def test_info_lengths_0_to_191_one_ragged_batch(kdf):
    got = _derive(kdf, None, K.INFO_IKM, K.INFO_ROWS, K.INFO_L)
    want = _want(None, K.INFO_IKM, K.INFO_ROWS, K.INFO_L)
    for r in range(3):  # T(1), T(2), T(3): which hash went wrong
        s = slice(32 * r, 32 * r + 32)
        assert np.array_equal(got[:, s], want[:, s]), f"T({r + 1}): info lengths {_differ(got[:, s], want[:, s])}"


def test_shared_info_equals_the_per_row_form(kdf):
    ikm = K.INFO_IKM[:K.SHARED_N]
    for n in K.SHARED_INFO_LENS:
        info = K.INFO_ROWS[n]
        shared = _derive(kdf, None, ikm, info, K.INFO_L)
        per_row = _derive(kdf, None, ikm, [info] * K.SHARED_N, K.INFO_L)
        assert np.array_equal(shared, per_row), f"info length {n}: shared and per-row forms differ"
        assert np.array_equal(shared, _want(None, ikm, info, K.INFO_L)), f"info length {n}"


def test_ikm_lengths(kdf):
    for n in K.IKM_LENS:
        rows = K.ikm_rows(n)
        got = _derive(kdf, None, rows, K.INFO_110, K.IKM_L)
        want = _want(None, rows, K.INFO_110, K.IKM_L)
        assert np.array_equal(got, want), f"IKM length {n}: {_differ(got, want)} (0: zeros, 1: ones)"


def test_salt_lengths(kdf):
    for n in K.SALT_LENS:
        salt = K.salt_of(n)
        got = _derive(kdf, salt, K.SALT_IKM, K.INFO_110, K.SALT_L)
        want = _want(salt, K.SALT_IKM, K.INFO_110, K.SALT_L)
        assert np.array_equal(got, want), f"salt length {n}: {_differ(got, want)}"


def test_zero_salts_are_one_key_and_65_zeros_another(kdf):
    """Through the C ABI, so that a one-byte and an all-zero salt reach the kernel as given."""
    outs = []
    for salt in K.ZERO_SALTS_EQUAL + [K.ZERO_SALT_OTHER]:
        rc, buf = _abi(kdf, K.SALT_IKM, K.INFO_110, K.SALT_L, salt=salt)
        assert rc == 0
        got = buf[:K.SALT_N * K.SALT_L].reshape(K.SALT_N, K.SALT_L)
        assert np.array_equal(got, _want(salt, K.SALT_IKM, K.INFO_110, K.SALT_L)), salt and len(salt)
        outs.append(got)
    assert all(np.array_equal(o, outs[0]) for o in outs[:-1])
    assert not (outs[-1] == outs[0]).all(axis=1).any()


def test_output_lengths_fill_their_rows_and_nothing_else(kdf):
    """n = 3 rows of L bytes in a buffer prefilled with 0xA5: every row exact (so no row's last, partial T
    block ran into the next row), the 64 bytes behind the last row untouched, and okm(L) a prefix of
    okm(8160)."""
    full = _want(None, K.OUT_IKM, K.INFO_110, K.MAX_L)
    for L in K.OUT_LENS:
        rc, buf = _abi(kdf, K.OUT_IKM, K.INFO_110, L)
        assert rc == 0
        got = buf[:K.OUT_N * L].reshape(K.OUT_N, L)
        assert np.array_equal(got, _want(None, K.OUT_IKM, K.INFO_110, L)), f"L = {L}: {_differ(got, full[:, :L])}"
        assert np.array_equal(got, full[:, :L]), f"L = {L}: not a prefix of okm(8160)"
        assert (buf[K.OUT_N * L:] == FILL).all(), f"L = {L}: bytes written behind the last row"


@pytest.mark.parametrize("L", K.OUT_REFUSED)
def test_refused_output_lengths_write_nothing(kdf, L):
    from qrkem._native import last_error
    rc, buf = _abi(kdf, K.OUT_IKM, K.INFO_110, L)
    assert rc == -1
    assert "8160" in last_error()
    assert (buf == FILL).all()


@pytest.mark.parametrize("n", K.GEOMETRY_N)
def test_batch_geometry(kdf, n):
    """Row i has an info of i bytes; L = 33 leaves one byte in the second T block."""
    ikm, infos = K.geometry_rows(n)
    rc, buf = _abi(kdf, ikm, infos, K.GEOMETRY_L)
    assert rc == 0
    got = buf[:n * K.GEOMETRY_L].reshape(n, K.GEOMETRY_L)
    want = _want(None, ikm, infos, K.GEOMETRY_L)
    assert np.array_equal(got, want), f"n = {n}: {_differ(got, want)}"
    assert (buf[n * K.GEOMETRY_L:] == FILL).all(), f"n = {n}: bytes written behind the last row"


def test_one_long_info(kdf):
    ikm = K.OUT_IKM[:2]
    got = _derive(kdf, None, ikm, K.LONG_INFO, K.LONG_L)
    assert np.array_equal(got, _want(None, ikm, K.LONG_INFO, K.LONG_L))
    got = _derive(kdf, None, ikm, [K.LONG_INFO, K.LONG_INFO[:999]], K.LONG_L)
    assert np.array_equal(got, _want(None, ikm, [K.LONG_INFO, K.LONG_INFO[:999]], K.LONG_L))
