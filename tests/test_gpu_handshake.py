"""GPU: HKDF-SHA256 kernel (hkdf.hip) and the batched handshake driver
(qrk_handshake_batch) vs the oracle, through the C ABI.  Bar: byte-exact.

The driver is generic over families, so every family runs through it here against the oracle's
handshake: ML-KEM and FrodoKEM-640-SHAKE by golden digests, and HQC-128 / 192 / 256 (a 64-byte shared
secret: HKDF's extract hash absorbs one whole block after the ipad block and pads in a block of its own),
FrodoKEM-976-SHAKE, FrodoKEM-1344-AES and FrodoKEM-640-AES (24-, 32- and 16-byte secrets) recomputed;
one call derives 33-byte keys.  HKDF's own length edges are in tests/test_gpu_hkdf_edges.py.

`agree`, the word bench.py counts as key_disagreements, is 1 on every honest handshake, so the compare
that writes it (k_keys_equal) is driven on chosen rows through qrk_dbg_keys_equal: one differing bit per
row at every byte and bit position, differences that straddle two rows, n around one workgroup, and a
prefilled output with a guard word.  The reference is numpy's (a == b).all(axis=1).
"""
import hashlib
import json

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kdf():
    from qrkem.handshake import KeyDerivation
    return KeyDerivation(device=0)


def test_rfc5869_vectors_on_gpu(kdf):
    from test_handshake_oracle import RFC5869
    for ikm, salt, info, L, _prk, okm in RFC5869:
        out = kdf.derive(np.frombuffer(ikm, np.uint8).reshape(1, -1), info, L, salt=salt or None)
        assert out[0].tobytes().hex() == okm


@pytest.mark.parametrize("ikm_len,L,salt_len", [(32, 32, 0), (16, 16, 0), (24, 24, 13), (32, 33, 64),
                                                (32, 100, 65), (1, 1, 200), (32, 8160, 0)])
def test_hkdf_ragged_infos_match_oracle(kdf, ikm_len, L, salt_len):
    import oracle as orc
    rng = np.random.default_rng(ikm_len * 1000 + L + salt_len)
    n = 37 if L < 1000 else 5
    ikm = rng.integers(0, 256, (n, ikm_len), dtype=np.uint8)
    infos = [rng.integers(0, 256, int(rng.integers(0, 300)), dtype=np.uint8).tobytes() for _ in range(n)]
    infos[0] = b""
    salt = rng.integers(0, 256, salt_len, dtype=np.uint8).tobytes() or None
    dev = kdf.derive(torch.from_numpy(ikm).cuda(), infos, L, salt=salt)
    torch.cuda.synchronize()
    ref = orc.batch_hkdf(ikm, infos, L, salt=salt)
    assert np.array_equal(dev.cpu().numpy(), ref)


def test_hkdf_shared_info_large_batch(kdf):
    import oracle as orc
    from qrkem.handshake import protocol_info
    info = protocol_info("b" * 36, "a" * 36, "AES-256-GCM")
    n = 70000
    ikm = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda")
    out = kdf.derive(ikm, info, 32).cpu().numpy()
    h = ikm.cpu().numpy()
    idx = list(range(0, n, 997)) + [n - 1]
    ref = orc.batch_hkdf(np.ascontiguousarray(h[idx]), [info] * len(idx), 32)
    assert np.array_equal(out[idx], ref)


@pytest.mark.parametrize("case", range(4))
def test_handshake_driver_matches_golden(golden_dir, case):
    from make_golden_handshake import CASES, inputs
    from qrkem.handshake import HandshakeDriver
    alg, n, sym = CASES[case]
    g = json.loads((golden_dir / "handshake.json").read_text())[f"{alg}|{n}|{sym}"]
    kpi, kpr, en, infos = inputs(alg, n, sym)
    drv = HandshakeDriver(alg, symmetric_name=sym)
    out = drv.run(infos, coins_kp_initiator=kpi, coins_kp_responder=kpr, coins_encaps=en)
    torch.cuda.synchronize()
    got = {"pk_i": out.pk_initiator, "pk_r": out.pk_responder, "ct": out.ciphertext, "key_i": out.key_initiator,
           "key_r": out.key_responder}
    for k, t in got.items():
        assert hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest() == g["digests"][k], k
    assert bool((out.agree == 1).all())


def test_handshake_driver_multi_chunk_random_coins():
    """OS-CSPRNG coins, batch larger than one chunk: both sides must agree everywhere."""
    from qrkem.handshake import HandshakeDriver
    drv = HandshakeDriver("ML-KEM-768", chunk=4096)
    n = 10000
    infos = [drv.info_for(f"peer-{i}", "server", ) for i in range(n)]
    out = drv.run(infos)
    torch.cuda.synchronize()
    assert int(out.agree.sum()) == n
    assert torch.equal(out.key_initiator, out.key_responder)
    assert not torch.equal(out.key_initiator[0], out.key_initiator[1])


def test_key_derivation_host_inputs(kdf):
    import hkdf_spec
    ss = [bytes(range(32)), bytes(range(32, 64))]
    info = hkdf_spec.protocol_info("x", "y", "ChaCha20-Poly1305")
    out = kdf.derive(ss, [info, info], 32)
    for i in range(2):
        assert out[i].tobytes() == hkdf_spec.hkdf_sha256(ss[i], info, 32)


@pytest.mark.parametrize("alg,n,chunk", [("ML-KEM-512", 3000, 2048), ("ML-KEM-768", 3000, 2048),
                                         ("ML-KEM-1024", 3000, 2048), ("ML-KEM-768", 1089, 1088)])
def test_handshake_driver_expanded_key_reuse_matches_oracle(alg, n, chunk):
    """Batched ML-KEM chunks (> 1024 handshakes) keep the initiator's sampled matrix A_hat from its
    KeyGen (messaging.py:590) for its Decaps (:1038) instead of re-running SampleNTT; the last chunk
    (952, or a single handshake) runs the one-launch kernels without reuse; 1088 is the first
    batched chunk size, a ragged 64-handshake tile.  Every output byte-exact vs the oracle's
    handshake (a wrong A_hat would re-encrypt differently and select the implicit-rejection key)."""
    import oracle as orc
    import hkdf_spec
    from make_golden_handshake import node_id
    from qrkem.handshake import HandshakeDriver
    sym = "AES-256-GCM"
    s = orc.sizes(alg)
    kp, enc = s["keypair_coins"], s["encaps_coins"]
    coins = orc.bench_coins(n, 2 * kp + enc, seed=0xA11 + kp)
    kpi, kpr, en = (np.ascontiguousarray(coins[:, a:b]) for a, b in ((0, kp), (kp, 2 * kp), (2 * kp, 2 * kp + enc)))
    infos = [hkdf_spec.protocol_info(node_id(b"a", i), node_id(b"b", i), sym) for i in range(n)]
    drv = HandshakeDriver(alg, symmetric_name=sym, chunk=chunk)
    out = drv.run(infos, coins_kp_initiator=kpi, coins_kp_responder=kpr, coins_encaps=en)
    torch.cuda.synchronize()
    want = orc.batch_handshake(alg, kpi, kpr, en, infos, hkdf_spec.SYMMETRIC_KEY_SIZE[sym])
    got = (out.pk_initiator, out.pk_responder, out.ciphertext, out.key_initiator, out.key_responder)
    for name, g, w in zip(("pk_i", "pk_r", "ct", "key_i", "key_r"), got, want):
        assert np.array_equal(g.cpu().numpy(), w), name
    assert bool((out.agree == 1).all())


def _fixed_inputs(alg, n, seed):
    import oracle as orc
    import hkdf_spec
    from make_golden_handshake import node_id
    s = orc.sizes(alg)
    kp, enc = s["keypair_coins"], s["encaps_coins"]
    coins = orc.bench_coins(n, 2 * kp + enc, seed=seed + kp)
    kpi, kpr, en = (np.ascontiguousarray(coins[:, a:b]) for a, b in ((0, kp), (kp, 2 * kp), (2 * kp, 2 * kp + enc)))
    infos = [hkdf_spec.protocol_info(node_id(b"a", i), node_id(b"b", i), "AES-256-GCM") for i in range(n)]
    return s, kpi, kpr, en, infos


@pytest.mark.parametrize("alg,n", [("HQC-128", 5), ("HQC-192", 5), ("HQC-256", 5), ("FrodoKEM-976-SHAKE", 3),
                                   ("FrodoKEM-1344-AES", 3), ("FrodoKEM-640-AES", 3)])
def test_handshake_driver_every_family_matches_oracle(alg, n):
    """The families the golden cases leave out, recomputed by the oracle's own handshake
    (orc.batch_handshake takes every one of these names): shared secrets of 64 (HQC), 24, 32 and 16 bytes
    through the same HKDF and compare.  Every output byte-exact, agree all 1."""
    import oracle as orc
    from qrkem.handshake import HandshakeDriver
    s, kpi, kpr, en, infos = _fixed_inputs(alg, n, 0xE6E5)
    assert s["ss"] == {"HQC": 64, "FrodoKEM-976": 24, "FrodoKEM-1344": 32, "FrodoKEM-640": 16}[alg.rsplit("-", 1)[0]]
    drv = HandshakeDriver(alg, symmetric_name="AES-256-GCM")
    out = drv.run(infos, coins_kp_initiator=kpi, coins_kp_responder=kpr, coins_encaps=en)
    torch.cuda.synchronize()
    want = orc.batch_handshake(alg, kpi, kpr, en, infos, 32)
    got = (out.pk_initiator, out.pk_responder, out.ciphertext, out.key_initiator, out.key_responder)
    for name, g, w in zip(("pk_i", "pk_r", "ct", "key_i", "key_r"), got, want):
        assert np.array_equal(g.cpu().numpy(), w), name
    assert np.array_equal(want[3], want[4])
    assert out.agree.cpu().tolist() == [1] * n


def test_handshake_abi_33_byte_keys_match_oracle():
    """qrk_handshake_batch itself with key_len = 33 (one byte of T(2); rows of the key arrays at an odd
    stride, for the compare too), ML-KEM-512, n = 70: one wave and six lanes."""
    import oracle as orc
    from qrkem._native import LIB, last_error
    from qrkem.batch import BatchKEM
    from qrkem.handshake import PackedInfos, _dev, _ptr
    alg, n, key_len = "ML-KEM-512", 70, 33
    s, kpi, kpr, en, infos = _fixed_inputs(alg, n, 0x33)
    e = BatchKEM(alg, device=0)
    inf = PackedInfos(infos, n, 0)
    coins = [_dev(c, 0) for c in (kpi, kpr, en)]
    pk_i, pk_r, c = e._empty(n, s["pk"]), e._empty(n, s["pk"]), e._empty(n, s["ct"])
    keys = torch.full((2, n * key_len + 64), 0xA5, dtype=torch.uint8, device="cuda")
    agree = torch.full((n + 1,), 7, dtype=torch.int32, device="cuda")
    rc = LIB.qrk_handshake_batch(e._ctx, e._name, n, *[_ptr(x) for x in coins], _ptr(inf.data), _ptr(inf.off), 0,
                                 key_len, _ptr(pk_i), _ptr(pk_r), _ptr(c), _ptr(keys[0]), _ptr(keys[1]), _ptr(agree),
                                 e._stream())
    assert rc == 0, last_error()
    torch.cuda.synchronize()
    want = orc.batch_handshake(alg, kpi, kpr, en, infos, key_len)
    k = keys.cpu().numpy()
    got = (pk_i.cpu().numpy(), pk_r.cpu().numpy(), c.cpu().numpy(), k[0, :n * key_len].reshape(n, key_len),
           k[1, :n * key_len].reshape(n, key_len))
    for name, g, w in zip(("pk_i", "pk_r", "ct", "key_i", "key_r"), got, want):
        assert np.array_equal(g, w), name
    assert (k[:, n * key_len:] == 0xA5).all()
    assert agree.cpu().tolist() == [1] * n + [7]


# ---- the key compare on chosen rows (qrk_dbg_keys_equal)

def _keys_equal(a, b):
    """agree of qrk_dbg_keys_equal for host rows a, b [n][len]; the output is prefilled with 7 and has one
    guard word, which must stay, and every other word must be exactly 0 or 1."""
    from qrkem._debug import bind
    from qrkem._native import last_error
    n, length = a.shape
    a_d, b_d = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (a, b))
    agree = torch.full((n + 1,), 7, dtype=torch.int32, device="cuda")
    rc = bind().qrk_dbg_keys_equal(n, a_d.data_ptr(), b_d.data_ptr(), length, agree.data_ptr(),
                                   torch.cuda.current_stream(0).cuda_stream)
    assert rc == 0, last_error()
    torch.cuda.synchronize()
    out = agree.cpu().numpy()
    assert out[n] == 7, "the word behind agree[n - 1] was written"
    assert np.isin(out[:n], (0, 1)).all(), f"words other than 0 / 1: {sorted(set(out[:n].tolist()) - {0, 1})}"
    return out[:n]


def _check_compare(a, b, what):
    want = (a == b).all(axis=1).astype(np.int32)
    got = _keys_equal(a, b)
    w = np.nonzero(got != want)[0]
    assert len(w) == 0, f"{what}: agree wrong on {len(w)} of {len(want)} rows, first {w[:8].tolist()}, " \
                        f"got {got[w[:8]].tolist()}"
    return want


@pytest.mark.parametrize("length", [16, 32, 33])
def test_keys_equal_sees_every_single_bit(length):
    """Odd row 2k + 1 differs in bit k % 8 of byte k // 8 and nowhere else; even rows are equal."""
    rng = np.random.default_rng(length)
    n = 2 * 8 * length
    a = rng.integers(0, 256, (n, length), dtype=np.uint8)
    b = a.copy()
    k = np.arange(8 * length)
    b[2 * k + 1, k // 8] ^= (1 << (k % 8)).astype(np.uint8)
    want = _check_compare(a, b, f"len {length}")
    assert want.tolist() == [1, 0] * (8 * length)


def test_keys_equal_longest_key():
    length = 8160
    pos = [0, 31, 32, length // 2, length - 1]
    rng = np.random.default_rng(8160)
    a = rng.integers(0, 256, (2 * len(pos), length), dtype=np.uint8)
    b = a.copy()
    for r, p in enumerate(pos):
        b[2 * r + 1, p] ^= 0x80 >> (r % 8)
    want = _check_compare(a, b, "len 8160")
    assert want.tolist() == [1, 0] * len(pos)


@pytest.mark.parametrize("length", [16, 32, 33])
@pytest.mark.parametrize("n", [255, 256, 257])
def test_keys_equal_row_stride_and_batch_geometry(n, length):
    """A difference in the last byte of row i and the first byte of row i + 1 only: exactly those two rows
    disagree under the right stride; a wrong one moves or merges them."""
    rng = np.random.default_rng(1000 * n + length)
    a = rng.integers(0, 256, (n, length), dtype=np.uint8)
    b = a.copy()
    pairs = [3, 100, n - 2]
    for i in pairs:
        b[i, length - 1] ^= 0x01
        b[i + 1, 0] ^= 0x80
    want = _check_compare(a, b, f"n {n} len {length}")
    assert np.nonzero(want == 0)[0].tolist() == [3, 4, 100, 101, n - 2, n - 1]
    # a single byte at the very end of the batch, and at the very start
    for r, p in ((n - 1, length - 1), (0, 0)):
        b = a.copy()
        b[r, p] ^= 0x10
        want = _check_compare(a, b, f"n {n} len {length} row {r}")
        assert np.nonzero(want == 0)[0].tolist() == [r]


@pytest.mark.parametrize("n", [255, 256, 257])
def test_keys_equal_all_equal_and_all_different(n):
    rng = np.random.default_rng(n)
    a = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    assert _check_compare(a, a.copy(), "all equal").all()
    assert not _check_compare(a, ~a, "all different").any()
    b = a.copy()
    b[:, 31] ^= 1  # every row, last byte only
    assert not _check_compare(a, b, "all different in the last byte").any()
