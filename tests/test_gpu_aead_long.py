"""GPU: the long AEAD calls (aead_long.hip: one row across many workgroups) through the C ABI, their MAC hooks
and the routing in qrkem.symmetric.  Bar: byte-exact against tests/golden/aead_long.json (sealed by OpenSSL),
against the one-lane calls and against tests/aead_spec.py; every tampered row refused with no plaintext byte
written; nothing left in the segment-partial scratch."""
import ctypes as ct
import hashlib
import json

import numpy as np
import pytest

import aead_spec
import make_golden_aead_long as gen

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

ALGS = aead_spec.ALGS
S, C = gen.S, gen.C
FILL = 0xA5


@pytest.fixture(scope="module")
def golden(golden_dir):
    return json.loads((golden_dir / "aead_long.json").read_text())["records"]


@pytest.fixture(scope="module")
def ciphers():
    from qrkem.symmetric import BY_NAME
    return {alg: BY_NAME[alg](device=0) for alg in ALGS}


def dev(b: bytes):
    return torch.from_numpy(np.frombuffer(bytes(b) or b"\0", dtype=np.uint8).copy()).cuda()


def offsets(rows):
    return torch.from_numpy(np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)).cuda()


def ptr(t):
    return ct.c_void_p(t.data_ptr()) if t is not None else None


def residue(ctx) -> int:
    from qrkem._debug import bind
    out = ct.c_uint64(123)
    assert bind().qrk_dbg_aead_long_residue(ctx, ct.byref(out)) == 0
    return out.value


def seal(ctx, alg, keys, nonces, pts, aads, max_len, long=True):
    """The sealed buffer (pt_off[n] + 28 n bytes over a FILL prefill) of qrk_aead_seal_long_batch, or of
    qrk_aead_seal_batch with long=False."""
    from qrkem import last_error
    from qrkem._native import LIB
    n = len(pts)
    out = torch.full((sum(map(len, pts)) + 28 * n,), FILL, dtype=torch.uint8, device="cuda")
    bufs = [dev(b"".join(keys)), dev(b"".join(nonces)), dev(b"".join(pts)), offsets(pts), dev(b"".join(aads)),
            offsets(aads)]
    args = [ctx, alg.encode(), n] + [ptr(b) for b in bufs] + [0]
    rc = (LIB.qrk_aead_seal_long_batch(*args, max_len, ptr(out), None) if long
          else LIB.qrk_aead_seal_batch(*args, ptr(out), None))
    assert rc == 0, last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy().tobytes()


def open_(ctx, alg, keys, sealed, aads, max_len, long=True):
    """(the plaintext buffer over a FILL prefill, status) of qrk_aead_open_long_batch / qrk_aead_open_batch."""
    from qrkem import last_error
    from qrkem._native import LIB
    n = len(sealed)
    out = torch.full((sum(map(len, sealed)) - 28,), FILL, dtype=torch.uint8, device="cuda")
    status = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    bufs = [dev(b"".join(keys)), dev(b"".join(sealed)), offsets(sealed), dev(b"".join(aads)), offsets(aads)]
    args = [ctx, alg.encode(), n] + [ptr(b) for b in bufs] + [0]
    rc = (LIB.qrk_aead_open_long_batch(*args, max_len, ptr(out), ptr(status), None) if long
          else LIB.qrk_aead_open_batch(*args, ptr(out), ptr(status), None))
    assert rc == 0, last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy().tobytes(), status.cpu().numpy().tolist()


def split(buf: bytes, lens, per_row: int):
    """Row i of a buffer laid out at offset sum(lens[:i]) + per_row i, len lens[i] + max(per_row, 0)."""
    out, o = [], 0
    for i, l in enumerate(lens):
        out.append(buf[o:o + l + max(per_row, 0)])
        o += l + per_row
    return out


def flip(b: bytes, byte: int, bit: int = 0) -> bytes:
    a = bytearray(b)
    a[byte] ^= 1 << bit
    return bytes(a)


@pytest.mark.parametrize("alg", ALGS)
def test_fixture_records_seal_and_open(ciphers, golden, alg):
    """Every record of the fixture in one batch: tag, ciphertext digest and end bytes as OpenSSL's; Open
    returns the plaintext with status 0; the partial scratch is zero after each call."""
    ctx = ciphers[alg]._context()
    recs = [r for r in golden if r["alg"] == alg]
    rows = [gen.inputs(alg, r["record"], r["pt_len"], r["aad_len"]) for r in recs]
    keys, nonces, aads, pts = (list(x) for x in zip(*rows))
    lens = [len(p) for p in pts]
    sealed = split(seal(ctx, alg, keys, nonces, pts, aads, max(lens)), lens, 28)
    assert residue(ctx) == 0
    for r, row, nonce in zip(recs, sealed, nonces):
        assert row[:12] == nonce and gen.summary(alg, r["record"], r["pt_len"], r["aad_len"], row) == r, r["record"]
    plain, status = open_(ctx, alg, keys, sealed, aads, max(lens))
    assert status == [0] * len(recs) and residue(ctx) == 0
    assert [hashlib.sha256(p).digest() for p in split(plain, lens, 0)] == [hashlib.sha256(p).digest() for p in pts]


def four_rows(alg):
    """Rows of 2S + 17, 0 and S - 1 bytes and one of 2S + 18 (above max_len = 2S + 17), fixed nonces, per-row aad."""
    rng = np.random.default_rng(4242 + len(alg))
    lens = [2 * S + 17, 0, S - 1, 2 * S + 18]
    keys, nonces = [rng.bytes(32) for _ in lens], [rng.bytes(12) for _ in lens]
    return keys, nonces, [rng.bytes(l) for l in lens], [rng.bytes(a) for a in (13, 100, 0, 16)], lens


@pytest.mark.parametrize("alg", ALGS)
def test_agrees_with_the_one_lane_calls_and_leaves_a_row_above_max_len_alone(ciphers, alg):
    ctx = ciphers[alg]._context()
    keys, nonces, pts, aads, lens = four_rows(alg)
    max_len = 2 * S + 17
    want = split(seal(ctx, alg, keys, nonces, pts, aads, 0, long=False), lens, 28)
    got = split(seal(ctx, alg, keys, nonces, pts, aads, max_len), lens, 28)
    assert got[:3] == want[:3]
    assert got[3] == bytes([FILL]) * (lens[3] + 28)  # above max_len: left unwritten
    assert residue(ctx) == 0
    # Open: the same three rows, and the sealed long row (one byte above max_len) refused and untouched
    old_plain, old_status = open_(ctx, alg, keys, want, aads, 0, long=False)
    plain, status = open_(ctx, alg, keys, want, aads, max_len)
    assert old_status == [0, 0, 0, 0] and status == [0, 0, 0, -1]
    assert split(plain, lens, 0)[:3] == split(old_plain, lens, 0)[:3] == pts[:3]
    assert split(plain, lens, 0)[3] == bytes([FILL]) * lens[3]
    assert residue(ctx) == 0


@pytest.mark.parametrize("alg", ALGS)
def test_every_tampered_row_is_refused_and_zeroed(ciphers, alg):
    """One bit flipped at the edges of the ciphertext and of the segments (the row's segments are counted from
    its end: 16 bytes, then two of S, so byte 15 | 16 and S + 15 | S + 16 are its own seams; S - 1 | S is the
    seam of a cut from the front), in each tag byte, in the nonce and in the aad."""
    ctx = ciphers[alg]._context()
    rng = np.random.default_rng(99 + len(alg))
    key, nonce, pt, aad = rng.bytes(32), rng.bytes(12), rng.bytes(2 * S + 17), rng.bytes(13)
    good = aead_spec.seal(alg, key, nonce, pt[:64], aad)  # a short honest row from the spec ...
    honest = split(seal(ctx, alg, [key], [nonce], [pt], [aad], len(pt)), [len(pt)], 28)[0]
    assert honest[:12 + 64] == good[:12 + 64]  # ... pins the long row's first bytes
    n_ct = len(pt)
    at = [0, 15, 16, S - 1, S, S + 15, S + 16, n_ct - 1]
    rows = [flip(honest, 12 + p, p % 8) for p in at] + [flip(honest, 12 + n_ct + t, t % 8) for t in range(16)]
    rows += [flip(honest, 5, 3), honest, honest]
    aads = [aad] * (len(rows) - 2) + [flip(aad, 7, 1), aad]
    plain, status = open_(ctx, alg, [key] * len(rows), rows, aads, n_ct)
    assert status == [-1] * (len(rows) - 1) + [0]
    spans = split(plain, [n_ct] * len(rows), 0)
    assert all(s == bytes(n_ct) for s in spans[:-1])  # zeros over the prefill, no plaintext byte
    assert spans[-1] == pt
    assert residue(ctx) == 0


COUNTS = (1, C // 16 - 1, C // 16, C // 16 + 1, S // 16 - 1, S // 16, S // 16 + 1, 2 * S // 16 + 1, 3 * S // 16)


def mac_rows(seed):
    rng = np.random.default_rng(seed)
    return [rng.bytes(16 * c) for c in COUNTS]


def run_hook(ctx, name, key, rows, max_len):
    from qrkem import last_error
    from qrkem._debug import bind
    n = len(rows)
    out = torch.full((16 * n,), FILL, dtype=torch.uint8, device="cuda")
    k, d, o = dev(key * n), dev(b"".join(rows)), offsets(rows)
    assert getattr(bind(), name)(ctx, n, ptr(k), ptr(d), ptr(o), max_len, ptr(out), None) == 0, last_error()
    torch.cuda.synchronize()
    return split(out.cpu().numpy().tobytes(), [16] * n, 0)


def bit_h(i: int) -> bytes:
    """H with only bit i set, bit 0 the coefficient of x^0: the top bit of the first byte."""
    return (1 << (127 - i)).to_bytes(16, "big")


GHASH_KEYS = {"zero": bytes(16), "ones": b"\xff" * 16, "random": bytes(range(1, 17)),
              **{f"bit{i}": bit_h(i) for i in (0, 1, 63, 64, 127)}}


@pytest.mark.parametrize("case", sorted(GHASH_KEYS) + ["ones_data"])
def test_ghash_hook_matches_spec_at_the_power_boundaries(ciphers, case):
    """Block counts on both sides of a lane (C / 16), of a segment (S / 16) and of two and three segments:
    where a wrong power of H in the tree or the tail shows."""
    ctx = ciphers["AES-256-GCM"]._context()
    h = GHASH_KEYS.get(case, bytes(range(100, 116)))
    rows = [b"\xff" * len(r) for r in mac_rows(1)] if case == "ones_data" else mac_rows(len(case))
    got = run_hook(ctx, "qrk_dbg_ghash_long_batch", h, rows, max(map(len, rows)))
    assert got == [aead_spec.ghash(h, r) for r in rows]
    assert residue(ctx) == 0


R_MAX = bytes.fromhex("ffffff0ffcffff0ffcffff0ffcffff0f")  # r at the clamped maximum
POLY_KEYS = {"r0": bytes(16) + bytes(range(16)), "r1": b"\x01" + bytes(15) + bytes(range(16)),
             "rmax_ones_data": R_MAX + bytes(range(16)), "s_max": bytes(range(3, 19)) + b"\xff" * 16,
             "rmax_s_max": R_MAX + b"\xff" * 16, "unclamped_ones": b"\xff" * 32}


@pytest.mark.parametrize("case", sorted(POLY_KEYS))
def test_poly1305_hook_matches_spec_at_the_power_boundaries(ciphers, case):
    ctx = ciphers["ChaCha20-Poly1305"]._context()
    key = POLY_KEYS[case]
    rows = [b"\xff" * len(r) for r in mac_rows(2)] if "ones" in case else mac_rows(len(case))
    got = run_hook(ctx, "qrk_dbg_poly1305_long_batch", key, rows, max(map(len, rows)))
    assert got == [aead_spec.poly1305(key, r) for r in rows]
    assert residue(ctx) == 0


@pytest.mark.parametrize("alg", ALGS)
def test_hook_row_above_max_len_is_left_alone(ciphers, alg):
    ctx = ciphers[alg]._context()
    name = "qrk_dbg_ghash_long_batch" if alg == "AES-256-GCM" else "qrk_dbg_poly1305_long_batch"
    key = bytes(range(16 if alg == "AES-256-GCM" else 32))
    rows = [bytes(32), bytes(48)]
    got = run_hook(ctx, name, key, rows, 32)
    spec = aead_spec.ghash if alg == "AES-256-GCM" else aead_spec.poly1305
    assert got == [spec(key, rows[0]), bytes([FILL]) * 16]


@pytest.mark.parametrize("alg", ALGS)
def test_python_routing_returns_the_same_bytes(ciphers, alg):
    """long_min_bytes = 0 (always the long pair) and None (never) give equal bytes under fixed nonces, for a
    list, a matrix and PackedRows with max_len=; the single calls round-trip 3S + 5 bytes and a tampered long
    message raises the reference's ValueError."""
    from qrkem.symmetric import AUTH_ERROR, PackedRows
    c = ciphers[alg]
    keys, nonces, pts, aads, _ = four_rows(alg)
    assert c.long_min_bytes is not None and c.long_min_bytes > 0
    try:
        out = {}
        for mode in (0, None):
            c.long_min_bytes = mode
            sealed = c.encrypt_batch(keys, pts, aads, nonces=nonces)
            plain, status = c.decrypt_batch(keys, sealed, aads)
            assert plain == pts and not status.any()
            matrix = torch.from_numpy(np.frombuffer(pts[2] * 2, dtype=np.uint8).copy()).cuda().reshape(2, S - 1)
            m_sealed = c.encrypt_batch(keys[:2], matrix, aads[:2], nonces=nonces[:2])
            packed = PackedRows.from_list(pts, 0)
            p_sealed = c.encrypt_batch(keys, packed, aads, nonces=nonces, max_len=max(map(len, pts)))
            p_plain, p_status = c.decrypt_batch(keys, p_sealed, aads, max_len=max(map(len, pts)))
            assert p_plain.to_list() == pts and not p_status.cpu().numpy().any()
            out[mode] = (sealed, m_sealed.cpu().numpy().tobytes(), p_sealed.to_list())
        assert out[0] == out[None]
        assert out[0][0] == out[0][2] == [aead_spec.seal(alg, k, n, p, a) if len(p) < 64 else s
                                          for k, n, p, a, s in zip(keys, nonces, pts, aads, out[0][0])]
        c.long_min_bytes = 0
        key, msg = c.generate_key(), np.random.default_rng(5).bytes(3 * S + 5)
        sealed = c.encrypt(key, msg, b"message-id")
        assert len(sealed) == len(msg) + 28 and c.decrypt(key, sealed, b"message-id") == msg
        c.long_min_bytes = None
        assert c.decrypt(key, sealed, b"message-id") == msg
        c.long_min_bytes = 0
        for bad in (flip(sealed, 12 + S, 2), flip(sealed, len(sealed) - 1, 7)):
            with pytest.raises(ValueError, match=AUTH_ERROR):
                c.decrypt(key, bad, b"message-id")
        with pytest.raises(ValueError, match=AUTH_ERROR):
            c.decrypt(key, sealed, b"message-ie")
    finally:
        del c.long_min_bytes  # back to the class's measured default
