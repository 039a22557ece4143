"""GPU: the batched AEAD kernels (aead.hip) through the C ABI and the reference-shaped classes.
Bar: byte-exact against tests/golden/aead.json (sealed by OpenSSL) and against tests/aead_spec.py
(pinned to the same fixture by tests/test_aead_spec.py); every tampered row refused, none excused."""
import ctypes as ct
import json

import numpy as np
import pytest

import aead_spec
from make_golden_aead import AAD_LENS, PT_LENS

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

ALGS = aead_spec.ALGS


@pytest.fixture(scope="module")
def golden(golden_dir):
    doc = json.loads((golden_dir / "aead.json").read_text())
    return {alg: [{k: bytes.fromhex(v) for k, v in r.items()} for r in doc["records"][alg]] for alg in ALGS}


@pytest.fixture(scope="module")
def ciphers():
    from qrkem.symmetric import BY_NAME
    return {alg: BY_NAME[alg](device=0) for alg in ALGS}


def flip(b: bytes, bit: int) -> bytes:
    a = bytearray(b)
    a[bit // 8] ^= 1 << (bit % 8)
    return bytes(a)


@pytest.mark.parametrize("alg", ALGS)
def test_golden_records_seal_and_open_byte_exact(ciphers, golden, alg):
    recs, c = golden[alg], ciphers[alg]
    keys, aads = [r["key"] for r in recs], [r["aad"] for r in recs]
    sealed = c.encrypt_batch(keys, [r["pt"] for r in recs], aads, nonces=[r["nonce"] for r in recs])
    assert sealed == [r["sealed"] for r in recs]
    plain, status = c.decrypt_batch(keys, [r["sealed"] for r in recs], aads)
    assert plain == [r["pt"] for r in recs] and not status.any()


def ragged_inputs(n: int, seed: int):
    rng = np.random.default_rng(seed)
    keys = [rng.bytes(32) for _ in range(n)]
    nonces = [rng.bytes(12) for _ in range(n)]
    pts = [rng.bytes(PT_LENS[(7 * i + 3) % len(PT_LENS)]) for i in range(n)]
    aads = [rng.bytes(AAD_LENS[(3 * i + 1) % len(AAD_LENS)]) for i in range(n)]
    return keys, nonces, pts, aads


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1100])
@pytest.mark.parametrize("aad_mode", ["none", "shared", "per_row"])
@pytest.mark.parametrize("alg", ALGS)
def test_ragged_batches_match_spec(ciphers, alg, aad_mode, n):
    """Every plaintext and AAD length of the fixture's sets mixed in one batch; batch sizes around the
    wave (64) and the workgroup (256), and several workgroups."""
    c = ciphers[alg]
    keys, nonces, pts, aads = ragged_inputs(n, 1000 * n + len(alg))
    aad = {"none": None, "shared": aads[n // 2] or b"shared", "per_row": aads}[aad_mode]
    row_aad = aads if aad_mode == "per_row" else [aad] * n
    want = [aead_spec.seal(alg, keys[i], nonces[i], pts[i], row_aad[i]) for i in range(n)]
    assert c.encrypt_batch(keys, pts, aad, nonces=nonces) == want
    plain, status = c.decrypt_batch(keys, want, aad)
    assert plain == pts and not status.any()
    # OS-drawn nonces: all distinct, and every row opens
    sealed = c.encrypt_batch(keys, pts, aad)
    assert [len(s) for s in sealed] == [len(p) + 28 for p in pts]
    assert len({s[:12] for s in sealed}) == n
    plain, status = c.decrypt_batch(keys, sealed, aad)
    assert plain == pts and not status.any()


@pytest.mark.parametrize("alg", ALGS)
def test_half_tampered_open_refuses_exactly_the_tampered_rows(ciphers, alg):
    """Odd rows are tampered, cycling through one bit in the ciphertext, the tag, the nonce and the
    aad, and a row truncated to 27 bytes.  Those rows get status -1 and an all-zero plaintext span;
    every even row opens exactly."""
    n, c = 130, ciphers[alg]
    rng = np.random.default_rng(77 + len(alg))
    keys = [rng.bytes(32) for _ in range(n)]
    pts = [rng.bytes(PT_LENS[1 + (5 * i) % (len(PT_LENS) - 1)]) for i in range(n)]  # non-empty: a ct bit to flip
    aads = [rng.bytes(AAD_LENS[1 + (3 * i) % (len(AAD_LENS) - 1)]) for i in range(n)]
    sealed = [aead_spec.seal(alg, keys[i], rng.bytes(12), pts[i], aads[i]) for i in range(n)]
    rows, row_aads, modes = list(sealed), list(aads), {}
    for j, i in enumerate(range(1, n, 2)):
        mode = modes[i] = ("ct", "tag", "nonce", "aad", "short")[j % 5]
        if mode == "ct":
            rows[i] = flip(rows[i], 96 + (11 * j) % (8 * len(pts[i])))
        elif mode == "tag":
            rows[i] = flip(rows[i], 8 * (12 + len(pts[i])) + (13 * j) % 128)
        elif mode == "nonce":
            rows[i] = flip(rows[i], (7 * j) % 96)
        elif mode == "aad":
            row_aads[i] = flip(aads[i], (5 * j) % (8 * len(aads[i])))
        else:
            rows[i] = rows[i][:27]
    assert set(modes.values()) == {"ct", "tag", "nonce", "aad", "short"}
    plain, status = c.decrypt_batch(keys, rows, row_aads)
    for i in range(n):
        if i % 2 == 0:
            assert status[i] == 0 and plain[i] == pts[i], i
        else:
            span = 0 if modes[i] == "short" else len(pts[i])
            assert status[i] == -1 and plain[i] == bytes(span), (i, modes[i])
            assert aead_spec.open_(alg, keys[i], rows[i], row_aads[i]) is None


@pytest.mark.parametrize("alg", ALGS)
def test_short_row_status_through_the_c_abi(ciphers, alg):
    """qrk_aead_open_batch itself gives a row shorter than 28 bytes status -1 (last row: the rows
    before it keep their places) and still opens the others."""
    from qrkem.symmetric import PackedRows, open_rows
    c = ciphers[alg]
    keys = [bytes([i]) * 32 for i in range(3)]
    pts = [b"first message", b"second", b""]
    rows = [aead_spec.seal(alg, keys[i], bytes([i + 1]) * 12, pts[i]) for i in range(3)]
    rows[2] = rows[2][:27]
    kd = torch.from_numpy(np.frombuffer(b"".join(keys), np.uint8).reshape(3, 32).copy()).cuda()
    out, status = open_rows(c._context(), alg, 0, kd, PackedRows.from_list(rows, 0), None)
    assert status.cpu().tolist() == [0, 0, -1]
    assert out.data.cpu().numpy()[:len(pts[0]) + len(pts[1])].tobytes() == pts[0] + pts[1]


def _packed(rows):
    off = np.zeros(len(rows) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    data = np.frombuffer(b"".join(rows) + b"\0", np.uint8).copy()
    return torch.from_numpy(data).cuda(), torch.from_numpy(off).cuda()


def _hook(name, fixed, rows):
    """Run a qrk_dbg_* hook: `fixed` = n byte strings of equal length, `rows` ragged; 16-byte outputs."""
    from qrkem._debug import bind
    from qrkem._native import last_error
    fn = getattr(bind(), name)
    n = len(rows)
    f = torch.from_numpy(np.frombuffer(b"".join(fixed), np.uint8).copy()).cuda()
    data, off = _packed(rows)
    out = torch.zeros(16 * n, dtype=torch.uint8, device="cuda")
    stream = ct.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    assert fn(n, f.data_ptr(), data.data_ptr(), off.data_ptr(), out.data_ptr(), stream) == 0, last_error()
    res = out.cpu().numpy()
    return [res[16 * i:16 * i + 16].tobytes() for i in range(n)]


def test_poly1305_final_reduction_wrap_and_clamped_maximum():
    """r = 1, s = 2^128 - 1 and three full blocks 2^127, 2^127 - 5 + k, 0: with the 2^128 bit of each
    block the accumulator before the final reduction is exactly p + k, so the tag is (k + s) mod 2^128 --
    a kernel without the full final reduction, or without the wrap of h + s, fails.  Then r with every
    clamped bit set over all-0xFF messages of 1, 2, 17 and 64 blocks, with and without a 1-byte last
    block: the largest limbs and carries the arithmetic can meet."""
    keys, msgs, want = [], [], []
    for k in range(5):
        keys.append((1).to_bytes(16, "little") + b"\xff" * 16)
        msgs.append((1 << 127).to_bytes(16, "little") + ((1 << 127) - 5 + k).to_bytes(16, "little") + bytes(16))
        want.append(((k - 1) % (1 << 128)).to_bytes(16, "little"))
    r_max = aead_spec.R_CLAMP.to_bytes(16, "little")
    for blocks in (1, 2, 17, 64):
        for tail in (0, 1):
            for s in (bytes(16), b"\xff" * 16):
                keys.append(r_max + s)
                msgs.append(b"\xff" * (16 * blocks + tail))
                want.append(aead_spec.poly1305(keys[-1], msgs[-1]))
    keys.append(b"\xff" * 32)  # unclamped r: the kernel clamps
    msgs.append(b"\x01")
    want.append(aead_spec.poly1305(keys[-1], msgs[-1]))
    assert [aead_spec.poly1305(k, m) for k, m in zip(keys[:5], msgs[:5])] == want[:5]
    assert _hook("qrk_dbg_poly1305_batch", keys, msgs) == want


def test_ghash_bit_order_and_reduction():
    """H with one bit at each end (the reflected bit order: x^0 is the top bit of byte 0, x^127 the low
    bit of byte 15, whose product with x wraps through the reduction polynomial), all-ones and E_0(0),
    over 1, 2 and 9 blocks, all-ones and random."""
    rng = np.random.default_rng(5)
    e0 = aead_spec.aes256_encrypt_block(aead_spec.aes256_expand_key(bytes(32)), bytes(16))
    hs, data = [], []
    for h in ((1 << 127).to_bytes(16, "big"), (1).to_bytes(16, "big"), b"\xff" * 16, e0):
        for blocks in (1, 2, 9):
            for d in (b"\xff" * (16 * blocks), rng.bytes(16 * blocks)):
                hs.append(h)
                data.append(d)
    assert _hook("qrk_dbg_ghash_batch", hs, data) == [aead_spec.ghash(h, d) for h, d in zip(hs, data)]


@pytest.mark.parametrize("alg", ALGS)
def test_reference_shaped_single_calls(ciphers, golden, alg):
    c = ciphers[alg]
    key = c.generate_key()
    sealed = c.encrypt(key, b"attack at dawn", b"header")
    assert len(sealed) == 14 + 28 and aead_spec.open_(alg, key, sealed, b"header") == b"attack at dawn"
    assert c.decrypt(key, sealed, b"header") == b"attack at dawn"
    assert c.decrypt(key, c.encrypt(key, b""), None) == b""
    assert c.encrypt(key, b"attack at dawn", b"header")[:12] != sealed[:12]  # a fresh nonce per call
    with pytest.raises(ValueError, match="^Authentication failed or decryption error$"):
        c.decrypt(key, flip(sealed, 100), b"header")
    with pytest.raises(ValueError, match="^Authentication failed or decryption error$"):
        c.decrypt(key, sealed, b"other header")
    with pytest.raises(ValueError, match="^Authentication failed or decryption error$"):
        c.decrypt(key, sealed[:20], b"header")  # has a nonce, lacks a tag
    with pytest.raises(ValueError, match="Key must be 32 bytes"):
        c.encrypt(key[:16], b"x")
    with pytest.raises(ValueError, match="Ciphertext too short"):
        c.decrypt(key, sealed[:11])
    r = golden[alg][5]
    assert c.decrypt(r["key"], r["sealed"], r["aad"] or None) == r["pt"]


def test_device_tensor_batches_stay_on_the_device(ciphers):
    c = ciphers["ChaCha20-Poly1305"]
    n = 70
    keys = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda")
    pts = torch.randint(0, 256, (n, 46), dtype=torch.uint8, device="cuda")
    sealed = c.encrypt_batch(keys, pts)
    assert sealed.is_cuda and tuple(sealed.shape) == (n, 74)
    plain, status = c.decrypt_batch(keys, sealed)
    assert plain.is_cuda and torch.equal(plain, pts) and not bool(status.any())
    k, s = keys.cpu().numpy(), sealed.cpu().numpy()
    assert aead_spec.open_("ChaCha20-Poly1305", k[n - 1].tobytes(), s[n - 1].tobytes()) == pts[n - 1].cpu().numpy().tobytes()
    with pytest.raises(ValueError, match="AEAD keys"):
        c.encrypt_batch(keys[:, :31].contiguous(), pts)
    with pytest.raises(ValueError, match="AEAD nonces"):
        c.encrypt_batch(keys, pts, nonces=torch.zeros((n, 16), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="batch size"):
        c.decrypt_batch(keys[:5].contiguous(), sealed)


@pytest.mark.parametrize("sym", ALGS)
def test_handshake_confirm(sym):
    """ML-KEM-768, n = 300, 46-byte messages of the reference's test-message shape
    (messaging.py:1103-1107): the initiator's sealed rows open under the responder's key."""
    from qrkem.handshake import HandshakeDriver
    n = 300
    drv = HandshakeDriver("ML-KEM-768", symmetric_name=sym)
    batch = drv.run([drv.info_for(f"peer-{i}", "server") for i in range(n)])
    msgs = [json.dumps({"test": True, "timestamp": 1700000000.000001 + i}).encode() for i in range(n)]
    assert {len(m) for m in msgs} == {46}
    sealed, ok = drv.confirm(batch, msgs)
    torch.cuda.synchronize()
    assert ok.dtype == torch.int32 and ok.cpu().tolist() == [1] * n
    key_r = batch.key_responder.cpu().numpy()
    assert [aead_spec.open_(sym, key_r[i].tobytes(), sealed[i]) for i in range(n)] == msgs
    assert len({s[:12] for s in sealed}) == n
    batch.key_responder[123] = torch.zeros(32, dtype=torch.uint8, device="cuda")
    _sealed, ok = drv.confirm(batch, msgs)
    assert ok.cpu().tolist() == [0 if i == 123 else 1 for i in range(n)]
