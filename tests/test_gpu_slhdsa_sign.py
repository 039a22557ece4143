"""GPU: batched SLH-DSA-SHA2 / SPHINCS+-SHA2-simple key generation and signing (qrk_sig_keypair_batch,
qrk_sig_sign_batch, csrc/slhdsa_sign.hip) against tests/slhdsa_spec.py, tests/golden/slhdsa.json and
tests/golden/slhdsa_sign.json.  Deterministic signatures are compared byte for byte through their stored
SHA3-256 (and located through the stored part hashes); everything else is checked through R = PRF_msg (cheap
in the spec), through qrk_sig_verify_batch, and for one row per test through the spec's verifier.  The spec
signs nothing here: one signature costs it 0.2 to 0.7 s.  No row of 2^31 bytes or more goes
through the ABI (a wrong comparison would read gibibytes from a short buffer): FLAG_LONG is reached here through a
row whose offsets decrease, and the 2^31 threshold of row_span is pinned on the offsets alone, with no memory
behind them, in tests/test_gpu_slhdsa_prims.py."""
import ctypes as ct
import hashlib

import numpy as np
import pytest

import make_golden_slhdsa as gold
import make_golden_slhdsa_sign as sgold
import slhdsa_spec as spec

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

NAMES = sorted(spec.PARAMS)
FIPS_NAMES = [n for n in NAMES if spec.PARAMS[n].fips]
LEVEL = {16: 1, 24: 3, 32: 5}
# |M'| that puts the HMAC inner stream opt_rand || M' (after the key block) on the padding edges: n + |M'| =
# 55, 56, 63, 64 for SHA-256 (n = 16) and 111, 112, 127, 128 for SHA-512
FRAMED = {16: (39, 40, 47, 48), 24: (87, 88, 103, 104), 32: (79, 80, 95, 96)}


@pytest.fixture(scope="module")
def fixture():
    return gold.load()


@pytest.fixture(scope="module")
def cases():
    return sgold.load()


@pytest.fixture(scope="module")
def lib():
    from qrkem._native import LIB
    return LIB


@pytest.fixture(scope="module")
def ctx(lib):
    h = ct.c_void_p()
    assert lib.qrk_ctx_create(ct.byref(h), 0) == 0
    yield h
    lib.qrk_ctx_destroy(h)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rows(blobs, width):
    return _dev(np.frombuffer(b"".join(blobs), np.uint8).reshape(len(blobs), width))


def _stream():
    return ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def _messages(msgs, offsets=None):
    data = b"".join(msgs)
    msg = _dev(np.frombuffer(data or b"\0", np.uint8))
    if offsets is None:
        offsets = np.cumsum([0] + [len(m) for m in msgs])
    return msg, _dev(np.asarray(offsets, dtype=np.uint64).view(np.int64))


def keygen(lib, ctx, name, seeds):
    """seeds: list of 3 n byte strings -> (pk list, sk list)."""
    import qrkem
    p = spec.PARAMS[name]
    n = len(seeds)
    sd = _rows(seeds, 3 * p.n)
    pk = torch.full((n, p.pk), 0xA5, dtype=torch.uint8, device="cuda")
    sk = torch.full((n, p.sk), 0xA5, dtype=torch.uint8, device="cuda")
    rc = lib.qrk_sig_keypair_batch(ctx, name.encode(), n, sd.data_ptr(), pk.data_ptr(), sk.data_ptr(), _stream())
    assert rc == 0, qrkem.last_error()
    torch.cuda.synchronize()
    return [r.tobytes() for r in pk.cpu().numpy()], [r.tobytes() for r in sk.cpu().numpy()]


def sign(lib, ctx, name, sks, msgs, opt_rand=None, context=b"", offsets=None):
    """-> (signatures as a list of bytes, status list).  Buffers have exactly the stated sizes."""
    import qrkem
    p = spec.PARAMS[name]
    n = len(sks)
    sk = _rows(sks, p.sk)
    msg, off = _messages(msgs, offsets)
    orand = _rows(opt_rand, p.n) if opt_rand is not None else None
    cs = _dev(np.frombuffer(context, np.uint8)) if context else None
    sig = torch.full((n, p.sig), 0xA5, dtype=torch.uint8, device="cuda")
    status = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    rc = lib.qrk_sig_sign_batch(ctx, name.encode(), n, sk.data_ptr(), msg.data_ptr(), off.data_ptr(),
                                orand.data_ptr() if orand is not None else None,
                                cs.data_ptr() if cs is not None else None, len(context), sig.data_ptr(),
                                status.data_ptr(), _stream())
    assert rc == 0, qrkem.last_error()
    torch.cuda.synchronize()
    return [r.tobytes() for r in sig.cpu().numpy()], status.cpu().tolist()


def verify(lib, ctx, name, pks, msgs, sigs, context=b""):
    import qrkem
    p = spec.PARAMS[name]
    n = len(pks)
    pk, sig = _rows(pks, p.pk), _rows(sigs, p.sig)
    msg, off = _messages(msgs)
    cs = _dev(np.frombuffer(context, np.uint8)) if context else None
    status = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    rc = lib.qrk_sig_verify_batch(ctx, name.encode(), n, pk.data_ptr(), msg.data_ptr(), off.data_ptr(), sig.data_ptr(),
                                  cs.data_ptr() if cs is not None else None, len(context), status.data_ptr(),
                                  _stream())
    assert rc == 0, qrkem.last_error()
    torch.cuda.synchronize()
    return status.cpu().tolist()


def spec_r(name, sk, msg, opt_rand=None, context=b""):
    return sgold.digest_of(name, sk, msg, opt_rand, context)[0]


def derived_seeds(name, tag, count):
    n = spec.PARAMS[name].n
    return [hashlib.shake_256(f"qrkem-slhdsa-sign-test-{name}-{tag}-{i}".encode()).digest(3 * n) for i in range(count)]


# ------------------------------------------------------------------ 1. key generation
@pytest.mark.parametrize("name", NAMES)
def test_keygen_matches_the_fixture_and_lays_out_sk(lib, ctx, fixture, name):
    p, f = spec.PARAMS[name], fixture[name]
    n = p.n
    base = b"".join(f["seeds"])
    sk_seed_flip = bytes([base[3] ^ 0x40]).join((base[:3], base[4:]))
    pk_seed_flip = bytes([base[2 * n + 5] ^ 0x01]).join((base[:2 * n + 5], base[2 * n + 6:]))
    seeds = [base, sk_seed_flip, pk_seed_flip]
    pks, sks = keygen(lib, ctx, name, seeds)
    assert pks[0] == f["pk"] and sks[0] == base + f["pk"][n:] == f["sk"]
    for sd, pk, sk in zip(seeds, pks, sks):
        assert pk[:n] == sd[2 * n:] and sk == sd + pk[n:]  # sk = SK.seed || SK.prf || PK.seed || PK.root
        assert (pk, sk) == spec.keygen(name, sd[:n], sd[n:2 * n], sd[2 * n:])
    assert len({pk[n:] for pk in pks}) == 3  # either seed changes the root
    # a single row is the same key
    assert keygen(lib, ctx, name, seeds[1:2]) == (pks[1:2], sks[1:2])


# ------------------------------------------------------------------ 2. deterministic signing, byte-exact
def first_difference(name, sig, parts_sha3) -> str:
    labels = ["R", "FORS"] + [f"XMSS signature of layer {j}" for j in range(spec.PARAMS[name].d)]
    for label, part, want in zip(labels, sgold.parts(name, sig), parts_sha3):
        if hashlib.sha3_256(part).hexdigest() != want:
            return label
    return "none of the parts"


@pytest.mark.parametrize("name", NAMES)
def test_deterministic_signatures_are_byte_exact(lib, ctx, fixture, cases, name):
    f = fixture[name]
    msgs = list(f["msgs"]) + [c["msg"] for c in cases[name]]
    want = [r["sig_sha3"] for r in f["records"]] + [c["sig_sha3"] for c in cases[name]]
    parts = [None] * len(f["records"]) + [c["parts_sha3"] for c in cases[name]]
    sigs, status = sign(lib, ctx, name, [f["sk"]] * len(msgs), msgs)
    assert status == [0] * len(msgs)
    for i, (sig, w) in enumerate(zip(sigs, want)):
        if hashlib.sha3_256(sig).hexdigest() != w:
            where = first_difference(name, sig, parts[i]) if parts[i] else "(no part hashes for slhdsa.json rows)"
            pytest.fail(f"{name} row {i} ({len(msgs[i])} bytes): signature differs from the spec's, first in {where}")
    assert verify(lib, ctx, name, [f["pk"]] * len(msgs), msgs, sigs) == [0] * len(msgs)


# ------------------------------------------------------------------ 3. HMAC padding edges
@pytest.mark.parametrize("name", NAMES)
def test_prf_msg_padding_edges(lib, ctx, fixture, name):
    p, f = spec.PARAMS[name], fixture[name]
    lengths = [x - (2 if p.fips else 0) for x in FRAMED[p.n]] + [0]
    msgs = [gold.message(name + "-edge", n) for n in lengths]
    sigs, status = sign(lib, ctx, name, [f["sk"]] * len(msgs), msgs)
    assert status == [0] * len(msgs)
    for m, s in zip(msgs, sigs):
        assert s[:p.n] == spec_r(name, f["sk"], m), len(m)
    assert verify(lib, ctx, name, [f["pk"]] * len(msgs), msgs, sigs) == [0] * len(msgs)
    assert spec.verify(name, f["pk"], msgs[1], sigs[1])


# ------------------------------------------------------------------ 4. hedged signing
@pytest.mark.parametrize("name", NAMES)
def test_per_row_opt_rand(lib, ctx, fixture, name):
    p, f = spec.PARAMS[name], fixture[name]
    m = gold.message(name + "-hedged", 77)
    rands = [hashlib.shake_256(b"opt_rand" + bytes([i])).digest(p.n) for i in range(3)] + [f["pk"][:p.n]]
    sigs, status = sign(lib, ctx, name, [f["sk"]] * 4, [m] * 4, opt_rand=rands)
    assert status == [0] * 4
    for r, s in zip(rands, sigs):
        assert s[:p.n] == spec_r(name, f["sk"], m, opt_rand=r)
    assert len(set(sigs)) == 4 and len({s[p.n:] for s in sigs}) == 4  # same key and message, different opt_rand
    assert verify(lib, ctx, name, [f["pk"]] * 4, [m] * 4, sigs) == [0] * 4
    # opt_rand = PK.seed is the deterministic variant
    assert sign(lib, ctx, name, [f["sk"]], [m])[0][0] == sigs[3]
    assert spec.verify(name, f["pk"], m, sigs[0])


# ------------------------------------------------------------------ 5. context strings
@pytest.mark.parametrize("name", FIPS_NAMES)
def test_context_strings(lib, ctx, fixture, name):
    p, f = spec.PARAMS[name], fixture[name]
    msgs = [gold.message(name + "-ctx", 100), b""]
    for context in (b"abc", bytes(range(255))):
        sigs, status = sign(lib, ctx, name, [f["sk"]] * 2, msgs, context=context)
        assert status == [0, 0]
        for m, s in zip(msgs, sigs):
            assert s[:p.n] == spec_r(name, f["sk"], m, context=context)
        assert verify(lib, ctx, name, [f["pk"]] * 2, msgs, sigs, context=context) == [0, 0]
        assert verify(lib, ctx, name, [f["pk"]] * 2, msgs, sigs) == [-1, -1]
        assert spec.verify(name, f["pk"], msgs[0], sigs[0], ctx=context)
        assert not spec.verify(name, f["pk"], msgs[0], sigs[0])


# ------------------------------------------------------------------ 6. batch shape and independence
@pytest.mark.parametrize("name", NAMES)
def test_rows_are_independent_of_batch_and_chunk(lib, fixture, name):
    p = spec.PARAMS[name]
    h = ct.c_void_p()
    assert lib.qrk_ctx_create(ct.byref(h), 0) == 0
    try:
        pks, sks = keygen(lib, h, name, derived_seeds(name, "batch", 5))
        msgs = [gold.message(name + "-batch", n) for n in (33, 0, 1, 200, 64)]
        whole, status = sign(lib, h, name, sks, msgs)
        assert status == [0] * 5 and len(set(whole)) == 5
        singles = [sign(lib, h, name, [sk], [m])[0][0] for sk, m in zip(sks, msgs)]
        # 66 rows (the five, cycled, each with its own message) so that a chunk of 64 really splits the batch
        many_sk = [sks[i % 5] for i in range(66)]
        many_msg = [msgs[i % 5] + bytes([i]) * (i // 5) for i in range(66)]
        many, status = sign(lib, h, name, many_sk, many_msg)
        assert status == [0] * 66
        assert lib.qrk_ctx_set_chunk(h, 2) == 0
        chunked, status = sign(lib, h, name, sks, msgs)
        assert status == [0] * 5
        many_chunked, status = sign(lib, h, name, many_sk, many_msg)
        assert status == [0] * 66
        ok = verify(lib, h, name, [pks[i % 5] for i in range(66)], many_msg, many)
    finally:
        lib.qrk_ctx_destroy(h)
    assert whole == singles == chunked
    assert many == many_chunked and many[:5] == whole and ok == [0] * 66
    assert spec.verify(name, pks[1], b"", whole[1])


# ------------------------------------------------------------------ 7. a row whose offsets decrease
@pytest.mark.parametrize("name", NAMES)
def test_row_with_decreasing_offsets(lib, ctx, fixture, name):
    p, f = spec.PARAMS[name], fixture[name]
    data = gold.message(name + "-offsets", 20)
    sigs, status = sign(lib, ctx, name, [f["sk"]] * 3, [data], offsets=[0, 10, 5, 20])
    assert status == [0, -1, 0]
    assert sigs[1] == bytes(p.sig)
    alone, st = sign(lib, ctx, name, [f["sk"]] * 2, [data[:10], data[5:20]])
    assert st == [0, 0] and [sigs[0], sigs[2]] == alone
    assert verify(lib, ctx, name, [f["pk"]] * 2, [data[:10], data[5:20]], alone) == [0, 0]


# ------------------------------------------------------------------ 8. a corrupt secret key
@pytest.mark.parametrize("name", NAMES)
def test_corrupt_secret_key(lib, ctx, fixture, name):
    import qrkem
    p, f = spec.PARAMS[name], fixture[name]
    sk = f["sk"]
    at = 3 * p.n + 7  # inside PK.root
    bad = sk[:at] + bytes([sk[at] ^ 0x04]) + sk[at + 1:]
    msgs = [b"one", b"two", b"three"]
    sigs, status = sign(lib, ctx, name, [sk, bad, sk], msgs)
    assert status == [0, -1, 0] and sigs[1] == bytes(p.sig)
    assert verify(lib, ctx, name, [f["pk"]] * 3, msgs, sigs) == [0, -1, 0]
    s = qrkem.SPHINCSSignature(LEVEL[p.n], fips205=p.fips, signing=True, deterministic=True)
    try:
        with pytest.raises(RuntimeError, match="1 of 3 rows were refused"):
            s.sign_batch([sk, bad, sk], msgs)
        out, st = s.sign_batch([sk, bad, sk], msgs, return_status=True)
        assert st.is_cuda and st.dtype == torch.int32 and st.cpu().tolist() == [0, -1, 0]
        assert [r.tobytes() for r in out.cpu().numpy()] == sigs
        with pytest.raises(RuntimeError):
            s.sign(bad, b"two")
    finally:
        s.close()


# ------------------------------------------------------------------ 9. the class
@pytest.mark.parametrize("name", NAMES)
def test_class(fixture, cases, name):
    import qrkem
    p, f = spec.PARAMS[name], fixture[name]
    c = cases[name][0]
    det = qrkem.SPHINCSSignature(LEVEL[p.n], fips205=p.fips, signing=True, deterministic=True)
    hedged = qrkem.SPHINCSSignature(LEVEL[p.n], fips205=p.fips, signing=True)
    try:
        assert det.variant == hedged.variant == name
        sig = det.sign(f["sk"], c["msg"])
        assert isinstance(sig, bytes) and hashlib.sha3_256(sig).hexdigest() == c["sig_sha3"]
        a, b = hedged.sign(f["sk"], c["msg"]), hedged.sign(f["sk"], c["msg"])
        assert a != b and a[:p.n] != b[:p.n] and len(a) == len(b) == p.sig
        assert hedged.verify(f["pk"], c["msg"], a) and hedged.verify(f["pk"], c["msg"], b)
        t = bytearray(a)
        t[p.sig // 2] ^= 1
        assert hedged.verify(f["pk"], c["msg"], bytes(t)) is False
        with pytest.raises(ValueError):
            hedged.sign(f["sk"][:-1], b"m")
        # a fresh key pair signs and verifies; sign then verify_status on one stream, no host wait between
        pk, sk = hedged.generate_keypair()
        assert len(pk) == p.pk and len(sk) == p.sk and sk[2 * p.n:] == pk
        pks, sks = hedged.generate_keypair_batch(3)
        assert pks.is_cuda and tuple(pks.shape) == (3, p.pk) and tuple(sks.shape) == (3, p.sk)
        assert torch.equal(sks[:, 2 * p.n:], pks) and len({r.tobytes() for r in pks.cpu().numpy()}) == 3
        msgs = [b"", b"handshake response", bytes(300)]
        data, off = _messages(msgs)
        sigs, st = hedged.sign_batch(sks, data, offsets=off, return_status=True)
        ok = hedged.verify_status(pks, data, sigs, offsets=off)
        swapped = hedged.verify_status(pks.flip(0).contiguous(), data, sigs, offsets=off)
        assert sigs.is_cuda and tuple(sigs.shape) == (3, p.sig)
        assert st.cpu().tolist() == [0, 0, 0] and ok.cpu().tolist() == [0, 0, 0]
        assert swapped.cpu().tolist() == [-1, 0, -1]
        assert hedged.verify(pk, b"m", hedged.sign(sk, b"m"))
    finally:
        det.close()
        hedged.close()
