"""GPU: batched ML-DSA key generation and signing (qrk_mldsa_keypair_batch, qrk_mldsa_sign_batch,
csrc/mldsa_sign.hip) against tests/mldsa_spec.py and tests/golden/mldsa_sign.json.  Keys are compared byte for
byte with the spec's; deterministic signatures through the stored SHA3-256 for the fixture rows (crafted keys
included) and byte for byte with the spec's loop for the others, with mu and the iteration count from the trace
hook qrk_dbg_mldsa_sign_trace.  A row of 2^31 bytes or more cannot be exercised in seconds; that flag is reached
through a row whose offsets decrease."""
import ctypes as ct
import hashlib

import numpy as np
import pytest

import make_golden_mldsa_sign as gold
import mldsa_spec as spec

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

NAMES = list(gold.NAMES)
LEVEL = {"ML-DSA-44": 2, "ML-DSA-65": 3, "ML-DSA-87": 5}
MAX_ITERS = 814


@pytest.fixture(scope="module")
def sets():
    return gold.load()


@pytest.fixture(scope="module")
def keys(sets):
    return {name: gold.Key(name, sets[name]["sk"]) for name in NAMES}


@pytest.fixture(scope="module")
def lib():
    from qrkem._debug import bind
    return bind()


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
    msg = _dev(np.frombuffer(b"".join(msgs) or b"\0", np.uint8))
    if offsets is None:
        offsets = np.cumsum([0] + [len(m) for m in msgs])
    return msg, _dev(np.asarray(offsets, dtype=np.uint64).view(np.int64))


def keygen(lib, ctx, name, xis):
    import qrkem
    p = spec.PARAMS[name]
    n = len(xis)
    xi = _rows(xis, 32)
    pk = torch.full((n, p.pk), 0xA5, dtype=torch.uint8, device="cuda")
    sk = torch.full((n, p.sk), 0xA5, dtype=torch.uint8, device="cuda")
    rc = lib.qrk_mldsa_keypair_batch(ctx, name.encode(), n, xi.data_ptr(), pk.data_ptr(), sk.data_ptr(), _stream())
    assert rc == 0, qrkem.last_error()
    torch.cuda.synchronize()
    return [r.tobytes() for r in pk.cpu().numpy()], [r.tobytes() for r in sk.cpu().numpy()]


def sign(lib, ctx, name, sks, msgs, rnd=None, context=b"", offsets=None, max_iters=None):
    """-> (signatures, status) and, with max_iters (the trace hook), also (mu, iters).  Buffers have exactly the
    stated sizes and are pre-filled, so a row the library does not write shows."""
    import qrkem
    p = spec.PARAMS[name]
    n = len(sks)
    sk = _rows(sks, p.sk)
    msg, off = _messages(msgs, offsets)
    rn = _rows(rnd, 32) if rnd is not None else None
    cs = _dev(np.frombuffer(context, np.uint8)) if context else None
    sig = torch.full((n, p.sig), 0xA5, dtype=torch.uint8, device="cuda")
    status = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    head = (ctx, name.encode(), n, sk.data_ptr(), msg.data_ptr(), off.data_ptr(),
            rn.data_ptr() if rn is not None else None, cs.data_ptr() if cs is not None else None, len(context),
            sig.data_ptr(), status.data_ptr())
    if max_iters is None:
        rc = lib.qrk_mldsa_sign_batch(*head, _stream())
    else:
        mu = torch.full((n, 64), 0xA5, dtype=torch.uint8, device="cuda")
        iters = torch.full((n,), 0x5A5A, dtype=torch.int32, device="cuda")
        rc = lib.qrk_dbg_mldsa_sign_trace(*head, max_iters, mu.data_ptr(), iters.data_ptr(), _stream())
    assert rc == 0, qrkem.last_error()
    torch.cuda.synchronize()
    out = [r.tobytes() for r in sig.cpu().numpy()], status.cpu().tolist()
    if max_iters is not None:
        out += ([r.tobytes() for r in mu.cpu().numpy()], iters.cpu().tolist())
    return out


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


def mu_of(row_sk, msg, context=b""):
    return spec.H(row_sk[64:128] + spec.format_message(msg, context), 64)


# ------------------------------------------------------------------ KeyGen
@pytest.mark.parametrize("name", NAMES)
def test_keygen_matches_the_spec(lib, ctx, sets, name):
    xis = [sets[name]["xi"]] + [spec.H(b"kg" + name.encode() + bytes([i]), 32) for i in range(64)]
    want = [spec.keygen_internal(x, name) for x in xis]
    for n in (1, 3, 65):  # 65: a second block of 64 lanes in the lane-per-row kernels
        pk, sk = keygen(lib, ctx, name, xis[:n])
        for i in range(n):
            assert pk[i] == want[i][0], (n, i)
            assert sk[i] == want[i][1], (n, i)
    assert want[0] == (sets[name]["pk"], sets[name]["sk"])


# ------------------------------------------------------------------ deterministic Sign
@pytest.mark.parametrize("name", NAMES)
def test_fixture_rows_byte_exact_with_iters_and_mu(lib, ctx, sets, name):
    for ctx_len in (0, 255):
        rows = [r for r in sets[name]["rows"] if r["ctx_len"] == ctx_len]
        context = gold.CTX255[:ctx_len]
        sigs, status, mu, iters = sign(lib, ctx, name, [r["sk"] for r in rows], [r["msg"] for r in rows],
                                       context=context, max_iters=MAX_ITERS)
        assert status == [0] * len(rows)
        for r, s, m, it in zip(rows, sigs, mu, iters):
            assert it == r["iters"], (r["kind"], r["counter"], it, r["iters"])
            assert m == mu_of(r["sk"], r["msg"], context), r["counter"]
            assert hashlib.sha3_256(s).hexdigest() == r["sig_sha3"], (r["kind"], r["counter"])
        # the public call gives the same bytes
        again, status = sign(lib, ctx, name, [r["sk"] for r in rows], [r["msg"] for r in rows], context=context)
        assert again == sigs and status == [0] * len(rows)
        honest = [(r, s) for r, s in zip(rows, sigs) if r["kind"] == "honest"]
        pk = sets[name]["pk"]
        assert verify(lib, ctx, name, [pk] * len(honest), [r["msg"] for r, _ in honest], [s for _, s in honest],
                      context) == [0] * len(honest)


@pytest.mark.parametrize("name,n", [("ML-DSA-44", 65), ("ML-DSA-65", 8), ("ML-DSA-87", 8)])
def test_batch_in_chunks(lib, sets, keys, name, n):
    """Fixture rows without a context (crafted keys among them) and fresh messages up to n rows; for ML-DSA-44 a
    context chunk of 64 rows, so the call is two launches."""
    rows = [r for r in sets[name]["rows"] if r["ctx_len"] == 0][:n]
    sks = [r["sk"] for r in rows] + [sets[name]["sk"]] * (n - len(rows))
    msgs = [r["msg"] for r in rows] + [gold.message(name, 5000 + i) for i in range(n - len(rows))]
    want = [(r["sig_sha3"], r["iters"]) for r in rows]
    for m in msgs[len(rows):]:
        s, it, _ = gold.trace(keys[name], m)
        want.append((hashlib.sha3_256(s).hexdigest(), it))
    h = ct.c_void_p()
    assert lib.qrk_ctx_create(ct.byref(h), 0) == 0
    try:
        if n > 64:
            assert lib.qrk_ctx_set_chunk(h, 64) == 0
        sigs, status, mu, iters = sign(lib, h, name, sks, msgs, max_iters=MAX_ITERS)
    finally:
        lib.qrk_ctx_destroy(h)
    assert status == [0] * n
    assert iters == [w[1] for w in want]
    assert [hashlib.sha3_256(s).hexdigest() for s in sigs] == [w[0] for w in want]
    assert mu == [mu_of(k, m) for k, m in zip(sks, msgs)]


# ------------------------------------------------------------------ the four rejection thresholds
@pytest.mark.parametrize("name", NAMES)
def test_threshold_pairs(lib, ctx, sets, name):
    """The fixture's threshold pairs in one batch: a row whose first iteration has ||z||, ||LowBits(w - c s2)||,
    ||c t0|| or the hint count exactly on the rejecting value is rejected there, its twin one unit inside signs in
    that iteration, and both give the spec's bytes (test_mldsa_sign_golden.py recomputes the exact values).  The
    edge_h twin has omega hints: sigEncode writes the last byte of the index area."""
    p = spec.PARAMS[name]
    pairs = gold.stored_pairs(sets[name]["rows"])
    assert [at["kind"] for at, _ in pairs] == ["edge_z"] * 2 + ["edge_r"] * 2 + \
        ["edge_t"] * (2 if name == "ML-DSA-44" else 0) + ["edge_h"]
    rows = [r for pair in pairs for r in pair]
    sigs, status, mu, iters = sign(lib, ctx, name, [r["sk"] for r in rows], [r["msg"] for r in rows],
                                   max_iters=MAX_ITERS)
    assert status == [0] * len(rows)
    for r, s, it in zip(rows, sigs, iters):
        what = (r["kind"], r.get("value", r.get("m")), it)
        if r["twin"]:
            assert it == 1, what
        else:
            assert it == r["iters"] >= 2, what
        assert hashlib.sha3_256(s).hexdigest() == r["sig_sha3"], what
    assert mu == [mu_of(r["sk"], r["msg"]) for r in rows]
    assert rows[-1]["kind"] == "edge_h" and rows[-1]["twin"] and sigs[-1][-1] == p.omega


# ------------------------------------------------------------------ hedged Sign
@pytest.mark.parametrize("name", NAMES)
def test_hedged_sign(lib, ctx, sets, name):
    import qrkem
    pk, sk = sets[name]["pk"], sets[name]["sk"]
    msgs = [b"", b"hedged", gold.message(name, 7000)]
    rnd = [spec.H(b"rnd" + bytes([i]), 32) for i in range(3)]
    for context in (b"", b"ctx"):
        sigs, status = sign(lib, ctx, name, [sk] * 3, msgs, rnd=rnd, context=context)
        assert status == [0, 0, 0]
        for m, r, s in zip(msgs, rnd, sigs):
            assert s == spec.sign(sk, m, context, rnd=r)
            assert spec.verify(pk, m, s, context)
        assert verify(lib, ctx, name, [pk] * 3, msgs, sigs, context) == [0, 0, 0]
    signer = qrkem.MLDSASigner(LEVEL[name])
    a, b = (signer.sign_batch([sk], [b"same message"])[0].cpu().numpy().tobytes() for _ in range(2))
    assert a != b
    assert verify(lib, ctx, name, [pk, pk], [b"same message"] * 2, [a, b]) == [0, 0]
    assert spec.verify(pk, b"same message", a) and spec.verify(pk, b"same message", b)
    det = qrkem.MLDSASigner(LEVEL[name], deterministic=True)
    assert det.sign(sk, b"same message") == det.sign(sk, b"same message") == spec.sign(sk, b"same message")


# ------------------------------------------------------------------ the loop's cap
@pytest.mark.parametrize("name", NAMES)
def test_loop_cap(lib, ctx, sets, name):
    """Rows with different iteration counts k in one batch: max_iters = k - 1 exhausts exactly the rows with
    k iterations or more, which get status -1 and zeros; every other row keeps its signature."""
    rows = [r for r in sets[name]["rows"] if r["ctx_len"] == 0]
    ks = sorted({r["iters"] for r in rows})
    assert len(ks) >= 3
    zero = bytes(spec.PARAMS[name].sig)
    for k in (ks[1], ks[-1]):
        for cap in (k - 1, k):
            sigs, status, _, iters = sign(lib, ctx, name, [r["sk"] for r in rows], [r["msg"] for r in rows],
                                          max_iters=cap)
            for r, s, st, it in zip(rows, sigs, status, iters):
                if r["iters"] <= cap:
                    assert st == 0 and it == r["iters"] and hashlib.sha3_256(s).hexdigest() == r["sig_sha3"]
                else:
                    assert st == -1 and s == zero and it == cap, (r["counter"], cap)
    # a cap of zero runs nothing
    sigs, status, _, iters = sign(lib, ctx, name, [rows[0]["sk"]], [rows[0]["msg"]], max_iters=0)
    assert (sigs, status, iters) == ([zero], [-1], [0])


# ------------------------------------------------------------------ refused rows
@pytest.mark.parametrize("name", NAMES)
def test_refused_rows(lib, ctx, sets, name):
    import qrkem
    p = spec.PARAMS[name]
    sk, pk = sets[name]["sk"], sets[name]["pk"]
    zero = bytes(p.sig)
    msgs = [b"first", b"second!", b"third"]
    good = [spec.sign(sk, m) for m in msgs]
    # offsets that decrease at row 1; rows 0 and 2 are ordinary rows of 5 bytes
    sigs, status, mu, iters = sign(lib, ctx, name, [sk] * 3, [b"firstthird"], offsets=[0, 5, 4, 9],
                                   max_iters=MAX_ITERS)
    assert status == [0, -1, 0] and sigs[1] == zero and iters[1] == 0 and mu[1] == bytes(64)
    assert sigs[0] == good[0] and sigs[2] == spec.sign(sk, b"tthir")  # bytes 4 .. 9 of the buffer
    # a secret key with an s1 / s2 field outside [-eta, eta]: the first field of s1, the last field of s2
    ebits = (2 * p.eta).bit_length()
    s2_end = 128 + 32 * ebits * (p.l + p.k)
    first = bytearray(sk)
    first[128] |= (1 << ebits) - 1
    last = bytearray(sk)
    last[s2_end - 1] |= 0xFF & ~((1 << (8 - ebits)) - 1)
    for bad in (bytes(first), bytes(last)):
        s1, s2 = spec.sk_decode(p, bad)[3:5]
        assert max(int(np.max(np.abs(v))) for v in s1 + s2) > p.eta
        sigs, status = sign(lib, ctx, name, [sk, bad, sk], msgs)
        assert status == [0, -1, 0] and sigs[1] == zero
        assert sigs[0] == good[0] and sigs[2] == good[2]
    signer = qrkem.MLDSASigner(LEVEL[name], deterministic=True)
    with pytest.raises(RuntimeError, match="1 of 3 rows were refused"):
        signer.sign_batch([sk, bytes(first), sk], msgs)
    sigs, status = signer.sign_batch([sk, bytes(first), sk], msgs, return_status=True)
    assert status.cpu().tolist() == [0, -1, 0]
    assert [r.tobytes() for r in sigs.cpu().numpy()] == [good[0], zero, good[2]]
    with pytest.raises(ValueError, match="secret keys"):
        signer.sign(sk[:-1], b"m")


# ------------------------------------------------------------------ the reference's call sequence
@pytest.mark.parametrize("level", [2, 3, 5])
def test_round_trip_as_the_reference_calls_it(level):
    import qrkem
    signer = qrkem.MLDSASigner(security_level=level)
    pk, sk = signer.generate_keypair()
    assert (len(pk), len(sk)) == (signer.public_key_size, signer.secret_key_size)
    sig = signer.sign(sk, b"key exchange message")
    assert len(sig) == signer.signature_size
    verifier = qrkem.MLDSASignature(security_level=level)
    assert verifier.verify(pk, b"key exchange message", sig) is True
    assert verifier.verify(pk, b"another message", sig) is False
    assert spec.verify(pk, b"key exchange message", sig)
    pks, sks = signer.generate_keypair_batch(3)
    assert pks.shape == (3, signer.public_key_size) and sks.shape == (3, signer.secret_key_size)
    assert len({r.tobytes() for r in pks.cpu().numpy()}) == 3
