"""GPU: batched ML-DSA.Verify (qrk_sig_verify_batch, csrc/mldsa.hip) against tests/golden/mldsa.json and
tests/mldsa_spec.py: status per row, and through the test hook qrk_dbg_mldsa_verify_trace the bytes of
mu, c~' and w1 and the flag word, so that parity is byte-level and not one boolean per row."""
import ctypes as ct
import hashlib

import numpy as np
import pytest

import make_golden_mldsa as gold
import mldsa_spec as spec

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SETS = sorted(spec.PARAMS)
LEVEL = {"ML-DSA-44": 2, "ML-DSA-65": 3, "ML-DSA-87": 5}


@pytest.fixture(scope="module")
def fixture():
    return gold.load()


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


def run(lib, ctx, name, rows, context=b"", trace=True, shared=None):
    """rows: (pk, msg, sig) triples -> dict of numpy outputs.  Buffers have exactly the stated sizes.
    shared = (buffer, offsets) replaces the rows' messages with one buffer and its len(rows) + 1 offsets."""
    import qrkem
    p = spec.PARAMS[name]
    n = len(rows)
    pk = _dev(np.frombuffer(b"".join(r[0] for r in rows), np.uint8).reshape(n, p.pk))
    sig = _dev(np.frombuffer(b"".join(r[2] for r in rows), np.uint8).reshape(n, p.sig))
    data = b"".join(r[1] for r in rows) if shared is None else shared[0]
    msg = _dev(np.frombuffer(data, np.uint8)) if data else torch.zeros(0, dtype=torch.uint8, device="cuda")
    offsets = np.cumsum([0] + [len(r[1]) for r in rows]) if shared is None else np.array(shared[1])
    assert len(offsets) == n + 1
    off = _dev(offsets.astype(np.uint64).view(np.int64))
    cs = _dev(np.frombuffer(context, np.uint8)) if context else None
    status = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    stream = ct.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = [ctx, name.encode(), n, pk.data_ptr(), msg.data_ptr() if data else pk.data_ptr(), off.data_ptr(),
            sig.data_ptr(), cs.data_ptr() if cs is not None else None, len(context), status.data_ptr()]
    out = {}
    if trace:
        mu = torch.full((n, 64), 0xA5, dtype=torch.uint8, device="cuda")
        ctl = torch.full((n, 64), 0xA5, dtype=torch.uint8, device="cuda")
        w1 = torch.full((n, p.w1), 0xA5, dtype=torch.uint8, device="cuda")
        flags = torch.full((n,), 0x55, dtype=torch.int32, device="cuda")
        rc = lib.qrk_dbg_mldsa_verify_trace(*args, mu.data_ptr(), ctl.data_ptr(), w1.data_ptr(), flags.data_ptr(), stream)
        assert rc == 0, qrkem.last_error()
        torch.cuda.synchronize()
        out = {"mu": mu.cpu().numpy(), "ctilde": ctl.cpu().numpy(), "w1": w1.cpu().numpy(),
               "flags": flags.cpu().numpy()}
    else:
        assert lib.qrk_sig_verify_batch(*args, stream) == 0, qrkem.last_error()
        torch.cuda.synchronize()
    out["status"] = status.cpu().numpy()
    return out


def check_trace(p, out, i, want):
    """Row i of the hook's outputs equals a spec trace (dict with mu, ctilde, w1, flags)."""
    assert int(out["flags"][i]) == want["flags"]
    assert out["mu"][i].tobytes() == want["mu"]
    assert out["ctilde"][i].tobytes() == want["ctilde"] + bytes(64 - p.ctilde)
    assert out["w1"][i].tobytes() == want["w1"]
    assert int(out["status"][i]) == (0 if want["flags"] == 0 else -1)


@pytest.mark.parametrize("name", SETS)
def test_fixture_records_verify_with_the_stored_trace(lib, ctx, fixture, name):
    p, f = spec.PARAMS[name], fixture[name]
    out = run(lib, ctx, name, [(f["pk"], m, s) for m, s in zip(f["msgs"], f["sigs"])])
    assert out["status"].tolist() == [0, 0, 0, 0] and out["flags"].tolist() == [0, 0, 0, 0]
    for i, rec in enumerate(f["records"]):
        assert out["mu"][i].tobytes().hex() == rec["mu"]
        assert out["ctilde"][i].tobytes() == bytes.fromhex(rec["ctilde"]) + bytes(64 - p.ctilde)
        assert out["ctilde"][i][:p.ctilde].tobytes() == f["sigs"][i][:p.ctilde]
        assert hashlib.sha3_256(out["w1"][i].tobytes()).hexdigest() == rec["w1_sha3"]
    plain = run(lib, ctx, name, [(f["pk"], m, s) for m, s in zip(f["msgs"], f["sigs"])], trace=False)
    assert plain["status"].tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("name", SETS)
def test_every_tamper_entry_is_rejected_with_the_stored_flag_word(lib, ctx, fixture, name):
    f = fixture[name]
    rows = [gold.apply_tamper(e, f["pk"], f["msgs"], f["sigs"]) for e in f["tampers"]]
    out = run(lib, ctx, name, rows)
    for i, e in enumerate(f["tampers"]):
        assert int(out["status"][i]) == -1, e["label"]
        assert int(out["flags"][i]) == e["flags"], e["label"]
        if e["flags"] & spec.FLAG_HINT:  # w1 is undefined without the hint: the trace outputs are zero
            assert not out["mu"][i].any() and not out["ctilde"][i].any() and not out["w1"][i].any(), e["label"]
    assert run(lib, ctx, name, rows, trace=False)["status"].tolist() == [-1] * len(rows)


MIX_LENGTHS = (0, 69, 70, 71, 205, 206, 207, 2500)


@pytest.fixture(scope="module")
def mixed(fixture):
    """Per set: 257 rows cycling fresh signatures over the mixed lengths (one key; signed once) and
    tampered copies in a fixed pattern, with what each row must return."""
    out = {}
    for name in SETS:
        f = fixture[name]
        _, sk = spec.keygen_internal(f["xi"], name)
        msgs = [gold.message(name + "-mix", n) for n in MIX_LENGTHS]
        sigs = [spec.sign(sk, m) for m in msgs]
        p = spec.PARAMS[name]
        rows, valid = [], []
        for i in range(257):
            j = i % len(msgs)
            pk, msg, sig = f["pk"], msgs[j], sigs[j]
            kind = (i * 7 + i // 8) % 5  # 0, 1: untouched; 2: message bit; 3: c~ bit; 4: hint count above omega
            if kind == 2:
                msg = msg + b"!" if not msg else bytes([msg[0] ^ 1]) + msg[1:]
            elif kind == 3:
                sig = bytes([sig[0] ^ 0x80]) + sig[1:]
            elif kind == 4:
                sig = sig[:-1] + bytes([p.omega + 1])
            rows.append((pk, msg, sig))
            valid.append(kind < 2)
        out[name] = (rows, valid)
    return out


@pytest.mark.parametrize("name", SETS)
def test_batches_of_mixed_rows(lib, ctx, mixed, name):
    p = spec.PARAMS[name]
    rows, valid = mixed[name]
    traced = {}
    for n in (1, 2, 63, 64, 65, 257):
        out = run(lib, ctx, name, rows[:n])
        assert out["status"].tolist() == [0 if v else -1 for v in valid[:n]], n  # none left at the prefill 7
        traced[n] = out
    out = traced[257]
    for i in list(range(10)) + [63, 64, 65, 128, 255, 256]:  # 16 rows against the spec's trace
        check_trace(p, out, i, spec.verify_trace(*rows[i]))
    for n in (1, 2, 63, 64, 65):  # a row's outputs do not depend on the batch around it
        for key in ("mu", "ctilde", "w1", "flags"):
            assert np.array_equal(traced[n][key], out[key][:n]), (n, key)


@pytest.mark.parametrize("name", SETS)
def test_chunked_batch_gives_identical_status(lib, mixed, name):
    rows, valid = mixed[name]
    h = ct.c_void_p()
    assert lib.qrk_ctx_create(ct.byref(h), 0) == 0
    try:
        whole = run(lib, h, name, rows)
        assert lib.qrk_ctx_set_chunk(h, 64) == 0  # 257 rows: four chunks of 64 and a one-row tail
        parts = run(lib, h, name, rows)
        plain = run(lib, h, name, rows, trace=False)
    finally:
        lib.qrk_ctx_destroy(h)
    assert parts["status"].tolist() == whole["status"].tolist() == plain["status"].tolist()
    assert whole["status"].tolist() == [0 if v else -1 for v in valid]
    for key in ("mu", "ctilde", "w1", "flags"):
        assert np.array_equal(parts[key], whole[key]), key


def test_context_string(lib, ctx, fixture):
    name = "ML-DSA-44"
    p, f = spec.PARAMS[name], fixture[name]
    _, sk = spec.keygen_internal(f["xi"], name)
    context = b"qrkem handshake v1"
    msg = gold.message(name + "-ctx", 100)
    sig = spec.sign(sk, msg, ctx=context)
    assert spec.verify(f["pk"], msg, sig, ctx=context) and not spec.verify(f["pk"], msg, sig)
    rows = [(f["pk"], msg, sig), (f["pk"], f["msgs"][1], f["sigs"][1])]
    with_ctx = run(lib, ctx, name, rows, context=context)
    assert with_ctx["status"].tolist() == [0, -1]
    check_trace(p, with_ctx, 0, spec.verify_trace(f["pk"], msg, sig, ctx=context))
    check_trace(p, with_ctx, 1, spec.verify_trace(f["pk"], f["msgs"][1], f["sigs"][1], ctx=context))
    without = run(lib, ctx, name, rows)
    assert without["status"].tolist() == [-1, 0]
    longest = bytes(range(255))
    sig255 = spec.sign(sk, msg, ctx=longest)
    assert run(lib, ctx, name, [(f["pk"], msg, sig255)], context=longest)["status"].tolist() == [0]


@pytest.mark.parametrize("name", SETS)
def test_class_agrees_with_the_abi(lib, ctx, fixture, mixed, name):
    import qrkem
    f = fixture[name]
    s = qrkem.MLDSASignature(LEVEL[name])
    assert s.verify(f["pk"], f["msgs"][3], f["sigs"][3]) is True
    assert s.verify(f["pk"], f["msgs"][3] + b"x", f["sigs"][3]) is False
    assert s.verify(f["pk"], f["msgs"][0], f["sigs"][1]) is False
    rows, valid = mixed[name]
    rows, valid = rows[:65], valid[:65]
    got = s.verify_batch([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows])
    assert got.dtype == np.bool_ and got.tolist() == valid
    assert got.tolist() == (run(lib, ctx, name, rows, trace=False)["status"] == 0).tolist()
    # already-resident tensors plus offsets
    p = spec.PARAMS[name]
    pk = _dev(np.frombuffer(b"".join(r[0] for r in rows), np.uint8).reshape(len(rows), p.pk))
    sig = _dev(np.frombuffer(b"".join(r[2] for r in rows), np.uint8).reshape(len(rows), p.sig))
    msg = _dev(np.frombuffer(b"".join(r[1] for r in rows), np.uint8))
    off = _dev(np.cumsum([0] + [len(r[1]) for r in rows]).astype(np.int64))
    assert s.verify_batch(pk, msg, sig, offsets=off).tolist() == valid
    st = s.verify_status(pk, msg, sig, offsets=off)
    assert st.is_cuda and st.dtype == torch.int32 and st.cpu().tolist() == [0 if v else -1 for v in valid]
    s.close()


@pytest.mark.parametrize("name", SETS)
def test_row_with_decreasing_offsets(lib, ctx, fixture, name):
    """Three rows over one 20-byte buffer with offsets [0, 10, 5, 20]: the middle row is refused with FLAG_LONG
    and an all-zero trace, the outer rows are verified exactly as they are alone."""
    p, f = spec.PARAMS[name], fixture[name]
    _, sk = spec.keygen_internal(f["xi"], name)
    data = gold.message(name + "-offsets", 20)
    parts = [data[:10], data[5:20]]
    sigs = [spec.sign(sk, m) for m in parts]
    alone = run(lib, ctx, name, [(f["pk"], m, s) for m, s in zip(parts, sigs)])
    assert alone["status"].tolist() == [0, 0]
    for i, (m, s) in enumerate(zip(parts, sigs)):
        check_trace(p, alone, i, spec.verify_trace(f["pk"], m, s))
    rows = [(f["pk"], parts[0], sigs[0]), (f["pk"], b"", sigs[0]), (f["pk"], parts[1], sigs[1])]
    out = run(lib, ctx, name, rows, shared=(data, [0, 10, 5, 20]))
    assert out["status"].tolist() == [0, -1, 0]
    assert int(out["flags"][1]) == 8  # FLAG_LONG (csrc/mldsa_arith.cuh)
    for key in ("mu", "ctilde", "w1"):
        assert not out[key][1].any(), key
        assert np.array_equal(out[key][[0, 2]], alone[key]), key
    assert out["flags"][[0, 2]].tolist() == [0, 0]
    assert run(lib, ctx, name, rows, shared=(data, [0, 10, 5, 20]), trace=False)["status"].tolist() == [0, -1, 0]
