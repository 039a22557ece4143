"""GPU: batched SLH-DSA-SHA2 / SPHINCS+-SHA2-simple verification (qrk_sig_verify_batch, csrc/slhdsa.hip)
against tests/slhdsa_spec.py and tests/golden/slhdsa.json: status per row, and through the test hook
qrk_dbg_slhdsa_verify_trace the H_msg digest, the FORS public key, the root of every hypertree layer and the
flag word, so that parity is byte-level per layer and not one boolean per row.

Inputs are built once per module: one key per name and spec signatures over messages whose lengths sit on the
padding edges of the outer hash (R || PK.seed || PK.root || M' of 55 / 56 / 63 / 64 bytes for SHA-256,
111 / 112 / 127 / 128 for SHA-512), plus 0 and 2500.  No row of 2^31 bytes or more goes through
the ABI (a wrong comparison would read gibibytes from a short buffer): FLAG_LONG is reached here through a row
whose offsets decrease, and the 2^31 threshold of row_span is pinned on the offsets alone, with no memory behind
them, in tests/test_gpu_slhdsa_prims.py."""
import ctypes as ct
import hashlib

import numpy as np
import pytest

import make_golden_slhdsa as gold
import slhdsa_spec as spec
from test_slhdsa_spec import check_divergence, other_flavour, tampers

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

NAMES = sorted(spec.PARAMS)
LEVEL = {16: 1, 24: 3, 32: 5}
# message lengths: the total R || PK.seed || PK.root || M sits on the hash's padding edges; then 0 and 2500
EDGES = {16: (7, 8, 15, 16), 24: (39, 40, 55, 56), 32: (15, 16, 31, 32)}


def lengths(p) -> tuple:
    e = EDGES[p.n]
    # FIPS 205 frames M with two more bytes: two of the edges again, two bytes earlier
    return e + (0, 2500) + ((e[1] - 2, e[3] - 2) if p.fips else ())


@pytest.fixture(scope="module")
def fixture():
    return gold.load()


@pytest.fixture(scope="module")
def signed(fixture):
    """Per name: (pk, [(msg, sig, spec trace)]) over lengths(p), signed once."""
    out = {}
    for name in NAMES:
        p, f = spec.PARAMS[name], fixture[name]
        rows = []
        for n in lengths(p):
            m = gold.message(name + "-gpu", n)
            s = spec.sign(name, f["sk"], m)
            tr = spec.verify_trace(name, f["pk"], m, s)
            assert tr["flags"] == 0
            rows.append((m, s, tr))
        out[name] = (f["pk"], rows)
    return out


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
        digest = torch.full((n, p.m), 0xA5, dtype=torch.uint8, device="cuda")
        fors = torch.full((n, p.n), 0xA5, dtype=torch.uint8, device="cuda")
        roots = torch.full((n, p.d * p.n), 0xA5, dtype=torch.uint8, device="cuda")
        flags = torch.full((n,), 0x55, dtype=torch.int32, device="cuda")
        rc = lib.qrk_dbg_slhdsa_verify_trace(*args, digest.data_ptr(), fors.data_ptr(), roots.data_ptr(),
                                             flags.data_ptr(), stream)
        assert rc == 0, qrkem.last_error()
        torch.cuda.synchronize()
        out = {"digest": digest.cpu().numpy(), "fors_pk": fors.cpu().numpy(), "roots": roots.cpu().numpy(),
               "flags": flags.cpu().numpy()}
    else:
        assert lib.qrk_sig_verify_batch(*args, stream) == 0, qrkem.last_error()
        torch.cuda.synchronize()
    out["status"] = status.cpu().numpy()
    return out


def row_trace(out, i) -> dict:
    return {"digest": out["digest"][i].tobytes(), "fors_pk": out["fors_pk"][i].tobytes(),
            "roots": out["roots"][i].tobytes(), "flags": int(out["flags"][i])}


def check_trace(out, i, want):
    """Row i of the hook's outputs equals a spec trace."""
    got = row_trace(out, i)
    assert got["flags"] == want["flags"]
    assert got["digest"] == want["digest"]
    assert got["fors_pk"] == want["fors_pk"]
    assert got["roots"] == want["roots"]
    assert int(out["status"][i]) == (0 if want["flags"] == 0 else -1)


@pytest.mark.parametrize("name", NAMES)
def test_inputs_reach_both_ends_of_the_chain_loop(signed, name):
    """On the spec's side: over the signed messages every WOTS+ digit 0..15 occurs, so chains run 0 to 15
    steps, and the last chain (a checksum digit; for n = 32 it is in the lanes' second pass) takes more than
    one value."""
    p = spec.PARAMS[name]
    seen, last = set(), set()
    for _, _, tr in signed[name][1]:
        for j in range(p.d):
            m = tr["fors_pk"] if j == 0 else tr["roots"][(j - 1) * p.n:j * p.n]
            d = spec.wots_digits(p, m)
            assert len(d) == p.len
            seen |= set(d[:p.len1])
            last.add(d[-1])
    assert seen == set(range(16)) and len(last) > 1 and max(last) > 0


@pytest.mark.parametrize("name", NAMES)
def test_fixture_records_verify_with_the_stored_trace(lib, ctx, fixture, name):
    f = fixture[name]
    sigs = gold.signatures(name, f)  # checks the stored SHA3-256 of every signature first
    rows = [(f["pk"], m, s) for m, s in zip(f["msgs"], sigs)]
    out = run(lib, ctx, name, rows)
    assert out["status"].tolist() == [0, 0, 0] and out["flags"].tolist() == [0, 0, 0]
    for i, rec in enumerate(f["records"]):
        assert out["digest"][i].tobytes().hex() == rec["digest"]
        assert out["fors_pk"][i].tobytes().hex() == rec["fors_pk"]
        assert hashlib.sha3_256(out["roots"][i].tobytes()).hexdigest() == rec["roots_sha3"]
        check_trace(out, i, spec.verify_trace(name, *rows[i]))
    assert run(lib, ctx, name, rows, trace=False)["status"].tolist() == [0, 0, 0]


@pytest.mark.parametrize("name", NAMES)
def test_signed_edge_lengths_verify(lib, ctx, signed, name):
    pk, rows = signed[name]
    out = run(lib, ctx, name, [(pk, m, s) for m, s, _ in rows])
    assert out["status"].tolist() == [0] * len(rows)
    for i, (_, _, tr) in enumerate(rows):
        check_trace(out, i, tr)


@pytest.mark.parametrize("name", NAMES)
def test_every_tamper_is_rejected_with_the_spec_trace(lib, ctx, signed, name):
    p = spec.PARAMS[name]
    pk, rows = signed[name]
    msg, sig, clean = rows[1]
    cases = tampers(p, pk, msg, sig)
    assert len(cases) == 9
    out = run(lib, ctx, name, [c[1:4] for c in cases])
    for i, (label, tpk, tmsg, tsig, stage) in enumerate(cases):
        assert int(out["status"][i]) == -1 and int(out["flags"][i]) == spec.FLAG_ROOT, label
        check_trace(out, i, spec.verify_trace(name, tpk, tmsg, tsig))
        check_divergence(p, clean, row_trace(out, i), stage, label)  # from the first affected layer, not before
    assert run(lib, ctx, name, [c[1:4] for c in cases], trace=False)["status"].tolist() == [-1] * 9


@pytest.fixture(scope="module")
def mixed(signed):
    """Per name: 257 rows cycling the signed messages with a fixed tamper pattern, and what each row returns."""
    out = {}
    for name in NAMES:
        p = spec.PARAMS[name]
        pk, srows = signed[name]
        ht = p.n * (1 + p.k * (p.a + 1))
        rows, valid = [], []
        for i in range(257):
            msg, sig, _ = srows[i % len(srows)]
            kind = (i * 7 + i // 8) % 5  # 0, 1: untouched; 2: message; 3: a chain of layer i % d; 4: R
            if kind == 2:
                msg = msg + b"!" if not msg else bytes([msg[0] ^ 1]) + msg[1:]
            elif kind == 3:
                at = ht + (i % p.d) * (p.hp + p.len) * p.n + (i % p.len) * p.n + i % p.n
                sig = sig[:at] + bytes([sig[at] ^ 0x10]) + sig[at + 1:]
            elif kind == 4:
                sig = bytes([sig[0] ^ 0x80]) + sig[1:]
            rows.append((pk, msg, sig))
            valid.append(kind < 2)
        out[name] = (rows, valid)
    return out


KEYS = ("digest", "fors_pk", "roots", "flags")


@pytest.mark.parametrize("name", NAMES)
def test_batches_of_mixed_rows(lib, ctx, mixed, name):
    rows, valid = mixed[name]
    traced = {}
    for n in (1, 2, 3, 4, 5, 63, 64, 65, 257):  # the edges of four rows per workgroup and of the front's 64 lanes
        out = run(lib, ctx, name, rows[:n])
        assert out["status"].tolist() == [0 if v else -1 for v in valid[:n]], n  # none left at the prefill 7
        traced[n] = out
    out = traced[257]
    for i in list(range(10)) + [63, 64, 65, 128, 255, 256]:  # 16 rows against the spec's trace
        check_trace(out, i, spec.verify_trace(name, *rows[i]))
    for n in (1, 2, 3, 4, 5, 63, 64, 65):  # a row's outputs do not depend on the batch around it
        for key in KEYS:
            assert np.array_equal(traced[n][key], out[key][:n]), (n, key)


@pytest.mark.parametrize("name", NAMES)
def test_chunked_batch_gives_identical_status_and_trace(lib, mixed, name):
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
    for key in KEYS:
        assert np.array_equal(parts[key], whole[key]), key


@pytest.mark.parametrize("name", NAMES)
def test_flavours_reject_each_other(lib, ctx, signed, name):
    pk, rows = signed[name]
    other = other_flavour(name)
    got = run(lib, ctx, other, [(pk, m, s) for m, s, _ in rows[:3]])
    assert got["status"].tolist() == [-1, -1, -1]
    for i, (m, s, _) in enumerate(rows[:3]):
        check_trace(got, i, spec.verify_trace(other, pk, m, s))


def test_context_string(lib, ctx, fixture, signed):
    import qrkem
    name = "SLH-DSA-SHA2-128f"
    f = fixture[name]
    pk, rows = signed[name]
    msg = gold.message(name + "-ctx", 100)
    for context in (b"qrkem handshake v1", bytes(range(255))):
        sig = spec.sign(name, f["sk"], msg, ctx=context)
        assert spec.verify(name, pk, msg, sig, ctx=context) and not spec.verify(name, pk, msg, sig)
        both = [(pk, msg, sig), (pk, rows[0][0], rows[0][1])]
        with_ctx = run(lib, ctx, name, both, context=context)
        assert with_ctx["status"].tolist() == [0, -1]
        check_trace(with_ctx, 0, spec.verify_trace(name, pk, msg, sig, ctx=context))
        check_trace(with_ctx, 1, spec.verify_trace(name, pk, rows[0][0], rows[0][1], ctx=context))
        assert run(lib, ctx, name, both)["status"].tolist() == [-1, 0]  # the same signature without its context
    # a SPHINCS+ name has no context string at all
    cs = _dev(np.frombuffer(b"x", np.uint8))
    assert lib.qrk_sig_verify_batch(ctx, b"SPHINCS+-SHA2-128f-simple", 1, cs.data_ptr(), cs.data_ptr(), cs.data_ptr(),
                                    cs.data_ptr(), cs.data_ptr(), 1, cs.data_ptr(), None) == -1
    assert "no context string" in qrkem.last_error()


@pytest.mark.parametrize("name", NAMES)
def test_class_agrees_with_the_abi(lib, ctx, signed, mixed, name):
    import qrkem
    p = spec.PARAMS[name]
    pk0, srows = signed[name]
    s = qrkem.SPHINCSSignature(LEVEL[p.n], fips205=p.fips)
    assert s.variant == name
    assert s.verify(pk0, srows[3][0], srows[3][1]) is True
    assert s.verify(pk0, srows[3][0] + b"x", srows[3][1]) is False
    assert s.verify(pk0, srows[0][0], srows[1][1]) is False
    rows, valid = mixed[name]
    rows, valid = rows[:65], valid[:65]
    got = s.verify_batch([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows])
    assert got.dtype == np.bool_ and got.tolist() == valid
    assert got.tolist() == (run(lib, ctx, name, rows, trace=False)["status"] == 0).tolist()
    # already-resident tensors plus offsets
    pk = _dev(np.frombuffer(b"".join(r[0] for r in rows), np.uint8).reshape(len(rows), p.pk))
    sig = _dev(np.frombuffer(b"".join(r[2] for r in rows), np.uint8).reshape(len(rows), p.sig))
    msg = _dev(np.frombuffer(b"".join(r[1] for r in rows), np.uint8))
    off = _dev(np.cumsum([0] + [len(r[1]) for r in rows]).astype(np.int64))
    assert s.verify_batch(pk, msg, sig, offsets=off).tolist() == valid
    st = s.verify_status(pk, msg, sig, offsets=off)
    assert st.is_cuda and st.dtype == torch.int32 and st.cpu().tolist() == [0 if v else -1 for v in valid]
    s.close()


@pytest.mark.parametrize("name", NAMES)
def test_row_with_decreasing_offsets(lib, ctx, fixture, name):
    """Three rows over one 20-byte buffer with offsets [0, 10, 5, 20]: the middle row is refused with FLAG_LONG
    and an all-zero trace, the outer rows are verified exactly as they are alone."""
    f = fixture[name]
    data = gold.message(name + "-offsets", 20)
    parts = [data[:10], data[5:20]]
    sigs = [spec.sign(name, f["sk"], m) for m in parts]
    alone = run(lib, ctx, name, [(f["pk"], m, s) for m, s in zip(parts, sigs)])
    assert alone["status"].tolist() == [0, 0]
    for i, (m, s) in enumerate(zip(parts, sigs)):
        check_trace(alone, i, spec.verify_trace(name, f["pk"], m, s))
    rows = [(f["pk"], parts[0], sigs[0]), (f["pk"], b"", sigs[0]), (f["pk"], parts[1], sigs[1])]
    out = run(lib, ctx, name, rows, shared=(data, [0, 10, 5, 20]))
    assert out["status"].tolist() == [0, -1, 0]
    assert int(out["flags"][1]) == spec.FLAG_LONG == 2
    for key in ("digest", "fors_pk", "roots"):
        assert not out[key][1].any(), key
        assert np.array_equal(out[key][[0, 2]], alone[key]), key
    assert out["flags"][[0, 2]].tolist() == [0, 0]
    assert run(lib, ctx, name, rows, shared=(data, [0, 10, 5, 20]), trace=False)["status"].tolist() == [0, -1, 0]
