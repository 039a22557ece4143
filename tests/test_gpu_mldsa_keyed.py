"""ML-DSA key sets (qrk_mldsa_pubkeys_load / qrk_mldsa_seckeys_load, qrk_mldsa_verify_keyed_batch,
qrk_mldsa_sign_keyed_batch, csrc/mldsa_keyed.hip) against tests/mldsa_spec.py and against the per-row calls on the
same rows: byte-level through the trace hooks, over every batch size, key count, index pattern and chunking at
which the keyed kernels take another path.  The fixture (3 keys, 8 messages at the SHAKE256 block edges of mu, each
signed once per key by the spec) is checked against the spec on the CPU first, in the one test without the gpu
mark."""
import ctypes as ct
import hashlib

import numpy as np
import pytest

import make_golden_mldsa as gold
import make_golden_mldsa_sign as sgold
import mldsa_spec as spec
import test_gpu_mldsa as per_row
import test_gpu_mldsa_sign as per_row_sign
from test_gpu_mldsa import MIX_LENGTHS, check_trace

torch = pytest.importorskip("torch")

gpu = pytest.mark.gpu
SETS = sorted(spec.PARAMS)
LEVEL = {"ML-DSA-44": 2, "ML-DSA-65": 3, "ML-DSA-87": 5}
FLAG_KEY = 16
SIZES = (1, 2, 63, 64, 65, 257)
KEYS = 3
# device bytes per key (public, secret): A_hat k l KiB, then t1_hat k KiB + tr, or the three NTT'd vectors
# (2 k + l) KiB + rho | K | tr + a flag word
SET_BYTES = {"ML-DSA-44": (20544, 28804), "ML-DSA-65": (36928, 48260), "ML-DSA-87": (65600, 81028)}
assert MIX_LENGTHS == (0, 69, 70, 71, 205, 206, 207, 2500)


# ------------------------------------------------------------------ the fixture, built once
def tamper(p, kind, msg, sig):
    """The pattern of test_gpu_mldsa.py: 2 a message bit, 3 a c~ bit, 4 a hint count above omega."""
    if kind == 2:
        msg = msg + b"!" if not msg else bytes([msg[0] ^ 1]) + msg[1:]
    elif kind == 3:
        sig = bytes([sig[0] ^ 0x80]) + sig[1:]
    elif kind == 4:
        sig = sig[:-1] + bytes([p.omega + 1])
    return msg, sig


def kind_of(i):
    return (i * 7 + i // 8) % 5


@pytest.fixture(scope="module")
def keyed():
    """Per set: 3 key pairs from fixed seeds, the 8 messages, the spec's deterministic signature of every message
    under every key, and 257 mixed rows (key i mod 3, message i mod 8, tampered in the fixed pattern)."""
    out = {}
    for name in SETS:
        p = spec.PARAMS[name]
        pairs = [spec.keygen_internal(spec.H(b"keyed" + name.encode() + bytes([j]), 32), name) for j in range(KEYS)]
        msgs = [gold.message(name + "-keyed", n) for n in MIX_LENGTHS]
        sigs = [[spec.sign(sk, m) for m in msgs] for _, sk in pairs]
        rows, index, valid = [], [], []
        for i in range(257):
            k, j = i % KEYS, i % len(msgs)
            msg, sig = tamper(p, kind_of(i), msgs[j], sigs[k][j])
            rows.append((msg, sig))
            index.append(k)
            valid.append(kind_of(i) < 2)
        out[name] = {"pks": [pk for pk, _ in pairs], "sks": [sk for _, sk in pairs], "msgs": msgs, "sigs": sigs,
                     "rows": rows, "index": index, "valid": valid}
    return out


def test_fixture_is_what_the_spec_says(keyed):
    """CPU: every untouched row verifies under spec.verify and every tampered row fails, so the fixture is known
    good before the GPU sees it (each distinct row once)."""
    for name in SETS:
        f = keyed[name]
        seen = {}
        for (msg, sig), k, want in zip(f["rows"], f["index"], f["valid"]):
            key = (k, msg, sig)
            if key not in seen:
                seen[key] = spec.verify(f["pks"][k], msg, sig)
            assert seen[key] is want, (name, k, len(msg))
        assert sum(f["valid"]) > 90 and len(f["valid"]) - sum(f["valid"]) > 140
        for k in range(KEYS):  # a signature under one key is not one under the next
            assert not spec.verify(f["pks"][(k + 1) % KEYS], f["msgs"][1], f["sigs"][k][1])


# ------------------------------------------------------------------ the library
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


def _stream():
    return ct.c_void_p(torch.cuda.current_stream().cuda_stream)


class KeySet:
    """A key set through the C ABI, freed on exit."""

    def __init__(self, lib, ctx, name, keys, secret):
        import qrkem
        p = spec.PARAMS[name]
        self.lib, self.h = lib, ct.c_void_p()
        blob = _dev(np.frombuffer(b"".join(keys), np.uint8).reshape(len(keys), p.sk if secret else p.pk))
        load = lib.qrk_mldsa_seckeys_load if secret else lib.qrk_mldsa_pubkeys_load
        assert load(ctx, name.encode(), len(keys), blob.data_ptr(), ct.byref(self.h), _stream()) == 0, qrkem.last_error()
        torch.cuda.synchronize()

    def info(self):
        out = (ct.c_size_t * 4)()
        assert self.lib.qrk_mldsa_keyset_info(self.h, out) == 0
        return list(out)

    def free(self):
        if self.h:
            self.lib.qrk_mldsa_keyset_free(self.h)
            self.h = ct.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
        return False


def _index(index):
    return None if index is None else _dev(np.asarray(index, dtype=np.uint32).view(np.int32))


def verify_keyed(lib, ctx, ks, name, rows, index, context=b"", trace=True, expect=0, shared=None):
    """rows: (msg, sig) pairs -> dict of numpy outputs, as test_gpu_mldsa.run gives them for the per-row call.
    shared = (buffer, offsets) replaces the rows' messages with one buffer and its len(rows) + 1 offsets."""
    import qrkem
    p = spec.PARAMS[name]
    n = len(rows)
    sig = _dev(np.frombuffer(b"".join(r[1] for r in rows), np.uint8).reshape(n, p.sig))
    data = b"".join(r[0] for r in rows) if shared is None else shared[0]
    msg = _dev(np.frombuffer(data or b"\0", np.uint8))
    offsets = np.cumsum([0] + [len(r[0]) for r in rows]) if shared is None else np.array(shared[1])
    assert len(offsets) == n + 1
    off = _dev(offsets.astype(np.uint64).view(np.int64))
    idx = _index(index)
    cs = _dev(np.frombuffer(context, np.uint8)) if context else None
    status = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    args = [ctx, ks.h, n, idx.data_ptr() if idx is not None else None, msg.data_ptr(), off.data_ptr(), sig.data_ptr(),
            cs.data_ptr() if cs is not None else None, len(context), status.data_ptr()]
    out = {}
    if trace:
        mu = torch.full((n, 64), 0xA5, dtype=torch.uint8, device="cuda")
        ctl = torch.full((n, 64), 0xA5, dtype=torch.uint8, device="cuda")
        w1 = torch.full((n, p.w1), 0xA5, dtype=torch.uint8, device="cuda")
        flags = torch.full((n,), 0x55, dtype=torch.int32, device="cuda")
        rc = lib.qrk_dbg_mldsa_verify_keyed_trace(*args, mu.data_ptr(), ctl.data_ptr(), w1.data_ptr(), flags.data_ptr(),
                                                  _stream())
    else:
        rc = lib.qrk_mldsa_verify_keyed_batch(*args, _stream())
    assert rc == expect, qrkem.last_error()
    torch.cuda.synchronize()
    if trace and rc == 0:
        out = {"mu": mu.cpu().numpy(), "ctilde": ctl.cpu().numpy(), "w1": w1.cpu().numpy(), "flags": flags.cpu().numpy()}
    out["status"] = status.cpu().numpy()
    return out


def sign_keyed(lib, ctx, ks, name, msgs, index, rnd=None, context=b"", max_iters=None, expect=0):
    """-> (signatures, status) and, with max_iters (the trace hook), also (mu, iters): what test_gpu_mldsa_sign.sign
    returns for the per-row call."""
    import qrkem
    p = spec.PARAMS[name]
    n = len(msgs)
    msg, off = per_row_sign._messages(msgs)
    idx = _index(index)
    rn = per_row_sign._rows(rnd, 32) if rnd is not None else None
    cs = _dev(np.frombuffer(context, np.uint8)) if context else None
    sig = torch.full((n, p.sig), 0xA5, dtype=torch.uint8, device="cuda")
    status = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    head = (ctx, ks.h, n, idx.data_ptr() if idx is not None else None, msg.data_ptr(), off.data_ptr(),
            rn.data_ptr() if rn is not None else None, cs.data_ptr() if cs is not None else None, len(context),
            sig.data_ptr(), status.data_ptr())
    if max_iters is None:
        rc = lib.qrk_mldsa_sign_keyed_batch(*head, _stream())
    else:
        mu = torch.full((n, 64), 0xA5, dtype=torch.uint8, device="cuda")
        iters = torch.full((n,), 0x5A5A, dtype=torch.int32, device="cuda")
        rc = lib.qrk_dbg_mldsa_sign_keyed_trace(*head, max_iters, mu.data_ptr(), iters.data_ptr(), _stream())
    assert rc == expect, qrkem.last_error()
    torch.cuda.synchronize()
    out = [r.tobytes() for r in sig.cpu().numpy()], status.cpu().tolist()
    if max_iters is not None:
        out += ([r.tobytes() for r in mu.cpu().numpy()], iters.cpu().tolist())
    return out


def same_trace(a, b, n=None):
    for key in ("mu", "ctilde", "w1", "flags", "status"):
        assert np.array_equal(a[key][:n], b[key][:n]), key


def per_row_rows(f, rows, index, pks=None):
    pks = pks or f["pks"]
    return [(pks[k], m, s) for (m, s), k in zip(rows, index)]


# ------------------------------------------------------------------ keyed verification
@gpu
@pytest.mark.parametrize("name", SETS)
def test_verify_matches_the_spec_and_the_per_row_hook(lib, ctx, keyed, name):
    """1: mu, c~', w1, flags and status equal the per-row hook's on all 257 mixed rows and the spec's trace on 16,
    at every batch size, and with the call cut into chunks of 64."""
    p, f = spec.PARAMS[name], keyed[name]
    rows, index = f["rows"], f["index"]
    want = per_row.run(lib, ctx, name, per_row_rows(f, rows, index))
    assert want["status"].tolist() == [0 if v else -1 for v in f["valid"]]
    with KeySet(lib, ctx, name, f["pks"], False) as ks:
        assert ks.info() == [KEYS, SETS.index(name), 0, KEYS * SET_BYTES[name][0]]
        for n in SIZES:
            got = verify_keyed(lib, ctx, ks, name, rows[:n], index[:n])
            same_trace(got, want, n)  # a row's outputs do not depend on the batch around it
            assert got["status"].tolist() == verify_keyed(lib, ctx, ks, name, rows[:n], index[:n],
                                                          trace=False)["status"].tolist()
        for i in list(range(10)) + [63, 64, 65, 128, 255, 256]:
            check_trace(p, got, i, spec.verify_trace(f["pks"][index[i]], *rows[i]))
        h = ct.c_void_p()
        assert lib.qrk_ctx_create(ct.byref(h), 0) == 0
        try:
            assert lib.qrk_ctx_set_chunk(h, 64) == 0  # 257 rows: four chunks of 64 and a one-row tail
            same_trace(verify_keyed(lib, h, ks, name, rows, index), want)
            assert verify_keyed(lib, h, ks, name, rows, index, trace=False)["status"].tolist() == want["status"].tolist()
        finally:
            lib.qrk_ctx_destroy(h)


@gpu
@pytest.mark.parametrize("name", SETS)
def test_verify_index_patterns_and_key_counts(lib, ctx, keyed, name):
    """All rows on key 0, all on key g - 1, cycling; g = 1 (with and without an index array), 3 and 65."""
    f = keyed[name]
    rows = f["rows"][:65]
    for g in (1, 3, 65):
        pks = [f["pks"][j % KEYS] for j in range(g)]
        with KeySet(lib, ctx, name, pks, False) as ks:
            assert ks.info()[:3] == [g, SETS.index(name), 0]
            patterns = [[0] * 65, [g - 1] * 65, [i % g for i in range(65)]] + ([None] if g == 1 else [])
            for index in patterns:
                flat = index or [0] * 65
                want = per_row.run(lib, ctx, name, per_row_rows(f, rows, flat, pks))
                same_trace(verify_keyed(lib, ctx, ks, name, rows, index), want)
            if g > 1:  # key_index == NULL is accepted only for a set of one key
                import qrkem
                verify_keyed(lib, ctx, ks, name, rows, None, expect=-1)
                assert "key_index" in qrkem.last_error()


@gpu
@pytest.mark.parametrize("name", SETS)
def test_verify_under_the_wrong_key(lib, ctx, keyed, name):
    """2: a signature valid under key 0, presented with key_index 1, fails with FLAG_HASH only."""
    f = keyed[name]
    rows = [(m, s) for m, s in zip(f["msgs"], f["sigs"][0])]
    with KeySet(lib, ctx, name, f["pks"], False) as ks:
        right = verify_keyed(lib, ctx, ks, name, rows, [0] * len(rows))
        wrong = verify_keyed(lib, ctx, ks, name, rows, [1] * len(rows))
    assert right["status"].tolist() == [0] * len(rows) and right["flags"].tolist() == [0] * len(rows)
    assert wrong["status"].tolist() == [-1] * len(rows) and wrong["flags"].tolist() == [spec.FLAG_HASH] * len(rows)


@gpu
@pytest.mark.parametrize("name", SETS)
def test_verify_bad_indices_are_refused_rows(lib, ctx, keyed, name):
    """An index of g and one of 0xFFFFFFFF between good rows: status -1, the flag word FLAG_KEY, zeros in the other
    trace outputs, and every other row as without them."""
    f = keyed[name]
    rows, index = f["rows"][:67], list(f["index"][:67])
    with KeySet(lib, ctx, name, f["pks"], False) as ks:
        clean = verify_keyed(lib, ctx, ks, name, rows, index)
        bad = {1: KEYS, 64: 0xFFFFFFFF, 66: KEYS + 61}
        for i, v in bad.items():
            index[i] = v
        got = verify_keyed(lib, ctx, ks, name, rows, index)
        plain = verify_keyed(lib, ctx, ks, name, rows, index, trace=False)
    for i in range(67):
        if i in bad:
            assert int(got["status"][i]) == -1 and int(got["flags"][i]) == FLAG_KEY
            assert not got["mu"][i].any() and not got["ctilde"][i].any() and not got["w1"][i].any()
        else:
            for key in ("mu", "ctilde", "w1", "flags", "status"):
                assert np.array_equal(got[key][i], clean[key][i]), (i, key)
    assert plain["status"].tolist() == got["status"].tolist()


@gpu
@pytest.mark.parametrize("name", SETS)
def test_verify_row_with_decreasing_offsets(lib, ctx, keyed, name):
    """As test_gpu_mldsa.test_row_with_decreasing_offsets, through the keyed call (its own copy of the offset
    check): offsets [0, 10, 5, 20] over one 20-byte buffer, the outer rows under two different keys."""
    f = keyed[name]
    data = gold.message(name + "-keyed-offsets", 20)
    parts, index = [data[:10], data[5:20]], [1, 2]
    sigs = [spec.sign(f["sks"][k], m) for k, m in zip(index, parts)]
    with KeySet(lib, ctx, name, f["pks"], False) as ks:
        alone = verify_keyed(lib, ctx, ks, name, list(zip(parts, sigs)), index)
        assert alone["status"].tolist() == [0, 0] and alone["flags"].tolist() == [0, 0]
        same_trace(alone, per_row.run(lib, ctx, name, per_row_rows(f, list(zip(parts, sigs)), index)))
        rows = [(parts[0], sigs[0]), (b"", sigs[0]), (parts[1], sigs[1])]
        for trace in (True, False):
            out = verify_keyed(lib, ctx, ks, name, rows, [1, 0, 2], trace=trace, shared=(data, [0, 10, 5, 20]))
            assert out["status"].tolist() == [0, -1, 0]
        out = verify_keyed(lib, ctx, ks, name, rows, [1, 0, 2], shared=(data, [0, 10, 5, 20]))
        assert int(out["flags"][1]) == 8  # FLAG_LONG
        for key in ("mu", "ctilde", "w1"):
            assert not out[key][1].any(), key
            assert np.array_equal(out[key][[0, 2]], alone[key]), key
        assert out["flags"][[0, 2]].tolist() == [0, 0]


@gpu
@pytest.mark.parametrize("name", SETS)
def test_verify_context_strings(lib, ctx, keyed, name):
    """3: context strings of 0, 1 and 255 bytes agree with the per-row call; 256 bytes are refused by the ABI."""
    import qrkem
    f = keyed[name]
    msg = f["msgs"][2]
    with KeySet(lib, ctx, name, f["pks"], False) as ks:
        for context in (b"", b"c", bytes(range(255))):
            sig = spec.sign(f["sks"][1], msg, ctx=context)
            rows, index = [(msg, sig)] + f["rows"][:8], [1] + f["index"][:8]
            got = verify_keyed(lib, ctx, ks, name, rows, index, context=context)
            same_trace(got, per_row.run(lib, ctx, name, per_row_rows(f, rows, index), context=context))
            assert int(got["status"][0]) == 0
            assert got["status"][1:].tolist() == ([0 if v else -1 for v in f["valid"][:8]] if not context else [-1] * 8)
        verify_keyed(lib, ctx, ks, name, f["rows"][:2], [0, 1], context=bytes(256), expect=-1)
        assert "255" in qrkem.last_error()
        verify_keyed(lib, ctx, ks, name, f["rows"][:2], [0, 1], context=bytes(256), trace=False, expect=-1)
        assert "255" in qrkem.last_error()


# ------------------------------------------------------------------ keyed signing
@pytest.fixture(scope="module")
def signing_rows(keyed):
    """Per set: 257 rows (key i mod 3, message i mod 8) with a randomiser per row."""
    out = {}
    for name in SETS:
        f = keyed[name]
        index = [i % KEYS for i in range(257)]
        msgs = [f["msgs"][i % len(f["msgs"])] for i in range(257)]
        rnd = [spec.H(b"keyed-rnd" + name.encode() + i.to_bytes(2, "little"), 32) for i in range(257)]
        out[name] = (index, msgs, rnd)
    return out


@gpu
@pytest.mark.parametrize("name", SETS)
def test_sign_matches_the_per_row_call_and_the_spec(lib, ctx, keyed, signing_rows, name):
    """4: with rnd given and with none (the deterministic case) the signatures equal qrk_mldsa_sign_batch's on all
    257 rows, mu and the iteration counts equal the per-row hook's, at every batch size and cut into chunks; the
    deterministic ones are the spec's own signatures of the fixture, and two hedged rows are checked against it."""
    f = keyed[name]
    index, msgs, rnd = signing_rows[name]
    sks = [f["sks"][k] for k in index]
    with KeySet(lib, ctx, name, f["sks"], True) as ks:
        assert ks.info() == [KEYS, SETS.index(name), 1, KEYS * SET_BYTES[name][1]]
        for r in (rnd, None):
            want = per_row_sign.sign(lib, ctx, name, sks, msgs, rnd=r, max_iters=814)
            assert want[1] == [0] * 257
            assert sign_keyed(lib, ctx, ks, name, msgs, index, rnd=r, max_iters=814) == want
            assert sign_keyed(lib, ctx, ks, name, msgs, index, rnd=r) == want[:2]
            for n in SIZES[:-1]:
                got = sign_keyed(lib, ctx, ks, name, msgs[:n], index[:n], rnd=r[:n] if r else None, max_iters=814)
                assert got == tuple(part[:n] for part in want), n
        # rnd = None: row i is the spec's signature of message i mod 8 under key i mod 3, which the fixture holds
        assert want[0] == [f["sigs"][k][i % 8] for i, k in enumerate(index)]
        hedged = sign_keyed(lib, ctx, ks, name, msgs[:2], index[:2], rnd=rnd[:2])[0]
        assert hedged == [spec.sign(sks[i], msgs[i], rnd=rnd[i]) for i in range(2)]
        h = ct.c_void_p()
        assert lib.qrk_ctx_create(ct.byref(h), 0) == 0
        try:
            assert lib.qrk_ctx_set_chunk(h, 64) == 0
            assert sign_keyed(lib, h, ks, name, msgs, index, max_iters=814) == want
        finally:
            lib.qrk_ctx_destroy(h)
        # g = 1 without an index array, and a context string
        with KeySet(lib, ctx, name, f["sks"][2:], True) as one:
            assert sign_keyed(lib, ctx, one, name, f["msgs"], None)[0] == f["sigs"][2]
            context = bytes(range(255))
            assert sign_keyed(lib, ctx, one, name, f["msgs"][:3], [0] * 3, rnd=rnd[:3], context=context) == \
                per_row_sign.sign(lib, ctx, name, [f["sks"][2]] * 3, f["msgs"][:3], rnd=rnd[:3], context=context)
        import qrkem
        sign_keyed(lib, ctx, ks, name, msgs[:2], index[:2], context=bytes(256), expect=-1)
        assert "255" in qrkem.last_error()
        sign_keyed(lib, ctx, ks, name, msgs[:2], None, expect=-1)
        assert "key_index" in qrkem.last_error()


@pytest.fixture(scope="module")
def golden_records():
    return sgold.load()


@gpu
@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("mode", [1, 2])
def test_sign_replays_the_golden_records(lib, ctx, golden_records, mode, name):
    """4: the records test_gpu_mldsa_sign.py replays from tests/golden/mldsa_sign.json (crafted keys and the
    threshold pairs among them) reproduce through the keyed call: one set of the distinct secret keys, one index
    per record.  Under both builds of the signing core (1: the NTT'd secret vectors held in LDS, 2: read from the
    set), each with status, mu, iteration counts and signatures equal to the per-row call's."""
    rows = golden_records[name]["rows"]
    sks = sorted({r["sk"] for r in rows})
    try:
        assert lib.qrk_dbg_mldsa_keyed_sign_mode(mode) == mode
        with KeySet(lib, ctx, name, sks, True) as ks:
            for ctx_len in (0, 255):
                part = [r for r in rows if r["ctx_len"] == ctx_len]
                msgs, context = [r["msg"] for r in part], sgold.CTX255[:ctx_len]
                got = sign_keyed(lib, ctx, ks, name, msgs, [sks.index(r["sk"]) for r in part], context=context,
                                 max_iters=814)
                assert got == per_row_sign.sign(lib, ctx, name, [r["sk"] for r in part], msgs, context=context,
                                                max_iters=814)
                sigs, status, mu, iters = got
                assert status == [0] * len(part)
                for r, s, m, it in zip(part, sigs, mu, iters):
                    assert it == r["iters"], (r["kind"], r["counter"])
                    assert m == per_row_sign.mu_of(r["sk"], r["msg"], context)
                    assert hashlib.sha3_256(s).hexdigest() == r["sig_sha3"], (r["kind"], r["counter"])
    finally:
        default = lib.qrk_dbg_mldsa_keyed_sign_mode(0)
    assert default in (1, 2)


@gpu
@pytest.mark.parametrize("name", SETS)
def test_sign_then_verify(lib, ctx, keyed, signing_rows, name):
    """5: every keyed signature verifies through verify_keyed and verify_batch, under a public set loaded from the
    public keys of the same key pairs; through the classes, with the index as a list, an array and a tensor."""
    import qrkem
    f = keyed[name]
    index, msgs, _ = signing_rows[name]
    index, msgs = index[:65], msgs[:65]
    signer = qrkem.MLDSASigner(LEVEL[name])
    with signer.load_secret_keys(f["sks"]) as sec, signer.load_public_keys(f["pks"]) as pub:
        assert (sec.g, sec.secret, sec.variant) == (KEYS, True, name) and sec.device_bytes == KEYS * SET_BYTES[name][1]
        assert (pub.g, pub.secret, pub.variant) == (KEYS, False, name) and pub.device_bytes == KEYS * SET_BYTES[name][0]
        sigs = signer.sign_keyed(sec, msgs, index)  # hedged
        assert sigs.is_cuda and tuple(sigs.shape) == (65, signer.signature_size)
        assert signer.verify_keyed(pub, msgs, sigs, index).tolist() == [True] * 65
        assert signer.verify_keyed(pub, msgs, sigs, np.asarray(index, dtype=np.int64)).tolist() == [True] * 65
        status = signer.verify_keyed_status(pub, msgs, sigs, torch.tensor(index, dtype=torch.int32, device="cuda"))
        assert status.is_cuda and status.dtype == torch.int32 and status.cpu().tolist() == [0] * 65
        assert signer.verify_batch([f["pks"][k] for k in index], msgs, sigs).tolist() == [True] * 65
        shifted = [(k + 1) % KEYS for k in index]
        assert signer.verify_keyed(pub, msgs, sigs, shifted).tolist() == [False] * 65
        host = [r.tobytes() for r in sigs.cpu().numpy()]
        assert all(spec.verify(f["pks"][index[i]], msgs[i], host[i]) for i in (0, 1, 64))
        assert host != [r.tobytes() for r in signer.sign_keyed(sec, msgs, index).cpu().numpy()]  # fresh rnd per call
        det = qrkem.MLDSASigner(LEVEL[name], deterministic=True)
        again = det.sign_keyed(sec, msgs[:8], index[:8])
        assert [r.tobytes() for r in again.cpu().numpy()] == [f["sigs"][index[i]][i] for i in range(8)]
        # refused rows: an index outside the set
        with pytest.raises(RuntimeError, match="1 of 3 rows were refused"):
            det.sign_keyed(sec, msgs[:3], [0, KEYS, 2])
        got, st = det.sign_keyed(sec, msgs[:3], [0, KEYS, 2], return_status=True)
        assert st.cpu().tolist() == [0, -1, 0] and not got[1].any()
        # a set of the other kind reaches neither call, in Python or through the ABI
        with pytest.raises(ValueError, match="public key set cannot sign"):
            signer.sign_keyed(pub, msgs, index)
        with pytest.raises(ValueError, match="secret key set cannot verify"):
            signer.verify_keyed(sec, msgs, sigs, index)
        buf = ct.c_void_p(sigs.data_ptr())
        assert lib.qrk_mldsa_sign_keyed_batch(signer._context(), pub._handle, 0, None, None, None, None, None, 0, None,
                                              None, None) == -1
        assert "foreign key set" in qrkem.last_error() and "cannot sign" in qrkem.last_error()
        assert lib.qrk_mldsa_verify_keyed_batch(signer._context(), sec._handle, 1, buf, buf, buf, buf, None, 256, buf,
                                                None) == -1
        assert "foreign key set" in qrkem.last_error() and "cannot verify" in qrkem.last_error()
    assert sec.closed and pub.closed and sec.device_bytes == 0
    with pytest.raises(ValueError, match="closed"):
        signer.verify_keyed(pub, msgs, sigs, index)
    signer.close()


@gpu
@pytest.mark.parametrize("name", SETS)
def test_sign_corrupt_secret_key(lib, ctx, keyed, signing_rows, name):
    """6: a set with one key whose first s1 field is 2 eta + 1 refuses exactly the rows that index it (status -1,
    zero signatures) and signs the others."""
    p, f = spec.PARAMS[name], keyed[name]
    index, msgs, _ = signing_rows[name]
    index, msgs = index[:65], msgs[:65]
    ebits = (2 * p.eta).bit_length()
    bad = bytearray(f["sks"][1])
    bad[128] = (bad[128] & ~((1 << ebits) - 1)) | (2 * p.eta + 1)
    s1 = spec.sk_decode(p, bytes(bad))[3]
    assert int(s1[0][0]) == p.eta - (2 * p.eta + 1) == -p.eta - 1
    zero = bytes(p.sig)
    with KeySet(lib, ctx, name, [f["sks"][0], bytes(bad), f["sks"][2]], True) as ks:
        sigs, status, mu, iters = sign_keyed(lib, ctx, ks, name, msgs, index, max_iters=814)
    for i, k in enumerate(index):
        if k == 1:
            assert status[i] == -1 and sigs[i] == zero and iters[i] == 0
        else:
            assert status[i] == 0 and sigs[i] == f["sigs"][k][i % 8]


@gpu
@pytest.mark.parametrize("name", SETS)
def test_sign_iteration_cap_and_bad_indices(lib, ctx, keyed, signing_rows, name):
    """7: max_iters = 1 gives status -1 and a zero signature exactly on the rows whose per-row trace reports more
    than one iteration.  And an index of g or 0xFFFFFFFF between good rows is a refused row that ran nothing."""
    p, f = spec.PARAMS[name], keyed[name]
    index, msgs, rnd = signing_rows[name]
    index, msgs, rnd = list(index[:67]), msgs[:67], rnd[:67]
    sks = [f["sks"][k] for k in index]
    zero = bytes(p.sig)
    full = per_row_sign.sign(lib, ctx, name, sks, msgs, rnd=rnd, max_iters=814)
    assert min(full[3]) == 1 < max(full[3])  # both kinds of row are present
    with KeySet(lib, ctx, name, f["sks"], True) as ks:
        sigs, status, mu, iters = sign_keyed(lib, ctx, ks, name, msgs, index, rnd=rnd, max_iters=1)
        for i in range(67):
            if full[3][i] > 1:
                assert status[i] == -1 and sigs[i] == zero and iters[i] == 1
            else:
                assert status[i] == 0 and sigs[i] == full[0][i] and iters[i] == 1
        assert mu == full[2]
        bad = {1: KEYS, 64: 0xFFFFFFFF, 66: KEYS + 61}
        for i, v in bad.items():
            index[i] = v
        sigs, status, mu, iters = sign_keyed(lib, ctx, ks, name, msgs, index, rnd=rnd, max_iters=814)
        for i in range(67):
            if i in bad:
                assert (status[i], sigs[i], iters[i], mu[i]) == (-1, zero, 0, bytes(64))
            else:
                assert (status[i], sigs[i], iters[i], mu[i]) == (0, full[0][i], full[3][i], full[2][i])


# ------------------------------------------------------------------ the handle
@gpu
@pytest.mark.parametrize("name", SETS)
def test_info_free_and_reload(lib, ctx, keyed, name):
    """8: qrk_mldsa_keyset_info reports g and the kind; after qrk_mldsa_keyset_free and a new load of other keys the
    results are those of the new keys."""
    f = keyed[name]
    rows = [(m, s) for m, s in zip(f["msgs"], f["sigs"][0])]
    ks = KeySet(lib, ctx, name, f["pks"][:2], False)
    assert ks.info() == [2, SETS.index(name), 0, 2 * SET_BYTES[name][0]]
    assert verify_keyed(lib, ctx, ks, name, rows, [0] * 8)["status"].tolist() == [0] * 8
    ks.free()
    with KeySet(lib, ctx, name, [f["pks"][2], f["pks"][1], f["pks"][0]], False) as ks:
        assert ks.info()[0] == 3
        assert verify_keyed(lib, ctx, ks, name, rows, [0] * 8)["status"].tolist() == [-1] * 8
        assert verify_keyed(lib, ctx, ks, name, rows, [2] * 8)["status"].tolist() == [0] * 8
    sec = KeySet(lib, ctx, name, f["sks"][:1], True)
    assert sec.info() == [1, SETS.index(name), 1, SET_BYTES[name][1]]
    assert sign_keyed(lib, ctx, sec, name, f["msgs"][:2], None)[0] == f["sigs"][0][:2]
    sec.free()
    with KeySet(lib, ctx, name, f["sks"][1:], True) as sec:
        assert sec.info()[:3] == [2, SETS.index(name), 1]
        assert sign_keyed(lib, ctx, sec, name, f["msgs"][:2], [0, 1])[0] == [f["sigs"][1][0], f["sigs"][2][1]]
