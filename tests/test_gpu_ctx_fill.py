"""GPU: no call depends on what the context's buffers held before it.

One qrk_ctx owns one device scratch that every family carves its own way, beside hs_scratch, dio, dstage and the
pinned hio / hstage; the buffers only grow, so a call finds whatever the last call left.  Everywhere else in the
suite that is either a fresh allocation (zeros) or the leftovers of an identical call (the right values already).
Here every call runs on an explicit context after qrk_dbg_ctx_fill has written 0xFF, then 0x00, over every one of
those buffers ("What a call finds in the context's buffers"), and every output byte is compared with
the oracle, the Python specs or a committed fixture -- never with a second run of the library.  A kernel that read
a word its own call had not written, or that relied on a region being zero, gives wrong bytes under one of the two
fills.

The wrapper classes (BatchKEM, the signature classes, the ciphers, the handshake driver) are thin ctypes shims over
the C ABI that pass `self._ctx`; Ctx.adopt points them at the context under test instead of one of their own.
"""
import ctypes as ct
import functools
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

import aead_spec
import oracle as orc

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

FILLS = (0xFF, 0x00)
MLKEM = ["ML-KEM-512", "ML-KEM-768", "ML-KEM-1024"]
FRODO = ["FrodoKEM-640-SHAKE", "FrodoKEM-976-SHAKE", "FrodoKEM-1344-SHAKE",
         "FrodoKEM-640-AES", "FrodoKEM-976-AES", "FrodoKEM-1344-AES"]
HQC = ["HQC-128", "HQC-192", "HQC-256"]
SMALL_MAX = 1024  # mlkem_small_max(): up to here ML-KEM runs its one-launch kernels, above it the batched ones
MLDSA_LEVEL = {"ML-DSA-44": 2, "ML-DSA-65": 3, "ML-DSA-87": 5}


# ------------------------------------------------------------------ the context under test
class Ctx:
    """One qrk_ctx, made and filled through the C ABI."""

    def __init__(self, chunk=None):
        from qrkem._debug import bind
        self.lib = bind()
        self.h = ct.c_void_p()
        assert self.lib.qrk_ctx_create(ct.byref(self.h), 0) == 0
        if chunk:
            assert self.lib.qrk_ctx_set_chunk(self.h, chunk) == 0

    def fill(self, byte):
        import qrkem
        assert self.lib.qrk_dbg_ctx_fill(self.h, byte) == 0, qrkem.last_error()

    def adopt(self, obj):
        """Point a wrapper object at this context; it no longer owns (or destroys) one."""
        if getattr(obj, "_ctx", None):
            obj.close()
        obj._ctx = self.h
        obj.close = lambda: None
        return obj

    def kem(self, alg):
        from qrkem.batch import BatchKEM
        return self.adopt(BatchKEM(alg, device=0))

    def close(self):
        self.lib.qrk_ctx_destroy(self.h)


@pytest.fixture
def ctx():
    c = Ctx()
    yield c
    c.close()


def through_fills(ctx, call, warm, rounds):
    """The shape of every test here.  call(inputs, dirty) makes the library calls under test and calls dirty()
    before each of them.  First on `warm`, with nothing filled: that sizes the context's buffers.  Then once per
    byte of FILLS on the next of `rounds` (same shapes as `warm`, different bytes), with dirty() filling every
    buffer of the context with that byte.  Returns the outputs of the rounds, for the reference to judge."""
    call(warm, lambda: None)
    assert len(rounds) == len(FILLS)
    return [call(inp, functools.partial(ctx.fill, byte)) for byte, inp in zip(FILLS, rounds)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ------------------------------------------------------------------ the hook bites
def aead_residue(ctx):
    out = ct.c_uint64(123)
    assert ctx.lib.qrk_dbg_aead_long_residue(ctx.h, ct.byref(out)) == 0
    return out.value


def test_fill_lands_in_the_long_aead_partials(ctx):
    import test_gpu_aead_long as tl
    keys, nonces, pts, aads, lens = tl.four_rows("AES-256-GCM")
    tl.seal(ctx.h, "AES-256-GCM", keys, nonces, pts, aads, 2 * tl.S + 17)
    assert aead_residue(ctx) == 0
    ctx.fill(0xFF)
    assert aead_residue(ctx) == 0xFF
    ctx.fill(0x00)
    assert aead_residue(ctx) == 0


def test_fill_lands_in_the_mlkem_records(ctx):
    alg, n = "ML-KEM-768", SMALL_MAX + 1  # the batched path: the one-launch kernels keep no records in the scratch
    eng = ctx.kem(alg)
    eng.keypair(coins=dev(orc.bench_coins(n, 64, seed=1)))
    torch.cuda.synchronize()
    out = ct.c_uint64(123)
    assert ctx.lib.qrk_dbg_mlkem_records_residue(ctx.h, alg.encode(), n, ct.byref(out)) == 0
    assert out.value == 0
    record_bytes = 16 * 8 * ((n + 63) // 64 * 64)  # seeds | m' | K' | Kbar: 4 u64 each, per handshake of the 64-tile
    ctx.fill(0xFF)
    assert ctx.lib.qrk_dbg_mlkem_records_residue(ctx.h, alg.encode(), n, ct.byref(out)) == 0
    assert out.value == record_bytes
    ctx.fill(0x00)
    assert ctx.lib.qrk_dbg_mlkem_records_residue(ctx.h, alg.encode(), n, ct.byref(out)) == 0
    assert out.value == 0


def test_fill_leaves_the_invariants_alone(ctx):
    """The ML-KEM counter words and the single-shot flag words are state, not scratch: the fill leaves the
    counters and the parity as they were and the flag words zero."""
    alg = "ML-KEM-768"
    eng = ctx.kem(alg)
    r = kem_ref(alg, 3, 77)
    eng.keypair(coins=r["kc"])  # host pointers: the pipelined single-shot KeyGen and its flag words
    eng.encaps(dev(kem_ref(alg, SMALL_MAX + 1, 78)["pk"]), coins=dev(kem_ref(alg, SMALL_MAX + 1, 78)["ec"]))
    torch.cuda.synchronize()
    words, parity, flags = (ct.c_uint32 * 2)(), ct.c_int(), ct.c_uint64(9)
    assert ctx.lib.qrk_dbg_fixc_words(ctx.h, words, ct.byref(parity)) == 0
    before = (list(words), parity.value)
    ctx.fill(0xFF)
    assert ctx.lib.qrk_dbg_fixc_words(ctx.h, words, ct.byref(parity)) == 0
    assert (list(words), parity.value) == before
    assert ctx.lib.qrk_dbg_kg_flags_residue(ctx.h, ct.byref(flags)) == 0 and flags.value == 0


# ------------------------------------------------------------------ KEMs against the oracle
@functools.lru_cache(maxsize=None)
def kem_ref(alg, n, seed):
    """Fixed coins and what the oracle makes of them; `bad` has every odd row's ciphertext tampered (first, middle
    and last byte in turn), `ss_bad` / `st_bad` are the oracle's Decaps of it."""
    s = orc.sizes(alg)
    kp, en = s["keypair_coins"], s["encaps_coins"]
    coins = orc.bench_coins(n, kp + en, seed=seed)
    kc, ec = np.ascontiguousarray(coins[:, :kp]), np.ascontiguousarray(coins[:, kp:])
    pk, sk = orc.batch_keypair(alg, kc, 8)
    c, ss = orc.batch_encaps(alg, pk, ec, 8)
    bad = c.copy()
    L = bad.shape[1]
    for i in range(1, n, 2):
        bad[i, (0, L // 2, L - 1)[(i // 2) % 3]] ^= 1 << (i % 8)
    ss_bad, st_bad = orc.batch_decaps(alg, sk, bad, 8, with_status=True)
    return {"kc": kc, "ec": ec, "pk": pk, "sk": sk, "ct": c, "ss": ss, "bad": bad, "ss_bad": ss_bad, "st_bad": st_bad}


def kem_warm(alg, n):
    """Inputs of the right shapes and arbitrary bytes: the warm-up's outputs are not looked at."""
    s = orc.sizes(alg)
    rng = np.random.default_rng(n + len(alg))
    b = lambda w: rng.integers(0, 256, (n, w), dtype=np.uint8)  # noqa: E731
    return {"kc": b(s["keypair_coins"]), "ec": b(s["encaps_coins"]), "pk": b(s["pk"]), "sk": b(s["sk"]), "bad": b(s["ct"])}


def kem_call(eng, inp, dirty, on_host=False):
    up = (lambda a: a) if on_host else dev
    dn = (lambda a: a) if on_host else host
    dirty()
    pk, sk = eng.keypair(coins=up(inp["kc"]))
    pk, sk = dn(pk), dn(sk)
    dirty()
    c, ss, st = eng.encaps(up(inp["pk"]), coins=up(inp["ec"]), return_status=True)
    c, ss, st = dn(c), dn(ss), dn(st)
    dirty()
    ss2, st2 = eng.decaps(up(inp["sk"]), up(inp["bad"]), return_status=True)
    return {"pk": pk, "sk": sk, "ct": c, "ss": ss, "st": st, "ss_bad": dn(ss2), "st_bad": dn(st2)}


def kem_check(r, out, what):
    n = len(r["kc"])
    for key in ("pk", "sk", "ct", "ss", "ss_bad"):
        assert np.array_equal(out[key], r[key]), (what, key)
    assert not out["st"].any(), what
    assert np.array_equal(out["st_bad"], r["st_bad"]), what
    # the tampering did what it is there for: every odd row took the rejection path
    assert not np.any(np.all(r["ss_bad"][1::2] == r["ss"][1::2], axis=1)), what
    assert np.array_equal(r["ss_bad"][0::2], r["ss"][0::2]) and len(r["ss"]) == n


def kem_through_fills(ctx, alg, n, on_host=False):
    eng = ctx.kem(alg)
    rounds = [kem_ref(alg, n, 0xF111 + 2 * n), kem_ref(alg, n, 0xF112 + 2 * n)]
    outs = through_fills(ctx, functools.partial(kem_call, eng, on_host=on_host), kem_warm(alg, n), rounds)
    for byte, r, out in zip(FILLS, rounds, outs):
        kem_check(r, out, (alg, n, hex(byte)))


@pytest.mark.parametrize("n", [1, 65, SMALL_MAX, SMALL_MAX + 1])
@pytest.mark.parametrize("alg", MLKEM)
def test_mlkem_after_fill(ctx, alg, n):
    kem_through_fills(ctx, alg, n)


@pytest.mark.parametrize("n", [1, 65])
@pytest.mark.parametrize("alg", FRODO + HQC)
def test_frodo_and_hqc_after_fill(ctx, alg, n):
    kem_through_fills(ctx, alg, n)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("alg", ["ML-KEM-512", "ML-KEM-768", "ML-KEM-1024", "FrodoKEM-640-SHAKE", "FrodoKEM-976-AES",
                                 "HQC-128"])
def test_host_pointer_calls_after_fill(ctx, alg, n):
    """The OQS-shaped path: host pointers, dio and the pinned mirror hio (ML-KEM: zero-copy through hio, the
    completion flag at n = 1, the pipelined KeyGen)."""
    kem_through_fills(ctx, alg, n, on_host=True)


@pytest.mark.parametrize("alg", ["ML-KEM-768", "FrodoKEM-976-AES", "HQC-192"])
def test_os_coins_after_fill(ctx, alg):
    """Coins from the OS go through hstage and dstage.  No fixed coins, so: both sides agree, and the oracle's
    Decaps of the returned (sk, ct) gives the same secret."""
    eng, n = ctx.kem(alg), 65

    def call(_, dirty):
        dirty()
        pk, sk = eng.keypair(n=n)
        dirty()
        c, ss = eng.encaps(pk)
        dirty()
        return {"sk": host(sk), "ct": host(c), "ss": host(ss), "ss2": host(eng.decaps(sk, c))}

    for byte, out in zip(FILLS, through_fills(ctx, call, None, [None, None])):
        assert np.array_equal(out["ss"], out["ss2"]), (alg, hex(byte))
        assert np.array_equal(orc.batch_decaps(alg, out["sk"], out["ct"], 8), out["ss"]), (alg, hex(byte))
        assert len({r.tobytes() for r in out["ss"]}) == n


@pytest.mark.parametrize("alg", ["ML-KEM-768", "FrodoKEM-640-SHAKE", "HQC-128"])
def test_chunks_of_one_call_reuse_each_others_scratch(alg):
    """qrk_ctx_set_chunk(64) and n = 130: three chunks of one call in the same scratch, after a fill."""
    ctx = Ctx(chunk=64)
    try:
        kem_through_fills(ctx, alg, 130)
    finally:
        ctx.close()


@pytest.mark.parametrize("alg", ["FrodoKEM-976-SHAKE", "FrodoKEM-640-AES"])
def test_frodo_forward_hooks_after_fill(ctx, alg):
    """qrk_dbg_frodo_sample and qrk_dbg_frodo_from_samples (both modes), n = 65 on the context under test: the
    sampler's regions with their zeroed pad columns, ct and pk against frodo_spec (tests/frodo_forward_cases.py)."""
    import frodo_forward_cases as W
    import frodo_spec as F
    import test_gpu_frodo_forward as tf
    eng, p, n = ctx.kem(alg), F.params(alg), 65
    gold = tf._gold()[alg]

    def call(seed, dirty):
        out = {}
        for kg in (False, True):
            words = np.roll(np.resize(W.every_word_rows(p, kg, True), (n, W.words_per_row(p, kg))), seed, axis=1)
            dirty()
            got = [None if g is None else host(g) for g in tf.run_sample(ctx.lib, eng, kg, dev(words.view(np.int16)))]
            out["sample", kg] = (got, W.sampler_expected(p, kg, words))
            inp = W.from_samples_inputs(alg, kg)
            idx = (np.arange(n) + seed) % len(inp["names"])
            dirty()
            got = tf.run_from_samples(ctx.lib, eng, kg, inp, idx)
            out["rows", kg] = (got[0] if kg else got, idx)
        return out

    for byte, out in zip(FILLS, through_fills(ctx, call, 0, [5, 11])):
        for kg in (False, True):
            got, want = out["sample", kg]
            for g, w in zip(got, want):
                assert (g is None and w is None) or np.array_equal(g.reshape(w.shape), w), (alg, hex(byte), kg)
            rows, idx = out["rows", kg]
            names = W.from_samples_inputs(alg, kg)["names"]
            assert W.digests(rows) == [gold["keygen" if kg else "encaps"][names[i]] for i in idx], (alg, hex(byte), kg)


# ------------------------------------------------------------------ key sets
def test_mlkem_key_sets_after_fill(ctx):
    alg, g, n = "ML-KEM-768", 5, 65
    eng = ctx.kem(alg)
    keys = kem_ref(alg, g, 0x5E7)
    pub, sec = eng.load_public_keys(dev(keys["pk"])), eng.load_secret_keys(dev(keys["sk"]))
    index = (np.arange(n) * 3 % g).astype(np.uint32)
    rounds = []
    for seed in (1, 2):
        coins = orc.bench_coins(n, 32, seed=0x5E70 + seed)
        c, ss = orc.batch_encaps(alg, keys["pk"][index], coins, 8)
        bad = c.copy()
        bad[1::2, 7] ^= 0x20
        rounds.append({"ec": coins, "ct": c, "ss": ss, "bad": bad, "ss_bad": orc.batch_decaps(alg, keys["sk"][index], bad, 8)})

    def call(inp, dirty):
        dirty()
        c, ss, st = eng.encaps_keyed(pub, index, coins=dev(inp["ec"]), return_status=True)
        c, ss, st = host(c), host(ss), host(st)
        dirty()
        ss2, st2 = eng.decaps_keyed(sec, dev(inp["bad"]), index, return_status=True)
        return {"ct": c, "ss": ss, "st": st, "ss_bad": host(ss2), "st2": host(st2)}

    try:
        warm = {"ec": orc.bench_coins(n, 32, seed=9), "bad": rounds[0]["ct"]}
        for byte, r, out in zip(FILLS, rounds, through_fills(ctx, call, warm, rounds)):
            for key in ("ct", "ss", "ss_bad"):
                assert np.array_equal(out[key], r[key]), (hex(byte), key)
            assert not out["st"].any() and not out["st2"].any()
    finally:
        pub.close()
        sec.close()


@pytest.mark.parametrize("name", sorted(MLDSA_LEVEL))
def test_mldsa_key_sets_after_fill(ctx, name):
    """Keyed verify over the fixture's signatures and the tamper entries that keep its key; keyed deterministic
    signing of the honest fixture rows: the set is loaded before the fill and must not notice it."""
    import qrkem
    import make_golden_mldsa as gold
    import make_golden_mldsa_sign as sgold
    f, s = gold.load()[name], sgold.load()[name]
    signer = ctx.adopt(qrkem.MLDSASigner(MLDSA_LEVEL[name], deterministic=True))
    pub, sec = signer.load_public_keys([f["pk"]]), signer.load_secret_keys([s["sk"]])
    rows = [(f["pk"], m, sg) for m, sg in zip(f["msgs"], f["sigs"])]
    rows += [t for t in (gold.apply_tamper(e, f["pk"], f["msgs"], f["sigs"]) for e in f["tampers"]) if t[0] == f["pk"]]
    want = [0] * len(f["msgs"]) + [-1] * (len(rows) - len(f["msgs"]))
    assert -1 in want
    honest = [r for r in s["rows"] if r["kind"] == "honest" and r["ctx_len"] == 0 and r["sk"] == s["sk"]]
    assert honest

    def call(_, dirty):
        dirty()
        st = host(signer.verify_keyed_status(pub, [r[1] for r in rows], [r[2] for r in rows]))
        dirty()
        sig, sst = signer.sign_keyed(sec, [r["msg"] for r in honest], return_status=True)
        return st.tolist(), host(sig), host(sst)

    try:
        for byte, (st, sig, sst) in zip(FILLS, through_fills(ctx, call, None, [None, None])):
            assert st == want, hex(byte)
            assert not sst.any()
            assert [hashlib.sha3_256(x.tobytes()).hexdigest() for x in sig] == [r["sig_sha3"] for r in honest], hex(byte)
    finally:
        pub.close()
        sec.close()


# ------------------------------------------------------------------ ML-DSA
def mldsa_verify_rows(name):
    import make_golden_mldsa as gold
    f = gold.load()[name]
    return f, [(f["pk"], m, s) for m, s in zip(f["msgs"], f["sigs"])] + \
        [gold.apply_tamper(e, f["pk"], f["msgs"], f["sigs"]) for e in f["tampers"]]


def mldsa_verify_check(ctx, name, rows=None):
    """qrk_dbg_mldsa_verify_trace over the fixture rows, then its tamper entries (status, flags, mu, c~', w1)."""
    import mldsa_spec as spec
    import test_gpu_mldsa as tv
    f, all_rows = mldsa_verify_rows(name)
    rows = all_rows if rows is None else rows
    p = spec.PARAMS[name]
    out = tv.run(ctx.lib, ctx.h, name, rows)
    for i, rec in enumerate(f["records"]):
        assert int(out["status"][i]) == 0 and int(out["flags"][i]) == 0
        assert out["mu"][i].tobytes().hex() == rec["mu"]
        assert out["ctilde"][i].tobytes() == bytes.fromhex(rec["ctilde"]) + bytes(64 - p.ctilde)
        assert hashlib.sha3_256(out["w1"][i].tobytes()).hexdigest() == rec["w1_sha3"]
    for i, e in enumerate(f["tampers"], start=len(f["records"])):
        assert int(out["status"][i]) == -1 and int(out["flags"][i]) == e["flags"], e["label"]
        if e["flags"] & spec.FLAG_HINT:
            assert not out["mu"][i].any() and not out["ctilde"][i].any() and not out["w1"][i].any(), e["label"]
    return out


@pytest.mark.parametrize("name", sorted(MLDSA_LEVEL))
def test_mldsa_verify_after_fill(ctx, name):
    import mldsa_spec as spec
    import test_gpu_mldsa as tv
    _, rows = mldsa_verify_rows(name)
    tv.run(ctx.lib, ctx.h, name, rows[::-1])  # warm-up: the same rows in another order
    want = {i: spec.verify_trace(*rows[i]) for i in (len(rows) - 1, len(rows) - 2)}
    for byte in FILLS:
        ctx.fill(byte)
        out = mldsa_verify_check(ctx, name)
        for i, tr in want.items():  # two tamper rows byte for byte against the spec's trace
            tv.check_trace(spec.PARAMS[name], out, i, tr)
        ctx.fill(byte)
        wide = tv.run(ctx.lib, ctx.h, name, [rows[i % len(rows)] for i in range(65)])  # a second block of 64 lanes
        for key in ("status", "flags", "mu", "ctilde", "w1"):
            assert np.array_equal(wide[key], out[key][np.arange(65) % len(rows)]), (hex(byte), key)


@pytest.mark.parametrize("name", sorted(MLDSA_LEVEL))
def test_mldsa_keygen_and_sign_after_fill(ctx, name):
    import make_golden_mldsa_sign as sgold
    import test_gpu_mldsa_sign as ts
    s = sgold.load()[name]
    rows = [r for r in s["rows"] if r["ctx_len"] == 0]
    ts.keygen(ctx.lib, ctx.h, name, [bytes(32)] * 65)
    ts.sign(ctx.lib, ctx.h, name, [r["sk"] for r in rows][::-1], [r["msg"] for r in rows][::-1])
    for byte in FILLS:
        for n in (1, 65):
            ctx.fill(byte)
            pk, sk = ts.keygen(ctx.lib, ctx.h, name, [s["xi"]] * n)
            assert pk == [s["pk"]] * n and sk == [s["sk"]] * n, (hex(byte), n)
        ctx.fill(byte)
        sigs, status = ts.sign(ctx.lib, ctx.h, name, [r["sk"] for r in rows], [r["msg"] for r in rows])
        assert status == [0] * len(rows)
        assert [hashlib.sha3_256(x).hexdigest() for x in sigs] == [r["sig_sha3"] for r in rows], hex(byte)
        ctx.fill(byte)
        one, status = ts.sign(ctx.lib, ctx.h, name, [rows[0]["sk"]], [rows[0]["msg"]])
        assert status == [0] and hashlib.sha3_256(one[0]).hexdigest() == rows[0]["sig_sha3"]


# ------------------------------------------------------------------ SLH-DSA
@functools.lru_cache(maxsize=None)
def slhdsa_rows(name):
    """The fixture's signed rows and the tampers of one of them, each with the spec's verify trace."""
    import make_golden_slhdsa as gold
    import slhdsa_spec as spec
    from test_slhdsa_spec import tampers
    f = gold.load()[name]
    sigs = gold.signatures(name, f)  # checks the stored SHA3-256 of every signature first
    rows = [(f["pk"], m, s) for m, s in zip(f["msgs"], sigs)]
    rows += [c[1:4] for c in tampers(spec.PARAMS[name], f["pk"], f["msgs"][1], sigs[1])]
    return f, rows, [spec.verify_trace(name, *r) for r in rows]


def slhdsa_verify_check(ctx, name):
    import test_gpu_slhdsa as tv
    f, rows, traces = slhdsa_rows(name)
    out = tv.run(ctx.lib, ctx.h, name, rows)
    for i, rec in enumerate(f["records"]):
        assert out["digest"][i].tobytes().hex() == rec["digest"] and out["fors_pk"][i].tobytes().hex() == rec["fors_pk"]
        assert hashlib.sha3_256(out["roots"][i].tobytes()).hexdigest() == rec["roots_sha3"]
    for i, tr in enumerate(traces):
        tv.check_trace(out, i, tr)
    assert out["status"].tolist() == [0] * len(f["records"]) + [-1] * (len(rows) - len(f["records"]))
    return out


SLH_NAMES = ["SPHINCS+-SHA2-128f-simple", "SLH-DSA-SHA2-128f", "SPHINCS+-SHA2-192f-simple", "SLH-DSA-SHA2-192f",
             "SPHINCS+-SHA2-256f-simple", "SLH-DSA-SHA2-256f"]


@pytest.mark.parametrize("name", SLH_NAMES)
def test_slhdsa_verify_after_fill(ctx, name):
    import test_gpu_slhdsa as tv
    _, rows, _ = slhdsa_rows(name)
    tv.run(ctx.lib, ctx.h, name, rows[::-1])
    for byte in FILLS:
        ctx.fill(byte)
        out = slhdsa_verify_check(ctx, name)
        ctx.fill(byte)
        wide = tv.run(ctx.lib, ctx.h, name, [rows[i % len(rows)] for i in range(65)])
        for key in ("status", "flags", "digest", "fors_pk", "roots"):
            assert np.array_equal(wide[key], out[key][np.arange(65) % len(rows)]), (hex(byte), key)
        ctx.fill(byte)
        one = tv.run(ctx.lib, ctx.h, name, rows[:1])
        tv.check_trace(one, 0, slhdsa_rows(name)[2][0])


@pytest.mark.parametrize("name", SLH_NAMES)
def test_slhdsa_sign_after_fill(ctx, name):
    """Deterministic signatures against the SHA3-256 the fixtures store; no signing in Python."""
    import make_golden_slhdsa as gold
    import make_golden_slhdsa_sign as sgold
    import test_gpu_slhdsa_sign as ts
    f, cases = gold.load()[name], sgold.load()[name]
    msgs = list(f["msgs"]) + [c["msg"] for c in cases]
    want = [r["sig_sha3"] for r in f["records"]] + [c["sig_sha3"] for c in cases]
    ts.keygen(ctx.lib, ctx.h, name, [bytes(len(b"".join(f["seeds"])))])
    ts.sign(ctx.lib, ctx.h, name, [f["sk"]] * len(msgs), msgs[::-1])
    for byte in FILLS:
        ctx.fill(byte)
        pks, sks = ts.keygen(ctx.lib, ctx.h, name, [b"".join(f["seeds"])])
        assert pks == [f["pk"]] and sks == [f["sk"]], hex(byte)
        ctx.fill(byte)
        sigs, status = ts.sign(ctx.lib, ctx.h, name, [f["sk"]] * len(msgs), msgs)
        assert status == [0] * len(msgs)
        assert [hashlib.sha3_256(s).hexdigest() for s in sigs] == want, hex(byte)
        ctx.fill(byte)
        one, status = ts.sign(ctx.lib, ctx.h, name, [f["sk"]], msgs[:1])
        assert status == [0] and hashlib.sha3_256(one[0]).hexdigest() == want[0]


# ------------------------------------------------------------------ AEAD
@pytest.mark.parametrize("alg", aead_spec.ALGS)
def test_aead_batch_after_fill(ctx, alg):
    """The one-lane batch, n = 65, ragged lengths and AADs; every odd row of the Open is tampered."""
    from qrkem.symmetric import BY_NAME
    from test_gpu_aead import ragged_inputs
    c, n = ctx.adopt(BY_NAME[alg](device=0)), 65
    c.long_min_bytes = None  # never the long pair here
    rounds = []
    for seed in (1, 2):
        keys, nonces, pts, aads = ragged_inputs(n, 0xAEAD + seed + len(alg))
        sealed = [aead_spec.seal(alg, k, nn, p, a) for k, nn, p, a in zip(keys, nonces, pts, aads)]
        bad = [s if i % 2 == 0 else s[:-1] + bytes([s[-1] ^ 1 << (i % 8)]) for i, s in enumerate(sealed)]
        rounds.append((keys, nonces, pts, aads, sealed, bad))

    def call(inp, dirty):
        keys, nonces, pts, aads, _, bad = inp
        dirty()
        sealed = c.encrypt_batch(keys, pts, aads, nonces=nonces)
        dirty()
        plain, status = c.decrypt_batch(keys, bad, aads)
        return sealed, plain, status

    warm = ragged_inputs(n, 5)
    warm = warm + ([aead_spec.seal(alg, *r) for r in zip(warm[0], warm[1], warm[2], warm[3])],) * 2
    for byte, inp, (sealed, plain, status) in zip(FILLS, rounds, through_fills(ctx, call, warm, rounds)):
        assert sealed == inp[4], hex(byte)
        for i in range(n):
            assert status[i] == (0 if i % 2 == 0 else -1), (hex(byte), i)
            assert plain[i] == (inp[2][i] if i % 2 == 0 else bytes(len(inp[2][i]))), (hex(byte), i)


@functools.lru_cache(maxsize=None)
def long_records(alg):
    """The fixture's records of 2S + 17, 0 and S - 1 bytes and one longer (3S + 5), above max_len = 2S + 17:
    (keys, nonces, aads, pts, lens, records)."""
    import make_golden_aead_long as gen
    golden = Path(__file__).resolve().parent / "golden"
    recs = {r["pt_len"]: r for r in json.loads((golden / "aead_long.json").read_text())["records"] if r["alg"] == alg}
    lens = [2 * gen.S + 17, 0, gen.S - 1, 3 * gen.S + 5]
    rows = [gen.inputs(alg, recs[l]["record"], l, recs[l]["aad_len"]) for l in lens]
    keys, nonces, aads, pts = (list(x) for x in zip(*rows))
    return keys, nonces, aads, pts, lens, [recs[l] for l in lens]


def long_pair_check(ctx, alg, dirty, what):
    """Seal and Open of the four fixture rows through the long pair.  The reference is the fixture OpenSSL sealed
    (tag, SHA-256 of the ciphertext, its ends) and the inputs themselves; the row above max_len is left at the
    prefill, the tampered row is refused with a zeroed span, and no partial outlives either call."""
    import make_golden_aead_long as gen
    import test_gpu_aead_long as tl
    keys, nonces, aads, pts, lens, recs = long_records(alg)
    max_len = lens[0]
    dirty()
    sealed = tl.split(tl.seal(ctx.h, alg, keys, nonces, pts, aads, max_len), lens, 28)
    assert aead_residue(ctx) == 0, what
    for r, row, nonce, l in zip(recs[:3], sealed, nonces, lens):
        assert row[:12] == nonce and gen.summary(alg, r["record"], l, r["aad_len"], row) == r, (what, l)
    assert sealed[3] == bytes([tl.FILL]) * (lens[3] + 28), what  # above max_len: left unwritten
    # Open: the three rows (now pinned to the fixture), the first once more with one ciphertext bit flipped, and a
    # row of 2S + 18 sealed bytes' worth of payload above max_len
    rows = sealed[:3] + [tl.flip(sealed[0], 12 + gen.S, 3), bytes(lens[0] + 1 + 28)]
    okeys = keys[:3] + [keys[0], keys[3]]
    oaads = aads[:3] + [aads[0], aads[3]]
    olens = lens[:3] + [lens[0], lens[0] + 1]
    dirty()
    plain, status = tl.open_(ctx.h, alg, okeys, rows, oaads, max_len)
    assert status == [0, 0, 0, -1, -1], what
    spans = tl.split(plain, olens, 0)
    assert spans[:3] == pts[:3], what
    assert spans[3] == bytes(lens[0]), what  # refused: zeros over the prefill, no plaintext byte
    assert spans[4] == bytes([tl.FILL]) * olens[4], what  # above max_len: untouched
    assert aead_residue(ctx) == 0, what


@pytest.mark.parametrize("alg", aead_spec.ALGS)
def test_aead_long_pair_after_fill(ctx, alg):
    import test_gpu_aead_long as tl
    keys, nonces, pts, aads, lens = tl.four_rows(alg)
    tl.seal(ctx.h, alg, keys, nonces, pts, aads, lens[0])  # warm-up on other bytes of the same shape
    for byte in FILLS:
        long_pair_check(ctx, alg, functools.partial(ctx.fill, byte), (alg, hex(byte)))


@pytest.mark.parametrize("alg", aead_spec.ALGS)
def test_aead_long_mac_hooks_after_fill(ctx, alg):
    import test_gpu_aead_long as tl
    gcm = alg == "AES-256-GCM"
    name = "qrk_dbg_ghash_long_batch" if gcm else "qrk_dbg_poly1305_long_batch"
    spec = aead_spec.ghash if gcm else aead_spec.poly1305
    key = bytes(range(1, 17)) if gcm else bytes(range(3, 19)) + bytes(range(16))
    tl.run_hook(ctx.h, name, key, tl.mac_rows(3), 3 * tl.S)
    for byte in FILLS:
        rows = tl.mac_rows(10 + byte)
        ctx.fill(byte)
        got = tl.run_hook(ctx.h, name, key, rows, max(map(len, rows)))
        assert got == [spec(key, r) for r in rows], hex(byte)
        assert aead_residue(ctx) == 0


# ------------------------------------------------------------------ the handshake driver
@pytest.mark.parametrize("alg", ["ML-KEM-768", "FrodoKEM-640-SHAKE", "HQC-128"])
def test_handshake_driver_after_fill(ctx, alg):
    """n = 65 through qrk_handshake_batch (hs_scratch and the scratch) and the key confirmation, against the
    oracle's handshake and aead_spec."""
    import hkdf_spec
    from make_golden_handshake import node_id
    from qrkem.handshake import HandshakeDriver
    sym, n = "AES-256-GCM", 65
    drv = HandshakeDriver(alg, symmetric_name=sym)
    ctx.adopt(drv.engine)
    s = orc.sizes(alg)
    kp, enc = s["keypair_coins"], s["encaps_coins"]
    infos = [hkdf_spec.protocol_info(node_id(b"a", i), node_id(b"b", i), sym) for i in range(n)]
    msgs = [b"key confirmation %d" % i + bytes(i % 7) for i in range(n)]
    rounds = []
    for seed in (0, 1, 2):
        coins = orc.bench_coins(n, 2 * kp + enc, seed=0xA11 + kp + seed)
        cs = [np.ascontiguousarray(coins[:, a:b]) for a, b in ((0, kp), (kp, 2 * kp), (2 * kp, 2 * kp + enc))]
        rounds.append((cs, np.random.default_rng(seed).integers(0, 256, (n, 12), dtype=np.uint8)))

    def call(inp, dirty):
        (kpi, kpr, en), nonces = inp
        dirty()
        out = drv.run(infos, coins_kp_initiator=kpi, coins_kp_responder=kpr, coins_encaps=en)
        torch.cuda.synchronize()
        dirty()
        sealed, ok = drv.confirm(out, msgs, nonces=nonces)
        return out, sealed, host(ok)

    for byte, inp, (out, sealed, ok) in zip(FILLS, rounds[1:], through_fills(ctx, call, rounds[0], rounds[1:])):
        want = orc.batch_handshake(alg, *inp[0], infos, hkdf_spec.SYMMETRIC_KEY_SIZE[sym], 8)
        got = (out.pk_initiator, out.pk_responder, out.ciphertext, out.key_initiator, out.key_responder)
        for what, g, w in zip(("pk_i", "pk_r", "ct", "key_i", "key_r"), got, want):
            assert np.array_equal(host(g), w), (alg, hex(byte), what)
        assert host(out.agree).tolist() == [1] * n and ok.tolist() == [1] * n
        assert sealed == [aead_spec.seal(sym, want[3][i].tobytes(), inp[1][i].tobytes(), msgs[i]) for i in range(n)]


# ------------------------------------------------------------------ one context, every family, no fill
def test_every_family_in_the_scratch_another_laid_out(ctx):
    """FrodoKEM-1344 (65), HQC-256, ML-KEM-768, a long AEAD seal / open, ML-DSA-87 verify, SLH-DSA verify,
    FrodoKEM-640 and ML-KEM-512 on one context, each against its reference, then the same in reverse order: what
    a family finds in the scratch is what the family before it left, at that family's offsets."""
    def kem_step(alg, n):
        eng, r = ctx.kem(alg), kem_ref(alg, n, 0x5EC + n)
        return lambda: kem_check(r, kem_call(eng, r, lambda: None), alg)

    steps = [kem_step("FrodoKEM-1344-SHAKE", 65), kem_step("HQC-256", 65), kem_step("ML-KEM-768", SMALL_MAX + 1),
             lambda: long_pair_check(ctx, "AES-256-GCM", lambda: None, "shared"),
             lambda: mldsa_verify_check(ctx, "ML-DSA-87"),
             lambda: slhdsa_verify_check(ctx, "SLH-DSA-SHA2-128f"),
             kem_step("FrodoKEM-640-AES", 65), kem_step("ML-KEM-512", SMALL_MAX + 1)]
    for step in steps + steps[::-1]:
        step()
