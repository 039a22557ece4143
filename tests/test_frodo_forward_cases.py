"""CPU: the reference side of tests/test_gpu_frodo_forward.py, before the GPU is compared with it.

(a) frodo_spec's factored functions (keygen_from_samples, encrypt_from_samples) reproduce keypair_derand and
    encaps_derand, which the C oracle and the NIST KATs pin, on honest inputs;
(b) on the crafted public and secret keys the C oracle and frodo_spec agree byte for byte;
(c) every sampler boundary word maps, under frodo_spec.sample, to the value its table states, both signs;
and tests/golden/frodo_forward.json regenerates identically from tests/frodo_forward_cases.py.
"""
import hashlib

import numpy as np
import pytest

import frodo_forward_cases as W
import frodo_spec as F
import make_golden_frodo_edge as E
import make_golden_frodo_forward as G
import oracle as orc

NBAR = F.NBAR
FAST = [a for a in W.ALGS if a.endswith("SHAKE")]


@pytest.fixture(autouse=True)
def memo_gen_a():
    with W.memo_gen_a():
        yield


# ---------------------------------------------------------------- (a) the factored spec functions
@pytest.mark.parametrize("alg", FAST + ["FrodoKEM-640-AES"])
def test_factored_functions_reproduce_the_derand_calls(alg):
    p = F.params(alg)
    n, sec = p["n"], p["sec"]
    coins = W.derive(alg, b"a coins", p["keypair_coins"])
    pk, sk = F.keypair_derand(alg, coins)
    assert (pk, sk) == orc.keypair(alg, coins)
    r = np.frombuffer(F._shake(p, b"\x5f" + coins[sec:2 * sec], 4 * n * NBAR), "<u2")
    St, Em = F.sample(p, r[:n * NBAR]).reshape(NBAR, n), F.sample(p, r[n * NBAR:]).reshape(n, NBAR)
    assert F.keygen_from_samples(p, pk[:16], St, Em) == pk
    assert F.keygen_from_samples(p, pk[:16], E.signed(St), E.signed(Em)) == pk  # signed or two's complement alike
    mu = W.derive(alg, b"a mu", p["len_mu"])
    ct, ss = F.encaps_derand(alg, pk, mu)
    assert (ct, ss) == orc.encaps(alg, pk, mu)
    seed_se = F._shake(p, F._shake(p, pk, sec) + mu, 2 * sec)[:sec]
    r = np.frombuffer(F._shake(p, b"\x96" + seed_se, (2 * n + NBAR) * NBAR * 2), "<u2")
    Sp, Ep, Epp = (E.signed(F.sample(p, x)) for x in (r[:n * NBAR], r[n * NBAR:2 * n * NBAR], r[2 * n * NBAR:]))
    Bp, C = F.encrypt_from_samples(p, pk, Sp.reshape(NBAR, n), Ep.reshape(NBAR, n), Epp.reshape(NBAR, NBAR), mu)
    assert F.pack(Bp, p["logq"]) + F.pack(C, p["logq"]) == ct
    assert F.decaps(alg, sk, ct) == ss


def test_case_list_covers_every_pairing():
    """Every matrix kind with every E kind, one-hot included, and both mu kinds with every matrix kind family."""
    for n in (640, 976, 1344):
        cases = W.case_list(n)
        assert len(cases) == 39 and len({W.case_name(c) for c in cases}) == 39
        kind = lambda c: c[0] if isinstance(c[0], str) else "onehot"  # noqa: E731
        pairs = {(kind(c), c[1]) for c in cases}
        for m in W.MATRIX_KINDS + ("onehot",):
            for e in W.E_KINDS:
                assert (m, e) in pairs
            assert {c[2] for c in cases if kind(c) == m} >= set(W.MU_KINDS), m
        hot = [c[0] for c in cases if kind(c) == "onehot"]
        assert [(h[1], h[2]) for h in hot] == W.onehot_positions(n)
        for j in {h[2] for h in hot}:
            assert {h[3] for h in hot if h[2] == j} == {1, -1}
        assert cases[0][:2] == ("+max", "+max") and cases[1][:2] == ("+max", "-max")
        assert cases[3][:2] == ("-max", "+max") and cases[4][:2] == ("-max", "-max")


@pytest.mark.parametrize("alg", W.ALGS)
def test_from_samples_inputs_are_in_range_and_extreme(alg):
    p = F.params(alg)
    m, n = W.smax(p), p["n"]
    for kg in (False, True):
        inp = W.from_samples_inputs(alg, kg)
        assert not inp["s8"][:, :, n:].any() and np.abs(inp["s8"]).max() == m == np.abs(inp["e16"]).max()
        i = inp["names"].index("S +max | E +max | mu 00")
        assert (inp["s8"][i, :, :n] == m).all() and (inp["e16"][i] == m).all()


# ---------------------------------------------------------------- the fixture
@pytest.fixture(scope="module")
def regenerated():
    with W.memo_gen_a():
        return {alg: G.generate(alg) for alg in W.ALGS}


def test_fixture_regenerates_identically(regenerated):
    assert G.load() == regenerated
    assert G.PATH.read_text() == G.dumps(regenerated)
    assert G.PATH.stat().st_size < 1 << 20


def test_all_zero_samples_leave_the_noise_alone(regenerated):
    """S' = 0: ct is Pack(E') || Pack(E'' + Encode(mu)), no A in it -- the same for the SHAKE and the AES name."""
    for n in (640, 976, 1344):
        for e in W.E_KINDS:
            name = f"S zero | E {e} | mu {dict(zip(W.E_KINDS, ('00', 'FF', '00')))[e]}"
            a, b = (regenerated[f"FrodoKEM-{n}-{prg}"]["encaps"] for prg in ("SHAKE", "AES"))
            p = F.params(f"FrodoKEM-{n}-AES")
            inp = W.from_samples_inputs(f"FrodoKEM-{n}-AES", False)
            i = inp["names"].index(name)
            q = 1 << p["logq"]
            want = F.pack(inp["e16"][i].astype(np.int64) % q, p["logq"]) + \
                F.pack((inp["epp16"][i].astype(np.int64).reshape(8, 8) + F.encode(p, inp["mu"][i].tobytes())) % q, p["logq"])
            assert b[name] == hashlib.sha256(want).hexdigest()
            assert a[name] == b[name]


# ---------------------------------------------------------------- (b) crafted keys: the C oracle against the spec
@pytest.mark.parametrize("alg", W.ALGS)
def test_c_oracle_and_spec_agree_on_the_crafted_public_keys(alg):
    r = W.encaps_rows(alg)
    names, B = W.crafted_b(alg)
    p = F.params(alg)
    assert len(names) == 10 and r["names"][0::2] == ["B " + x for x in names]
    assert np.array_equal(E.unpack_rows(r["pk"][0::2, 16:], p["logq"]), B.reshape(len(names), -1))
    ct, ss = orc.batch_encaps(alg, r["pk"], r["mu"])
    for i in range(0, len(r["names"]), 2):  # the crafted rows share the name's seedA: one Gen(A)
        assert F.encaps_derand(alg, r["pk"][i].tobytes(), r["mu"][i].tobytes()) == (ct[i].tobytes(), ss[i].tobytes()), \
            r["names"][i]
    if alg in FAST:  # the honest rows have a seedA each
        for i in (1, len(r["names"]) - 1):
            assert F.encaps_derand(alg, r["pk"][i].tobytes(), r["mu"][i].tobytes()) == (ct[i].tobytes(), ss[i].tobytes())


@pytest.mark.parametrize("alg", W.ALGS)
def test_c_oracle_and_spec_agree_on_the_crafted_secret_keys(alg):
    """Every row under a crafted pk (the honest-pk rows too where Gen(A) is cheap): frodo_spec.decaps is the oracle's
    ss; rows with a replaced ciphertext field reject, ss = H(ct || s); the honest pair's row accepts."""
    p = F.params(alg)
    r = W.decaps_rows(alg)
    ss, st = orc.batch_decaps(alg, r["sk"], r["ct"], with_status=True)
    assert not st.any() and len(r["names"]) == 1 + 10 + 4 * 9 - 1
    honest_pk = len(W.crafted_b(alg)[0])
    checked = 0
    for i, (ip, skind, b, c) in enumerate(r["plan"]):
        tampered = b != "honest" or c != "honest"
        if tampered:
            assert ss[i].tobytes() == E.shake(p, r["ct"][i].tobytes() + r["sk"][i, :p["sec"]].tobytes(), p["sec"]), r["names"][i]
        if ip == honest_pk and alg not in FAST:
            continue
        assert F.decaps(alg, r["sk"][i].tobytes(), r["ct"][i].tobytes()) == ss[i].tobytes(), r["names"][i]
        checked += 1
    assert checked >= len(r["plan"]) - 5
    assert ss[0].tobytes() == r["ss_enc"][0].tobytes()
    for kind in W.ST_KINDS:
        assert sum(t[1] == kind for t in r["plan"]) >= 8


# ---------------------------------------------------------------- (c) the boundary table
@pytest.mark.parametrize("n", [640, 976, 1344])
def test_boundary_words_map_to_the_stated_samples(n):
    p = F.params(f"FrodoKEM-{n}-SHAKE")
    table = W.boundary_table(p)
    m = W.smax(p)
    assert len(table) == 4 * m + 4
    words = np.array([w for w, _, _ in table], np.uint16)
    got = E.signed(F.sample(p, words))
    assert got.tolist() == [v for _, v, _ in table]
    # both signs of every magnitude 0..max, and each table entry from both sides
    assert {v for _, v, _ in table} == set(range(-m, m + 1))
    for j, t in enumerate(p["cdf"][:-1]):
        assert E.signed(F.sample(p, np.array([2 * t, 2 * t + 1, 2 * t + 2, 2 * t + 3], np.uint16))).tolist() == [j, -j, j + 1, -j - 1]
    # the streams place each word where the region table says, alone
    for kg in (False, True):
        words, meta = W.boundary_streams(p, kg)
        assert len(meta) == len(table) * (4 if kg else 6) and words.shape[1] == W.words_per_row(p, kg)
        assert (np.count_nonzero(words, axis=1) <= 1).all()
        s8, e16, epp = W.sampler_expected(p, kg, words[:8])
        assert not s8[:, :, n:].any()


def test_every_word_rows_hold_every_word():
    for n in (640, 976, 1344):
        p = F.params(f"FrodoKEM-{n}-SHAKE")
        for kg in (False, True):
            a, b = W.every_word_rows(p, kg, False), W.every_word_rows(p, kg, True)
            assert a.shape == b.shape and not np.array_equal(a, b)
            for x in (a, b):
                assert len(np.unique(x)) == 1 << 16
            assert np.array_equal(a.ravel()[:1 << 16], np.arange(1 << 16))


def test_hooks_are_exported_undeclared_and_check_their_arguments_first():
    """As qrk_dbg_frodo_decaps_trace: exported, kept out of the public header; an unknown name, a name of another
    family, a null context and null buffers are refused before any device work."""
    import ctypes as ct

    import qrkem
    from qrkem._debug import bind
    from test_abi import declared_functions, exported_symbols
    lib = bind()
    ctx = ct.c_void_p(1)  # never dereferenced: the name and the buffers are checked first
    for name, nargs in (("qrk_dbg_frodo_sample", 5), ("qrk_dbg_frodo_from_samples", 8)):
        assert name in exported_symbols() and name not in declared_functions()
        fn = getattr(lib, name)
        nulls = [None] * nargs
        for alg, msg in ((b"ML-KEM-768", "not a FrodoKEM parameter set"), (b"HQC-128", "not a FrodoKEM parameter set"),
                         (b"FrodoKEM-640", "unsupported KEM")):
            assert fn(ctx, alg, 0, 1, *nulls) == -1
            assert msg in qrkem.last_error()
        assert fn(None, b"FrodoKEM-640-SHAKE", 0, 1, *nulls) == -1
        assert "null context" in qrkem.last_error()
        for kg in (0, 1):
            assert fn(ctx, b"FrodoKEM-640-SHAKE", kg, 1, *nulls) == -1
            assert "null buffer" in qrkem.last_error()
