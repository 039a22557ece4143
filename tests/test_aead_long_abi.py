"""CPU: the long AEAD calls (one row across many workgroups) are exported, declared and bound, their layout is
the one tests/golden/aead_long.json was generated for, they check their arguments in the documented order
before any device work, and the fixture itself agrees with tests/aead_spec.py where the pure-Python spec is
quick enough (records of at most 64 KiB: 0.16 s per 16 KiB of GCM)."""
import ctypes as ct
import hashlib
import json

import pytest

import aead_spec
import make_golden_aead_long as gen
from test_abi import declared_functions, exported_symbols
from test_debug_abi import DEBUG_HEADER

ALGS = aead_spec.ALGS
CALLS = {"qrk_aead_long_layout": 2, "qrk_aead_seal_long_batch": 13, "qrk_aead_open_long_batch": 13}
HOOKS = {"qrk_dbg_ghash_long_batch": 8, "qrk_dbg_poly1305_long_batch": 8, "qrk_dbg_aead_long_residue": 2}


@pytest.fixture(scope="module")
def golden(golden_dir):
    return json.loads((golden_dir / "aead_long.json").read_text())


def test_symbols_exported_declared_and_bound():
    """The calls are in the public header and its binding table, their three test hooks in the hook header and
    its table (and in no other), and all six in the library."""
    from qrkem import _debug
    from qrkem._native import LIB
    exported = exported_symbols()
    public, hooks = declared_functions(), declared_functions(DEBUG_HEADER)
    assert _debug.bind() is LIB
    for name, nargs in {**CALLS, **HOOKS}.items():
        assert name in exported, name
        assert (name in hooks and name not in public) if name in HOOKS else (name in public and name not in hooks), name
        assert (name in _debug.HOOKS) == (name in HOOKS), name
        fn = getattr(LIB, name)
        assert fn.restype is ct.c_int and fn.argtypes is not None and len(fn.argtypes) == nargs, name


@pytest.mark.parametrize("alg", ALGS)
def test_layout_is_the_generators(golden, alg):
    from qrkem._native import LIB
    out = (ct.c_size_t * 4)()
    assert LIB.qrk_aead_long_layout(alg.encode(), out) == 0
    s, c, fan_in, per_segment = out
    assert (s, c, fan_in) == (gen.S, gen.C, gen.F) == (golden["S"], golden["C"], golden["F"])
    assert s == 256 * c and c % 64 == 0
    assert per_segment == {"AES-256-GCM": 16, "ChaCha20-Poly1305": 32}[alg]


def test_layout_refuses_unknown_names_and_null():
    import qrkem
    from qrkem._native import LIB
    out = (ct.c_size_t * 4)()
    assert LIB.qrk_aead_long_layout(b"AES-128-GCM", out) == -1 and "unsupported AEAD" in qrkem.last_error()
    assert LIB.qrk_aead_long_layout(b"AES-256-GCM", None) == -1 and "null argument" in qrkem.last_error()


def seal(LIB, ctx, alg, n, bufs, aad, aad_off, aad_len, max_len):
    k, p = (ct.c_void_p(1) if bufs else None), (ct.c_void_p(1) if aad else None)
    return LIB.qrk_aead_seal_long_batch(ctx, alg, n, k, None, k, k, p, ct.c_void_p(1) if aad_off else None, aad_len,
                                        max_len, k, None)


def open_(LIB, ctx, alg, n, bufs, aad, aad_off, aad_len, max_len):
    k, p = (ct.c_void_p(1) if bufs else None), (ct.c_void_p(1) if aad else None)
    return LIB.qrk_aead_open_long_batch(ctx, alg, n, k, k, k, p, ct.c_void_p(1) if aad_off else None, aad_len,
                                        max_len, k, k, None)


@pytest.mark.parametrize("call", [seal, open_], ids=["seal", "open"])
def test_argument_checks_in_the_documented_order_without_a_device(call):
    """ctx, alg, n == 0, NULL buffers, aad_len, max_len, the grid, the scratch budget: each check fails with
    every later one also wrong, so the order is what the header says.  No pointer here is ever dereferenced
    (ctx = 1 is not a context): every refusal comes before any device work."""
    import qrkem
    from qrkem._native import LIB
    ctx, gcm, bad = ct.c_void_p(1), b"AES-256-GCM", 1 << 31
    assert call(LIB, None, b"nope", 1, False, False, True, bad, 0) == -1 and "null context" in qrkem.last_error()
    assert call(LIB, ctx, b"nope", 1, False, False, True, bad, 0) == -1 and "unsupported AEAD" in qrkem.last_error()
    for alg in (b"AES-256-GCM", b"ChaCha20-Poly1305"):
        assert call(LIB, ctx, alg, 0, False, False, True, bad, 0) == 0  # n == 0 returns 0 before anything else
    assert call(LIB, ctx, gcm, 1, False, True, False, bad, 0) == -1 and "null buffer" in qrkem.last_error()
    assert call(LIB, ctx, gcm, 1, True, False, True, 0, 0) == -1 and "null buffer" in qrkem.last_error()  # aad_off, no aad
    assert call(LIB, ctx, gcm, 1, True, False, False, 5, 0) == -1 and "null buffer" in qrkem.last_error()  # aad_len, no aad
    assert call(LIB, ctx, gcm, 1, True, True, False, bad, 0) == -1 and "aad_len must be below 2^31" in qrkem.last_error()
    for max_len in (0, 1 << 31, 1 << 40):
        assert call(LIB, ctx, gcm, 1, True, True, False, 0, max_len) == -1
        assert "max_len must be at least 1 and below 2^31" in qrkem.last_error()
    # 2^31 - 1 bytes are 2^15 segments: 2^16 such rows are 2^31 workgroups
    assert call(LIB, ctx, gcm, 1 << 16, True, True, False, 0, bad - 1) == -1 and "2^31 workgroups" in qrkem.last_error()
    # 2^15 segments of 32 bytes and a verdict word per row: 49153 ChaCha20-Poly1305 rows pass 48 GiB
    assert call(LIB, ctx, b"ChaCha20-Poly1305", 49153, True, True, False, 0, bad - 1) == -1
    assert "scratch budget" in qrkem.last_error()


def test_hooks_check_their_arguments_without_a_device():
    import qrkem
    from qrkem._debug import bind
    LIB = bind()
    one = ct.c_void_p(1)
    for fn in (LIB.qrk_dbg_ghash_long_batch, LIB.qrk_dbg_poly1305_long_batch):
        assert fn(None, 1, one, one, one, 16, one, None) == -1 and "null context" in qrkem.last_error()
        assert fn(one, 0, None, None, None, 0, None, None) == 0
        assert fn(one, 1, one, None, one, 16, one, None) == -1 and "null buffer" in qrkem.last_error()
        assert fn(one, 1, one, one, one, 0, one, None) == -1 and "max_len" in qrkem.last_error()
    assert LIB.qrk_dbg_aead_long_residue(None, None) == -1 and "null argument" in qrkem.last_error()


def test_fixture_plan_covers_the_geometry(golden):
    """The generator's lengths are the issue's list over this S and C, the aad lengths cycle, and the extra
    record gives the tail a two-partial lane walk with a ragged lane: F + 1 segments, the short one ragged."""
    s, c, f = gen.S, gen.C, gen.F
    assert gen.PT_LENS == (0, 1, 15, 16, 17, c - 1, c, c + 1, s - 16, s - 1, s, s + 1, s + c + 1, 2 * s - 1, 2 * s,
                           2 * s + 17, 3 * s + 5)
    assert gen.AAD_LENS == (0, 1, 13, 16, 100)
    assert -(-gen.TREE_LEN // s) == f + 1 and gen.TREE_LEN % 16 and gen.TREE_LEN <= 8 << 20
    recs = golden["records"]
    assert len(recs) == len(ALGS) * (len(gen.PT_LENS) + 1)
    for alg in ALGS:
        mine = [r for r in recs if r["alg"] == alg]
        assert [(r["pt_len"], r["aad_len"]) for r in mine] == gen.plan()
        assert [r["record"] for r in mine] == list(range(len(mine)))
        assert {r["aad_len"] for r in mine} == set(gen.AAD_LENS)


SMALL = [(alg, j) for alg in ALGS for j, (pt_len, _) in enumerate(gen.plan()) if pt_len <= 64 << 10]


@pytest.mark.parametrize("alg,record", SMALL)
def test_spec_reproduces_the_fixture(golden, alg, record):
    rec = next(r for r in golden["records"] if r["alg"] == alg and r["record"] == record)
    key, nonce, aad, pt = gen.inputs(alg, record, rec["pt_len"], rec["aad_len"])
    sealed = aead_spec.seal(alg, key, nonce, pt, aad)
    assert sealed[:12] == nonce
    assert gen.summary(alg, record, rec["pt_len"], rec["aad_len"], sealed) == rec
    assert hashlib.sha256(sealed[12:-16]).hexdigest() == rec["ct_sha256"]
