"""GPU: Decaps of keys made on the same context reuses KeyGen's sampled matrix, and never shows it.

A batched ML-KEM KeyGen keeps A_hat = SampleNTT(rho) and a 32-byte rho tag per row in the context (the kept
region, csrc/qrkem_internal.h); a Decaps chunk of the same geometry compares each row's rho with its tag on the
device (k_rho_match) and samples only the rows that miss.  Outputs never depend on the region, only time does: every
check here is byte-exact against oracle.batch_decaps(..., with_status=True), whatever the rows hit.

The signal for "reused" is the launch names of the profile hooks: a Decaps chunk under a valid region runs
k_rho_match and names its SampleNTT role k_xof_miss (its lanes return where their row hit); any other batched
Decaps chunk names it k_xof.  Hits are decided per aligned quad of rows (one wave of the re-encryption core), so a
row beside a missing one is sampled with it.

Shapes: n = 1100 at the default chunk (one batched chunk of 1152 rows, just above the one-launch kernels' 1024 and
no multiple of 64), all three parameter sets; n = 3000 at chunk 2048, ML-KEM-768 (the batch driver splits a call
into equal chunks, so this is 1536 + 1464 rows, both batched and both kept; the 2048 + 952 split, whose short chunk
runs the one-launch kernels and is never kept, is the handshake driver's, in its own reuse test and here with the
cap at 0).
"""
import functools

import numpy as np
import pytest

import oracle as orc

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SHAPES = [("ML-KEM-512", 1100, None), ("ML-KEM-768", 1100, None), ("ML-KEM-1024", 1100, None),
          ("ML-KEM-768", 3000, 2048)]
OTHER = {"ML-KEM-512": "ML-KEM-768", "ML-KEM-768": "ML-KEM-1024", "ML-KEM-1024": "ML-KEM-512"}


@functools.lru_cache(maxsize=None)
def keys(alg, n, seed):
    """(KeyGen coins, pk, sk, ct, ss) of n oracle handshakes; computed once per (alg, n, seed), never modified."""
    return _keys(alg, n, seed)[:1] + _keys(alg, n, seed)[2:]


@functools.lru_cache(maxsize=None)
def _keys(alg, n, seed):
    """... with the Encaps coins: (KeyGen coins, Encaps coins, pk, sk, ct, ss)."""
    coins = orc.bench_coins(n, 96, seed=seed)
    kc, ec = np.ascontiguousarray(coins[:, :64]), np.ascontiguousarray(coins[:, 64:])
    pk, sk = orc.batch_keypair(alg, kc)
    c, ss = orc.batch_encaps(alg, pk, ec)
    out = (kc, ec, pk, sk, c, ss)
    for a in out:
        a.setflags(write=False)
    return out


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def engine(alg, chunk=None, ctx_of=None):
    """A BatchKEM; with ctx_of, one for another parameter set on ctx_of's context."""
    from qrkem.batch import BatchKEM
    eng = BatchKEM(alg, device=0, chunk=chunk)
    if ctx_of is not None:
        eng.close()
        eng._ctx = ctx_of._ctx
        eng.close = lambda: None
    return eng


def keygen(eng, alg, n, seed):
    """KeyGen of the oracle's keys on eng's context: the device sk, checked against the oracle's."""
    kc, pk, sk, _, _ = keys(alg, n, seed)
    dpk, dsk = eng.keypair(coins=dev(kc))
    assert np.array_equal(host(dpk), pk) and np.array_equal(host(dsk), sk)
    return dsk


def roles(eng, call):
    """The result of call() and the kernel names (roles of multi-role launches apart) it launched."""
    eng.profile(True)
    out = call()
    torch.cuda.synchronize()
    prof = eng.profile_read()
    eng.profile(False)
    return out, [r for name in prof for r in name.split("+")], prof


def decaps_checked(eng, alg, sk, c, reused):
    """Decaps of (sk, c) rows on the device: byte-exact against the oracle; `reused` (True / False / None: either)
    is what the launch names must say about every batched chunk."""
    sk, c = np.ascontiguousarray(sk), np.ascontiguousarray(c)
    want, want_status = orc.batch_decaps(alg, sk, c, with_status=True)
    (ss, status), names, prof = roles(eng, lambda: eng.decaps(dev(sk), dev(c), return_status=True))
    assert np.array_equal(host(ss), want)
    assert np.array_equal(host(status), want_status)
    if reused is True:
        assert "k_xof_miss" in names and "k_rho_match" in names and "k_xof" not in names, prof
    elif reused is False:
        assert "k_xof" in names and "k_xof_miss" not in names and "k_rho_match" not in names, prof
    return prof


@pytest.fixture(autouse=True)
def default_cap(monkeypatch):
    monkeypatch.delenv("QRK_KEEP_MIB", raising=False)


# ------------------------------------------------------------------ 1. aligned reuse
@pytest.mark.parametrize("alg,n,chunk", SHAPES)
def test_aligned_reuse_skips_sampling(alg, n, chunk):
    _, pk, sk, c, ss = keys(alg, n, 0xA1)
    eng = engine(alg, chunk)
    dsk = keygen(eng, alg, n, 0xA1)
    dct, dss = eng.encaps(dev(pk), coins=dev(_keys(alg, n, 0xA1)[1]))
    assert np.array_equal(host(dct), c) and np.array_equal(host(dss), ss)
    out, names, prof = roles(eng, lambda: eng.decaps(dsk, dct))
    assert np.array_equal(host(out), ss)
    assert "k_xof_miss" in names and "k_rho_match" in names and "k_xof" not in names, prof
    nchunks = 1 if chunk is None else -(-n // chunk)
    assert prof["k_rho_match"][1] == nchunks  # every chunk of the call was kept
    # Encaps never reuses (the other party's matrix), and a context with no KeyGen samples
    _, names, prof = roles(eng, lambda: eng.encaps(dev(pk)))
    assert "k_xof" in names and "k_xof_miss" not in names, prof
    decaps_checked(engine(alg, chunk), alg, sk, c, reused=False)
    # the serial schedule (one kernel per launch) takes the same path
    eng.set_streams(1)
    decaps_checked(eng, alg, sk, c, reused=True)


# ------------------------------------------------------------------ 2. all rows miss
@pytest.mark.parametrize("alg,n,chunk", SHAPES)
def test_all_rows_miss(alg, n, chunk):
    _, _, sk, c, _ = keys(alg, n, 0xA1)
    eng = engine(alg, chunk)
    keygen(eng, alg, n, 0xA1)
    decaps_checked(eng, alg, sk[::-1], c[::-1], reused=True)  # every rho beside another row's tag
    other = engine(alg, chunk)
    dsk2 = keygen(other, alg, n, 0xB2)                        # keys of a second context
    _, _, sk2, c2, ss2 = keys(alg, n, 0xB2)
    assert np.array_equal(host(eng.decaps(dsk2, dev(c2))), ss2)
    decaps_checked(eng, alg, sk2, c2, reused=True)
    decaps_checked(eng, alg, sk, c, reused=True)              # and the region still serves its own keys


# ------------------------------------------------------------------ 3. mixed wave
@pytest.mark.parametrize("alg,n,chunk", SHAPES)
def test_mixed_hits_and_misses_in_one_tile(alg, n, chunk):
    _, _, sk, c, _ = keys(alg, n, 0xA1)
    _, _, sk2, c2, _ = keys(alg, n, 0xB2)
    sk, c = np.array(sk), np.array(c)
    sk[[5, 9]], c[[5, 9]] = sk[[9, 5]], c[[9, 5]]  # two rows of the first 64-row tile swapped
    sk[70], c[70] = sk2[70], c2[70]                # one row's dk from another KeyGen
    sk[n - 1], c[n - 1] = sk2[3], c2[3]            # and the last row of the ragged last tile
    eng = engine(alg, chunk)
    keygen(eng, alg, n, 0xA1)
    decaps_checked(eng, alg, sk, c, reused=True)


# ------------------------------------------------------------------ 4. invalidation
@pytest.mark.parametrize("byte", [0xFF, 0x00])
@pytest.mark.parametrize("alg,n,chunk", SHAPES)
def test_context_fill_invalidates(alg, n, chunk, byte):
    from qrkem._debug import bind
    _, _, sk, c, _ = keys(alg, n, 0xA1)
    eng = engine(alg, chunk)
    keygen(eng, alg, n, 0xA1)
    assert bind().qrk_dbg_ctx_fill(eng._ctx, byte) == 0
    decaps_checked(eng, alg, sk, c, reused=False)  # the filled region is never read
    keygen(eng, alg, n, 0xA1)
    decaps_checked(eng, alg, sk, c, reused=True)   # and the next KeyGen makes it valid again


@pytest.mark.parametrize("alg,n,chunk", SHAPES)
def test_keygen_of_another_parameter_set_invalidates(alg, n, chunk):
    _, _, sk, c, _ = keys(alg, n, 0xA1)
    eng = engine(alg, chunk)
    keygen(eng, alg, n, 0xA1)
    keygen(engine(OTHER[alg], ctx_of=eng), OTHER[alg], n, 0xC3)
    decaps_checked(eng, alg, sk, c, reused=False)


@pytest.mark.parametrize("alg,n,chunk", SHAPES)
def test_keygen_with_another_chunk_size_invalidates(alg, n, chunk):
    from qrkem._native import LIB
    _, _, sk, c, _ = keys(alg, n, 0xA1)
    eng = engine(alg, chunk)
    keygen(eng, alg, n, 0xA1)
    # 1100 rows: one chunk of 1152 before, two one-launch chunks of 576 after (nothing kept, nothing reused);
    # 3000 rows: 1536 + 1464 before, one chunk of 3008 after (kept: the first keys' Decaps at that chunk size
    # finds the second keys' tags and misses everywhere)
    assert LIB.qrk_ctx_set_chunk(eng._ctx, 4096 if chunk else 1088) == 0
    keygen(eng, alg, n, 0xB2)
    decaps_checked(eng, alg, sk, c, reused=None)
    assert LIB.qrk_ctx_set_chunk(eng._ctx, chunk or (1 << 20)) == 0
    decaps_checked(eng, alg, sk, c, reused=None)


@pytest.mark.parametrize("alg,n,chunk", SHAPES)
def test_keygen_of_fewer_rows_leaves_no_stale_tags(alg, n, chunk):
    """A second KeyGen of n - 8 rows (the same 64-row tiles): the rows beyond it still hold the first KeyGen's
    tags and entries, and must not hit.  Decaps of the second KeyGen's keys followed by the first's last rows."""
    _, _, sk, c, _ = keys(alg, n, 0xA1)
    _, _, sk2, c2, _ = keys(alg, n, 0xB2)
    eng = engine(alg, chunk)
    keygen(eng, alg, n, 0xA1)
    few = n - 8
    kc2 = keys(alg, n, 0xB2)[0][:few]
    _, dsk2 = eng.keypair(coins=dev(kc2))
    assert np.array_equal(host(dsk2), sk2[:few])
    mixed_sk, mixed_c = np.concatenate([sk2[:few], sk[few:]]), np.concatenate([c2[:few], c[few:]])
    decaps_checked(eng, alg, mixed_sk, mixed_c, reused=None)
    decaps_checked(eng, alg, sk, c, reused=None)
    decaps_checked(eng, alg, sk2[:few], c2[:few], reused=True)


@pytest.mark.parametrize("alg,n,chunk", SHAPES)
def test_keys_overwritten_in_place(alg, n, chunk):
    """The caller's sk tensor, the very buffer KeyGen wrote, overwritten with other keys at the same address."""
    _, _, _, c, ss = keys(alg, n, 0xA1)
    _, _, sk2, c2, ss2 = keys(alg, n, 0xB2)
    eng = engine(alg, chunk)
    dsk = keygen(eng, alg, n, 0xA1)
    assert np.array_equal(host(eng.decaps(dsk, dev(c))), ss)
    ptr = dsk.data_ptr()
    dsk.copy_(dev(sk2))
    assert dsk.data_ptr() == ptr
    out, names, prof = roles(eng, lambda: eng.decaps(dsk, dev(c2)))
    assert np.array_equal(host(out), ss2)
    assert "k_xof_miss" in names, prof


# ------------------------------------------------------------------ 5. implicit rejection
@pytest.mark.parametrize("alg,n,chunk", SHAPES)
def test_implicit_rejection_under_reuse(alg, n, chunk):
    _, _, sk, c, ss = keys(alg, n, 0xA1)
    eng = engine(alg, chunk)
    keygen(eng, alg, n, 0xA1)
    dct = dev(c)
    eng.tamper(dct, 0x7A, 2)  # Bernoulli(1/2) per row
    bad = host(dct)
    tampered = (bad != c).any(axis=1)
    assert 0 < tampered.sum() < n
    decaps_checked(eng, alg, sk, bad, reused=True)  # ss on valid rows, J(z || c) on tampered ones, status as the oracle
    want = orc.batch_decaps(alg, np.ascontiguousarray(sk), bad, with_status=True)[0]
    assert np.array_equal((want == ss).all(axis=1), ~tampered)


# ------------------------------------------------------------------ 6. budget
@pytest.mark.parametrize("mib", ["0", "1"])  # nothing kept; a cap below the 1.8 / 4.0 / 7.1 MB of one chunk
@pytest.mark.parametrize("alg,n,chunk", SHAPES)
def test_cap_keeps_nothing_and_changes_no_byte(alg, n, chunk, mib, monkeypatch):
    from qrkem._native import LIB
    import ctypes as ct
    monkeypatch.setenv("QRK_KEEP_MIB", mib)
    out = (ct.c_size_t * 4)()
    assert LIB.qrk_mlkem_keep_plan(alg.encode(), n, chunk or (1 << 20), ct.c_size_t(-1).value, out) == 0
    assert out[1] >= 1 and out[2] == 0
    _, _, sk, c, _ = keys(alg, n, 0xA1)
    eng = engine(alg, chunk)
    keygen(eng, alg, n, 0xA1)
    decaps_checked(eng, alg, sk, c, reused=False)


# ------------------------------------------------------------------ 7. handshake driver
def test_handshake_driver_with_the_cap_at_zero(monkeypatch):
    """The driver's reuse scenario (2048 + 952 rows) with nothing kept: same bytes, and the batch does not fail."""
    from test_gpu_handshake import test_handshake_driver_expanded_key_reuse_matches_oracle as scenario
    monkeypatch.setenv("QRK_KEEP_MIB", "0")
    scenario("ML-KEM-768", 3000, 2048)


def test_handshake_driver_reuses_the_initiators_matrix():
    """The driver's Decaps runs under the initiator's kept matrix: the responder's KeyGen in between leaves it."""
    from qrkem.handshake import HandshakeDriver
    import hkdf_spec
    alg, n, sym = "ML-KEM-768", 1100, "AES-256-GCM"
    coins = orc.bench_coins(n, 160, seed=0xD4)
    kpi, kpr, en = (np.ascontiguousarray(coins[:, a:b]) for a, b in ((0, 64), (64, 128), (128, 160)))
    infos = [hkdf_spec.protocol_info(f"a{i}", f"b{i}", sym) for i in range(n)]
    drv = HandshakeDriver(alg, symmetric_name=sym)
    drv.engine.profile(True)
    out = drv.run(infos, coins_kp_initiator=kpi, coins_kp_responder=kpr, coins_encaps=en)
    torch.cuda.synchronize()
    prof = drv.engine.profile_read()
    drv.engine.profile(False)
    want = orc.batch_handshake(alg, kpi, kpr, en, infos, hkdf_spec.SYMMETRIC_KEY_SIZE[sym])
    got = (out.pk_initiator, out.pk_responder, out.ciphertext, out.key_initiator, out.key_responder)
    for g, w in zip(got, want):
        assert np.array_equal(g.cpu().numpy(), w)
    names = [r for name in prof for r in name.split("+")]
    assert "k_xof_miss" in names and "k_xof" in names and prof["k_rho_match"][1] == 1, prof  # Encaps samples
