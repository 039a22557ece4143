"""ML-KEM key sets (qrk_mlkem_pubkeys_load / qrk_mlkem_seckeys_load, qrk_mlkem_encaps_keyed_batch,
qrk_mlkem_decaps_keyed_batch, csrc/mlkem_keyed.hip) against the per-row calls on the gathered key rows with the same
coins and against the C oracle: byte for byte on ct, ss and status, over every set size, row count, index pattern
and chunking at which the keyed kernels take another path.  The 65 keys come from tests/golden/mlkem_keyed.json,
whose seeds put at least one key of every parameter set on the SampleNTT fix-up path (asserted here again)."""
import ctypes as ct

import numpy as np
import pytest

import mlkem_keyed_cases as cases
import oracle as orc

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
ALGS = cases.ALGS
K_OF = {"ML-KEM-512": 2, "ML-KEM-768": 3, "ML-KEM-1024": 4}
SET_SIZES = (1, 2, 65)
ROWS = (1, 15, 16, 17, 63, 64, 65, 257)
CHUNK = 128  # 257 rows: three chunks with a one-row tail
NMAX = 257
FILL = 0xA5


def al256(x):
    return (x + 255) & ~255


def set_bytes(alg, secret, g):
    """A_hat (384 bytes per entry) | the key rows | public: H(ek) | a word per key; every part 256-aligned."""
    k = K_OF[alg]
    s = orc.sizes(alg)
    total = al256(k * k * g * 384) + al256((s["sk"] if secret else s["pk"]) * g)
    return total if secret else total + al256(32 * g) + al256(4 * g)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def patterns(g, n):
    """name -> key_index (uint32 [n]), or None for the NULL index of a set of one key"""
    i = np.arange(n, dtype=np.uint32)
    out = {"zeros": np.zeros(n, np.uint32), "last": np.full(n, g - 1, np.uint32), "mod": i % g,
           "reversed": (g - 1 - i % g).astype(np.uint32),
           "random": np.random.default_rng(0xC0FFEE + 1000 * g + n).integers(0, g, n, dtype=np.uint32)}
    if g == 1:
        out["null"] = None
    return out


class Case:
    """One parameter set: the engine (chunk 128), the 65 key pairs, 257 coins, and raw keyed calls that pre-fill
    their outputs, so a row the kernels did not write shows."""

    def __init__(self, alg):
        from qrkem.batch import BatchKEM
        self.alg = alg
        self.s = orc.sizes(alg)
        fx = cases.load_fixture()
        self.seeds = np.stack([np.frombuffer(bytes.fromhex(h), np.uint8) for h in fx["seeds"]])
        self.pk, self.sk = orc.batch_keypair(alg, self.seeds)
        self.coins = orc.bench_coins(NMAX, 32, seed=0x6B65 + K_OF[alg])
        self.eng = BatchKEM(alg, device=0, chunk=CHUNK)
        self.d_pk, self.d_sk, self.d_coins = dev(self.pk), dev(self.sk), dev(self.coins)
        self.pub, self.sec = {}, {}

    def public(self, g):
        if g not in self.pub:
            self.pub[g] = self.eng.load_public_keys(self.d_pk[:g])
        return self.pub[g]

    def secret(self, g):
        if g not in self.sec:
            self.sec[g] = self.eng.load_secret_keys(self.d_sk[:g])
        return self.sec[g]

    def raw_encaps(self, ks, n, index, coins):
        from qrkem._native import LIB
        c = torch.full((n, self.s["ct"]), FILL, dtype=torch.uint8, device="cuda")
        ss = torch.full((n, 32), FILL, dtype=torch.uint8, device="cuda")
        st = torch.full((n,), 77, dtype=torch.int32, device="cuda")
        idx = dev(index.view(np.int32)) if index is not None else None
        rc = LIB.qrk_mlkem_encaps_keyed_batch(self.eng._ctx, ks._handle, n, ct.c_void_p(idx.data_ptr()) if idx is not None
                                              else None, ct.c_void_p(c.data_ptr()), ct.c_void_p(ss.data_ptr()),
                                              ct.c_void_p(coins.data_ptr()), ct.c_void_p(st.data_ptr()),
                                              self.eng._stream())
        torch.cuda.synchronize()
        return rc, host(c), host(ss), host(st)

    def raw_decaps(self, ks, cts, index):
        from qrkem._native import LIB
        n = cts.shape[0]
        ss = torch.full((n, 32), FILL, dtype=torch.uint8, device="cuda")
        st = torch.full((n,), 77, dtype=torch.int32, device="cuda")
        idx = dev(index.view(np.int32)) if index is not None else None
        d_ct = dev(cts)
        rc = LIB.qrk_mlkem_decaps_keyed_batch(self.eng._ctx, ks._handle, n, ct.c_void_p(idx.data_ptr()) if idx is not None
                                              else None, ct.c_void_p(ss.data_ptr()), ct.c_void_p(d_ct.data_ptr()),
                                              ct.c_void_p(st.data_ptr()), self.eng._stream())
        torch.cuda.synchronize()
        return rc, host(ss), host(st)

    def per_row_encaps(self, pk_rows, coins):
        c, ss, st = self.eng.encaps(dev(pk_rows), coins=dev(coins), return_status=True)
        return host(c), host(ss), host(st)

    def per_row_decaps(self, sk_rows, cts):
        ss, st = self.eng.decaps(dev(sk_rows), dev(cts), return_status=True)
        return host(ss), host(st)

    def close(self):
        for ks in list(self.pub.values()) + list(self.sec.values()):
            ks.close()
        self.eng.close()


@pytest.fixture(scope="module", params=ALGS)
def case(request):
    c = Case(request.param)
    yield c
    c.close()


def gather(index, n):
    return np.zeros(n, np.int64) if index is None else index.astype(np.int64)


def test_the_keys_still_cover_the_fixup_path(case):
    """The chosen seeds put a key of this parameter set on the SampleNTT fix-up path, in every set of 65 keys; the
    oracle's keys are the spec's for these seeds."""
    with_fixup = cases.keys_with_fixup(case.alg, [bytes(r) for r in case.seeds])
    assert with_fixup and max(with_fixup) < 65
    t = with_fixup[0]
    assert bytes(case.pk[t]) == cases.spec.keypair_derand(case.alg, bytes(case.seeds[t]))[0]


def test_encaps_every_size_set_and_pattern(case):
    for g in SET_SIZES:
        ks = case.public(g)
        for n in ROWS:
            coins = case.coins[:n]
            for name, index in patterns(g, n).items():
                rows = case.pk[gather(index, n)]
                rc, c, ss, st = case.raw_encaps(ks, n, index, case.d_coins[:n])
                assert rc == 0, (g, n, name)
                oc, oss = orc.batch_encaps(case.alg, rows, coins)
                assert np.array_equal(c, oc) and np.array_equal(ss, oss) and not st.any(), (g, n, name, "oracle")
                if name in ("mod", "random", "null"):  # the per-row call on the gathered rows
                    pc, pss, pst = case.per_row_encaps(rows, coins)
                    assert np.array_equal(c, pc) and np.array_equal(ss, pss) and np.array_equal(st, pst), (g, n, name)


def test_null_index_is_refused_for_two_keys(case):
    import qrkem
    rc, c, ss, st = case.raw_encaps(case.public(2), 3, None, case.d_coins[:3])
    assert rc == -1 and "only for a key set of one key" in qrkem.last_error()
    assert (c == FILL).all() and (ss == FILL).all() and (st == 77).all()
    rc, ss, st = case.raw_decaps(case.secret(2), np.zeros((3, case.s["ct"]), np.uint8), None)
    assert rc == -1 and "only for a key set of one key" in qrkem.last_error() and (ss == FILL).all()
    with pytest.raises(ValueError, match="only for a key set of one key"):
        case.eng.encaps_keyed(case.public(2), n=3)


def flip(cts, row, byte, bit=0):
    cts[row, byte] ^= 1 << bit


def decaps_rows(case, g, n, kind):
    """(key_index, ct rows) of a Decaps case: ciphertexts the oracle made for key a[i], decapsulated under key b[i]"""
    rng = np.random.default_rng(0xDECA + 100 * g + n)
    a = rng.integers(0, g, n, dtype=np.uint32)
    b = a.copy()
    if kind in ("cross", "mix"):
        sel = np.arange(n) % 3 == 1 if kind == "mix" else np.ones(n, bool)
        b[sel] = (a[sel] + 1 + rng.integers(0, max(g - 1, 1), int(sel.sum()), dtype=np.uint32)) % g if g > 1 else a[sel]
    cts, _ = orc.batch_encaps(case.alg, case.pk[a.astype(np.int64)], case.coins[:n])
    cts = cts.copy()
    u_len = case.s["ct"] - 32 * (5 if K_OF[case.alg] == 4 else 4)
    edges = (0, u_len - 1, u_len, case.s["ct"] - 1)  # first and last byte of u and of v
    if kind in ("flip", "mix"):
        for i in range(n):
            if kind == "flip" or i % 3 == 2:
                flip(cts, i, edges[(i // 3) % 4], bit=(i % 8))
    return b, cts


def test_decaps_honest_flipped_cross_key_and_mixed(case):
    for g in SET_SIZES:
        ks = case.secret(g)
        for n in ROWS:
            for kind in ("honest", "flip", "cross", "mix"):
                if n not in (17, 65, 257) and kind != "mix":
                    continue  # every size sees the mixed batch; the pure kinds at three sizes
                index, cts = decaps_rows(case, g, n, kind)
                rows = case.sk[index.astype(np.int64)]
                rc, ss, st = case.raw_decaps(ks, cts, index)
                assert rc == 0 and not st.any(), (g, n, kind)
                assert np.array_equal(ss, orc.batch_decaps(case.alg, rows, cts)), (g, n, kind, "oracle")
                pss, pst = case.per_row_decaps(rows, cts)
                assert np.array_equal(ss, pss) and np.array_equal(st, pst), (g, n, kind, "per row")
                if kind == "honest":  # and what Encaps agreed on
                    _, oss = orc.batch_encaps(case.alg, case.pk[index.astype(np.int64)], case.coins[:n])
                    assert np.array_equal(ss, oss)
        # the NULL index of a set of one key
        index, cts = decaps_rows(case, 1, 65, "mix")
        rc, ss, st = case.raw_decaps(case.secret(1), cts, None)
        assert rc == 0 and np.array_equal(ss, orc.batch_decaps(case.alg, case.sk[np.zeros(65, np.int64)], cts))


def set_coeff(pk, coeff, value):
    """The 12-bit field `coeff` of ByteEncode_12(t_hat) in a public key"""
    out = pk.copy()
    bit = 12 * coeff
    v = int.from_bytes(bytes(out[bit // 8: bit // 8 + 2]), "little")
    sh = bit % 8
    v = (v & ~(0xFFF << sh)) | (value << sh)
    out[bit // 8: bit // 8 + 2] = np.frombuffer(v.to_bytes(2, "little"), np.uint8)
    return out


def test_malformed_keys_load_and_answer_as_the_per_row_call(case):
    k = K_OF[case.alg]
    bad = [set_coeff(case.pk[1 + t], coeff, value)
           for t, (coeff, value) in enumerate((c, v) for c in (0, 256 * k - 1, 256 * (k - 1) + 128) for v in (3329, 4095))]
    keys = np.stack([case.pk[0]] + bad + [case.pk[7]])  # good, six bad ones, good
    for b in bad:
        assert not cases.spec.ek_modulus_ok(case.alg, bytes(b))
    with case.eng.load_public_keys(dev(keys)) as ks:
        assert ks.g == 8
        for n in (17, 257):
            index = (np.arange(n, dtype=np.uint32) * 5) % 8
            rows = keys[index.astype(np.int64)]
            rc, c, ss, st = case.raw_encaps(ks, n, index, case.d_coins[:n])
            assert rc == 0
            isbad = (index >= 1) & (index <= 6)
            assert np.array_equal(st, np.where(isbad, -1, 0)) and isbad.any() and not isbad.all()
            pc, pss, pst = case.per_row_encaps(rows, case.coins[:n])
            assert np.array_equal(c, pc) and np.array_equal(ss, pss) and np.array_equal(st, pst)
            oc, oss = orc.batch_encaps(case.alg, rows[~isbad], case.coins[:n][~isbad])
            assert np.array_equal(c[~isbad], oc) and np.array_equal(ss[~isbad], oss)


def test_bad_indices_are_refused_zeroed_and_leave_the_rest_exact(case):
    n = NMAX
    refused = {0: 0, 64: 1, 127: 2, 128: 2, 200: 0, 255: 1, 256: 2}  # first, middle, last row of a chunk; the tail
    for g in (2, 65):
        values = (g, g + 1, 0xFFFFFFFF)
        index = np.arange(n, dtype=np.uint32) % g
        good = index.copy()
        for row, which in refused.items():
            index[row] = values[which]
        ok = np.ones(n, bool)
        ok[list(refused)] = False
        # Encaps
        rc, c, ss, st = case.raw_encaps(case.public(g), n, index, case.d_coins[:n])
        assert rc == 0
        oc, oss = orc.batch_encaps(case.alg, case.pk[good.astype(np.int64)], case.coins[:n])
        assert np.array_equal(st, np.where(ok, 0, -1))
        assert not c[~ok].any() and not ss[~ok].any()
        assert np.array_equal(c[ok], oc[ok]) and np.array_equal(ss[ok], oss[ok])
        # Decaps of those ciphertexts
        rc, dss, dst = case.raw_decaps(case.secret(g), oc, index)
        assert rc == 0 and np.array_equal(dst, np.where(ok, 0, -1))
        assert not dss[~ok].any() and np.array_equal(dss[ok], oss[ok])
        # the next calls on the context are exact
        rc, c, ss, st = case.raw_encaps(case.public(g), n, good, case.d_coins[:n])
        assert rc == 0 and np.array_equal(c, oc) and np.array_equal(ss, oss) and not st.any()
        rc, dss, dst = case.raw_decaps(case.secret(g), oc, good)
        assert rc == 0 and np.array_equal(dss, oss) and not dst.any()


def test_set_lifetime(case):
    from qrkem._native import LIB
    alg, n = case.alg, 65
    which = ALGS.index(alg)
    for g in SET_SIZES:
        for secret, ks in ((False, case.public(g)), (True, case.secret(g))):
            out = (ct.c_size_t * 4)()
            assert LIB.qrk_mlkem_keyset_info(ks._handle, out) == 0
            assert list(out) == [g, which, int(secret), set_bytes(alg, secret, g)]
            assert ks.device_bytes == set_bytes(alg, secret, g) and ks.g == g and not ks.closed
    # two public sets alive at once on one context, used alternately: keys 0..1 and keys 2..3
    other = case.eng.load_public_keys(case.d_pk[2:4])
    index = np.arange(n, dtype=np.uint32) % 2
    for _ in range(2):
        for ks, base in ((case.public(2), 0), (other, 2)):
            c, ss = case.eng.encaps_keyed(ks, index, coins=case.coins[:n])
            oc, oss = orc.batch_encaps(alg, case.pk[index.astype(np.int64) + base], case.coins[:n])
            assert np.array_equal(host(c), oc) and np.array_equal(host(ss), oss)
    # free and reload; a closed set raises
    other.close()
    assert other.closed and other.device_bytes == 0
    with pytest.raises(ValueError, match="closed"):
        case.eng.encaps_keyed(other, index, coins=case.coins[:n])
    with case.eng.load_public_keys(case.pk[2:4]) as again:  # host keys this time
        c, ss, st = case.eng.encaps_keyed(again, torch.from_numpy(index.view(np.int32)).cuda(), coins=case.d_coins[:n],
                                          return_status=True)
        oc, oss = orc.batch_encaps(alg, case.pk[index.astype(np.int64) + 2], case.coins[:n])
        assert np.array_equal(host(c), oc) and np.array_equal(host(ss), oss) and not host(st).any()
    assert again.closed
    sec = case.eng.load_secret_keys(case.sk[:2])
    sec.close()
    with pytest.raises(ValueError, match="closed"):
        case.eng.decaps_keyed(sec, oc, index)
    # a public set cannot decapsulate, a secret one cannot encapsulate (the library's own check)
    import qrkem
    rc, _, _ = case.raw_decaps(case.public(2), oc, index)
    assert rc == -1 and "public key set cannot decapsulate" in qrkem.last_error()
    rc, _, _, _ = case.raw_encaps(case.secret(2), n, index, case.d_coins[:n])
    assert rc == -1 and "secret key set cannot encapsulate" in qrkem.last_error()


def test_round_trip_through_the_two_halves(case):
    """Encaps under the pk halves (OS coins), Decaps under the sk halves of the same keys: ss equal on both sides."""
    g, n = 65, 257
    index = np.random.default_rng(5).integers(0, g, n, dtype=np.uint32)
    c, ss, st = case.eng.encaps_keyed(case.public(g), index, return_status=True)
    ss2, st2 = case.eng.decaps_keyed(case.secret(g), c, index, return_status=True)
    assert torch.equal(ss, ss2) and not host(st).any() and not host(st2).any()
    assert len({bytes(r) for r in host(ss)}) == n  # OS coins: every row its own secret
    assert np.array_equal(host(ss), orc.batch_decaps(case.alg, case.sk[index.astype(np.int64)], host(c)))
