"""Adversarial but legal ML-KEM inputs, end to end through the C ABI.

The parity tests feed honest keys, pseudo-random coins and single-bit flips.  These feed what a
peer may legally send instead: encapsulation keys on both sides of the FIPS 203 section 7.2 modulus
check at every coefficient position, decapsulation keys whose 12-bit fields are non-canonical
(ByteDecode_12 reduces them mod q, Decaps checks nothing), a stored H(ek) that is not the hash of
the stored ek, a bit flip at every ciphertext byte, extreme ciphertext bytes, and degenerate keys
and coins.  Expected bytes come from the C oracle (pinned against the Python restatement on the
same kinds of input by tests/test_mlkem_malformed_oracle.py).

Every case runs on both schedules: n <= 1024 (one-launch kernels) and the same rows padded with
honest rows to n > 1024 (batched kernels); a handful of rows also go through the host-pointer
entry points and the single-shot OQS wrapper.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

ALGS = ["ML-KEM-512", "ML-KEM-768", "ML-KEM-1024"]
Q = 3329
NH = 1100  # honest rows per algorithm (also the padding of the batched runs)
SMALL = 1000  # rows per call on the one-launch schedule (n <= 1024)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def dec12(b):
    """[..., 384 m] bytes -> [..., 256 m] 12-bit fields (no reduction)."""
    b = np.asarray(b, np.int64).reshape(b.shape[:-1] + (-1, 3))
    lo = b[..., 0] | ((b[..., 1] & 0x0F) << 8)
    hi = (b[..., 1] >> 4) | (b[..., 2] << 4)
    return np.stack([lo, hi], axis=-1).reshape(b.shape[:-2] + (-1,))


def enc12(f):
    """[..., 256 m] 12-bit fields -> [..., 384 m] bytes."""
    f = np.asarray(f, np.int64).reshape(f.shape[:-1] + (-1, 2))
    a, b = f[..., 0], f[..., 1]
    by = np.stack([a & 0xFF, (a >> 8) | ((b & 0xF) << 4), b >> 4], axis=-1)
    return by.reshape(f.shape[:-2] + (-1,)).astype(np.uint8)


def set12(row, p, v):
    """Field p of a 12-bit-packed byte row := v (in place)."""
    o = 3 * (p // 2)
    if p % 2 == 0:
        row[o] = v & 0xFF
        row[o + 1] = (row[o + 1] & 0xF0) | (v >> 8)
    else:
        row[o + 1] = (row[o + 1] & 0x0F) | ((v & 0xF) << 4)
        row[o + 2] = v >> 4


class Ctx:
    def __init__(self, alg):
        import mlkem_spec as spec
        import oracle as orc
        from qrkem.batch import BatchKEM
        self.alg = alg
        self.k = spec.PARAMS[alg][0]
        self.du, self.dv = spec.PARAMS[alg][3:5]
        self.eng = BatchKEM(alg, device=0)
        coins = orc.bench_coins(NH, 96, seed=0xAD5E + self.k)
        self.kc, self.ec = np.ascontiguousarray(coins[:, :64]), np.ascontiguousarray(coins[:, 64:])
        self.pk, self.sk = orc.batch_keypair(alg, self.kc)
        self.ct, self.ss = orc.batch_encaps(alg, self.pk, self.ec)

    # -- both schedules: [(label, outputs for the first len(rows) rows)]
    def encaps_both(self, pk, coins):
        n, out = len(pk), []
        parts = [self.eng.encaps(_dev(pk[i:i + SMALL]), coins=_dev(coins[i:i + SMALL]), return_status=True)
                 for i in range(0, n, SMALL)]
        out.append(("one-launch",) + tuple(np.concatenate([_host(p[j]) for p in parts]) for j in range(3)))
        pad = max(0, 1025 - n) + 7
        r = self.eng.encaps(_dev(np.concatenate([pk, self.pk[:pad]])), coins=_dev(np.concatenate([coins, self.ec[:pad]])),
                            return_status=True)
        c, s, st = (_host(t) for t in r)
        assert np.array_equal(c[n:], self.ct[:pad]) and np.array_equal(s[n:], self.ss[:pad]) and not st[n:].any()
        out.append(("batched", c[:n], s[:n], st[:n]))
        return out

    def decaps_both(self, sk, ct):
        n, out = len(sk), []
        parts = [_host(self.eng.decaps(_dev(sk[i:i + SMALL]), _dev(ct[i:i + SMALL]))) for i in range(0, n, SMALL)]
        out.append(("one-launch", np.concatenate(parts)))
        pad = max(0, 1025 - n) + 7
        s = _host(self.eng.decaps(_dev(np.concatenate([sk, self.sk[:pad]])), _dev(np.concatenate([ct, self.ct[:pad]]))))
        assert np.array_equal(s[n:], self.ss[:pad])
        out.append(("batched", s[:n]))
        return out

    def decaps_few(self, sk, ct, idx):
        """Host-pointer and single-shot OQS calls for the rows idx."""
        from qrkem import oqs
        idx = list(idx)
        host = self.eng.decaps(np.ascontiguousarray(sk[idx]), np.ascontiguousarray(ct[idx]))
        single = np.array([np.frombuffer(oqs.KeyEncapsulation(self.alg, sk[i].tobytes()).decap_secret(ct[i].tobytes()),
                                         np.uint8) for i in idx])
        return [("host", host), ("single-shot", single)]


@pytest.fixture(scope="module")
def ctxs():
    return {a: Ctx(a) for a in ALGS}


@pytest.mark.parametrize("alg", ALGS)
def test_modulus_check_every_position(ctxs, alg):
    """For every coefficient position p of ek: field p = 3329 is rejected (status -1), field p = 3328
    is accepted and byte-exact.  Rows alternate rejected / accepted, so every accepted row sits
    between rejected ones; a few rows carry 4095 and several bad fields.  Nothing is asserted about
    ct / ss of rejected rows (include/qrkem.h documents only the status)."""
    import oracle as orc
    from qrkem import oqs
    c = ctxs[alg]
    npos = 256 * c.k
    rows, bad = [], []
    for p in range(npos):
        for v in (Q, Q - 1):
            r = c.pk[p % NH].copy()
            set12(r, p, v)
            rows.append(r)
            bad.append(v >= Q)
    for fields in ([(0, 4095)], [(npos - 1, 4095)], [(1, 4095), (npos - 2, Q)], [(p, 4095) for p in range(npos)],
                   [(255, Q), (256, Q)]):
        r = c.pk[5].copy()
        for p, v in fields:
            set12(r, p, v)
        rows += [r, c.pk[6].copy()]  # an honest row after each
        bad += [True, False]
    pk = np.array(rows)
    bad = np.array(bad)
    n = len(pk)
    coins = np.ascontiguousarray(np.resize(c.ec, (n, 32)))
    want_ct, want_ss = orc.batch_encaps(alg, pk[~bad], coins[~bad])
    for label, ct, ss, st in c.encaps_both(pk, coins):
        assert np.array_equal(st, np.where(bad, -1, 0)), (label, np.nonzero(st != np.where(bad, -1, 0))[0][:8])
        assert np.array_equal(ct[~bad], want_ct), label
        assert np.array_equal(ss[~bad], want_ss), label
    # host pointers and single shots: first, an odd and the last position, both values
    few = [0, 1, 2, 3, 2 * (npos - 1), 2 * (npos - 1) + 1, n - 2, n - 1]
    ct, ss, st = c.eng.encaps(np.ascontiguousarray(pk[few]), coins=np.ascontiguousarray(coins[few]), return_status=True)
    assert np.array_equal(st, np.where(bad[few], -1, 0))
    ok = ~bad[few]
    wc, ws = orc.batch_encaps(alg, pk[few][ok], coins[few][ok])
    assert np.array_equal(ct[ok], wc) and np.array_equal(ss[ok], ws)
    for i in few:
        kem = oqs.KeyEncapsulation(alg)
        if bad[i]:
            with pytest.raises(RuntimeError):
                kem.encap_secret_derand(pk[i].tobytes(), coins[i].tobytes())
        else:
            assert kem.encap_secret_derand(pk[i].tobytes(), coins[i].tobytes()) == orc.encaps(
                alg, pk[i].tobytes(), coins[i].tobytes())


@pytest.mark.parametrize("alg", ALGS)
def test_aliased_decapsulation_keys(ctxs, alg):
    """dk' = dk with fields v < 767 re-encoded as v + q (still 12 bits).  ByteDecode_12 reduces mod
    q and Decaps applies no modulus check, so dk' behaves as dk: the honest ct is accepted with the
    honest ss, a tampered ct gives the oracle's J(z || c)."""
    import oracle as orc
    c = ctxs[alg]
    k = c.k
    npos = 256 * k
    sk_rows, src = [], []

    def variant(i, s_mask, t_mask):
        r = c.sk[i].copy()
        for off, mask in ((0, s_mask), (384 * k, t_mask)):
            f = dec12(r[off:off + 384 * k])
            f = np.where(mask & (f < 4096 - Q), f + Q, f)
            assert f.max() < 4096
            r[off:off + 384 * k] = enc12(f)
        sk_rows.append(r)
        src.append(i)

    every = np.ones(npos, bool)
    none = np.zeros(npos, bool)
    second = np.arange(npos) % 2 == 0
    i = 0
    for s_mask, t_mask in [(every, none), (none, every), (every, every), (second, ~second), (~second, second)]:
        for _ in range(3):
            variant(i, s_mask, t_mask)
            i += 1
    # single fields: the first and the last position of each polynomial (any eligible honest row)
    for pos in [256 * j + e for j in range(k) for e in (0, 255)]:
        for region in (0, 1):
            one = none.copy()
            one[pos] = True
            for j in range(i, NH):
                if dec12(c.sk[j][384 * k * region:384 * k * (region + 1)])[pos] < 4096 - Q:
                    break
            else:
                pytest.fail("no honest key with an eligible field")
            variant(j, one if region == 0 else none, one if region == 1 else none)
    sk = np.array(sk_rows)
    src = np.array(src)
    assert not np.array_equal(sk, c.sk[src]) and (dec12(sk[:, :768 * k]) >= Q).any(axis=1).all()
    ct = c.ct[src].copy()
    tampered = ct.copy()
    tampered[np.arange(len(ct)), (37 * np.arange(len(ct))) % ct.shape[1]] ^= 0x10
    sk2, ct2 = np.concatenate([sk, sk]), np.concatenate([ct, tampered])
    want = orc.batch_decaps(alg, sk2, ct2)
    n = len(sk)
    assert np.array_equal(want[:n], c.ss[src])  # the oracle accepts too
    assert np.array_equal(want[n:], orc.batch_decaps(alg, c.sk[src], tampered))  # and rejects as for dk
    assert not (want[n:] == c.ss[src]).all(axis=1).any()
    for label, ss in c.decaps_both(sk2, ct2) + c.decaps_few(sk2, ct2, [0, 3, 6, n - 1, n, 2 * n - 1]):
        w = want if len(ss) == 2 * n else want[[0, 3, 6, n - 1, n, 2 * n - 1]]
        assert np.array_equal(ss, w), label


@pytest.mark.parametrize("alg", ALGS)
def test_foreign_h_is_used_as_stored(ctxs, alg):
    """dk's h replaced by arbitrary bytes; the ciphertext built with the Python restatement from
    (K, r) = G(m || h).  Decaps must return K: it uses the stored h, it does not recompute H(ek)."""
    import mlkem_spec as spec
    c = ctxs[alg]
    k = c.k
    rng = np.random.default_rng(1203 + k)
    n = 3
    sk = c.sk[:n].copy()
    cts, keys = [], []
    for i in range(n):
        h = bytes(rng.integers(0, 256, 32, dtype=np.uint8)) if i else bytes(range(32))
        sk[i, 768 * k + 32:768 * k + 64] = np.frombuffer(h, np.uint8)
        m = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
        K, r = spec.G(m + h)
        cts.append(np.frombuffer(spec.kpke_encrypt(alg, c.pk[i].tobytes(), m, r), np.uint8))
        keys.append(np.frombuffer(K, np.uint8))
    ct, keys = np.array(cts), np.array(keys)
    assert not np.array_equal(ct, c.ct[:n])
    for label, ss in c.decaps_both(sk, ct) + c.decaps_few(sk, ct, range(n)):
        assert np.array_equal(ss, keys), label


@pytest.mark.parametrize("alg", ALGS)
def test_ciphertext_bit_flip_at_every_byte(ctxs, alg):
    """One honest (dk, ct) replicated ct_len times, row i with bit i mod 8 of byte i flipped: both
    ends of c1, both ends of c2 and the seam are covered by construction.  Every row equals the
    oracle's J(z || c), differs from the honest ss and from every other row."""
    import oracle as orc
    c = ctxs[alg]
    L = c.ct.shape[1]
    sk = np.repeat(c.sk[3:4], L, axis=0)
    ct = np.repeat(c.ct[3:4], L, axis=0)
    i = np.arange(L)
    ct[i, i] ^= (1 << (i % 8)).astype(np.uint8)
    want = orc.batch_decaps(alg, sk, ct)
    assert not (want == c.ss[3]).all(axis=1).any()
    assert len(np.unique(want, axis=0)) == L
    seam = 32 * c.du * c.k
    few = [0, 1, seam - 1, seam, L - 4, L - 1]
    for label, ss in c.decaps_both(sk, ct) + c.decaps_few(sk, ct, few):
        assert np.array_equal(ss, want if len(ss) == L else want[few]), (label, np.nonzero((ss != want[:len(ss)]).any(axis=1))[0][:8])


@pytest.mark.parametrize("alg", ALGS)
def test_extreme_ciphertext_bytes(ctxs, alg):
    """All 0x00, all 0xFF (every du- and dv-field at its maximum), 0xAA / 0x55, c1 and c2 at opposite
    extremes, and 64 rows of seeded uniform bytes, against the oracle."""
    import oracle as orc
    c = ctxs[alg]
    L = c.ct.shape[1]
    seam = 32 * c.du * c.k
    rows = [np.zeros(L, np.uint8), np.full(L, 0xFF, np.uint8), np.full(L, 0xAA, np.uint8), np.full(L, 0x55, np.uint8),
            np.where(np.arange(L) % 2 == 0, 0xAA, 0x55).astype(np.uint8)]
    for a, b in ((0xFF, 0x00), (0x00, 0xFF)):
        r = np.full(L, a, np.uint8)
        r[seam:] = b
        rows.append(r)
    rng = np.random.default_rng(1204 + c.k)
    ct = np.concatenate([np.array(rows), rng.integers(0, 256, (64, L), dtype=np.uint8)])
    sk = np.ascontiguousarray(c.sk[10:10 + len(ct)])
    want = orc.batch_decaps(alg, sk, ct)
    for label, ss in c.decaps_both(sk, ct) + c.decaps_few(sk, ct, range(7)):
        assert np.array_equal(ss, want[:len(ss)]), label


@pytest.mark.parametrize("alg", ALGS)
def test_degenerate_keys_and_coins(ctxs, alg):
    """Encaps with t_hat all 0, all 3328 or alternating, rho all 0x00 / 0xFF, coins all 0x00 / 0xFF;
    Decaps with s_hat = 0 and t_hat = 0 accepts the ciphertext made for that key (v = e2 + mu, so
    m' = m) and returns the Encaps ss; KeyGen with all-zero and all-0xFF coins."""
    import hashlib
    import oracle as orc
    from qrkem import oqs
    c = ctxs[alg]
    k = c.k
    j = np.arange(256 * k)
    that = [enc12(np.zeros(256 * k, np.int64)), enc12(np.full(256 * k, Q - 1)), enc12(np.where(j % 2 == 0, 0, Q - 1)),
            enc12(np.where(j % 2 == 0, Q - 1, 0))]
    rhos = [c.pk[0, 384 * k:], np.zeros(32, np.uint8), np.full(32, 0xFF, np.uint8)]
    coin = [c.ec[0], np.zeros(32, np.uint8), np.full(32, 0xFF, np.uint8)]
    pk = np.array([np.concatenate([t, r]) for t in that for r in rhos for _ in coin])
    coins = np.array([m for _ in that for _ in rhos for m in coin])
    want_ct, want_ss = orc.batch_encaps(alg, pk, coins)
    for label, ct, ss, st in c.encaps_both(pk, coins):
        assert not st.any(), label
        assert np.array_equal(ct, want_ct) and np.array_equal(ss, want_ss), label
    ct, ss, st = c.eng.encaps(np.ascontiguousarray(pk[:9]), coins=np.ascontiguousarray(coins[:9]), return_status=True)
    assert not st.any() and np.array_equal(ct, want_ct[:9]) and np.array_equal(ss, want_ss[:9])
    assert oqs.KeyEncapsulation(alg).encap_secret_derand(pk[4].tobytes(), coins[4].tobytes()) == (
        want_ct[4].tobytes(), want_ss[4].tobytes())
    # s_hat = 0, t_hat = 0: the first 9 rows above carry t_hat = 0
    n0 = 9
    sk = np.zeros((n0, c.sk.shape[1]), np.uint8)
    sk[:, 384 * k:768 * k + 32] = pk[:n0]
    for i in range(n0):
        sk[i, 768 * k + 32:768 * k + 64] = np.frombuffer(hashlib.sha3_256(pk[i].tobytes()).digest(), np.uint8)
    sk[:, 768 * k + 64:] = c.sk[:n0, 768 * k + 64:]
    assert np.array_equal(orc.batch_decaps(alg, sk, want_ct[:n0]), want_ss[:n0])
    for label, ss in c.decaps_both(sk, want_ct[:n0]) + c.decaps_few(sk, want_ct[:n0], range(3)):
        assert np.array_equal(ss, want_ss[:len(ss)]), label
    # KeyGen
    kc = np.array([np.zeros(64, np.uint8), np.full(64, 0xFF, np.uint8)])
    wpk, wsk = orc.batch_keypair(alg, kc)
    pk1, sk1 = c.eng.keypair(coins=_dev(kc))
    assert np.array_equal(_host(pk1), wpk) and np.array_equal(_host(sk1), wsk)
    padded = np.concatenate([kc, c.kc[:1030]])
    pk2, sk2 = c.eng.keypair(coins=_dev(padded))
    assert np.array_equal(_host(pk2)[:2], wpk) and np.array_equal(_host(sk2)[:2], wsk)
    assert np.array_equal(_host(pk2)[2:], c.pk[:1030]) and np.array_equal(_host(sk2)[2:], c.sk[:1030])
    pk3, sk3 = c.eng.keypair(coins=kc)
    assert np.array_equal(pk3, wpk) and np.array_equal(sk3, wsk)
    for i in range(2):
        kem = oqs.KeyEncapsulation(alg)
        assert kem.generate_keypair_derand(kc[i].tobytes()) == wpk[i].tobytes()
        assert kem.export_secret_key() == wsk[i].tobytes()
