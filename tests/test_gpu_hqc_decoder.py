"""HIP HQC concatenated-code decoder (k_hqc_decode's RM stage, k_hqc_rs) at and beyond its
correction radius, against the pure-Python spec (oracle/py/hqc_spec.py).

Honest ciphertexts reach the Reed-Solomon decoder with 0 (rarely 1 or 2) wrong symbols and a
one-bit tamper is absorbed by RM, so tests/test_gpu_hqc.py never makes the decoder correct
anything.  Two ways in here:

* public path -- tests/golden/hqc_noisy.json: encapsulations under a perturbed key (valid
  under it, so accepted exactly when the decoder returns m) that carry e = 0..delta+1 and
  >= 2 delta wrong symbols; ct / ss / status byte-exact, the oracle side pinned in
  tests/test_hqc_noisy_oracle.py;
* qrk_hqc_code_decode -- with u = 0 the decoded word is v itself, so the RM symbols and m'
  are compared with rm_decode_symbol / rs_decode on inputs chosen bit for bit.

Bar: byte-exact (integer work).
"""
import hashlib
import json
import random
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

ALGS = ["HQC-128", "HQC-192", "HQC-256"]
GOLD = json.loads((Path(__file__).parent / "golden" / "hqc_noisy.json").read_text())
COOP_MAX = 256  # QRK_HQC_COOP_MAX: cooperative sponges up to here, lane kernels above


@pytest.fixture(scope="module")
def engines():
    from qrkem.batch import BatchKEM
    return {a: BatchKEM(a, device=0) for a in ALGS}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _rows(items):
    return np.stack([np.frombuffer(bytes(b), np.uint8) for b in items])


# ---------------------------------------------------------------- public path, perturbed keys
def _interleave(recs):
    """Neighbours with very different error counts (the lower half of the counts interleaved
    with the upper half: 0, 9, 1, 10, ..., far, far): k_hqc_rs runs four handshakes per
    workgroup, one wave each, on wave-divergent loops."""
    by_e = sorted(range(len(recs)), key=lambda i: recs[i]["e"])
    half = (len(by_e) + 1) // 2
    return [i for pair in zip(by_e[:half], by_e[half:] + [None]) for i in pair if i is not None]


_NOISY = {}


def _noisy(alg):
    """(records in test order, pk', sk', enc coins, ct, Encaps ss) -- keys and ciphertexts from
    the C oracle, which test_hqc_noisy_oracle.py holds to the spec on these records."""
    if alg not in _NOISY:
        import make_golden_hqc_noisy as N
        import oracle as orc
        recs = GOLD[alg]["records"]
        recs = [recs[i] for i in _interleave(recs)]
        assert min(abs(a["e"] - b["e"]) for a, b in zip(recs, recs[1:])) >= GOLD[alg]["delta"] // 2
        kc = _rows(bytes.fromhex(r["kp_coins"]) for r in recs)
        ec = _rows(bytes.fromhex(r["enc_coins"]) for r in recs)
        pk, sk = orc.batch_keypair(alg, kc)
        pert = [N.perturb(alg, pk[i].tobytes(), sk[i].tobytes(), r["delta_bits"]) for i, r in enumerate(recs)]
        pk2, sk2 = _rows(t[0] for t in pert), _rows(t[1] for t in pert)
        ct, ss = orc.batch_encaps(alg, pk2, ec)
        _NOISY[alg] = (recs, pk2, sk2, ec, ct, ss)
    return _NOISY[alg]


@pytest.mark.parametrize("alg", ALGS)
def test_noisy_records(engines, alg):
    """Encaps under pk' gives the fixture's ct and ss; Decaps with sk' gives the fixture's ss and
    status (0 for e <= delta, else -1 with ss = K(sigma || ct)) on the device-tensor path and
    on the host-array path."""
    eng = engines[alg]
    recs, pk2, sk2, ec, ct, ss = _noisy(alg)
    want_ss = _rows(bytes.fromhex(r["ss"]) for r in recs)
    want_st = np.array([r["status"] for r in recs], np.int32)
    assert sorted(set(want_st)) == [-1, 0]
    g_ct, g_ss = eng.encaps(_dev(pk2), coins=_dev(ec))
    g_ct, g_ss = _host(g_ct), _host(g_ss)
    assert np.array_equal(g_ct, ct) and np.array_equal(g_ss, ss)
    for i, r in enumerate(recs):
        assert hashlib.sha256(g_ct[i].tobytes()).hexdigest() == r["ct"]
        assert (g_ss[i].tobytes().hex() == r["ss"]) == (r["status"] == 0)
    d_ss, d_st = eng.decaps(_dev(sk2), _dev(ct), return_status=True)
    d_ss, d_st = _host(d_ss), _host(d_st)
    for i, r in enumerate(recs):  # per record first, so a failure names its error count
        assert (d_ss[i].tobytes().hex(), int(d_st[i])) == (r["ss"], r["status"]), f"{alg} e={r['e']}"
    h_ss, h_st = eng.decaps(sk2, ct, return_status=True)
    assert np.array_equal(h_ss, want_ss) and np.array_equal(h_st, want_st)


@pytest.mark.parametrize("alg", ALGS)
def test_noisy_records_tiled_past_coop_max(engines, alg):
    """The same list tiled to 260 records: the lane-per-handshake seedexpander / K-hash kernels
    (n > QRK_HQC_COOP_MAX) and 65 full k_hqc_rs workgroups."""
    eng = engines[alg]
    recs, _, sk2, _, ct, _ = _noisy(alg)
    n = 260
    assert n > COOP_MAX
    idx = np.arange(n) % len(recs)
    want_ss = _rows(bytes.fromhex(recs[i]["ss"]) for i in idx)
    want_st = np.array([recs[i]["status"] for i in idx], np.int32)
    d_ss, d_st = eng.decaps(_dev(sk2[idx]), _dev(ct[idx]), return_status=True)
    assert np.array_equal(_host(d_st), want_st)
    assert np.array_equal(_host(d_ss), want_ss)
    h_ss, h_st = eng.decaps(sk2[idx], ct[idx], return_status=True)
    assert np.array_equal(h_st, want_st) and np.array_equal(h_ss, want_ss)


# ---------------------------------------------------------------- the decoder alone, u = 0
def _code_decode(eng, alg, words):
    """qrk_hqc_code_decode on ciphertexts with u = 0, v = words[i] (ints of n1 n2 bits), salt 0:
    (syms [n, n1], mprime [n, k])."""
    import hqc_spec as H
    import oracle as orc
    p = H.params(alg)
    n = len(words)
    ct = np.zeros((n, p["ct"]), np.uint8)
    ct[:, p["nb"]:p["nb"] + p["vb"]] = _rows(w.to_bytes(p["vb"], "little") for w in words)
    sk1 = orc.keypair(alg, bytes(range(p["kp_coins"])))[1]
    sk = np.tile(np.frombuffer(sk1, np.uint8), (n, 1))
    syms, mp = eng.hqc_code_decode(_dev(sk), _dev(ct))
    return _host(syms), _host(mp)


def _rm_table(mult):
    import hqc_spec as H
    return [sum(H.rm_codeword(b) << (128 * c) for c in range(mult)) for b in range(256)]


def _peaks(t):
    """indices where |t| attains its maximum"""
    m = max(abs(x) for x in t)
    return [i for i, x in enumerate(t) if abs(x) == m]


def _rm_blocks(alg):
    """(blocks, tied): duplicated-RM blocks (ints of 128 mult bits) and the indices of the
    heavy-noise ones whose maximum |Hadamard| value is attained more than once.  The noise
    sample grows until the spec itself shows >= 20 such blocks, one tie between a positive
    and a negative peak and one between an index < 64 and an index >= 64."""
    import hqc_spec as H
    p = H.params(alg)
    mult, n2 = p["mult"], p["n2"]
    cw = _rm_table(mult)
    blocks = list(cw)                                    # all 256 symbols, clean
    blocks += [0, (1 << n2) - 1]                         # all-zero, all-ones
    for c in range(mult):                                # one flipped bit: every position of every copy
        for j in range(128):
            blocks.append(cw[(37 * j + 11 * c + 5) & 255] ^ (1 << (128 * c + j)))
    rng = random.Random(f"rm/{alg}")
    tied, mixed_sign, across = [], False, False
    heavy = 0
    while heavy < 200 or len(tied) < 20 or not (mixed_sign and across):
        assert heavy < 4000, "the sample does not meet the tie conditions"
        b = cw[rng.randrange(256)]
        for q in rng.sample(range(n2), round(0.45 * n2)):
            b ^= 1 << q
        t = H.rm_hadamard(b, mult)
        pk = _peaks(t)
        if len(pk) > 1:
            tied.append(len(blocks))
            mixed_sign |= len({t[i] > 0 for i in pk}) == 2
            across |= pk[0] < 64 <= pk[-1]
        blocks.append(b)
        heavy += 1
    return blocks, tied


@pytest.mark.parametrize("alg", ALGS)
def test_rm_symbols_match_spec(engines, alg):
    """k_hqc_decode's RM stage vs rm_decode_symbol: clean codewords, constant blocks, single
    flips in every lane / word half / copy, and heavy noise with tied peaks (first maximum,
    sign of that maximum; ties across the sign and across the k0 / k1 halves)."""
    import hqc_spec as H
    p = H.params(alg)
    mult, n1, span = p["mult"], p["n1"], p["n2"]
    blocks, tied = _rm_blocks(alg)
    assert len(tied) >= 20
    want = [H.rm_decode_symbol(b, mult) for b in blocks]
    assert want[:256] == list(range(256)) and want[256:258] == [0, 128]
    pad = -len(blocks) % n1
    padded = blocks + [0] * pad
    words = [sum(padded[r * n1 + i] << (span * i) for i in range(n1)) for r in range(len(padded) // n1)]
    syms, _ = _code_decode(engines[alg], alg, words)
    got = syms.reshape(-1)[:len(blocks)].tolist()
    bad = [i for i in range(len(blocks)) if got[i] != want[i]]
    assert not bad, f"{alg}: {len(bad)} blocks differ, first {bad[0]}: got {got[bad[0]]} want {want[bad[0]]}" \
                    f" (tied: {bad[0] in tied})"
    assert syms.reshape(-1)[len(blocks):].tolist() == [0] * pad


def _spread(e, n1):
    return sorted({round(i * (n1 - 1) / (e - 1)) for i in range(e)}) if e > 1 else [n1 // 2]


def _rs_cases(alg):
    """(received words, messages, number with a mid-stream zero discrepancy): rs_encode(msg)
    with e <= delta symbol errors."""
    import hqc_spec as H
    p = H.params(alg)
    n1, k, delta = p["n1"], p["k"], p["delta"]
    t2 = 2 * delta
    rng = random.Random(f"rs/{alg}")
    cases = []

    def add(msg, pos, vals):
        r = H.rs_encode(p, msg)
        for q, x in zip(pos, vals):
            assert 0 <= q < n1 and 1 <= x <= 255
            r[q] ^= x
        cases.append((r, bytes(msg), len(pos)))

    rnd = lambda e: [rng.randrange(1, 256) for _ in range(e)]  # noqa: E731
    for e in range(delta + 1):
        add(bytes(k), range(e), [1] * e)                                     # parity part from symbol 0, value 1
        add(b"\xff" * k, range(n1 - e, n1), [255] * e)                        # message part up to n1-1, value 255
        lo = t2 - (e + 1) // 2
        add(rng.randbytes(k), range(lo, lo + e), rnd(e))                     # consecutive, across 2 delta - 1 | 2 delta
        sp = _spread(e, n1) if e else []
        add(rng.randbytes(k), sp, ([1] + rnd(len(sp) - 2) + [255])[:len(sp)] if len(sp) > 1 else rnd(len(sp)))
        add(rng.randbytes(k) if e % 3 else bytes(k), sorted(rng.sample(range(n1), e)), rnd(e))  # anywhere
    add(rng.randbytes(k), [t2], [255])
    # a zero discrepancy in the middle of Berlekamp-Massey: d == 0 at a step i < 2e with L > 0
    zero_mid, trials = 0, 0
    while zero_mid < 6:
        trials += 1
        assert trials < 5000, "no mid-stream zero discrepancy found"
        e = delta - trials % (delta - 1)  # delta .. 2
        msg, pos, vals = rng.randbytes(k), sorted(rng.sample(range(n1), e)), rnd(e)
        r = H.rs_encode(p, msg)
        for q, x in zip(pos, vals):
            r[q] ^= x
        trace = []
        H.rs_berlekamp_massey(H.rs_syndromes(p, r), trace)
        if any(d == 0 and 0 < L and i < 2 * e for i, L, d in trace):
            add(msg, pos, vals)
            zero_mid += 1
    return cases, zero_mid


@pytest.mark.parametrize("alg", ALGS)
def test_rs_message_matches_spec(engines, alg):
    """k_hqc_rs vs rs_decode on clean RM encodings of RS codewords with e = 0..delta symbol
    errors: runs from symbol 0, up to symbol n1-1 and across 2 delta - 1 | 2 delta, evenly
    spaced and scattered positions, error values 1 and 255, the all-zero and the all-0xFF
    message, and received words whose Berlekamp-Massey run meets a zero discrepancy mid-stream."""
    import hqc_spec as H
    p = H.params(alg)
    n1, delta, mult, span = p["n1"], p["delta"], p["mult"], p["n2"]
    t2 = 2 * delta
    cases, zero_mid = _rs_cases(alg)
    assert zero_mid >= 5
    assert {e for _, _, e in cases} == set(range(delta + 1))
    cw = _rm_table(mult)
    words = [sum(cw[s] << (span * i) for i, s in enumerate(r)) for r, _, _ in cases]
    dec = [H.rs_decode(p, r) for r, _, _ in cases]
    want = [bytes(c[t2:]) for c in dec]
    assert all(w == m for w, (_, m, _) in zip(want, cases))  # within the radius the spec returns msg
    hit = {q for c, (r, _, _) in zip(dec, cases) for q in range(n1) if c[q] != r[q]}
    assert {0, t2 - 1, t2, n1 - 1} <= hit
    syms, mp = _code_decode(engines[alg], alg, words)
    assert syms.tolist() == [r for r, _, _ in cases]
    bad = [i for i in range(len(cases)) if mp[i].tobytes() != want[i]]
    assert not bad, f"{alg}: {len(bad)} of {len(cases)} differ, first: case {bad[0]} with e={cases[bad[0]][2]}"


def test_code_decode_rejects_oversize_batch():
    """More records than the context chunk is an error, not a partial run."""
    from qrkem.batch import BatchKEM
    eng = BatchKEM("HQC-128", device=0, chunk=64)
    n = eng.effective_chunk + 1
    sk = torch.zeros((n, eng.sk_len), dtype=torch.uint8, device="cuda")
    ct = torch.zeros((n, eng.ct_len), dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="chunk"):
        eng.hqc_code_decode(sk, ct)
