"""The one-bit tampers of tests/fo_compare_cases.py are what they are built to be (CPU).

For every parameter set and family: each row differs from the honest ciphertext in exactly one bit; the
rows of a family cover every unit of the HIP compare (64-bit words of the FrodoKEM ciphertext, 32-bit
words of HQC's u and v), the count taken from oracle.sizes; the C oracle rejects every row.

Absorbed by the decryption, so that only the compare can reject:
* every FrodoKEM `silent` row has frodo_spec's mu' = Decode(C - B'S) equal to the honest mu;
* HQC: hqc_spec's m' equals the honest m on every `edge` and `salt` row and on the `word` rows at
  stride 16 from row 0, plus u's last word, v's first and v's last (the pure-Python RM decoder costs
  about 0.2 ms per changed block, and a flipped bit of u changes w of them).

The oracle's FrodoKEM Decaps expands A for every row, so its pass over the 2704 rows of a FrodoKEM-1344
family is the slowest case here (about ten seconds on eight cores); every row is checked all the same.
"""
import numpy as np
import pytest

import fo_compare_cases as K

ALL = [(a, f) for a in K.FRODO_ALGS + K.HQC_ALGS for f in K.FAMILIES[a]]
WORD_STRIDE = 16


def _flipped(alg, family):
    """(names, ct_bad, byte, mask) with the single flipped bit of every row located from the data."""
    names, bad = K.rows(alg, family)
    ct = np.frombuffer(K.honest(alg)["ct"], np.uint8)
    x = bad ^ ct
    assert bad.shape == (len(names), len(ct))
    assert (np.unpackbits(x, axis=1).sum(axis=1) == 1).all(), f"{alg} {family}: a row is not a one-bit flip"
    byte = x.argmax(axis=1)
    return names, bad, byte, x[np.arange(len(bad)), byte]


@pytest.mark.parametrize("alg,family", ALL)
def test_rows_flip_one_bit_and_are_rejected(alg, family):
    """One bit per row, no row twice, and the C oracle rejects every row: ss differs from the honest one
    (HQC: status -1 as well)."""
    import oracle as orc
    names, bad, _, _ = _flipped(alg, family)
    h = K.honest(alg)
    assert len({r.tobytes() for r in bad}) == len(bad) and len(set(names)) == len(names)
    sk = np.tile(np.frombuffer(h["sk"], np.uint8), (len(bad), 1))
    ss, st = orc.batch_decaps(alg, sk, bad, with_status=True)
    assert orc.decaps_rc(alg, h["sk"], h["ct"]) == (h["ss"], 0)
    accepted = [names[i] for i in np.nonzero((ss == np.frombuffer(h["ss"], np.uint8)).all(axis=1))[0]]
    assert not accepted, f"{alg}: the oracle accepts {accepted[:4]}"
    if alg.startswith("HQC"):
        assert (st == -1).all(), f"{alg}: status 0 on {[names[i] for i in np.nonzero(st != -1)[0][:4]]}"


@pytest.mark.parametrize("alg", K.FRODO_ALGS)
def test_frodo_families_cover_every_word(alg):
    import oracle as orc
    words = orc.sizes(alg)["ct"] // 8
    p = K.F.params(alg)
    c1w = p["logq"] * p["n"] // 8  # words of Pack(B')
    for family in ("silent", "cycle"):
        _, _, byte, mask = _flipped(alg, family)
        assert sorted(byte // 8) == list(range(words)), f"{alg} {family}"
        if family == "cycle":  # bit (37 w) mod 64 of the little-endian word: every position, both halves
            bit = 8 * (byte % 8) + np.log2(mask).astype(np.int64)
            assert np.array_equal(bit, (37 * (byte // 8)) % 64)
            assert set(bit.tolist()) == set(range(64))
            for part in (slice(0, c1w), slice(c1w, words)):  # in Pack(B') and in Pack(C)
                assert {b < 32 for b in bit[part].tolist()} == {True, False}
    _, _, byte, mask = _flipped(alg, "ends")
    got = sorted(zip((byte // 8).tolist(), (8 * (byte % 8) + np.log2(mask).astype(np.int64)).tolist()))
    assert got == [(w, b) for w in (0, c1w - 1, c1w, words - 1) for b in range(64)]


@pytest.mark.parametrize("alg", K.FRODO_ALGS)
def test_frodo_silent_rows_decrypt_to_mu(alg):
    """The flipped bit is the LSB of a packed coefficient, and frodo_spec's mu' is the honest mu on every
    row; the honest ciphertext itself decrypts to mu by the same function."""
    p = K.F.params(alg)
    h = K.honest(alg)
    _, bad, byte, mask = _flipped(alg, "silent")
    pos = 8 * byte + 7 - np.log2(mask).astype(np.int64)  # MSB-first stream position
    assert (pos % p["logq"] == p["logq"] - 1).all()
    mu = np.frombuffer(h["msg"], np.uint8)
    assert np.array_equal(K.frodo_mu_prime(alg, h["sk"], np.frombuffer(h["ct"], np.uint8)[None])[0], mu)
    got = K.frodo_mu_prime(alg, h["sk"], bad)
    wrong = np.nonzero((got != mu).any(axis=1))[0]
    assert len(wrong) == 0, f"{alg}: mu' != mu on {len(wrong)} rows, first word {byte[wrong[0]] // 8}"


@pytest.mark.parametrize("alg", K.HQC_ALGS)
def test_hqc_families_cover_every_unit(alg):
    import oracle as orc
    s = orc.sizes(alg)
    nb = s["pk"] - 40
    vb = s["ct"] - 16 - nb
    n = K.H.params(alg)["n"]
    assert (nb, vb) == (K.H.params(alg)["nb"], K.H.params(alg)["vb"])
    units = [("u", j) for j in range((nb + 3) // 4)] + [("v", j) for j in range(vb // 4)]
    _, _, byte, mask = _flipped(alg, "word")
    assert [K.hqc_unit(alg, b) for b in byte.tolist()] == units
    bit = np.log2(mask).astype(np.int64)
    stray = (byte == nb - 1) & (bit >= n - 8 * (nb - 1))
    assert not stray.any()
    inword = 8 * np.where(byte < nb, byte % 4, (byte - nb) % 4) + bit
    assert len(set(inword[byte >= nb].tolist())) == 32 and {b < 16 for b in inword.tolist()} == {True, False}
    # edge: every bit of the bytes around the boundaries, but for u's bits at and above X^n
    _, _, byte, mask = _flipped(alg, "edge")
    bit = np.log2(mask).astype(np.int64)
    want = [(b, k) for b in [*range(8), *range(nb - 8, nb + 8), *range(nb + vb - 8, nb + vb + 8)] for k in range(8)
            if 8 * b + k < n or b >= nb]
    assert sorted(zip(byte.tolist(), bit.tolist())) == want
    assert {K.hqc_unit(alg, b)[0] for b in byte.tolist()} == {"u", "v", "salt"}
    _, _, byte, _ = _flipped(alg, "salt")
    assert byte.tolist() == list(range(nb + vb, nb + vb + 16)) and s["ct"] == nb + vb + 16


@pytest.mark.parametrize("alg", K.HQC_ALGS)
def test_hqc_rows_decode_to_m(alg):
    """hqc_spec's m' = m: all `edge` and `salt` rows, `word` rows at stride WORD_STRIDE and the three
    boundary units."""
    import oracle as orc
    h = K.honest(alg)
    s = orc.sizes(alg)
    nw = (s["pk"] - 40 + 3) // 4
    dec = K.HqcDecoder(alg, h["sk"])
    assert dec.mprime(h["ct"]) == h["msg"]
    assert K.H.decaps(alg, h["sk"], h["ct"]) == (h["ss"], 0)  # the memoised steps sit inside this Decaps
    for family in K.HQC_FAMILIES:
        names, bad = K.rows(alg, family)
        pick = range(len(bad)) if family != "word" else sorted({*range(0, len(bad), WORD_STRIDE), nw - 1, nw, len(bad) - 1})
        wrong = [names[i] for i in pick if dec.mprime(bad[i].tobytes()) != h["msg"]]
        assert not wrong, f"{alg}: m' != m on {wrong[:4]}"
