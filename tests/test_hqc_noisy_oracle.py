"""HQC ciphertexts that carry many symbol errors (CPU): the C oracle against the pure-Python
restatement on tests/golden/hqc_noisy.json.

Each record is an encapsulation under a perturbed key (tests/golden/make_golden_hqc_noisy.py):
valid under that key, so Decaps accepts it exactly when the concatenated-code decoder returns
m, while the decoder meets e wrong Reed-Solomon symbols, e = 0..delta+1 and two far beyond.
The GPU path is held to the same records in tests/test_gpu_hqc_decoder.py.
"""
import json
from pathlib import Path

import numpy as np
import pytest

import hqc_spec as H
import make_golden_hqc_noisy as N
import oracle as orc

GOLD = json.loads((Path(__file__).parent / "golden" / "hqc_noisy.json").read_text())
ALGS = ["HQC-128", "HQC-192", "HQC-256"]


@pytest.fixture(scope="module")
def rebuilt():
    """alg -> [(pk', sk', ct, ss of Encaps)] by the Python spec, once."""
    return {alg: [N.rebuild(alg, r) for r in GOLD[alg]["records"]] for alg in ALGS}


@pytest.mark.parametrize("alg", ALGS)
def test_fixture_conditions(alg):
    """Every count 0..delta+1 once and in order, two records at e >= 2 delta, corrected errors
    in symbol 0 and in symbol n1-1, at least 10 tied RM blocks, status 0 exactly when e <= delta."""
    recs = GOLD[alg]["records"]
    assert GOLD[alg]["delta"] == H.params(alg)["delta"]
    N.check(alg, recs)
    delta = H.params(alg)["delta"]
    for r in recs:
        assert (r["status"] == 0) == (r["e"] <= delta)
        assert r["e"] == len(r["wrong_symbols"])


@pytest.mark.parametrize("alg", ALGS)
def test_c_oracle_and_spec_agree(alg, rebuilt):
    """Encaps under pk' and Decaps with sk': the C oracle, the Python spec and the fixture give
    the same ct, ss and status for every record; a rejected record's ss is K(sigma || ct)."""
    p = H.params(alg)
    recs = GOLD[alg]["records"]
    arr = lambda i: np.stack([np.frombuffer(t[i], np.uint8) for t in rebuilt[alg]])  # noqa: E731
    pk, sk, ct = arr(0), arr(1), arr(2)
    ec = np.stack([np.frombuffer(bytes.fromhex(r["enc_coins"]), np.uint8) for r in recs])
    oct_, oss = orc.batch_encaps(alg, pk, ec)
    assert np.array_equal(oct_, ct)
    dss, dst = orc.batch_decaps(alg, sk, ct, with_status=True)
    for i, (r, (_, sk2, c, ss)) in enumerate(zip(recs, rebuilt[alg])):
        assert oss[i].tobytes() == ss
        assert H.decaps(alg, sk2, c) == (bytes.fromhex(r["ss"]), r["status"])
        assert (dss[i].tobytes().hex(), int(dst[i])) == (r["ss"], r["status"])
        if r["status"] == 0:
            assert r["ss"] == ss.hex()
        else:
            sigma = sk2[H.SEED_BYTES:H.SEED_BYTES + p["k"]]
            assert r["ss"] == H.shake_ds(sigma + c[:p["nb"] + p["vb"]], H.D_K).hex()


@pytest.mark.parametrize("alg", ALGS)
def test_recorded_error_counts(alg, rebuilt):
    """The recorded e, wrong positions and tie counts are what rm_decode_symbol and rs_encode
    give for v - u y."""
    k = H.params(alg)["k"]
    for r, (_, sk2, c, _) in zip(GOLD[alg]["records"], rebuilt[alg]):
        wrong, ties = N.decoder_view(alg, sk2, c, bytes.fromhex(r["enc_coins"])[:k])
        assert (len(wrong), wrong, ties) == (r["e"], r["wrong_symbols"], r["tied_blocks"])
