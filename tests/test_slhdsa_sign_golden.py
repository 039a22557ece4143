"""CPU: tests/golden/slhdsa_sign.json holds what its generator says: every stored case meets the predicates it
is stored for (the digest alone is recomputed), all five predicates are served for every name, and one 128f
case is regenerated in full by the spec."""
import hashlib

import pytest

import make_golden_slhdsa as gold
import make_golden_slhdsa_sign as sgold
import slhdsa_spec as spec

NAMES = sorted(spec.PARAMS)


@pytest.fixture(scope="module")
def keys():
    return {name: spec.keygen(name, *gold.seeds(name)) for name in NAMES}


@pytest.fixture(scope="module")
def cases():
    return sgold.load()


@pytest.mark.parametrize("name", NAMES)
def test_stored_cases_meet_their_predicates(keys, cases, name):
    p = spec.PARAMS[name]
    assert 1 <= len(cases[name]) <= 5
    served = []
    for c in cases[name]:
        assert c["len"] == len(c["msg"]) == c["counter"]
        r, digest = sgold.digest_of(name, keys[name][1], c["msg"])
        assert r.hex() == c["r"] and digest.hex() == c["digest"]
        hit = sgold.predicates(name, digest)
        assert c["serves"] and all(hit[k] for k in c["serves"]), c["counter"]
        assert len(c["parts_sha3"]) == 2 + p.d
        served += c["serves"]
    assert sorted(served) == sorted(sgold.PREDICATES)  # each exactly once: the first counter that meets it


def test_one_case_regenerated_by_the_spec(keys, cases):
    name = "SPHINCS+-SHA2-128f-simple"
    c = cases[name][0]
    sig = spec.sign(name, keys[name][1], c["msg"])
    assert hashlib.sha3_256(sig).hexdigest() == c["sig_sha3"]
    assert [hashlib.sha3_256(x).hexdigest() for x in sgold.parts(name, sig)] == c["parts_sha3"]
    assert sig[:16].hex() == c["r"] and spec.verify(name, keys[name][0], c["msg"], sig)
