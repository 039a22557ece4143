"""CPU: the ML-KEM key-set seeds (tests/golden/mlkem_keyed.json) have the SampleNTT fix-up property according to the
spec, and the generator reproduces the committed fixture."""
import make_golden_mlkem_keyed as gen
import mlkem_keyed_cases as cases
import oracle as orc


def test_generator_reproduces_the_fixture():
    assert gen.render(gen.build()) == cases.FIXTURE.read_text()


def test_every_parameter_set_has_a_key_on_the_fixup_path():
    fx = cases.load_fixture()
    rows = [bytes.fromhex(h) for h in fx["seeds"]]
    assert len(rows) == cases.G_KEYS and len(set(rows)) == cases.G_KEYS and all(len(r) == 64 for r in rows)
    assert rows == cases.seeds(fx["counter"])
    for alg in cases.ALGS:
        found = {str(t): [list(e) for e in cases.fixup_entries(alg, c)] for t, c in enumerate(rows)
                 if cases.fixup_entries(alg, c)}
        assert found and found == fx["fixup"][alg], alg


def test_the_property_is_about_the_key_the_oracle_generates():
    """rho as the test derives it is the rho in the oracle's public key, and a listed entry is short of 256
    coefficients after three blocks while an unlisted one is not."""
    fx = cases.load_fixture()
    for alg in cases.ALGS:
        k = cases.spec.PARAMS[alg][0]
        t, ents = next(iter(fx["fixup"][alg].items()))
        coins = bytes.fromhex(fx["seeds"][int(t)])
        pk, _ = orc.keypair(alg, coins)
        rho = pk[384 * k:]
        assert rho == cases.spec.G(coins[:32] + bytes([k]))[0]
        listed = {tuple(e) for e in ents}
        for i in range(k):
            for j in range(k):
                short = cases.accepted_in_fast_path(rho + bytes([j, i])) < 256
                assert short == ((i, j) in listed)
