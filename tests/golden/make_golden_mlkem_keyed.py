"""ML-KEM key-set seeds (tests/golden/mlkem_keyed.json) -- TEST INFRASTRUCTURE.

A key set samples A_hat once per key when it is loaded, the SampleNTT fix-up included.  About 0.7 % of matrix
entries need a 4th SHAKE128 block, so 65 arbitrary keys may hold none at ML-KEM-512 (260 entries).  This searches
the counter-derived seed lists of tests/mlkem_keyed_cases.py for the first one under which every parameter set has
at least one such key, and stores the 65 seeds with, per parameter set, the keys and entries that have the property
according to the pure-Python spec (oracle/py/mlkem_spec.py).

    python tests/golden/make_golden_mlkem_keyed.py
"""
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import mlkem_keyed_cases as cases  # noqa: E402


def build() -> dict:
    counter = 0
    while True:
        rows = cases.seeds(counter)
        found = {alg: {str(t): cases.fixup_entries(alg, c) for t, c in enumerate(rows) if cases.fixup_entries(alg, c)}
                 for alg in cases.ALGS}
        if all(found.values()):
            return {"counter": counter, "seeds": [r.hex() for r in rows],
                    "fixup": {alg: {t: [list(e) for e in ents] for t, ents in found[alg].items()} for alg in cases.ALGS}}
        counter += 1


def render(doc: dict) -> str:
    return json.dumps(doc, indent=1) + "\n"


if __name__ == "__main__":
    cases.FIXTURE.write_text(render(build()))
    print(f"wrote {cases.FIXTURE}")
