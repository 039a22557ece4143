"""SHA-256 of the expected outputs of the FrodoKEM from-samples cases (tests/golden/frodo_forward.json) -- TEST
INFRASTRUCTURE.

tests/frodo_forward_cases.py builds every case by rule and computes its expected bytes with oracle/py/frodo_spec.py.
For the AES names that needs A = Gen(seedA) from a pure-Python AES: 1.6 s / 3.7 s / 7 s per matrix, too long for every
GPU session, so the digests of the expected rows are stored here per name, mode and case, and the GPU test compares
digests where it does not compute the bytes.  Inputs are never stored.  tests/test_frodo_forward_cases.py regenerates
the file and compares.

    python tests/golden/make_golden_frodo_forward.py
"""
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE.parents[1] / "oracle" / "py"), str(HERE.parents[1] / "oracle"), str(HERE.parent), str(HERE)]

import frodo_forward_cases as W  # noqa: E402

PATH = HERE / "frodo_forward.json"


def generate(alg: str) -> dict:
    out = {"seedA": W.seed_a(alg).hex()}
    for mode, kg in (("encaps", False), ("keygen", True)):
        names = W.from_samples_inputs(alg, kg)["names"]
        out[mode] = dict(zip(names, W.digests(W.from_samples_expected(alg, kg))))
        assert len(out[mode]) == len(names)
    return out


def dumps(gold: dict) -> str:
    """One case per line."""
    sets = []
    for alg, d in gold.items():
        modes = []
        for mode in ("encaps", "keygen"):
            rows = ",\n".join(f"   {json.dumps(k)}:{json.dumps(v)}" for k, v in d[mode].items())
            modes.append(f'  {json.dumps(mode)}:{{\n{rows}\n  }}')
        sets.append(f' {json.dumps(alg)}:{{"seedA":{json.dumps(d["seedA"])},\n' + ",\n".join(modes) + "\n }")
    return "{\n" + ",\n".join(sets) + "\n}\n"


def load() -> dict:
    return json.loads(PATH.read_text())


def main():
    gold = {alg: generate(alg) for alg in W.ALGS}
    text = dumps(gold)
    assert json.loads(text) == gold
    PATH.write_text(text)
    print(f"{PATH.name}: {len(text)} bytes, {sum(len(d['encaps']) + len(d['keygen']) for d in gold.values())} cases")


if __name__ == "__main__":
    main()
