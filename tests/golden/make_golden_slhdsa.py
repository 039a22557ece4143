"""Writes tests/golden/slhdsa.json from tests/slhdsa_spec.py (deterministic; regenerates bit-identically):

    python tests/golden/make_golden_slhdsa.py

Per name (three parameter sets, two flavours each): the key seeds, the public key, three messages (stored as
lengths: the messages are message(name, length)) and per message the SHA3-256 of the spec's signature and,
from verify_trace, the H_msg digest, the FORS public key and the SHA3-256 of the d layer roots.  Signatures
are not stored (17 to 50 KB each): `signatures()` regenerates them from the spec and checks the stored
SHA3-256 first.  The lengths are 0, one outer-hash padding edge of the set (R || PK.seed || PK.root || M
of 56 bytes for SHA-256, 112 for SHA-512) and 2500.

Cost of the spec, measured when this was written (one CPU core): a bare seeded F (copy + update + digest)
0.53 us; one signature 0.21 s (128f, about 0.1 M hashes), 0.35 s (192f), 0.67 s (256f, about 0.35 M);
one key 0.01 to 0.03 s; one verification 12 to 18 ms.  The whole file takes about 8 s.
"""
from __future__ import annotations

import hashlib
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import slhdsa_spec as spec  # noqa: E402

OUT = HERE / "slhdsa.json"
LENGTHS = {16: (0, 8, 2500), 24: (0, 40, 2500), 32: (0, 16, 2500)}


def seeds(name: str):
    """SK.seed, SK.prf, PK.seed of the fixture key of `name`."""
    n = spec.PARAMS[name].n
    s = hashlib.shake_256(b"qrkem-slhdsa-seed" + name.encode()).digest(3 * n)
    return s[:n], s[n:2 * n], s[2 * n:]


def message(name: str, length: int) -> bytes:
    return hashlib.shake_256(b"qrkem-slhdsa-msg" + name.encode() + length.to_bytes(4, "little")).digest(length)


def build() -> dict:
    doc = {"note": "tests/golden/make_golden_slhdsa.py; spec signatures with opt_rand = PK.seed, empty context",
           "sets": {}}
    for name, p in spec.PARAMS.items():
        sd = seeds(name)
        pk, sk = spec.keygen(name, *sd)
        assert (len(pk), len(sk)) == (p.pk, p.sk)
        records = []
        for length in LENGTHS[p.n]:
            m = message(name, length)
            sig = spec.sign(name, sk, m)
            tr = spec.verify_trace(name, pk, m, sig)
            assert len(sig) == p.sig and tr["flags"] == 0 and tr["roots"][-p.n:] == pk[p.n:]
            records.append({"len": length, "sig_sha3": hashlib.sha3_256(sig).hexdigest(), "digest": tr["digest"].hex(),
                            "fors_pk": tr["fors_pk"].hex(), "roots_sha3": hashlib.sha3_256(tr["roots"]).hexdigest()})
        doc["sets"][name] = {"seeds": [s.hex() for s in sd], "pk": pk.hex(), "records": records}
    return doc


def load(path: Path = OUT) -> dict:
    """The fixture with its byte strings decoded: per name seeds, pk, sk (rebuilt by keygen), msgs, records."""
    doc = json.loads(path.read_text())
    out = {}
    for name, s in doc["sets"].items():
        sd = [bytes.fromhex(x) for x in s["seeds"]]
        pk, sk = spec.keygen(name, *sd)
        out[name] = {"seeds": sd, "pk": bytes.fromhex(s["pk"]), "sk": sk, "keygen_pk": pk,
                     "msgs": [message(name, r["len"]) for r in s["records"]], "records": s["records"]}
    return out


def signatures(name: str, entry: dict) -> list:
    """The spec's signatures over the fixture messages of `name`, checked against the stored SHA3-256."""
    sigs = [spec.sign(name, entry["sk"], m) for m in entry["msgs"]]
    for sig, rec in zip(sigs, entry["records"]):
        assert hashlib.sha3_256(sig).hexdigest() == rec["sig_sha3"], name
    return sigs


if __name__ == "__main__":
    text = json.dumps(build(), indent=0, separators=(",", ":")) + "\n"
    OUT.write_text(text)
    print(f"wrote {OUT} ({len(text)} bytes)")
