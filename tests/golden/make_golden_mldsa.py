"""Writes tests/golden/mldsa.json from tests/mldsa_spec.py (deterministic; regenerates bit-identically):

    python tests/golden/make_golden_mldsa.py

Per parameter set: one key from a fixed xi (pk stored as hex, sk not stored: keygen_internal(xi)
rebuilds it), four records signed with the empty context and rnd = 0^32 (the standard's
deterministic variant), and a fixed tamper list.  Messages are message(set, length), so only their
lengths are stored; 70 is the length at which tr || M' fills exactly one SHAKE256 block
(64 + 2 + 70 = 136) and 2500 is about the size of an init message carrying a base64 ML-KEM-768 key.
Per record: the signature (base64, which is what keeps the file under 100 KB), mu, c~' and SHA3-256 of
the w1Encode bytes, from verify_trace.

A tamper entry names a record and one edit: {"flip": [where, byte, bit]} with where in sig / pk / msg,
{"set": [[sig byte, value], ...]} for the structural edits (each malformed-hint class, z coefficients on
and next to the norm bound), or {"sig_of": record} for a signature moved from another row.  `flags`
is the spec's flag word for the edited row.  This script asserts that the spec verifies every record
and rejects every entry, so no test has to excuse a row.
"""
from __future__ import annotations

import base64
import hashlib
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import mldsa_spec as spec  # noqa: E402

OUT = HERE / "mldsa.json"
LENGTHS = (0, 70, 71, 2500)
XI = {name: hashlib.shake_256(b"qrkem-mldsa-xi" + name.encode()).digest(32) for name in spec.PARAMS}


def message(name: str, length: int) -> bytes:
    return hashlib.shake_256(b"qrkem-mldsa-msg" + name.encode() + length.to_bytes(4, "little")).digest(length)


def apply_tamper(entry: dict, pk: bytes, msgs: list, sigs: list):
    """(pk, msg, sig) of the row the entry describes."""
    r = entry["record"]
    pk, msg, sig = bytearray(pk), bytearray(msgs[r]), bytearray(sigs[r])
    if "flip" in entry:
        where, byte, bit = entry["flip"]
        {"sig": sig, "pk": pk, "msg": msg}[where][byte] ^= 1 << bit
    elif "set" in entry:
        for byte, value in entry["set"]:
            sig[byte] = value
    else:
        sig = bytearray(sigs[entry["sig_of"]])
    return bytes(pk), bytes(msg), bytes(sig)


def _z_coeff0(p, sig: bytes, value: int) -> list:
    """Byte writes that make coefficient 0 of z[0] equal `value` (BitPack stores gamma1 - z)."""
    n = (p.zbits + 7) // 8
    word = int.from_bytes(sig[p.ctilde:p.ctilde + n], "little")
    word = (word & ~((1 << p.zbits) - 1)) | (p.gamma1 - value)
    return [[p.ctilde + i, b] for i, b in enumerate(word.to_bytes(n, "little"))]


def tamper_list(p, sigs: list) -> list:
    hint = p.sig - p.omega - p.k  # sig offset of the hint bytes y[0 .. omega + k)
    zmid = p.ctilde + (hint - p.ctilde) // 2
    out = [
        {"label": "ctilde bit", "record": 0, "flip": ["sig", 0, 0]},
        {"label": "ctilde last byte", "record": 1, "flip": ["sig", p.ctilde - 1, 7]},
        {"label": "z low bit", "record": 2, "flip": ["sig", zmid, 0]},
        {"label": "z first byte", "record": 3, "flip": ["sig", p.ctilde, 3]},
        {"label": "z last byte top bit", "record": 0, "flip": ["sig", hint - 1, 7]},
        {"label": "hint index bit", "record": 1, "flip": ["sig", hint, 0]},
        {"label": "hint index high bit", "record": 2, "flip": ["sig", hint + 1, 7]},
        {"label": "hint count bit", "record": 3, "flip": ["sig", hint + p.omega, 0]},
        {"label": "hint last count bit", "record": 0, "flip": ["sig", p.sig - 1, 1]},
        {"label": "hint padding bit", "record": 1, "flip": ["sig", hint + p.omega - 1, 0]},
        {"label": "rho bit", "record": 2, "flip": ["pk", 0, 0]},
        {"label": "rho last byte", "record": 3, "flip": ["pk", 31, 7]},
        {"label": "t1 bit", "record": 0, "flip": ["pk", 32 + 5, 2]},
        {"label": "t1 last byte", "record": 1, "flip": ["pk", p.pk - 1, 7]},
        {"label": "message first bit", "record": 1, "flip": ["msg", 0, 0]},
        {"label": "message byte 69 (last of the one-block record)", "record": 1, "flip": ["msg", 69, 7]},
        {"label": "message byte 70 (first of the second block)", "record": 2, "flip": ["msg", 70, 0]},
        {"label": "message last byte", "record": 3, "flip": ["msg", 2499, 4]},
        {"label": "signature of the next row", "record": 0, "sig_of": 1},
        {"label": "signature of the previous row", "record": 3, "sig_of": 2},
    ]
    for r in (0, 2):
        y = sigs[r][hint:]
        counts = list(y[p.omega:])
        total = counts[-1]
        # first polynomial with two hints: its second index made equal to its first
        i2 = next(i for i in range(p.k) if counts[i] - (counts[i - 1] if i else 0) >= 2)
        first = counts[i2 - 1] if i2 else 0
        out.append({"label": "hint index not increasing", "record": r, "set": [[hint + first + 1, y[first]]]})
        i1 = next(i for i in range(1, p.k) if counts[i - 1] >= 1)
        out.append({"label": "hint count decreasing", "record": r,
                    "set": [[hint + p.omega + j, counts[i1 - 1] - 1] for j in range(i1, p.k)]})
        out.append({"label": "hint count above omega", "record": r, "set": [[p.sig - 1, p.omega + 1]]})
        assert total < p.omega
        out.append({"label": "hint padding nonzero", "record": r, "set": [[hint + p.omega - 1, 1]]})
        out.append({"label": "hint padding nonzero right after the last index", "record": r,
                    "set": [[hint + total, 255]]})
    bound = p.gamma1 - p.beta
    for label, value in (("z coefficient +(gamma1 - beta)", bound), ("z coefficient -(gamma1 - beta)", -bound),
                         ("z coefficient gamma1 - beta - 1", bound - 1), ("z coefficient gamma1 (largest encodable)",
                                                                          p.gamma1)):
        out.append({"label": label, "record": 1, "set": _z_coeff0(p, sigs[1], value)})
    return out


def build() -> dict:
    doc = {"note": "tests/golden/make_golden_mldsa.py; FIPS 204 pure ML-DSA, empty context, rnd = 0^32",
           "lengths": list(LENGTHS), "sets": {}}
    for name, p in spec.PARAMS.items():
        pk, sk = spec.keygen_internal(XI[name], name)
        assert (len(pk), len(sk)) == (p.pk, p.sk)
        msgs = [message(name, n) for n in LENGTHS]
        sigs = [spec.sign(sk, m) for m in msgs]
        records = []
        for m, s in zip(msgs, sigs):
            tr = spec.verify_trace(pk, m, s)
            assert len(s) == p.sig and tr["flags"] == 0 and tr["ctilde"] == s[:p.ctilde]
            records.append({"len": len(m), "sig": base64.b64encode(s).decode(), "mu": tr["mu"].hex(),
                            "ctilde": tr["ctilde"].hex(), "w1_sha3": hashlib.sha3_256(tr["w1"]).hexdigest()})
        tampers = tamper_list(p, sigs)
        for e in tampers:
            tpk, tmsg, tsig = apply_tamper(e, pk, msgs, sigs)
            assert (tpk, tmsg, tsig) != (pk, msgs[e["record"]], sigs[e["record"]]), e["label"]
            e["flags"] = spec.verify_trace(tpk, tmsg, tsig)["flags"]
            assert e["flags"] != 0 and not spec.verify(tpk, tmsg, tsig), e["label"]
        doc["sets"][name] = {"xi": XI[name].hex(), "pk": pk.hex(), "records": records, "tampers": tampers}
    return doc


def load(path: Path = OUT) -> dict:
    """The fixture with its byte strings decoded: per set pk, msgs, sigs, records, tampers."""
    doc = json.loads(path.read_text())
    out = {}
    for name, s in doc["sets"].items():
        recs = s["records"]
        out[name] = {"xi": bytes.fromhex(s["xi"]), "pk": bytes.fromhex(s["pk"]),
                     "msgs": [message(name, r["len"]) for r in recs],
                     "sigs": [base64.b64decode(r["sig"]) for r in recs], "records": recs, "tampers": s["tampers"]}
    return out


if __name__ == "__main__":
    text = json.dumps(build(), indent=0, separators=(",", ":")) + "\n"
    OUT.write_text(text)
    print(f"wrote {OUT} ({len(text)} bytes)")
