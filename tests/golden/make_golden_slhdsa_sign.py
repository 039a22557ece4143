"""Writes tests/golden/slhdsa_sign.json from tests/slhdsa_spec.py (deterministic; regenerates bit-identically):

    python tests/golden/make_golden_slhdsa_sign.py

Signing cases at the edges of the index space, for the GPU signer (csrc/slhdsa_sign.hip).  Per name, with the
fixture key of make_golden_slhdsa.py and opt_rand = PK.seed, the messages message(name + "-sign", counter)
(so a case's length is its counter) are searched in order of the counter, with PRF_msg + H_msg only, for the
first one that satisfies each of

    leaf_first   idx_leaf = 0                      leaf_last   idx_leaf = 2^h' - 1
    fors_first   some FORS index = 0               fors_last   some FORS index = 2^a - 1
    tree_top     the top bit of idx_tree set (bit 63 for 256f, where h - h' = 64; bit 62 otherwise)

One counter may serve several predicates; at most five cases per name.  The rarest predicate (a FORS index at
one end for 256f: 35 / 512) holds for about 7 % of the candidates; the search gives up after 65 536.  Per case:
the counter, the length, the digest, R, the predicates it serves, the SHA3-256 of the spec's whole signature
and of its parts in order (R, the FORS part, each of the d XMSS signatures), so that a mismatch can be located
without running the spec.  Every signature contains the WOTS+ digits 0 and 15 (asserted).  About 15 s.
"""
from __future__ import annotations

import hashlib
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE))

import make_golden_slhdsa as gold  # noqa: E402
import slhdsa_spec as spec  # noqa: E402

OUT = HERE / "slhdsa_sign.json"
CAP = 1 << 16
PREDICATES = ("leaf_first", "leaf_last", "fors_first", "fors_last", "tree_top")


def message(name: str, counter: int) -> bytes:
    return gold.message(name + "-sign", counter)


def digest_of(name: str, sk: bytes, msg: bytes, opt_rand: bytes = None, ctx: bytes = b""):
    """(R, digest) of signing `msg` under `sk`: PRF_msg and H_msg only."""
    p = spec.PARAMS[name]
    n = p.n
    sk_prf, pk_seed, pk_root = sk[n:2 * n], sk[2 * n:3 * n], sk[3 * n:]
    hs = spec.Hasher(p, pk_seed)
    m = spec._frame(p, msg, ctx)
    r = hs.PRF_msg(sk_prf, pk_seed if opt_rand is None else opt_rand, m)
    return r, hs.H_msg(r, pk_root, m)


def predicates(name: str, digest: bytes) -> dict:
    p = spec.PARAMS[name]
    md, tree, leaf = spec.split_digest(p, digest)
    idx = spec._fors_indices(p, md)
    return {"leaf_first": leaf == 0, "leaf_last": leaf == (1 << p.hp) - 1, "fors_first": 0 in idx,
            "fors_last": (1 << p.a) - 1 in idx, "tree_top": bool(tree >> (p.h - p.hp - 1))}


def parts(name: str, sig: bytes) -> list:
    """R, the FORS part and the d XMSS signatures of a signature."""
    p = spec.PARAMS[name]
    n = p.n
    fors = p.k * (p.a + 1) * n
    xl = (p.hp + p.len) * n
    out = [sig[:n], sig[n:n + fors]] + [sig[n + fors + j * xl:n + fors + (j + 1) * xl] for j in range(p.d)]
    assert sum(len(x) for x in out) == len(sig) == p.sig
    return out


def search(name: str, sk: bytes) -> dict:
    """counter -> the predicates it is the first to satisfy."""
    need, found = list(PREDICATES), {}
    for counter in range(CAP):
        if not need:
            break
        hit = predicates(name, digest_of(name, sk, message(name, counter))[1])
        for key in [k for k in need if hit[k]]:
            found.setdefault(counter, []).append(key)
            need.remove(key)
    assert not need, (name, need)
    return found


def build() -> dict:
    doc = {"note": "tests/golden/make_golden_slhdsa_sign.py; spec signatures with opt_rand = PK.seed, empty context, "
                   "over message(name + '-sign', counter) under the key of slhdsa.json", "sets": {}}
    for name, p in spec.PARAMS.items():
        sd = gold.seeds(name)
        pk, sk = spec.keygen(name, *sd)
        cases = []
        for counter, keys in sorted(search(name, sk).items()):
            m = message(name, counter)
            r, digest = digest_of(name, sk, m)
            sig = spec.sign(name, sk, m)
            tr = spec.verify_trace(name, pk, m, sig)
            assert tr["flags"] == 0 and tr["digest"] == digest and sig[:p.n] == r
            digits = set()
            for j in range(p.d):
                digits |= set(spec.wots_digits(p, tr["fors_pk"] if j == 0 else tr["roots"][(j - 1) * p.n:j * p.n]))
            assert {0, 15} <= digits, (name, counter)
            cases.append({"counter": counter, "len": len(m), "serves": keys, "digest": digest.hex(), "r": r.hex(),
                          "sig_sha3": hashlib.sha3_256(sig).hexdigest(),
                          "parts_sha3": [hashlib.sha3_256(x).hexdigest() for x in parts(name, sig)]})
        assert 1 <= len(cases) <= 5
        doc["sets"][name] = {"cases": cases}
    return doc


def load(path: Path = OUT) -> dict:
    """name -> the stored cases, each with its message under "msg"."""
    doc = json.loads(path.read_text())
    return {name: [dict(c, msg=message(name, c["counter"])) for c in s["cases"]] for name, s in doc["sets"].items()}


if __name__ == "__main__":
    text = json.dumps(build(), indent=0, separators=(",", ":")) + "\n"
    OUT.write_text(text)
    print(f"wrote {OUT} ({len(text)} bytes)")
