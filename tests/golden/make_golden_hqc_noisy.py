"""Golden HQC ciphertexts that carry many symbol errors (tests/golden/hqc_noisy.json) --
TEST INFRASTRUCTURE.

An honest ciphertext reaches the Reed-Solomon decoder with 0 (rarely 1 or 2) wrong symbols, so
it never makes the decoder correct anything.  These records do, on the public path: the key is
perturbed.  With (pk, sk) = keypair(kp_coins), a sparse Delta is XORed into the s part of pk
and into the copy of pk inside sk; Encaps under that pk' gives a ciphertext that is a valid
encryption under pk', and Decaps with sk' re-encrypts with pk', so the ciphertext is accepted
exactly when the decoder returns m.  The decoder's noise is (x + Delta) r2 - r1 y + e instead
of x r2 - r1 y + e.  Every Delta bit is at a position >= 320: theta = G(m || pk[0:80] || salt)
reads the seed and the first 320 bits of s only, so r1, r2 and e do not depend on Delta.

Search (deterministic): candidate c of a set has
  keypair coins = SHAKE256("qrk-noisy" || alg || LE64(2c)), first kp_coins bytes;
  encaps coins  = SHAKE256("qrk-noisy" || alg || LE64(2c+1)), first enc_coins bytes;
  Delta         = random.Random("<alg>/<c>") drawing a weight from the set's range and that many
                  distinct positions in [320, n);
and its error count e = the number of symbols where the RM decoding of v - u y differs from
rs_encode(m).  The first candidate found for each e in 0..delta+1 is kept (a later one replaces
it only when it supplies an error in symbol 0 or in symbol n1-1 that no kept record within the
radius has yet, so both edge positions occur in records the decoder must correct),
then two records with e >= 2 delta from heavier Deltas.  Stored per record: the coins, Delta's
bit positions, e, the wrong symbol positions, the number of RM blocks whose two largest
|Hadamard| values tie, SHA-256 of the ciphertext, and the decaps status and ss of the pure-Python
spec (oracle/py/hqc_spec.py).

    python tests/golden/make_golden_hqc_noisy.py
"""
import hashlib
import json
import random
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE.parents[1] / "oracle" / "py")]

import hqc_spec as H  # noqa: E402

ALGS = ("HQC-128", "HQC-192", "HQC-256")
# |Delta| ranges of the search: (within the radius and just beyond, far beyond)
WEIGHTS = {"HQC-128": ((0, 85), (130, 200)), "HQC-192": ((0, 150), (230, 350)), "HQC-256": ((0, 140), (260, 400))}
THETA_BITS = 8 * H.SEED_BYTES  # theta reads pk[0:80]: the 40-byte seed and the first 320 bits of s
FAR = 2  # records with e >= 2 delta
MIN_TIES = 10
MAX_CANDIDATES = 2000


def coins(alg: str, i: int, n: int) -> bytes:
    return hashlib.shake_256(b"qrk-noisy" + alg.encode() + i.to_bytes(8, "little")).digest(n)


def perturb(alg: str, pk: bytes, sk: bytes, delta_bits) -> tuple[bytes, bytes]:
    """pk', sk': Delta XORed into s in pk and in the pk held inside sk."""
    p = H.params(alg)
    b = bytearray(pk)
    for q in delta_bits:
        assert THETA_BITS <= q < p["n"]
        b[H.SEED_BYTES + q // 8] ^= 1 << (q % 8)
    pk2 = bytes(b)
    return pk2, sk[:H.SEED_BYTES + p["k"]] + pk2


def rebuild(alg: str, rec: dict) -> tuple[bytes, bytes, bytes, bytes]:
    """(pk', sk', ct, ss) of a record, by the pure-Python spec."""
    pk, sk = H.keypair(alg, bytes.fromhex(rec["kp_coins"]))
    pk2, sk2 = perturb(alg, pk, sk, rec["delta_bits"])
    ct, ss = H.encaps(alg, pk2, bytes.fromhex(rec["enc_coins"]))
    return pk2, sk2, ct, ss


def decoder_view(alg: str, sk: bytes, ct: bytes, m: bytes) -> tuple[list[int], int]:
    """What the decoder meets in Decaps(sk, ct): the positions where the RM-decoded symbols of
    v - u y differ from rs_encode(m), and the number of RM blocks with a tied maximum."""
    p = H.params(alg)
    n, k, nb, vb, mult = p["n"], p["k"], p["nb"], p["vb"], p["mult"]
    se = H.SeedExpander(sk[:H.SEED_BYTES])
    H.fixed_weight_support(se, n, p["w"])
    y = H.fixed_weight_support(se, n, p["w"])
    u = int.from_bytes(ct[:nb], "little")
    v = int.from_bytes(ct[nb:nb + vb], "little")
    word = (v ^ H.mul_sparse(y, u, n)) & ((1 << p["n1n2"]) - 1)
    span = 128 * mult
    want = H.rs_encode(p, m)
    wrong, ties = [], 0
    for i in range(p["n1"]):
        block = (word >> (span * i)) & ((1 << span) - 1)
        if H.rm_decode_symbol(block, mult) != want[i]:
            wrong.append(i)
        a = sorted((abs(t) for t in H.rm_hadamard(block, mult)), reverse=True)
        ties += a[0] == a[1]
    return wrong, ties


def candidate(alg: str, c: int, lo: int, hi: int) -> dict:
    p = H.params(alg)
    kc, ec = coins(alg, 2 * c, p["kp_coins"]), coins(alg, 2 * c + 1, p["enc_coins"])
    rng = random.Random(f"{alg}/{c}")
    delta_bits = sorted(rng.sample(range(THETA_BITS, p["n"]), rng.randint(lo, hi)))
    rec = {"kp_coins": kc.hex(), "enc_coins": ec.hex(), "delta_bits": delta_bits}
    _, sk2, ct, _ = rebuild(alg, rec)
    wrong, ties = decoder_view(alg, sk2, ct, ec[:p["k"]])
    rec.update(e=len(wrong), wrong_symbols=wrong, tied_blocks=ties)
    return rec


def search(alg: str) -> tuple[list[dict], int]:
    p = H.params(alg)
    delta, n1 = p["delta"], p["n1"]
    (lo, hi), (flo, fhi) = WEIGHTS[alg]
    kept: dict[int, dict] = {}
    edges = lambda: {q for r in kept.values() if r["e"] <= delta  # noqa: E731
                     for q in r["wrong_symbols"] if q in (0, n1 - 1)}
    c = 0
    while len(kept) < delta + 2 or len(edges()) < 2:
        assert c < MAX_CANDIDATES, f"{alg}: search did not finish"
        rec = candidate(alg, c, lo, hi)
        c += 1
        e = rec["e"]
        if e > delta + 1:
            continue
        mine = {q for q in rec["wrong_symbols"] if q in (0, n1 - 1)}
        if e not in kept:
            kept[e] = rec
        elif e <= delta and mine - edges() and not {q for q in kept[e]["wrong_symbols"] if q in (0, n1 - 1)}:
            kept[e] = rec  # same count, supplies a missing edge position and drops none
    far = []
    while len(far) < FAR:
        assert c < MAX_CANDIDATES, f"{alg}: search did not finish"
        rec = candidate(alg, c, flo, fhi)
        c += 1
        if rec["e"] >= 2 * delta:
            far.append(rec)
    return [kept[e] for e in range(delta + 2)] + far, c


def finish(alg: str, rec: dict) -> dict:
    """Expected status and ss from the spec's full Decaps; status 0 exactly within the radius."""
    p = H.params(alg)
    _, sk2, ct, ss = rebuild(alg, rec)
    ss_d, rc = H.decaps(alg, sk2, ct)
    assert (rc == 0) == (rec["e"] <= p["delta"]), (alg, rec["e"], rc)
    assert (ss_d == ss) == (rc == 0)
    sigma = sk2[H.SEED_BYTES:H.SEED_BYTES + p["k"]]
    if rc != 0:
        assert ss_d == H.shake_ds(sigma + ct[:p["nb"] + p["vb"]], H.D_K)
    return dict(rec, ct=hashlib.sha256(ct).hexdigest(), status=rc, ss=ss_d.hex())


def check(alg: str, recs: list[dict]) -> None:
    """The conditions the fixture must meet (not tunable)."""
    p = H.params(alg)
    delta, n1 = p["delta"], p["n1"]
    counts = [r["e"] for r in recs]
    assert counts[:delta + 2] == list(range(delta + 2)), counts
    assert len(counts) == delta + 2 + FAR and all(e >= 2 * delta for e in counts[delta + 2:]), counts
    inside = [r for r in recs if r["e"] <= delta]
    assert any(0 in r["wrong_symbols"] for r in inside), "no corrected error in symbol 0 (parity part)"
    assert any(n1 - 1 in r["wrong_symbols"] for r in inside), "no corrected error in symbol n1-1 (message part)"
    assert sum(r["tied_blocks"] for r in recs) >= MIN_TIES
    for r in recs:
        assert r["status"] == (0 if r["e"] <= delta else -1)
        assert all(THETA_BITS <= q < p["n"] for q in r["delta_bits"])


def main():
    out = {}
    for alg in ALGS:
        recs, tried = search(alg)
        recs = [finish(alg, r) for r in recs]
        check(alg, recs)
        out[alg] = {"delta": H.params(alg)["delta"], "candidates_tried": tried, "records": recs}
        print(f"{alg}: {tried} candidates, e = {[r['e'] for r in recs]}, "
              f"tied blocks = {sum(r['tied_blocks'] for r in recs)}")
    # one record per line
    sets = []
    for alg, d in out.items():
        recs = ",\n".join("   " + json.dumps(r, separators=(",", ":")) for r in d.pop("records"))
        head = json.dumps(d, separators=(",", ":"))[1:-1]
        sets.append(f' {json.dumps(alg)}:{{{head},"records":[\n{recs}\n ]}}')
    text = "{\n" + ",\n".join(sets) + "\n}\n"
    json.loads(text)
    (HERE / "hqc_noisy.json").write_text(text)


if __name__ == "__main__":
    main()
