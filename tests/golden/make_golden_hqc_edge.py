"""HQC ring products at the edges of support and operand (tests/golden/hqc_edge.json) --
TEST INFRASTRUCTURE.

Every HQC operation rests on the sparse x dense product in F2[X]/(X^n - 1).  Honest traffic does
not reach the places where an implementation of it can be wrong: support position 0 (probability
1/n per vector), the last operand word, bits a malformed pk / ct carries above X^(n-1).  The
records here do, one property each.

Sparse edges (searched over a counter-derived sequence; the first hit is kept):
  pos0      the support contains position 0, drawn as s_0 = 0 (about n tries; a replaced
            duplicate s_0 := 0 also gives it, about n / w tries, but that is the dup property)
  posn1     the support contains position n - 1
  dup       the sampling drew a duplicate, replaced by s_i := i (the small positions)
  align32   the support contains a position k with (n - k) % 32 == 0
for KeyGen as coins whose y has the property:
  kp coins = SHAKE256("qrk-hqc-edge/kg" || alg || LE64(c)), first kp_coins bytes;
for Encaps as (m, salt) coins whose r2 has it under a given public key (theta reads pk[0:80], so
the search is per distinct pk[0:80], the "theta class" of the key):
  enc coins = SHAKE256("qrk-hqc-edge/enc" || alg || class || LE64(c)), first enc_coins bytes.

Dense edges (DENSE), NB = ceil(n / 8) bytes, used as s in a crafted public key
pk = PK_SEED(alg) || s for Encaps and as u in a crafted ciphertext u || v || 0^16 for Decaps:
  zero, x0, xn1 (X^(n-1)), x31, x32, xw1 / xw (X^(32 N32 - 1), X^(32 N32): the two sides of the
  last-word boundary), ones (all n bits), ff (all NB bytes 0xFF, stray bits above n included),
  stray (only the bits above n), aa (0xAA repeated), rand (SHAKE256-seeded).
The ciphertexts take v in V = zero, ff (all bytes 0xFF), rand; (u, v) = (ff, zero) and (zero, ff)
are the pair that shows a leak across the word that straddles from u into v.

Stored: coins, counters, labels and SHA-256 digests of what the pure-Python spec
(oracle/py/hqc_spec.py) computes -- pk and sk, ct || ss, and per secret key the words v - u y, the
shared secrets and the statuses of Decaps on every crafted ciphertext.

    python tests/golden/make_golden_hqc_edge.py
"""
import hashlib
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE.parents[1] / "oracle" / "py")]

import hqc_spec as H  # noqa: E402

ALGS = ("HQC-128", "HQC-192", "HQC-256")
PROPS = ("pos0", "posn1", "dup", "align32")
DENSE = ("zero", "x0", "xn1", "x31", "x32", "xw1", "xw", "ones", "ff", "stray", "aa", "rand")
V = ("zero", "ff", "rand")
MAX_TRIES = 2_000_000


def _shake(tag: str, alg: str, extra: bytes, n: int) -> bytes:
    return hashlib.shake_256(tag.encode() + alg.encode() + extra).digest(n)


def dense(alg: str, label: str) -> bytes:
    """The NB bytes of a dense-edge operand."""
    p = H.params(alg)
    n, nb = p["n"], p["nb"]
    last = 32 * (n >> 5)
    v = {
        "zero": 0, "x0": 1, "xn1": 1 << (n - 1), "x31": 1 << 31, "x32": 1 << 32,
        "xw1": 1 << (last - 1), "xw": 1 << last, "ones": (1 << n) - 1, "ff": (1 << 8 * nb) - 1,
        "stray": ((1 << 8 * nb) - 1) ^ ((1 << n) - 1), "aa": int.from_bytes(b"\xaa" * nb, "little"),
    }.get(label)
    if v is None:
        assert label == "rand"
        return _shake("qrk-hqc-edge/dense", alg, b"", nb)
    return v.to_bytes(nb, "little")


def v_part(alg: str, label: str) -> bytes:
    vb = H.params(alg)["vb"]
    return {"zero": bytes(vb), "ff": b"\xff" * vb}.get(label) or _shake("qrk-hqc-edge/v", alg, b"", vb)


def edge_pk(alg: str, label: str) -> bytes:
    return _shake("qrk-hqc-edge/pkseed", alg, b"", H.SEED_BYTES) + dense(alg, label)


def edge_ct(alg: str, u: str, v: str) -> bytes:
    return dense(alg, u) + v_part(alg, v) + bytes(H.SALT_BYTES)


def theta_class(alg: str, label: str) -> str:
    """The first dense label whose key has the same pk[0:80] (all theta reads of the key)."""
    head = edge_pk(alg, label)[:2 * H.SEED_BYTES]
    return next(d for d in DENSE if edge_pk(alg, d)[:2 * H.SEED_BYTES] == head)


def kg_coins(alg: str, c: int) -> bytes:
    return _shake("qrk-hqc-edge/kg", alg, c.to_bytes(8, "little"), H.params(alg)["kp_coins"])


def enc_coins(alg: str, cls: str, c: int) -> bytes:
    return _shake("qrk-hqc-edge/enc", alg, cls.encode() + c.to_bytes(8, "little"), H.params(alg)["enc_coins"])


def _raw_second(se_seed: bytes, n: int, weight: int) -> list[int]:
    """The second fixed-weight vector of seedexpander(se_seed) before duplicate removal."""
    se = H.SeedExpander(se_seed)
    se.read(4 * weight)
    raw = se.read(4 * weight)
    return [i + ((int.from_bytes(raw[4 * i:4 * i + 4], "little") * (n - i)) >> 32) for i in range(weight)]


def y_of(alg: str, kp_coins: bytes) -> tuple[list[int], list[int]]:
    """(raw, final) support of y = the second vector of seedexpander(sk_seed)."""
    p = H.params(alg)
    raw = _raw_second(kp_coins[:H.SEED_BYTES], p["n"], p["w"])
    se = H.SeedExpander(kp_coins[:H.SEED_BYTES])
    H.fixed_weight_support(se, p["n"], p["w"])
    return raw, H.fixed_weight_support(se, p["n"], p["w"])


def r2_of(alg: str, pk: bytes, coins: bytes) -> tuple[list[int], list[int]]:
    """(raw, final) support of r2 in Encaps(pk, coins), by the spec's own steps."""
    p = H.params(alg)
    m, salt = coins[:p["k"]], coins[p["k"]:p["k"] + H.SALT_BYTES]
    theta = H.shake_ds(bytes(m) + bytes(pk[:2 * H.SEED_BYTES]) + bytes(salt), H.D_G)
    raw = _raw_second(theta[:H.SEED_BYTES], p["n"], p["wr"])
    se = H.SeedExpander(theta[:H.SEED_BYTES])
    H.fixed_weight_support(se, p["n"], p["wr"])
    return raw, H.fixed_weight_support(se, p["n"], p["wr"])


def has_property(alg: str, prop: str, raw: list[int], final: list[int]) -> bool:
    """The named property of a support (raw: as drawn, final: after the spec's duplicate removal)."""
    n = H.params(alg)["n"]
    assert len(set(final)) == len(final)
    if prop == "pos0":
        return raw[0] == 0 and 0 in final
    if prop == "posn1":
        return n - 1 in final
    if prop == "dup":
        return any(f != r and f == i for i, (r, f) in enumerate(zip(raw, final)))
    assert prop == "align32"
    return any((n - k) % 32 == 0 for k in final)


def _prefilter(alg: str, prop: str, raw: list[int]) -> bool:
    """Cheap necessary condition on the raw draw (the search confirms with the spec)."""
    n = H.params(alg)["n"]
    if prop == "pos0":
        return raw[0] == 0
    if prop == "posn1":
        return n - 1 in raw
    if prop == "dup":
        return len(set(raw)) < len(raw)
    return True


def search_kg(alg: str, prop: str) -> int:
    p = H.params(alg)
    for c in range(MAX_TRIES):
        coins = kg_coins(alg, c)
        if _prefilter(alg, prop, _raw_second(coins[:H.SEED_BYTES], p["n"], p["w"])) and \
                has_property(alg, prop, *y_of(alg, coins)):
            return c
    raise AssertionError(f"{alg} kg {prop}: search did not finish")


def search_enc(alg: str, cls: str, prop: str) -> int:
    p = H.params(alg)
    k, n, wr = p["k"], p["n"], p["wr"]
    pk = edge_pk(alg, cls)
    head = bytes(pk[:2 * H.SEED_BYTES])
    for c in range(MAX_TRIES):
        coins = enc_coins(alg, cls, c)
        theta = H.shake_ds(coins[:k] + head + coins[k:k + H.SALT_BYTES], H.D_G)
        if _prefilter(alg, prop, _raw_second(theta[:H.SEED_BYTES], n, wr)) and \
                has_property(alg, prop, *r2_of(alg, pk, coins)):
            return c
    raise AssertionError(f"{alg} enc {cls} {prop}: search did not finish")


def secret_y(alg: str, sk: bytes) -> list[int]:
    p = H.params(alg)
    se = H.SeedExpander(sk[:H.SEED_BYTES])
    H.fixed_weight_support(se, p["n"], p["w"])
    return H.fixed_weight_support(se, p["n"], p["w"])


def decode_word(alg: str, y: list[int], ct: bytes) -> bytes:
    """The n1 n2 bits of v - u y that Decaps hands to the decoder, little-endian."""
    p = H.params(alg)
    u = int.from_bytes(ct[:p["nb"]], "little")
    v = int.from_bytes(ct[p["nb"]:p["nb"] + p["vb"]], "little")
    return ((v ^ H.mul_sparse(y, u, p["n"])) & ((1 << p["n1n2"]) - 1)).to_bytes(p["vb"], "little")


def ct_list(alg: str) -> list[tuple[str, str]]:
    """(u label, v label) of the crafted ciphertexts, in fixture order."""
    return [(u, v) for u in DENSE for v in V]


def decaps_group(alg: str, sk: bytes) -> dict:
    """Digests of Decaps with one secret key on every crafted ciphertext (spec)."""
    y = secret_y(alg, sk)
    t, ss, status = hashlib.sha256(), hashlib.sha256(), []
    for u, v in ct_list(alg):
        ct = edge_ct(alg, u, v)
        t.update(decode_word(alg, y, ct))
        s, rc = H.decaps(alg, sk, ct)
        ss.update(s)
        status.append(rc)
    return {"t": t.hexdigest(), "ss": ss.hexdigest(), "status": status}


def build(alg: str) -> dict:
    kg, groups = [], []
    for prop in PROPS:
        c = search_kg(alg, prop)
        coins = kg_coins(alg, c)
        assert has_property(alg, prop, *y_of(alg, coins))
        pk, sk = H.keypair(alg, coins)
        kg.append({"prop": prop, "c": c, "kp_coins": coins.hex(), "pk": hashlib.sha256(pk).hexdigest(),
                   "sk": hashlib.sha256(sk).hexdigest()})
        groups.append(dict({"sk": prop}, **decaps_group(alg, sk)))
    classes = sorted({theta_class(alg, d) for d in DENSE}, key=DENSE.index)
    enc_c = {cls: {prop: search_enc(alg, cls, prop) for prop in PROPS} for cls in classes}
    enc = []
    for d in DENSE:
        cls, pk = theta_class(alg, d), edge_pk(alg, d)
        for prop in PROPS:
            coins = enc_coins(alg, cls, enc_c[cls][prop])
            assert has_property(alg, prop, *r2_of(alg, pk, coins))
            ct, ss = H.encaps(alg, pk, coins)
            enc.append({"pk": d, "prop": prop, "ct_ss": hashlib.sha256(ct + ss).hexdigest()})
    return {"kg": kg, "enc_counters": enc_c, "enc": enc, "decaps": groups}


def main():
    out = {}
    for alg in ALGS:
        out[alg] = build(alg)
        print(f"{alg}: kg counters {[r['c'] for r in out[alg]['kg']]}, "
              f"enc pos0 counters {[v['pos0'] for v in out[alg]['enc_counters'].values()]}")
    # one record per line
    sets = []
    for alg, d in out.items():
        parts = []
        for key in ("kg", "enc", "decaps"):
            rows = ",\n".join("   " + json.dumps(r, separators=(",", ":")) for r in d[key])
            parts.append(f'  "{key}":[\n{rows}\n  ]')
        parts.insert(1, '  "enc_counters":' + json.dumps(d["enc_counters"], separators=(",", ":")))
        sets.append(f' {json.dumps(alg)}:{{\n' + ",\n".join(parts) + "\n }")
    text = "{\n" + ",\n".join(sets) + "\n}\n"
    assert json.loads(text) == out
    (HERE / "hqc_edge.json").write_text(text)


if __name__ == "__main__":
    main()
