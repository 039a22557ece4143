"""One-bit tampers aimed at every unit of the Decaps re-encryption compare -- TEST INFRASTRUCTURE.

FrodoKEM and HQC Decaps decrypt, re-encrypt and compare the result with the received ciphertext.  A
one-bit change that the decryption absorbs (mu' = mu, m' = m) is rejected by that compare alone, so a
compare that skipped one word, half a word or a boundary byte would accept a forgery.  This module
builds, from one honest (pk, sk, ct, ss) of the C oracle per parameter set (fixed coins), ciphertexts
that differ from the honest one in exactly one bit, placed so that every unit of the compare is hit:

FrodoKEM (k_fr_pack step 4 compares CT / 8 aligned little-endian 64-bit words; ct = Pack(B') || Pack(C),
fields LOGQ bits wide, MSB first):
  silent  one row per word w: the least significant bit of the first packed coefficient whose LSB lies
          in w.  B'[i][j] +- 1 moves M = C - B'S by one entry of S (at most 12), C +- 1 moves it by 1:
          far inside the decode cell, so mu' = mu and the re-encryption is the honest ciphertext.
  cycle   one row per word w: bit (37 w) mod 64 of the word as the kernel loads it (bit b = bit b % 8 of
          byte 8 w + b / 8): every bit position, both 32-bit halves.  No claim about mu'.
  ends    every bit of the first word, of the last word of Pack(B'), of the first word of Pack(C) and
          of the last word.

HQC (the REENC branch of k_hqc_enc_mul compares u in ceil(NB / 4) 32-bit words from byte 0, the last one
partly v's, and v in VB / 4 words from byte NB, unaligned; ct = u || v || salt):
  word    one row per unit j of that list (u's words, then v's): bit (13 j) mod 32 of the unit, except
          in u's last word, where the bit is (13 j) mod (n mod 32): the bits of u below X^n.
  edge    every bit of every byte within 8 bytes either side of the u | v boundary and of the v | salt
          boundary, and of the first 8 bytes; the stray bits above X^(n-1) of u's last byte are left out
          (tests/test_gpu_hqc.py::test_stray_bits_above_n).
  salt    one bit, (5 i + 1) mod 8, of each salt byte i.
The concatenated code absorbs one flipped bit of v, and the weight-w pattern X^b y a flipped bit of u
adds to v - u y, so m' = m (hqc_mprime checks that against hqc_spec); a salt bit changes theta only.

rows(alg, family) returns (names, ct_bad [rows, ct]); a name gives the family, the byte, the bit of
that byte, and the compare unit.  tests/test_fo_compare_cases.py holds these rows to what they are built
for, on frodo_spec / hqc_spec and the C oracle; tests/test_gpu_fo_compare.py runs the HIP Decaps on them.
"""
import functools

import numpy as np

import frodo_spec as F
import hqc_spec as H

FRODO_ALGS = ["FrodoKEM-640-SHAKE", "FrodoKEM-976-SHAKE", "FrodoKEM-1344-SHAKE", "FrodoKEM-640-AES"]
HQC_ALGS = ["HQC-128", "HQC-192", "HQC-256"]
FRODO_FAMILIES = ("silent", "cycle", "ends")
HQC_FAMILIES = ("word", "edge", "salt")
FAMILIES = {**{a: FRODO_FAMILIES for a in FRODO_ALGS}, **{a: HQC_FAMILIES for a in HQC_ALGS}}


@functools.lru_cache(maxsize=None)
def honest(alg: str) -> dict:
    """pk, sk, ct, ss (bytes) of the C oracle from fixed coins, and msg: the Encaps message (mu / m)."""
    import oracle as orc
    s = orc.sizes(alg)
    pk, sk = orc.keypair(alg, bytes(range(s["keypair_coins"])))
    coins = bytes((7 * i + 3) & 0xFF for i in range(s["encaps_coins"]))
    ct, ss = orc.encaps(alg, pk, coins)
    msg = coins if alg.startswith("Frodo") else coins[:H.params(alg)["k"]]
    return dict(pk=pk, sk=sk, ct=ct, ss=ss, msg=msg)


def _flip(ct: bytes, byte: np.ndarray, bit: np.ndarray) -> np.ndarray:
    out = np.tile(np.frombuffer(ct, np.uint8), (len(byte), 1))
    out[np.arange(len(byte)), byte] ^= (1 << bit).astype(np.uint8)
    return out


# ---------------------------------------------------------------- FrodoKEM
def frodo_unit(byte: int) -> int:
    """The 64-bit word of the compare a ciphertext byte belongs to."""
    return byte // 8


def frodo_positions(alg: str, family: str) -> np.ndarray:
    """(byte, bit of that byte) [rows, 2] of the flipped bit of every row."""
    p = F.params(alg)
    logq, words = p["logq"], p["ct"] // 8
    c1w = logq * p["n"] * F.NBAR // 64  # words of Pack(B'): a whole number for every parameter set
    assert p["ct"] % 8 == 0 and (logq * p["n"] * F.NBAR) % 64 == 0
    if family == "silent":
        lsb = np.arange(p["ct"] * 8 // logq, dtype=np.int64) * logq + logq - 1  # MSB-first stream position
        first = np.searchsorted(lsb // 64, np.arange(words))                    # first coefficient per word
        pos = lsb[first]
        assert np.array_equal(pos // 64, np.arange(words))
        return np.stack([pos // 8, 7 - pos % 8], axis=1)
    if family == "cycle":
        w = np.arange(words, dtype=np.int64)
        b = (37 * w) % 64
        return np.stack([8 * w + b // 8, b % 8], axis=1)
    if family == "ends":
        w = np.repeat(np.array([0, c1w - 1, c1w, words - 1], np.int64), 64)
        b = np.tile(np.arange(64, dtype=np.int64), 4)
        return np.stack([8 * w + b // 8, b % 8], axis=1)
    raise ValueError(family)


def frodo_mu_prime(alg: str, sk: bytes, cts: np.ndarray) -> np.ndarray:
    """frodo_spec's mu' = Decode(C - B'S) of every ciphertext row -> uint8 [rows, len_mu]."""
    import make_golden_frodo_edge as E
    p = F.params(alg)
    n, logq = p["n"], p["logq"]
    off = p["sec"] + p["pk"]
    St = E.signed(np.frombuffer(sk[off:off + 2 * F.NBAR * n], "<u2")).reshape(F.NBAR, n)
    c1 = logq * n * F.NBAR // 8
    out = np.zeros((len(cts), p["len_mu"]), np.uint8)
    for lo in range(0, len(cts), 64):
        part = cts[lo:lo + 64]
        Bp = E.unpack_rows(part[:, :c1], logq).reshape(-1, F.NBAR, n)
        C = E.unpack_rows(part[:, c1:], logq).reshape(-1, F.NBAR, F.NBAR)
        M = (C - Bp @ St.T) & ((1 << logq) - 1)
        for r in range(len(part)):
            out[lo + r] = np.frombuffer(F.decode(p, M[r]), np.uint8)
    return out


# ---------------------------------------------------------------- HQC
def hqc_units(alg: str) -> list[tuple[str, int, int, int]]:
    """The compare's units (part, index, first byte, usable bits): u's 32-bit words from byte 0 (the last
    one holds n mod 32 bits of u), then v's from byte NB."""
    p = H.params(alg)
    nw = (p["nb"] + 3) // 4
    units = [("u", j, 4 * j, 32 if j < nw - 1 else p["n"] - 32 * (nw - 1)) for j in range(nw)]
    assert p["vb"] % 4 == 0 and 0 < units[-1][3] < 32
    return units + [("v", j, p["nb"] + 4 * j, 32) for j in range(p["vb"] // 4)]


def hqc_unit(alg: str, byte: int) -> tuple[str, int]:
    """The compare unit a ciphertext byte belongs to, or ("salt", byte of the salt)."""
    p = H.params(alg)
    if byte < p["nb"]:
        return "u", byte // 4
    if byte < p["nb"] + p["vb"]:
        return "v", (byte - p["nb"]) // 4
    return "salt", byte - p["nb"] - p["vb"]


def hqc_positions(alg: str, family: str) -> np.ndarray:
    p = H.params(alg)
    nb, vb, n = p["nb"], p["vb"], p["n"]
    if family == "word":
        pos = [(first + b // 8, b % 8) for j, (_, _, first, bits) in enumerate(hqc_units(alg))
               for b in [(13 * j) % bits]]
    elif family == "edge":
        spans = [range(0, 8), range(nb - 8, nb + 8), range(nb + vb - 8, nb + vb + 8)]
        top = n - 8 * (nb - 1)  # bits of u in its last byte
        pos = [(byte, bit) for span in spans for byte in span for bit in range(8)
               if not (byte == nb - 1 and bit >= top)]
    elif family == "salt":
        pos = [(nb + vb + i, (5 * i + 1) % 8) for i in range(H.SALT_BYTES)]
    else:
        raise ValueError(family)
    return np.array(pos, np.int64)


class HqcDecoder:
    """hqc_spec's m' = C.decode(v - u y) for many ciphertexts under one sk.  The steps are hqc_spec's own
    (fixed_weight_support, mul_sparse, rm_decode_symbol, rs_decode: what code_decode does); the results
    of the two decoders are memoised by their input, since neighbouring rows share most RM blocks."""

    def __init__(self, alg: str, sk: bytes):
        self.p = p = H.params(alg)
        se = H.SeedExpander(sk[:H.SEED_BYTES])
        H.fixed_weight_support(se, p["n"], p["w"])  # x
        self.y = H.fixed_weight_support(se, p["n"], p["w"])
        self._rm, self._rs = {}, {}

    def mprime(self, ct: bytes) -> bytes:
        p = self.p
        nb, vb, mult = p["nb"], p["vb"], p["mult"]
        u = int.from_bytes(ct[:nb], "little")
        v = int.from_bytes(ct[nb:nb + vb], "little")
        t = (v ^ H.mul_sparse(self.y, u, p["n"])) & ((1 << p["n1n2"]) - 1)
        span = 128 * mult
        mask = (1 << span) - 1
        syms = []
        for i in range(p["n1"]):
            blk = (t >> (span * i)) & mask
            if blk not in self._rm:
                self._rm[blk] = H.rm_decode_symbol(blk, mult)
            syms.append(self._rm[blk])
        key = tuple(syms)
        if key not in self._rs:
            self._rs[key] = bytes(H.rs_decode(p, syms)[p["n1"] - p["k"]:])
        return self._rs[key]


# ---------------------------------------------------------------- rows
def positions(alg: str, family: str) -> np.ndarray:
    return frodo_positions(alg, family) if alg.startswith("Frodo") else hqc_positions(alg, family)


def unit_name(alg: str, byte: int) -> str:
    if alg.startswith("Frodo"):
        return f"word {frodo_unit(byte)}"
    part, j = hqc_unit(alg, byte)
    return f"{part} word {j}" if part != "salt" else f"salt byte {j}"


def rows(alg: str, family: str) -> tuple[list[str], np.ndarray]:
    """(names, ct_bad uint8 [rows, ct]): the honest ciphertext with one bit flipped per row."""
    pos = positions(alg, family)
    names = [f"{family}: byte {byte} bit {bit} ({unit_name(alg, byte)})" for byte, bit in pos.tolist()]
    return names, _flip(honest(alg)["ct"], pos[:, 0], pos[:, 1])
