"""Writes tests/golden/aead_long.json: long AES-256-GCM and ChaCha20-Poly1305 records sealed by OpenSSL.

The long AEAD calls (qrk_aead_seal_long_batch / qrk_aead_open_long_batch) cut a row into segments of S
bytes, C bytes per lane, and combine the segments' partial MACs in a tail tree of fan-in F per lane walk.
The records sit on every boundary of that geometry.  Inputs are not stored: each is
SHAKE256("qrk-aead-long" || alg || LE32(record) || field name) cut to length (`field`).  A record keeps
the plaintext and aad lengths, the tag, SHA-256 of the ciphertext and the ciphertext's first and last 32
bytes, all from libcrypto's EVP interface (make_golden_aead.load_libcrypto / evp_seal), so the file stays
small and regenerates bit-identically:

    python tests/golden/make_golden_aead_long.py

S, C and F are written here, not read from the library: tests/test_aead_long_abi.py checks that
qrk_aead_long_layout still says the same.
"""
from __future__ import annotations

import hashlib
import json
import struct
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

from make_golden_aead import ALGS, evp_seal, load_libcrypto, openssl_version  # noqa: E402

C = 256
S = 256 * C
F = 64  # tail: every lane walks ceil(segments / F) partials, then a tree over the F lanes
PT_LENS = (0, 1, 15, 16, 17, C - 1, C, C + 1, S - 16, S - 1, S, S + 1, S + C + 1, 2 * S - 1, 2 * S, 2 * S + 17,
           3 * S + 5)
AAD_LENS = (0, 1, 13, 16, 100)
# The smallest length at which every level of the tail has two nodes and a ragged last one: F + 1 segments
# make the lane walk two partials long with one lane left a single partial, the tree above it then has 33
# live lanes, and the 17 bytes past F S make the short segment a ragged one.  Below the 8 MiB cap.
TREE_LEN = F * S + 17
assert TREE_LEN <= 8 << 20


def field(alg: str, record: int, name: str, length: int) -> bytes:
    return hashlib.shake_256(b"qrk-aead-long" + alg.encode() + struct.pack("<I", record) + name.encode()).digest(length)


def inputs(alg: str, record: int, pt_len: int, aad_len: int):
    """(key, nonce, aad, pt) of one record."""
    return (field(alg, record, "key", 32), field(alg, record, "nonce", 12), field(alg, record, "aad", aad_len),
            field(alg, record, "pt", pt_len))


def plan():
    """(pt_len, aad_len) of every record of one algorithm, in order."""
    lens = PT_LENS + (TREE_LEN,)
    return [(pt_len, AAD_LENS[j % len(AAD_LENS)]) for j, pt_len in enumerate(lens)]


def summary(alg: str, record: int, pt_len: int, aad_len: int, sealed: bytes) -> dict:
    """What a record keeps of nonce || ct || tag."""
    ct, tag = sealed[12:-16], sealed[-16:]
    assert len(ct) == pt_len
    return {"alg": alg, "record": record, "pt_len": pt_len, "aad_len": aad_len, "tag": tag.hex(),
            "ct_sha256": hashlib.sha256(ct).hexdigest(), "ct_head": ct[:32].hex(), "ct_tail": ct[-32:].hex()}


def generate(lib) -> dict:
    doc = {"openssl": openssl_version(lib), "S": S, "C": C, "F": F,
           "inputs": 'SHAKE256("qrk-aead-long" || alg || LE32(record) || field name), field in key, nonce, aad, pt',
           "records": []}
    for alg in ALGS:
        for record, (pt_len, aad_len) in enumerate(plan()):
            key, nonce, aad, pt = inputs(alg, record, pt_len, aad_len)
            doc["records"].append(summary(alg, record, pt_len, aad_len, evp_seal(lib, alg, key, nonce, pt, aad)))
    return doc


def render(doc: dict) -> str:
    return json.dumps(doc, indent=0, sort_keys=True) + "\n"


if __name__ == "__main__":
    lib = load_libcrypto()
    if lib is None:
        sys.exit("no OpenSSL libcrypto found on this machine")
    (HERE / "aead_long.json").write_text(render(generate(lib)))
    print(f"wrote {HERE / 'aead_long.json'} ({openssl_version(lib)})")
