"""Writes tests/golden/aead.json: AES-256-GCM and ChaCha20-Poly1305 records sealed by OpenSSL.

The reference encrypts with the `cryptography` package (quantum_resistant_p2p/crypto/symmetric.py:
14, 113-116, 211-214), a thin binding over OpenSSL's EVP AEAD interface.  This script calls the same
interface of the machine's libcrypto through ctypes, so the fixture pins the AEAD layer to the library
the reference runs on (its version string is recorded).  Records: key, nonce, aad, pt and
sealed = nonce || ciphertext || tag, hex.  Inputs come from a fixed kat_drbg seed, so the file
regenerates bit-identically:

    python tests/golden/make_golden_aead.py

tests/test_aead_spec.py checks tests/aead_spec.py against this file (and against libcrypto directly
where it loads); the GPU tests check libqrkem against both.
"""
from __future__ import annotations

import ctypes as ct
import ctypes.util
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parents[1] / "oracle" / "py"))

ALGS = ("AES-256-GCM", "ChaCha20-Poly1305")
PT_LENS = (0, 1, 15, 16, 17, 31, 32, 33, 46, 63, 64, 65, 127, 128, 129, 255, 256, 257)
AAD_LENS = (0, 1, 12, 13, 16, 17, 64, 100)
RECORDS = 64

EVP_CTRL_AEAD_SET_IVLEN = 0x9
EVP_CTRL_AEAD_GET_TAG = 0x10


def load_libcrypto():
    """The machine's OpenSSL libcrypto, or None."""
    for name in ("libcrypto.so.3", ctypes.util.find_library("crypto"), "libcrypto.so.1.1"):
        if not name:
            continue
        try:
            lib = ct.CDLL(name)
            lib.EVP_aes_256_gcm, lib.EVP_chacha20_poly1305, lib.EVP_EncryptInit_ex  # noqa: B018
        except (OSError, AttributeError):
            continue
        P, I = ct.c_void_p, ct.c_int
        lib.EVP_CIPHER_CTX_new.restype = P
        lib.EVP_CIPHER_CTX_free.argtypes = [P]
        lib.EVP_aes_256_gcm.restype = P
        lib.EVP_chacha20_poly1305.restype = P
        lib.EVP_EncryptInit_ex.argtypes = [P, P, P, ct.c_char_p, ct.c_char_p]
        lib.EVP_CIPHER_CTX_ctrl.argtypes = [P, I, I, P]
        lib.EVP_EncryptUpdate.argtypes = [P, P, ct.POINTER(I), ct.c_char_p, I]
        lib.EVP_EncryptFinal_ex.argtypes = [P, P, ct.POINTER(I)]
        lib.OpenSSL_version.restype = ct.c_char_p
        return lib
    return None


def openssl_version(lib) -> str:
    return lib.OpenSSL_version(0).decode()


def evp_seal(lib, alg: str, key: bytes, nonce: bytes, pt: bytes, aad: bytes = b"") -> bytes:
    """nonce || ciphertext || tag through EVP_Encrypt* (what AESGCM(key).encrypt / ChaCha20Poly1305(key)
    .encrypt of `cryptography` run, prefixed with the nonce as symmetric.py:119 does)."""
    cipher = lib.EVP_aes_256_gcm() if alg == "AES-256-GCM" else lib.EVP_chacha20_poly1305()
    ctx = lib.EVP_CIPHER_CTX_new()
    try:
        n = ct.c_int(0)
        ok = lib.EVP_EncryptInit_ex(ctx, cipher, None, None, None) == 1
        ok = ok and lib.EVP_CIPHER_CTX_ctrl(ctx, EVP_CTRL_AEAD_SET_IVLEN, len(nonce), None) == 1
        ok = ok and lib.EVP_EncryptInit_ex(ctx, None, None, key, nonce) == 1
        if aad:
            ok = ok and lib.EVP_EncryptUpdate(ctx, None, ct.byref(n), aad, len(aad)) == 1
        out = ct.create_string_buffer(len(pt) + 16)
        ok = ok and lib.EVP_EncryptUpdate(ctx, out, ct.byref(n), pt, len(pt)) == 1
        done = n.value
        ok = ok and lib.EVP_EncryptFinal_ex(ctx, ct.byref(out, done), ct.byref(n)) == 1
        done += n.value
        tag = ct.create_string_buffer(16)
        ok = ok and lib.EVP_CIPHER_CTX_ctrl(ctx, EVP_CTRL_AEAD_GET_TAG, 16, tag) == 1
        if not ok or done != len(pt):
            raise RuntimeError(f"libcrypto {alg} encryption failed")
        return nonce + out.raw[:done] + tag.raw
    finally:
        lib.EVP_CIPHER_CTX_free(ctx)


# Two published vectors lead each cipher's records: RFC 8439 section 2.8.2, and AES-256-GCM with an
# all-zero key, IV and one zero block (test case 14 of the GCM specification's vectors).
PUBLISHED = {
    "ChaCha20-Poly1305": {
        "key": bytes(range(0x80, 0xA0)).hex(),
        "nonce": "070000004041424344454647",
        "aad": "50515253c0c1c2c3c4c5c6c7",
        "pt": (b"Ladies and Gentlemen of the class of '99: If I could offer you only one tip for the future, "
               b"sunscreen would be it.").hex(),
        "tag": "1ae10b594f09e26a7e902ecbd0600691",
    },
    "AES-256-GCM": {
        "key": "00" * 32, "nonce": "00" * 12, "aad": "", "pt": "00" * 16,
        "ct": "cea7403d4d606b6e074ec5d3baf39d18", "tag": "d0d1c8a799996bf0265b98b5d48ab919",
    },
}


def inputs(alg: str):
    """The (key, nonce, aad, pt) of every record of `alg`: the published vector first, then RECORDS
    drawn from the DRBG with every plaintext and AAD length of the lists above."""
    from kat_drbg import KatDrbg
    p = PUBLISHED[alg]
    rows = [tuple(bytes.fromhex(p[k]) for k in ("key", "nonce", "aad", "pt"))]
    drbg = KatDrbg(bytes(range(48)), ("qrkem-aead-golden|" + alg).encode().ljust(48, b"\0"))
    for j in range(RECORDS):
        pt_len = PT_LENS[j % len(PT_LENS)]
        aad_len = AAD_LENS[(5 * j + j // len(PT_LENS)) % len(AAD_LENS)]
        rows.append((drbg.randombytes(32), drbg.randombytes(12), drbg.randombytes(aad_len) if aad_len else b"",
                     drbg.randombytes(pt_len) if pt_len else b""))
    return rows


def generate(lib) -> dict:
    doc = {"openssl": openssl_version(lib), "framing": "sealed = nonce || ciphertext || tag", "records": {}}
    for alg in ALGS:
        recs = []
        for key, nonce, aad, pt in inputs(alg):
            sealed = evp_seal(lib, alg, key, nonce, pt, aad)
            recs.append({"key": key.hex(), "nonce": nonce.hex(), "aad": aad.hex(), "pt": pt.hex(),
                         "sealed": sealed.hex()})
        p = PUBLISHED[alg]
        assert recs[0]["sealed"].endswith(p["tag"]) and recs[0]["sealed"][24:-32] == p.get("ct", recs[0]["sealed"][24:-32])
        doc["records"][alg] = recs
    return doc


def render(doc: dict) -> str:
    return json.dumps(doc, indent=0, sort_keys=True) + "\n"


if __name__ == "__main__":
    lib = load_libcrypto()
    if lib is None:
        sys.exit("no OpenSSL libcrypto found on this machine")
    (HERE / "aead.json").write_text(render(generate(lib)))
    print(f"wrote {HERE / 'aead.json'} ({openssl_version(lib)})")
