"""AES-256-GCM and ChaCha20-Poly1305 restated from their specifications -- TEST INFRASTRUCTURE ONLY.

Pure Python (ints for Poly1305 and GF(2^128), a table-free AES-256 with the S-box computed from
the GF(2^8) inverse), so the GPU tests can check libqrkem's AEAD kernels on a machine that has no
libcrypto.  tests/test_aead_spec.py pins this file to OpenSSL through tests/golden/aead.json.

``seal`` / ``open_`` use the reference's framing (quantum_resistant_p2p/crypto/symmetric.py:
116-119, 144-153): sealed = nonce (12) || ciphertext || tag (16).
"""
from __future__ import annotations

import struct
from typing import Optional

ALGS = ("AES-256-GCM", "ChaCha20-Poly1305")
OVERHEAD = 28  # 12-byte nonce + 16-byte tag

# ------------------------------------------------------------------ ChaCha20 (RFC 8439 section 2)
M32 = 0xFFFFFFFF


def _rotl(x: int, n: int) -> int:
    return ((x << n) | (x >> (32 - n))) & M32


def _quarter(s: list, a: int, b: int, c: int, d: int) -> None:
    """RFC 8439 section 2.1."""
    s[a] = (s[a] + s[b]) & M32; s[d] = _rotl(s[d] ^ s[a], 16)
    s[c] = (s[c] + s[d]) & M32; s[b] = _rotl(s[b] ^ s[c], 12)
    s[a] = (s[a] + s[b]) & M32; s[d] = _rotl(s[d] ^ s[a], 8)
    s[c] = (s[c] + s[d]) & M32; s[b] = _rotl(s[b] ^ s[c], 7)


def chacha20_block(key: bytes, counter: int, nonce: bytes) -> bytes:
    """RFC 8439 section 2.3: constants | key | 32-bit block counter | 96-bit nonce, 20 rounds."""
    init = [0x61707865, 0x3320646E, 0x79622D32, 0x6B206574, *struct.unpack("<8I", key), counter & M32,
            *struct.unpack("<3I", nonce)]
    s = list(init)
    for _ in range(10):
        _quarter(s, 0, 4, 8, 12); _quarter(s, 1, 5, 9, 13); _quarter(s, 2, 6, 10, 14); _quarter(s, 3, 7, 11, 15)
        _quarter(s, 0, 5, 10, 15); _quarter(s, 1, 6, 11, 12); _quarter(s, 2, 7, 8, 13); _quarter(s, 3, 4, 9, 14)
    return struct.pack("<16I", *[(x + y) & M32 for x, y in zip(s, init)])


def chacha20_xor(key: bytes, counter: int, nonce: bytes, data: bytes) -> bytes:
    """RFC 8439 section 2.4."""
    out = bytearray()
    for b in range(0, len(data), 64):
        ks = chacha20_block(key, counter + b // 64, nonce)
        out += bytes(x ^ y for x, y in zip(data[b:b + 64], ks))
    return bytes(out)


# ------------------------------------------------------------------ Poly1305 (RFC 8439 section 2.5)
P1305 = (1 << 130) - 5
R_CLAMP = 0x0FFFFFFC0FFFFFFC0FFFFFFC0FFFFFFF


def poly1305(key32: bytes, msg: bytes) -> bytes:
    """RFC 8439 section 2.5.1: key32 = r || s; r is clamped; every block gets a 0x01 byte appended."""
    r = int.from_bytes(key32[:16], "little") & R_CLAMP
    s = int.from_bytes(key32[16:], "little")
    h = 0
    for i in range(0, len(msg), 16):
        blk = msg[i:i + 16]
        h = (h + int.from_bytes(blk + b"\x01", "little")) * r % P1305
    return ((h + s) & ((1 << 128) - 1)).to_bytes(16, "little")


def _pad16(x: bytes) -> bytes:
    return bytes(-len(x) % 16)


def chacha20_poly1305_encrypt(key: bytes, nonce: bytes, pt: bytes, aad: bytes = b"") -> tuple[bytes, bytes]:
    """RFC 8439 section 2.8: one-time key = block 0 (section 2.6), payload from counter 1, tag over
    aad | pad16 | ct | pad16 | le64(len aad) | le64(len ct)."""
    otk = chacha20_block(key, 0, nonce)[:32]
    ct = chacha20_xor(key, 1, nonce, pt)
    mac = aad + _pad16(aad) + ct + _pad16(ct) + struct.pack("<QQ", len(aad), len(ct))
    return ct, poly1305(otk, mac)


def chacha20_poly1305_decrypt(key: bytes, nonce: bytes, ct: bytes, tag: bytes, aad: bytes = b"") -> Optional[bytes]:
    otk = chacha20_block(key, 0, nonce)[:32]
    mac = aad + _pad16(aad) + ct + _pad16(ct) + struct.pack("<QQ", len(aad), len(ct))
    if poly1305(otk, mac) != tag:
        return None
    return chacha20_xor(key, 1, nonce, ct)


# ------------------------------------------------------------------ AES-256 (FIPS 197)
def _xtime(a: int) -> int:
    a <<= 1
    return (a ^ 0x11B) & 0xFF if a & 0x100 else a


def _gf8_mul(a: int, b: int) -> int:
    """FIPS 197 section 4.2: multiplication in GF(2^8) modulo x^8 + x^4 + x^3 + x + 1."""
    r = 0
    while b:
        if b & 1:
            r ^= a
        a = _xtime(a)
        b >>= 1
    return r


def _sub_byte(x: int) -> int:
    """FIPS 197 section 5.1.1: the multiplicative inverse (x^254), then the affine map."""
    inv, b = 1, x
    for bit in range(8):
        if (254 >> bit) & 1:
            inv = _gf8_mul(inv, b)
        b = _gf8_mul(b, b)
    if x == 0:
        inv = 0
    s = inv
    for sh in range(1, 5):
        s ^= ((inv << sh) | (inv >> (8 - sh))) & 0xFF
    return s ^ 0x63


_SB = [_sub_byte(x) for x in range(256)]  # computed at import, not a pasted table


def aes256_expand_key(key: bytes) -> list:
    """FIPS 197 section 5.2, Nk = 8, Nr = 14: 60 words as 15 round keys of 16 bytes."""
    assert len(key) == 32
    w = [list(key[4 * i:4 * i + 4]) for i in range(8)]
    rcon = 1
    for i in range(8, 60):
        t = list(w[i - 1])
        if i % 8 == 0:
            t = [_SB[b] for b in t[1:] + t[:1]]
            t[0] ^= rcon
            rcon = _xtime(rcon)
        elif i % 8 == 4:
            t = [_SB[b] for b in t]
        w.append([a ^ b for a, b in zip(w[i - 8], t)])
    return [sum(w[4 * r:4 * r + 4], []) for r in range(15)]


def aes256_encrypt_block(rk: list, block: bytes) -> bytes:
    """FIPS 197 section 5.1 (Cipher); the state is column-major, s[4 c + row]."""
    s = [b ^ k for b, k in zip(block, rk[0])]
    for r in range(1, 15):
        s = [_SB[b] for b in s]
        s = [s[((c + row) % 4) * 4 + row] for c in range(4) for row in range(4)]  # ShiftRows
        if r != 14:  # MixColumns
            t = []
            for c in range(4):
                a = s[4 * c:4 * c + 4]
                t += [_xtime(a[0]) ^ _xtime(a[1]) ^ a[1] ^ a[2] ^ a[3], a[0] ^ _xtime(a[1]) ^ _xtime(a[2]) ^ a[2] ^ a[3],
                      a[0] ^ a[1] ^ _xtime(a[2]) ^ _xtime(a[3]) ^ a[3], _xtime(a[0]) ^ a[0] ^ a[1] ^ a[2] ^ _xtime(a[3])]
            s = t
        s = [b ^ k for b, k in zip(s, rk[r])]
    return bytes(s)


# ------------------------------------------------------------------ GCM (NIST SP 800-38D)
GCM_R = 0xE1 << 120


def gf128_mul(x: int, y: int) -> int:
    """SP 800-38D section 6.3, Algorithm 1.  Blocks are integers whose most significant bit is
    bit 0 of the block (the coefficient of x^0)."""
    z, v = 0, y
    for i in range(128):
        if (x >> (127 - i)) & 1:
            z ^= v
        v = (v >> 1) ^ GCM_R if v & 1 else v >> 1
    return z


def ghash(h: bytes, data: bytes) -> bytes:
    """SP 800-38D section 6.4, Algorithm 2; len(data) is a multiple of 16."""
    assert len(data) % 16 == 0
    hv, y = int.from_bytes(h, "big"), 0
    for i in range(0, len(data), 16):
        y = gf128_mul(y ^ int.from_bytes(data[i:i + 16], "big"), hv)
    return y.to_bytes(16, "big")


def _gctr(rk: list, icb: bytes, data: bytes) -> bytes:
    """SP 800-38D section 6.5, Algorithm 3, with inc32 (section 6.2) on the last four bytes."""
    out = bytearray()
    head, ctr = icb[:12], int.from_bytes(icb[12:], "big")
    for b in range(0, len(data), 16):
        ks = aes256_encrypt_block(rk, head + ((ctr + b // 16) & M32).to_bytes(4, "big"))
        out += bytes(x ^ y for x, y in zip(data[b:b + 16], ks))
    return bytes(out)


def _gcm_tag(rk: list, nonce: bytes, ct: bytes, aad: bytes) -> bytes:
    h = aes256_encrypt_block(rk, bytes(16))
    s = ghash(h, aad + _pad16(aad) + ct + _pad16(ct) + struct.pack(">QQ", 8 * len(aad), 8 * len(ct)))
    return _gctr(rk, nonce + b"\0\0\0\1", s)


def aes256_gcm_encrypt(key: bytes, nonce: bytes, pt: bytes, aad: bytes = b"") -> tuple[bytes, bytes]:
    """SP 800-38D section 7.1, Algorithm 4, 96-bit IV (J0 = IV || 0^31 || 1), 128-bit tag."""
    assert len(nonce) == 12
    rk = aes256_expand_key(key)
    ct = _gctr(rk, nonce + b"\0\0\0\2", pt)  # inc32(J0)
    return ct, _gcm_tag(rk, nonce, ct, aad)


def aes256_gcm_decrypt(key: bytes, nonce: bytes, ct: bytes, tag: bytes, aad: bytes = b"") -> Optional[bytes]:
    """SP 800-38D section 7.2, Algorithm 5."""
    rk = aes256_expand_key(key)
    if _gcm_tag(rk, nonce, ct, aad) != tag:
        return None
    return _gctr(rk, nonce + b"\0\0\0\2", ct)


# ------------------------------------------------------------------ the reference's framing
_ENC = {"AES-256-GCM": aes256_gcm_encrypt, "ChaCha20-Poly1305": chacha20_poly1305_encrypt}
_DEC = {"AES-256-GCM": aes256_gcm_decrypt, "ChaCha20-Poly1305": chacha20_poly1305_decrypt}


def seal(alg: str, key: bytes, nonce: bytes, pt: bytes, aad: Optional[bytes] = None) -> bytes:
    """nonce || ciphertext || tag, the bytes symmetric.py:116-119 returns."""
    assert len(key) == 32 and len(nonce) == 12
    ct, tag = _ENC[alg](key, nonce, pt, aad or b"")
    return nonce + ct + tag


def open_(alg: str, key: bytes, sealed: bytes, aad: Optional[bytes] = None) -> Optional[bytes]:
    """The plaintext, or None where the row is shorter than 28 bytes or its tag does not verify."""
    if len(sealed) < OVERHEAD:
        return None
    return _DEC[alg](key, sealed[:12], sealed[12:-16], sealed[-16:], aad or b"")
