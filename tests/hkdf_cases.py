"""Boundary tables for HKDF-SHA256 (csrc/hkdf.hip), and a plain reference.  Pure Python, no GPU.

k_hkdf_sha256 is one lane of SHA-256 with hand-rolled padding (sha::tail of csrc/sha2.cuh): each place it
can go wrong is a single length.  Every HMAC inner hash has a 64-byte pad block and then m message bytes;
the padding's 0x80 and the 8-byte length fit the message's last block while m mod 64 <= 55 and take a block
of their own from 56, and at m mod 64 = 0 the padding block holds no message byte at all.  The tables put
lengths on both sides of 55 | 56 and 63 | 0 in each hash the kernel runs:

* extract, H(ipad || IKM): m = len(IKM)                                      -> IKM_LENS
* expand, r = 1, H(ipad || info || 01): m = len(info) + 1                   -> INFO_LENS
* expand, r > 1, H(ipad || T(r-1) || info || r): m = 32 + len(info) + 1     -> INFO_LENS
* a salt above 64 bytes, hashed first, H(salt): no pad block, m = len(salt) -> SALT_LENS

tests/test_hkdf_cases.py proves that reach with a model that knows nothing of the kernel and holds
`hkdf_ref` to oracle/py/hkdf_spec.py and the C oracle on every case; tests/test_gpu_hkdf_edges.py runs
the tables on the device.
"""
import hashlib
import hmac

MAX_L = 255 * 32


def hkdf_ref(salt, ikm, info, L):
    """RFC 5869 on the standard library's hmac alone.  salt None or empty: 32 zero bytes."""
    if not 0 < L <= MAX_L:
        raise ValueError("L must be 1..8160")
    prk = hmac.new(salt or bytes(32), ikm, hashlib.sha256).digest()
    okm, t, r = b"", b"", 1
    while len(okm) < L:
        t = hmac.new(prk, t + info + bytes([r]), hashlib.sha256).digest()
        okm += t
        r += 1
    return okm[:L]


def prand(tag, n):
    """n reproducible bytes named by `tag`."""
    return hashlib.shake_256(b"hkdf_cases|" + tag.encode()).digest(n)


def info_row(i, length=None):
    """Info row i (of length i unless given): byte j is 0x80 | ((i + 3 j) & 0x7F) and every 17th byte is
    0xFF, so every byte has bit 7 set (a sign-extending load shows) and row i ends where row i + 1, which
    starts on another value, begins (an off-by-one gather picks up a wrong byte)."""
    n = i if length is None else length
    return bytes(0xFF if j % 17 == 16 else 0x80 | ((i + 3 * j) & 0x7F) for j in range(n))


# ---- info lengths: one ragged batch, packed back to back, three T blocks
INFO_LENS = list(range(192))
INFO_L = 96
INFO_ROWS = [info_row(i) for i in INFO_LENS]
INFO_IKM = [prand(f"info-ikm-{i}", 32) for i in INFO_LENS]
# the same lengths through the shared-info form (info_off NULL): the seams of r = 1 (54 | 55, 62 | 63),
# of r > 1 (22 | 23, 30 | 31), a whole block and the next seam
SHARED_INFO_LENS = [0, 22, 23, 30, 31, 54, 55, 62, 63, 64, 118, 119]
SHARED_N = 3

# ---- IKM lengths: 5 rows each, the protocol's 110-byte info, one T block
IKM_LENS = [1, 31, 32, 33, 54, 55, 56, 63, 64, 65, 118, 119, 120, 127, 128]
INFO_110 = ("quantum_resistant_p2p-v1-" + "a" * 36 + "-" + "b" * 36 + "-AES-256-GCM").encode()
IKM_L = 32


def ikm_rows(length):
    return [bytes(length), b"\xff" * length] + [prand(f"ikm-{length}-{k}", length) for k in range(3)]


# ---- salt lengths: 64 | 65 switches to a hashed key, whose hash has its own seams at 119 | 120 and 127 | 128
# (127 is what puts m mod 64 = 63 into that hash; no shorter salt is hashed)
SALT_LENS = [None, 1, 31, 32, 33, 54, 55, 56, 63, 64, 65, 118, 119, 120, 127, 128, 200]
SALT_N = 3
SALT_IKM = [prand(f"salt-ikm-{k}", 32) for k in range(SALT_N)]
SALT_L = 32
# RFC 2104 pads a short key with zeros: these four are one key.  65 zero bytes are hashed: another key.
ZERO_SALTS_EQUAL = [None, b"\0", bytes(32), bytes(64)]
ZERO_SALT_OTHER = bytes(65)


def salt_of(length):
    return None if length is None else prand(f"salt-{length}", length)


# ---- output lengths: around one and two T blocks, and the last three lengths there are
OUT_LENS = [1, 31, 32, 33, 63, 64, 65, 8129, 8159, 8160]
OUT_REFUSED = [0, 8161]
OUT_N = 3
OUT_IKM = [prand(f"out-ikm-{k}", 32) for k in range(OUT_N)]

# ---- batch geometry (one workgroup is 256 lanes) and one long info
GEOMETRY_N = [1, 255, 256, 257]
GEOMETRY_L = 33
LONG_INFO = info_row(7, 1000)
LONG_L = 64


def geometry_rows(n):
    """(ikm rows, info rows): row i has an info of i bytes, so no two rows share a length."""
    return [prand(f"geo-ikm-{i}", 32) for i in range(n)], [info_row(i) for i in range(n)]


def all_cases():
    """Every case of every table, one HKDF each: (table, salt, ikm, info, L)."""
    for ikm, info in zip(INFO_IKM, INFO_ROWS):
        yield "info", None, ikm, info, INFO_L
    for n in SHARED_INFO_LENS:
        for ikm in INFO_IKM[:SHARED_N]:
            yield "info-shared", None, ikm, INFO_ROWS[n], INFO_L
    for n in IKM_LENS:
        for ikm in ikm_rows(n):
            yield "ikm", None, ikm, INFO_110, IKM_L
    for salt in [salt_of(n) for n in SALT_LENS] + ZERO_SALTS_EQUAL + [ZERO_SALT_OTHER]:
        for ikm in SALT_IKM:
            yield "salt", salt, ikm, INFO_110, SALT_L
    for L in OUT_LENS:
        for ikm in OUT_IKM:
            yield "out", None, ikm, INFO_110, L
    for ikm, info in zip(*geometry_rows(max(GEOMETRY_N))):
        yield "geometry", None, ikm, info, GEOMETRY_L
    yield "long-info", None, OUT_IKM[0], LONG_INFO, LONG_L
