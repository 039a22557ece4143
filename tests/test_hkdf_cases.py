"""CPU: the HKDF boundary tables of tests/hkdf_cases.py are right and reach what they claim.

(a) `hkdf_ref` (hmac), oracle/py/hkdf_spec.py (hashlib) and the C oracle's batch_hkdf give the same bytes on
    every case of every table, so the GPU tests may compare with any of them.
(b) Reach, by a model that knows nothing of the kernel: `traced_hkdf` is HKDF written out on bare SHA-256
    that notes, for each of the four kinds of hash, the byte count m after the 64-byte pad block (for the
    hash of a salt above 64 bytes, which has no pad block, the whole message).  SHA-256's padding changes
    shape with m mod 64 at 55 | 56 (0x80 and the length still fit / need a block of their own) and at 63 | 0
    (the padding block holds one last message byte / none), and the number of blocks after the pad block is
    (m + 9 + 63) // 64.  For every kind both sides of both seams occur, and 1, 2 and 3 blocks occur (2 and 3
    for the hashed salt, which is above 64 bytes).  No case is left out.
(c) Every byte of the info rows has bit 7 set, and in the packed batch no row reads the same one byte off.
"""
import hashlib
from collections import defaultdict

import numpy as np
import pytest

import hkdf_cases as K
import hkdf_spec
import oracle as orc

CASES = list(K.all_cases())
KINDS = ("extract", "expand-first", "expand-next", "salt-hash")


def traced_hkdf(salt, ikm, info, L, seen):
    """HKDF-SHA256 on hashlib.sha256 alone; seen[kind] collects m of every inner message."""
    def hmac_(key, msg, kind):
        if len(key) > 64:
            seen["salt-hash"].add(len(key))
            key = hashlib.sha256(key).digest()
        k0 = key.ljust(64, b"\0")
        seen[kind].add(len(msg))
        inner = hashlib.sha256(bytes(x ^ 0x36 for x in k0) + msg).digest()
        return hashlib.sha256(bytes(x ^ 0x5C for x in k0) + inner).digest()

    prk = hmac_(salt or bytes(32), ikm, "extract")
    okm, t = b"", b""
    for r in range(1, (L + 31) // 32 + 1):
        t = hmac_(prk, t + info + bytes([r]), "expand-first" if r == 1 else "expand-next")
        okm += t
    return okm[:L]


def test_three_references_agree_on_every_case():
    for table, salt, ikm, info, L in CASES:
        want = K.hkdf_ref(salt, ikm, info, L)
        assert len(want) == L
        assert hkdf_spec.hkdf_sha256(ikm, info, L, salt) == want, (table, len(ikm), len(info), L)
    # the C oracle, batched: cases that share salt, IKM length and L go in one call
    groups = defaultdict(list)
    for table, salt, ikm, info, L in CASES:
        groups[(salt, len(ikm), L)].append((ikm, info))
    for (salt, ikm_len, L), rows in groups.items():
        ikm = np.frombuffer(b"".join(r[0] for r in rows), np.uint8).reshape(len(rows), ikm_len)
        got = orc.batch_hkdf(ikm, [r[1] for r in rows], L, salt=salt)
        for g, (k, info) in zip(got, rows):
            assert g.tobytes() == K.hkdf_ref(salt, k, info, L), (salt and len(salt), ikm_len, len(info), L)


def test_refused_lengths():
    for L in K.OUT_REFUSED:
        with pytest.raises(ValueError):
            K.hkdf_ref(None, K.OUT_IKM[0], K.INFO_110, L)
        with pytest.raises(ValueError):
            hkdf_spec.hkdf_sha256(K.OUT_IKM[0], K.INFO_110, L)
        with pytest.raises(ValueError):
            orc.hkdf_sha256(K.OUT_IKM[0], K.INFO_110, L)


def test_tables_reach_every_padding_seam_of_every_hash():
    seen = {k: set() for k in KINDS}
    for table, salt, ikm, info, L in CASES:
        assert traced_hkdf(salt, ikm, info, L, seen) == K.hkdf_ref(salt, ikm, info, L), table
    for kind in KINDS:
        classes = {m % 64 for m in seen[kind]}
        assert {55, 56, 63, 0} <= classes, (kind, sorted({55, 56, 63, 0} - classes))
        blocks = {(m + 9 + 63) // 64 for m in seen[kind]}
        assert ({2, 3} if kind == "salt-hash" else {1, 2, 3}) <= blocks, (kind, sorted(blocks))
    assert min(seen["salt-hash"]) == 65  # and 64 is not hashed: the switch is between them
    assert 64 in {len(s) for _, s, *_ in CASES if s}
    # each table alone reaches the seams of the hash it is there for
    def only(table):
        s = {k: set() for k in KINDS}
        for t, salt, ikm, info, L in CASES:
            if t == table:
                traced_hkdf(salt, ikm, info, L, s)
        return {k: {m % 64 for m in v} for k, v in s.items()}
    assert {55, 56, 63, 0} <= only("ikm")["extract"]
    assert {55, 56, 63, 0} <= only("info")["expand-first"] and {55, 56, 63, 0} <= only("info")["expand-next"]
    assert {55, 56, 63, 0} <= only("info-shared")["expand-first"]
    assert {55, 56, 63, 0} <= only("info-shared")["expand-next"]
    assert {55, 56, 63, 0} <= only("salt")["salt-hash"]


def test_tables_are_the_stated_ones():
    assert K.INFO_LENS == list(range(192)) and [len(r) for r in K.INFO_ROWS] == K.INFO_LENS and K.INFO_L == 96
    assert K.IKM_LENS == [1, 31, 32, 33, 54, 55, 56, 63, 64, 65, 118, 119, 120, 127, 128]
    for n in K.IKM_LENS:
        rows = K.ikm_rows(n)
        assert len(rows) == 5 and all(len(r) == n for r in rows) and len(set(rows)) == 5
        assert rows[0] == bytes(n) and rows[1] == b"\xff" * n
    assert len(K.INFO_110) == 110 and K.IKM_L == 32
    assert set(K.SALT_LENS) >= {None, 1, 31, 32, 33, 54, 55, 56, 63, 64, 65, 118, 119, 120, 128, 200}
    assert all(s is None or len(K.salt_of(s)) == s for s in K.SALT_LENS)
    assert K.OUT_LENS == [1, 31, 32, 33, 63, 64, 65, 8129, 8159, 8160] and K.OUT_REFUSED == [0, 8161]
    assert K.SHARED_INFO_LENS == [0, 22, 23, 30, 31, 54, 55, 62, 63, 64, 118, 119]
    assert K.GEOMETRY_N == [1, 255, 256, 257] and len(K.LONG_INFO) == 1000 and K.LONG_L == 64
    ikm, infos = K.geometry_rows(257)
    assert [len(x) for x in infos] == list(range(257)) and len(set(ikm)) == 257


def test_info_rows_have_bit7_set_and_differ_at_their_seams():
    for row in K.INFO_ROWS + [K.LONG_INFO] + K.geometry_rows(257)[1]:
        assert all(b & 0x80 for b in row)
    for i, row in enumerate(K.INFO_ROWS):
        assert row == bytes(0xFF if j % 17 == 16 else 0x80 | ((i + 3 * j) & 0x7F) for j in range(i))
    # packed back to back, a gather that starts one byte early or late reads another string (one that
    # stops early or late hashes another length, whatever the bytes)
    packed = b"".join(K.INFO_ROWS)
    off = 0
    for row in K.INFO_ROWS:
        n = len(row)
        if n and off:
            assert packed[off - 1:off - 1 + n] != row, n
        if n and off + 1 + n <= len(packed):
            assert packed[off + 1:off + 1 + n] != row, n
        off += n


def test_zero_salts_are_one_key_and_65_zeros_another():
    outs = [[K.hkdf_ref(s, ikm, K.INFO_110, K.SALT_L) for ikm in K.SALT_IKM] for s in K.ZERO_SALTS_EQUAL]
    assert all(o == outs[0] for o in outs)
    other = [K.hkdf_ref(K.ZERO_SALT_OTHER, ikm, K.INFO_110, K.SALT_L) for ikm in K.SALT_IKM]
    assert all(a != b for a, b in zip(other, outs[0]))


def test_output_prefix_property():
    for ikm in K.OUT_IKM:
        full = K.hkdf_ref(None, ikm, K.INFO_110, K.MAX_L)
        for L in K.OUT_LENS:
            assert K.hkdf_ref(None, ikm, K.INFO_110, L) == full[:L]
