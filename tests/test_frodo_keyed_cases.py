"""CPU: the models tests/test_gpu_frodo_keyed.py holds the key-set kernels to (tests/frodo_keyed_cases.py) are right
themselves -- the row grouping on every index pattern the GPU tests use, the limb split on every 16-bit value, and
the plain-arithmetic ciphertext against frodo_spec.encrypt_from_samples."""
import numpy as np
import pytest

import frodo_keyed_cases as K
import frodo_spec as F


def _patterns():
    for g in K.SET_SIZES:
        for n in K.ROW_COUNTS:
            for name, idx in K.index_patterns(g, n).items():
                yield g, n, name, idx
            # the refused-row cases: first row, last row and a tile border
            idx = K.index_patterns(g, n)["mod"].copy()
            for r in {0, n - 1, min(n - 1, K.TILE)}:
                idx[r] = g if r else K.REFUSED
            yield g, n, "refused", idx


def test_grouping_model_on_every_pattern():
    for g, n, name, idx in _patterns():
        perm, tiles, refused = K.group_model(idx, g)
        where = f"g={g} n={n} {name}"
        valid = np.flatnonzero(idx.astype(np.int64) < g)
        # every row with a valid index is in the permutation exactly once, every other row nowhere
        assert sorted(perm.tolist()) == valid.tolist(), where
        assert sorted(refused.tolist()) == sorted(set(range(n)) - set(valid.tolist())), where
        # the tiles partition the permutation in order, never exceed TILE rows and never span two keys
        slot = 0
        for key, first, rows in tiles:
            assert first == slot and 1 <= rows <= K.TILE, where
            assert set(idx[perm[first:first + rows]].tolist()) == {key}, where
            slot += rows
        assert slot == len(perm), where
        # a key's tiles are all full but its last; keys ascend; rows of a key keep their order (stable)
        keys = [t[0] for t in tiles]
        assert keys == sorted(keys), where
        for key in set(keys):
            sizes = [t[2] for t in tiles if t[0] == key]
            assert all(s == K.TILE for s in sizes[:-1]), where
            mine = perm[idx[perm] == key]
            assert mine.tolist() == sorted(mine.tolist()), where
        # no more tiles than the launcher's grid: n / TILE + min(n, g)
        assert len(tiles) <= n // K.TILE + min(n, g), where


def test_grouping_model_lone_row_and_null_index():
    idx = K.index_patterns(17, 65)["lone"]
    perm, tiles, _ = K.group_model(idx, 17)
    assert tiles[0] == (0, 0, 1) and perm[0] == 32 and [t[0] for t in tiles[1:]] == [16] * 4
    perm, tiles, refused = K.group_model(np.zeros(33, np.uint32), 1)  # what a NULL key_index means
    assert perm.tolist() == list(range(33)) and tiles == [(0, 0, 16), (0, 16, 16), (0, 32, 1)] and not len(refused)


def test_limb_split_on_every_value():
    a = np.arange(1 << 16, dtype=np.int64)
    lo, hi = K.limb_split(a)
    assert lo.dtype == np.int8 and hi.dtype == np.int8
    assert np.array_equal((256 * hi.astype(np.int64) + lo.astype(np.int64)) & 0xFFFF, a)
    # the edges: the low limb changes sign at 0x80, the high limb at 0x7F80, and wraps to 0 at 0xFF80
    pick = {0x007F: (127, 0), 0x0080: (-128, 1), 0x00FF: (-1, 1), 0x7F7F: (127, 127), 0x7F80: (-128, -128),
            0x7FFF: (-1, -128), 0x8000: (0, -128), 0xFF7F: (127, -1), 0xFF80: (-128, 0), 0xFFFF: (-1, 0)}
    for v, want in pick.items():
        assert (int(lo[v]), int(hi[v])) == want, hex(v)
    assert set(K.EDGE_VALUES) <= set(pick) | {0}


def test_set_bytes_formula():
    per_key = {640: (829472, 839744), 976: (1920800, 1936448), 1344: (3634208, 3655744)}
    for n, (pub, sec) in per_key.items():
        assert (2 * n * n + 16 * n + 32, 2 * n * n + 32 * n + 64) == (pub, sec)
        for g in (1, 2, 17, 64):
            for secret, key in ((False, pub), (True, sec)):
                b = K.set_bytes(n, secret, g)
                assert g * key + 256 <= b <= g * key + 256 + 5 * 255 and b % 256 == 0


@pytest.mark.parametrize("alg", K.SHAKE)
def test_chosen_matrices_cover_the_borders(alg):
    n = F.params(alg)["n"]
    mats = dict(K.chosen_matrices(alg))
    assert len(mats) == len(K.edge_values(n)) + 10
    R, C = K.border_rows(n), K.border_cols(n)
    assert {0, 63, 64, 127, 128, n - 1} <= set(R) and {0, 15, 16, 127, 128, n - 1} <= set(C)
    used = set()
    for label, A in mats.items():
        if label.startswith("tile borders"):
            nz = np.argwhere(A)
            assert set(nz[:, 0]) == set(R) and set(nz[:, 1]) == set(C)
            used |= set(A[A != 0].tolist())
        if n == 640:
            assert A.max() < 0x8000
    assert used == set(K.edge_values(n)) - {0}
    for label, S in K.sample_patterns(alg):
        assert np.abs(S).max() == K.SMAX[n], label


def test_expected_ct_is_the_specification(monkeypatch):
    """expected_ct from a matrix == frodo_spec.encrypt_from_samples with gen_a returning that matrix."""
    alg = "FrodoKEM-640-SHAKE"
    p = F.params(alg)
    rows = K.edge_rows(alg)
    for i in (0, 13, len(rows["labels"]) - 1):
        key = int(rows["key_index"][i])
        A, pk = rows["matrices"][key], rows["pk"][key].tobytes()
        monkeypatch.setattr(F, "gen_a", lambda p_, s_, A=A: A)
        Sp = rows["s8"][i][:, :p["n"]].astype(np.int64) & 0xFFFF
        Ep = rows["e16"][i].reshape(8, -1).astype(np.int64) & 0xFFFF
        Epp = rows["epp16"][i].reshape(8, 8).astype(np.int64) & 0xFFFF
        Bp, C = F.encrypt_from_samples(p, pk, Sp, Ep, Epp, rows["mu"][i].tobytes())
        want = F.pack(Bp, p["logq"]) + F.pack(C, p["logq"])
        got = K.expected_ct(alg, A, pk, rows["s8"][i], rows["e16"][i], rows["epp16"][i], rows["mu"][i].tobytes())
        assert got == want and len(got) == p["ct"], rows["labels"][i]
    # neighbouring rows name different keys
    assert all(a != b for a, b in zip(rows["key_index"][:-1], rows["key_index"][1:]))
