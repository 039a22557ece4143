"""CPU: the arithmetic that decides which sampled matrices a batched ML-KEM KeyGen keeps for the same
context's Decaps (qrk_mlkem_keep_plan over mlkem_keep_plan, csrc/qrkem_internal.h).  Pure host code: no
device is touched.  A kept chunk is its rho tags (32 bytes per row) followed by K^2 384 bytes per row."""
import ctypes as ct

import pytest

from qrkem._native import LIB

K = {"ML-KEM-512": 2, "ML-KEM-768": 3, "ML-KEM-1024": 4}
CONFIGURED = ct.c_size_t(-1).value  # cap_bytes = (size_t)-1: the cap in force


def plan(alg, n, chunk, cap=CONFIGURED):
    out = (ct.c_size_t * 4)()
    assert LIB.qrk_mlkem_keep_plan(alg.encode(), n, chunk, cap, out) == 0
    return tuple(out)  # rows per chunk, batched chunks, kept chunks, kept bytes


def chunk_bytes(alg, rows):
    return rows * (32 + K[alg] ** 2 * 384)


@pytest.fixture(autouse=True)
def default_cap(monkeypatch):
    monkeypatch.delenv("QRK_KEEP_MIB", raising=False)


@pytest.mark.parametrize("alg", sorted(K))
def test_default_cap_covers_one_chunk_of_2p20(alg):
    n = 1 << 20
    assert plan(alg, n, n) == (n, 1, 1, chunk_bytes(alg, n))
    assert chunk_bytes("ML-KEM-1024", n) <= 8192 << 20 < 2 * chunk_bytes("ML-KEM-1024", n)
    # the documented footprint: K^2 384 bytes per handshake, 3.6 GB / 6.4 GB per 2^20 chunk
    assert round(n * 9 * 384 / 1e9, 1) == 3.6 and round(n * 16 * 384 / 1e9, 1) == 6.4


def test_only_batched_chunks_count():
    assert plan("ML-KEM-768", 1024, 1 << 20) == (1024, 0, 0, 0)       # the one-launch kernels
    assert plan("ML-KEM-768", 1025, 1 << 20) == (1088, 1, 1, chunk_bytes("ML-KEM-768", 1088))
    assert plan("ML-KEM-768", 1100, 1 << 20) == (1152, 1, 1, chunk_bytes("ML-KEM-768", 1152))
    assert plan("ML-KEM-768", 5000, 1024)[1:] == (0, 0, 0)            # every chunk small
    assert plan("ML-KEM-768", 0, 1 << 20) == (0, 0, 0, 0)
    # equal chunks of 1088 rows and a last one of 88: 19 batched chunks, the short one is never kept
    assert plan("ML-KEM-768", 20760, 1088) == (1088, 19, 19, 19 * chunk_bytes("ML-KEM-768", 1088))


def test_whole_chunks_in_order_up_to_the_cap():
    one = chunk_bytes("ML-KEM-768", 1536)
    assert plan("ML-KEM-768", 3000, 2048) == (1536, 2, 2, 2 * one)    # 1536 + 1464 rows
    assert plan("ML-KEM-768", 3000, 2048, 2 * one - 1) == (1536, 2, 1, one)
    assert plan("ML-KEM-768", 3000, 2048, one) == (1536, 2, 1, one)
    assert plan("ML-KEM-768", 3000, 2048, one - 1) == (1536, 2, 0, 0)
    assert plan("ML-KEM-768", 3000, 2048, 0) == (1536, 2, 0, 0)


def test_environment_sets_the_cap(monkeypatch):
    monkeypatch.setenv("QRK_KEEP_MIB", "0")
    assert plan("ML-KEM-768", 1100, 1 << 20) == (1152, 1, 0, 0)
    monkeypatch.setenv("QRK_KEEP_MIB", "1")  # 1 MiB: below the 4.0 MB of one 1152-row ML-KEM-768 chunk
    assert plan("ML-KEM-768", 1100, 1 << 20) == (1152, 1, 0, 0)
    monkeypatch.setenv("QRK_KEEP_MIB", "4")
    assert plan("ML-KEM-768", 1100, 1 << 20) == (1152, 1, 1, chunk_bytes("ML-KEM-768", 1152))
    assert plan("ML-KEM-768", 1 << 20, 1 << 20)[2] == 0
    # an explicit cap ignores the environment
    assert plan("ML-KEM-768", 1100, 1 << 20, 0)[2] == 0 and plan("ML-KEM-768", 1100, 1 << 20, 1 << 40)[2] == 1


def test_other_families_are_refused():
    out = (ct.c_size_t * 4)()
    assert LIB.qrk_mlkem_keep_plan(b"HQC-128", 4096, 4096, 0, out) == -1
    assert LIB.qrk_mlkem_keep_plan(b"ML-KEM-768", 4096, 0, 0, out) == -1
