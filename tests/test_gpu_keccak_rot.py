"""The lane-per-state Keccak-f[1600] (csrc/keccak.cuh) at the places where its rotation forms can go
wrong, through existing entry points.

Theta's rot-1 in the batched SampleNTT main pass is a 64-bit x + x whose carries travel between the
halves and wrap round, elsewhere two funnel shifts: a mistake shows in bits 0, 31, 32 and 63 only.
Random data reaches those bits too, but the bench-coin sponge's input carries the seed verbatim, so
seeds with exactly those bits set put them into the first column parities.  Everything is integer
work: byte-exact, against hashlib and the C oracle.
"""
import hashlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SEEDS = [0, 1 << 63, (1 << 64) - 1, 0x8000000080000000]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def kem768():
    from qrkem.batch import BatchKEM
    return BatchKEM("ML-KEM-768", device=0)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_bench_coins_match_hashlib(kem768, n, seed):
    """SHAKE256('qrk-bench' || LE64(seed) || LE64(i)) per row, the whole first block (136 bytes,
    the most the entry point gives)."""
    length = 136
    got = _host(kem768.bench_coins(n, length, seed))
    want = np.stack([np.frombuffer(hashlib.shake_256(b"qrk-bench" + seed.to_bytes(8, "little") +
                                                     i.to_bytes(8, "little")).digest(length), np.uint8)
                     for i in range(n)])
    assert np.array_equal(got, want)


def _tamper_quarter(ct, seed):
    bad = ct.copy()
    rng = np.random.default_rng(seed)
    flip = np.arange(ct.shape[0]) % 4 == 1
    for i in np.nonzero(flip)[0]:
        bit = int(rng.integers(0, 8 * bad.shape[1]))
        bad[i, bit // 8] ^= 1 << (bit % 8)
    return bad, flip


@pytest.mark.parametrize("alg,k", [("ML-KEM-768", 3), ("ML-KEM-512", 2)])
def test_mlkem_every_sponge_role(alg, k):
    """KeyGen, Encaps and Decaps (a quarter of the ciphertexts tampered) at n = 257 run H, G, J, PRF
    and SampleNTT in the one-launch kernels; Encaps under a rho whose matrix needs a 4th SHAKE128
    block runs the SampleNTT fix-up, at n = 257 and at n = 1100, where the batched schedule's main
    pass (the carry form of theta) and its fix-up list run."""
    import oracle as orc
    from qrkem.batch import BatchKEM
    from test_gpu_mlkem import _sample_ntt_needs_4th_block  # the rho construction of its fix-up test
    eng = BatchKEM(alg, device=0)
    n = 257
    coins = orc.bench_coins(n, 96, seed=0xC0FFEE + k)
    kc, ec = np.ascontiguousarray(coins[:, :64]), np.ascontiguousarray(coins[:, 64:])
    opk, osk = orc.batch_keypair(alg, kc)
    oct_, oss = orc.batch_encaps(alg, opk, ec)
    pk, sk = eng.keypair(coins=_dev(kc))
    ct, ss = eng.encaps(pk, coins=_dev(ec))
    pk, sk, ct, ss = map(_host, (pk, sk, ct, ss))
    assert np.array_equal(pk, opk) and np.array_equal(sk, osk)
    assert np.array_equal(ct, oct_) and np.array_equal(ss, oss)
    bad, flip = _tamper_quarter(oct_, 5 + k)
    got = _host(eng.decaps(_dev(osk), _dev(bad)))
    assert np.array_equal(got, orc.batch_decaps(alg, osk, bad))
    assert np.array_equal(got[~flip], oss[~flip]) and not np.any(np.all(got[flip] == oss[flip], axis=1))

    rng = np.random.default_rng(77 + k)
    for _ in range(4000):
        rho = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
        if any(_sample_ntt_needs_4th_block(rho, i, j) for i in range(k) for j in range(k)):
            break
    else:
        pytest.fail("no rho with a 4-block SampleNTT entry found")
    fpk = opk.copy()
    fpk[:, -32:] = np.frombuffer(rho, dtype=np.uint8)
    fct, fss = eng.encaps(_dev(fpk), coins=_dev(ec))
    woct, woss = orc.batch_encaps(alg, fpk, ec)
    assert np.array_equal(_host(fct), woct) and np.array_equal(_host(fss), woss)
    n = 1100
    ec = np.ascontiguousarray(orc.bench_coins(n, 32, seed=0xBA7C + k))
    fpk = np.repeat(fpk[:1], n, axis=0)
    fct, fss = eng.encaps(_dev(fpk), coins=_dev(ec))
    woct, woss = orc.batch_encaps(alg, fpk, ec)
    assert np.array_equal(_host(fct), woct) and np.array_equal(_host(fss), woss)


@pytest.mark.parametrize("alg", ["FrodoKEM-640-SHAKE", "HQC-128"])
def test_other_families_roundtrip(alg):
    """The batched FrodoKEM and HQC paths hash with the same permutation."""
    import oracle as orc
    from qrkem.batch import BatchKEM
    eng = BatchKEM(alg, device=0)
    n = 64
    s = orc.sizes(alg)
    kc = orc.bench_coins(n, s["keypair_coins"], seed=811)
    ec = orc.bench_coins(n, s["encaps_coins"], seed=812)
    opk, osk = orc.batch_keypair(alg, kc)
    oct_, oss = orc.batch_encaps(alg, opk, ec)
    pk, sk = eng.keypair(coins=_dev(kc))
    ct, ss = eng.encaps(pk, coins=_dev(ec))
    ss2 = eng.decaps(sk, ct)
    pk, sk, ct, ss, ss2 = map(_host, (pk, sk, ct, ss, ss2))
    assert np.array_equal(pk, opk) and np.array_equal(sk, osk)
    assert np.array_equal(ct, oct_) and np.array_equal(ss, oss) and np.array_equal(ss2, oss)
