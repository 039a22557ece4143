"""The two ML-KEM restatements (oracle/src/mlkem.c and oracle/py/mlkem_spec.py) agree byte for byte
on malformed but legal inputs -- the corners tests/test_gpu_mlkem_adversarial.py takes its
expectations from: aliased decapsulation keys, a foreign h, extreme ciphertexts, degenerate keys and
the modulus-check boundary.  CPU only, a few rows per case.
"""
import hashlib

import numpy as np
import pytest

import mlkem_spec as spec
import oracle as orc

ALGS = ["ML-KEM-512", "ML-KEM-768", "ML-KEM-1024"]
Q = 3329


def _fields(b: bytes) -> list:
    acc = int.from_bytes(b, "little")
    return [(acc >> (12 * i)) & 0xFFF for i in range(len(b) * 2 // 3)]


def _bytes(f: list) -> bytes:
    acc = 0
    for i, v in enumerate(f):
        acc |= v << (12 * i)
    return acc.to_bytes(len(f) * 3 // 2, "little")


@pytest.fixture(scope="module", params=ALGS)
def honest(request):
    alg = request.param
    k = spec.PARAMS[alg][0]
    kc = orc.bench_coins(2, 64, seed=0x0A11 + k)
    ec = orc.bench_coins(2, 32, seed=0x0B22 + k)
    keys = [orc.keypair(alg, kc[i].tobytes()) for i in range(2)]
    enc = [orc.encaps(alg, keys[i][0], ec[i].tobytes()) for i in range(2)]
    return alg, k, keys, enc, ec


def _both_decaps(alg, dk: bytes, c: bytes) -> bytes:
    got = orc.decaps(alg, dk, c)
    assert got == spec.decaps(alg, dk, c)
    return got


def test_aliased_dk(honest):
    alg, k, keys, enc, _ = honest
    (ek, dk), (c, ss) = keys[0], enc[0]
    for region, step in ((0, 1), (1, 1), (0, 2)):
        f = _fields(dk[384 * k * region:384 * k * (region + 1)])
        g = [v + Q if v < 4096 - Q and i % step == 0 else v for i, v in enumerate(f)]
        assert g != f and max(g) < 4096
        dk2 = dk[:384 * k * region] + _bytes(g) + dk[384 * k * (region + 1):]
        assert _both_decaps(alg, dk2, c) == ss
        bad = bytearray(c)
        bad[-1] ^= 0x80
        assert _both_decaps(alg, dk2, bytes(bad)) == _both_decaps(alg, dk, bytes(bad)) != ss


def test_foreign_h(honest):
    alg, k, keys, _, ec = honest
    ek, dk = keys[1]
    h = bytes(range(100, 132))
    dk2 = dk[:768 * k + 32] + h + dk[768 * k + 64:]
    m = ec[1].tobytes()
    K, r = spec.G(m + h)
    c = spec.kpke_encrypt(alg, ek, m, r)
    assert _both_decaps(alg, dk2, c) == K
    # under the honest dk the same ciphertext is rejected: h takes part in the re-encryption coins
    assert _both_decaps(alg, dk, c) == spec.J(dk[768 * k + 64:] + c)


def test_extreme_ciphertexts(honest):
    alg, k, keys, enc, _ = honest
    dk = keys[0][1]
    L = len(enc[0][0])
    rng = np.random.default_rng(k)
    for c in (bytes(L), b"\xff" * L, b"\xaa" * L, bytes([0xAA, 0x55] * (L // 2)), rng.integers(0, 256, L, dtype=np.uint8).tobytes()):
        assert _both_decaps(alg, dk, c) == spec.J(dk[768 * k + 64:] + c)


def test_degenerate_keys_and_coins(honest):
    alg, k, keys, _, ec = honest
    rho = keys[0][0][384 * k:]
    cases = [(_bytes([0] * 256 * k), rho, ec[0].tobytes()), (_bytes([Q - 1] * 256 * k), bytes(32), bytes(32)),
             (_bytes([0, Q - 1] * 128 * k), b"\xff" * 32, b"\xff" * 32)]
    for that, r, m in cases:
        ek = that + r
        assert spec.ek_modulus_ok(alg, ek)
        c, ss = orc.encaps(alg, ek, m)
        assert (c, ss) == spec.encaps_derand(alg, ek, m)
    # s_hat = 0, t_hat = 0: v = e2 + mu, so Decaps recovers m and accepts
    ek = cases[0][0] + rho
    c, ss = orc.encaps(alg, ek, ec[0].tobytes())
    dk = bytes(384 * k) + ek + hashlib.sha3_256(ek).digest() + bytes(range(32))
    assert _both_decaps(alg, dk, c) == ss
    for coins in (bytes(64), b"\xff" * 64):
        assert orc.keypair(alg, coins) == spec.keypair_derand(alg, coins)


def test_modulus_check_boundary(honest):
    alg, k, keys, _, ec = honest
    ek = keys[0][0]
    f = _fields(ek[:384 * k])
    m = ec[0].tobytes()
    for pos in (0, 1, 255, 256 * k - 1):
        for v, ok in ((Q - 1, True), (Q, False), (4095, False)):
            g = list(f)
            g[pos] = v
            ek2 = _bytes(g) + ek[384 * k:]
            assert spec.ek_modulus_ok(alg, ek2) == ok
            if ok:
                assert orc.encaps(alg, ek2, m) == spec.encaps_derand(alg, ek2, m)
            else:
                with pytest.raises(RuntimeError):
                    orc.encaps(alg, ek2, m)
