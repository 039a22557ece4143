"""The ML-KEM key-set cases: 65 KeyGen seeds per parameter set, chosen so that at least one key of each set has a
matrix entry that takes the SampleNTT fix-up path (it needs more SHAKE128 blocks than the three the fast path
squeezes), which honest keys do for about 0.7 % of their entries.  Shared by the fixture's generator
(tests/golden/make_golden_mlkem_keyed.py), its CPU check and the GPU test."""
import hashlib
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "oracle" / "py"))
import mlkem_spec as spec  # noqa: E402

FIXTURE = ROOT / "tests" / "golden" / "mlkem_keyed.json"
ALGS = ("ML-KEM-512", "ML-KEM-768", "ML-KEM-1024")
G_KEYS = 65
FAST_BLOCKS = 3  # what the SampleNTT fast path squeezes: 3 x 168 bytes, 336 candidates


def seeds(counter: int) -> list[bytes]:
    """The 65 KeyGen coins d || z of attempt `counter`."""
    return [hashlib.shake_256(b"qrk-mlkem-keyed/kg" + counter.to_bytes(8, "little") + i.to_bytes(8, "little")).digest(64)
            for i in range(G_KEYS)]


def accepted_in_fast_path(b34: bytes) -> int:
    """Candidates below q among the first FAST_BLOCKS blocks of SHAKE128(rho || j || i), capped at 256."""
    stream = hashlib.shake_128(b34).digest(168 * FAST_BLOCKS)
    cnt = 0
    for p in range(0, len(stream), 3):
        c0, c1, c2 = stream[p], stream[p + 1], stream[p + 2]
        cnt += (c0 + 256 * (c1 % 16) < spec.Q) + (c1 // 16 + 16 * c2 < spec.Q)
    return min(cnt, 256)


def fixup_entries(alg: str, coins: bytes) -> list[tuple[int, int]]:
    """The (i, j) of the key's matrix entries that the fast path leaves short of 256 coefficients.  The spec's
    SampleNTT then squeezes further blocks (spec.sample_ntt starts at the same three)."""
    k = spec.PARAMS[alg][0]
    rho, _ = spec.G(coins[:32] + bytes([k]))
    out = []
    for i in range(k):
        for j in range(k):
            b = rho + bytes([j, i])
            if accepted_in_fast_path(b) < 256:
                assert len(spec.sample_ntt(b)) == 256
                out.append((i, j))
    return out


def keys_with_fixup(alg: str, coin_rows) -> list[int]:
    return [t for t, c in enumerate(coin_rows) if fixup_entries(alg, c)]


def load_fixture() -> dict:
    return json.loads(FIXTURE.read_text())
