"""CPU: the threaded tests' plans are deterministic and their checker bites (tests/thread_cases.py).

tests/test_gpu_threads.py passes only if thread_cases.check finds nothing and thread_cases.overlaps is above zero.
So here check is shown a result swapped with another thread's, shifted by one row and left at its prefill, and
overlaps a serial log and a hand-made overlapping one: the proof that the GPU tests can fail."""
import copy

import numpy as np
import pytest

import thread_cases as tc


@pytest.fixture(scope="module")
def shared():
    return tc.plan("shared")


def perfect(step):
    """What a correct library returns for the step: the expected outputs, as arrays the way the GPU harness has them."""
    return {k: (v.copy() if isinstance(v, np.ndarray) else list(v)) for k, v in step.want.items()}


@pytest.mark.parametrize("kind", ["shared", "mixed", "errors", "keyed"])
def test_two_builds_of_a_plan_are_equal(kind):
    tc.kem_ref.cache_clear()
    a = tc.fingerprint(tc.plan(kind))
    tc.kem_ref.cache_clear()
    assert tc.fingerprint(tc.plan(kind)) == a


def test_the_fingerprint_sees_one_byte():
    a = tc.plan("keyed")
    b = copy.deepcopy(a)
    b[3][-2].inputs["ct"][16, 1087] ^= 1
    assert tc.fingerprint(a) != tc.fingerprint(b)


def test_shared_plan_shape(shared):
    """Eight threads, four rounds of KeyGen -> Encaps -> Decaps at the issue's row counts, odd threads on host
    pointers, the three parameter sets below 1025 rows and ML-KEM-768 above, and one thread with the half-tampered
    Decaps whose expected keys are the oracle's rejection keys."""
    assert len(shared) == tc.T == 8
    assert {s.alg for steps in shared for s in steps if s.n <= 1024} == set(tc.MLKEM)
    for t, steps in enumerate(shared):
        assert {s.n for s in steps} == {tc.MLKEM_N[t]} and {s.host for s in steps} == {t % 2 == 1}
        assert {s.round for s in steps} == set(range(4))
        if tc.MLKEM_N[t] > 1024:
            assert {s.alg for s in steps} == {"ML-KEM-768"}
        ops = [s.op for s in steps if s.round == 0]
        assert ops[:3] == ["keypair", "encaps", "decaps"] and (ops[3:] == ["decaps_tampered"]) == (t == tc.TAMPER_THREAD)
        # coins are the thread's own: no two threads, and no two rounds, share a key
        assert len({s.inputs["coins"].tobytes() for s in steps if s.op == "keypair"}) == 4
    keys = [s.want["pk"][0].tobytes() for steps in shared for s in steps if s.op == "keypair"]
    assert len(set(keys)) == len(keys) == 32
    for s in shared[tc.TAMPER_THREAD]:
        if s.op == "decaps_tampered":
            flipped = np.any(s.want["ct_tampered"] != s.inputs["ct"], axis=1)
            good = next(x for x in shared[tc.TAMPER_THREAD] if x.round == s.round and x.op == "decaps").want["ss"]
            assert 0.3 < flipped.mean() < 0.7
            assert not np.any(np.all(s.want["ss"][flipped] == good[flipped], axis=1))
            assert np.array_equal(s.want["ss"][~flipped], good[~flipped])


def test_every_thread_of_the_mixed_plan_is_another_family():
    plan = tc.plan("mixed")
    families = [{s.family for s in steps} for steps in plan]
    assert all(len(f) == 1 for f in families) and len(set.union(*families)) == len(plan) == 8
    assert [(steps[0].alg, steps[0].n) for steps in plan[:4]] == [("ML-KEM-512", 300), ("ML-KEM-1024", 1100),
                                                                   ("HQC-128", 64), ("FrodoKEM-640-SHAKE", 8)]
    assert all({s.round for s in steps} == {0, 1, 2} for steps in plan)
    assert {s.op for s in plan[4]} == {"sig_keygen", "sig_sign", "sig_verify"}
    assert {s.op for s in plan[6]} == {"aead_seal", "aead_open", "hkdf"} and {s.op for s in plan[7]} == {"b64_encode", "b64_decode"}
    # the verify steps hold valid and invalid rows, the opens refused ones
    for steps in (plan[4], plan[5]):
        assert all({0, -1} == set(s.want["status"]) for s in steps if s.op == "sig_verify")
    assert all({0, -1} == set(s.want["status"]) for s in plan[6] if s.op == "aead_open")


def test_check_accepts_the_expected_outputs():
    for kind in ("shared", "mixed", "errors", "keyed"):
        for steps in tc.plan(kind):
            for s in steps:
                assert tc.check(s, perfect(s)) is None


def test_check_reports_a_result_swapped_with_another_threads(shared):
    """Thread 2's KeyGen of round 1 returning thread 0's keys (the kept-matrix or staging mix-up this is about), and
    one row of a thread's own result in another row's place."""
    mine, other = shared[2][3], shared[0][3]
    assert mine.op == other.op == "keypair" and mine.alg != other.alg
    msg = tc.check(mine, perfect(other))
    assert msg and "thread 2 round 1 step 3" in msg and "pk" in msg
    # the same parameter set, so the same shapes: threads 5 and 6 (n = 1025, 1100)
    a, b = shared[5][1], shared[6][1]
    got = perfect(a)
    got["ss"][7] = b.want["ss"][7]
    msg = tc.check(a, got)
    assert msg and "thread 5 round 0 step 1" in msg and "ss row 7 differs" in msg
    got = perfect(a)
    got["ct"][[3, 9]] = got["ct"][[9, 3]]
    msg = tc.check(a, got)
    assert msg and "ct row 3 differs (it is the expected row 9)" in msg


def test_check_reports_a_shift_by_one_row(shared):
    s = shared[3][2]
    got = perfect(s)
    got["ss"] = np.roll(got["ss"], 1, axis=0)
    msg = tc.check(s, got)
    assert msg and "thread 3 round 0 step 2" in msg and "ss row 0 differs (it is the expected row 299)" in msg
    got = perfect(s)
    got["ss"][200:] = np.roll(got["ss"][200:], -1, axis=0)
    assert "ss row 200 differs (it is the expected row 201)" in tc.check(s, got)


def test_check_reports_an_output_left_at_its_prefill(shared):
    s = shared[7][1]
    got = perfect(s)
    got["ct"][63] = tc.FILL
    assert "ct row 63 differs (left at its prefill)" in tc.check(s, got)
    got = perfect(s)
    got["status"][5] = tc.STATUS_FILL
    assert "status row 5 differs (left at its prefill)" in tc.check(s, got)
    got = perfect(s)
    del got["ss"]
    assert "no output 'ss'" in tc.check(s, got)
    got = perfect(s)
    got["ss"] = got["ss"][:-1]
    assert "63 rows, expected 64" in tc.check(s, got)


def test_check_sees_one_bit_and_another_threads_error_text():
    plan = tc.plan("errors")
    s = next(x for x in plan[0] if x.op == "fail_unknown_sig")
    got = perfect(s)
    got["error"] = [tc.ERR_KEM.encode()]
    assert "error row 0 differs" in tc.check(s, got)
    s = tc.plan("mixed")[7][0]
    got = perfect(s)
    got["text"][64, -1] ^= 1
    assert "text row 64 differs" in tc.check(s, got)


def test_overlaps():
    ms = 1_000_000
    serial = [(t, (3 * t + k) * ms, (3 * t + k) * ms + ms // 2) for t in range(8) for k in range(3)]
    assert tc.overlaps(serial) == 0
    assert tc.overlaps([]) == 0
    # one thread's own calls never count, however they lie
    assert tc.overlaps([(0, 0, 10), (0, 5, 15), (0, 1, 2)]) == 0
    # A [0, 10] meets B [5, 15] and C [10, 12] (closed intervals); B meets C; D [16, 20] meets nothing
    log = [(0, 0, 10), (1, 5, 15), (2, 10, 12), (3, 16, 20)]
    assert tc.overlaps(log) == 3
    assert tc.overlaps(log[::-1]) == 3
    # one long call across many short ones of two other threads
    log = [(0, 0, 100)] + [(1 + k % 2, 10 * k, 10 * k + 4) for k in range(10)]
    assert tc.overlaps(log) == 10


def test_tamper_is_the_documented_definition():
    ct = np.zeros((200, 1088), np.uint8)
    bad = tc.tamper(ct, 77)
    per_row = np.unpackbits(bad, axis=1).sum(axis=1)
    assert set(per_row) == {0, 1} and 70 < per_row.sum() < 130
    assert np.array_equal(tc.tamper(ct, 77), bad) and not np.array_equal(tc.tamper(ct, 78), bad)
    assert (np.unpackbits(tc.tamper(ct, 77, 1), axis=1).sum(axis=1) == 1).all()
