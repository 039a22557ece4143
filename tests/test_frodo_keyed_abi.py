"""CPU: the FrodoKEM key-set calls (qrk_frodo_pubkeys_load .. qrk_frodo_decaps_keyed_batch) are exported, declared and
bound, check their arguments in the ML-KEM key sets' order before any device work and say which argument they
refuse; FrodoKeySet and FrodoBatchKEM have the stated surface, make the wrapper checks
before any library call, and BatchKEM itself still has key sets for ML-KEM only."""
import ctypes as ct
import inspect
import re

import pytest

from test_abi import HEADER, declared_functions, exported_symbols

NAMES = ("FrodoKEM-640-SHAKE", "FrodoKEM-640-AES", "FrodoKEM-976-SHAKE", "FrodoKEM-976-AES", "FrodoKEM-1344-SHAKE",
         "FrodoKEM-1344-AES")
CTX = ct.c_void_p(1)  # never dereferenced: every check below comes before the context is used
BUF = ct.c_void_p(8)  # a non-null buffer, never dereferenced either
PUBLIC = {"qrk_frodo_pubkeys_load": 6, "qrk_frodo_seckeys_load": 6, "qrk_frodo_keyset_info": 2,
          "qrk_frodo_keyset_free": 1, "qrk_frodo_encaps_keyed_batch": 9, "qrk_frodo_decaps_keyed_batch": 8}


def load(which, ctx, alg, g, keys=None, out=True):
    from qrkem._native import LIB
    h = ct.c_void_p()
    rc = getattr(LIB, which)(ctx, alg, g, keys, ct.byref(h) if out else None, None)
    assert not h.value  # no handle comes back from a refused load
    return rc


def encaps(ctx, ks, n, bufs=None, index=None):
    from qrkem._native import LIB
    return LIB.qrk_frodo_encaps_keyed_batch(ctx, ks, n, index, bufs, bufs, None, None, None)


def decaps(ctx, ks, n, bufs=None, index=None):
    from qrkem._native import LIB
    return LIB.qrk_frodo_decaps_keyed_batch(ctx, ks, n, index, bufs, bufs, None, None)


def test_symbols_are_exported_declared_and_bound():
    from qrkem._native import LIB
    exported, declared = exported_symbols(), declared_functions()
    text = HEADER.read_text()
    assert "typedef struct qrk_frodo_keyset qrk_frodo_keyset;" in text
    for name, nargs in PUBLIC.items():
        assert name in exported and name in declared and len(getattr(LIB, name).argtypes) == nargs, name
        m = re.search(r"\b(?:int|void)\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, re.S)
        assert m and len(m.group(1).split(",")) == nargs, name


def test_documented_bytes_per_key():
    """The header states the bytes per key; they are the formula of the set's parts."""
    text = " ".join(HEADER.read_text().split())
    for n in (640, 976, 1344):
        for v in (2 * n * n + 16 * n + 32, 2 * n * n + 32 * n + 64):
            assert f"{v:,}" in text, (n, v)


def test_loaders_check_order_and_messages():
    import qrkem
    for which in ("qrk_frodo_pubkeys_load", "qrk_frodo_seckeys_load"):
        for alg in NAMES:
            a = alg.encode()
            # 1. null context, even with everything else wrong too
            assert load(which, None, a, 0) == -1 and "null context" in qrkem.last_error()
            assert load(which, None, b"nonsense", 0, out=False) == -1 and "null context" in qrkem.last_error()
            # 3. g == 0, before the pointers
            assert load(which, CTX, a, 0) == -1 and "at least one key" in qrkem.last_error()
            assert load(which, CTX, a, 0, BUF) == -1 and "at least one key" in qrkem.last_error()
            # 4. null pointers
            assert load(which, CTX, a, 1) == -1 and "null buffer" in qrkem.last_error()
            assert load(which, CTX, a, 1, BUF, out=False) == -1 and "null buffer" in qrkem.last_error()
            # 5. more keys than one allocation may hold
            assert load(which, CTX, a, 1 << 40, BUF) == -1
            assert "scratch budget" in qrkem.last_error() and alg in qrkem.last_error()
        # 2. the name, before g: ML-KEM and HQC are refused by name, anything else as an unsupported KEM
        for a in (b"ML-KEM-768", b"ML-KEM-1024", b"HQC-128", b"HQC-256"):
            assert load(which, CTX, a, 0) == -1
            assert "key sets are FrodoKEM only" in qrkem.last_error() and a.decode() in qrkem.last_error()
        for a in (b"ML-DSA-65", b"FrodoKEM-641-SHAKE", b"FrodoKEM-640", b""):
            assert load(which, CTX, a, 0) == -1 and "unsupported KEM" in qrkem.last_error()
        assert load(which, CTX, None, 1, BUF) == -1 and "unsupported KEM" in qrkem.last_error()


def test_keyed_calls_check_order_and_messages():
    import qrkem
    for call in (encaps, decaps):
        # 1. null context first, whatever else is wrong
        assert call(None, None, 1) == -1 and "null context" in qrkem.last_error()
        assert call(None, BUF, 0) == -1 and "null context" in qrkem.last_error()
        # 2. then the key set: a null one is named, before n == 0 and before the buffers
        for n in (0, 1):
            assert call(CTX, None, n, bufs=BUF) == -1 and "null key set" in qrkem.last_error()
            assert call(CTX, None, n) == -1 and "null key set" in qrkem.last_error()


def test_info_and_free_take_null():
    import qrkem
    from qrkem._native import LIB
    out = (ct.c_size_t * 4)(7, 7, 7, 7)
    assert LIB.qrk_frodo_keyset_info(None, out) == -1 and "null key set" in qrkem.last_error()
    assert list(out) == [7, 7, 7, 7]
    assert LIB.qrk_frodo_keyset_info(None, None) == -1
    LIB.qrk_frodo_keyset_free(None)  # a no-op
    # the ML-KEM loaders refuse FrodoKEM as they did
    h = ct.c_void_p()
    assert LIB.qrk_mlkem_pubkeys_load(CTX, b"FrodoKEM-640-AES", 1, BUF, ct.byref(h), None) == -1
    assert "key sets are ML-KEM only" in qrkem.last_error()


def test_surface():
    import qrkem
    from qrkem.batch import BatchKEM, FrodoBatchKEM, FrodoKeySet, MLKEMKeySet
    assert qrkem.FrodoKeySet is FrodoKeySet and qrkem.FrodoBatchKEM is FrodoBatchKEM
    assert issubclass(FrodoBatchKEM, BatchKEM) and not issubclass(FrodoKeySet, MLKEMKeySet)
    ks = FrodoKeySet(None, "FrodoKEM-976-AES", 3, True)
    assert (ks.g, ks.secret, ks.alg, ks.device, ks.closed, ks.device_bytes) == (3, True, "FrodoKEM-976-AES", 0, True, 0)
    assert "FrodoKeySet" in repr(ks) and "closed" in repr(ks)
    for attr in ("close", "__enter__", "__exit__", "__del__"):
        assert callable(getattr(ks, attr))
    with ks as inner:
        assert inner is ks
    ks.close()  # closing twice is harmless

    def params(f):
        return list(inspect.signature(f).parameters)
    for name in ("load_public_keys", "load_secret_keys", "encaps_keyed", "decaps_keyed"):
        assert name in FrodoBatchKEM.__dict__, name  # overridden, not inherited
        assert params(getattr(FrodoBatchKEM, name)) == params(getattr(BatchKEM, name)), name
        theirs, ours = (inspect.signature(getattr(c, name)).parameters for c in (BatchKEM, FrodoBatchKEM))
        assert [p.default for p in ours.values()] == [p.default for p in theirs.values()], name
    assert params(FrodoBatchKEM.encaps_keyed) == ["self", "keyset", "key_index", "n", "coins", "return_status"]
    assert params(FrodoBatchKEM.decaps_keyed) == ["self", "keyset", "ct_", "key_index", "return_status"]


def _NoDevice(cls, alg):
    """An engine without a context: the wrappers' own checks come before any library call."""
    eng = cls.__new__(cls)
    eng.alg, eng._name, eng.device, eng._ctx = alg, alg.encode(), 0, None
    eng.pk_len = eng.sk_len = eng.ct_len = eng.ss_len = eng.enc_coins = 32
    return eng


def test_batchkem_still_refuses_frodo_and_frodobatchkem_other_names():
    from qrkem.batch import BatchKEM, FrodoBatchKEM, FrodoKeySet, MLKEMKeySet
    for alg in NAMES:
        eng = _NoDevice(BatchKEM, alg)
        for ks in (MLKEMKeySet(None, "ML-KEM-768", 1, False), FrodoKeySet(None, alg, 1, False)):
            for call in (lambda: eng.load_public_keys([bytes(32)]), lambda: eng.load_secret_keys([bytes(32)]),
                         lambda: eng.encaps_keyed(ks, n=1), lambda: eng.decaps_keyed(ks, [bytes(32)])):
                with pytest.raises(ValueError, match="key sets are ML-KEM only: " + re.escape(alg)):
                    call()
    for alg in ("ML-KEM-768", "HQC-128", "Kyber768", ""):
        with pytest.raises(ValueError, match="FrodoBatchKEM is for FrodoKEM names"):
            FrodoBatchKEM(alg)
        eng = _NoDevice(FrodoBatchKEM, alg)
        with pytest.raises(ValueError, match="FrodoBatchKEM is for FrodoKEM names"):
            eng.load_public_keys([bytes(32)])


def test_mismatched_sets_are_value_errors_before_any_gpu_call():
    from qrkem.batch import FrodoBatchKEM, FrodoKeySet, MLKEMKeySet
    alg = "FrodoKEM-976-SHAKE"
    eng = _NoDevice(FrodoBatchKEM, alg)
    pub, sec = FrodoKeySet(None, alg, 1, False), FrodoKeySet(None, alg, 1, True)
    with pytest.raises(ValueError, match="holds FrodoKEM-976-AES keys, this object is FrodoKEM-976-SHAKE"):
        eng.encaps_keyed(FrodoKeySet(None, "FrodoKEM-976-AES", 1, False), n=1)
    with pytest.raises(ValueError, match="secret key set cannot encapsulate"):
        eng.encaps_keyed(sec, n=1)
    for other in (object(), MLKEMKeySet(None, "ML-KEM-768", 1, False)):
        with pytest.raises(ValueError, match="must be a FrodoKeySet"):
            eng.encaps_keyed(other, n=1)
    with pytest.raises(ValueError, match="only for a key set of one key"):
        eng.encaps_keyed(FrodoKeySet(None, alg, 2, False), n=1)
    with pytest.raises(ValueError, match="on device 1"):
        eng.encaps_keyed(FrodoKeySet(None, alg, 1, False, device=1), n=1)
    with pytest.raises(ValueError, match="give key_index, coins or n"):
        eng.encaps_keyed(pub)
    with pytest.raises(ValueError, match="the key set is closed"):
        eng.encaps_keyed(pub, n=1)
    with pytest.raises(ValueError, match="expected a .n, 32. uint8 array"):
        eng.load_public_keys([bytes(31)])
