"""CPU: the ML-KEM key-set calls (qrk_mlkem_pubkeys_load .. qrk_mlkem_decaps_keyed_batch) are exported, declared and
bound, check their arguments in the documented order before any device work and say which argument they refuse;
MLKEMKeySet and the keyed BatchKEM methods have the stated surface and refuse FrodoKEM / HQC."""
import ctypes as ct
import inspect
import re

import pytest

from test_abi import HEADER, declared_functions, exported_symbols

NAMES = ("ML-KEM-512", "ML-KEM-768", "ML-KEM-1024")
CTX = ct.c_void_p(1)  # never dereferenced: every check below comes before the context is used
BUF = ct.c_void_p(8)  # a non-null buffer, never dereferenced either
PUBLIC = {"qrk_mlkem_pubkeys_load": 6, "qrk_mlkem_seckeys_load": 6, "qrk_mlkem_keyset_info": 2,
          "qrk_mlkem_keyset_free": 1, "qrk_mlkem_encaps_keyed_batch": 9, "qrk_mlkem_decaps_keyed_batch": 8}


def load(which, ctx, alg, g, keys=None, out=True):
    from qrkem._native import LIB
    h = ct.c_void_p()
    rc = getattr(LIB, which)(ctx, alg, g, keys, ct.byref(h) if out else None, None)
    assert not h.value  # no handle comes back from a refused load
    return rc


def encaps(ctx, ks, n, bufs=None, index=None):
    from qrkem._native import LIB
    return LIB.qrk_mlkem_encaps_keyed_batch(ctx, ks, n, index, bufs, bufs, None, None, None)


def decaps(ctx, ks, n, bufs=None, index=None):
    from qrkem._native import LIB
    return LIB.qrk_mlkem_decaps_keyed_batch(ctx, ks, n, index, bufs, bufs, None, None)


def test_symbols_are_exported_declared_and_bound():
    from qrkem._native import LIB
    exported = exported_symbols()
    declared = declared_functions()
    for name, nargs in PUBLIC.items():
        assert name in exported and name in declared and len(getattr(LIB, name).argtypes) == nargs, name
    text = HEADER.read_text()
    assert "typedef struct qrk_mlkem_keyset qrk_mlkem_keyset;" in text
    # the prototypes' parameter counts are what _native.py binds
    for name, nargs in PUBLIC.items():
        m = re.search(r"\b(?:int|void)\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, re.S)
        assert m and len(m.group(1).split(",")) == nargs, name


def test_loaders_check_order_and_messages():
    import qrkem
    for which in ("qrk_mlkem_pubkeys_load", "qrk_mlkem_seckeys_load"):
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
        # 2. the name, before g: FrodoKEM and HQC are refused by name, anything else as an unsupported KEM
        for a in (b"FrodoKEM-640-AES", b"FrodoKEM-1344-SHAKE", b"HQC-128", b"HQC-256"):
            assert load(which, CTX, a, 0) == -1
            assert "key sets are ML-KEM only" in qrkem.last_error() and a.decode() in qrkem.last_error()
        for a in (b"ML-DSA-65", b"ML-KEM-769", b"Kyber768", b""):
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
    assert LIB.qrk_mlkem_keyset_info(None, out) == -1 and "null key set" in qrkem.last_error()
    assert list(out) == [7, 7, 7, 7]
    assert LIB.qrk_mlkem_keyset_info(None, None) == -1
    LIB.qrk_mlkem_keyset_free(None)  # a no-op
    # the per-row calls are as they were
    assert LIB.qrk_kem_encaps_batch(None, b"ML-KEM-768", 0, None, None, None, None, None, None) == -1
    assert "null context" in qrkem.last_error()


def test_surface():
    import qrkem
    from qrkem.batch import BatchKEM, MLKEMKeySet
    assert qrkem.MLKEMKeySet is MLKEMKeySet and qrkem.BatchKEM is BatchKEM
    ks = MLKEMKeySet(None, "ML-KEM-768", 3, True)
    assert (ks.g, ks.secret, ks.alg, ks.device, ks.closed, ks.device_bytes) == (3, True, "ML-KEM-768", 0, True, 0)
    for attr in ("close", "__enter__", "__exit__", "__del__"):
        assert callable(getattr(ks, attr))
    with ks as inner:
        assert inner is ks
    ks.close()  # closing twice is harmless

    def params(f):
        return list(inspect.signature(f).parameters)
    assert params(BatchKEM.load_public_keys) == ["self", "pk"]
    assert params(BatchKEM.load_secret_keys) == ["self", "sk"]
    assert params(BatchKEM.encaps_keyed) == ["self", "keyset", "key_index", "n", "coins", "return_status"]
    assert params(BatchKEM.decaps_keyed) == ["self", "keyset", "ct_", "key_index", "return_status"]
    for f in (BatchKEM.encaps_keyed, BatchKEM.decaps_keyed):
        defaults = {k: p.default for k, p in inspect.signature(f).parameters.items() if p.default is not p.empty}
        assert defaults.pop("return_status") is False and set(defaults.values()) == {None}


def _NoDevice(alg):
    """A BatchKEM without a context: the wrappers' own checks come before any library call."""
    from qrkem.batch import BatchKEM
    eng = BatchKEM.__new__(BatchKEM)
    eng.alg, eng._name, eng.device, eng._ctx = alg, alg.encode(), 0, None
    eng.pk_len = eng.sk_len = eng.ct_len = eng.ss_len = eng.enc_coins = 32
    return eng


def test_wrappers_raise_on_frodo_and_hqc():
    from qrkem.batch import MLKEMKeySet
    ks = MLKEMKeySet(None, "ML-KEM-768", 1, False)
    for alg in ("FrodoKEM-640-AES", "FrodoKEM-976-SHAKE", "HQC-128", "HQC-256"):
        eng = _NoDevice(alg)
        for call in (lambda: eng.load_public_keys([bytes(32)]), lambda: eng.load_secret_keys([bytes(32)]),
                     lambda: eng.encaps_keyed(ks, n=1), lambda: eng.decaps_keyed(ks, [bytes(32)])):
            with pytest.raises(ValueError, match="key sets are ML-KEM only: " + re.escape(alg)):
                call()


def test_mismatched_sets_are_value_errors_before_any_gpu_call():
    from qrkem.batch import MLKEMKeySet
    eng = _NoDevice("ML-KEM-768")
    pub, sec = MLKEMKeySet(None, "ML-KEM-768", 1, False), MLKEMKeySet(None, "ML-KEM-768", 1, True)
    with pytest.raises(ValueError, match="holds ML-KEM-512 keys, this object is ML-KEM-768"):
        eng.encaps_keyed(MLKEMKeySet(None, "ML-KEM-512", 1, False), n=1)
    with pytest.raises(ValueError, match="secret key set cannot encapsulate"):
        eng.encaps_keyed(sec, n=1)
    with pytest.raises(ValueError, match="must be an MLKEMKeySet"):
        eng.encaps_keyed(object(), n=1)
    with pytest.raises(ValueError, match="only for a key set of one key"):
        eng.encaps_keyed(MLKEMKeySet(None, "ML-KEM-768", 2, False), n=1)
    with pytest.raises(ValueError, match="on device 1"):
        eng.encaps_keyed(MLKEMKeySet(None, "ML-KEM-768", 1, False, device=1), n=1)
    with pytest.raises(ValueError, match="give key_index, coins or n"):
        eng.encaps_keyed(pub)
    with pytest.raises(ValueError, match="the key set is closed"):
        eng.encaps_keyed(pub, n=1)
