"""ctypes signatures of the library's test hooks, the qrk_dbg_* functions csrc/qrkem_debug.h declares.

Tests and tools only: ``qrkem/__init__.py`` does not import this module and the product path never
calls a hook (``BatchKEM.hqc_decaps_trace``, a test helper, imports it when called).  ``bind()`` is the one place outside ``_native._bind`` that sets ``argtypes`` on a
library function; tests/test_debug_abi.py checks the table against the header, name by name and
parameter by parameter, so a hook cannot be called with a device pointer narrowed to a C int.
"""
from __future__ import annotations

import ctypes as ct

from ._native import LIB

P, SZ, I, U32 = ct.c_void_p, ct.c_size_t, ct.c_int, ct.c_uint32
_VERIFY_TRACE = [P, ct.c_char_p, SZ, P, P, P, P, P, SZ, P, P, P, P, P, P]

# name -> (restype, argtypes), as in _native._bind
HOOKS = {
    "qrk_dbg_kg_late": (I, [I]),
    "qrk_dbg_fail_launch": (I, [I]),
    "qrk_dbg_ctx_fill": (I, [P, I]),
    "qrk_dbg_fail_after_flip": (I, [I]),
    "qrk_dbg_fixc_words": (I, [P, ct.POINTER(U32), ct.POINTER(I)]),
    "qrk_dbg_kg_flags_residue": (I, [P, ct.POINTER(ct.c_uint64)]),
    "qrk_dbg_mlkem_records_residue": (I, [P, ct.c_char_p, SZ, ct.POINTER(ct.c_uint64)]),
    "qrk_dbg_poly1305_batch": (I, [SZ, P, P, P, P, P]),
    "qrk_dbg_ghash_batch": (I, [SZ, P, P, P, P, P]),
    "qrk_dbg_keys_equal": (I, [SZ, P, P, SZ, P, P]),
    "qrk_dbg_ghash_long_batch": (I, [P, SZ, P, P, P, SZ, P, P]),
    "qrk_dbg_poly1305_long_batch": (I, [P, SZ, P, P, P, SZ, P, P]),
    "qrk_dbg_aead_long_residue": (I, [P, ct.POINTER(ct.c_uint64)]),
    "qrk_dbg_mldsa_sign_trace": (I, [P, ct.c_char_p, SZ, P, P, P, P, P, SZ, P, P, U32, P, P, P]),
    "qrk_dbg_mldsa_verify_trace": (I, _VERIFY_TRACE),
    "qrk_dbg_mldsa_verify_keyed_trace": (I, [P, P, SZ, P, P, P, P, P, SZ, P, P, P, P, P, P]),
    "qrk_dbg_mldsa_sign_keyed_trace": (I, [P, P, SZ, P, P, P, P, P, SZ, P, P, U32, P, P, P]),
    "qrk_dbg_mldsa_keyed_sign_mode": (I, [I]),
    "qrk_dbg_slhdsa_verify_trace": (I, _VERIFY_TRACE),
    "qrk_dbg_frodo_decaps_trace": (I, [P, ct.c_char_p, SZ, P, P, P, P, P]),
    "qrk_dbg_frodo_sample": (I, [P, ct.c_char_p, I, SZ, P, P, P, P, P]),
    "qrk_dbg_frodo_from_samples": (I, [P, ct.c_char_p, I, SZ, P, P, P, P, P, P, P, P]),
    "qrk_dbg_hqc_decaps_trace": (I, [P, ct.c_char_p, SZ, P, P, P, P, P, P]),
    "qrk_dbg_host_trace": (I, [ct.POINTER(ct.c_longlong)]),
    "qrk_dbg_ss_trace": (I, [ct.POINTER(ct.c_ulonglong)]),
    "qrk_dbg_hqc_trace": (I, [ct.POINTER(ct.c_ulonglong)]),
}
# defined only in a -DQRK_HOST_TRACE=1 / -DQRK_SS_TRACE=1 / -DQRK_HQC_TRACE=1 build (tools/build_variant.sh)
TRACE_BUILD = {"qrk_dbg_host_trace", "qrk_dbg_ss_trace", "qrk_dbg_hqc_trace"}


def bind(lib: ct.CDLL = LIB) -> ct.CDLL:
    """Set restype and argtypes of every hook on `lib` and return it.  A trace-build hook the library
    does not export is skipped; any other missing name raises AttributeError, as in _native._bind."""
    for name, (res, args) in HOOKS.items():
        if name in TRACE_BUILD and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib
