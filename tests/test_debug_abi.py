"""CPU: the test hooks (qrk_dbg_*) have one declaration, csrc/qrkem_debug.h, and one ctypes binding table,
qrkem/_debug.py, and the two agree with each other and with what the library exports.  A hook called with
argtypes unset or one pointer short would get a Python int as a C int, i.e. a truncated device pointer."""
import ctypes as ct
import re

from test_abi import ROOT, declared_functions, exported_symbols

DEBUG_HEADER = ROOT / "quantum-resistant-p2p_amd" / "csrc" / "qrkem_debug.h"
GUARDS = {"QRK_HOST_TRACE": "qrk_dbg_host_trace", "QRK_SS_TRACE": "qrk_dbg_ss_trace", "QRK_HQC_TRACE": "qrk_dbg_hqc_trace"}
SCALARS = {"size_t": ct.c_size_t, "int": ct.c_int, "uint32_t": ct.c_uint32}


def parse(text):
    """name -> parameter kinds ("pointer", "size_t", "int", "uint32_t") of every `int qrk_dbg_*(...);` in text."""
    out = {}
    for name, params in re.findall(r"\bint\s+(qrk_dbg_\w+)\s*\(([^)]*)\)\s*;", text):
        kinds = []
        for p in params.split(","):
            kind = "pointer" if "*" in p else " ".join(p.split()[:-1])  # the last word is the parameter's name
            assert kind == "pointer" or kind in SCALARS, (name, p)
            kinds.append(kind)
        assert name not in out, name
        out[name] = kinds
    return out


def header_hooks():
    """(hooks in every build, hooks under a trace guard), each name -> parameter kinds."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", DEBUG_HEADER.read_text(), flags=re.S)
    blocks = re.findall(r"#if (QRK_\w+_TRACE)\n(.*?)#endif", text, flags=re.S)
    guarded = {}
    for macro, body in blocks:
        hooks = parse(body)
        assert list(hooks) == [GUARDS[macro]], macro
        guarded.update(hooks)
    always = parse(re.sub(r"#if QRK_\w+_TRACE\n.*?#endif", "", text, flags=re.S))
    # every function the header names was parsed, so each returns int and is a plain declaration
    assert sorted(always | guarded) == declared_functions(DEBUG_HEADER)
    return always, guarded


def kind_of(argtype):
    if argtype in (ct.c_void_p, ct.c_char_p) or issubclass(argtype, ct._Pointer):
        return "pointer"
    return next(k for k, t in SCALARS.items() if argtype is t)


def test_header_table_and_library_agree():
    from qrkem import _debug
    always, guarded = header_hooks()
    assert len(always) == 23 and set(guarded) == set(GUARDS.values()) == _debug.TRACE_BUILD
    # 0. the public header declares no hook: this header is their one home
    assert not [n for n in declared_functions() if n.startswith("qrk_dbg_")]
    # 1. nothing is exported undeclared, nothing is declared unbuilt
    exported = {n for n in exported_symbols() if n.startswith("qrk_dbg_")}
    assert exported == set(always) | (set(guarded) & exported)
    # 2. the table has exactly the header's names
    assert set(_debug.HOOKS) == set(always) | set(guarded)
    # 3. and the header's parameters, position by position
    for name, kinds in {**always, **guarded}.items():
        restype, argtypes = _debug.HOOKS[name]
        assert restype is ct.c_int, name
        assert [kind_of(a) for a in argtypes] == kinds, name
    # 4. bind() leaves no exported hook without argtypes
    lib = _debug.bind()
    for name in exported & set(_debug.HOOKS):
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is ct.c_int, name
