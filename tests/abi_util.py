"""What the test_*_abi.py files share: the public headers' prototypes against the ctypes tables of
spnerf_amd._*_lib, and the small helpers of their argument-error cases."""
import ctypes
import os
import re

from spnerf_amd import _lib, _ortho_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# non-NULL pointers far apart that are never dereferenced: the arguments are refused first
A, B, C, D = (ctypes.c_void_p(k << 32) for k in (1, 2, 3, 4))
ONE = ctypes.c_void_p(256)

# C type of a prototype (pointers written `T*`) → ctypes; any other `*` type is a c_void_p
C_TYPES = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double,
           "const char*": ctypes.c_char_p, "char*": ctypes.c_char_p,
           "const spnerf_ortho_grid*": ctypes.POINTER(_ortho_lib.OrthoGrid),
           "const spnerf_model_cfg*": ctypes.POINTER(_lib.ModelCfg), "const spnerf_rng*": ctypes.POINTER(_lib.Rng)}
PP = ctypes.POINTER(ctypes.c_void_p)   # `T*const*`: a host list of device pointers


def header_path(name):
    return os.path.join(ROOT, "include", name)


def prototypes(header, prefix="spnerf_"):
    """{name: (return C type, [argument C type, ...])} of every function the file ``header`` declares whose
    name starts with ``prefix``; comments stripped, argument names dropped, `T *x` written `T*`."""
    code = re.sub(r"/\*.*?\*/|//[^\n]*", "", open(header).read(), flags=re.S)
    out = {}
    for res, name, args in re.findall(r"\b(int32_t|int64_t|const char\s*\*)\s*(%s[a-z0-9_]*)\s*\(([^)]*)\)\s*;" % prefix, code):
        types = []
        for a in ([] if args.strip() == "void" else args.split(",")):
            a = re.sub(r"\s*\w+(\[\d*\])?$", lambda m: "*" if m.group(1) else "", " ".join(a.split()))
            types.append(re.sub(r"\s*\*\s*", "*", a))
        out[name] = (re.sub(r"\s*\*", "*", res), types)
    return out


def check_table(module, header, prefix, c_types=None):
    """``module.SIGNATURES`` is ``header``: every prototype has an entry with exactly its ctypes, the
    table has no other entry, the built library exports each, and ``module.lib()`` is the one handle.
    ``c_types`` adds to (or overrides in) C_TYPES; a key may be ``(export, argument index)`` where one
    C type stands for a host array in one export and a device pointer in another.  Returns the
    prototypes' sorted names."""
    types = {**C_TYPES, **(c_types or {})}
    protos = prototypes(header, prefix)
    assert sorted(module.SIGNATURES) == sorted(protos), f"{module.__name__}.SIGNATURES out of sync with {os.path.basename(header)}"
    L = module.lib()
    assert L is _lib.lib()
    for name, (res, args) in protos.items():
        assert hasattr(L, name), name
        for t in args:
            assert t in types or t.endswith("*"), (name, t)
        want = [types.get((name, i), types.get(t, PP if t.endswith("*const*") else ctypes.c_void_p)) for i, t in enumerate(args)]
        got_res, got = module.SIGNATURES[name]
        assert got_res is types[res], (name, res)
        assert got == want, (name, [i for i, (g, w) in enumerate(zip(got, want)) if g is not w], len(got), len(want))
    return sorted(protos)


def defines(header, prefix):
    """{NAME: int} of the header's `#define <prefix>... <integer>` lines (an integer may be in parentheses)."""
    txt = open(header).read()
    return {k: int(v) for k, v in re.findall(r"#define (%s[A-Z0-9_]+) \(?(-?\d+)\)?(?!\w)" % prefix, txt)}


def refused(L, rc, text, what):
    assert rc == _lib.SPNERF_E_ARG == -1, what
    assert text in L.spnerf_last_error(), (what, L.spnerf_last_error())


def grid_of(xsize=15, ysize=9, res=0.5, zone=17, xoff=438638.0, ytop=3353655.0):
    return ctypes.byref(_ortho_lib.OrthoGrid(xoff, ytop, res, xsize, ysize, zone, 0, 1))
