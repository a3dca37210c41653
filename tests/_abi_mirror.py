"""The comparison of a header declaration with its ctypes binding, shared by tests/test_abi_mirror_host.py (all twelve
headers) and the per-header tests that check their own prototypes.  The C-type table is explicit: a type it does not know is
reported as a mismatch, never accepted."""
import ctypes as C
import re

# C scalar -> the ctypes type of the same width and signedness (parameters, struct-free return types)
SCALARS = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double, "uint32_t": C.c_uint32,
           "uint64_t": C.c_uint64}
# what a `T*` / `const T*` parameter may point at besides a mirrored struct; bound as c_void_p or as POINTER(that type)
POINTEES = {"void": None, "float": C.c_float, "double": C.c_double, "int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64,
            "uint8_t": C.c_uint8, "uint32_t": C.c_uint32}


def accepted(ctype, structs, returned=False):
    """The ctypes types that bind the C type `ctype` correctly (a tuple; empty when the table does not know the type)."""
    if returned and ctype == "const char*":
        return (C.c_char_p,)
    if ctype.endswith("*"):
        base = re.sub(r"^const\s+", "", ctype[:-1]).strip()
        if base in structs:
            return (C.c_void_p, C.POINTER(structs[base]))
        if base in POINTEES:
            return (C.c_void_p,) if POINTEES[base] is None else (C.c_void_p, C.POINTER(POINTEES[base]))
        return ()
    if ctype in structs:
        return (structs[ctype],)                # a struct by value
    return (SCALARS[ctype],) if ctype in SCALARS else ()


def mismatches(name, declared, bound, structs):
    """`declared`: (return type, [parameter types]) as _lib.declarations gives them; `bound`: (restype, argtypes) of the
    registry.  Returns one line per disagreement; an empty list means the binding matches the declaration."""
    (ret, params), (restype, argtypes) = declared, bound
    out = []
    if restype not in accepted(ret, structs, returned=True):
        out.append(f"{name}: returns {ret!r}, bound as {restype}")
    if len(params) != len(argtypes):
        out.append(f"{name}: {len(params)} parameters declared, {len(argtypes)} bound")
    for i, (p, a) in enumerate(zip(params, argtypes)):
        if a not in accepted(p, structs):
            out.append(f"{name}: parameter {i} is {p!r}, bound as {a}")
    return out
