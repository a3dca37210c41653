"""vitssl_hip._lib mirrors the C ABI in one registry (functions), one mapping (structs) and a few constants; the twelve headers
under include/ are what it is checked against here: names, every signature, every struct layout (against a C program compiled
from the headers), the constants, and that each header is clean C11 on its own.  No GPU."""
import copy
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

import _abi_mirror as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("hip", "transforms", "metrics", "classify", "attention_hd", "patch", "optim", "mixup", "droppath", "layerscale", "lamb", "bce")
CONSTANTS = {"VITSSL_EPI_BF16": "EPI_BF16", "VITSSL_EPI_F32": "EPI_F32", "VITSSL_EPI_GELU": "EPI_GELU", "VITSSL_EPI_RESID": "EPI_RESID",
             "VITSSL_EPI_DGELU": "EPI_DGELU", "VITSSL_EPI_EMBED": "EPI_EMBED", "VITSSL_DROPPATH_SITE_BIT": "DROPPATH_SITE_BIT",
             "VITSSL_DROPPATH_MAX_SITES": "DROPPATH_MAX_SITES", "VITSSL_LAMB_ALWAYS_ADAPT": "LAMB_ALWAYS_ADAPT",
             "VITSSL_LAMB_TRUST_CLIP": "LAMB_TRUST_CLIP"}


@pytest.fixture(scope="module")
def L():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    from vitssl_hip import _lib
    return _lib


@pytest.fixture(scope="module")
def clang():
    import __graft_entry__ as ge
    hipcc = os.path.realpath(shutil.which(ge.HIPCC) or ge.HIPCC)             # the clang that hipcc itself drives
    path = os.path.join(os.path.dirname(os.path.dirname(hipcc)), "lib", "llvm", "bin", "clang")
    assert os.path.exists(path), f"no clang at {path} beside {ge.HIPCC}"
    return path


def header_structs(L):
    """C struct name -> field names in order, from the `typedef struct { ... } name;` of all twelve headers"""
    found = {}
    for key in KEYS:
        for body, name in re.findall(r"typedef\s+struct\s*\{([^{}]*)\}\s*(\w+)\s*;", L.header_text(key)):
            assert name not in found, name
            found[name] = [re.search(r"(\w+)\s*$", d).group(1) for decl in body.split(";") if decl.strip() for d in decl.split(",")]
    return found


def test_the_header_keys_are_these_twelve(L):
    assert tuple(L.HEADERS) == KEYS == tuple(L.REGISTRY)
    assert sorted(os.path.basename(p) for p in L.HEADERS.values()) == sorted(os.listdir(os.path.join(ROOT, "include")))


@pytest.mark.parametrize("key", KEYS)
def test_names(L, key):
    declared = L.declarations(key)
    assert set(declared) == set(L.REGISTRY[key]) == set(L.header_symbols(key)) and declared
    # the parser misses no declaration: every `vitssl_x(` left once comments and macros are gone is one of its names
    assert set(re.findall(r"\b(vitssl_[a-z0-9_]+)\s*\(", L.header_text(key))) == set(declared)
    for other in KEYS:
        assert other == key or not set(declared) & set(L.REGISTRY[other]), (key, other)
    raw = C.CDLL(L.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), f"{name} declared in include/vitssl_{key}.h but not exported"


def test_all_95_functions_are_bound_as_registered(L):
    l = L.lib()
    names = [n for key in KEYS for n in L.REGISTRY[key]]
    assert len(names) == len(set(names)) == 95
    for key in KEYS:
        for name, (restype, argtypes) in L.REGISTRY[key].items():
            fn = getattr(l, name)
            assert fn.restype is restype and list(fn.argtypes) == argtypes, name


@pytest.mark.parametrize("key", KEYS)
def test_signatures(L, key):
    bad = [m for name, d in L.declarations(key).items() for m in M.mismatches(name, d, L.REGISTRY[key][name], L.STRUCTS)]
    assert not bad, "\n".join(bad)


def test_the_signature_check_is_not_vacuous(L):
    reg = copy.deepcopy({k: L.REGISTRY[k] for k in ("hip", "optim")})      # ctypes types copy as themselves
    decl = {k: L.declarations(k) for k in reg}
    restype, args = reg["hip"]["vitssl_cast_bf16"]
    i = args.index(C.c_int64)
    args[i] = C.c_int                                                      # int64_t n truncated to int
    reg["optim"]["vitssl_adamw_segments"][1].pop(5)                        # int nseg gone: everything behind it shifts
    r1 = M.mismatches("vitssl_cast_bf16", decl["hip"]["vitssl_cast_bf16"], reg["hip"]["vitssl_cast_bf16"], L.STRUCTS)
    r2 = M.mismatches("vitssl_adamw_segments", decl["optim"]["vitssl_adamw_segments"], reg["optim"]["vitssl_adamw_segments"], L.STRUCTS)
    assert len(r1) == 1 and f"parameter {i} is 'int64_t'" in r1[0], r1
    assert any("15 parameters declared, 14 bound" in m for m in r2) and any("parameter 5 is 'int'" in m for m in r2), r2
    assert L.REGISTRY["hip"]["vitssl_cast_bf16"][1][i] is C.c_int64        # the registry itself was not touched
    # and a C type the table does not know is a mismatch, whatever it is bound as
    assert M.mismatches("f", ("int", ["size_t"]), (C.c_int, [C.c_size_t]), L.STRUCTS) and M.accepted("long", L.STRUCTS) == ()
    assert M.mismatches("f", ("const char*", []), (C.c_void_p, []), L.STRUCTS)


@pytest.mark.parametrize("key", KEYS)
def test_header_is_clean_c11_on_its_own(L, clang, key):
    r = subprocess.run([clang, "-x", "c", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", L.HEADERS[key]],
                       capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip() and not r.stdout.strip(), r.stderr


@pytest.fixture(scope="module")
def compiled(L, clang, tmp_path_factory):
    """what a C program that includes all twelve headers prints: `S struct size`, `F struct field offset size`, `K name value`"""
    lines = ["#include <stddef.h>", "#include <stdio.h>"] + [f'#include "{os.path.basename(L.HEADERS[k])}"' for k in KEYS]
    lines.append("int main(void) {")
    for s, fields in header_structs(L).items():
        lines.append(f'  printf("S {s} %zu\\n", sizeof({s}));')
        lines += [f'  printf("F {s} {f} %zu %zu\\n", offsetof({s}, {f}), sizeof((({s}*)0)->{f}));' for f in fields]
    lines += [f'  printf("K {k} %lld\\n", (long long)({k}));' for k in CONSTANTS]
    lines += ["  return 0;", "}"]
    d = tmp_path_factory.mktemp("abi_mirror")
    src, exe = d / "layout.c", d / "layout"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run([clang, "-x", "c", "-std=c11", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    return [ln.split() for ln in out.splitlines()]


def test_struct_layouts(L, compiled):
    fields = header_structs(L)
    assert set(fields) == set(L.STRUCTS) and len(fields) == 12
    sizes = {r[1]: int(r[2]) for r in compiled if r[0] == "S"}
    layout = {(r[1], r[2]): (int(r[3]), int(r[4])) for r in compiled if r[0] == "F"}
    assert set(sizes) == set(fields) and len(layout) == sum(len(f) for f in fields.values())
    for s, mirror in L.STRUCTS.items():
        assert [f[0] for f in mirror._fields_] == fields[s], s                       # names and order as the typedef
        assert C.sizeof(mirror) == sizes[s], s
        for f in fields[s]:
            assert (getattr(mirror, f).offset, getattr(mirror, f).size) == layout[s, f], (s, f)


def test_constants(L, compiled):
    got = {r[1]: int(r[2]) for r in compiled if r[0] == "K"}
    assert set(got) == set(CONSTANTS)
    for cname, pyname in CONSTANTS.items():
        assert getattr(L, pyname) == got[cname], cname
    # the enumerators the header has are exactly the six mirrored ones
    assert set(re.findall(r"\bVITSSL_EPI_[A-Z0-9]+\b", L.header_text("hip"))) == {c for c in CONSTANTS if c.startswith("VITSSL_EPI_")}


def test_the_package_still_exports_header_symbols_of_vitssl_hip_h(L):
    import vitssl_hip
    assert vitssl_hip.header_symbols() == L.header_symbols("hip") == sorted(L.REGISTRY["hip"]) and len(vitssl_hip.header_symbols()) == 60
