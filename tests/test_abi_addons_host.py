"""The add-on tables of vitssl_hip._lib (ADDON_HEADERS / ADDON_REGISTRY: entry points of libvitssl_hip.so declared under
include_addons/, outside the twelve-header ABI and the extension table) held to the checks of tests/test_abi_mirror_host.py
through tests/_abi_mirror.py, as tests/test_abi_ext_host.py holds the extension table: names, every signature, clean C11,
exported symbols, no collision with the other tables, and that lib() binds them.  The keys are whatever headers the directory
holds: nothing here pins them, a new add-on header is checked the day it appears.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

import _abi_mirror as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDONS = os.path.join(ROOT, "include_addons")
KEYS = sorted(f[len("vitssl_"):-2] for f in os.listdir(ADDONS))          # from the directory listing; every file must be a vitssl_<key>.h


@pytest.fixture(scope="module")
def L():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    from vitssl_hip import _lib
    return _lib


def test_the_add_on_keys_are_the_directory_listing(L):
    assert KEYS and "pool" in KEYS
    assert sorted(os.listdir(ADDONS)) == [f"vitssl_{k}.h" for k in KEYS], "include_addons/ holds something that is no vitssl_<key>.h"
    assert list(L.ADDON_HEADERS) == KEYS == list(L.ADDON_REGISTRY)
    assert not set(L.ADDON_HEADERS) & (set(L.HEADERS) | set(L.EXT_HEADERS))
    for key, path in L.ADDON_HEADERS.items():
        assert path == os.path.join(ADDONS, f"vitssl_{key}.h") and L.header_path(key) == path
    for key, path in list(L.HEADERS.items()) + list(L.EXT_HEADERS.items()):       # header_path resolves all three directories
        assert L.header_path(key) == path
    with pytest.raises(KeyError):
        L.header_path("no_such_header")


def test_build_and_the_isa_diff_tool_know_the_directory(L):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_isa_diff
    assert "include_addons" in kernel_isa_diff.TREES and kernel_isa_diff.TREES[:3] == ("vit-ssl_amd/csrc", "include", "include_ext")
    import __graft_entry__ as ge
    # a touched add-on header rebuilds the objects: build() lists the directory among the dependencies
    src = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "include_addons" in src and "pool.hip" in ge.SOURCES


@pytest.mark.parametrize("key", KEYS)
def test_names(L, key):
    declared = L.declarations(key)
    assert set(declared) == set(L.ADDON_REGISTRY[key]) == set(L.header_symbols(key)) and declared
    # the parser misses no declaration: every `vitssl_x(` left once comments and macros are gone is one of its names
    assert set(re.findall(r"\b(vitssl_[a-z0-9_]+)\s*\(", L.header_text(key))) == set(declared)
    others = list(L.REGISTRY.items()) + list(L.EXT_REGISTRY.items()) + [(k, t) for k, t in L.ADDON_REGISTRY.items() if k != key]
    for other, table in others:
        assert not set(declared) & set(table), (key, other)
    raw = C.CDLL(L.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), f"{name} declared in include_addons/vitssl_{key}.h but not exported"


def test_the_pool_header_declares_its_two_entry_points(L):
    assert L.declarations("pool") == {
        "vitssl_pool_tokens_fwd": ("int", ["const float*", "float*", "int", "int", "int", "void*"]),
        "vitssl_pool_tokens_bwd": ("int", ["const float*", "float*", "int", "int", "int", "void*"])}


@pytest.mark.parametrize("key", KEYS)
def test_signatures(L, key):
    bad = [m for name, d in L.declarations(key).items() for m in M.mismatches(name, d, L.ADDON_REGISTRY[key][name], L.STRUCTS)]
    assert not bad, "\n".join(bad)
    # and the check bites, on every entry point of the table: an int bound as int64_t, a missing parameter, a float result
    for name, (restype, args) in L.ADDON_REGISTRY[key].items():
        d = L.declarations(key)[name]
        wrong = [C.c_int64 if a is C.c_int else C.c_int if a is C.c_int64 else a for a in args]
        if wrong != list(args):
            got = M.mismatches(name, d, (restype, wrong), L.STRUCTS)
            assert got and all(name in line for line in got), name
        assert M.mismatches(name, d, (restype, list(args)[:-1]), L.STRUCTS)
        assert M.mismatches(name, d, (C.c_float, list(args)), L.STRUCTS)


def test_a_deliberately_wrong_pool_binding_is_reported(L):
    d = L.declarations("pool")["vitssl_pool_tokens_fwd"]
    restype, args = L.ADDON_REGISTRY["pool"]["vitssl_pool_tokens_fwd"]
    assert M.mismatches("vitssl_pool_tokens_fwd", d, (restype, args), L.STRUCTS) == []
    wrong = list(args)
    wrong[3] = C.c_int64                                                          # T bound as int64_t
    assert M.mismatches("vitssl_pool_tokens_fwd", d, (restype, wrong), L.STRUCTS) == ["vitssl_pool_tokens_fwd: parameter 3 is 'int', bound as "
                                                                                     + str(C.c_int64)]


@pytest.mark.parametrize("key", KEYS)
def test_header_is_clean_c11_on_its_own_and_adds_no_struct_or_constant(L, key):
    import __graft_entry__ as ge
    hipcc = os.path.realpath(shutil.which(ge.HIPCC) or ge.HIPCC)
    clang = os.path.join(os.path.dirname(os.path.dirname(hipcc)), "lib", "llvm", "bin", "clang")
    assert os.path.exists(clang), f"no clang at {clang} beside {ge.HIPCC}"
    r = subprocess.run([clang, "-x", "c", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", L.ADDON_HEADERS[key]],
                       capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip() and not r.stdout.strip(), r.stderr
    text = L.header_text(key)
    assert "struct" not in text and "enum" not in text
    with open(L.ADDON_HEADERS[key]) as f:
        assert re.findall(r"^\s*#\s*define\s+(\w+)", f.read(), flags=re.M) == [f"VITSSL_{key.upper()}_H"]      # the include guard only


def test_lib_binds_the_add_on_tables_and_the_other_tables_are_what_they_were(L):
    l = L.lib()
    for key in KEYS:
        for name, (restype, argtypes) in L.ADDON_REGISTRY[key].items():
            fn = getattr(l, name)
            assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert sum(len(t) for t in L.REGISTRY.values()) == 95 and len(L.HEADERS) == 12
    assert list(L.EXT_HEADERS) == ["mae"] and len(L.EXT_REGISTRY["mae"]) == 8
    assert L.ABI_VERSION == 3 and l.vitssl_version() == 3
