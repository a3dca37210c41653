"""The extension tables of vitssl_hip._lib (EXT_HEADERS / EXT_REGISTRY: entry points of libvitssl_hip.so declared under
include_ext/, outside the twelve-header ABI) held to the checks of tests/test_abi_mirror_host.py through tests/_abi_mirror.py:
names, every signature, clean C11, exported symbols, no collision with REGISTRY, and that lib() binds them.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

import _abi_mirror as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT_KEYS = ("mae",)
MAE_NAMES = {"vitssl_mae_tokens_fwd", "vitssl_mae_tokens_bwd", "vitssl_mae_unshuffle_fwd", "vitssl_mae_unshuffle_bwd", "vitssl_mae_loss",
             "vitssl_mae_gather_rows_bf16", "vitssl_mae_gather_rows_f32", "vitssl_mae_scatter_rows_f32"}


@pytest.fixture(scope="module")
def L():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    from vitssl_hip import _lib
    return _lib


def test_the_extension_keys_and_where_their_headers_live(L):
    assert tuple(L.EXT_HEADERS) == EXT_KEYS == tuple(L.EXT_REGISTRY)
    assert not set(L.EXT_HEADERS) & set(L.HEADERS)
    assert sorted(os.path.basename(p) for p in L.EXT_HEADERS.values()) == sorted(os.listdir(os.path.join(ROOT, "include_ext")))
    for key, path in L.EXT_HEADERS.items():
        assert path == os.path.join(ROOT, "include_ext", f"vitssl_{key}.h") and L.header_path(key) == path


@pytest.mark.parametrize("key", EXT_KEYS)
def test_names(L, key):
    declared = L.declarations(key)
    assert set(declared) == set(L.EXT_REGISTRY[key]) == set(L.header_symbols(key)) and declared
    assert key != "mae" or set(declared) == MAE_NAMES
    # the parser misses no declaration: every `vitssl_x(` left once comments and macros are gone is one of its names
    assert set(re.findall(r"\b(vitssl_[a-z0-9_]+)\s*\(", L.header_text(key))) == set(declared)
    for other, table in list(L.REGISTRY.items()) + [(k, t) for k, t in L.EXT_REGISTRY.items() if k != key]:
        assert not set(declared) & set(table), (key, other)
    raw = C.CDLL(L.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), f"{name} declared in include_ext/vitssl_{key}.h but not exported"


@pytest.mark.parametrize("key", EXT_KEYS)
def test_signatures(L, key):
    bad = [m for name, d in L.declarations(key).items() for m in M.mismatches(name, d, L.EXT_REGISTRY[key][name], L.STRUCTS)]
    assert not bad, "\n".join(bad)
    # and the check bites: an int64_t bound as int is reported
    restype, args = L.EXT_REGISTRY["mae"]["vitssl_mae_loss"]
    wrong = [C.c_int if a is C.c_int64 else a for a in args]
    assert M.mismatches("vitssl_mae_loss", L.declarations("mae")["vitssl_mae_loss"], (restype, wrong), L.STRUCTS)


@pytest.mark.parametrize("key", EXT_KEYS)
def test_header_is_clean_c11_on_its_own_and_adds_no_struct_or_constant(L, key):
    import __graft_entry__ as ge
    hipcc = os.path.realpath(shutil.which(ge.HIPCC) or ge.HIPCC)
    clang = os.path.join(os.path.dirname(os.path.dirname(hipcc)), "lib", "llvm", "bin", "clang")
    assert os.path.exists(clang), f"no clang at {clang} beside {ge.HIPCC}"
    r = subprocess.run([clang, "-x", "c", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", L.EXT_HEADERS[key]],
                       capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip() and not r.stdout.strip(), r.stderr
    text = L.header_text(key)
    assert "struct" not in text and "enum" not in text
    with open(L.EXT_HEADERS[key]) as f:
        assert re.findall(r"^\s*#\s*define\s+(\w+)", f.read(), flags=re.M) == [f"VITSSL_{key.upper()}_H"]      # the include guard only


def test_lib_binds_the_extension_table_after_the_registry(L):
    l = L.lib()
    for key in EXT_KEYS:
        for name, (restype, argtypes) in L.EXT_REGISTRY[key].items():
            fn = getattr(l, name)
            assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert sum(len(t) for t in L.REGISTRY.values()) == 95 and len(L.HEADERS) == 12      # the twelve-header ABI is what it was


def test_the_ops_wrappers_exist():
    from vitssl_hip import ops
    for name in ("mae_tokens_fwd", "mae_tokens_bwd", "mae_unshuffle_fwd", "mae_unshuffle_bwd", "mae_loss", "mae_gather_rows_bf16",
                 "mae_gather_rows_f32", "mae_scatter_rows_f32"):
        assert callable(getattr(ops, name)), name
