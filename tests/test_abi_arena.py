"""No GPU needed: the guarded arena of tests/_arena.py catches what it is there to catch, the case table of
tests/test_gpu_abi_bounds.py covers every launching entry point that include/vitssl_hip.h declares, and every arena test of the
tests/test_gpu_*_bounds.py files has an off-stream twin (tests/_offstream.py) that leaves no entry point of any header out."""
import glob
import importlib
import inspect
import os
import re
import types

import pytest
import torch

from _arena import ALIGN, GUARD_MIN, GUARD_ROWS, Arena, ArenaError

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vitssl_hip.h")


def _arena():
    a = Arena("cpu", mib=4)
    x = a.put("x", torch.randn(37, 100))
    y = a.empty("y", (5, 260), torch.bfloat16)
    s = a.empty("scalar", (1,), torch.float32)
    return a, x, y, s


def test_arena_layout_and_poison():
    a, x, y, s = _arena()
    for t in (x, y, s):
        assert t.is_contiguous() and t.data_ptr() % ALIGN == 0
    assert a.dtypes == [torch.float32, torch.bfloat16, torch.float32]                    # one element type a region, in carving order
    assert torch.isnan(y.float()).all() and torch.isnan(s).all()                         # 0xFF is NaN as bf16 and fp32
    assert torch.isnan(a.empty("e", (8,), torch.float8_e4m3fn).float()).all()            # and as e4m3fn
    assert int(a.empty("i", (3,), torch.int32)[0]) == -1 and int(a.empty("u", (3,), torch.uint8)[0]) == 255
    regs = a.regions
    assert len(a.dtypes) == len(regs) and a.dtypes[3:] == [torch.float8_e4m3fn, torch.int32, torch.uint8]
    assert regs[0][1] >= max(GUARD_ROWS * 100 * 4, GUARD_MIN)                            # guard in front of the first tensor
    for (n0, s0, e0, g0), (n1, s1, e1, g1) in zip(regs, regs[1:]):
        assert s1 - e0 >= max(g0, g1), (n0, n1)                                          # both neighbours' conditions hold
    assert a.top <= a.buf.numel()
    for name, st, en, g in regs:                                                          # guards are 0xFF right up to the tensor
        assert g >= GUARD_MIN and bool((a.buf[st - g:st] == 0xFF).all()) and bool((a.buf[en:en + g] == 0xFF).all())
    a.check()
    assert not Arena.untouched(x) and Arena.untouched(y)
    Arena.fill(y, 0)
    assert float(y.float().abs().sum()) == 0.0
    a.check()                                                                             # writes inside a tensor are fine
    with pytest.raises(ArenaError, match="too small"):
        a.empty("big", (1 << 22,), torch.float32)


@pytest.mark.parametrize("side", ["before", "after"])
def test_arena_catches_a_one_byte_stray_write(side):
    a, x, y, s = _arena()
    _, st, en, _ = next(r for r in a.regions if r[0] == "y")
    a.buf[st - 1 if side == "before" else en] = 0
    want = "1 bytes before the start of 'y'" if side == "before" else "0 bytes after the end of 'y'"
    with pytest.raises(ArenaError, match=want) as e:
        a.check()
    assert "1 guard bytes overwritten" in str(e.value)


def test_arena_reports_a_hit_far_from_any_tensor():
    a, *_ = _arena()
    a.buf[a.buf.numel() - 1] = 7
    with pytest.raises(ArenaError, match="outside every guard"):
        a.check()


# ---------------------------------------------------------------------------------------------- completeness of the case table
def _prototypes():
    """name -> parameter text of every function of the header"""
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(?:int|int64_t|const char\*)\s+(vitssl_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", txt)}


def test_every_launching_entry_point_has_a_case():
    import test_gpu_abi_bounds as T
    protos = _prototypes()
    assert len(protos) >= 60 and "vitssl_gemm_bf16_nt" in protos and "vitssl_aug_blur_to_tensor" in protos
    launching = {n for n, args in protos.items() if re.search(r"void\s*\*\s*stream", args)}
    assert len(launching) >= 45
    covered = {c.entry for c in T.CASES}
    assert not (launching - covered), f"entry points without a case in tests/test_gpu_abi_bounds.py: {sorted(launching - covered)}"
    assert not (covered - launching), f"cases of unknown entry points: {sorted(covered - launching)}"
    # entry points that take a sized workspace / scratch pointer (the two NT GEMMs take theirs inside vitssl_gemm_t): at least
    # one case each with the exact-size, poisoned-workspace, repeat-bits and one-float-short steps (Case.ws and Case.det).
    # vitssl_attn_bwd's delta_ws has no size argument: its cases carve it as exactly [B, H, N] and compare bits (Case.det).
    sized = {n for n in launching if re.search(r"\b(workspace|t_ws)_floats\b", protos[n]) or "vitssl_gemm_t*" in protos[n].replace(" *", "*")}
    assert {"vitssl_layernorm_bwd", "vitssl_gemm_bf16_nt", "vitssl_gemm_fp8_nt", "vitssl_dino_loss", "vitssl_embed_bwd"} <= sized
    assert len(sized) >= 14, sorted(sized)
    for n in sorted(sized):
        assert any(c.entry == n and c.ws and c.det for c in T.CASES), f"{n}: no case with the workspace steps"
    assert any(c.entry == "vitssl_attn_bwd" and c.det for c in T.CASES)
    for c in T.CASES:
        assert c.bar, c.id
        assert not c.ws or c.entry in sized, f"{c.id}: workspace steps on an entry point without a sized workspace"


# ---------------------------------------------------------------------------------------------- completeness of the off-stream twins
TESTS = os.path.dirname(os.path.abspath(__file__))
ARENA_TEST = re.compile(r"test_abi_case|test_transforms_abi_case|test_on_the_arena|test_\w+_on_the_arena")


def _params(test):
    return [m.args for m in getattr(test, "pytestmark", []) if m.name == "parametrize" and m.args[0] != "mode"]


def _reached(fn, seen):
    """entry points named in `fn` or in the functions of tests/ it names: quoted, as `.vitssl_x(` or through a module constant"""
    if fn in seen:
        return set()
    seen.add(fn)
    src = inspect.getsource(fn)
    found = set(re.findall(r"[\"'](vitssl_[a-z0-9_]+)[\"']", src)) | set(re.findall(r"\.(vitssl_[a-z0-9_]+)\(", src))
    for ident in set(re.findall(r"\b[A-Za-z_]\w*\b", src)):
        v = fn.__globals__.get(ident)
        if isinstance(v, str) and v.startswith("vitssl_"):
            found.add(v)
        elif isinstance(v, types.FunctionType) and os.path.dirname(os.path.abspath(v.__code__.co_filename)) == TESTS:
            found |= _reached(v, seen)
    return found


def test_every_arena_test_has_an_off_stream_twin_and_no_entry_point_is_left_out():
    import _offstream as OS
    hdrs = OS.headers()
    assert len(hdrs) >= 13 and HEADER in hdrs
    assert OS.launching(HEADER) == {n for n, args in _prototypes().items() if re.search(r"void\s*\*\s*stream", args)}
    assert OS.MODES == ("gate", "graph") and OS.GATE_MS >= 50.0
    mods = [importlib.import_module(os.path.basename(p)[:-3]) for p in sorted(glob.glob(os.path.join(TESTS, "test_gpu_*_bounds.py")))]
    assert len(mods) >= 13
    gated, twins = set(), 0
    for mod in mods:
        arena_tests = [f for n, f in vars(mod).items() if ARENA_TEST.fullmatch(n) and getattr(f, "__module__", None) == mod.__name__]
        assert arena_tests, f"{mod.__name__}: no arena test found"
        for t in arena_tests:
            name = t.__name__
            twin = getattr(mod, name + "_off_stream", None)
            assert twin is not None, f"{mod.__name__}::{name} has no twin {name}_off_stream"
            assert re.search(rf"offstream\(mode, {name}[,)]", inspect.getsource(twin)), f"{twin.__name__} does not run the body of {name}"
            assert any(m.name == "gpu" for m in twin.pytestmark + [getattr(mod, "pytestmark", twin.pytestmark[0])])
            modes = [m.args[1] for m in twin.pytestmark if m.name == "parametrize" and m.args[0] == "mode"]
            assert modes and "gate" in modes[0], f"{twin.__name__}: no gate mode"
            twins += 1
            if name == "test_abi_case":                                  # the one twin with cases left out, and only by the two rules
                (_, all_cases), (_, kept) = _params(t)[0][:2], _params(twin)[0][:2]
                assert set(kept) <= set(all_cases)
                for c in all_cases:
                    assert (c in kept) == (c.mib <= OS.MAX_ARENA_MIB and not c.reserve), c.id
                gated |= {c.entry for c in kept}
            else:
                assert _params(twin) == _params(t), f"{twin.__name__}: parametrised otherwise than {name}"
                gated |= _reached(t, set())
    assert twins >= 24
    for h in hdrs:
        missing = OS.launching(h) - gated
        assert not missing, f"{os.path.basename(h)}: no off-stream (gate) case launches {sorted(missing)}"
