"""No GPU needed: the guarded arena of tests/_arena.py catches what it is there to catch, and the case table of
tests/test_gpu_abi_bounds.py covers every launching entry point that include/vitssl_hip.h declares."""
import os
import re

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
    assert torch.isnan(y.float()).all() and torch.isnan(s).all()                         # 0xFF is NaN as bf16 and fp32
    assert torch.isnan(a.empty("e", (8,), torch.float8_e4m3fn).float()).all()            # and as e4m3fn
    assert int(a.empty("i", (3,), torch.int32)[0]) == -1 and int(a.empty("u", (3,), torch.uint8)[0]) == 255
    regs = a.regions
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
