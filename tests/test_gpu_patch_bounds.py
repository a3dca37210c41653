"""Every launching entry point of include/vitssl_patch.h on guarded-arena tensors (tests/_arena.py), in the manner of
tests/test_gpu_attention_hd_bounds.py: inputs, outputs and EXACT-size workspaces are carved from a 0xFF-poisoned arena.  Per case:
no guard byte changes, no NaN poison reaches a result (every output element is written, no input is read past its end), the
inputs are unchanged, the results are the exact ones.  Shapes: the smallest and the most ragged of tests/_patch_cases.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _patch_cases as PC
from _arena import Arena
from _offstream import offstream, twin_of  # noqa: F401  (offstream is a fixture)
from oracle import vit_oracle as O

DEV = torch.device("cuda:0")
F32, BF16 = torch.float32, torch.bfloat16
gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COVERED = {"vitssl_patchify_ld_bf16", "vitssl_gather_patches_any_f32", "vitssl_l1_loss_ld", "vitssl_accumulate_ld_f32",
           "vitssl_cast_transpose_batch_ld"}        # the entry points the tests below launch


def P(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def test_every_launching_function_has_a_case():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vitssl_patch.h")).read(), flags=re.S)
    launching = {m.group(1) for m in re.finditer(r"\bint\s+(vitssl_[a-z0-9_]+)\s*\(([^)]*void\s*\*\s*stream[^)]*)\)\s*;", txt)}
    assert launching == COVERED


@gpu
@pytest.mark.parametrize("C_,P_,H,W,B", [(1, 2, 8, 8, 1), (3, 5, 15, 15, 3), (1, 7, 28, 28, 2), (3, 14, 28, 42, 3)], ids=str)
def test_patchify_and_gather_on_the_arena(C_, P_, H, W, B):
    from vitssl_hip import _lib as L
    x = PC.image(B, C_, H, W, seed=P_)
    want = O.patchify(x, P_).reshape(-1, C_ * P_ * P_)
    Pd, rows = want.shape[1], want.shape[0]
    ld = PC.padded(Pd)
    idx = torch.arange(rows - 1, -1, -2, dtype=torch.int32)           # descending, ends on the first or second patch
    a = Arena(DEV, mib=16)
    img, idx_a = a.put("img", x), a.put("idx", idx)
    out, tg = a.empty("patches", (rows, ld), BF16), a.empty("targets", (idx.numel(), Pd), F32)
    L.call("vitssl_patchify_ld_bf16", P(img), P(out), B, C_, H, W, P_, ld, S())
    L.call("vitssl_gather_patches_any_f32", P(img), P(idx_a), P(tg), idx.numel(), C_, H, W, P_, S())
    torch.cuda.synchronize()
    a.check()
    assert torch.equal(img.cpu(), x) and torch.equal(idx_a.cpu(), idx), "inputs are inputs"
    assert torch.equal(PC.bits16(out[:, :Pd]), PC.bits16(want.to(BF16)))
    assert int(PC.bits16(out[:, Pd:]).abs().max()) == 0
    assert torch.equal(tg.cpu(), want[idx.long()])


@gpu
@pytest.mark.parametrize("rows,cols,ld_p,ld_d", [(1, 4, 4, 64), (7, 75, 128, 128), (3, 49, 49, 64)], ids=str)
def test_l1_and_accumulate_on_the_arena(rows, cols, ld_p, ld_d):
    from vitssl_hip import _lib as L
    g = torch.Generator().manual_seed(cols)
    pred, tgt = torch.randn(rows, ld_p, generator=g), torch.randn(rows, cols, generator=g)
    n = rows * cols
    wsn = int(L.lib().vitssl_sum_workspace_floats(n, 1))
    a = Arena(DEV, mib=16)
    # pred as the column prefix of a buffer of exactly rows * ld_p floats: what follows the last row's pad is guard
    p_a, t_a = a.put("pred", pred), a.put("target", tgt)
    loss, dp, ws = a.zeros("loss", (1,), F32), a.empty("dpred", (rows, ld_d), BF16), a.empty("ws", (wsn,), F32)
    L.call("vitssl_l1_loss_ld", P(p_a), ld_p, P(t_a), cols, P(loss), P(dp), ld_d, 1.0 / n, rows, cols, P(ws), wsn, S())
    dst0, src = torch.randn(rows, cols, generator=g), torch.randn(rows, ld_p, generator=g)
    d_a, s_a = a.put("dst", dst0), a.put("src", src)
    L.call("vitssl_accumulate_ld_f32", P(d_a), P(s_a), rows, cols, ld_p, S())
    torch.cuda.synchronize()
    a.check()
    assert torch.equal(p_a.cpu(), pred) and torch.equal(t_a.cpu(), tgt) and torch.equal(s_a.cpu(), src), "inputs are inputs"
    assert not torch.isnan(dp.float()).any() and not torch.isnan(loss).any()
    d = pred[:, :cols] - tgt
    assert abs(float(loss) / n - float(d.abs().sum() / n)) < 1e-6
    want = torch.zeros(rows, ld_d, dtype=BF16)
    want[:, :cols] = (torch.sign(d) / n).to(BF16)
    assert torch.equal(dp.cpu().float(), want.float()) and int(PC.bits16(dp[:, cols:]).abs().max()) == 0
    assert torch.equal(d_a.cpu(), dst0 + src[:, :cols])


@gpu
def test_padded_cast_on_the_arena():
    from vitssl_hip import _lib as L
    g = torch.Generator().manual_seed(11)
    srcs = [torch.randn(75, 72, generator=g), torch.randn(64, 49, generator=g)]
    shapes = [((75, 128), (72, 128)), ((64, 64), (64, 64))]        # (dst, dst_t): [R, ld >= C], [>= C rows, ld >= R]
    a = Arena(DEV, mib=16)
    rec = np.zeros(2, dtype=np.dtype([("src", "<u8"), ("dst", "<u8"), ("dst_t", "<u8"), ("R", "<i4"), ("C", "<i4"), ("ld", "<i4"), ("ldt", "<i4")]))
    starts = np.zeros(3, dtype=np.int32)
    keep = []
    for i, (s, (ds, dts)) in enumerate(zip(srcs, shapes)):
        s_a, d, dt = a.put(f"src{i}", s), a.zeros(f"dst{i}", ds, BF16), a.zeros(f"dst_t{i}", dts, BF16)
        keep.append((s_a, d, dt))
        rec[i] = (s_a.data_ptr(), d.data_ptr(), dt.data_ptr(), s.shape[0], s.shape[1], ds[1], dts[1])
        starts[i + 1] = starts[i] + ((s.shape[0] + 63) // 64) * ((s.shape[1] + 63) // 64)
    jobs = a.put("jobs", torch.from_numpy(rec.view(np.uint8).copy()))
    st = a.put("starts", torch.from_numpy(starts))
    L.call("vitssl_cast_transpose_batch_ld", P(jobs), P(st), 2, int(starts[-1]), S())
    torch.cuda.synchronize()
    a.check()
    for (s_a, d, dt), s in zip(keep, srcs):
        R, Cn = s.shape
        assert torch.equal(s_a.cpu(), s)
        want, want_t = torch.zeros(d.shape, dtype=BF16), torch.zeros(dt.shape, dtype=BF16)
        want[:R, :Cn], want_t[:Cn, :R] = s.to(BF16), s.t().to(BF16)
        assert torch.equal(PC.bits16(d), PC.bits16(want)) and torch.equal(PC.bits16(dt), PC.bits16(want_t))


# ============================================================================================ off the default stream (tests/_offstream.py)
@twin_of(test_patchify_and_gather_on_the_arena)
def test_patchify_and_gather_on_the_arena_off_stream(C_, P_, H, W, B, mode, offstream):
    offstream(mode, test_patchify_and_gather_on_the_arena, C_, P_, H, W, B)


@twin_of(test_l1_and_accumulate_on_the_arena)
def test_l1_and_accumulate_on_the_arena_off_stream(rows, cols, ld_p, ld_d, mode, offstream):
    offstream(mode, test_l1_and_accumulate_on_the_arena, rows, cols, ld_p, ld_d)


@twin_of(test_padded_cast_on_the_arena)
def test_padded_cast_on_the_arena_off_stream(mode, offstream):
    offstream(mode, test_padded_cast_on_the_arena)
