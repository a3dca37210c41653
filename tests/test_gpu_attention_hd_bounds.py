"""Both launching entry points of include/vitssl_attention_hd.h on guarded-arena tensors (tests/_arena.py), in the manner of
tests/test_gpu_metrics_bounds.py: qkv, dout, every output and an EXACT-size delta workspace are carved from a 0xFF-poisoned
arena.  Per case: no guard byte changes (a head's slice is read and written in place: what lies behind the last head's last row
is guard); no NaN poison reaches a result (every output element is written, delta_ws is written before it is read, no input is
read past its end, the pad columns of the tiles are zero); the inputs are unchanged; the results hold the whole-tensor bars."""
import ctypes as C
import os
import re

import pytest
import torch

import _attn_hd as A
from _arena import Arena
from _offstream import offstream, twin_of  # noqa: F401  (offstream is a fixture)

DEV = torch.device("cuda:0")
F32, BF16 = torch.float32, torch.bfloat16
gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COVERED = {"vitssl_attn_hd_fwd", "vitssl_attn_hd_bwd"}        # the entry points test_on_the_arena launches


def P(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def test_every_launching_function_has_a_case():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vitssl_attention_hd.h")).read(), flags=re.S)
    launching = {m.group(1) for m in re.finditer(r"\bint\s+(vitssl_[a-z0-9_]+)\s*\(([^)]*void\s*\*\s*stream[^)]*)\)\s*;", txt)}
    assert launching == COVERED


@gpu
@pytest.mark.parametrize("dh,N", A.BOUNDS, ids=str)
def test_on_the_arena(dh, N):
    from vitssl_hip import _lib as L
    B, H = A.B, A.H
    (q, k, v, dout, qkv), ref = A.randn_case(dh, N)
    a = Arena(DEV, mib=32)
    qkv_a, dout_a = a.put("qkv", qkv), a.put("dout", A.pack_rows(dout))
    out, lse = a.empty("out", (B * N, H * dh), BF16), a.empty("lse", (B, H, N), F32)
    probs = a.empty("probs", (B, H, N, N), F32)
    dqkv, ws = a.empty("dqkv", (B * N, 3 * H * dh), BF16), a.empty("delta_ws", (B, H, N), F32)      # exactly B * H * N floats
    L.call("vitssl_attn_hd_fwd", P(qkv_a), P(out), P(lse), P(probs), B, N, H, dh, S())
    L.call("vitssl_attn_hd_bwd", P(qkv_a), P(out), P(dout_a), P(lse), P(dqkv), P(ws), B, N, H, dh, S())
    torch.cuda.synchronize()
    a.check()
    for name, t in (("out", out), ("lse", lse), ("probs", probs), ("dqkv", dqkv), ("delta_ws", ws)):
        assert not torch.isnan(t.float()).any(), f"{name}: poison left or read"
    assert torch.equal(qkv_a.cpu().view(torch.int16), qkv.view(torch.int16)), "inputs are inputs"
    assert torch.equal(dout_a.cpu().view(torch.int16), A.pack_rows(dout).view(torch.int16))
    dq, dk, dv = A.unpack_dqkv(dqkv.cpu(), B, N, H, dh)
    got = {"out": A.unpack_rows(out.cpu(), B, N, H, dh), "lse": lse.cpu(), "probs": probs.cpu(), "dq": dq, "dk": dk, "dv": dv}
    A.check_whole(got, ref, f"arena dh={dh} N={N}", inputs=(q, k, v, dout))
    # without probs: the same bits, still no guard byte touched
    out2 = a.empty("out2", (B * N, H * dh), BF16)
    L.call("vitssl_attn_hd_fwd", P(qkv_a), P(out2), P(lse), P(None), B, N, H, dh, S())
    torch.cuda.synchronize()
    a.check()
    assert torch.equal(out.view(torch.int16), out2.view(torch.int16))


# ============================================================================================ off the default stream (tests/_offstream.py)
@twin_of(test_on_the_arena)
def test_on_the_arena_off_stream(dh, N, mode, offstream):
    offstream(mode, test_on_the_arena, dh, N)
