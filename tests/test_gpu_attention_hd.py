"""The head-dim-templated attention kernels (csrc/attention_hd.hip, include/vitssl_attention_hd.h) on the GPU.

Cases, references and checkers are those of tests/_attn_hd.py; tests/test_attn_hd_host.py runs the oracle's bf16 emulation
through the same checks on the CPU and shows that the per-row checker catches one localised fault.
  whole-tensor parity   Gaussian inputs, the bars of test_gpu_ops.py::test_attention_fwd_bwd, every head dim class
  per-row parity        planted keys, 3 x the emulation's own worst row error; lengths on the edges of the 64-row streamed tile
                        and of the 128-row workgroup tile, head dims with and without pad columns in every instantiation
  dh = 64               the new family against the dh = 64 kernels
  poison / determinism  NaN-filled outputs come back finite, two runs are bit-equal
  large logits, limits"""
import pytest
import torch

import _attn_hd as A

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NAN = float("nan")
B, H = A.B, A.H


@pytest.fixture(scope="module")
def ops():
    from vitssl_hip import ops as _ops
    return _ops


def _nan(shape, dtype=torch.bfloat16):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def run(fwd, bwd, qkv, dout, Bn, N, Hn, dh, probs=False):
    """forward and backward on NaN-filled outputs -> dict out, lse, dq, dk, dv (and probs) on the CPU, plus the raw device tensors"""
    qkv_d, dout_d = qkv.to(DEV), A.pack_rows(dout).to(DEV)
    out, lse = _nan((Bn * N, Hn * dh)), _nan((Bn, Hn, N), torch.float32)
    pr = _nan((Bn, Hn, N, N), torch.float32) if probs else None
    fwd(qkv_d, out, lse, Bn, N, Hn, dh, probs=pr)
    dqkv, delta_ws = _nan((Bn * N, 3 * Hn * dh)), _nan((Bn, Hn, N), torch.float32)
    bwd(qkv_d, out, dout_d, lse, dqkv, delta_ws, Bn, N, Hn, dh)
    dq, dk, dv = A.unpack_dqkv(dqkv.cpu(), Bn, N, Hn, dh)
    got = {"out": A.unpack_rows(out.cpu(), Bn, N, Hn, dh), "lse": lse.cpu(), "dq": dq, "dk": dk, "dv": dv}
    if probs:
        got["probs"] = pr.cpu()
    return got, (out, lse, dqkv)


@pytest.mark.parametrize("N", A.WHOLE_NS)
@pytest.mark.parametrize("dh", A.WHOLE_DHS)
def test_whole_tensor_parity(ops, dh, N):
    (q, k, v, dout, qkv), ref = A.randn_case(dh, N)
    got, (out, _, _) = run(ops.attn_hd_fwd, ops.attn_hd_bwd, qkv, dout, B, N, H, dh, probs=True)
    A.check_whole(got, ref, f"dh={dh} N={N}")
    out2, lse2 = _nan(out.shape), _nan((B, H, N), torch.float32)
    ops.attn_hd_fwd(qkv.to(DEV), out2, lse2, B, N, H, dh)            # probs=None: `out` must not depend on the probs pointer
    assert torch.equal(out.view(torch.int16), out2.view(torch.int16))


@pytest.mark.parametrize("perm", A.PERMS)
@pytest.mark.parametrize("N", A.ROW_NS)
@pytest.mark.parametrize("dh", A.ROW_DHS)
def test_rows_planted(ops, dh, N, perm):
    case = A.planted_case(dh, N, perm)
    q, k, v, dout = case[0]
    got, _ = run(ops.attn_hd_fwd, ops.attn_hd_bwd, A.pack_qkv(q, k, v), dout, B, N, H, dh)
    A.check_rows(got, case, f"dh={dh} N={N} {perm}")


@pytest.mark.parametrize("perm", A.PERMS)
@pytest.mark.parametrize("dh,N", A.ROW_LONG)
def test_rows_planted_multi_workgroup(ops, dh, N, perm):
    """three 128-row workgroup tiles per item, five streamed tiles with a ragged tail"""
    case = A.planted_case(dh, N, perm)
    q, k, v, dout = case[0]
    got, _ = run(ops.attn_hd_fwd, ops.attn_hd_bwd, A.pack_qkv(q, k, v), dout, B, N, H, dh)
    A.check_rows(got, case, f"dh={dh} N={N} {perm}")


@pytest.mark.parametrize("N", A.CROSS_NS)
def test_dh64_against_the_dh64_kernels(ops, N):
    """both families at dh = 64: each holds the whole-tensor bars against the oracle and the per-row bars on planted keys, and
    they agree with each other at the whole-tensor bars"""
    (q, k, v, dout, qkv), ref = A.randn_case(64, N)
    new, _ = run(ops.attn_hd_fwd, ops.attn_hd_bwd, qkv, dout, B, N, H, 64, probs=True)
    old, _ = run(ops.attn_fwd, ops.attn_bwd, qkv, dout, B, N, H, 64, probs=True)
    A.check_whole(new, ref, f"hd family, dh=64 N={N}")
    A.check_whole(old, ref, f"dh=64 family, N={N}")
    A.check_whole(new, {n: x.float() for n, x in old.items()}, f"hd family against the dh=64 family, N={N}")
    case = A.planted_case(64, N, "rev")
    q, k, v, dout = case[0]
    got, _ = run(ops.attn_hd_fwd, ops.attn_hd_bwd, A.pack_qkv(q, k, v), dout, B, N, H, 64)
    A.check_rows(got, case, f"hd family, dh=64 N={N} rev")


@pytest.mark.parametrize("N", [257, 300])
def test_dh64_run_time_and_folded_head_dim_are_bit_equal(ops, N):
    """dh = 64 above 256 tokens: ops.attn_hd_* (dh and scale as launch arguments) and ops.attn_* (both folded at compile time)
    are two instantiations of one template, with the same instruction order per accumulator and an exact scale of 1 / 8: every
    output is the same bits.  257: one row in the third query tile, one key in the fifth streamed tile; 300: a ragged tail."""
    q, k, v, dout, qkv = A.randn_inputs(B, N, H, 64, seed=6400 + N)
    run_time, _ = run(ops.attn_hd_fwd, ops.attn_hd_bwd, qkv, dout, B, N, H, 64, probs=True)
    folded, _ = run(ops.attn_fwd, ops.attn_bwd, qkv, dout, B, N, H, 64, probs=True)
    for n in ("out", "lse", "probs", "dq", "dk", "dv"):
        a, b = run_time[n].contiguous(), folded[n].contiguous()
        bits = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
        assert a.dtype == b.dtype and torch.equal(a.view(bits), b.view(bits)), f"N={N}: {n} differs"


def test_poisoned_buffers_and_determinism(ops):
    dh, N = A.POISON
    (q, k, v, dout, qkv), ref = A.randn_case(dh, N)
    got1, raw1 = run(ops.attn_hd_fwd, ops.attn_hd_bwd, qkv, dout, B, N, H, dh)      # out, lse, dqkv, delta_ws start as NaN
    for t in raw1:
        assert torch.isfinite(t.float()).all()
    A.check_whole(got1, ref, f"dh={dh} N={N}")
    got2, raw2 = run(ops.attn_hd_fwd, ops.attn_hd_bwd, qkv, dout, B, N, H, dh)
    for a, b in zip(raw1, raw2):
        assert torch.equal(a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32),
                           b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32))


@pytest.mark.parametrize("dh,N", A.LARGE)
def test_large_logits(ops, dh, N):
    """inputs x 4 (scores of magnitude ~10^2 at dh = 128) and a ragged tail: finite, and the bars of
    test_gpu_ops.py::test_attention_large_logits"""
    from _util import max_abs, rel_l2
    (q, k, v, dout, qkv), ref = A.randn_case(dh, N, scale=4.0, Bn=2, Hn=2)
    got, _ = run(ops.attn_hd_fwd, ops.attn_hd_bwd, qkv, dout, 2, N, 2, dh)
    figs = {"lse abs": max_abs(got["lse"], ref["lse"]), "out rel": rel_l2(got["out"], ref["out"]),
            "dqkv rel": rel_l2(torch.stack([got[n].float() for n in ("dq", "dk", "dv")]), torch.stack([ref[n] for n in ("dq", "dk", "dv")]))}
    print(f"dh={dh} N={N} x4: " + "  ".join(f"{n} {x:.2e}" for n, x in figs.items()))
    for n in ("out", "lse", "dq", "dk", "dv"):
        assert torch.isfinite(got[n].float()).all(), n
    assert figs["lse abs"] < 1e-2 and figs["out rel"] < 2e-2 and figs["dqkv rel"] < 4e-2


def test_limits(ops):
    from vitssl_hip import _lib as L

    def z(*shape, dtype=torch.bfloat16):
        return torch.zeros(*shape, dtype=dtype, device=DEV)
    for Bn, N, Hn, dh, msg in [(1, 2049, 1, 32, "2048"), (1, 2049, 1, 8, "2048"), (1, 2049, 1, 80, "2048"), (1, 2049, 1, 128, "2048"),
                               (1, 4, 1, 136, "dh=136"), (1, 4, 1, 12, "dh=12")]:
        qkv, out, lse = z(Bn * N, 3 * Hn * dh), z(Bn * N, Hn * dh), z(Bn, Hn, N, dtype=torch.float32)
        with pytest.raises(L.VitsslError, match=msg):
            ops.attn_hd_fwd(qkv, out, lse, Bn, N, Hn, dh)
        with pytest.raises(L.VitsslError, match=msg):
            ops.attn_hd_bwd(qkv, out, out, lse, torch.empty_like(qkv), torch.empty_like(lse), Bn, N, Hn, dh)
    with pytest.raises(L.VitsslError, match="supported"):
        ops.attn_fwd_any(z(4, 3 * 136), z(4, 136), z(1, 1, 4, dtype=torch.float32), 1, 4, 1, 136)
