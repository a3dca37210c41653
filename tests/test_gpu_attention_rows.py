"""Every attention kernel family on planted-key inputs, judged per row (tests/_attn_planted.py).

The Gaussian tests judge out with atol 4e-3 and the gradients with rel-L2 < 2e-2 over a tensor or an item; one dropped
(query, key) pair stays 12x below that (tests/test_attn_planted_host.py).  Here every query has one key that carries 0.57-0.70
of its row, every key is some query's, and out, dq, dk, dv are asserted row by row at 3 x the worst row error of the oracle's
bf16 emulation of the same case against fp64, lse at 1e-4.  The lengths sit on the tile edges of each family:
  fused, <= 128        one 16-key step, ragged steps, both wave counts
  persistent, 129-224  and, under a CU reserve, 3-4 items per workgroup
  pipelined, 225-256
  streaming, 257-2048  ragged and exact 64-row streamed tiles, 128-row stationary tiles with one row over (forward, delta,
                       dK/dV and dQ kernels)."""
import ctypes as C

import pytest
import torch

import _attn_planted as P

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DH = P.DH
NAN = float("nan")
PERMS = ["rev", "shift"]

FAMILIES = {
    "fused": ((2, 3), [5, 16, 17, 33, 64, 65, 128]),
    "persistent": ((2, 3), [129, 160, 197, 224]),
    "pipelined": ((2, 3), [225, 256]),
    "streaming": ((1, 2), [257, 320, 321, 385, 2048]),
}
CASES = [pytest.param(fam, BH, N, id=f"{fam}-N{N}") for fam, (BH, lengths) in FAMILIES.items() for N in lengths]


@pytest.fixture(scope="module")
def ops():
    from vitssl_hip import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture
def reserve():
    """set(n) -> vitssl_set_reserved_cus(n); the count in force before the test is restored afterwards, also on failure."""
    from vitssl_hip import _lib as L
    lib = L.lib()
    old = lib.vitssl_get_reserved_cus()

    def set_(n):
        L.call("vitssl_set_reserved_cus", C.c_int(n))
        assert lib.vitssl_get_reserved_cus() == n
    yield set_
    torch.cuda.synchronize()
    L.call("vitssl_set_reserved_cus", C.c_int(old))
    assert lib.vitssl_get_reserved_cus() == old


def _nan(shape, dtype=torch.bfloat16):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def _run(ops, qkv, dout, B, N, H):
    """forward and backward through the public ops on NaN-filled outputs -> dict out, lse, dq, dk, dv on the CPU"""
    qkv_d, dout_d = qkv.to(DEV), P.pack_rows(dout).to(DEV)
    out, lse = _nan((B * N, H * DH)), _nan((B, H, N), torch.float32)
    ops.attn_fwd(qkv_d, out, lse, B, N, H, DH)
    dqkv, delta_ws = _nan((B * N, 3 * H * DH)), _nan((B, H, N), torch.float32)
    ops.attn_bwd(qkv_d, out, dout_d, lse, dqkv, delta_ws, B, N, H, DH)
    dq, dk, dv = P.unpack_dqkv(dqkv.cpu(), B, N, H)
    return {"out": P.unpack_rows(out.cpu(), B, N, H), "lse": lse.cpu(), "dq": dq, "dk": dk, "dv": dv}


def _check(ops, B, N, H, perm, what):
    q, k, v, dout, qkv = P.planted(B, N, H, perm, seed=10 * N + PERMS.index(perm))
    ref = P.ref64(q, k, v, dout)
    bar, emu_worst = P.bars(ref, P.emu(q, k, v, dout))
    got = _run(ops, qkv, dout, B, N, H)
    lse_err = float((got["lse"].double() - ref["lse"]).abs().max())
    worst = {n: float(P.row_err(got[n], ref[n]).max()) for n in P.TENSORS}
    print(f"{what} N={N} {perm}: max row error (kernel / emulation) "
          + "  ".join(f"{n} {worst[n]:.2e} / {emu_worst[n]:.2e}" for n in P.TENSORS) + f"  lse {lse_err:.2e}")
    for n in ("out", "lse", "dq", "dk", "dv"):
        assert not torch.isnan(got[n].float()).any(), f"{n}: NaN left"
    assert lse_err < P.LSE_BAR, f"lse: max abs error {lse_err:.3e}"
    bad = P.failures(got, ref, bar)
    assert not bad, "; ".join(f"{n}: row error {e:.3e} > {bar[n]:.3e} at (b, h, row) = {at}" for n, (e, at) in bad.items())


@pytest.mark.parametrize("perm", PERMS)
@pytest.mark.parametrize("family,BH,N", CASES)
def test_attention_rows(ops, family, BH, N, perm):
    _check(ops, BH[0], N, BH[1], perm, family)


@pytest.mark.parametrize("perm", PERMS)
@pytest.mark.parametrize("N", [197, 224])
def test_attention_rows_swept_items(ops, cus, reserve, N, perm):
    """27 items on 8 workgroups: the persistent kernels sweep 3-4 items each; every item row by row"""
    from vitssl_hip import _lib as L
    B, H = 9, 3
    reserve(cus - 8)
    _check(ops, B, N, H, perm, "persistent, 8 workgroups")
    assert L.lib().vitssl_debug_last_attn_fwd_grid() == 8
