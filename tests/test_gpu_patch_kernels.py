"""The kernels of include/vitssl_patch.h bit for bit: patchify with a row stride and zeroed pad columns, the target gather, the
strided L1 loss, the strided accumulate, the padded weight cast, and the padded GEMM chain on small-integer operands
(tests/_gemm_exact.py), where an un-zeroed pad column or a gradient landed one row / column off is an integer difference."""
import pytest
import torch

import _gemm_exact as X
import _patch_cases as PC
from oracle import vit_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32, BF16 = torch.float32, torch.bfloat16
NAN_BF16 = 0x7FC1                # a NaN pattern as int16


@pytest.mark.parametrize("C,P,H,W", PC.KERNEL_CASES, ids=str)
@pytest.mark.parametrize("B", [1, 3])
def test_patchify_ld_and_gather(C, P, H, W, B):
    from vitssl_hip import ops
    x = PC.image(B, C, H, W, seed=C * 1000 + P)
    want = O.patchify(x, P).reshape(-1, C * P * P)
    Pd, rows = C * P * P, want.shape[0]
    for ld in sorted({PC.padded(Pd), Pd + (Pd & 1), PC.padded(Pd) + 64}):
        out = torch.empty(rows, ld, dtype=BF16, device=DEV)
        out.view(torch.int16).fill_(NAN_BF16)
        ops.patchify_ld_bf16(x.to(DEV), out, P)
        got = out.cpu()
        assert torch.equal(PC.bits16(got[:, :Pd]), PC.bits16(want.to(BF16))), (ld, "patch columns")
        assert int(PC.bits16(got[:, Pd:]).abs().max() if ld > Pd else 0) == 0, (ld, "pad columns must be +0")
    g = torch.Generator().manual_seed(P)
    idx = torch.randperm(rows, generator=g)[:max(1, (rows * 3) // 5)].sort().values.to(torch.int32)
    tg = torch.full((idx.numel(), Pd), float("nan"), device=DEV)
    ops.gather_patches_any_f32(x.to(DEV), idx.to(DEV), tg, P)
    assert torch.equal(tg.cpu(), want[idx.long()])


def test_patchify_ld_equals_patchify_on_a_native_geometry():
    from vitssl_hip import ops
    x = PC.image(2, 3, 32, 32, seed=5).to(DEV)
    a = torch.empty(8, 768, dtype=BF16, device=DEV)
    b = torch.empty(8, 768, dtype=BF16, device=DEV)
    ops.patchify_bf16(x, a, 16)
    ops.patchify_ld_bf16(x, b, 16)
    assert torch.equal(PC.bits16(a), PC.bits16(b))


def test_patchify_ld_many_blocks():
    """more patches than one workgroup takes, a last workgroup with fewer, patches of one workgroup on two grid rows"""
    from vitssl_hip import ops
    C, P, H, W, B = 3, 14, 70, 98, 5
    x = PC.image(B, C, H, W, seed=9)
    want = O.patchify(x, P).reshape(-1, C * P * P).to(BF16)
    out = torch.empty(want.shape[0], 640, dtype=BF16, device=DEV)
    out.view(torch.int16).fill_(NAN_BF16)
    ops.patchify_ld_bf16(x.to(DEV), out, P)
    assert torch.equal(PC.bits16(out[:, :588]), PC.bits16(want)) and int(PC.bits16(out[:, 588:]).abs().max()) == 0


@pytest.mark.parametrize("rows,cols,ld_p,ld_d", [(5, 75, 128, 128), (7, 588, 588, 640), (3, 49, 64, 64), (1, 4, 4, 64), (37, 48, 48, 64)], ids=str)
def test_l1_loss_ld(rows, cols, ld_p, ld_d):
    from vitssl_hip import ops
    g = torch.Generator().manual_seed(rows * cols)
    pred, tgt = torch.randn(rows, cols, generator=g), torch.randn(rows, cols, generator=g)
    tgt[0, ::3] = pred[0, ::3]                                    # exact ties: gradient 0
    wide = torch.full((rows, ld_p), float("nan"), device=DEV)
    wide[:, :cols] = pred.to(DEV)
    p_d = wide[:, :cols] if ld_p != cols else wide
    n = rows * cols
    want_d = (torch.sign(pred - tgt) / n).to(BF16)
    for _ in range(2):                                            # the second call accumulates nothing stale
        loss = torch.zeros(1, device=DEV)
        dp = torch.empty(rows, ld_d, dtype=BF16, device=DEV)
        dp.view(torch.int16).fill_(NAN_BF16)
        ops.l1_loss_ld(p_d, tgt.to(DEV), loss, dp, gscale=1.0 / n)
        print("l1_loss_ld", rows, cols, float(loss) / n, float(O.l1_loss_mean(pred, tgt)))
        assert abs(float(loss) / n - float(O.l1_loss_mean(pred, tgt))) < 1e-6
        got = dp.cpu()
        assert torch.equal(PC.bits16(got[:, :cols]) & 0x7FFF, PC.bits16(want_d) & 0x7FFF)          # magnitudes
        assert torch.equal(torch.sign(got[:, :cols].float()), torch.sign(want_d.float()))
        assert int(PC.bits16(got[0, :cols:3]).abs().max()) == 0, "ties are +0"
        assert ld_d == cols or int(PC.bits16(got[:, cols:]).abs().max()) == 0, "pad columns must be +0"
    loss2 = torch.zeros(1, device=DEV)
    ops.l1_loss_ld(p_d, tgt.to(DEV), loss2, None)
    assert abs(float(loss2) / n - float(O.l1_loss_mean(pred, tgt))) < 1e-6


@pytest.mark.parametrize("rows,cols,ld", [(64, 75, 128), (588, 64, 64), (1, 49, 64), (130, 588, 640)], ids=str)
def test_accumulate_ld(rows, cols, ld):
    from vitssl_hip import ops
    g = torch.Generator().manual_seed(ld + rows)
    dst, src = torch.randn(rows, cols, generator=g), torch.randn(rows, ld, generator=g)
    d = dst.to(DEV)
    ops.accumulate_ld_f32(d, src.to(DEV))
    assert torch.equal(d.cpu(), dst + src[:, :cols])


def test_padded_cast_plan_keeps_the_pad_at_zero():
    from vitssl_hip import ops
    g = torch.Generator().manual_seed(3)
    w = torch.randn(75, 72, generator=g).to(DEV)
    dst, dst_t = torch.zeros(128, 128, dtype=BF16, device=DEV), torch.zeros(128, 192, dtype=BF16, device=DEV)
    plan = ops.CastPlanLd()
    for _ in range(2):
        plan.run([(w, dst, dst_t)])
        want, want_t = torch.zeros(128, 128, dtype=BF16), torch.zeros(128, 192, dtype=BF16)
        want[:75, :72], want_t[:72, :75] = w.cpu().to(BF16), w.cpu().t().to(BF16)
        assert torch.equal(PC.bits16(dst), PC.bits16(want)) and torch.equal(PC.bits16(dst_t), PC.bits16(want_t))
        w.mul_(1.5)


@pytest.mark.parametrize("C,P,H,W", [(3, 4, 16, 16), (3, 5, 15, 15), (3, 14, 42, 42)], ids=str)
def test_padded_gemm_chain_is_exact(C, P, H, W):
    """Patch projection forward, its weight gradient, head forward, head input gradient and head weight / bias gradients at
    Pd = 48, 75, 588 through the SimMIM runtime's own buffers, every workspace poisoned beforehand, on integer operands:
    all elements as bits against the integer reference."""
    from vit_core.ssl.simmim import SimMIMViT
    from vitssl_hip import _lib as L, ops
    B, D = 2, 64
    Pd, N = C * P * P, (H // P) * (W // P)
    model = SimMIMViT(num_blocks=1, input_shape=(C, H, W), embed_dim=D, patch_size=P, num_heads=1, mlp_dim=64, dropout=0.0).to(DEV)
    rt = model.runtime(DEV)
    st, geo = rt.store, rt.geo
    assert not geo.native and rt.Pdp == PC.padded(Pd)
    with torch.no_grad():
        model.projection.weight.copy_(X.int_values((D, Pd), -2, 2, 1))
        model.projection.bias.copy_(X.int_values((D,), -3, 3, 2))
        model.simmim_head.weight.copy_(X.int_values((Pd, D), -2, 2, 3))
        model.simmim_head.bias.copy_(X.int_values((Pd,), -3, 3, 4))
        model.positional_embedding.copy_(X.int_values((1, N, D), -4, 4, 5))
    x = X.int_values((B, C, H, W), -3, 3, 6)
    M = B * N
    st.refresh_weights()
    for key in ("proj", "head", "head.T"):                       # the images: pad zero, body the integers
        img = st.w(key).cpu().float()
        src = {"proj": model.projection.weight, "head": model.simmim_head.weight, "head.T": model.simmim_head.weight.t()}[key].detach().cpu()
        want = torch.zeros_like(img)
        want[:src.shape[0], :src.shape[1]] = src
        assert torch.equal(img, want), key
    # --- forward of the projection, on poisoned workspaces
    for name, shape, dt in (("patches", (M, rt.Pdp), BF16), ("x0", (M, D), F32)):
        rt.ws.get(name, shape, dt, DEV).view(torch.int16 if dt == BF16 else torch.int32).fill_(-1)
    x0, patches = rt.embed(x.to(DEV), None)
    pm = O.patchify(x, P).reshape(M, Pd)
    want_x0 = pm.double() @ model.projection.weight.detach().cpu().double().t() + model.projection.bias.detach().cpu().double() \
        + model.positional_embedding.detach().cpu().double()[0].repeat(B, 1)
    X.check_exact(x0, X.to_f32_exact(want_x0), "projection forward")
    # --- weight gradient of the projection
    dproj = X.int_values((M, D), -3, 3, 7).to(BF16)
    gw = st.gview("projection.weight", (D, Pd))
    gw.copy_(X.int_values((D, Pd), -5, 5, 8))
    rt.ws.get("pad.proj_wgrad", (D, rt.Pdp), F32, DEV).fill_(float("nan"))
    geo.proj_wgrad(dproj.to(DEV), patches, gw, rt.ws)
    X.check_exact(gw, X.to_f32_exact(X.int_values((D, Pd), -5, 5, 8).double() + dproj.double().t() @ pm.double()), "projection wgrad")
    # --- head forward / backward through runtime.forward's tail and runtime.backward's head
    Mm = 5
    sel = X.int_values((Mm, D), -2, 2, 9).to(BF16)
    hw, hb = model.simmim_head.weight.detach().cpu().double(), model.simmim_head.bias.detach().cpu().double()
    if rt.Np == Pd:
        pred = torch.full((Mm, Pd), float("nan"), device=DEV)
        ops.gemm_nt(sel.to(DEV), st.w("head")[:Pd], pred, L.EPI_F32, bias=st.view("simmim_head.bias"))
    else:
        bias = torch.zeros(rt.Np, device=DEV)
        bias[:Pd] = st.view("simmim_head.bias")
        wide = torch.full((Mm, rt.Np), float("nan"), device=DEV)
        ops.gemm_nt(sel.to(DEV), st.w("head"), wide, L.EPI_F32, bias=bias)
        assert float(wide[:, Pd:].abs().max()) == 0.0, "pad columns of the prediction"
        pred = wide[:, :Pd]
    X.check_exact(pred.contiguous(), X.to_f32_exact(sel.double() @ hw.t() + hb), "head forward")
    dpred = torch.zeros(Mm, rt.Pdp, dtype=BF16)
    dpred[:, :Pd] = X.int_values((Mm, Pd), -2, 2, 10).to(BF16)
    dsel = torch.empty(Mm, D, dtype=BF16, device=DEV)
    ops.gemm_nt(dpred.to(DEV), st.w("head.T"), dsel, L.EPI_BF16)
    X.check_exact(dsel, X.bf16_rne(dpred[:, :Pd].double() @ hw), "head input gradient")
    # weight and bias gradient of the head exactly as runtime.backward forms them
    st.gflat.zero_()
    for name, shape in (("pad.head_bgrad", (1, rt.Pdp)), ("pad.head_wgrad", (rt.Pdp, D))):
        rt.ws.get(name, shape, F32, DEV).fill_(float("nan"))
    hbg, hwg = rt.ws.get("pad.head_bgrad", (1, rt.Pdp), F32, DEV), rt.ws.get("pad.head_wgrad", (rt.Pdp, D), F32, DEV)
    hbg.zero_(); hwg.zero_()
    ops.colsum_bf16(dpred.to(DEV), hbg.view(rt.Pdp))
    ops.gemm_tn(dpred.to(DEV), sel.to(DEV), hwg)
    ops.accumulate_ld_f32(st.gview("simmim_head.bias", (1, Pd)), hbg)
    ops.accumulate_ld_f32(st.gview("simmim_head.weight", (Pd, D)), hwg[:Pd])
    X.check_exact(st.gview("simmim_head.weight", (Pd, D)), X.to_f32_exact(dpred[:, :Pd].double().t() @ sel.double()), "head wgrad")
    X.check_exact(st.gview("simmim_head.bias", (1, Pd)), X.to_f32_exact(dpred[:, :Pd].double().sum(0, keepdim=True)), "head bias grad")
    assert float(hwg[Pd:].abs().max()) == 0.0 and float(hbg[:, Pd:].abs().max()) == 0.0
