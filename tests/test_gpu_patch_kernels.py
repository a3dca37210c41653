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


def _chain_runtime(kind, C, P, H, W, D):
    """-> (model, its runtime, the head's nn.Linear, its name in the store): one block per stack, D = Dd"""
    if kind == "simmim":
        from vit_core.ssl.simmim import SimMIMViT
        model = SimMIMViT(num_blocks=1, input_shape=(C, H, W), embed_dim=D, patch_size=P, num_heads=1, mlp_dim=64, dropout=0.0).to(DEV)
        return model, model.runtime(DEV), model.simmim_head, "simmim_head"
    from vit_core.ssl.mae import MAEViT
    model = MAEViT(num_blocks=1, input_shape=(C, H, W), embed_dim=D, patch_size=P, num_heads=1, mlp_dim=64, decoder_embed_dim=D,
                   decoder_blocks=1, decoder_heads=1, decoder_mlp_dim=64).to(DEV)
    return model, model.runtime(DEV), model.decoder_pred, "decoder_pred"


@pytest.mark.parametrize("C,P,H,W", [(3, 4, 16, 16), (3, 5, 15, 15), (3, 14, 42, 42), (3, 8, 16, 16)], ids=str)
@pytest.mark.parametrize("kind", ["simmim", "mae"])
def test_padded_gemm_chain_is_exact(kind, C, P, H, W):
    """Patch projection forward (SimMIM's embed; MAE embeds gathered rows, tests/test_gpu_mae_models.py), its weight gradient, and
    the three methods of the runtime's own engine.PatchHead -- forward, input gradient, weight / bias gradients -- at Pd = 48
    (Np = Pd, Pdp 64), 75 (Np = Pdp = 128), 588 (Np = Pd, Pdp 640) and the native 192, every workspace poisoned beforehand, on
    integer operands: all elements as bits against the integer reference, pad columns and rows exactly zero."""
    B, D = 2, 64
    Pd, N = C * P * P, (H // P) * (W // P)
    model, rt, head, hname = _chain_runtime(kind, C, P, H, W, D)
    st, geo, key = rt.store, rt.geo, rt.head.key
    assert rt.Pdp == PC.padded(Pd) and (rt.Pdp != Pd or (C, P) == (3, 8))
    with torch.no_grad():
        model.projection.weight.copy_(X.int_values((D, Pd), -2, 2, 1))
        model.projection.bias.copy_(X.int_values((D,), -3, 3, 2))
        head.weight.copy_(X.int_values((Pd, D), -2, 2, 3))
        head.bias.copy_(X.int_values((Pd,), -3, 3, 4))
        if kind == "simmim":
            model.positional_embedding.copy_(X.int_values((1, N, D), -4, 4, 5))
    x = X.int_values((B, C, H, W), -3, 3, 6)
    M = B * N
    st.refresh_weights()
    for k in ("proj", key, key + ".T"):                          # the images: pad zero, body the integers
        img = st.w(k).cpu().float()
        src = {"proj": model.projection.weight, key: head.weight, key + ".T": head.weight.t()}[k].detach().cpu()
        want = torch.zeros_like(img)
        want[:src.shape[0], :src.shape[1]] = src
        assert torch.equal(img, want), k
    # --- forward of the projection, on poisoned workspaces
    for name, shape, dt in (("patches", (M, rt.Pdp), BF16), ("x0", (M, D), F32)):
        rt.ws.get(name, shape, dt, DEV).view(torch.int16 if dt == BF16 else torch.int32).fill_(-1)
    pm = O.patchify(x, P).reshape(M, Pd)
    if kind == "simmim":
        x0, patches = rt.embed(x.to(DEV), None)
        want_x0 = pm.double() @ model.projection.weight.detach().cpu().double().t() + model.projection.bias.detach().cpu().double() \
            + model.positional_embedding.detach().cpu().double()[0].repeat(B, 1)
        X.check_exact(x0, X.to_f32_exact(want_x0), "projection forward")
    else:
        patches = rt.ws.get("patches", (M, rt.Pdp), BF16, DEV)
        geo.patchify(x.to(DEV), patches)
    # --- weight gradient of the projection
    dproj = X.int_values((M, D), -3, 3, 7).to(BF16)
    gw = st.gview("projection.weight", (D, Pd))
    gw.copy_(X.int_values((D, Pd), -5, 5, 8))
    rt.ws.get("pad.proj_wgrad", (D, rt.Pdp), F32, DEV).fill_(float("nan"))
    geo.proj_wgrad(dproj.to(DEV), patches, gw, rt.ws)
    X.check_exact(gw, X.to_f32_exact(X.int_values((D, Pd), -5, 5, 8).double() + dproj.double().t() @ pm.double()), "projection wgrad")
    # --- the head: the methods runtime.forward and runtime.backward call, on poisoned workspaces
    Mm = 5
    pads = {n: rt.ws.get(f"pad.{key}_{n}", shape, F32, DEV) for n, shape in (("bias", (rt.Np,)), ("bgrad", (1, rt.Pdp)), ("wgrad", (rt.Pdp, D)))}
    sel = X.int_values((Mm, D), -2, 2, 9).to(BF16)
    hw, hb = head.weight.detach().cpu().double(), head.bias.detach().cpu().double()
    pads["bias"].fill_(float("nan"))
    pred = rt.head.forward(sel.to(DEV))
    assert pred.shape == (Mm, Pd) and pred.dtype == F32
    if rt.Np != Pd:
        assert pred._base.shape == (Mm, rt.Np) and float(pred._base[:, Pd:].abs().max()) == 0.0, "pad columns of the prediction"
    X.check_exact(pred.contiguous(), X.to_f32_exact(sel.double() @ hw.t() + hb), "head forward")
    dpred = torch.zeros(Mm, rt.Pdp, dtype=BF16)
    dpred[:, :Pd] = X.int_values((Mm, Pd), -2, 2, 10).to(BF16)
    dsel = torch.empty(Mm, D, dtype=BF16, device=DEV)
    dsel.view(torch.int16).fill_(NAN_BF16)
    rt.head.dgrad(dpred.to(DEV), dsel)
    X.check_exact(dsel, X.bf16_rne(dpred[:, :Pd].double() @ hw), "head input gradient")
    st.gflat.zero_()
    pads["bgrad"].fill_(float("nan"))
    pads["wgrad"].fill_(float("nan"))
    rt.head.wgrad(dpred.to(DEV), sel.to(DEV))
    X.check_exact(st.gview(hname + ".weight", (Pd, D)), X.to_f32_exact(dpred[:, :Pd].double().t() @ sel.double()), "head wgrad")
    X.check_exact(st.gview(hname + ".bias", (1, Pd)), X.to_f32_exact(dpred[:, :Pd].double().sum(0, keepdim=True)), "head bias grad")
    if rt.Pdp != Pd:
        assert float(pads["wgrad"][Pd:].abs().max()) == 0.0 and float(pads["bgrad"][:, Pd:].abs().max()) == 0.0



def test_widen_grad():
    """PatchGeometry.widen_grad, the autograd bridges' way into the engine's backward: bf16 at the width Pdp, the body the
    round-to-nearest image of the gradient, the pad columns +0; an empty gradient stays empty."""
    from vitssl_hip.engine import PatchGeometry
    for C, P in ((3, 5), (3, 8)):                                 # Pd 75 -> Pdp 128; the native 192
        geo = PatchGeometry(C, P)
        Pd, Pdp = geo.Pd, PC.padded(geo.Pd)
        empty = geo.widen_grad(torch.empty(0, Pd, device=DEV))
        assert empty.shape == (0, Pdp) and empty.dtype == BF16 and empty.device.type == "cuda"
        x = torch.randn(7, Pd, generator=torch.Generator().manual_seed(P))
        for src in (x, x.double(), x.t().contiguous().t()):       # f32, another dtype, not contiguous
            got = geo.widen_grad(src.to(DEV))
            assert got.shape == (7, Pdp) and got.dtype == BF16 and got.is_contiguous()
            assert torch.equal(PC.bits16(got[:, :Pd]), PC.bits16(x.to(BF16))), "body"
            assert Pdp == Pd or int(PC.bits16(got[:, Pd:]).abs().max()) == 0, "pad columns must be +0"
