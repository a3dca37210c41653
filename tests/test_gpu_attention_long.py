"""Streaming attention for 257-2048 tokens (dh = 64: the <64, 64> instantiations of csrc/attention_hd.hip) against the CPU oracle: op parity with the bars of
tests/test_gpu_ops.py::test_attention_fwd_bwd, multi-round grids, run-to-run determinism, large logits with a ragged tail,
the limits (2048 tokens with bf16 operands, 256 with fp8 operands) and the module / model level at patch 8."""
import math

import pytest
import torch

from _util import rel_l2, max_abs, l1_backward_with_signs
from oracle import vit_oracle as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
QUERY_TILE = 128      # queries per workgroup of the streaming forward (WG_ROWS in csrc/attention_hd.hip)


@pytest.fixture(scope="module")
def ops():
    from vitssl_hip import ops as _ops
    return _ops


def bf(x):
    return x.to(torch.bfloat16)


def gpu(x):
    return x.to(DEV).contiguous()


def close_bf16(got, ref, atol=2e-3, what=""):
    got = got.float().cpu()
    ref = ref.float().cpu()
    err = (got - ref).abs()
    lim = ref.abs() * 2.0 ** -7 + atol
    bad = err > lim
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} outside bf16 tolerance, max err {float(err.max())}"


def _attn_ref(qkv, Bn, N, H, dh, emu="bf16"):
    x = qkv.float().view(Bn, N, 3, H, dh)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))      # [B,H,N,dh]
    o, p = O.sdpa(q, k, v, emu)
    s = (q @ k.transpose(-2, -1)) / math.sqrt(dh)
    lse = torch.logsumexp(s, dim=-1)
    return o.transpose(1, 2).reshape(Bn * N, H * dh), p, lse


def _fwd(ops, qkv_d, Bn, N, H, dh, probs=False):
    out = torch.empty(Bn * N, H * dh, dtype=torch.bfloat16, device=DEV)
    lse = torch.empty(Bn, H, N, device=DEV)
    pr = torch.empty(Bn, H, N, N, device=DEV) if probs else None
    ops.attn_fwd(qkv_d, out, lse, Bn, N, H, dh, probs=pr)
    return out, lse, pr


def _bwd(ops, qkv_d, out, dout_d, lse, Bn, N, H, dh):
    dqkv = torch.full((Bn * N, 3 * H * dh), float("nan"), dtype=torch.bfloat16, device=DEV)
    delta = torch.empty(Bn, H, N, device=DEV)
    ops.attn_bwd(qkv_d, out, dout_d, lse, dqkv, delta, Bn, N, H, dh)
    return dqkv


# ----------------------------------------------------------------------------- 1. op parity
@pytest.mark.parametrize("N", [257, 320, 577, 785, 1025, 2048])
def test_attention_long_fwd_bwd(ops, N):
    torch.manual_seed(N)
    Bn, H, dh = 2, 3, 64
    qkv = bf(torch.randn(Bn * N, 3 * H * dh))
    out, lse, probs = _fwd(ops, gpu(qkv), Bn, N, H, dh, probs=True)
    ro, rp, rl = _attn_ref(qkv, Bn, N, H, dh)
    print(f"N={N}: probs rel {rel_l2(probs, rp):.3e} max {max_abs(probs, rp):.3e}  lse max {max_abs(lse, rl):.3e}  "
          f"out max {max_abs(out.float(), bf(ro).float()):.3e}")
    assert rel_l2(probs, rp) < 1e-3 and max_abs(probs, rp) < 2e-4
    assert max_abs(lse, rl) < 1e-4
    close_bf16(out, bf(ro), atol=4e-3, what="attn out")

    dout = bf(torch.randn(Bn * N, H * dh))
    leaf = qkv.float().clone().requires_grad_(True)
    ro2, _, _ = _attn_ref(leaf, Bn, N, H, dh, emu=None)
    (ro2 * dout.float()).sum().backward()
    dqkv = _bwd(ops, gpu(qkv), out, gpu(dout), lse, Bn, N, H, dh)
    got = dqkv.float().cpu().view(Bn, N, 3, H, dh)
    ref = leaf.grad.view(Bn, N, 3, H, dh)
    assert not torch.isnan(got).any()
    for i, name in enumerate("qkv"):
        print(f"N={N}: d{name} rel {rel_l2(got[:, :, i], ref[:, :, i]):.3e}")
        assert rel_l2(got[:, :, i], ref[:, :, i]) < 2e-2, name


# ----------------------------------------------------------------------------- 2. probs=None path
def test_attention_long_out_independent_of_probs(ops):
    torch.manual_seed(11)
    Bn, H, dh, N = 2, 3, 64, 785
    qkv = gpu(bf(torch.randn(Bn * N, 3 * H * dh)))
    out1, lse1, _ = _fwd(ops, qkv, Bn, N, H, dh, probs=True)
    out2, lse2, _ = _fwd(ops, qkv, Bn, N, H, dh, probs=False)
    assert torch.equal(out1, out2) and torch.equal(lse1, lse2)


# ----------------------------------------------------------------------------- 3. many workgroups
def test_attention_long_many_workgroups(ops):
    """More than two rounds of workgroups per CU: every lse row, and out / dqkv of items spread over the grid."""
    torch.manual_seed(5)
    Bn, H, dh, N = 24, 12, 64, 785
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    assert Bn * H * math.ceil(N / QUERY_TILE) > 2 * cus
    qkv = bf(torch.randn(Bn * N, 3 * H * dh))
    dout = bf(torch.randn(Bn * N, H * dh))
    qkv_d, dout_d = gpu(qkv), gpu(dout)
    out, lse, _ = _fwd(ops, qkv_d, Bn, N, H, dh)
    dqkv = _bwd(ops, qkv_d, out, dout_d, lse, Bn, N, H, dh)
    out_c = out.float().cpu().view(Bn, N, H, dh)
    got = dqkv.float().cpu().view(Bn, N, 3, H, dh)
    assert not torch.isnan(got).any()
    x = qkv.float().view(Bn, N, 3, H, dh)
    lse_c = lse.cpu()
    for b in range(Bn):                                  # all of lse, one image at a time
        q, k = x[b, :, 0].transpose(0, 1), x[b, :, 1].transpose(0, 1)        # [H,N,dh]
        rl = torch.logsumexp((q @ k.transpose(-2, -1)) / math.sqrt(dh), dim=-1)
        assert max_abs(lse_c[b], rl) < 1e-4, b
    items = [(0, 0), (0, 11), (3, 5), (7, 1), (11, 6), (12, 0), (16, 9), (20, 3), (23, 10), (23, 11)]
    for b, h in items:
        one = qkv.view(Bn, N, 3, H, dh)[b, :, :, h].reshape(N, 3 * dh)         # a one-image, one-head problem
        ro, _, _ = _attn_ref(one, 1, N, 1, dh)
        close_bf16(out_c[b, :, h], bf(ro), atol=4e-3, what=f"attn out item {(b, h)}")
        leaf = one.float().clone().requires_grad_(True)
        ro2, _, _ = _attn_ref(leaf, 1, N, 1, dh, emu=None)
        (ro2 * dout.float().view(Bn, N, H, dh)[b, :, h]).sum().backward()
        ref = leaf.grad.view(N, 3, dh)
        for i, name in enumerate("qkv"):
            assert rel_l2(got[b, :, i, h], ref[:, i]) < 2e-2, (b, h, name)


# ----------------------------------------------------------------------------- 4. determinism
def test_attention_long_is_deterministic(ops):
    torch.manual_seed(6)
    Bn, H, dh, N = 24, 12, 64, 785
    assert Bn * H > torch.cuda.get_device_properties(DEV).multi_processor_count
    qkv = gpu(bf(torch.randn(Bn * N, 3 * H * dh)))
    dout = gpu(bf(torch.randn(Bn * N, H * dh)))
    runs = []
    for _ in range(2):
        out, lse, _ = _fwd(ops, qkv, Bn, N, H, dh)
        dqkv = _bwd(ops, qkv, out, dout, lse, Bn, N, H, dh)
        runs.append((out, lse, dqkv))
    for a, b in zip(*runs):
        assert not torch.isnan(a.float()).any() and torch.equal(a, b)


# ----------------------------------------------------------------------------- 5. large logits, ragged tail
def test_attention_long_large_logits(ops):
    """Scores of magnitude ~10^2 over several key tiles (the running maximum moves, most keys underflow) and a ragged tail."""
    torch.manual_seed(3)
    Bn, H, dh, N = 2, 2, 64, 333
    qkv = bf(torch.randn(Bn * N, 3 * H * dh) * 4.0)
    out, lse, _ = _fwd(ops, gpu(qkv), Bn, N, H, dh)
    ro, _, rl = _attn_ref(qkv, Bn, N, H, dh, emu=None)
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all()
    assert max_abs(lse, rl) < 1e-2
    assert rel_l2(out.float().cpu(), ro) < 2e-2
    dout = bf(torch.randn(Bn * N, H * dh))
    leaf = qkv.float().clone().requires_grad_(True)
    ro2, _, _ = _attn_ref(leaf, Bn, N, H, dh, emu=None)
    (ro2 * dout.float()).sum().backward()
    dqkv = _bwd(ops, gpu(qkv), out, gpu(dout), lse, Bn, N, H, dh)
    got = dqkv.float().cpu()
    assert torch.isfinite(got).all()
    assert rel_l2(got, leaf.grad) < 4e-2


# ----------------------------------------------------------------------------- 6. boundaries
def test_attention_long_limit_is_2048(ops):
    from vitssl_hip import _lib as L
    Bn, H, dh, N = 1, 1, 64, 2049
    qkv = torch.zeros(Bn * N, 3 * H * dh, dtype=torch.bfloat16, device=DEV)
    out = torch.zeros(Bn * N, H * dh, dtype=torch.bfloat16, device=DEV)
    lse = torch.zeros(Bn, H, N, device=DEV)
    with pytest.raises(L.VitsslError, match="2048"):
        ops.attn_fwd(qkv, out, lse, Bn, N, H, dh)
    with pytest.raises(L.VitsslError, match="2048"):
        ops.attn_bwd(qkv, out, out, lse, torch.zeros_like(qkv), torch.zeros_like(lse), Bn, N, H, dh)


def test_attention_256_keeps_its_path(ops):
    """256 tokens: one persistent workgroup per (image, head) item as before; 257 tokens: one per (item, query tile)."""
    from vitssl_hip import _lib as L
    Bn, H, dh = 2, 3, 64
    grids = {}
    for N in (256, 257):
        _fwd(ops, gpu(bf(torch.randn(Bn * N, 3 * H * dh))), Bn, N, H, dh)
        grids[N] = int(L.lib().vitssl_debug_last_attn_fwd_grid())
    assert grids[256] == Bn * H
    assert grids[257] == Bn * H * math.ceil(257 / QUERY_TILE)


def test_fp8_operands_refuse_long_sequences_early(ops, monkeypatch):
    """fp8 operand mode ends at 256 tokens: the op says so, and a model says so before it has launched anything."""
    from vitssl_hip import _lib as L, engine
    from vit_core.ssl.simmim import SimMIMViT
    Bn, H, dh, N = 1, 2, 64, 257
    qkv = torch.zeros(Bn * N, 3 * H * dh, dtype=torch.bfloat16, device=DEV)
    out = torch.zeros(Bn * N, H * dh, dtype=torch.bfloat16, device=DEV)
    out8 = torch.zeros(Bn * N, H * dh, dtype=ops.FP8, device=DEV)
    with pytest.raises(L.VitsslError, match="bf16"):
        ops.attn_fwd(qkv, out, torch.zeros(Bn, H, N, device=DEV), Bn, N, H, dh, out_fp8=out8)

    before = engine.linear_operands()
    engine.set_linear_operands("fp8")
    try:
        torch.manual_seed(0)
        model = SimMIMViT(num_blocks=1, input_shape=(3, 144, 144), embed_dim=128, patch_size=8, num_heads=2, mlp_dim=128,
                          dropout=0.0, mask_ratio=0.6).to(DEV).train()
        x = torch.rand(1, 3, 144, 144, device=DEV)
        torch.cuda.synchronize()
        launched = []
        real_call = ops.call
        monkeypatch.setattr(ops, "call", lambda name, *a, **k: (launched.append(name), real_call(name, *a, **k))[1])
        with pytest.raises(L.VitsslError, match="bf16"):
            model(x)
        assert launched == []
    finally:
        engine.set_linear_operands(before)


# ----------------------------------------------------------------------------- 7. module and model level
def test_multi_headed_attention_300_tokens():
    from vit_core import MultiHeadedAttention
    torch.manual_seed(1)
    mha = MultiHeadedAttention(128, 2).to(DEV)
    sd = {k: v.detach().cpu() for k, v in mha.state_dict().items()}
    x = torch.randn(2, 300, 128)
    xd = x.to(DEV).requires_grad_(True)
    out, probs = mha(xd, xd, xd, return_attn=True)
    assert out.shape == (2, 300, 128) and probs.shape == (2, 2, 300, 300)
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    xr = x.clone().requires_grad_(True)
    ro, rp = O.mha(xr, leaves, "", 2, emu="bf16", return_attn=True)
    assert rel_l2(out, ro) < 1e-2 and rel_l2(probs, rp) < 1e-2
    out.square().sum().backward()
    ro.square().sum().backward()
    assert rel_l2(xd.grad, xr.grad) < 5e-2
    for k, p in mha.named_parameters():
        assert p.grad is not None, k
        assert rel_l2(p.grad, leaves[k].grad) < 6e-2, (k, rel_l2(p.grad, leaves[k].grad))


def test_simmim_patch8_324_tokens_against_oracle():
    from vit_core.ssl.simmim import SimMIMViT
    from vit_core.ssl.simmim.masking import draw_mask
    torch.manual_seed(144)
    B, img, patch, D, H, F = 2, 144, 8, 128, 2, 192
    model = SimMIMViT(num_blocks=2, input_shape=(3, img, img), embed_dim=D, patch_size=patch, num_heads=H, mlp_dim=F,
                      dropout=0.0, mask_ratio=0.6)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.to(DEV).train()
    x = torch.rand(B, 3, img, img)
    N = (img // patch) ** 2
    assert N == 324
    torch.manual_seed(77)
    mask = draw_mask(B, N, 0.6)
    torch.manual_seed(77)                                                    # the model draws the same mask
    pred, tgt, bm = model(x.to(DEV), return_bool_mask=True)
    assert torch.equal(bm[..., 0].cpu(), mask)
    loss = torch.nn.L1Loss()(pred, tgt)
    loss.backward()
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    pe, te = O.simmim_forward(leaves, x, mask, patch, H, emu="bf16")
    assert pred.shape == pe.shape and torch.equal(tgt.cpu(), te)
    assert rel_l2(pred, pe) < 1e-2
    ref_loss = float(O.l1_loss_mean(pe.detach(), te))
    assert abs(float(loss.detach()) - ref_loss) < 1e-2 * ref_loss
    l1_backward_with_signs(pe, te, pred, tgt)
    for k, p in model.named_parameters():
        assert p.grad is not None, k
        assert rel_l2(p.grad, leaves[k].grad) < 2e-2, (k, rel_l2(p.grad, leaves[k].grad))


def test_vit_patch8_290_tokens_against_oracle():
    from vit_core import ViT
    torch.manual_seed(136)
    B, img, patch, D, H, F, C = 2, 136, 8, 128, 2, 192, 10
    model = ViT(num_classes=C, num_blocks=2, input_shape=(3, img, img), embed_dim=D, patch_size=patch, num_heads=H,
                mlp_dim=F, dropout=0.0)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.to(DEV).train()
    x = torch.rand(B, 3, img, img)
    labels = torch.tensor([3, 7])
    logits, attn = model(x.to(DEV), return_attn=True)
    T = (img // patch) ** 2 + 1
    assert T == 290 and attn.shape == (B, H, T, T)
    loss = torch.nn.CrossEntropyLoss()(logits, labels.to(DEV))
    loss.backward()
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    rlogits, rattn = O.vit_forward(leaves, x, patch, H, emu="bf16", return_attn=True)
    rloss = O.cross_entropy_mean(rlogits, labels)
    rloss.backward()
    assert rel_l2(logits, rlogits) < 2e-2
    assert rel_l2(attn, rattn) < 2e-2
    assert abs(float(loss.detach()) - float(rloss.detach())) < 1e-2 * abs(float(rloss.detach()))
    for k, p in model.named_parameters():
        assert p.grad is not None, k
        assert rel_l2(p.grad, leaves[k].grad) < 2e-2, (k, rel_l2(p.grad, leaves[k].grad))
