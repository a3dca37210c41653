"""Host-side checks of MAEViT (no GPU): the masking against the paper's formulation, the constructor's refusals, the sin-cos
tables, the state_dict keys, the restatement tests/_mae_ref.py against a plain-torch transcription of the paper's forward, and
the MAE branch of utils.model_builder._place."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _mae_ref as Ref
from vit_core.ssl.mae import MAEViT
from vit_core.ssl.mae import masking as Mk
from vit_core.ssl.mae.model import sincos_2d_table

TINY = dict(num_blocks=2, input_shape=(3, 24, 24), embed_dim=64, patch_size=8, num_heads=1, mlp_dim=128, decoder_embed_dim=64,
            decoder_blocks=1, decoder_heads=2)


def test_masking_is_the_papers_random_masking():
    B, N, K = 7, 49, Mk.num_kept(49, 0.75)
    assert K == 12
    torch.manual_seed(11)
    keep, restore = Mk.draw_keep(B, N, K)
    torch.manual_seed(11)
    noise = torch.rand(B, N)                                  # the first draw of the step
    ids_shuffle = torch.argsort(noise, dim=1)
    ids_restore = torch.argsort(ids_shuffle, dim=1)
    assert torch.equal(keep, ids_shuffle[:, :K]) and torch.equal(restore, ids_restore)
    mask = torch.ones(B, N)                                   # the paper: 0 is keep, 1 is remove, un-shuffled
    mask[:, :K] = 0
    mask = torch.gather(mask, 1, ids_restore)
    assert torch.equal(Mk.bool_mask(restore, K), mask.bool())
    # keep / restore are inverse permutations; N - K masked patches per row
    assert torch.equal(torch.gather(restore, 1, keep), torch.arange(K).expand(B, K))
    assert torch.equal(torch.sort(restore, dim=1).values, torch.arange(N).expand(B, N))
    assert torch.equal(Mk.bool_mask(restore, K).sum(1), torch.full((B,), N - K))
    assert Mk.draw_keep(2, 9, 2)[0].dtype == torch.int64


def test_index_tables_and_masked_row_order():
    B, N, K = 5, 9, 2
    torch.manual_seed(3)
    keep, restore = Mk.draw_keep(B, N, K)
    idx = Mk.MAEIndices(keep, restore, K)
    mask = (restore >= K).reshape(-1).numpy()
    assert idx.Mm == B * (N - K) and np.array_equal(idx.midx, np.flatnonzero(mask))
    assert np.all(np.diff(idx.midx) > 0)                       # ascending (b, n): the order of SimMIM's pred / targets
    b, n = idx.midx // N, idx.midx % N
    assert np.array_equal(idx.mrows, b * (N + 1) + 1 + n)
    assert np.array_equal(idx.keep_rows.reshape(B, K), keep.numpy() + np.arange(B)[:, None] * N)
    assert np.array_equal(idx.inv[idx.mrows], np.arange(idx.Mm)) and (idx.inv >= 0).sum() == idx.Mm
    assert all(getattr(idx, name).dtype == np.int32 for name in idx.NAMES)
    # a given keep table: the kept patches at their shuffle positions, the masked ones behind them
    r2 = Mk.restore_from_keep(keep, N)
    assert torch.equal(torch.gather(r2, 1, keep), torch.arange(K).expand(B, K)) and torch.equal(r2 >= K, restore >= K)
    assert torch.equal(torch.sort(r2, dim=1).values, torch.arange(N).expand(B, N))
    with pytest.raises(ValueError):
        Mk.restore_from_keep(torch.tensor([[1, 1]]), N)
    with pytest.raises(ValueError):
        Mk.MAEIndices(keep, restore.flip(1), K)


@pytest.mark.parametrize("change,text", [(dict(mask_ratio=0.95), "K must lie"), (dict(mask_ratio=0.0), "K must lie"),
                                         (dict(dropout=0.1), "dropout must be 0"), (dict(num_heads=16), "head dim"),
                                         (dict(decoder_heads=3), "not divisible"), (dict(decoder_embed_dim=96, decoder_heads=1), "multiples of 64"),
                                         (dict(input_shape=(3, 24, 20)), "divisible by patch_size")])
def test_constructor_refusals(change, text):
    with pytest.raises(ValueError, match=text):
        MAEViT(**{**TINY, **change})


def test_constructor_defaults_are_the_papers_decoder():
    m = MAEViT(1, (3, 32, 32), 64, 16, num_heads=1, mlp_dim=64, decoder_blocks=1)
    assert (m.decoder_embed_dim, m.decoder_heads, m.decoder_mlp_dim, m.mask_ratio, m.norm_pix_loss) == (512, 16, 2048, 0.75, True)
    assert m.num_kept == 1 and m.num_patches == 4
    with pytest.raises(TypeError):
        MAEViT(1, (3, 32, 32), 64, 16, 1, 64, 0.0, 0.75, 512)         # the decoder options are keyword-only


def test_sincos_tables():
    for dim, gh, gw in [(64, 3, 3), (128, 2, 5), (192, 14, 14)]:
        got = sincos_2d_table(dim, gh, gw)
        assert got.shape == (1, gh * gw + 1, dim) and got.dtype == torch.float32
        assert torch.equal(got, Ref.sincos_table(dim, gh, gw))
        assert not got[0, 0].any()                               # the CLS row
        # patch (r, c): the first half encodes the column, the second the row; sin block then cos block, frequency 0 first
        r, c = gh - 1, gw - 2
        row = got[0, 1 + r * gw + c]
        q = dim // 4
        assert row[0] == np.float32(math.sin(c)) and row[q] == np.float32(math.cos(c))
        assert row[2 * q] == np.float32(math.sin(r)) and row[3 * q] == np.float32(math.cos(r))
    m = MAEViT(**TINY)
    assert torch.equal(m.pos_embed, Ref.sincos_table(64, 3, 3)) and torch.equal(m.decoder_pos_embed, Ref.sincos_table(64, 3, 3))
    assert not m.pos_embed.requires_grad and "pos_embed" not in dict(m.named_parameters())


def _block_keys(prefix):
    leaves = ["self_attention.w_query.weight", "self_attention.w_key.weight", "self_attention.w_value.weight", "self_attention.final_linear.weight",
              "feed_forward.linear_in.weight", "feed_forward.linear_in.bias", "feed_forward.linear_out.weight", "feed_forward.linear_out.bias",
              "layer_norm1.weight", "layer_norm1.bias", "layer_norm2.weight", "layer_norm2.bias"]
    return [prefix + leaf for leaf in leaves]


def test_state_dict_keys_and_token_init():
    torch.manual_seed(0)
    m = MAEViT(**{**TINY, "embed_dim": 256, "num_heads": 4, "decoder_embed_dim": 256})
    want = (["cls_token", "mask_token", "pos_embed", "decoder_pos_embed"] + _block_keys("encoder_blocks.0.") + _block_keys("encoder_blocks.1.")
            + ["projection.weight", "projection.bias", "norm.weight", "norm.bias", "decoder_embed.weight", "decoder_embed.bias"]
            + _block_keys("decoder_blocks.0.") + ["decoder_norm.weight", "decoder_norm.bias", "decoder_pred.weight", "decoder_pred.bias"])
    assert sorted(m.state_dict()) == sorted(want)
    # registration order of the submodules (the module's own tokens and buffers lead, as in every nn.Module)
    order = []
    for k in m.state_dict():
        if "." in k and k.split(".")[0] not in order:
            order.append(k.split(".")[0])
    assert order == ["encoder_blocks", "projection", "norm", "decoder_embed", "decoder_blocks", "decoder_norm", "decoder_pred"]
    assert m.cls_token.shape == (1, 1, 256) and m.mask_token.shape == (1, 1, 256)
    for tok in (m.cls_token, m.mask_token):                      # normal(std = 0.02)
        assert 0.012 < float(tok.detach().std()) < 0.028 and float(tok.detach().abs().max()) < 0.1
    assert m.projection.weight.shape == (256, 192) and m.decoder_pred.weight.shape == (192, 256)


# ---- the restatement against a plain-torch transcription of the paper's forward ---------------------------------------------
def _attention(x, sd, pre, heads):
    B, T, D = x.shape
    q, k, v = (F.linear(x, sd[pre + f"w_{n}.weight"]).view(B, T, heads, D // heads).transpose(1, 2) for n in ("query", "key", "value"))
    att = F.softmax(q @ k.transpose(-2, -1) * (D // heads) ** -0.5, dim=-1)
    return F.linear((att @ v).transpose(1, 2).reshape(B, T, D), sd[pre + "final_linear.weight"])


def _block(x, sd, pre, heads):
    D = x.shape[-1]
    x = x + _attention(F.layer_norm(x, (D,), sd[pre + "layer_norm1.weight"], sd[pre + "layer_norm1.bias"]), sd, pre + "self_attention.", heads)
    h = F.layer_norm(x, (D,), sd[pre + "layer_norm2.weight"], sd[pre + "layer_norm2.bias"])
    h = F.linear(F.gelu(F.linear(h, sd[pre + "feed_forward.linear_in.weight"], sd[pre + "feed_forward.linear_in.bias"])),
                 sd[pre + "feed_forward.linear_out.weight"], sd[pre + "feed_forward.linear_out.bias"])
    return x + h


def paper_forward(sd, imgs, noise, patch, heads, dec_heads, blocks, dec_blocks, mask_ratio, norm_pix):
    """forward_encoder / forward_decoder / forward_loss of the paper's published model, statement by statement, on this
    project's parameter names and its (c, kh, kw) patch features.  -> (loss, pred [B, N, Pd], mask [B, N], target [B, N, Pd])"""
    x = F.linear(F.unfold(imgs, patch, stride=patch).transpose(1, 2), sd["projection.weight"], sd["projection.bias"])      # patch_embed
    x = x + sd["pos_embed"][:, 1:, :]
    N, L, D = x.shape                                            # random_masking
    len_keep = int(L * (1 - mask_ratio))
    ids_shuffle = torch.argsort(noise, dim=1)
    ids_restore = torch.argsort(ids_shuffle, dim=1)
    ids_keep = ids_shuffle[:, :len_keep]
    x = torch.gather(x, dim=1, index=ids_keep.unsqueeze(-1).repeat(1, 1, D))
    mask = torch.ones([N, L])
    mask[:, :len_keep] = 0
    mask = torch.gather(mask, dim=1, index=ids_restore)
    cls_tokens = (sd["cls_token"] + sd["pos_embed"][:, :1, :]).expand(x.shape[0], -1, -1)
    x = torch.cat((cls_tokens, x), dim=1)
    for i in range(blocks):
        x = _block(x, sd, f"encoder_blocks.{i}.", heads)
    x = F.layer_norm(x, (D,), sd["norm.weight"], sd["norm.bias"])
    x = F.linear(x, sd["decoder_embed.weight"], sd["decoder_embed.bias"])                                                  # forward_decoder
    mask_tokens = sd["mask_token"].repeat(x.shape[0], ids_restore.shape[1] + 1 - x.shape[1], 1)
    x_ = torch.cat([x[:, 1:, :], mask_tokens], dim=1)
    x_ = torch.gather(x_, dim=1, index=ids_restore.unsqueeze(-1).repeat(1, 1, x.shape[2]))
    x = torch.cat([x[:, :1, :], x_], dim=1)
    x = x + sd["decoder_pos_embed"]
    for i in range(dec_blocks):
        x = _block(x, sd, f"decoder_blocks.{i}.", dec_heads)
    x = F.layer_norm(x, (x.shape[-1],), sd["decoder_norm.weight"], sd["decoder_norm.bias"])
    pred = F.linear(x, sd["decoder_pred.weight"], sd["decoder_pred.bias"])[:, 1:, :]
    target = F.unfold(imgs, patch, stride=patch).transpose(1, 2)                                                           # forward_loss
    if norm_pix:
        mean = target.mean(dim=-1, keepdim=True)
        var = target.var(dim=-1, keepdim=True)
        target = (target - mean) / (var + 1.e-6) ** .5
    loss = ((pred - target) ** 2).mean(dim=-1)
    return (loss * mask).sum() / mask.sum(), pred, mask, target


@pytest.mark.parametrize("norm_pix", [True, False])
def test_restatement_equals_the_papers_forward(norm_pix):
    torch.manual_seed(5)
    m = MAEViT(**TINY, norm_pix_loss=norm_pix)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    for k in sd:                                                  # biases and norms away from their 0 / 1 initial values
        if k.endswith(".bias") or "norm" in k:
            sd[k] = sd[k] + 0.1 * torch.randn_like(sd[k])
    B, N, K = 4, 9, 2
    imgs, noise = torch.rand(B, 3, 24, 24), torch.rand(B, N)
    keep, restore, mask = Ref.shuffle(noise, K)
    pred, raw = Ref.forward(sd, imgs, keep, restore, 8, 1, 2, emu=None)
    loss, t64 = Ref.loss64(pred, raw, norm_pix)
    want_loss, want_pred, want_mask, want_target = paper_forward(sd, imgs, noise, 8, 1, 2, 2, 1, 0.75, norm_pix)
    assert torch.equal(mask, want_mask.bool())
    assert float((pred - want_pred[mask]).abs().max()) < 1e-5
    assert float((t64.float() - want_target[mask]).abs().max()) < 1e-5
    assert abs(float(loss) - float(want_loss)) < 1e-5 * max(1.0, float(want_loss))
    inf = Ref.inference(sd, imgs, 8, 1)
    assert inf.shape == (B, N, 64)


# ---- the MAE branch of utils.model_builder._place -------------------------------------------------------------------------------
def test_place_carries_an_mae_checkpoint_into_a_vit_and_leaves_simmim_alone():
    from utils.model_builder import _MAE_MARK, _place
    from vit_core.ssl.simmim import SimMIMViT
    from vit_core.vit import ViT
    torch.manual_seed(2)
    mae = MAEViT(**TINY)
    source = {k: v.detach().clone() for k, v in mae.state_dict().items()}
    vit = ViT(num_classes=5, num_blocks=2, input_shape=(3, 24, 24), embed_dim=64, patch_size=8, num_heads=1, mlp_dim=128, dropout=0.0)
    target = vit.state_dict()
    assert _MAE_MARK in source and _MAE_MARK not in target
    placed, skipped = {}, {}
    for k, v in source.items():
        dst, res = _place(k, v, target, mae=True)
        if dst is None:
            skipped[k] = res
        else:
            assert dst not in placed
            placed[dst] = res
    # every tensor below the classification head lands
    assert set(placed) == {k for k in target if not k.startswith("classification_head.")}
    for k in target:
        if k.startswith("encoder_blocks."):
            assert torch.equal(placed[k], source[k])
    assert torch.equal(placed["patch_embedding.conv.weight"], source["projection.weight"].reshape(64, 3, 8, 8))
    assert torch.equal(placed["patch_embedding.conv.bias"], source["projection.bias"])
    assert torch.equal(placed["patch_embedding.cls_token"], source["cls_token"])
    assert torch.equal(placed["patch_embedding.positional_embedding"], source["pos_embed"])
    # the same linear map: the convolution of the reshaped weight is the projection of the unfolded patches
    x = torch.rand(2, 3, 24, 24)
    conv = F.conv2d(x, placed["patch_embedding.conv.weight"], placed["patch_embedding.conv.bias"], stride=8).flatten(2).transpose(1, 2)
    lin = F.linear(F.unfold(x, 8, stride=8).transpose(1, 2), source["projection.weight"], source["projection.bias"])
    assert float((conv - lin).abs().max()) < 1e-5
    # the decoder, the final norm and the mask token are skipped with their reason
    assert set(skipped) == {k for k in source if k == "mask_token" or k.startswith(("norm.", "decoder_"))}
    assert set(skipped.values()) == {"pre-training-only tensor"}
    vit.load_state_dict(placed, strict=False)
    # a SimMIM state dict is placed exactly as before (the branch is not taken: the default, and what load_weights passes)
    sim = SimMIMViT(num_blocks=2, input_shape=(3, 24, 24), embed_dim=64, patch_size=8, num_heads=1, mlp_dim=128, dropout=0.0).state_dict()
    assert _MAE_MARK not in sim
    for k, v in sim.items():
        dst, res = _place(k, v, target)
        dst2, res2 = _place(k, v, target, mae=False)
        assert dst == dst2 and (torch.equal(res, res2) if dst is not None else res == res2)
        if k.startswith("projection."):
            assert dst is None or dst == "patch_embedding." + k
        elif k == "positional_embedding":
            assert dst == "patch_embedding.positional_embedding" and torch.equal(res[:, 1:], v) and not res[:, 0].any()
        elif k in ("mask_token",) or k.startswith("simmim_head."):
            assert dst is None and res == "pre-training-only tensor"
        else:
            assert dst == k and torch.equal(res, v)


def test_load_weights_and_build_model_mode_mae(tmp_path):
    from utils.model_builder import build_model, load_weights
    from vit_core.vit import ViT
    cfg = {"training": {"type": "mae"}, "data": {"img_size": 24},
           "model": {"in_channels": 3, "patch_size": 8, "embed_dim": 64, "num_blocks": 2, "num_heads": 1, "mlp_dim": 128, "dropout": 0.0,
                     "mask_ratio": 0.75, "decoder_embed_dim": 64, "decoder_blocks": 1, "decoder_heads": 2, "norm_pix_loss": False}}
    m = build_model(cfg)
    assert isinstance(m, MAEViT) and (m.decoder_embed_dim, m.decoder_heads, len(m.decoder_blocks), m.norm_pix_loss) == (64, 2, 1, False)
    del cfg["model"]["norm_pix_loss"], cfg["model"]["mask_ratio"]
    assert build_model(cfg).norm_pix_loss is True and build_model(cfg).mask_ratio == 0.75
    with pytest.raises(ValueError, match="drop_path_rate"):
        build_model({**cfg, "model": {**cfg["model"], "drop_path_rate": 0.1}})
    path = tmp_path / "mae.pth"
    torch.save({"model_state_dict": m.state_dict()}, path)
    vit = ViT(num_classes=5, num_blocks=2, input_shape=(3, 24, 24), embed_dim=64, patch_size=8, num_heads=1, mlp_dim=128, dropout=0.0)
    load_weights(vit, str(path))
    assert torch.equal(vit.patch_embedding.conv.weight.detach().reshape(64, -1), m.projection.weight.detach())
    assert torch.equal(vit.encoder_blocks[1].feed_forward.linear_out.weight, m.encoder_blocks[1].feed_forward.linear_out.weight)
    again = MAEViT(**TINY)                                        # and an MAE checkpoint loads into an MAEViT key for key
    load_weights(again, str(path))
    assert all(torch.equal(v, m.state_dict()[k]) for k, v in again.state_dict().items())


def test_trainer_refuses_pixel_metrics_on_normalised_targets():
    from torch import nn
    from utils.trainers import MAETrainer, SimMIMTrainer
    assert issubclass(MAETrainer, SimMIMTrainer)

    def cfg(metrics, criterion="MSELoss"):
        c = {"training": {"type": "mae", "num_epochs": 2, "warmup_epochs": 1, "warmup_initial_learning_rate": 1e-6,
                          "warmup_final_learning_rate": 1e-3, "criterion": {"name": criterion, "params": {"reduction": "mean"}},
                          "optimizer": {"name": "SGD", "params": {"lr": 1e-3}},
                          "lr_scheduler": {"main": {"name": "CosineAnnealingLR", "params": {"eta_min": 1e-6}}, "warmup": {"params": {}}}},
             "eval": {}, "data": {"img_size": 24}}
        if metrics:
            c["metrics"] = metrics
        return c

    data = [torch.rand(2, 3, 24, 24)]
    for metrics in (["PSNR", "SSIM"], ["SSIM"], ["PSNR"]):
        with pytest.raises(ValueError, match="norm_pix_loss"):
            MAETrainer(MAEViT(**TINY), "unused", cfg(metrics), data, data, "cpu")
        MAETrainer(MAEViT(**TINY, norm_pix_loss=False), "unused", cfg(metrics), data, data, "cpu")      # raw pixels: as for SimMIM
    tr = MAETrainer(MAEViT(**TINY), "unused", cfg(None), data, data, "cpu")
    assert isinstance(tr.criterion, nn.MSELoss) and not tr._fused_ok()                                  # SGD: the autograd path
