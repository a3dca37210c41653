"""Global average pooling without a GPU: the restatement of tests/_pool_ref.py against the oracle, that the bit comparison the
kernel tests make tells a wrong mean from the right one, and the Python surface (ViT's keyword, the state dict, the config key)."""
import pytest
import torch

import _pool_ref as PR
from oracle import vit_oracle as O

TINY = dict(num_classes=5, num_blocks=2, input_shape=(3, 24, 24), embed_dim=64, patch_size=8, num_heads=1, mlp_dim=128, dropout=0.0)


def _vit(**kw):
    from vit_core.vit import ViT
    return ViT(**{**TINY, **kw})


@pytest.mark.parametrize("emu", [None, "bf16"], ids=["fp32", "bf16"])
def test_the_cls_restatement_is_the_oracle_bit_for_bit(emu):
    torch.manual_seed(0)
    sd = {k: v.detach().clone() for k, v in _vit().state_dict().items()}
    x = torch.rand(3, 3, 24, 24)
    mine, probs = PR.vit_forward(sd, x, 8, 1, "cls", emu, return_attn=True)
    want, wprobs = O.vit_forward(sd, x, 8, 1, emu=emu, return_attn=True)
    assert torch.equal(mine.view(torch.int32), want.view(torch.int32)) and torch.equal(probs, wprobs)
    assert torch.equal(PR.vit_forward(sd, x, 8, 1, "cls", emu), want)
    assert not torch.equal(PR.vit_forward(sd, x, 8, 1, "avg", emu), want)      # and the other mode is another function


def test_the_restated_kernels():
    B, T, D = 2, 5, 8
    x = torch.arange(B * T * D, dtype=torch.float32).view(B * T, D)
    out = PR.pool_fwd(x, B, T)
    assert out.dtype == torch.float32 and out.shape == (B, D)
    assert torch.equal(out, x.view(B, T, D)[:, 1:].sum(1) * 0.25)             # T - 1 = 4: the scale is exact
    g = PR.pool_bwd(out, B, T).view(B, T, D)
    assert not g[:, 0].view(torch.int32).any()                                  # +0, not -0
    assert all(torch.equal(g[:, t], out * 0.25) for t in range(1, T))
    assert PR.scale(4) == float(torch.tensor(1.0) / torch.tensor(3.0)) != 1.0 / 3.0      # the fp32 quotient


@pytest.mark.parametrize("B,T,D", [(1, 2, 64), (3, 3, 64), (5, 17, 128), (1, 197, 768)], ids=str)
def test_the_bit_comparison_tells_a_wrong_mean_from_the_right_one(B, T, D):
    """What tests/test_gpu_pool_kernels.py does with the kernel's result, done here with three wrong means."""
    g = torch.Generator().manual_seed(T)
    x = torch.randint(-8, 9, (B, T, D), generator=g).float()
    x[:, 0] = 7.0                                                               # a CLS row that shows when it is read
    x[:, -1] += 9.0                                                             # and a last token that shows when it is dropped
    want = PR.pool_fwd(x.view(B * T, D), B, T)
    r = torch.tensor(PR.scale(T))
    same = lambda got: torch.equal(got.view(torch.int32), want.view(torch.int32))      # noqa: E731
    assert same(x[:, 1:].flip(1).sum(1) * r)                                   # integers: any order gives the same bits
    assert not same(x.sum(1) * r), "a mean that includes the CLS row passes"
    assert not same(x[:, 1:].sum(1) * torch.tensor(1.0 / T)), "a mean that divides by T passes"
    if T > 2:
        assert not same(x[:, 1:-1].sum(1) * r), "a mean that drops the last token passes"
    else:
        assert not same(torch.zeros(B, D)), "a mean of no token passes"


def test_vit_takes_cls_and_avg_and_nothing_else():
    assert _vit().global_pool == "cls" and _vit(global_pool="avg").global_pool == "avg"
    for bad in ("max", "token", "", None):
        with pytest.raises(ValueError, match="global_pool"):
            _vit(global_pool=bad)


def test_the_state_dict_does_not_know_the_mode():
    torch.manual_seed(1)
    a = _vit()
    torch.manual_seed(1)
    b = _vit(global_pool="avg")
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert [n for n, _ in a.named_parameters()] == [n for n, _ in b.named_parameters()]
    assert [n for n, _ in a.named_buffers()] == [n for n, _ in b.named_buffers()]
    a.load_state_dict(sb)                                                       # and the checkpoints are interchangeable
    b.load_state_dict(sa)


def _cfg(mode, **model):
    return {"training": {"type": mode}, "data": {"img_size": 24},
            "model": {"in_channels": 3, "patch_size": 8, "embed_dim": 64, "num_blocks": 2, "num_heads": 1, "mlp_dim": 128, "dropout": 0.0,
                      "num_classes": 5, "mask_ratio": 0.5, "output_dim": 64, "center_momentum": 0.9, **model}}


def test_build_model_reads_the_key_for_the_supervised_vit_and_refuses_it_elsewhere(tmp_path):
    from utils.model_builder import build_model
    from vit_core.vit import ViT
    assert build_model(_cfg("supervised")).global_pool == "cls"
    assert build_model(_cfg("supervised", global_pool="cls")).global_pool == "cls"
    m = build_model(_cfg("supervised", global_pool="avg"))
    assert isinstance(m, ViT) and m.global_pool == "avg"
    with pytest.raises(ValueError, match="global_pool"):
        build_model(_cfg("supervised", global_pool="max"))
    for mode in ("simmim", "dino", "mae"):
        build_model(_cfg(mode))                                                 # the configuration itself builds
        for value in ("avg", "cls"):
            with pytest.raises(ValueError, match=rf"'{mode}'.*global_pool"):
                build_model(_cfg(mode, global_pool=value))
    # finetune: the key is read, and a pre-training checkpoint lands where it lands without it
    path = tmp_path / "pre.pth"
    torch.save({"model_state_dict": build_model(_cfg("simmim")).state_dict()}, path)
    cfg = _cfg("finetune", global_pool="avg")
    cfg["training"]["pretrained_path"] = str(path)
    torch.manual_seed(3)
    avg = build_model(cfg)
    cfg["model"].pop("global_pool")
    torch.manual_seed(3)
    cls = build_model(cfg)
    assert (avg.global_pool, cls.global_pool) == ("avg", "cls")
    sa, sc = avg.state_dict(), cls.state_dict()
    assert list(sa) == list(sc) and all(torch.equal(sa[k], sc[k]) for k in sa)
    fresh = torch.nn.LayerNorm(64)                                              # the head norm: MAE's fc_norm, at its fresh initialisation
    assert torch.equal(sa["classification_head.norm.weight"], fresh.weight) and torch.equal(sa["classification_head.norm.bias"], fresh.bias)


def test_the_source_and_the_wrappers_are_there():
    import __graft_entry__ as ge
    assert "pool.hip" in ge.SOURCES and "elementwise.hip" in ge.SOURCES
    from vitssl_hip import ops
    assert callable(ops.pool_tokens_fwd) and callable(ops.pool_tokens_bwd)
    from vit_core._backbone import POOLS
    assert POOLS == PR.POOLS == ("cls", "avg")
