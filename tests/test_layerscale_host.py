"""LayerScale without a GPU: the constructors and the config key, the state_dict keys and the flat store's layout, the optimizer's
per-parameter rules for the new names, checkpoints without the keys, freeze_backbone, the C ABI's symbol list and argument checks,
and the reference of the GPU tests (tests/_layerscale_ref.py): the oracle's keep route against a plain restatement of
x + g (.) branch, and the negative control of the model tests, oracle against oracle with g1 / g2 swapped."""
import ctypes
import logging
import os
import re
import sys

import pytest
import torch

import _layerscale_ref as LS
from _util import rel_l2
from oracle import vit_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(num_blocks=3, input_shape=(3, 32, 32), embed_dim=64, patch_size=16, num_heads=1, mlp_dim=64, dropout=0.0)
INIT = 1e-5


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    import vitssl_hip
    return vitssl_hip


def _makers():
    from vit_core import EncoderBlock, ViT
    from vit_core.ssl.dino.model import DINOViT, ViTBackbone
    from vit_core.ssl.simmim import SimMIMViT
    return {
        "ViT": lambda **e: ViT(num_classes=5, **KW, **e),
        "SimMIMViT": lambda **e: SimMIMViT(**KW, **e),
        "DINOViT": lambda **e: DINOViT(output_dim=64, **KW, **e),
        "ViTBackbone": lambda **e: ViTBackbone(**KW, **e),
        "EncoderBlock": lambda **e: EncoderBlock(64, 1, 64, 0.0, **e),
    }


WHO = ["ViT", "SimMIMViT", "DINOViT", "ViTBackbone", "EncoderBlock"]


# ------------------------------------------------------------------------------------------------ constructors, keys, layout
@pytest.mark.parametrize("who", WHO)
def test_keys_exist_only_with_the_keyword_and_hold_init(built, who):
    make = _makers()[who]
    torch.manual_seed(3)
    plain = make()
    state = torch.get_rng_state()
    torch.manual_seed(3)
    none, ls = make(layer_scale_init=None), None
    torch.manual_seed(3)
    ls = make(layer_scale_init=INIT)
    assert torch.equal(torch.get_rng_state(), state), "LayerScale must not draw from the generator"
    assert list(none.state_dict()) == list(plain.state_dict())
    new = [k for k in ls.state_dict() if k not in plain.state_dict()]
    blocks = 1 if who == "EncoderBlock" else KW["num_blocks"]
    stacks = ["teacher_backbone.", "student_backbone."] if who == "DINOViT" else [""]
    want = [f"{s}{'' if who == 'EncoderBlock' else f'encoder_blocks.{i}.'}layer_scale{k}.gamma" for s in stacks for i in range(blocks) for k in (1, 2)]
    assert sorted(new) == sorted(want) and len(new) == 2 * blocks * len(stacks)
    for k in new:
        assert ls.state_dict()[k].shape == (64,) and bool((ls.state_dict()[k] == torch.tensor(INIT)).all())
    for k, v in plain.state_dict().items():                                  # every other tensor: the same initial values
        assert torch.equal(ls.state_dict()[k], v), k
    assert [k for k in ls.state_dict() if k in plain.state_dict()] == list(plain.state_dict())      # ... in the same order
    if who == "DINOViT":                                                     # the teacher's gammas are frozen like the teacher
        assert all(not p.requires_grad for n, p in ls.named_parameters() if n.startswith("teacher_"))
        assert all(p.requires_grad for n, p in ls.named_parameters() if n.startswith("student_") and "layer_scale" in n)


@pytest.mark.parametrize("who", WHO)
@pytest.mark.parametrize("bad", [0, 0.0, -1e-5, float("nan"), float("inf"), "1e-5", True])
def test_bad_values_are_value_errors(built, who, bad):
    with pytest.raises(ValueError, match="layer_scale_init"):
        _makers()[who](layer_scale_init=bad)


def test_layer_scale_module_is_exported(built):
    import vit_core
    m = vit_core.LayerScale(8, 0.5)
    assert "LayerScale" in vit_core.__all__ and list(m.state_dict()) == ["gamma"] and bool((m.gamma == 0.5).all())
    with pytest.raises(ValueError):
        vit_core.LayerScale(8, 0.0)


def test_store_layout_keeps_every_other_offset(built):
    """inside a block every existing parameter keeps its offset from the block's start (the gammas come last, so the fused-QKV span
    stays one view); block 0 keeps its absolute offsets; the gammas lie inside the block's prefix_span"""
    from vitssl_hip import engine as E
    mk = _makers()["ViT"]
    cpu = torch.device("cpu")
    st0, st = E.FlatStore(mk(), cpu), E.FlatStore(mk(layer_scale_init=INIT), cpu)
    for i in range(KW["num_blocks"]):
        pre = f"encoder_blocks.{i}."
        base0, base = st0.prefix_span(pre)[0], st.prefix_span(pre)[0]
        for n in st0.names:
            if n.startswith(pre):
                assert st.offsets[n][0] - base == st0.offsets[n][0] - base0 and st.offsets[n][1] == st0.offsets[n][1], n
        lo, hi = st.prefix_span(pre)
        for k in (1, 2):
            o, n = st.offsets[f"{pre}layer_scale{k}.gamma"]
            assert lo <= o and o + n <= hi and n == 64
        assert st.offsets[f"{pre}layer_scale1.gamma"][0] > max(st.offsets[n][0] for n in st0.names if n.startswith(pre))
        st.span_view(pre + "self_attention.w_query.weight", pre + "self_attention.w_value.weight", (3 * 64, 64))
    assert all(st.offsets[n] == st0.offsets[n] for n in st0.names if n.startswith("encoder_blocks.0."))
    prefixes = [f"encoder_blocks.{i}." for i in range(KW["num_blocks"])]
    assert E.EncoderStack(st, prefixes, 64, 1, 64, 0.0, layer_scale=True).layer_scale
    assert not E.EncoderStack(st0, prefixes, 64, 1, 64, 0.0).layer_scale
    from vitssl_hip import _lib as L
    with pytest.raises(L.VitsslError, match=r"encoder_blocks\.0\.layer_scale1\.gamma"):
        E.EncoderStack(st0, prefixes, 64, 1, 64, 0.0, layer_scale=True)      # the missing key is named


def test_fp8_operands_are_refused_at_construction(built):
    from vit_core import ViT
    from vitssl_hip import _lib as L
    from vitssl_hip import engine as E
    cpu = torch.device("cpu")
    E.set_linear_operands("fp8")
    try:
        m = ViT(5, 2, (3, 32, 32), 128, 16, 2, 128, 0.0, layer_scale_init=INIT)
        args = (E.FlatStore(m, cpu), ["encoder_blocks.0.", "encoder_blocks.1."], 128, 2, 128, 0.0)
        with pytest.raises(L.VitsslError, match="bf16"):
            E.EncoderStack(*args, layer_scale=True)
        assert E.EncoderStack(*args).fp8                                    # without LayerScale fp8 stacks build as before
    finally:
        E.set_linear_operands("bf16")


# ------------------------------------------------------------------------------------------------ config, optimizer rules, checkpoints
def _cfg(mode, **model_extra):
    model = {"in_channels": 3, "patch_size": 16, "embed_dim": 64, "num_blocks": 3, "num_heads": 1, "mlp_dim": 64, "dropout": 0.0,
             "mask_ratio": 0.6, "num_classes": 5, "output_dim": 64, "center_momentum": 0.9}
    model.update(model_extra)
    return {"training": {"type": mode}, "eval": {}, "data": {"img_size": 32}, "model": model}


@pytest.mark.parametrize("mode", ["supervised", "simmim", "dino"])
def test_build_model_reads_the_optional_key(built, mode):
    from utils.model_builder import build_model
    plain = build_model(_cfg(mode))
    assert plain.layer_scale_init is None and not any("layer_scale" in k for k in plain.state_dict())
    assert build_model(_cfg(mode, layer_scale_init=None)).layer_scale_init is None
    m = build_model(_cfg(mode, layer_scale_init=1e-4, drop_path_rate=0.1))
    assert m.layer_scale_init == 1e-4 and m.drop_path_rate == 0.1
    assert sum("layer_scale" in k for k in m.state_dict()) == 2 * 3 * (2 if mode == "dino" else 1)
    for bad in (0.0, -1.0, "x"):
        with pytest.raises(ValueError):
            build_model(_cfg(mode, layer_scale_init=bad))


def test_new_names_are_exempt_from_weight_decay_and_take_the_blocks_layer_id(built):
    from vitssl_hip.engine import exempt_from_weight_decay, layer_id, num_layers
    m = _makers()["ViT"](layer_scale_init=INIT)
    names = [n for n, _ in m.named_parameters()]
    assert num_layers(names) == 3
    for pre in ("", "student_backbone."):
        for i in range(3):
            for k in (1, 2):
                n = f"{pre}encoder_blocks.{i}.layer_scale{k}.gamma"
                assert exempt_from_weight_decay(n, 1) and layer_id(n, 3) == i + 1


def test_load_weights_leaves_missing_gammas_at_init(built, tmp_path, caplog):
    from utils.model_builder import load_weights
    mk = _makers()["ViT"]
    torch.manual_seed(1)
    old = mk()
    path = str(tmp_path / "old.pt")
    torch.save({"model_state_dict": old.state_dict()}, path)
    torch.manual_seed(2)
    new = mk(layer_scale_init=INIT)
    with caplog.at_level(logging.WARNING):
        load_weights(new, path)
    assert "left at their initial values" in caplog.text and "layer_scale1.gamma" in caplog.text
    sd = new.state_dict()
    for k, v in old.state_dict().items():
        assert torch.equal(sd[k], v)
    assert all(bool((v == torch.tensor(INIT)).all()) for k, v in sd.items() if "layer_scale" in k)
    # and a checkpoint WITH the keys restores them
    with torch.no_grad():
        new.encoder_blocks[1].layer_scale2.gamma.fill_(0.25)
    torch.save(new.state_dict(), path)
    again = load_weights(mk(layer_scale_init=INIT), path)
    assert bool((again.encoder_blocks[1].layer_scale2.gamma == 0.25).all())


def test_freeze_backbone_freezes_the_gammas(built):
    from utils.model_builder import freeze_backbone
    m = _makers()["ViT"](layer_scale_init=INIT)
    freeze_backbone(m)
    assert all(not p.requires_grad for n, p in m.named_parameters() if "layer_scale" in n)
    assert m.patch_embedding.cls_token.requires_grad


# ------------------------------------------------------------------------------------------------ C ABI
def test_header_symbols_equal_the_prototypes_and_the_library_exports_them(built):
    from vitssl_hip import _lib as L
    want = {"vitssl_gemm_bf16_nt_ls", "vitssl_layernorm_bwd_ls", "vitssl_grad_mask_cast_ls", "vitssl_layerscale_workspace_floats"}
    assert set(L.header_symbols("layerscale")) == want == set(L.REGISTRY["layerscale"])
    raw = ctypes.CDLL(built.LIB_PATH)
    for s in want:
        assert hasattr(raw, s), f"{s} declared in include/vitssl_layerscale.h but not exported"
    # the other headers keep their symbol lists, vitssl_hip.h its version
    assert not want & set(L.header_symbols()) and not want & set(L.REGISTRY["hip"]) and not want & set(L.header_symbols("droppath"))
    assert built.lib().vitssl_version() == L.ABI_VERSION == 3
    txt = re.sub(r"/\*.*?\*/", "", open(L.HEADERS["layerscale"]).read(), flags=re.S)
    assert re.search(r"typedef struct \{\s*const float\* gamma;\s*int cols;\s*\} vitssl_colscale_t;", txt)
    assert ctypes.sizeof(L.ColScale) == 16


def test_workspace_query_covers_four_sums_and_never_undercuts_the_common_one(built):
    lib = built.lib()
    assert lib.vitssl_layerscale_workspace_floats(0, 64) == 0
    for rows, cols in ((1, 4), (64, 64), (272, 384), (591, 384), (591, 768), (50432, 768), (50432, 384), (80, 2048)):
        need, base = lib.vitssl_layerscale_workspace_floats(rows, cols), lib.vitssl_sum_workspace_floats(rows, cols)
        assert need >= base and need >= 4 * min((rows + 3) // 4, 2 * 8) * cols      # (at least 8 CUs on any device)


def test_argument_errors_are_reported_before_any_launch(built):
    from vitssl_hip import _lib as L
    lib = built.lib()
    g, c, r = L.Gemm(), L.ColScale(), L.RowScale()
    assert lib.vitssl_gemm_bf16_nt_ls(ctypes.byref(g), None, None, None, None) == -1 and b"null column scales" in lib.vitssl_last_error()
    assert lib.vitssl_gemm_bf16_nt_ls(ctypes.byref(g), ctypes.byref(c), None, None, None) == -1 and b"null operand" in lib.vitssl_last_error()
    fake = ctypes.c_void_p(256)                                              # never dereferenced: every call below is refused first
    drop = L.Dropout(0.0, 0, 0)
    c.gamma, c.cols = 256, 60
    assert lib.vitssl_grad_mask_cast_ls(fake, fake, None, drop, None, ctypes.byref(c), fake, fake, 16, 64, None, 0, None) == -1
    assert b"column scales hold 60" in lib.vitssl_last_error()
    c.cols = 64
    assert lib.vitssl_grad_mask_cast_ls(fake, fake, None, drop, None, ctypes.byref(c), fake, None, 16, 64, None, 0, None) == -1
    assert b"together" in lib.vitssl_last_error()
    assert lib.vitssl_grad_mask_cast_ls(fake, fake, None, drop, None, None, fake, fake, 16, 64, None, 0, None) == -1
    r.scale, r.groups, r.rows_per_group = 256, 3, 5                          # 15 rows
    assert lib.vitssl_grad_mask_cast_ls(fake, fake, None, drop, ctypes.byref(r), ctypes.byref(c), fake, fake, 16, 64, None, 0, None) == -1
    assert b"must equal rows" in lib.vitssl_last_error()
    assert lib.vitssl_grad_mask_cast_ls(fake, fake, None, drop, None, ctypes.byref(c), fake, fake, 16, 64, None, 0, None) == -1
    assert b"vitssl_layerscale_workspace_floats" in lib.vitssl_last_error()  # no workspace: refused, nothing launched
    assert lib.vitssl_layernorm_bwd_ls(fake, fake, fake, fake, fake, None, fake, None, fake, fake, None, drop, None, ctypes.byref(c), fake, fake,
                                       16, 64, None, 0, None) == -1 and b"null pointer" in lib.vitssl_last_error()      # gm_bf16 is required
    assert lib.vitssl_layernorm_bwd_ls(fake, fake, fake, fake, fake, None, fake, fake, fake, fake, None, drop, None, ctypes.byref(c), fake, fake,
                                       16, 64, None, 0, None) == -1 and b"vitssl_layerscale_workspace_floats" in lib.vitssl_last_error()


# ------------------------------------------------------------------------------------------------ the reference
def _block_sd(D=32, F=64, seed=4):
    from vit_core import EncoderBlock
    torch.manual_seed(seed)
    blk = EncoderBlock(D, 2, F, 0.0, layer_scale_init=INIT)
    sd = {k: v.detach().clone() for k, v in blk.state_dict().items()}
    sd.update(LS.random_gammas(sd, D))
    return sd


def test_oracle_keep_route_equals_the_plain_restatement():
    """fp32 oracle with keep = (g1 * ones, ones, g2 * ones) against x + g (.) branch in plain torch: output and d g1 / d g2"""
    D, F, B, T = 32, 64, 3, 7
    sd = _block_sd(D, F)
    x = torch.randn(B, T, D, generator=torch.Generator().manual_seed(5))
    w = torch.randn(B, T, D, generator=torch.Generator().manual_seed(6))
    grads = []
    for fn in (lambda s: LS.block_forward(s, x, 2, D, F, emu=None), lambda s: LS.plain_block(x, s, "", 2)):
        leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        y = fn(leaves)
        (y * w).sum().backward()
        grads.append((y.detach(), leaves["layer_scale1.gamma"].grad, leaves["layer_scale2.gamma"].grad))
    (y1, a1, b1), (y2, a2, b2) = grads
    assert rel_l2(y1, y2) < 1e-6 and rel_l2(a1, a2) < 1e-5 and rel_l2(b1, b2) < 1e-5
    assert float(a2.abs().max()) > 0 and float(b2.abs().max()) > 0
    # with emu="bf16" the gradients flow the same way
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    (LS.block_forward(leaves, x, 2, D, F, emu="bf16") * w).sum().backward()
    assert rel_l2(leaves["layer_scale1.gamma"].grad, a2) < 2e-2 and rel_l2(leaves["layer_scale2.gamma"].grad, b2) < 2e-2


def test_negative_control_exceeds_the_gradient_bar():
    """what tests/test_gpu_layerscale_models.py relies on: the reference with g1 / g2 of one block swapped differs from the
    reference by more than the 2e-2 gradient bar (oracle against oracle, tiny ViT)"""
    from vit_core import ViT
    D, F = 64, 64
    torch.manual_seed(7)
    m = ViT(num_classes=5, **KW, layer_scale_init=INIT)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    sd.update(LS.random_gammas(sd, D))
    g = torch.Generator().manual_seed(8)
    x, y = torch.rand(4, 3, 32, 32, generator=g), torch.randint(0, 5, (4,), generator=g)
    got = []
    for swap in (None, 1):
        leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        O.cross_entropy_mean(LS.vit_forward(leaves, x, 16, 1, D, F, swap=swap), y).backward()
        got.append(leaves)
    worst = max(rel_l2(got[1][k].grad, got[0][k].grad) for k in got[0])
    assert worst > 2e-2, worst
