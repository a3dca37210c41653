"""Stochastic depth (drop path) without a GPU: the rate schedule, the argument checks, the config key, the C ABI's symbol list, the
site rule, and the NumPy restatement of the table (tests/_droppath_ref.py) that the GPU tests compare the kernel with."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import _droppath_ref as DP
from test_dropout_stream import keep_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    import vitssl_hip
    return vitssl_hip


# ------------------------------------------------------------------------------------------------ schedule and arguments
@pytest.mark.parametrize("layers", [1, 2, 12])
@pytest.mark.parametrize("rate", [0.0, 0.1, 0.4])
def test_rate_schedule_is_linspace(built, layers, rate):
    from vitssl_hip.engine import drop_path_rates
    got = drop_path_rates(rate, layers)
    want = np.linspace(0.0, rate, layers)
    assert len(got) == layers and got[0] == 0.0
    np.testing.assert_allclose(got, want, rtol=1e-14, atol=0)
    if layers > 1:
        assert got[-1] == rate
    # the same effective rates (the kernels round a rate to 1 / 65536)
    assert [DP.r_eff(a) for a in got] == [DP.r_eff(float(b)) for b in want]


def _makers():
    from vit_core import EncoderBlock, ViT
    from vit_core.ssl.dino.model import DINOViT, ViTBackbone
    from vit_core.ssl.simmim import SimMIMViT
    kw = dict(num_blocks=2, input_shape=(3, 32, 32), embed_dim=64, patch_size=16, num_heads=1, mlp_dim=64, dropout=0.0)
    return {
        "ViT": lambda r: ViT(num_classes=5, drop_path_rate=r, **kw),
        "SimMIMViT": lambda r: SimMIMViT(drop_path_rate=r, **kw),
        "DINOViT": lambda r: DINOViT(output_dim=64, drop_path_rate=r, **kw),
        "ViTBackbone": lambda r: ViTBackbone(drop_path_rate=r, **kw),
        "EncoderBlock": lambda r: EncoderBlock(64, 1, 64, 0.0, drop_path=r),
    }


@pytest.mark.parametrize("who", ["ViT", "SimMIMViT", "DINOViT", "ViTBackbone", "EncoderBlock"])
def test_rates_outside_the_unit_interval_are_value_errors(built, who):
    make = _makers()[who]
    for bad in (-0.1, 1.0):
        with pytest.raises(ValueError):
            make(bad)
    m, m0 = make(0.3), make(0.0)
    assert getattr(m, "drop_path_rate", getattr(m, "drop_path", None)) == 0.3
    # not parameters, not buffers: the state_dict is what it is without the key
    assert list(m.state_dict()) == list(m0.state_dict())
    assert [n for n, _ in m.named_parameters()] == [n for n, _ in m0.named_parameters()]


def test_positional_signatures_are_untouched(built):
    import inspect
    from vit_core import EncoderBlock, ViT
    from vit_core.ssl.dino.model import DINOViT, ViTBackbone
    from vit_core.ssl.simmim import SimMIMViT
    for cls, last in ((ViT, "drop_path_rate"), (SimMIMViT, "drop_path_rate"), (DINOViT, "drop_path_rate"), (ViTBackbone, "drop_path_rate"),
                      (EncoderBlock, "drop_path")):
        params = list(inspect.signature(cls.__init__).parameters.values())
        assert params[-1].name == last and params[-1].default == 0.0, cls


def _cfg(mode, **model_extra):
    model = {"in_channels": 3, "patch_size": 16, "embed_dim": 64, "num_blocks": 3, "num_heads": 1, "mlp_dim": 64, "dropout": 0.0,
             "mask_ratio": 0.6, "num_classes": 5, "output_dim": 64, "center_momentum": 0.9}
    model.update(model_extra)
    return {"training": {"type": mode}, "eval": {}, "data": {"img_size": 32}, "model": model}


@pytest.mark.parametrize("mode", ["supervised", "simmim", "dino"])
def test_build_model_reads_the_optional_key(built, mode):
    from utils.model_builder import build_model
    assert build_model(_cfg(mode)).drop_path_rate == 0.0
    assert build_model(_cfg(mode, drop_path_rate=0.0)).drop_path_rate == 0.0
    assert build_model(_cfg(mode, drop_path_rate=0.2)).drop_path_rate == 0.2
    with pytest.raises(ValueError):
        build_model(_cfg(mode, drop_path_rate=1.5))


def test_stack_without_rates_has_none_and_draws_no_seed(built):
    """EncoderStack on a CPU store (nothing is launched by building one): no rates -> no drop path, and the seed is drawn exactly when
    element dropout asks for it, as before; with rates a training forward draws one whatever the dropout."""
    from vit_core import ViT
    from vitssl_hip import _lib as L
    from vitssl_hip import engine as E
    cpu = torch.device("cpu")

    def stack(p, rates):
        m = ViT(5, 3, (3, 32, 32), 64, 16, 1, 64, p)
        return E.EncoderStack(E.FlatStore(m, cpu), [f"encoder_blocks.{i}." for i in range(3)], 64, 1, 64, p, drop_path=rates)

    for rates in (None, [0.0, 0.0, 0.0]):
        s = stack(0.0, rates)
        assert s.drop_path is None and not s.needs_seed(True) and not s.needs_seed(False) and s.drop_path_sites() == []
        assert stack(0.1, rates).needs_seed(True) and not stack(0.1, rates).needs_seed(False)
    s = stack(0.0, E.drop_path_rates(0.5, 3))
    assert s.drop_path == [0.0, 0.25, 0.5] and s.needs_seed(True) and not s.needs_seed(False)
    sites = s.drop_path_sites()
    assert [r for r, _ in sites] == [0.0, 0.0, 0.25, 0.25, 0.5, 0.5]
    assert [v for _, v in sites] == [DP.site(i, br) for i in range(3) for br in (0, 1)]
    with pytest.raises(ValueError):
        stack(0.0, [0.1, 0.2])                                              # one rate per block
    with pytest.raises(ValueError):
        stack(0.0, [0.0, 0.5, 1.0])
    # fp8 operands: refused at construction, and the message names the way out
    E.set_linear_operands("fp8")
    try:
        m = ViT(5, 2, (3, 32, 32), 128, 16, 2, 128, 0.0)
        args = (E.FlatStore(m, cpu), ["encoder_blocks.0.", "encoder_blocks.1."], 128, 2, 128, 0.0)
        with pytest.raises(L.VitsslError, match="bf16"):
            E.EncoderStack(*args, drop_path=[0.0, 0.1])
        assert E.EncoderStack(*args, drop_path=[0.0, 0.0]).drop_path is None      # rate 0: fp8 stacks build as before
    finally:
        E.set_linear_operands("bf16")


def test_sites_are_disjoint_from_every_dropout_site(built):
    """dropout: site_base + 3 i + which (small numbers); drop path: the high bit | (site_base + 2 i + branch)"""
    from vitssl_hip import _lib as L
    assert L.DROPPATH_SITE_BIT == DP.SITE_BIT == 0x80000000
    for base in (0, 1000):
        drop = {base + 3 * i + w for i in range(64) for w in range(3)}
        path = {DP.site(i, br, base) for i in range(64) for br in (0, 1)}
        assert len(path) == 128 and not (drop & path) and all(s >> 31 == 1 for s in path) and all(s >> 31 == 0 for s in drop)
    txt = open(L.HEADERS["droppath"]).read()
    assert "VITSSL_DROPPATH_SITE_BIT 0x80000000u" in txt and "site_base + 3 * block + which" in txt      # the rule is documented


# ------------------------------------------------------------------------------------------------ C ABI
def test_header_declares_the_four_entry_points_and_the_library_exports_them(built):
    from vitssl_hip import _lib as L
    want = {"vitssl_droppath_table", "vitssl_gemm_bf16_nt_rows", "vitssl_layernorm_bwd_rows", "vitssl_grad_mask_cast_rows"}
    assert set(L.header_symbols("droppath")) == want == set(L.REGISTRY["droppath"])
    raw = ctypes.CDLL(built.LIB_PATH)
    for s in want:
        assert hasattr(raw, s), f"{s} declared in include/vitssl_droppath.h but not exported"
    # vitssl_hip.h keeps its symbol list, its structs and its version
    assert not want & set(L.header_symbols()) and not want & set(L.REGISTRY["hip"])
    assert built.lib().vitssl_version() == L.ABI_VERSION == 3
    txt = re.sub(r"/\*.*?\*/", "", open(L.HEADERS["droppath"]).read(), flags=re.S)
    assert re.search(r"const float\* scale;\s*int64_t groups;\s*int rows_per_group;", txt)
    assert ctypes.sizeof(L.RowScale) == 24


def test_argument_errors_are_reported_before_any_launch(built):
    from vitssl_hip import _lib as L
    lib = built.lib()
    g = L.Gemm()
    r = L.RowScale()
    assert lib.vitssl_gemm_bf16_nt_rows(ctypes.byref(g), None, None) == -1 and b"null row scales" in lib.vitssl_last_error()
    assert lib.vitssl_gemm_bf16_nt_rows(ctypes.byref(g), ctypes.byref(r), None) == -1 and b"null operand" in lib.vitssl_last_error()
    rates, sites = (ctypes.c_float * 1)(0.5), (ctypes.c_uint32 * 1)(7)
    assert lib.vitssl_droppath_table(None, rates, sites, 1, 4, 1, None) == -1 and b"null pointer" in lib.vitssl_last_error()
    fake = ctypes.c_void_p(256)                                              # never dereferenced: every call below is refused first
    assert lib.vitssl_droppath_table(fake, rates, sites, 0, 4, 1, None) == -1 and b"sites" in lib.vitssl_last_error()
    assert lib.vitssl_droppath_table(fake, rates, sites, L.DROPPATH_MAX_SITES + 1, 4, 1, None) == -1
    assert lib.vitssl_droppath_table(fake, rates, sites, 1, 0, 1, None) == -1 and b"B = 0" in lib.vitssl_last_error()
    for bad in (1.0, float("nan")):
        rates[0] = bad
        assert lib.vitssl_droppath_table(fake, rates, sites, 1, 4, 1, None) == -1 and b"must be < 1" in lib.vitssl_last_error()
    drop = L.Dropout(0.0, 0, 0)
    r.scale, r.groups, r.rows_per_group = 256, 3, 5                          # 15 rows
    assert lib.vitssl_grad_mask_cast_rows(fake, fake, None, drop, ctypes.byref(r), 16, 64, None, 0, None) == -1
    assert b"must equal rows" in lib.vitssl_last_error()
    assert lib.vitssl_grad_mask_cast_rows(fake, fake, None, drop, None, 15, 64, None, 0, None) == -1
    assert lib.vitssl_layernorm_bwd_rows(fake, fake, fake, fake, fake, None, fake, fake, fake, fake, None, drop, ctypes.byref(r), 16, 64,
                                         None, 0, None) == -1 and b"must equal rows" in lib.vitssl_last_error()
    assert lib.vitssl_layernorm_bwd_rows(fake, fake, fake, fake, fake, None, fake, None, fake, fake, None, drop, ctypes.byref(r), 15, 64,
                                         None, 0, None) == -1 and b"null pointer" in lib.vitssl_last_error()      # gm_bf16 is required


# ------------------------------------------------------------------------------------------------ the table, restated
@pytest.mark.parametrize("B", [1, 5, 64, 4096])
@pytest.mark.parametrize("rate", [0.0, 0.1, 0.5])
def test_table_restatement(B, rate):
    seed, site = 12345, DP.site(2, 1)
    s = DP.path_scales(B, rate, seed, site)
    assert s.dtype == np.float32 and s.shape == (B,)
    if rate == 0.0:
        assert (s == 1.0).all()
        return
    thr = int(rate * 65536 + 0.5)
    scale = np.float32(65536.0) / np.float32(65536 - thr)
    assert set(np.unique(s)) <= {np.float32(0), scale}
    assert abs(float(scale) * (1 - DP.r_eff(rate)) - 1.0) < 1e-6             # the reciprocal of 1 - r_eff, rounded once to fp32
    # keep[b] is the stream's keep bit of element b of a [1, B] tensor (B rounded up to the stream's 4-element groups)
    keep = keep_mask(1, (B + 3) // 4 * 4, rate, seed, site)[0, :B]
    assert np.array_equal(s != 0, keep != 0)
    if B == 4096:
        sd = (rate * (1 - rate) / B) ** 0.5
        assert abs(float((s != 0).mean()) - (1 - DP.r_eff(rate))) < 4 * sd
    # another site, another seed: other draws
    if B >= 64:
        assert not np.array_equal(s, DP.path_scales(B, rate, seed, DP.site(2, 0)))
        assert not np.array_equal(s, DP.path_scales(B, rate, seed + 1, site))


def test_table_layout_and_seed_choice():
    block_rates = DP.rates(0.5, 3)
    assert block_rates == [0.0, 0.25, 0.5]
    seed = DP.pick_seed(block_rates, 5)
    tab = DP.table(block_rates, 5, seed)
    assert tab.shape == (6, 5) and (tab[:2] == 1).all() and DP.mixed(tab, block_rates)
    assert np.array_equal(tab[3], DP.path_scales(5, 0.25, seed, DP.site(1, 1)))
    keeps = DP.oracle_keeps(tab, 4, 8, 16)
    assert len(keeps) == 3 and keeps[2][0].shape == (5, 4, 8) and keeps[2][1].shape == (5, 4, 16)
    assert torch.equal(keeps[2][2][:, 0, 0], torch.from_numpy(tab[5])) and bool((keeps[0][0] == 1).all())
