"""No GPU needed: the Pillow fixture of the crop / flip / ToTensor and Resize / ToTensor transform lists against the oracle,
`TransformSpec.from_config`, the crop / flip sampling, and the completeness of everything that hangs on
include/vitssl_transforms.h (bindings, exported symbols, the guarded-buffer case table)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

from _util import load_golden
from oracle import augment_oracle as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vitssl_transforms.h")

# the reference's transform lists, literally (configs/<dir>/<file>.yaml with data.img_size resolved)
CROP_224 = [{"name": "RandomResizedCrop", "params": {"size": 224, "scale": [0.9, 1.0]}}, {"name": "RandomHorizontalFlip", "params": {}},
            {"name": "ToTensor"}]
RESIZE_224 = [{"name": "Resize", "params": {"size": [224, 224]}}, {"name": "ToTensor"}]
RESIZE_192 = [{"name": "Resize", "params": {"size": [192, 192]}}, {"name": "ToTensor"}]
REFERENCE_LISTS = {
    "simmim/train_transforms": CROP_224, "supervised/train_transforms": CROP_224, "finetune/train_transforms": CROP_224,
    "simmim/val_transforms": RESIZE_224, "supervised/val_transforms": RESIZE_224, "finetune/val_transforms": RESIZE_224,
    "unsupervised_eval/transforms": RESIZE_192, "supervised_eval/transforms": RESIZE_192,
}
FIXTURE_CASES = ("rect_crop_flip", "up_32_to_224", "down_600x500_to_384", "resize_96_to_192")


def fixture_cases():
    """name -> (img u8 [H,W,3], (top, left, h, w, flip), (SH, SW), Pillow's uint8 output [SH,SW,3])"""
    g = load_golden("transforms")
    assert tuple(g["names"]) == FIXTURE_CASES
    out = {}
    for name in FIXTURE_CASES:
        p = [int(v) for v in g[f"{name}_params"]]
        out[name] = (g[f"{name}_img"], tuple(p[:5]), (p[5], p[6]), g[f"{name}_out"])
    return out


def to_tensor_torch(u8):
    """torchvision F.to_tensor of a uint8 RGB image: channel-first, float32, div(255)"""
    return torch.from_numpy(np.ascontiguousarray(u8)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)


# ---------------------------------------------------------------------------------------------- fixture from Pillow
@pytest.mark.parametrize("name", FIXTURE_CASES)
def test_oracle_reproduces_pillow(name):
    img, (top, left, h, w, flip), (SH, SW), want = fixture_cases()[name]
    assert want.shape == (SH, SW, 3) and want.dtype == np.uint8
    got = A.resized_crop_u8(img, top, left, h, w, SH, SW, bool(flip))
    assert np.array_equal(got, want)
    assert torch.equal(torch.from_numpy(A.to_tensor(got)), to_tensor_torch(want))


def test_fixture_covers_what_it_should():
    c = fixture_cases()
    img, (top, left, h, w, flip), (SH, SW), _ = c["rect_crop_flip"]
    assert flip == 1 and h != w and SH != SW and img.shape[0] != img.shape[1]
    assert c["up_32_to_224"][0].shape == (32, 32, 3) and c["up_32_to_224"][2] == (224, 224)
    assert c["down_600x500_to_384"][0].shape == (600, 500, 3) and c["down_600x500_to_384"][2] == (384, 384)
    img, box, size, _ = c["resize_96_to_192"]
    assert img.shape == (96, 96, 3) and box == (0, 0, 96, 96, 0) and size == (192, 192)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "transforms.npz")) < 1 << 20


# ---------------------------------------------------------------------------------------------- TransformSpec.from_config
@pytest.mark.parametrize("key", sorted(REFERENCE_LISTS))
def test_from_config_accepts_the_reference_lists(key):
    from data import TransformSpec
    spec = TransformSpec.from_config(REFERENCE_LISTS[key])
    if "train" in key:
        assert spec.kind == "crop" and spec.size == (224, 224) and spec.scale == (0.9, 1.0) and spec.flip_p == 0.5
        assert spec.ratio == (3.0 / 4.0, 4.0 / 3.0)
    else:
        side = 192 if "eval" in key else 224
        assert spec.kind == "resize" and spec.size == (side, side) and spec.output_size(96, 96) == (side, side)


def test_from_config_sizes_params_and_refusals():
    from data import TransformSpec
    crop = lambda **p: [{"name": "RandomResizedCrop", "params": p}, {"name": "RandomHorizontalFlip", "params": {"p": 0.25}},  # noqa: E731
                        {"name": "ToTensor", "params": {}}]
    s = TransformSpec.from_config(crop(size=[384, 512], scale=[0.2, 0.7], ratio=[0.5, 2.0]))
    assert s.size == (384, 512) and s.scale == (0.2, 0.7) and s.ratio == (0.5, 2.0) and s.flip_p == 0.25
    assert TransformSpec.from_config(crop(size=96)).size == (96, 96)
    assert TransformSpec.from_config(crop(size=96)).scale == (0.08, 1.0)                   # torchvision's default
    r = TransformSpec.from_config([{"name": "Resize", "params": {"size": 64}}, {"name": "ToTensor"}])
    assert r.output_size(96, 192) == (64, 128) and r.output_size(192, 96) == (128, 64)     # Resize(int): the shorter side
    jitter = CROP_224[:2] + [{"name": "ColorJitter", "params": {"brightness": 0.4}}, {"name": "ToTensor"}]
    with pytest.raises(ValueError, match="ColorJitter"):
        TransformSpec.from_config(jitter)
    with pytest.raises(ValueError, match="Normalize"):
        TransformSpec.from_config(RESIZE_224 + [{"name": "Normalize", "params": {"mean": [0.5], "std": [0.5]}}])
    for bad in ([{"name": "ToTensor"}], CROP_224[:1] + CROP_224[2:], [CROP_224[1], CROP_224[0], CROP_224[2]], RESIZE_224[::-1]):
        with pytest.raises(ValueError, match="neither"):
            TransformSpec.from_config(bad)


def test_get_transforms_carries_the_transform_spec(monkeypatch):
    from utils.train_utils import get_transforms
    monkeypatch.setitem(sys.modules, "torchvision", None)                                  # import torchvision -> ImportError
    dino = CROP_224[:2] + [{"name": "ColorJitter", "params": {"brightness": 0.4}},
                           {"name": "GaussianBlur", "params": {"kernel_size": 7}}, {"name": "ToTensor"}]
    tf = get_transforms({"transforms": {"train": CROP_224, "val": RESIZE_192, "globals": dino}})
    assert tf["train"].transform_spec.kind == "crop" and tf["train"].transform_spec.size == (224, 224)
    assert tf["val"].transform_spec.kind == "resize" and tf["val"].transform_spec.size == (192, 192)
    assert tf["globals"].transform_spec is None and tf["globals"].view_spec is not None
    from vitssl_hip import VitsslError
    with pytest.raises(VitsslError, match="GPUTransform"):
        tf["val"](object())


# ---------------------------------------------------------------------------------------------- sampling
@pytest.mark.parametrize("H,W,scale,p", [(96, 96, (0.9, 1.0), 0.5), (120, 200, (0.3, 0.8), 0.2), (600, 500, (0.08, 1.0), 0.7)])
def test_sampled_boxes_areas_and_flip_rate(H, W, scale, p):
    from data import TransformSpec, sample_transform_params
    spec = TransformSpec(kind="crop", size=(64, 64), scale=scale, flip_p=p)
    n = 4000
    d = sample_transform_params(spec, H, W, n, torch.Generator().manual_seed(H + W))
    top, left, h, w, flip = (np.asarray(d[k]) for k in ("top", "left", "h", "w", "flip"))
    assert all(len(v) == n for v in (top, left, h, w, flip))
    assert (top >= 0).all() and (left >= 0).all() and (h >= 1).all() and (w >= 1).all()
    assert (top + h <= H).all() and (left + w <= W).all()
    # area = round(sqrt(a r)) * round(sqrt(a / r)): each factor is off its real value by <= 1/2, so the product is off a by
    # at most (h + w) / 2 + 1/4 pixels
    area, slack = h * w, (h + w) / 2 + 0.25
    assert (area >= scale[0] * H * W - slack).all() and (area <= scale[1] * H * W + slack).all()
    # binomial(n, p): 5 standard deviations
    assert abs(flip.mean() - p) < 5 * np.sqrt(p * (1 - p) / n)
    ratio = w / h
    assert (ratio > 3 / 4 * 0.9).all() and (ratio < 4 / 3 * 1.1).all()


def test_resize_draws_nothing():
    from data import TransformSpec, sample_transform_params
    gen = torch.Generator().manual_seed(3)
    before = gen.get_state()
    d = sample_transform_params(TransformSpec(kind="resize", size=(192, 192)), 96, 80, 5, gen)
    assert torch.equal(gen.get_state(), before)
    assert list(d["top"]) == [0] * 5 and list(d["h"]) == [96] * 5 and list(d["w"]) == [80] * 5 and not d["flip"].any()


def test_draws_equal_those_of_a_dino_view():
    """The crop and flip draws come first in a DINO view (colour and blur draws follow): with one seed the transform
    sampler and the view sampler give the same boxes and flips -- the scalar samplers image after image as long as the
    generator is re-seeded per image (the view consumes more draws), the batch samplers for a batch of one image (their
    uniform blocks are [n, 23] and [n, 32])."""
    from data import TransformSpec, ViewSpec, sample_batch_params, sample_transform_params, sample_view_params
    from data.transforms import sample_transform_params_scalar
    ts = TransformSpec(kind="crop", size=(224, 224), scale=(0.4, 1.0), flip_p=0.5)
    vs = ViewSpec(size=224, scale=(0.4, 1.0), gray_p=0.2)
    keys = ("top", "left", "h", "w", "flip")
    flips = 0
    for seed in range(40):
        a = sample_transform_params_scalar(ts, 96, 120, torch.Generator().manual_seed(seed))
        b = sample_view_params(vs, 96, 120, torch.Generator().manual_seed(seed))
        assert set(a) == set(keys) and [a[k] for k in keys] == [b[k] for k in keys], seed
        c = sample_transform_params(ts, 96, 120, 1, torch.Generator().manual_seed(seed))
        d = sample_batch_params(vs, 96, 120, 1, torch.Generator().manual_seed(seed))
        assert [int(c[k][0]) for k in keys] == [int(d[k][0]) for k in keys], seed
        flips += int(a["flip"])
    assert 5 < flips < 35


def test_pack_layout():
    from data.transforms import pack_transform_params
    arr = dict(top=np.array([1, 2]), left=np.array([3, 4]), h=np.array([5, 6]), w=np.array([7, 8]), flip=np.array([True, False]))
    want = np.array([[1, 3, 5, 7, 1], [2, 4, 6, 8, 0]], np.int32)
    got = pack_transform_params(arr)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert np.array_equal(pack_transform_params([dict(top=1, left=3, h=5, w=7, flip=True), dict(top=2, left=4, h=6, w=8, flip=False)]), want)


def test_uint8_batch_without_a_transform_list_is_named():
    """The trainers' `_batch` names the missing `transforms.<split>` list (checked before anything touches a GPU)."""
    from types import SimpleNamespace
    from utils.trainers.base_trainer import BaseTrainer
    u8 = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    for cfg in ({}, {"transforms": None}, {"transforms": {"train": []}}):
        me = SimpleNamespace(device="cpu", config=cfg, _gpu_transforms={}, transform_generator=None)
        with pytest.raises(ValueError, match=r"no `transforms\.val` list"):
            BaseTrainer._batch(me, (u8, torch.zeros(2, dtype=torch.long)), "val")
    me = SimpleNamespace(device="cpu", config={}, _gpu_transforms={}, transform_generator=None)
    x = torch.zeros(2, 3, 8, 8)
    got, labels = BaseTrainer._batch(me, x, "train")                         # float batches need no list
    assert got is x and labels is None


# ---------------------------------------------------------------------------------------------- header completeness
@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    import vitssl_hip
    return vitssl_hip


def _prototypes():
    """name -> parameter text of every function of include/vitssl_transforms.h"""
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(?:int|int64_t|const char\*)\s+(vitssl_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", txt)}


def test_transforms_header_is_bound_exported_and_covered(built):
    import test_gpu_transforms_bounds as T
    from vitssl_hip import _lib
    protos = _prototypes()
    assert "vitssl_tf_resized_crop_to_tensor" in protos and set(protos) == set(_lib.header_symbols("transforms")) == set(_lib.REGISTRY["transforms"])
    launching = {n for n, args in protos.items() if re.search(r"void\s*\*\s*stream", args)}
    assert launching == {"vitssl_tf_resized_crop_to_tensor"}
    table = {n: _lib.REGISTRY["transforms"][n][1] for n in launching}
    assert launching | {"vitssl_debug_tf_tile_rows"} == set(_lib.REGISTRY["transforms"])      # the getter returns a count
    for n in launching:                                                      # one ctypes argument per C parameter
        assert len(table[n]) == len([a for a in protos[n].split(",") if a.strip()]), n
    raw = ctypes.CDLL(built.LIB_PATH)
    for n in protos:
        assert hasattr(raw, n), f"{n} declared in include/vitssl_transforms.h but not exported"
    lib = built.lib()
    for n in launching:
        assert getattr(lib, n).argtypes == table[n] and getattr(lib, n).restype is ctypes.c_int
    covered = {c.entry for c in T.CASES}
    assert not (launching - covered), f"entry points without a case in tests/test_gpu_transforms_bounds.py: {sorted(launching - covered)}"
    assert not (covered - launching), f"cases of unknown entry points: {sorted(covered - launching)}"
    assert all(c.bar for c in T.CASES) and len({c.id for c in T.CASES}) == len(T.CASES) >= 4
    # the ABI of include/vitssl_hip.h is what it was: no symbol of the new header in it, its table or its version
    assert not set(protos) & set(_lib.header_symbols()) and not set(protos) & set(_lib.REGISTRY["hip"])
    assert lib.vitssl_version() == _lib.ABI_VERSION and set(_lib.REGISTRY["hip"]) == set(_lib.header_symbols())


def test_tile_plan_and_argument_errors(built):
    """Host-side checks run before anything is launched, so they can be exercised without a GPU."""
    from vitssl_hip import _lib, ops
    lib = built.lib()
    # the shapes the kernel must serve, each with a tile that is a power of two <= 32
    for H, W, SH, SW in [(32, 32, 224, 224), (96, 96, 224, 224), (512, 512, 96, 96), (600, 600, 512, 512), (256, 256, 224, 224),
                         (600, 500, 384, 384), (96, 96, 192, 192), (120, 160, 64, 48), (512, 512, 512, 512)]:
        tr = ops.tf_tile_rows(H, W, SH, SW)
        assert tr in (1, 2, 4, 8, 16, 32), (H, W, SH, SW, tr)
    assert ops.tf_tile_rows(6912, 8, 512, 512) == 1                          # one output row per tile: 512 tiles an image
    with pytest.raises(_lib.VitsslError, match="the limit is 65536"):
        ops.tf_tile_rows(50000, 8, 512, 512)
    with pytest.raises(_lib.VitsslError, match="more than 127x"):
        ops.tf_tile_rows(96, 4096, 96, 32)
    # shapes whose LDS need passes 2^31 bytes are refused by the same limit, with the true figure in the message.  The first:
    # 8355968 * (1 + 3) * 4 of column taps + (1 + 167) * 4 of row taps + 166 rows * 25067904 bytes = 2^32 + 928 for a one-row
    # tile (2^32 + 1600 for a two-row tile: a small number once truncated to 32 bits); the second passes 2^31 with 32-row tiles only
    for shape, need in [((166, 8, 2, 8355968), "4294968224"), ((12700, 8, 100, 170000), None), ((1, 1, 1, (1 << 23) - 1), None)]:
        with pytest.raises(_lib.VitsslError, match="the limit is 65536") as e:
            ops.tf_tile_rows(*shape)
        assert need is None or f"needs {need} bytes" in str(e.value), str(e.value)
    fn = lib.vitssl_tf_resized_crop_to_tensor
    one = ctypes.c_void_p(256)                                               # never dereferenced: every call below is refused
    for args, msg in [((None, one, one, 1, 8, 8, 8, 8), b"null pointer"), ((one, None, one, 1, 8, 8, 8, 8), b"null pointer"),
                      ((one, one, None, 1, 8, 8, 8, 8), b"null pointer"), ((one, one, one, 0, 8, 8, 8, 8), b"empty batch"),
                      ((one, one, one, 1, 0, 8, 8, 8), b"bad shape"), ((one, one, one, 1, 8, 8, 8, 0), b"bad shape"),
                      ((one, one, one, 1, 50000, 8, 512, 512), b"the limit is 65536"),
                      ((one, one, one, 1, 166, 8, 2, 8355968), b"the limit is 65536"),
                      ((one, one, one, 1, 12700, 8, 100, 170000), b"the limit is 65536")]:
        assert fn(*args, None) == -1 and msg in lib.vitssl_last_error(), (args, lib.vitssl_last_error())
    with pytest.raises(_lib.VitsslError, match="CUDA"):                      # no CPU fallback in the wrapper either
        ops.tf_resized_crop_to_tensor(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, 5, dtype=torch.int32), torch.zeros(1, 3, 8, 8))
