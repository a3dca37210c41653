"""The fused transform-list kernel (include/vitssl_transforms.h) and `data.GPUTransform` on the GPU: float32 output equal,
element for element (torch.equal), to the Pillow-pinned oracle (oracle/augment_oracle.py: resized_crop_u8 + to_tensor) and
to Pillow's own output in tests/golden/transforms.npz; the trainers fed uint8 batches."""
import numpy as np
import pytest
import torch

from oracle import augment_oracle as A
from test_gpu_transforms_bounds import boxes_for, oracle_batch
from test_transforms_host import CROP_224, FIXTURE_CASES, fixture_cases, to_tensor_torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from vitssl_hip import ops as o
    return o


def _run(ops, imgs, ip, SH, SW):
    out = torch.full((imgs.shape[0], 3, SH, SW), float("nan"), device=DEV)
    ops.tf_resized_crop_to_tensor(torch.from_numpy(imgs).to(DEV), torch.from_numpy(np.ascontiguousarray(ip, np.int32)).to(DEV), out)
    return out.cpu()


# source H, W -> output SH, SW, box kind.  The four fixture shapes; the shapes the issue names (CIFAR 32 and STL10 96 to 224,
# 512 to 96, an output of 512); one-row and one-column boxes ("rows") and whole-image boxes ("full") at several ratios;
# the smallest tile count (one tile an image: SH <= rows per tile) and the largest (one output row per tile at SH = 512, the
# largest output the kernel is specified for: 6912 source rows are the fewest for which two output rows no longer fit LDS).
GRID = [
    (120, 160, 64, 48, "rows"), (32, 32, 224, 224, "random"), (600, 500, 384, 384, "random"), (96, 96, 192, 192, "full"),
    (32, 32, 224, 224, "full"), (96, 96, 224, 224, "random"), (96, 96, 224, 224, "rows"), (512, 512, 96, 96, "random"),
    (512, 512, 96, 96, "full"), (600, 600, 512, 512, "random"), (256, 256, 224, 224, "random"), (224, 224, 224, 224, "full"),
    (100, 75, 384, 512, "rows"), (333, 217, 50, 70, "random"), (64, 48, 33, 21, "rows"), (40, 30, 7, 5, "full"),
    (50, 60, 16, 64, "random"),                        # smallest tile count: 1
    (6912, 8, 512, 512, "full"),                       # largest tile count: 512
]


@pytest.mark.parametrize("H,W,SH,SW,kind", GRID, ids=lambda v: str(v))
def test_equals_oracle(ops, H, W, SH, SW, kind):
    B = 1 if H * W > 50000 or kind == "full" else 3
    rng = np.random.default_rng(H * 7 + W * 3 + SH + SW)
    imgs = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    ip = boxes_for(rng, B, H, W, kind)
    tiles = -(-SH // ops.tf_tile_rows(H, W, SH, SW))
    if (H, W, SH, SW) == (50, 60, 16, 64):
        assert tiles == 1
    if (H, W, SH, SW) == (6912, 8, 512, 512):
        assert tiles == 512
    got = _run(ops, imgs, ip, SH, SW)
    want = torch.from_numpy(oracle_batch(imgs, ip, SH, SW))
    assert got.shape == want.shape and not torch.isnan(got).any()
    assert torch.equal(got, want), (ip.tolist(), int((got != want).sum()), float((got - want).abs().max()))
    # the same boxes with the flip bit inverted: the mirrored image
    ip2 = ip.copy()
    ip2[:, 4] ^= 1
    assert torch.equal(_run(ops, imgs, ip2, SH, SW), want.flip(3))


@pytest.mark.parametrize("name", FIXTURE_CASES)
def test_equals_pillow_fixture(ops, name):
    img, box, (SH, SW), pillow_u8 = fixture_cases()[name]
    got = _run(ops, img[None], np.array([box]), SH, SW)[0]
    assert torch.equal(got, to_tensor_torch(pillow_u8))
    assert torch.equal(got, torch.from_numpy(A.to_tensor(A.resized_crop_u8(img, *box[:4], SH, SW, bool(box[4])))))


def test_every_image_of_a_batch_has_its_own_box(ops):
    """one source image repeated with different boxes: the per-image parameters are read per image"""
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (1, 90, 110, 3), dtype=np.uint8)
    imgs = np.repeat(img, 6, 0)
    ip = boxes_for(rng, 6, 90, 110, "rows")
    got = _run(ops, imgs, ip, 48, 64)
    assert torch.equal(got, torch.from_numpy(oracle_batch(imgs, ip, 48, 64)))
    assert len({got[b].numpy().tobytes() for b in range(6)}) == 6


# ---------------------------------------------------------------------------------------------- GPUTransform
def test_gpu_transform_seeded_against_oracle():
    from data import GPUTransform, TransformSpec, sample_transform_params
    rng = np.random.default_rng(5)
    imgs = rng.integers(0, 256, (7, 96, 120, 3), dtype=np.uint8)
    d_imgs = torch.from_numpy(imgs).to(DEV)
    for spec in (TransformSpec.from_config(CROP_224), TransformSpec(kind="crop", size=(64, 80), scale=(0.2, 0.9), flip_p=0.5),
                 TransformSpec.from_config([{"name": "Resize", "params": {"size": [192, 160]}}, {"name": "ToTensor"}]),
                 TransformSpec.from_config([{"name": "Resize", "params": {"size": 48}}, {"name": "ToTensor"}])):
        tf = GPUTransform(spec)
        SH, SW = spec.output_size(96, 120)
        first = None
        for rep in range(2):                                                 # the second call reuses the buffers
            got = tf(d_imgs, torch.Generator().manual_seed(17))
            assert got.dtype == torch.float32 and tuple(got.shape) == (7, 3, SH, SW)
            prm = sample_transform_params(spec, 96, 120, 7, torch.Generator().manual_seed(17))
            ip = np.stack([np.asarray(prm[k]).astype(np.int32) for k in ("top", "left", "h", "w", "flip")], 1)
            assert torch.equal(got.cpu(), torch.from_numpy(oracle_batch(imgs, ip, SH, SW)))
            if first is None:
                first = got
            else:
                assert got.data_ptr() == first.data_ptr()                    # the output buffer is reused
        other = tf(d_imgs, torch.Generator().manual_seed(18)).cpu()
        if spec.kind == "crop":
            assert not torch.equal(other, torch.from_numpy(oracle_batch(imgs, ip, SH, SW)))     # another seed, other boxes
        assert torch.equal(tf.render(d_imgs, prm).cpu(), torch.from_numpy(oracle_batch(imgs, ip, SH, SW)))


def test_gpu_transform_refuses_cpu_tensors():
    from data import GPUTransform, TransformSpec
    from vitssl_hip import VitsslError
    tf = GPUTransform(TransformSpec.from_config(CROP_224))
    with pytest.raises(VitsslError, match="no CPU fallback"):
        tf(torch.zeros(2, 96, 96, 3, dtype=torch.uint8))
    with pytest.raises(VitsslError, match="no CPU fallback"):
        tf.render(torch.zeros(2, 96, 96, 3, dtype=torch.uint8), [])
    with pytest.raises(VitsslError, match="uint8"):
        tf(torch.zeros(2, 96, 96, 3, device=DEV))


def test_gpu_transform_refuses_wrong_rank_and_strided_batches():
    """Both entries name the expected layout before anything is unpacked or copied: a strided batch is never made
    contiguous behind the caller's back (that would be an allocation per batch)."""
    from data import GPUTransform, TransformSpec
    from vitssl_hip import VitsslError
    tf = GPUTransform(TransformSpec.from_config(CROP_224))
    flat = torch.zeros(96, 96, 3, dtype=torch.uint8, device=DEV)
    chw = torch.zeros(2, 3, 96, 96, dtype=torch.uint8, device=DEV)
    for call in (lambda x: tf(x), lambda x: tf.render(x, [])):
        with pytest.raises(VitsslError, match=r"expected uint8 \[B,H,W,3\]"):
            call(flat)
        with pytest.raises(VitsslError, match=r"expected uint8 \[B,H,W,3\]"):
            call(chw)
        with pytest.raises(VitsslError, match="not contiguous"):
            call(chw.permute(0, 2, 3, 1))
    assert tf._out is None                                                   # nothing was allocated for a refused batch


# ---------------------------------------------------------------------------------------------- trainers
def _train_cfg(mode):
    crop = [{"name": "RandomResizedCrop", "params": {"size": 32, "scale": [0.9, 1.0]}}, {"name": "RandomHorizontalFlip", "params": {}},
            {"name": "ToTensor"}]
    resize = [{"name": "Resize", "params": {"size": [32, 32]}}, {"name": "ToTensor"}]
    crit = {"name": "L1Loss", "params": {"reduction": "mean"}} if mode == "simmim" else {"name": "CrossEntropyLoss", "params": {}}
    return {"training": {"type": mode, "num_epochs": 1, "warmup_epochs": 1, "warmup_initial_learning_rate": 1e-6,
                         "warmup_final_learning_rate": 1e-3, "criterion": crit,
                         "optimizer": {"name": "AdamW", "params": {"lr": 1e-3, "weight_decay": 1e-3}},
                         "lr_scheduler": {"main": {"name": "CosineAnnealingLR", "params": {"eta_min": 1e-6}}, "warmup": {"params": {}}}},
            "eval": {}, "data": {"img_size": 32}, "transforms": {"train": crop, "val": resize},
            "model": {"in_channels": 3, "patch_size": 8, "embed_dim": 128, "num_blocks": 2, "num_heads": 2, "mlp_dim": 192,
                      "dropout": 0.0, "mask_ratio": 0.6, "num_classes": 10, "output_dim": 256, "center_momentum": 0.9}}


def _prerender(cfg, split, batches, seed):
    """the float32 batches the trainer's own GPUTransform makes of `batches` with generator seed `seed`"""
    from data import GPUTransform, TransformSpec
    tf = GPUTransform(TransformSpec.from_config(cfg["transforms"][split]))
    gen = torch.Generator().manual_seed(seed)
    return [tf(b.to(DEV), gen).clone() for b in batches]


@pytest.mark.parametrize("mode", ["simmim", "simmim-with-labels", "supervised"])
def test_trainers_render_uint8_batches(tmp_path, mode):
    """One tiny epoch (train + validate) from uint8 [B,H,W,3] batches gives a finite loss, the SAME loss as the run fed the
    float32 batches rendered beforehand with the same crop / flip seed (same initial weights, same mask / dropout seeds)."""
    from utils.model_builder import build_model
    from utils.trainers import SimMIMTrainer, SupervisedTrainer
    kind = mode.split("-")[0]
    cfg = _train_cfg(kind)
    Trainer = SimMIMTrainer if kind == "simmim" else SupervisedTrainer
    g = torch.Generator().manual_seed(3)
    raw = [torch.randint(0, 256, (8, 40, 48, 3), dtype=torch.uint8, generator=g) for _ in range(3)]
    labels = [torch.randint(0, 10, (8,), generator=g) for _ in range(3)]
    with_labels = mode != "simmim"
    pack = lambda xs: [(x, y) for x, y in zip(xs, labels)] if with_labels else list(xs)     # noqa: E731

    def run(train, val, tag):
        torch.manual_seed(21)                                                # same initial weights
        model = build_model(cfg).to(DEV)
        tr = Trainer(model, str(tmp_path / tag), cfg, pack(train), pack(val)[:2], DEV)
        tr.transform_generator = torch.Generator().manual_seed(99)
        torch.manual_seed(22)                                                # same masks
        t = tr.train_epoch(1)
        torch.manual_seed(23)
        v = tr.validate()
        return t, v, tr

    t8, v8, tr8 = run(raw, raw, "u8")
    assert set(tr8._gpu_transforms) == {"train", "val"}
    assert tr8._gpu_transforms["train"].spec.kind == "crop" and tr8._gpu_transforms["val"].spec.kind == "resize"
    tf, vf, trf = run(_prerender(cfg, "train", raw, 99), _prerender(cfg, "val", raw[:2], 0), "f32")
    assert not trf._gpu_transforms                                           # float batches go through untouched
    for m in (t8, v8):
        assert np.isfinite(m["Loss"])
    assert t8 == tf and v8 == vf, (t8, tf, v8, vf)
    if kind == "supervised":
        assert 0.0 <= t8["Accuracy"] <= 1.0
        with pytest.raises(ValueError, match="labels"):
            SupervisedTrainer(build_model(cfg).to(DEV), str(tmp_path / "nolabels"), cfg, raw, raw[:1], DEV).train_epoch(1)
    bare = dict(cfg, transforms={"train": cfg["transforms"]["train"]})      # uint8 validation batches, no list for them
    with pytest.raises(ValueError, match=r"no `transforms\.val` list"):
        Trainer(build_model(cfg).to(DEV), str(tmp_path / "nolist"), bare, pack(raw), pack(raw)[:1], DEV).validate()
