"""SimMIM / supervised / finetune / eval transform lists rendered on the GPU (reference: utils/train_utils.py:54-68 with
configs/{simmim,supervised,finetune}/train_transforms.yaml, configs/*/val_transforms.yaml,
configs/unsupervised_eval/transforms.yaml, configs/supervised_eval/transforms.yaml).

The reference runs, per image and on the CPU, one of two torchvision lists on a PIL image:
    RandomResizedCrop(size, scale) -> RandomHorizontalFlip -> ToTensor          (train)
    Resize([h, w]) -> ToTensor                                                   (val / eval)
Here a whole batch of decoded uint8 images goes through ONE HIP launch (vitssl_tf_resized_crop_to_tensor: crop box, Pillow
BILINEAR resize, flip, /255, channel-first), bit-identical to Pillow (oracle/augment_oracle.py).  What stays on the host is
the drawing of the crop boxes and flips, by the code the DINO views use for the same two transforms
(data/multicrop.py: `crop_flip_from_uniforms` for a batch, `sample_crop_flip` for the scalar order of torchvision's
`get_params`); `Resize` draws nothing.  No CPU fallback: the batch is produced by libvitssl_hip or not at all.
"""
from dataclasses import dataclass
from typing import Optional, Tuple, Union

import numpy as np
import torch

from vitssl_hip import _lib as L
from vitssl_hip import ops

from .multicrop import CROP_FLIP_UNIFORMS, crop_flip_from_uniforms, sample_crop_flip

_CROP_LIST = ("RandomResizedCrop", "RandomHorizontalFlip", "ToTensor")
_RESIZE_LIST = ("Resize", "ToTensor")


def _pair(size, what):
    if isinstance(size, (int, np.integer)):
        return int(size), int(size)
    size = tuple(int(s) for s in size)
    if len(size) == 1:
        return size[0], size[0]
    if len(size) != 2:
        raise ValueError(f"GPUTransform: {what} size must be an int or [h, w], got {size}")
    return size


@dataclass
class TransformSpec:
    """One of the two transform lists above, reduced to its numbers."""
    kind: str                                           # "crop" (RandomResizedCrop, flip, ToTensor) | "resize" (Resize, ToTensor)
    size: Union[int, Tuple[int, int]]                   # (h, w); a bare int only for Resize(int): the SHORTER side, as torchvision
    scale: Tuple[float, float] = (0.08, 1.0)
    ratio: Tuple[float, float] = (3.0 / 4.0, 4.0 / 3.0)
    flip_p: float = 0.5

    @classmethod
    def from_config(cls, sequence) -> "TransformSpec":
        """sequence: the list of {name, params} entries of a transform YAML."""
        entries = [(str(e["name"]).strip(), dict(e.get("params") or {})) for e in sequence]
        names = tuple(n for n, _ in entries)
        for n in names:
            if n not in _CROP_LIST and n not in _RESIZE_LIST:
                raise ValueError(f"GPUTransform: transform {n!r} is not part of the crop / flip / ToTensor or Resize / ToTensor lists")
        prm = dict(entries)
        if names == _CROP_LIST:
            p = prm["RandomResizedCrop"]
            kw = dict(kind="crop", size=_pair(p["size"], "RandomResizedCrop"), scale=tuple(float(v) for v in p.get("scale", (0.08, 1.0))),
                      flip_p=float(prm["RandomHorizontalFlip"].get("p", 0.5)))
            if "ratio" in p:
                kw["ratio"] = tuple(float(v) for v in p["ratio"])
            return cls(**kw)
        if names == _RESIZE_LIST:
            size = prm["Resize"]["size"]
            return cls(kind="resize", size=int(size) if isinstance(size, (int, np.integer)) else _pair(size, "Resize"))
        raise ValueError(f"GPUTransform: the list {list(names)} is neither {list(_CROP_LIST)} nor {list(_RESIZE_LIST)}")

    def output_size(self, height: int, width: int) -> Tuple[int, int]:
        if isinstance(self.size, tuple):
            return self.size
        # torchvision Resize(int): the shorter side becomes `size`, the other keeps the aspect ratio (truncated)
        if height <= width:
            return self.size, int(self.size * width / height)
        return int(self.size * height / width), self.size


def sample_transform_params(spec: TransformSpec, height: int, width: int, n: int,
                            generator: Optional[torch.Generator] = None) -> dict:
    """Boxes and flips of `n` images as arrays (top, left, h, w, flip).  A crop list draws ONE [n, 23] block of uniforms,
    mapped to parameters as `sample_batch_params` maps the first 23 columns of its block (its colour and blur columns are
    simply not drawn); a Resize list draws nothing and returns the full-image box."""
    if spec.kind == "resize":
        full = np.ones(n, np.int64)
        return dict(top=0 * full, left=0 * full, h=height * full, w=width * full, flip=np.zeros(n, bool))
    u = torch.rand(n, CROP_FLIP_UNIFORMS, generator=generator, dtype=torch.float64).numpy()
    return crop_flip_from_uniforms(spec, height, width, u)


def sample_transform_params_scalar(spec: TransformSpec, height: int, width: int, generator: Optional[torch.Generator] = None) -> dict:
    """One image's box and flip in torchvision's own draw order (`get_params`, then the flip): the draws of a DINO view
    (`sample_view_params`) with the colour and blur draws removed."""
    if spec.kind == "resize":
        return dict(top=0, left=0, h=height, w=width, flip=False)
    return sample_crop_flip(spec, height, width, generator)


def pack_transform_params(params, out: Optional[np.ndarray] = None) -> np.ndarray:
    """array dict of `sample_transform_params`, or a list of per-image dicts -> int32 [B, 5] in the kernel's layout"""
    if not isinstance(params, dict):
        params = {k: np.asarray([p[k] for p in params]) for k in ("top", "left", "h", "w", "flip")}
    n = len(params["top"])
    ip = np.empty((n, ops.TF_IP), np.int32) if out is None else out
    for j, k in enumerate(("top", "left", "h", "w", "flip")):
        ip[:, j] = params[k]
    return ip


class GPUTransform:
    """images uint8 [B, H, W, 3] on the GPU -> float32 [B, 3, SH, SW].  The output buffer and the pinned parameter
    array are reused between calls: consume (or clone) a batch before rendering the next one."""

    def __init__(self, spec: TransformSpec):
        self.spec = spec
        self._out = None
        self._pinned = None                             # int32 [B, 5], page-locked
        self._copied = None                             # event behind the last copy out of it

    def _params_device(self, params, B, dev):
        if self._pinned is None or self._pinned.shape[0] != B:
            self._pinned = torch.empty(B, ops.TF_IP, dtype=torch.int32).pin_memory()
            self._copied = torch.cuda.Event()
        else:
            self._copied.synchronize()                  # the previous batch's asynchronous copy has read the array
        pack_transform_params(params, self._pinned.numpy())
        ip_d = self._pinned.to(dev, non_blocking=True)
        self._copied.record(torch.cuda.current_stream(dev))
        return ip_d

    @staticmethod
    def _check(images):
        if not isinstance(images, torch.Tensor) or images.device.type != "cuda":
            raise L.VitsslError("GPUTransform: images are on the CPU; move the uint8 batch to 'cuda' (no CPU fallback)")
        if images.dim() != 4 or images.shape[3] != 3 or images.dtype != torch.uint8:
            raise L.VitsslError(f"GPUTransform: expected uint8 [B,H,W,3], got {images.dtype} {tuple(images.shape)}")
        if not images.is_contiguous():
            raise L.VitsslError(f"GPUTransform: the uint8 batch {tuple(images.shape)} is not contiguous (strides {images.stride()}); "
                                "it is read in place, never copied")

    def render(self, images: torch.Tensor, params) -> torch.Tensor:
        """The batch with explicit parameters (array dict or list of per-image dicts)."""
        self._check(images)
        B, H, W, _ = images.shape
        SH, SW = self.spec.output_size(H, W)
        dev = images.device
        ip_d = self._params_device(params, B, dev)
        if self._out is None or tuple(self._out.shape) != (B, 3, SH, SW) or self._out.device != dev:
            self._out = torch.empty(B, 3, SH, SW, dtype=torch.float32, device=dev)
        ops.tf_resized_crop_to_tensor(images, ip_d, self._out)
        return self._out

    def __call__(self, images: torch.Tensor, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        self._check(images)
        B, H, W, _ = images.shape
        return self.render(images, sample_transform_params(self.spec, H, W, B, generator))
