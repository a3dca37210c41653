"""Mixup / CutMix for the fused supervised step: the draws on the host, the mixing on the GPU.

The fine-tune recipes of DeiT, BEiT, MAE and SimMIM and the DINO evaluation protocol train against mixed images with
two-label soft targets, through timm's `Mixup(mixup_alpha, cutmix_alpha, prob, switch_prob, mode)`.  Its semantics, restated:

  * the partner of row i is row B-1-i (the batch flipped);
  * with probability `prob` a draw mixes, otherwise the row is a copy with lam = 1;
  * when both alphas are > 0 CutMix is chosen with probability `switch_prob`, else whichever alpha is > 0 decides;
  * lam ~ Beta(alpha, alpha) of the chosen kind;
  * Mixup: x[i] <- lam x[i] + (1 - lam) x[partner];
  * CutMix: ratio = sqrt(1 - lam), cut = int(side * ratio) per side, a uniform integer centre, edges centre -+ cut // 2
    clipped to the image; the box of x[partner] is pasted into x[i] and lam becomes 1 - area / (H W);
  * the target of row i is lam s(y[i]) + (1 - lam) s(y[partner]), s the label-smoothed one-hot row;
  * mode "batch": one draw for the whole batch; "elem": one per row (rows i and B-1-i share nothing).

What stays on the host is the drawing (`sample_mix_params`), a pure function of ONE int64 taken from the torch generator (as
vit_core._runtime.next_seed takes the dropout seed), so that torch.manual_seed reproduces a run.  The mixing is one HIP
launch (vitssl_mix_batch) and the soft-target loss another (vitssl_classify_loss_mix); there is no CPU fallback.
"""
from dataclasses import dataclass
from typing import NamedTuple, Optional

import numpy as np
import torch

from vitssl_hip import _lib as L
from vitssl_hip import ops

_MODES = ("batch", "elem")
_KEYS = ("mixup_alpha", "cutmix_alpha", "prob", "switch_prob", "mode")


@dataclass
class MixSpec:
    mixup_alpha: float = 0.8
    cutmix_alpha: float = 1.0
    prob: float = 1.0
    switch_prob: float = 0.5
    mode: str = "batch"

    def __post_init__(self):
        if self.mode not in _MODES:
            raise ValueError(f"MixSpec: mode must be one of {list(_MODES)}, got {self.mode!r}")
        if self.mixup_alpha < 0 or self.cutmix_alpha < 0:
            raise ValueError(f"MixSpec: mixup_alpha = {self.mixup_alpha} and cutmix_alpha = {self.cutmix_alpha} must be >= 0")
        if not (0.0 <= self.prob <= 1.0 and 0.0 <= self.switch_prob <= 1.0):
            raise ValueError(f"MixSpec: prob = {self.prob} and switch_prob = {self.switch_prob} must lie in [0, 1]")

    @classmethod
    def from_config(cls, node) -> "MixSpec":
        """node: the mapping under `training.mixup` (any of mixup_alpha, cutmix_alpha, prob, switch_prob, mode)."""
        node = dict(node or {})
        unknown = sorted(set(node) - set(_KEYS))
        if unknown:
            raise ValueError(f"training.mixup: unknown key(s) {unknown}; the keys are {list(_KEYS)}")
        kw = {k: (str(v) if k == "mode" else float(v)) for k, v in node.items()}
        return cls(**kw)


def _draw_seed(generator: Optional[torch.Generator]) -> int:
    return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, generator=generator).item())


def sample_mix_params(spec: MixSpec, B: int, H: int, W: int, generator: Optional[torch.Generator] = None) -> dict:
    """-> dict of arrays [B]: kind (0 copy, 1 blend, 2 paste), partner, y0, y1, x0, x1 (int32) and lam (float32)."""
    rng = np.random.default_rng(_draw_seed(generator))
    n = B if spec.mode == "elem" else 1
    ma, ca = float(spec.mixup_alpha), float(spec.cutmix_alpha)
    # every draw is made whether or not it is used, so that one decision never shifts the stream of another
    u_apply, u_switch = rng.random(n), rng.random(n)
    lam_mix = rng.beta(ma, ma, n) if ma > 0 else np.ones(n)
    lam_cut = rng.beta(ca, ca, n) if ca > 0 else np.ones(n)
    cy, cx = rng.integers(0, H, n), rng.integers(0, W, n)

    apply = (u_apply < spec.prob) & ((ma > 0) or (ca > 0))
    cut = (u_switch < spec.switch_prob) if (ma > 0 and ca > 0) else np.full(n, ca > 0)
    lam = np.where(cut, lam_cut, lam_mix).astype(np.float64)

    ratio = np.sqrt(1.0 - lam)
    cut_h, cut_w = (H * ratio).astype(np.int64), (W * ratio).astype(np.int64)
    y0, y1 = np.clip(cy - cut_h // 2, 0, H), np.clip(cy + cut_h // 2, 0, H)
    x0, x1 = np.clip(cx - cut_w // 2, 0, W), np.clip(cx + cut_w // 2, 0, W)
    area = (y1 - y0) * (x1 - x0)
    lam_box = (1.0 - area.astype(np.float64) / float(H * W)).astype(np.float32)

    paste = apply & cut & (area > 0)                                # an empty box mixes nothing
    lam32 = lam.astype(np.float32)
    blend = apply & ~cut & (lam32 < 1.0)                            # lam == 1 mixes nothing either: never a blend with lam 1
    kind = np.where(paste, ops.MIX_PASTE, np.where(blend, ops.MIX_BLEND, ops.MIX_COPY))
    out_lam = np.where(paste, lam_box, np.where(blend, lam32, np.float32(1.0))).astype(np.float32)
    zero = np.zeros(n, np.int64)
    cols = dict(kind=kind, y0=np.where(paste, y0, zero), y1=np.where(paste, y1, zero), x0=np.where(paste, x0, zero),
                x1=np.where(paste, x1, zero))
    out = {k: np.broadcast_to(v.astype(np.int32), (B,)).copy() for k, v in cols.items()}
    out["partner"] = (B - 1 - np.arange(B)).astype(np.int32)
    out["lam"] = np.broadcast_to(out_lam, (B,)).copy()
    return out


_IP_COLUMNS = ("kind", "partner", "y0", "y1", "x0", "x1")


def pack_mix_params(params: dict, out: Optional[np.ndarray] = None) -> np.ndarray:
    """dict of `sample_mix_params` -> int32 [8 B]: the kernel's [B, 6] table, the bits of lam [B], the partners [B]"""
    B = len(params["kind"])
    block = np.empty(8 * B, np.int32) if out is None else out
    ip = block[:6 * B].reshape(B, ops.MIX_IP)
    for j, k in enumerate(_IP_COLUMNS):
        ip[:, j] = params[k]
    block[6 * B:7 * B] = np.asarray(params["lam"], np.float32).view(np.int32)
    block[7 * B:] = params["partner"]
    return block


class MixParams(NamedTuple):
    """One batch's mix on the device: iparams int32 [B, 6] and lam f32 [B] as vitssl_mix_batch reads them, partner int32 [B]
    as vitssl_classify_loss_mix does."""
    iparams: torch.Tensor
    lam: torch.Tensor
    partner: torch.Tensor


class GPUMixup:
    """Draws a batch's mix parameters and applies them on the GPU.  The pinned parameter block and the output buffer are
    reused between calls, as data.GPUTransform reuses its own: consume (or clone) a batch before mixing the next one."""

    def __init__(self, spec: MixSpec):
        self.spec = spec
        self._out = None
        self._pinned = None                             # int32 [8 B], page-locked
        self._copied = None                             # event behind the last copy out of it

    def to_device(self, params: dict, device=None) -> MixParams:
        """The arrays of `sample_mix_params` (or hand-made ones) as one non-blocking copy."""
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise L.VitsslError(f"GPUMixup: the parameters go to a 'cuda' device, got {dev} (no CPU fallback)")
        B = len(params["kind"])
        if self._pinned is None or self._pinned.shape[0] != 8 * B:
            self._pinned = torch.empty(8 * B, dtype=torch.int32).pin_memory()
            self._copied = torch.cuda.Event()
        else:
            self._copied.synchronize()                  # the previous batch's asynchronous copy has read the block
        pack_mix_params(params, self._pinned.numpy())
        block = self._pinned.to(dev, non_blocking=True)
        self._copied.record(torch.cuda.current_stream(dev))
        return MixParams(block[:6 * B].view(B, ops.MIX_IP), block[6 * B:7 * B].view(torch.float32), block[7 * B:])

    def draw(self, B: int, H: int, W: int, generator: Optional[torch.Generator] = None, device=None) -> MixParams:
        return self.to_device(sample_mix_params(self.spec, B, H, W, generator), device)

    def apply(self, x: torch.Tensor, params: MixParams) -> torch.Tensor:
        """x f32 [B,C,H,W] on the GPU -> the mixed batch, in this object's output buffer."""
        if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
            raise L.VitsslError("GPUMixup: the batch is on the CPU; move it to 'cuda' (no CPU fallback)")
        if self._out is None or self._out.shape != x.shape or self._out.device != x.device:
            self._out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        ops.mix_batch(x, self._out, params.iparams, params.lam)
        return self._out
