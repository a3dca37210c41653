"""Host-side composition of the HIP kernels into the vit_core forward/backward.

Design (MI355X-first, not a translation of the reference's eager module graph):
  * every parameter of a model lives in ONE flat fp32 buffer (FlatStore) with a
    matching flat gradient buffer; q/k/v weights are adjacent, so the fused QKV weight
    [3D, D] and its gradient are free views.  AdamW, EMA and the data-parallel
    all-reduce operate on the flat buffers (one kernel / few large collectives).
  * bf16 copies of every GEMM weight, plus the transposed copy the dgrad GEMM reads,
    are refreshed only when the flat buffer's version changes (once per optimizer step).
  * activations needed by backward are kept in step-persistent workspaces (288 GB of
    HBM: nothing is recomputed except dropout masks, which are counter-based).
  * backward is an explicit reverse schedule (no autograd graph inside the stack), so
    gradient ranges become ready in a known order and the reducer overlaps their
    all-reduce with the remaining backward on a side stream.
"""
from __future__ import annotations

import re
from typing import Callable, Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch
from torch import nn

from . import _lib as L
from . import ops

BF16 = torch.bfloat16
F32 = torch.float32
FP8 = ops.FP8
ALIGN = 64  # elements; keeps every parameter 256-byte aligned inside the flat buffer
MAX_TOKENS = 2048       # attention: streaming kernels for 257-2048 tokens (bf16 operands), csrc/attention_hd.hip with dh = 64 folded
FP8_MAX_TOKENS = 256    # the fp8 attention entry points (e4m3 images of out / dqkv) end where the one-workgroup-per-head kernels do

# Operand type of the FORWARD Linear products inside the encoder blocks: "bf16" (default, the reference's
# autocast contract) or "fp8" (OCP e4m3, BASELINE.json configs[4]; backward products stay bf16).  Read when an
# EncoderStack is built: set VITSSL_LINEAR_OPERANDS=fp8 or call set_linear_operands("fp8") before the model's
# first forward.
import os as _os

_LINEAR_OPERANDS = _os.environ.get("VITSSL_LINEAR_OPERANDS", "bf16")


def set_linear_operands(kind: str):
    global _LINEAR_OPERANDS
    if kind not in ("bf16", "fp8"):
        raise L.VitsslError(f"linear operands must be 'bf16' or 'fp8', got {kind!r}")
    _LINEAR_OPERANDS = kind


def linear_operands() -> str:
    if _LINEAR_OPERANDS not in ("bf16", "fp8"):
        raise L.VitsslError(f"VITSSL_LINEAR_OPERANDS must be 'bf16' or 'fp8', got {_LINEAR_OPERANDS!r}")
    return _LINEAR_OPERANDS


def _round_up(n: int, a: int) -> int:
    return (n + a - 1) // a * a


def as_f32(x: torch.Tensor) -> torch.Tensor:
    if x.dtype != F32:
        x = x.float()
    return x.contiguous()


class PatchGeometry:
    """Widths of the patch path of one model.  Pd = C * P * P is the contraction length of the patch projection and of the SimMIM
    head's input-gradient GEMM, and the output width of the head.  A geometry the kernels of vitssl_hip.h take as it is
    (P % 4 == 0 and Pd % 64 == 0) keeps its entry points and buffers.  Every other one runs at the padded width
    Pdp = round_up(Pd, 64) inside the engine (include/vitssl_patch.h): patches, the bf16 weight images and the head's gradient
    carry zero pad columns; parameters, gradients and the public tensors keep the reference's shapes."""

    def __init__(self, C: int, P: int):
        self.C, self.P = int(C), int(P)
        self.Pd = self.C * self.P * self.P
        self.native = self.P % 4 == 0 and self.Pd % 64 == 0
        self.Pdp = self.Pd if self.native else _round_up(self.Pd, 64)
        if self.C < 1 or self.P < 1:
            raise L.VitsslError(f"patch_size={P} and the channel count {C} of input_shape must be positive")
        if not self.native and self.C * self.P * (self.P + 31) > 16000:      # the LDS tile of csrc/patch.hip (include/vitssl_patch.h)
            raise L.VitsslError(f"patch_size={P} with {C} channels: the channel rows of one patch do not fit the patchify kernel's "
                                f"LDS tile (C * P * (P + 31) = {self.C * self.P * (self.P + 31)} > 16000); a patch size that is a multiple "
                                "of 4 with C * P * P a multiple of 64 has no such limit")
        # output width of the head GEMM (N % 4 == 0): Pd itself where it qualifies, else the padded width
        self.Np = self.Pd if self.Pd % 4 == 0 else self.Pdp

    # Every choice between the entry points of vitssl_hip.h and those of vitssl_patch.h is made below: callers never ask which.
    def patchify(self, x, patches):
        (ops.patchify_bf16 if self.native else ops.patchify_ld_bf16)(x, patches, self.P)

    def register_proj(self, store: "FlatStore", key: str, src: Callable[[], torch.Tensor], D: int):
        """The bf16 image [D, Pdp] of the patch projection weight src() [D, Pd] (zero pad columns); no transpose: nothing takes
        the projection's input gradient."""
        if self.native:
            store.register_weight(key, src, transposed_too=False)
        else:
            store.register_padded_weight(key, src, D, self.Pdp, transposed_too=False)

    def proj_image(self, w):
        """register_proj without a store: a fresh bf16 [D, Pdp] image of the f32 weight w [D, Pd] (D % 8 == 0)."""
        if self.native:
            wb = torch.empty(w.shape, dtype=BF16, device=w.device)
            ops.cast_transpose_bf16(w, wb, None)
        else:
            wb = torch.zeros(w.shape[0], self.Pdp, dtype=BF16, device=w.device)
            ops.CastPlanLd().run([(w, wb, None)])
        return wb

    def proj_wgrad(self, dproj, patches, gw, ws: "Workspace"):
        """gw f32 [D, Pd] += dproj^T @ patches[:, :Pd]"""
        if self.native:
            ops.gemm_tn(dproj, patches, gw)
            return
        tmp = ws.get("pad.proj_wgrad", (gw.shape[0], self.Pdp), F32, gw.device)
        tmp.zero_()
        ops.gemm_tn(dproj, patches, tmp)
        ops.accumulate_ld_f32(gw, tmp)      # the column prefix of the padded result

    def gather_targets(self, x, idx, out):
        """out f32 [len(idx), Pd] = the patches idx (rows b * N + n) of the image x, bit for bit"""
        (ops.gather_patches_f32 if self.native else ops.gather_patches_any_f32)(x, idx, out, self.P)

    def l1_loss(self, pred, targets, loss_sum, dpred, gscale):
        """loss_sum += sum |pred - targets|; dpred bf16 [Mm, Pdp] = gscale * sign(pred - targets), pad columns zero"""
        (ops.l1_loss if self.native else ops.l1_loss_ld)(pred, targets, loss_sum, dpred, gscale=gscale)

    def widen_grad(self, dpred):
        """A gradient [Mm, Pd] handed in by autograd -> the bf16 [Mm, Pdp] the engine's backward reads (pad columns zero); an
        empty one (SimMIM without a masked token) launches nothing."""
        dp = as_f32(dpred)
        if dp.numel() == 0:
            return torch.empty(0, self.Pdp, dtype=BF16, device=dp.device)
        dpb = torch.empty(dp.shape, dtype=BF16, device=dp.device)
        ops.cast_bf16(dp, dpb)
        if self.Pdp != self.Pd:
            wide = torch.zeros(dp.shape[0], self.Pdp, dtype=BF16, device=dp.device)
            wide[:, :self.Pd] = dpb
            dpb = wide
        return dpb


class Workspace:
    """Named device buffers reused across steps (no allocation in steady state)."""

    def __init__(self):
        self._bufs: Dict[str, torch.Tensor] = {}

    def get(self, name: str, shape, dtype, device) -> torch.Tensor:
        t = self._bufs.get(name)
        shape = tuple(int(s) for s in shape)
        if t is None or t.shape != shape or t.dtype != dtype or t.device != device:
            t = torch.empty(shape, dtype=dtype, device=device)
            self._bufs[name] = t
        return t

    def clear(self):
        self._bufs.clear()


class PatchHead:
    """The Linear D -> Pd that predicts patch pixels (SimMIM's head, MAE's decoder_pred) on a flat store.  A native geometry runs
    it as it is.  Any other keeps the weight images at [Pdp, D] / [D, Pdp] with zero pad (`key`, `key + '.T'`), takes the
    gradient of the prediction at the width Pdp and forms the weight and bias gradients at that width in the workspaces
    `pad.<key>_*` of `ws`; parameters, gradients and the prediction keep the reference's shapes."""

    def __init__(self, store: "FlatStore", geo: PatchGeometry, key: str, weight_name: str, bias_name: str, D: int, ws: Workspace):
        self.store, self.geo, self.key, self.wname, self.bname, self.D, self.ws = store, geo, key, weight_name, bias_name, int(D), ws
        src = lambda: store.view(weight_name, (geo.Pd, self.D))      # noqa: E731
        if geo.native:
            store.register_weight(key, src)
        else:
            store.register_padded_weight(key, src, geo.Pdp, self.D)

    def forward(self, h):
        """h bf16 [Mm, D] -> pred f32 [Mm, Pd], a fresh tensor"""
        st, Pd, Np = self.store, self.geo.Pd, self.geo.Np
        if Np == Pd:
            pred = torch.empty(h.shape[0], Pd, dtype=F32, device=h.device)
            ops.gemm_nt(h, st.w(self.key)[:Pd], pred, L.EPI_F32, bias=st.view(self.bname))
            return pred
        # Pd % 4 != 0: the GEMM writes the padded width (zero weight rows and zero bias give zero pad columns); the prediction
        # is the column prefix of that buffer
        bias = self.ws.get(f"pad.{self.key}_bias", (Np,), F32, h.device)
        bias.zero_()
        bias[:Pd].copy_(st.view(self.bname))
        wide = torch.empty(h.shape[0], Np, dtype=F32, device=h.device)
        ops.gemm_nt(h, st.w(self.key), wide, L.EPI_F32, bias=bias)
        return wide[:, :Pd]

    def wgrad(self, dpred, h):
        """the flat gradients of bias and weight += column sums of dpred bf16 [Mm, Pdp] (pad columns zero), dpred^T @ h"""
        Pd, Pdp = self.geo.Pd, self.geo.Pdp
        gb, gw = self.store.gview(self.bname, (1, Pd)), self.store.gview(self.wname, (Pd, self.D))
        if self.geo.native:
            ops.colsum_bf16(dpred, gb.view(Pd))
            ops.gemm_tn(dpred, h, gw)
            return
        # at the padded width, then the first Pd entries / rows into the flat buffer
        hb = self.ws.get(f"pad.{self.key}_bgrad", (1, Pdp), F32, h.device)
        hw = self.ws.get(f"pad.{self.key}_wgrad", (Pdp, self.D), F32, h.device)
        hb.zero_()
        hw.zero_()
        ops.colsum_bf16(dpred, hb.view(Pdp))
        ops.gemm_tn(dpred, h, hw)
        ops.accumulate_ld_f32(gb, hb)
        ops.accumulate_ld_f32(gw, hw[:Pd])

    def dgrad(self, dpred, out):
        """out bf16 [Mm, D] = dpred @ W"""
        ops.gemm_nt(dpred, self.store.w(self.key + ".T"), out, L.EPI_BF16)


class HostStage:
    """Host index tables -> device, through a ring of `slots` persistent pinned buffers: one hipHostMalloc per slot and size,
    ever (pinning fresh pages every step costs milliseconds and serialises with the launch queue on ROCm: measured 15 ms of GPU
    idle per step), and one copy per upload.  The views an upload returns are overwritten by the `slots`-th later upload."""

    def __init__(self, slots: int = 4):
        self.slots, self._ring, self._key, self._pos = int(slots), [], None, 0

    def upload(self, arrays, dev) -> List[torch.Tensor]:
        """NumPy arrays (1-D, contiguous, any dtypes) -> device views of the same dtypes and lengths: packed at 256-byte
        aligned offsets into the next slot's pinned bytes and copied to the slot's device buffer on the current stream.  A slot
        is reused only after the event recorded behind its last copy has completed."""
        offs, total = [], 0
        for a in arrays:
            offs.append(total)
            total = _round_up(total + a.nbytes, 256)
        if self._key != (total, str(dev)):
            self._ring = [[torch.empty(total, dtype=torch.uint8).pin_memory(), torch.empty(total, dtype=torch.uint8, device=dev), None]
                          for _ in range(self.slots)]
            self._key, self._pos = (total, str(dev)), 0
        slot = self._ring[self._pos % self.slots]
        self._pos += 1
        host, d, ev = slot
        if ev is not None:
            ev.synchronize()
        staged = host.numpy()
        for o, a in zip(offs, arrays):
            staged[o:o + a.nbytes] = a.view(np.uint8)          # plain memcpy into the pinned pages (no torch CPU op)
        d.copy_(host, non_blocking=True)
        slot[2] = torch.cuda.Event()
        slot[2].record(torch.cuda.current_stream())
        return [d[o:o + a.nbytes].view(torch.from_numpy(a[:0]).dtype) for o, a in zip(offs, arrays)]


# ---- parameter names of the stores: what the optimizer's per-parameter settings are keyed by -------------------------------------
# A store keeps the module tree's names: `encoder_blocks.<i>.` inside a backbone (ViT / SimMIMViT directly, DINOViT under
# `student_backbone.` / `teacher_backbone.`), the embedding as `patch_embedding.*` (ViT, DINOViT) or `projection.*`,
# `positional_embedding`, `mask_token` (SimMIMViT); everything else is a head.
_BLOCK_NAME = re.compile(r"(?:^|\.)encoder_blocks\.(\d+)\.")
_TOKEN_NAMES = ("cls_token", "positional_embedding", "mask_token")


def num_layers(names) -> int:
    """Number of encoder blocks among the parameter names of a store."""
    ids = [int(m.group(1)) for m in map(_BLOCK_NAME.search, names) if m]
    return max(ids) + 1 if ids else 0


def layer_id(name: str, layers: int) -> int:
    """Depth of a parameter for layer-wise lr decay: 0 for the patch embedding / projection, the tokens and the positional table,
    i + 1 for `encoder_blocks.i`, layers + 1 for everything else (the heads)."""
    m = _BLOCK_NAME.search(name)
    if m:
        return int(m.group(1)) + 1
    parts = name.split(".")
    if "patch_embedding" in parts or parts[0] == "projection" or parts[-1] in _TOKEN_NAMES:
        return 0
    return layers + 1


def exempt_from_weight_decay(name: str, ndim: int) -> bool:
    """The ViT recipes' rule: biases and norm parameters (ndim <= 1), the tokens and the positional table are not decayed."""
    return ndim <= 1 or name.split(".")[-1] in _TOKEN_NAMES


class FlatStore:
    """Flat fp32 parameter / gradient buffers behind an nn.Module tree.

    The module keeps ordinary nn.Parameters with the reference's state_dict keys; their
    storage is re-pointed into `self.flat` (and `.grad` into `self.gflat` on request).
    """

    def __init__(self, module: nn.Module, device: torch.device, only: Optional[Callable[[str], bool]] = None,
                 forward_only: bool = False):
        self.module = module
        self.device = device
        # forward_only: no backward ever runs through these weights (DINO's teacher): the transposed bf16 images, operands of
        # the input-gradient GEMMs only, are not kept (a third of the cast's bytes per optimizer step)
        self.forward_only = bool(forward_only)
        self.names: List[str] = []
        self.params: List[nn.Parameter] = []
        self.offsets: Dict[str, Tuple[int, int]] = {}
        off = 0
        for name, p in module.named_parameters():
            if only is not None and not only(name):
                continue
            n = p.numel()
            self.names.append(name)
            self.params.append(p)
            self.offsets[name] = (off, n)
            off = _round_up(off + n, ALIGN)
        self.numel = off
        self.flat = torch.zeros(off, dtype=F32, device=device)
        self.gflat = torch.zeros(off, dtype=F32, device=device)
        with torch.no_grad():
            for name, p in zip(self.names, self.params):
                o, n = self.offsets[name]
                view = self.flat[o:o + n].view(p.shape)
                view.copy_(p.data)
                p.data = view
        self._bf16: Dict[str, torch.Tensor] = {}
        self._bf16_key = None
        self.generation = 0   # bumped whenever the flat buffer is rewritten behind torch's back
        self._cast_jobs: List[Tuple[str, Callable[[], torch.Tensor], bool, bool]] = []
        self._cast_pad: Dict[str, Tuple[int, int]] = {}    # key -> padded (rows, cols) of its bf16 images
        self._fp8: Dict[str, torch.Tensor] = {}
        self._fp8_jobs: List[Tuple[str, Callable[[], torch.Tensor]]] = []
        self._fp8_plan = None
        self._fp8_index: Dict[str, int] = {}

    # ---- bookkeeping -------------------------------------------------------
    def is_attached(self) -> bool:
        """True while every Parameter still aliases the flat buffer (a .to()/.cuda() or
        load with assign=True re-allocates them)."""
        base = self.flat.data_ptr()
        for name, p in zip(self.names, self.params):
            o, _ = self.offsets[name]
            if p.data_ptr() != base + 4 * o:
                return False
        return True

    def view(self, name: str, shape=None) -> torch.Tensor:
        o, n = self.offsets[name]
        v = self.flat[o:o + n]
        return v.view(shape) if shape is not None else v

    def gview(self, name: str, shape=None) -> torch.Tensor:
        o, n = self.offsets[name]
        v = self.gflat[o:o + n]
        return v.view(shape) if shape is not None else v

    def span(self, first: str, last: str) -> Tuple[int, int]:
        lo = self.offsets[first][0]
        o, n = self.offsets[last]
        return lo, o + n

    def prefix_span(self, prefix: str) -> Tuple[int, int]:
        """span() of the parameters whose names start with `prefix` (one submodule: adjacent in the store)."""
        names = [n for n in self.names if n.startswith(prefix)]
        return self.span(names[0], names[-1])

    def span_view(self, first: str, last: str, shape, grad=False) -> torch.Tensor:
        lo, hi = self.span(first, last)
        buf = self.gflat if grad else self.flat
        v = buf[lo:hi]
        if v.numel() != int(torch.Size(shape).numel()):
            raise L.VitsslError(f"parameters {first}..{last} are not contiguous in the flat store")
        return v.view(shape)

    def attach_grads(self):
        """Make every p.grad a view of the flat gradient buffer (fused-step mode)."""
        for name, p in zip(self.names, self.params):
            p.grad = self.gview(name, p.shape)

    def mark_dirty(self):
        """Called by everything that rewrites the flat buffer through a raw pointer (the HIP
        AdamW / EMA kernels, broadcasts): torch's version counters do not see those writes."""
        self.generation += 1

    def weights_key(self):
        """Changes whenever any parameter value may have changed.  `p.data = flat_view` gives
        every Parameter its OWN version counter, so in-place updates through the Parameters
        (any torch optimizer, load_state_dict, p.copy_ / p.mul_ ...) bump p._version and leave
        flat._version alone: the key has to include both (about 150 integers per model)."""
        pv = 0
        for p in self.params:
            pv += p._version
        return (self.generation, self.flat._version, pv)

    # ---- bf16 weight caches --------------------------------------------------
    def register_weight(self, key: str, src: Callable[[], torch.Tensor], transposed_too: bool = True, plain: bool = True):
        """Declare a 2-D GEMM weight [N,K]; caches `key` (bf16 [N,K], unless plain=False) and, if asked,
        `key + '.T'` (bf16 [K,N], the operand of the dgrad GEMM)."""
        self._cast_jobs.append((key, src, transposed_too and not self.forward_only, plain))

    def register_padded_weight(self, key: str, src: Callable[[], torch.Tensor], rows: int, cols: int, transposed_too: bool = True):
        """register_weight for a patch-facing weight [N,K] whose bf16 images are kept at the padded shape [rows, cols] /
        [cols, rows] (rows >= N, cols >= K).  The images are allocated zeroed and the cast writes the source's image only
        (one launch for the whole store, ops.CastPlanLd), so the pad rows and columns are zero after every refresh."""
        self._cast_pad[key] = (int(rows), int(cols))
        self.register_weight(key, src, transposed_too)

    def register_fp8_weight(self, key: str, src: Callable[[], torch.Tensor]):
        """Declare a 2-D GEMM weight [N,K] whose GEMM operands are e4m3 images with a per-tensor power-of-two
        scale: `w8(key)` returns (image [N,K], dequantisation factor as a 1-element device tensor), `w8t(key)`
        the transposed image [K,N] (operand of the input-gradient GEMM) with the same factor."""
        self._fp8_index[key] = len(self._fp8_jobs)
        self._fp8_jobs.append((key, src))

    def refresh_weights(self):
        key = self.weights_key()
        if key == self._bf16_key and (self._bf16 or self._fp8):
            return
        jobs = []
        for wname, src, tr, plain in self._cast_jobs:     # (never `key`: that is the cache key stored below)
            w = src()
            R, Cn = w.shape
            alloc = torch.empty
            if wname in self._cast_pad:      # padded images: zeroed once, the cast never touches the pad
                R, Cn = self._cast_pad[wname]
                alloc = torch.zeros
            dst = self._bf16.get(wname) if plain else None
            if plain and (dst is None or dst.shape != (R, Cn)):
                dst = alloc(R, Cn, dtype=BF16, device=self.device)
                self._bf16[wname] = dst
            dst_t = None
            if tr:
                dst_t = self._bf16.get(wname + ".T")
                if dst_t is None or dst_t.shape != (Cn, R):
                    dst_t = alloc(Cn, R, dtype=BF16, device=self.device)
                    self._bf16[wname + ".T"] = dst_t
            jobs.append((w.contiguous(), dst, dst_t))
        if jobs:      # every weight of the store in one launch (was ~50 launches of ~12 us)
            if getattr(self, "_cast_plan", None) is None:
                self._cast_plan = ops.CastPlanLd() if self._cast_pad else ops.CastPlan()
            self._cast_plan.run(jobs)
        if self._fp8_jobs:
            jobs8 = []
            for k8, src in self._fp8_jobs:
                w = src()
                R, Cn = w.shape
                dst, dst_t = self._fp8.get(k8), self._fp8.get(k8 + ".T")
                if dst is None or dst.shape != (R, Cn):
                    dst = torch.empty(R, Cn, dtype=FP8, device=self.device)
                    dst_t = torch.empty(Cn, R, dtype=FP8, device=self.device)
                    self._fp8[k8], self._fp8[k8 + ".T"] = dst, dst_t
                jobs8.append((w.contiguous(), dst, dst_t))
            if self._fp8_plan is None:
                self._fp8_plan = ops.Fp8WeightPlan()
            self._fp8_plan.run(jobs8)
        self._bf16_key = key

    def w(self, key: str) -> torch.Tensor:
        return self._bf16[key]

    def w8(self, key: str) -> Tuple[torch.Tensor, torch.Tensor]:
        j = self._fp8_index[key]
        return self._fp8[key], self._fp8_plan.alpha[j:j + 1]

    def w8t(self, key: str) -> Tuple[torch.Tensor, torch.Tensor]:
        j = self._fp8_index[key]
        return self._fp8[key + ".T"], self._fp8_plan.alpha[j:j + 1]


RESERVED_CUS_DEFAULT = 8


def configure_collectives(reserve_cus: int = RESERVED_CUS_DEFAULT):
    """Size the collective library to the CUs the persistent GEMM grids leave alone.  Call BEFORE
    torch.distributed.init_process_group (RCCL reads its environment when the communicator is built).

    RCCL launches one workgroup per channel and a ring only progresses while all of them are resident.  RCCL 2.26 on
    gfx950 sets up 128 collective channels (tools/rccl_probe.py, NCCL_DEBUG=INFO, one MI355X); with the GEMM grids holding
    every other CU for a whole kernel, a collective of more channels than reserved CUs would only start at kernel
    boundaries.  So the channel count is capped at the reserve (unless the user has set NCCL_MAX_NCHANNELS): 8 channels
    move the 345 MB of ViT-B gradients (604 MB per GPU through the ring) well inside one backward pass.
    Returns the values in force."""
    if "NCCL_MAX_NCHANNELS" not in _os.environ:
        _os.environ["NCCL_MAX_NCHANNELS"] = str(max(1, int(reserve_cus)))
    if "NCCL_MIN_NCHANNELS" not in _os.environ:
        _os.environ["NCCL_MIN_NCHANNELS"] = str(min(int(_os.environ["NCCL_MAX_NCHANNELS"]), max(1, int(reserve_cus))))
    return {k: _os.environ.get(k) for k in ("NCCL_MAX_NCHANNELS", "NCCL_MIN_NCHANNELS")}


class GradReducer:
    """Data-parallel gradient averaging over RCCL (torch.distributed 'nccl' on ROCm),
    overlapped with backward: the engine calls `ready(lo, hi)` as soon as a contiguous
    range of the flat gradient buffer is final; ranges are coalesced into buckets of
    >= `bucket_elems` and all-reduced (sum) on a side stream.  The 1/world factor is
    folded into the optimizer kernel.  On CPU tensors (gloo, tests) it runs inline."""

    def __init__(self, gflat: torch.Tensor, group=None, bucket_mb: float = 32.0, expect=None,
                 reserve_cus: int = RESERVED_CUS_DEFAULT):
        """`expect` = (lo, hi) range of the flat buffer that one backward must hand over exactly once
        (default: the whole buffer); finish() checks it, so a schedule change that forgets or repeats a
        range fails loudly on one GPU instead of silently de-synchronising replicas on eight.
        A LIST of (lo, hi) ranges (the trainable spans of a partly frozen model, ViT.reduce_ranges) is checked as exactly
        those: every one handed over once and nothing outside them."""
        import torch.distributed as dist
        self.dist = dist
        self.gflat = gflat
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
        if self.world > 1 and gflat.is_cuda:
            # The persistent GEMM workgroups take a CU's whole register file: the collective library's kernels can only run
            # beside them on CUs the GEMM grids leave alone.  Explicit library state, re-read on
            # every launch: it does not matter whether a forward ran before this reducer was built.  VITSSL_RESERVE_CUS
            # (if set) is the user's choice and wins; otherwise `reserve_cus`.
            if "VITSSL_RESERVE_CUS" not in _os.environ:
                L.call("vitssl_set_reserved_cus", int(reserve_cus))
        self.bucket_elems = int(bucket_mb * 1024 * 1024 / 4)
        self.pending: List[Tuple[int, int]] = []
        self.pending_elems = 0
        self.handles = []
        self.cuda = gflat.is_cuda
        # high priority: when a CU frees up, the collective's workgroups are dispatched ahead of the queued GEMM workgroups
        self.comm_stream = torch.cuda.Stream(device=gflat.device, priority=-1) if self.cuda else None
        self.launched: List[Tuple[int, int]] = []
        self.expect = expect if expect is not None else (0, gflat.numel())
        self.check_coverage = True
        # diagnostics (bench.py, first real multi-GPU run): with `timing` on, every bucket is bracketed by events on the
        # communication stream, and begin() drops one on the compute stream, so bucket_times() can tell whether buckets
        # queue behind the persistent GEMMs (start late / run long) or finish under the backward
        self.timing = False
        self._t0 = None
        self._bucket_events = []

    def _flush(self):
        if not self.pending:
            return
        # merge adjacent ranges (the backward schedule hands them over high-to-low)
        rng = sorted(self.pending)
        merged = [list(rng[0])]
        for lo, hi in rng[1:]:
            if lo <= merged[-1][1]:
                merged[-1][1] = max(merged[-1][1], hi)
            else:
                merged.append([lo, hi])
        self.pending, self.pending_elems = [], 0
        for lo, hi in merged:
            self.launched.append((lo, hi))
            if self.world == 1:
                continue
            chunk = self.gflat[lo:hi]
            if self.cuda:
                self.comm_stream.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(self.comm_stream):
                    if self.timing:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(self.comm_stream)
                    self.dist.all_reduce(chunk, group=self.group)
                    if self.timing:
                        e1.record(self.comm_stream)
                        self._bucket_events.append((4 * (hi - lo), e0, e1))
            else:
                self.handles.append(self.dist.all_reduce(chunk, group=self.group, async_op=True))

    def begin(self):
        self.pending, self.pending_elems, self.handles, self.launched = [], 0, [], []
        if self.timing and self.cuda:
            self._bucket_events = []
            self._t0 = torch.cuda.Event(enable_timing=True)
            self._t0.record(torch.cuda.current_stream())

    def bucket_times(self):
        """[(bytes, ms from begin() to the bucket's start on the communication stream, ms the all-reduce took)] of the last
        step run with `timing` on (synchronises)."""
        if not self._bucket_events:
            return []
        torch.cuda.synchronize()
        return [(nbytes, round(self._t0.elapsed_time(e0), 3), round(e0.elapsed_time(e1), 3)) for nbytes, e0, e1 in self._bucket_events]

    def ready(self, lo: int, hi: int):
        self.pending.append((lo, hi))
        self.pending_elems += hi - lo
        if self.pending_elems >= self.bucket_elems:
            self._flush()

    def finish(self):
        """Launch what is left and make the compute stream wait for all buckets."""
        self._flush()
        for h in self.handles:
            h.wait()
        self.handles = []
        if self.cuda and self.world > 1:
            torch.cuda.current_stream().wait_stream(self.comm_stream)
        if self.check_coverage:
            self._assert_covered()

    def _assert_covered(self):
        """Every element of the expected range was handed over exactly once (alignment padding between
        parameters may be skipped: it is never read)."""
        if isinstance(self.expect, list):
            return self._assert_covered_ranges()
        pos = self.expect[0]
        for lo, hi in sorted(self.launched):
            if lo < pos:
                raise L.VitsslError(f"GradReducer: gradient range [{lo}, {hi}) was reduced twice (previous range ended at {pos})")
            if lo - pos >= ALIGN:
                raise L.VitsslError(f"GradReducer: gradient range [{pos}, {lo}) was never handed to the reducer")
            pos = hi
        if self.expect[1] - pos >= ALIGN:
            raise L.VitsslError(f"GradReducer: gradient range [{pos}, {self.expect[1]}) was never handed to the reducer")

    @staticmethod
    def _minus(a, b):
        """the pieces of the ranges `a` that the sorted ranges `b` do not cover (alignment padding does not count)"""
        out = []
        for lo, hi in sorted(a):
            pos = lo
            for blo, bhi in b:
                if bhi <= pos or blo >= hi:
                    continue
                if blo - pos >= ALIGN:
                    out.append((pos, blo))
                pos = max(pos, bhi)
            if hi - pos >= ALIGN:
                out.append((pos, hi))
        return out

    def _assert_covered_ranges(self):
        """`expect` is a list: every range of the list was handed over once, and nothing outside the list."""
        got, want = sorted(self.launched), sorted(self.expect)
        pos = None
        for lo, hi in got:
            if pos is not None and lo < pos:
                raise L.VitsslError(f"GradReducer: gradient range [{lo}, {hi}) was reduced twice (previous range ended at {pos})")
            pos = hi
        for lo, hi in self._minus(want, got):
            raise L.VitsslError(f"GradReducer: gradient range [{lo}, {hi}) was never handed to the reducer")
        for lo, hi in self._minus(got, want):
            raise L.VitsslError(f"GradReducer: gradient range [{lo}, {hi}) is outside the expected ranges {want}")

    def stats(self):
        """(number of buckets, bytes) of the last step."""
        return len(self.launched), 4 * sum(hi - lo for lo, hi in self.launched)

    @property
    def grad_scale(self) -> float:
        return 1.0 / self.world


def drop_path_rates(rate: float, layers: int) -> List[float]:
    """The stochastic-depth schedule of the ViT recipes (timm's `drop_path_rate`): block i of `layers` drops its two residual
    branches with probability rate * i / (layers - 1), i.e. linspace(0, rate, layers); 0 for a single block."""
    rate = float(rate)
    if not 0.0 <= rate < 1.0:
        raise ValueError(f"drop_path_rate must lie in [0, 1), got {rate}")
    if layers <= 1:
        return [0.0] * max(layers, 0)
    return [rate * i / (layers - 1) for i in range(layers)]


class _GradOperand(NamedTuple):
    """A gradient tensor that GEMMs read.  bf16 operands: the bf16 image x.  fp8 operands: the e4m3 image x8 = e4m3(value * scale)
    with 1-element views of the slot's delayed-scaling state (amax receives max |value|, inv = 1 / scale); x exists only in the
    self-calibrating first backward of a slot."""
    x: Optional[torch.Tensor]
    x8: Optional[torch.Tensor] = None
    scale: Optional[torch.Tensor] = None
    amax: Optional[torch.Tensor] = None
    inv: Optional[torch.Tensor] = None


class EncoderStack:
    """L pre-LN transformer blocks (vit_core/encoder_block.py:40-53) on a flat store.

    `drop_path` (stochastic depth, include/vitssl_droppath.h): per-block probabilities with which a training forward drops a
    whole sample from the block's attention branch and, drawn independently, from its MLP branch; survivors are scaled by
    1 / (1 - rate).  None or all zeros: nothing of it is launched.  bf16 operands only.

    `layer_scale` (LayerScale, include/vitssl_layerscale.h): the store holds `<block>layer_scale1.gamma` and
    `<block>layer_scale2.gamma` (f32 [D]) and every forward, in every mode, multiplies the attention branch by the first and the
    MLP branch by the second, per channel; a saving forward also keeps the two branches as bf16 images (2 * L * M * D * 2 bytes),
    from which the backward sums gamma's gradients.  False: nothing of it is launched.  bf16 operands only."""

    def __init__(self, store: FlatStore, block_prefixes: List[str], D: int, H: int, F: int, p_drop: float,
                 site_base: int = 0, drop_path: Optional[List[float]] = None, layer_scale: bool = False):
        if D % H != 0:
            raise AssertionError(f"d_model({D}) must be cleanly divisible by num_heads({H})!")
        self.store = store
        self.bp = list(block_prefixes)     # e.g. ["encoder_blocks.0.", ...] or [""] for a lone block
        self._spans = [store.prefix_span(b) for b in self.bp]      # what the backward hands to the reducer, block by block
        self.L, self.D, self.H, self.F = len(self.bp), D, H, F
        self.dh = D // H
        self.p = float(p_drop)
        self.site_base = site_base
        self.ws = Workspace()
        self._saved = {}
        self.fp8 = linear_operands() == "fp8"
        rates = [float(r) for r in drop_path] if drop_path is not None else []
        if rates and len(rates) != self.L:
            raise ValueError(f"drop_path holds {len(rates)} rates for {self.L} blocks")
        if any(not 0.0 <= r < 1.0 for r in rates):
            raise ValueError(f"drop_path rates must lie in [0, 1), got {rates}")
        self.drop_path = rates if any(r > 0.0 for r in rates) else None
        if self.drop_path is not None and self.fp8:
            raise L.VitsslError("drop path (drop_path_rate > 0) is built for bf16 linear operands only: use bf16 operands "
                                "(set_linear_operands('bf16') or VITSSL_LINEAR_OPERANDS=bf16) or drop_path_rate = 0")
        if self.drop_path is not None and 2 * self.L > L.DROPPATH_MAX_SITES:
            raise L.VitsslError(f"drop path covers up to {L.DROPPATH_MAX_SITES // 2} blocks a stack, got {self.L}")
        self.layer_scale = bool(layer_scale)
        if self.layer_scale:
            if self.fp8:
                raise L.VitsslError("LayerScale (layer_scale_init) is built for bf16 linear operands only: use bf16 operands "
                                    "(set_linear_operands('bf16') or VITSSL_LINEAR_OPERANDS=bf16) or leave layer_scale_init out")
            for b in self.bp:
                for leaf in ("layer_scale1.gamma", "layer_scale2.gamma"):
                    if b + leaf not in store.offsets:
                        raise L.VitsslError(f"LayerScale: the store holds no parameter {b + leaf!r}")
                    if store.offsets[b + leaf][1] != D:
                        raise L.VitsslError(f"LayerScale: {b + leaf!r} holds {store.offsets[b + leaf][1]} values, expected embed_dim = {D}")
        if self.fp8 and (D % 128 != 0 or F % 128 != 0):
            raise L.VitsslError(f"fp8 linear operands need embed_dim ({D}) and mlp_dim ({F}) to be multiples of 128")
        for b in self.bp:
            a = b + "self_attention."
            srcs = {
                "wqkv": lambda a=a, D=D: store.span_view(a + "w_query.weight", a + "w_value.weight", (3 * D, D)),
                "wo": lambda a=a: store.view(a + "final_linear.weight", (D, D)),
                "w1": lambda b=b: store.view(b + "feed_forward.linear_in.weight", (F, D)),
                "w2": lambda b=b: store.view(b + "feed_forward.linear_out.weight", (D, F)),
            }
            for leaf, src in srcs.items():
                if self.fp8:      # e4m3 images [N,K] (forward) and [K,N] (input gradients); no bf16 copies
                    store.register_fp8_weight(b + leaf, src)
                else:
                    store.register_weight(b + leaf, src)
        # fp8: per block, scales of the four gradient tensors that feed an input-gradient GEMM
        # (0: d(FFN out) -> FC2, 1: d(FFN hidden) -> FC1, 2: d(attention out) -> out-projection, 3: dQKV -> QKV).
        # Delayed scaling: a step quantises with the power-of-two scale derived from the PREVIOUS step's max |value|
        # (one bit of headroom); the very first backward derives each scale from the tensor itself (one extra pass).
        # The state is kept PER SLOT: DINO runs the student stack's backward twice per step (local crops, then global
        # crops: different row counts and gradient magnitudes), and a scale taken from the other pass's maxima would
        # clamp or lose low bits whenever the two differ by more than the one bit of headroom.
        self._gs_by_slot: Dict[str, dict] = {}    # slot -> {"scale", "inv", "amax", "used": [L, 4] device tensors, "valid": bool}
        self._gs = None                           # state of the slot whose backward is running / ran last

    # names ----------------------------------------------------------------
    def _n(self, i, leaf):
        return self.bp[i] + leaf

    def block_span(self, i) -> Tuple[int, int]:
        return self._spans[i]

    def _drop(self, i, which, seed, training):
        if not training or self.p <= 0.0:
            return ops.NO_DROP
        return ops.make_dropout(self.p, seed, self.site_base + 3 * i + which)

    def needs_seed(self, training: bool) -> bool:
        """Whether a forward in this mode draws from the dropout stream (element dropout or drop path): callers take a step seed
        from the torch generator exactly then."""
        return bool(training) and (self.p > 0.0 or self.drop_path is not None)

    def drop_path_sites(self) -> List[Tuple[float, int]]:
        """(rate, site) of the table's rows: row 2 i is block i's attention branch, row 2 i + 1 its MLP branch.  The sites carry
        VITSSL_DROPPATH_SITE_BIT, which no dropout site (site_base + 3 i + which) has, plus site_base, so the stacks of one model
        (spaced like their dropout sites) draw apart as well."""
        return [(r, L.DROPPATH_SITE_BIT | ((self.site_base + 2 * i + br) & 0x7FFFFFFF)) for i, r in enumerate(self.drop_path or [])
                for br in (0, 1)]

    def drop_path_table(self, slot: str = "a") -> Optional[torch.Tensor]:
        """The f32 [2 L, B] table of branch scales the last saving forward of `slot` applied (None: drop path did not run)."""
        return self._saved[slot].get("dp")

    def check_tokens(self, T: int):
        """Refuse a head dim or a sequence length the attention kernels of this operand mode do not cover.  Models call it at the top of
        their forward, before the first kernel of the step; forward() below repeats it for lone blocks."""
        if self.fp8 and self.dh != 64:
            raise L.VitsslError(f"fp8 linear operands support head dim 64 only, got embed_dim / num_heads = {self.D} / {self.H} = "
                                f"{self.dh}: use bf16 operands (set_linear_operands('bf16') or VITSSL_LINEAR_OPERANDS=bf16), which "
                                f"cover {ops.HD_SUPPORTED}")
        ops.attn_family(self.dh)      # an unsupported head dim is refused here, before the first kernel of the step
        if self.fp8 and T > FP8_MAX_TOKENS:
            raise L.VitsslError(f"fp8 linear operands support sequences of up to {FP8_MAX_TOKENS} tokens, got {T}: use bf16 "
                                f"operands (set_linear_operands('bf16') or VITSSL_LINEAR_OPERANDS=bf16), which cover up to "
                                f"{MAX_TOKENS} tokens")
        if T > MAX_TOKENS:
            raise L.VitsslError(f"sequence length {T} > {MAX_TOKENS} unsupported by the attention kernels")

    # what differs between the operand kinds ------------------------------------------
    # bf16: every GEMM reads bf16 images.  fp8: every GEMM reads e4m3 images, which the producer of a tensor writes next to (forward:
    # instead of) the bf16 one; the gradient images carry a per-tensor scale (_GradOperand).  The schedules below are written once
    # and go through these launches; drop path and LayerScale exist with bf16 operands only, so _scaled() is empty with fp8.
    def _scaled(self, dp, T, i, k, branch=None, dls=False):
        """Keyword arguments of the launch that emits branch k (1: attention, 2: MLP) of block i, forward or backward: rows= of the
        drop-path table `dp` (a block whose rate is 0 -- the first one of every schedule -- keeps the plain launches: its rows of
        the table are ones); cols= of LayerScale's gamma with branch= (its bf16 image: written by a saving forward, read by the
        backward) and, if `dls`, dls= (the slot of gamma's gradient)."""
        kw = {}
        if dp is not None and self.drop_path[i] > 0.0:
            kw["rows"] = (dp[2 * i + k - 1], T)
        if self.layer_scale:
            name = self._n(i, f"layer_scale{k}.gamma")
            kw["cols"] = self.store.view(name)
            if branch is not None:
                kw["branch"] = branch
            if dls:
                kw["dls"] = self.store.gview(name)
        return kw

    def _ln_fwd(self, x, i, leaf, y, mean, rstd):
        """y = the operand image of LayerNorm `leaf` of block i over x (fp8: no bf16 image, nothing reads it)"""
        gamma, beta = self.store.view(self._n(i, leaf + ".weight")), self.store.view(self._n(i, leaf + ".bias"))
        if self.fp8:
            ops.layernorm_fwd_fp8(x, gamma, beta, None, y, mean, rstd)
        else:
            ops.layernorm_fwd(x, gamma, beta, y, mean, rstd)

    def _gemm(self, A, i, leaf, out, epilogue, dgrad=False, image=None, **kw):
        """out = A @ W^T (dgrad: A @ W) of weight `leaf` of block i with the fused epilogue; `image`: the operand image of the
        epilogue's second result (EPI_GELU: out1 in bf16, or its e4m3 image; EPI_DGELU with fp8 operands: the e4m3 image of out)."""
        name = self._n(i, leaf)
        if self.fp8:
            w, alpha = (self.store.w8t if dgrad else self.store.w8)(name)
            ops.gemm_fp8_nt(A, w, out, epilogue, alpha=alpha, out_fp8=image, **kw)
        else:
            ops.gemm_nt(A, self.store.w(name + ".T" if dgrad else name), out, epilogue, out1=image, **kw)

    def _attn_fwd(self, qkv, att, att_op, lse, B, T, probs):
        if self.fp8:
            ops.attn_fwd(qkv, att, lse, B, T, self.H, self.dh, probs=probs, out_fp8=att_op)
        else:
            ops.attn_fwd_any(qkv, att, lse, B, T, self.H, self.dh, probs=probs)

    def _attn_bwd(self, s, dout, q, delta, B, T):
        """the gradient operand q = dQKV of the block saved as s"""
        if self.fp8:
            ops.attn_bwd(s["qkv"], s["att"], dout, s["lse"], q.x, delta, B, T, self.H, self.dh, dqkv_fp8=q.x8, scale=q.scale, amax=q.amax)
            self._settle(q)
        else:
            ops.attn_bwd_any(s["qkv"], s["att"], dout, s["lse"], q.x, delta, B, T, self.H, self.dh)

    def _dgrad(self, q, i, leaf, out, epilogue=L.EPI_BF16, emits=None, **kw):
        """input-gradient GEMM of weight `leaf` of block i on the gradient operand q; `emits`: the gradient operand the EPI_DGELU
        epilogue writes (out is its bf16 image)"""
        if self.fp8:
            kw["alpha2"] = q.inv
            if emits is not None:
                kw.update(image=emits.x8, out_scale=emits.scale, out_amax=emits.amax)
        self._gemm(q.x8 if self.fp8 else q.x, i, leaf, out, epilogue, dgrad=True, **kw)
        if self.fp8 and emits is not None:
            self._settle(emits)

    def _ln_bwd(self, ln, g, q, gm_colsum, drop, **scaled):
        """The producer of the masked gradient operand q: LayerNorm backward, ln = (dy, x, mean, rstd, block, leaf), adding into
        the residual gradient g in place, or (ln = None) the mask + cast of g at the top of the chain.  gm_colsum: the bias
        gradient q sums to."""
        f8 = (q.x8, q.scale, q.amax) if self.fp8 else ()
        if ln is None:
            (ops.grad_mask_cast_fp8 if self.fp8 else ops.grad_mask_cast)(g, q.x, *f8, gm_colsum, drop, **scaled)
        else:
            *head, i, leaf = ln
            w, b = self._n(i, leaf + ".weight"), self._n(i, leaf + ".bias")
            (ops.layernorm_bwd_fp8 if self.fp8 else ops.layernorm_bwd)(*head, self.store.view(w), g, g, q.x, *f8, self.store.gview(w),
                                                                       self.store.gview(b), gm_colsum, drop, **scaled)
        if self.fp8:
            self._settle(q)

    # forward ----------------------------------------------------------------
    def forward(self, x: torch.Tensor, B: int, T: int, training: bool, seed: int, save: bool, slot: str = "a",
                return_attn: bool = False):
        """x: fp32 [B*T, D] (left untouched).  Returns (x_out fp32 [B*T, D], probs or None)."""
        st, D, H, F = self.store, self.D, self.H, self.F
        self.check_tokens(T)
        M = B * T
        dev = x.device
        g = self.ws.get
        probs = None
        rec = {"B": B, "T": T, "seed": seed, "training": training, "blocks": []}
        # drop path: one table of per-sample scales for the whole call, kept with the slot for the backward
        dp = None
        if training and self.drop_path is not None:
            dp = ops.droppath_table(self.drop_path_sites(), B, seed, g(f"{slot}.dp" if save else f"{slot}.tmp.dp", (2 * self.L, B), F32, dev))
        rec["dp"] = dp
        cur = x
        for i in range(self.L):
            tag = f"{slot}.{i}." if save else f"{slot}.tmp."
            # the operand images of the block's four GEMM inputs, kept for the weight gradients: bf16, or e4m3 (one byte per element)
            img = lambda n, n8, cols: g(tag + (n8 if self.fp8 else n), (M, cols), FP8 if self.fp8 else BF16, dev)   # noqa: E731
            h1, h2, a = img("h1", "h1_8", D), img("h2", "h2_8", D), img("a", "a8", F)
            att = g(tag + "att", (M, D), BF16, dev)      # the attention backward reads the bf16 image with either kind
            att_op = img("att", "att8", D) if self.fp8 else att
            # LayerScale: both residual launches of every block take the column-scaled entry; only a saving forward writes the branches
            ls1 = g(tag + "ls1", (M, D), BF16, dev) if self.layer_scale and save else None
            ls2 = g(tag + "ls2", (M, D), BF16, dev) if self.layer_scale and save else None
            mean1, rstd1 = g(tag + "mean1", (M,), F32, dev), g(tag + "rstd1", (M,), F32, dev)
            mean2, rstd2 = g(tag + "mean2", (M,), F32, dev), g(tag + "rstd2", (M,), F32, dev)
            qkv = g(tag + "qkv", (M, 3 * D), BF16, dev)
            lse = g(tag + "lse", (B, H, T), F32, dev)
            xmid = g(tag + "xmid", (M, D), F32, dev)
            u = g(tag + "u", (M, F), BF16, dev)
            # block output: a fresh buffer per block when saving (it is the next block's
            # LN input), otherwise ping-pong
            xout = g(f"{slot}.{i}.xout" if save else f"{slot}.tmp.xout{i & 1}", (M, D), F32, dev)

            if return_attn and i == self.L - 1:
                probs = torch.empty(B, H, T, T, dtype=F32, device=dev)
            b1, b2 = st.view(self._n(i, "feed_forward.linear_in.bias")), st.view(self._n(i, "feed_forward.linear_out.bias"))
            self._ln_fwd(cur, i, "layer_norm1", h1, mean1, rstd1)
            self._gemm(h1, i, "wqkv", qkv, L.EPI_BF16)
            self._attn_fwd(qkv, att, att_op, lse, B, T, probs if i == self.L - 1 else None)
            self._gemm(att_op, i, "wo", xmid, L.EPI_RESID, aux=cur, drop=self._drop(i, 0, seed, training), **self._scaled(dp, T, i, 1, branch=ls1))
            self._ln_fwd(xmid, i, "layer_norm2", h2, mean2, rstd2)
            self._gemm(h2, i, "w1", u, L.EPI_GELU, bias=b1, image=a, drop=self._drop(i, 1, seed, training))
            self._gemm(a, i, "w2", xout, L.EPI_RESID, bias=b2, aux=xmid, drop=self._drop(i, 2, seed, training), **self._scaled(dp, T, i, 2, branch=ls2))
            if save:
                rec["blocks"].append(dict(xin=cur, h1=h1, mean1=mean1, rstd1=rstd1, qkv=qkv, att=att, att_op=att_op, lse=lse, xmid=xmid,
                                          h2=h2, mean2=mean2, rstd2=rstd2, u=u, a=a, ls1=ls1, ls2=ls2))
            cur = xout
        if save:
            self._saved[slot] = rec
        return cur, probs

    # backward ---------------------------------------------------------------
    def backward(self, g: torch.Tensor, slot: str = "a", reducer: Optional[GradReducer] = None,
                 scale_key: Optional[str] = None, input_grad_only: bool = False) -> torch.Tensor:
        """g: fp32 [M, D] gradient wrt the stack output (overwritten in place; returned
        holding the gradient wrt the stack input).  Parameter gradients are ACCUMULATED
        into the store's flat gradient buffer.  `scale_key` (fp8 operands only) names the delayed-scaling state this pass
        uses; default = the slot, i.e. one state per kind of pass (callers that merely rotate slot names over the same kind
        of pass -- vit_core._functions.StackRunner -- pass one fixed key).
        `input_grad_only` (bf16 operands; every block parameter frozen): the input-gradient chain runs as always, no
        weight-gradient GEMM is launched and no block range is handed to the reducer.  The per-column sums the chain's kernels
        write anyway (bias and LayerNorm gradients) still land in the blocks' slots of the gradient buffer; nothing applies
        them.  With fp8 operands the full schedule runs.

        With fp8 operands all eight backward GEMMs of every block run on e4m3 operands: the transposed weight images of the
        store, the activation images saved by the forward, and gradient images written by the producers of the gradients
        (LayerNorm backward, the dGELU epilogue, the attention backward's store phase)."""
        st, D, H, F = self.store, self.D, self.H, self.F
        rec = self._saved[slot]
        B, T, seed, training, dp = rec["B"], rec["T"], rec["seed"], rec["training"], rec.get("dp")
        M = B * T
        dev = g.device
        w = self.ws.get
        bw = f"bwd{M}."     # keyed by the row count: slots of different sizes (DINO local / global crops) keep their own buffers
        gv = st.gview
        last = self.L - 1
        wgrad = self.fp8 or not input_grad_only
        gs = self._grad_scale_state(dev, scale_key or slot) if self.fp8 else None
        jit = self.fp8 and not gs["valid"]
        # The four gradient operands of a block: 0 d(FFN out), 1 d(FFN hidden), 2 d(attention out), 3 dQKV.  The four weight
        # gradients of a block run as ONE launch at the end of the block's backward (ops.gemm_tn_batch: one split count and one reduce
        # pass for all their tiles instead of four rounds of the CUs with 66 MB of partial tiles each), so all four operands must be
        # alive there: the LayerNorm-2 backward writes operand 2 into a second buffer (gm2 / gm8b) instead of over operand 0.
        # fp8: the bf16 images exist only in the self-calibrating first backward (_settle re-quantises from them); afterwards
        # every consumer reads the e4m3 image and the producers skip the bf16 store.
        kinds = (("gm", "gm8", D), ("du", "du8", F), ("gm2" if wgrad and not self.fp8 else "gm", "gm8b", D), ("dqkv", "dq8", 3 * D))
        x = [w(bw + n, (M, cols), BF16, dev) if not self.fp8 or jit else None for n, _, cols in kinds]
        x8 = [w(bw + n8, (M, cols), FP8, dev) if self.fp8 else None for _, n8, cols in kinds]
        dh_ = w(bw + "dh", (M, D), BF16, dev)
        delta = w(bw + "delta", (B, H, T), F32, dev)

        plain = [_GradOperand(t) for t in x]

        def grad(i, t):
            """gradient operand t of block i: with fp8 operands every (i, t) has its own scale"""
            if not self.fp8:
                return plain[t]
            return _GradOperand(x[t], x8[t], gs["scale"][i, t:t + 1], gs["amax"][i, t:t + 1], gs["inv"][i, t:t + 1])

        def scaled(i, k):
            """_scaled() of the producer of the masked operand of branch k of block i (LayerScale: gamma's gradient needs the saved
            branch; not with frozen blocks)"""
            return self._scaled(dp, T, i, k, branch=rec["blocks"][i][f"ls{k}"] if wgrad else None, dls=wgrad)

        # top of the chain: dropout-mask + cast of g, and the last block's linear_out bias grad
        gm = grad(last, 0)
        self._ln_bwd(None, g, gm, gv(self._n(last, "feed_forward.linear_out.bias")), self._drop(last, 2, seed, training), **scaled(last, 2))
        for i in range(last, -1, -1):
            s = rec["blocks"][i]
            a_ = self.bp[i] + "self_attention."
            du, gm2, dqkv = grad(i, 1), grad(i, 2), grad(i, 3)
            # MLP
            self._dgrad(gm, i, "w2", du.x, L.EPI_DGELU, emits=du, aux=s["u"],
                        colsum=gv(self._n(i, "feed_forward.linear_in.bias")))   # s["u"] holds g' = keep*scale*gelu'(u)
            self._dgrad(du, i, "w1", dh_)
            self._ln_bwd((dh_, s["xmid"], s["mean2"], s["rstd2"], i, "layer_norm2"), g, gm2, None, self._drop(i, 0, seed, training),
                         **scaled(i, 1))
            # attention
            self._dgrad(gm2, i, "wo", dh_)
            self._attn_bwd(s, dh_, dqkv, delta, B, T)
            self._dgrad(dqkv, i, "wqkv", dh_)
            if wgrad:      # before the LayerNorm-1 backward below overwrites operand 0 for the next block
                jobs = [(gm, s["a"], gv(self._n(i, "feed_forward.linear_out.weight"), (D, F))),
                        (du, s["h2"], gv(self._n(i, "feed_forward.linear_in.weight"), (F, D))),
                        (gm2, s["att_op"], gv(a_ + "final_linear.weight", (D, D))),
                        (dqkv, s["h1"], st.span_view(a_ + "w_query.weight", a_ + "w_value.weight", (3 * D, D), grad=True))]
                if self.fp8:
                    ops.gemm_fp8_tn_batch([(q.x8, act, dw, None, q.inv) for q, act, dw in jobs])
                else:
                    ops.gemm_tn_batch([(q.x, act, dw) for q, act, dw in jobs])
            ln1 = (dh_, s["xin"], s["mean1"], s["rstd1"])
            if i > 0:
                gm = grad(i - 1, 0)
                self._ln_bwd(ln1 + (i, "layer_norm1"), g, gm, gv(self._n(i - 1, "feed_forward.linear_out.bias")),
                             self._drop(i - 1, 2, seed, training), **scaled(i - 1, 2))
            else:      # nothing reads a masked operand below the first block: the plain launch with either kind
                ops.layernorm_bwd(*ln1, st.view(self._n(i, "layer_norm1.weight")), g, g, None,
                                  gv(self._n(i, "layer_norm1.weight")), gv(self._n(i, "layer_norm1.bias")), None, ops.NO_DROP)
            if reducer is not None and wgrad:
                # every gradient of block i is final, except linear_out.bias of block i-1,
                # which belongs to the next (lower) range.  (LayerScale: layer_scale1.gamma of block i came from this block's
                # LayerNorm-2 backward, layer_scale2.gamma of block i from the LayerNorm-1 backward of block i + 1 -- or from the
                # top grad_mask_cast -- before that block's range was handed over; the launch just above wrote layer_scale2.gamma
                # of block i - 1, which like its linear_out.bias belongs to the next range.)
                lo, hi = self.block_span(i)
                reducer.ready(lo, hi)
        if self.fp8:
            # scales of the NEXT backward: this step's max |value| with one bit of headroom
            gs["used"].copy_(gs["scale"])
            self._rescale(gs["scale"], gs["inv"], gs["amax"], margin=1)
            gs["amax"].zero_()
            gs["valid"] = True
        return g

    # fp8 gradient operands: delayed scaling ------------------------------------------
    @staticmethod
    def _scale_from_amax(amax: torch.Tensor, margin: int) -> torch.Tensor:
        """2^(floor(log2(448 / amax)) - margin) on the binary representation (the rule of csrc/fp8.hip)."""
        mant, e = torch.frexp(amax)                     # amax = mant * 2^e, mant in [0.5, 1)
        k = (9 - e - (mant > 0.875).to(e.dtype) - margin).clamp(-120, 120)
        # an exact power of two from its exponent field (torch.ldexp multiplies by pow(2, k), which is not exact on the GPU)
        return torch.bitwise_left_shift(k.to(torch.int32) + 127, 23).view(torch.float32)

    def _grad_scale_state(self, dev, slot: str = "a"):
        gs = self._gs_by_slot.get(slot)
        if gs is None or gs["scale"].device != dev:
            mk = lambda v: torch.full((self.L, 4), v, dtype=F32, device=dev)  # noqa: E731
            gs = {"scale": mk(1.0), "inv": mk(1.0), "amax": mk(0.0), "used": mk(1.0), "valid": False}
            self._gs_by_slot[slot] = gs
        self._gs = gs
        return gs

    def _rescale(self, scale, inv, amax, margin: int):
        """scale / inv (views of the slot's state) from the recorded max |value| (left alone where that is 0 or not finite)."""
        ok = (amax > 0) & torch.isfinite(amax)
        new = torch.where(ok, self._scale_from_amax(torch.where(ok, amax, torch.ones_like(amax)), margin), scale)
        scale.copy_(new)
        inv.copy_(1.0 / new)

    def _settle(self, q):
        """first fp8 backward of a slot only (q has both images): the producer of q has just recorded max |q|; take the scale from
        it and quantise again"""
        if q.x is not None and q.x8 is not None:
            self._rescale(q.scale, q.inv, q.amax, margin=0)
            ops.quantize_fp8(q.x, q.x8, scale=q.scale)

    def fp8_grad_scales(self, slot: Optional[str] = None) -> torch.Tensor:
        """[L, 4] scales the last backward (of `slot`, default: whichever ran last) quantised its gradient operands with
        (tests hand them to the oracle)."""
        gs = self._gs if slot is None else self._gs_by_slot[slot]
        return gs["used"].clone()

    def recalibrate_fp8(self):
        """Derive the gradient scales from the tensors themselves in the next backward of every slot (as the first one does)."""
        for gs in self._gs_by_slot.values():
            gs["valid"] = False
