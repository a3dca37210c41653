"""SimMIMViT on the MI355X HIP engine (reference: vit_core/ssl/simmim/model.py:8-93).

Same constructor, forward signature, returns and state_dict keys as the reference.
Per step: patch gather (bf16) -> projection GEMM whose epilogue substitutes the mask
token and adds the positional embedding -> L fused encoder blocks -> masked-row gather
-> reconstruction-head GEMM.  Targets are gathered straight from the image in fp32
(bit-exact with ``patches[bool_mask]``).

Two ways to train:
  * reference style: ``pred, tgt = model(x); loss = criterion(pred, tgt); loss.backward()``
    (one torch.autograd.Function around the whole engine), any torch optimizer;
  * fused: ``loss = model.train_step(x, optimizer, reducer)`` -- L1 loss, backward,
    overlapped RCCL gradient all-reduce and flat AdamW with no autograd graph at all
    (what utils.trainers.SimMIMTrainer and bench.py use).
"""
from typing import Optional

import torch
from torch import nn
from torch.autograd import Function

from ... import _runtime as R
from ..._runtime import BF16, F32, L, ops
from ...encoder_block import EncoderBlock, check_layer_scale_init
from .masking import draw_mask, mask_indices_np


class _SimMIMRuntime:
    """Flat store + encoder stack + step workspaces of one SimMIMViT on one device."""

    def __init__(self, model: "SimMIMViT", device):
        self.model = model
        self.device = device
        C, H, W = model.input_shape
        self.P = model.patch_size
        self.C, self.H, self.W = C, H, W
        self.N = (H // self.P) * (W // self.P)
        self.geo = R.PatchGeometry(C, self.P)     # widths of the patch path (padded inside the engine where the GEMMs need it)
        self.Pd, self.Pdp, self.Np = self.geo.Pd, self.geo.Pdp, self.geo.Np
        self.D = model.embed_dim
        self.store = R.FlatStore(model, device)
        st = self.store
        prefixes = [f"encoder_blocks.{i}." for i in range(len(model.encoder_blocks))]
        self.stack = R.EncoderStack(st, prefixes, self.D, model.num_heads, model.mlp_dim, model.dropout_p,
                                    drop_path=R.drop_path_rates(model.drop_path_rate, len(prefixes)),
                                    layer_scale=model.layer_scale_init is not None)
        self.ws = R.Workspace()
        self.geo.register_proj(st, "proj", lambda: st.view("projection.weight", (self.D, self.Pd)), self.D)
        self.head = R.PatchHead(st, self.geo, "head", "simmim_head.weight", "simmim_head.bias", self.D, self.ws)
        self.stage = R.HostStage()
        self.rec = None
        self.save_gen = 0      # id of the forward whose activations `rec` / the stack hold

    def valid_for(self, device) -> bool:
        return device == self.device and self.store.is_attached()

    # ------------------------------------------------------------------ forward
    def embed(self, x, mask_d, tag=""):
        """image -> encoder input tokens fp32 [B*N, D] (also leaves bf16 patches in ws).
        `tag` separates the buffers of forwards that save nothing from those a pending backward
        still needs."""
        st, ws = self.store, self.ws
        B = x.shape[0]
        M = B * self.N
        patches = ws.get(tag + "patches", (M, self.Pdp), BF16, x.device)
        self.geo.patchify(x, patches)
        x0 = ws.get(tag + "x0", (M, self.D), F32, x.device)
        ops.gemm_nt(patches, st.w("proj"), x0, L.EPI_EMBED, bias=st.view("projection.bias"),
                    embed=(mask_d, st.view("mask_token") if mask_d is not None else None,
                           st.view("positional_embedding", (self.N, self.D)), self.N, self.N, 0))
        return x0, patches

    def prepare_mask(self, mask_cpu, dev):
        """Host mask -> (idx, inv, mask_u8) device tensors, staged as one copy through the runtime's ring of pinned buffers
        (engine.HostStage: they stay valid until the fourth later call)."""
        return tuple(self.stage.upload(mask_indices_np(mask_cpu.contiguous()), dev))

    def forward(self, x, training: bool, save: bool, mask_cpu=None, prepared=None):
        st, ws = self.store, self.ws
        if x.dim() != 4 or tuple(x.shape[1:]) != (self.C, self.H, self.W):
            raise L.VitsslError(f"SimMIMViT: expected input [B,{self.C},{self.H},{self.W}], got {tuple(x.shape)}")
        self.stack.check_tokens(self.N)
        x = R.as_f32(x)
        B = x.shape[0]
        M = B * self.N
        st.refresh_weights()
        dev = x.device
        if prepared is None:
            if mask_cpu is None:
                mask_cpu = draw_mask(B, self.N, self.model.mask_ratio)      # host RNG first (reference order)
            prepared = self.prepare_mask(mask_cpu, dev)
        seed = R.next_seed() if self.stack.needs_seed(training) else 0
        idx_d, inv_d, mask_d = prepared
        Mm = idx_d.numel()

        targets = torch.empty(Mm, self.Pd, dtype=F32, device=dev)
        if Mm == 0:
            # int(N * mask_ratio) == 0 (a single token, or ratio 0): the reference indexes with an all-false mask and returns
            # empty pred / targets (simmim/model.py:56-62); nothing observable depends on the encoder then
            if save:
                self.save_gen += 1
                self.rec = dict(B=B, M=M, Mm=0)
            return torch.empty(0, self.Pd, dtype=F32, device=dev), targets, mask_d.view(B, self.N, 1).bool()
        self.geo.gather_targets(x, idx_d, targets)
        tag = "" if save else "tmp."
        x0, patches = self.embed(x, mask_d, tag)
        xL, _ = self.stack.forward(x0, B, self.N, training, seed, save=save, slot="a")
        sel = ws.get(tag + "sel", (Mm, self.D), BF16, dev)
        ops.gather_rows_bf16(xL, idx_d, sel)
        pred = self.head.forward(sel)
        if save:
            self.save_gen += 1
            self.rec = dict(B=B, M=M, Mm=Mm, idx=idx_d, inv=inv_d, mask=mask_d, patches=patches, sel=sel)
        return pred, targets, mask_d.view(B, self.N, 1).bool()

    # ------------------------------------------------------------------ backward
    def backward(self, dpred_bf16, reducer=None):
        """dpred_bf16: bf16 [Mm, Pdp] (Pdp = Pd unless the geometry is padded; pad columns zero).  Accumulates every parameter
        gradient into the store's flat gradient buffer (caller zeroes it)."""
        st, ws, rec = self.store, self.ws, self.rec
        B, M, Mm = rec["B"], rec["M"], rec["Mm"]
        if Mm == 0:                                      # empty prediction: every gradient is zero (the buffer already is)
            if reducer is not None:
                reducer.ready(0, st.gflat.numel())
            return
        dev = dpred_bf16.device
        gv = st.gview
        self.head.wgrad(dpred_bf16, rec["sel"])
        dsel = ws.get("dsel", (Mm, self.D), BF16, dev)
        self.head.dgrad(dpred_bf16, dsel)
        g = ws.get("g", (M, self.D), F32, dev)
        ops.scatter_rows_f32(dsel, rec["inv"], g)
        if reducer is not None:
            reducer.ready(*st.span("simmim_head.weight", "simmim_head.bias"))
        g = self.stack.backward(g, slot="a", reducer=reducer)
        dproj = ws.get("dproj", (M, self.D), BF16, dev)
        ops.embed_bwd(g, rec["mask"], dproj, gv("positional_embedding", (self.N, self.D)), gv("mask_token"),
                      gv("projection.bias"), None, B, self.N, 0, self.D)
        self.geo.proj_wgrad(dproj, rec["patches"], gv("projection.weight", (self.D, self.Pd)), ws)
        if reducer is not None:
            reducer.ready(*st.span("mask_token", "positional_embedding"))
            reducer.ready(*st.span("projection.weight", "projection.bias"))


class _SimMIMFn(Function):
    @staticmethod
    def forward(ctx, rt, x, training, need, *params):
        pred, targets, mask = rt.forward(x, training, save=need)
        ctx.rt, ctx.gen = rt, rt.save_gen
        ctx.mark_non_differentiable(targets, mask)
        return pred, targets, mask

    @staticmethod
    def backward(ctx, dpred, _dt, _dm):
        rt = ctx.rt
        return (None, None, None, None, *R.backward_grads("SimMIMViT", ctx.gen, rt.save_gen, rt.store,
                                                          lambda: rt.backward(rt.geo.widen_grad(dpred))))      # the engine reads the padded width


class SimMIMViT(nn.Module):
    def __init__(
        self,
        num_blocks: int,
        input_shape,
        embed_dim: int,
        patch_size: int,
        num_heads: int = 8,
        mlp_dim: int = 3072,
        dropout: float = 0.1,
        mask_ratio: float = 0.6,
        *,
        layer_scale_init: Optional[float] = None,
        drop_path_rate: float = 0.0,
    ):
        super().__init__()
        self.layer_scale_init = check_layer_scale_init(layer_scale_init)      # LayerScale: None = none of it; else a finite float > 0
        self.encoder_blocks = nn.ModuleList(
            [EncoderBlock(embed_dim, num_heads, mlp_dim, dropout, layer_scale_init=self.layer_scale_init) for _ in range(num_blocks)]
        )
        self.unfold = nn.Unfold(kernel_size=(patch_size, patch_size), stride=patch_size)
        self.projection = nn.Linear((input_shape[0] * patch_size * patch_size), embed_dim)
        self.mask_token = nn.Parameter(torch.randn(1, 1, embed_dim))
        self.positional_embedding = nn.Parameter(torch.rand(1, (input_shape[1] // patch_size) ** 2, embed_dim))
        self.simmim_head = nn.Linear(embed_dim, input_shape[0] * patch_size * patch_size)

        self.mask_ratio = mask_ratio
        self.input_shape = tuple(input_shape)
        self.embed_dim, self.patch_size = embed_dim, patch_size
        self.num_heads, self.mlp_dim, self.dropout_p = num_heads, mlp_dim, float(dropout)
        self.drop_path_rate = float(drop_path_rate)               # stochastic depth, linspace(0, rate, num_blocks); not a parameter
        R.drop_path_rates(self.drop_path_rate, num_blocks)        # a rate outside [0, 1) is a ValueError here
        if input_shape[1] % patch_size != 0 or input_shape[2] % patch_size != 0:
            raise ValueError(
                f"Image dimensions H={input_shape[1]}, W={input_shape[2]} must be divisible by patch_size={patch_size}")
        self._rt = None

    # ------------------------------------------------------------------ runtime
    def runtime(self, device=None) -> _SimMIMRuntime:
        return R.model_runtime(self, "SimMIMViT", _SimMIMRuntime, self.mask_token, device)

    def flat_store(self):
        return self.runtime().store

    # ------------------------------------------------------------------ reference API
    def forward(self, x: torch.Tensor, return_bool_mask=False):
        R.require_gpu(x, "SimMIMViT")
        rt = self.runtime(x.device)
        need = torch.is_grad_enabled() and any(p.requires_grad for p in rt.store.params)
        pred, targets, mask = _SimMIMFn.apply(rt, x, self.training, need, *rt.store.params)
        if return_bool_mask:
            return pred, targets, mask
        return pred, targets

    @torch.no_grad()
    def inference_forward(self, x: torch.Tensor, return_patch_features=False):
        """Unmasked encode; mean-pooled [B, D] or all tokens [B, N, D]
        (reference: ssl/simmim/model.py:65-93; switches the module to eval like it)."""
        self.eval()
        R.require_gpu(x, "SimMIMViT")
        rt = self.runtime(x.device)
        rt.stack.check_tokens(rt.N)
        rt.store.refresh_weights()
        x = R.as_f32(x)
        B = x.shape[0]
        x0, _ = rt.embed(x, None, "inf.")
        xL, _ = rt.stack.forward(x0, B, rt.N, False, 0, save=False, slot="inf")
        feats = xL.view(B, rt.N, rt.D)
        return feats.clone() if return_patch_features else feats.mean(dim=1)

    # ------------------------------------------------------------------ fused step
    def train_step(self, x: torch.Tensor, optimizer, reducer=None, mask_cpu=None, prepared=None) -> torch.Tensor:
        """One full optimisation step (zero_grad -> forward -> L1(mean) -> backward ->
        gradient all-reduce -> AdamW) with no autograd graph; returns the loss as a
        device scalar (no host sync).  Equivalent to utils/trainers/simmim_trainer.py:61-76
        of the reference with criterion nn.L1Loss(mean)."""
        R.require_gpu(x, "SimMIMViT.train_step")
        rt = self.runtime(x.device)
        with R.fused_step(self, rt.store, optimizer, reducer) as apply:
            pred, targets, _ = rt.forward(x, True, save=True, mask_cpu=mask_cpu, prepared=prepared)
            n = pred.numel()
            loss_sum = rt.ws.get("loss_sum", (1,), F32, x.device)
            loss_sum.zero_()
            if n == 0:
                # no masked token: the reference's L1Loss(mean) of an empty prediction is nan, every gradient zero, and the
                # optimizer still steps (weight decay only)
                loss_sum.fill_(float("nan"))
                n = 1
                rt.backward(pred, reducer)
            else:
                dpb = rt.ws.get("dpred", (pred.shape[0], rt.Pdp), BF16, x.device)
                rt.geo.l1_loss(pred, targets, loss_sum, dpb, gscale=1.0 / n)
                rt.backward(dpb, reducer)
            apply()
            self.last_pred, self.last_targets = pred, targets
            return loss_sum[0] / n
