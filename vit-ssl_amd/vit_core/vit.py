"""Supervised ViT (reference: vit_core/vit.py:9-45): ConvolutionalPatchEmbedding ->
encoder blocks -> CLS token (or, with global_pool="avg", the mean of the patch tokens) -> MLPHead, run as one engine schedule
on a flat store.

Two ways to train, as for SimMIMViT:
  * reference style: ``loss = criterion(model(x), y); loss.backward()`` (one torch.autograd.Function around the engine);
  * fused: ``loss = model.train_step(x, y, optimizer, reducer)`` -- cross-entropy (csrc/classify.hip), backward into the flat
    gradient buffer, overlapped all-reduce and flat AdamW with no autograd graph; ``model.eval_step(x, y)`` is its no-grad
    half.  The backward does only what the parameters' `requires_grad` asks for (`_ViTRuntime.schedule`).
Both run the one classification head of `_ViTRuntime` (`forward` / `loss` / `backward`: workspace buffers, GEMM operands cached
on the store's `weights_key()`); `_ViTFn` only slices and copies the logits out and pads the incoming gradient.  The runtime keeps
the activations of ONE saving forward, whichever path made it: a backward through an older graph raises VitsslError."""
from typing import Optional

import torch
from torch import nn
from torch.autograd import Function

from . import _runtime as R
from ._runtime import BF16, F32, L, _round_up, ops
from ._backbone import POOLS, BackboneRuntime
from .encoder_block import EncoderBlock, check_layer_scale_init
from .mlp_head import MLPHead
from .patch_embedding import ConvolutionalPatchEmbedding


class _ViTRuntime:
    def __init__(self, model: "ViT", device):
        self.model, self.device = model, device
        C, Hh, Ww = model.input_shape
        P = model.patch_size
        self.store = R.FlatStore(model, device)
        st = self.store
        self.D = model.embed_dim
        self.bb = BackboneRuntime(
            st, "", dict(weight="patch_embedding.conv.weight", bias="patch_embedding.conv.bias",
                         cls="patch_embedding.cls_token", pos="patch_embedding.positional_embedding"),
            len(model.encoder_blocks), C, P, (Hh // P, Ww // P), self.D, model.num_heads, model.mlp_dim, model.dropout_p,
            drop_path=R.drop_path_rates(model.drop_path_rate, len(model.encoder_blocks)),
            layer_scale=model.layer_scale_init is not None)
        self.ncls = model.num_classes
        self.rec = None                   # what the last saving forward keeps of the head for its backward
        self.save_gen = 0                 # id of that forward
        self.ws = R.Workspace()
        self._head = None                 # cached GEMM operands of the classifier (head_operands)
        self._head_key = None
        self.counters = torch.zeros(2, dtype=torch.int64, device=device)      # (correct, valid) when the caller brings none
        self.bad_labels = torch.zeros(1, dtype=torch.int32, device=device)    # labels outside [0, C) seen so far

    def valid_for(self, device):
        return device == self.device and self.store.is_attached()

    def schedule(self) -> str:
        """Which backward the parameters' requires_grad asks for (read at every call; about 150 flags):
        "full": an encoder-block parameter trains -- every gradient (what the autograd path always runs);
        "input_grad": the blocks are frozen and something below them trains (utils.model_builder.freeze_backbone leaves the
            CLS token trainable) -- the input-gradient chain without the blocks' weight-gradient GEMMs (bf16 operands; with
            fp8 operands this case runs the full schedule);
        "head": nothing below the classification head trains -- the backbone forward saves nothing and the backward ends
            after the head's LayerNorm."""
        blocks = below = False
        for n, p in zip(self.store.names, self.store.params):
            if not p.requires_grad:
                continue
            if n.startswith("encoder_blocks."):
                blocks = True
                break
            below = below or n.startswith("patch_embedding.")
        if blocks or (below and self.bb.stack.fp8):
            return "full"
        return "input_grad" if below else "head"

    def reduce_ranges(self):
        """The ranges of the flat gradient buffer one fused backward hands to a GradReducer in the current frozen state:
        None = the whole buffer (full schedule), else the list for GradReducer(expect=...)."""
        sched, st = self.schedule(), self.store
        if sched == "full":
            return None
        head = st.prefix_span("classification_head.")
        return [head] if sched == "head" else [st.prefix_span("patch_embedding."), head]

    def head_operands(self):
        """(bf16 classifier weight [Nk, D] zero-padded to the GEMM granule, its transpose [D, Nk], padded fp32 bias [Nk], Nk),
        rebuilt only when the store's weights_key() has changed."""
        st, D, C = self.store, self.D, self.ncls
        key = st.weights_key()
        if self._head is None:
            Nk = _round_up(C, 64)
            self._head = dict(w32=torch.zeros(Nk, D, dtype=F32, device=self.device), wb=torch.empty(Nk, D, dtype=BF16, device=self.device),
                              wt=torch.empty(D, Nk, dtype=BF16, device=self.device), bias=torch.zeros(Nk, dtype=F32, device=self.device), Nk=Nk)
            self._head_key = None
        hd = self._head
        if key != self._head_key:
            hd["w32"][:C].copy_(st.view("classification_head.linear.weight", (C, D)))
            hd["bias"][:C].copy_(st.view("classification_head.linear.bias"))
            ops.cast_transpose_bf16(hd["w32"], hd["wb"], hd["wt"])
            self._head_key = key
        return hd["wb"], hd["wt"], hd["bias"], hd["Nk"]

    def forward(self, x, training, save, save_backbone=None, return_attn=False):
        """-> (padded logits f32 [B, Nk] in a workspace buffer, attention probabilities or None).  A saving forward keeps the
        head's tensors in `rec` (and the backbone's unless `save_backbone` is False: the "head" schedule) and takes a new
        `save_gen`; one that saves nothing (no_grad, eval_step) leaves the buffers of a pending backward alone."""
        st, g = self.store, self.ws.get
        tag = "head." if save else "head.tmp."
        st.refresh_weights()
        seed = R.next_seed() if self.bb.stack.needs_seed(training) else 0
        feats, probs = self.bb.forward(x, training, seed, save=save if save_backbone is None else save_backbone, slot="a",
                                       return_attn=return_attn, pool=self.model.global_pool)
        B, dev = feats.shape[0], feats.device
        h = g(tag + "h", (B, self.D), BF16, dev)
        mean, rstd = g(tag + "mean", (B,), F32, dev), g(tag + "rstd", (B,), F32, dev)
        ops.layernorm_fwd(feats, st.view("classification_head.norm.weight"), st.view("classification_head.norm.bias"), h, mean, rstd)
        wb, wt, bias, Nk = self.head_operands()
        logits = g(tag + "logits", (B, Nk), F32, dev)
        ops.gemm_nt(h, wb, logits, L.EPI_F32, bias=bias)
        if save:
            self.save_gen += 1
            self.rec = dict(feats=feats, h=h, mean=mean, rstd=rstd, wt=wt, Nk=Nk, B=B)
        return logits, probs

    def loss(self, logits, labels, tag, label_smoothing, ignore_index, counters, dlogits=None, dbias=None, mix=None, bce=None):
        """csrc/classify.hip on the padded logits -> (loss as a device scalar, pred i64 [B]).  `mix` (data.MixParams): against
        the two-label targets of a mixed batch.  `bce` ((target_threshold, sum_classes), from `loss_spec`): binary cross-entropy
        (vitssl_classify_bce, one- or two-label) instead of softmax cross-entropy."""
        B, dev = logits.shape[0], logits.device
        if labels.dtype != torch.int64 or not labels.is_contiguous():
            labels = labels.to(torch.int64).contiguous()
        loss_out = self.ws.get(tag + "loss_out", (2,), F32, dev)
        pred = self.ws.get(tag + "pred", (B,), torch.int64, dev)
        counters = self.counters if counters is None else counters
        if bce is not None:
            ops.classify_bce(logits, labels, self.ncls, loss_out, pred, counters, self.bad_labels,
                             partner=None if mix is None else mix.partner, lam=None if mix is None else mix.lam, dlogits=dlogits,
                             dbias=dbias, smoothing=label_smoothing, target_threshold=bce[0], sum_classes=bce[1], ignore_index=ignore_index)
        elif mix is None:
            ops.classify_loss(logits, labels, self.ncls, loss_out, pred, counters, self.bad_labels,
                              dlogits=dlogits, dbias=dbias, label_smoothing=label_smoothing, ignore_index=ignore_index)
        else:
            ops.classify_loss_mix(logits, labels, mix.partner, mix.lam, self.ncls, loss_out, pred, counters, self.bad_labels,
                                  dlogits=dlogits, dbias=dbias, label_smoothing=label_smoothing, ignore_index=ignore_index)
        return loss_out[0] / loss_out[1], pred         # 0 / 0 = nan when every row is ignored, as torch gives

    def backward(self, dlb, sched, reducer=None):
        """dlb: bf16 [B, Nk], the gradient of the padded logits; the classifier's bias gradient is the caller's (the loss
        kernel accumulates it)."""
        st, g, rec = self.store, self.ws.get, self.rec
        B, Nk, C, D = rec["B"], rec["Nk"], self.ncls, self.D
        dev = dlb.device
        gv = st.gview
        dw = g("head.dw", (Nk, D), F32, dev)
        dw.zero_()
        ops.gemm_tn(dlb, rec["h"], dw)
        gv("classification_head.linear.weight", (C, D)).add_(dw[:C])
        dh = g("head.dh", (B, D), BF16, dev)
        ops.gemm_nt(dlb, rec["wt"], dh, L.EPI_BF16)
        dfeats = g("head.dfeats", (B, D), F32, dev)
        ops.layernorm_bwd(dh, rec["feats"], rec["mean"], rec["rstd"], st.view("classification_head.norm.weight"), None, dfeats,
                          None, gv("classification_head.norm.weight"), gv("classification_head.norm.bias"))
        if reducer is not None:
            reducer.ready(*st.prefix_span("classification_head."))
        if sched == "head":
            return
        proj = sched == "full" or self.model.patch_embedding.conv.weight.requires_grad
        self.bb.backward(dfeats, "a", reducer, input_grad_only=sched == "input_grad", proj_wgrad=proj)
        if reducer is not None:
            reducer.ready(*st.prefix_span("patch_embedding."))


class _ViTFn(Function):
    """The autograd path: a thin adapter over the runtime's one head forward / backward."""

    @staticmethod
    def forward(ctx, rt, x, training, return_attn, need, *params):
        logits, probs = rt.forward(x, training, save=need, return_attn=return_attn)
        ctx.rt, ctx.gen = rt, rt.save_gen
        if return_attn:
            ctx.mark_non_differentiable(probs)
        return logits[:, :rt.ncls].clone(), probs        # a copy: the workspace buffer belongs to the next forward

    @staticmethod
    def backward(ctx, dlogits, _dp):
        rt = ctx.rt
        st, C = rt.store, rt.ncls

        def run():
            dl = torch.zeros(dlogits.shape[0], rt.rec["Nk"], dtype=F32, device=dlogits.device)
            dl[:, :C] = R.as_f32(dlogits)
            dlb = torch.empty(dl.shape, dtype=BF16, device=dl.device)
            ops.cast_bf16(dl, dlb)
            st.gview("classification_head.linear.bias").add_(dl[:, :C].sum(0))
            rt.backward(dlb, "full")

        return (None, None, None, None, None, *R.backward_grads("ViT", ctx.gen, rt.save_gen, st, run))


def loss_spec(loss, target_threshold, sum_classes):
    """The `loss`, `target_threshold` and `sum_classes` keywords of train_step / eval_step -> what `_ViTRuntime.loss` takes as
    `bce`: None for "ce" (nothing new is launched), (target_threshold, sum_classes) for "bce"."""
    if loss == "ce":
        if target_threshold is not None or sum_classes:
            raise ValueError('ViT: target_threshold and sum_classes belong to loss="bce"; loss="ce" takes neither')
        return None
    if loss != "bce":
        raise ValueError(f'ViT: loss = {loss!r} is neither "ce" (softmax cross-entropy) nor "bce" (binary cross-entropy)')
    if target_threshold is not None and not float(target_threshold) >= 0.0:
        raise ValueError(f"ViT: target_threshold = {target_threshold!r} must be None or a number >= 0")
    return (None if target_threshold is None else float(target_threshold), bool(sum_classes))


class ViT(nn.Module):
    def __init__(
        self,
        num_classes: int,
        num_blocks: int,
        input_shape,
        embed_dim: int,
        patch_size: int,
        num_heads: int = 8,
        mlp_dim: int = 3072,
        dropout: float = 0.1,
        *,
        global_pool: str = "cls",
        layer_scale_init: Optional[float] = None,
        drop_path_rate: float = 0.0,
    ):
        super().__init__()
        # what the head reads (timm's global_pool): "cls" = the CLS token, "avg" = the mean of the patch tokens (the MAE
        # fine-tune recipe; classification_head.norm is then its fc_norm).  Not a parameter, buffer or state_dict key
        if global_pool not in POOLS:
            raise ValueError(f'ViT: global_pool = {global_pool!r} is neither "cls" nor "avg"')
        self.global_pool = global_pool
        # LayerScale (timm's init_values): None = no new parameter, key or launch; else a finite float > 0 (ValueError otherwise)
        self.layer_scale_init = check_layer_scale_init(layer_scale_init)
        self.encoder_blocks = nn.ModuleList(
            [EncoderBlock(embed_dim, num_heads, mlp_dim, dropout, layer_scale_init=self.layer_scale_init) for _ in range(num_blocks)]
        )
        self.patch_embedding = ConvolutionalPatchEmbedding(input_shape, embed_dim, patch_size)
        self.classification_head = MLPHead(embed_dim, num_classes)
        self.input_shape = tuple(input_shape)
        self.num_classes, self.embed_dim, self.patch_size = num_classes, embed_dim, patch_size
        self.num_heads, self.mlp_dim, self.dropout_p = num_heads, mlp_dim, float(dropout)
        # stochastic depth (timm's drop_path_rate): block i drops a sample from each residual branch with probability
        # rate * i / (num_blocks - 1) while training; not a parameter
        self.drop_path_rate = float(drop_path_rate)
        R.drop_path_rates(self.drop_path_rate, num_blocks)        # a rate outside [0, 1) is a ValueError here
        self._rt = None

    def runtime(self, device=None) -> _ViTRuntime:
        return R.model_runtime(self, "ViT", _ViTRuntime, self.patch_embedding.cls_token, device)

    def flat_store(self):
        return self.runtime().store

    def forward(self, x: torch.Tensor, return_attn=False):
        R.require_gpu(x, "ViT")
        rt = self.runtime(x.device)
        need = torch.is_grad_enabled() and any(p.requires_grad for p in rt.store.params)
        logits, probs = _ViTFn.apply(rt, x, self.training, return_attn, need, *rt.store.params)
        if return_attn:
            return logits, probs
        return logits

    # ------------------------------------------------------------------ fused step
    def reduce_ranges(self):
        """`expect` of the GradReducer that fits the model's current frozen state (None: the whole gradient buffer)."""
        return self.runtime().reduce_ranges()

    def check_labels(self):
        """Raise if a fused step has seen a label outside [0, num_classes) that was not the ignore_index (the kernel treats
        such a row as ignored and counts it on the device).  One host read: call it once per epoch."""
        rt = self.runtime()
        n = int(rt.bad_labels.item())
        if n:
            rt.bad_labels.zero_()
            raise L.VitsslError(f"ViT: {n} label(s) outside [0, {self.num_classes}) reached train_step / eval_step; their rows were ignored")

    def train_step(self, x: torch.Tensor, labels: torch.Tensor, optimizer, reducer=None, label_smoothing: float = 0.0,
                   ignore_index: int = -100, counters=None, mix=None, loss: str = "ce", target_threshold=None,
                   sum_classes: bool = False) -> torch.Tensor:
        """One full optimisation step (zero_grad -> forward -> CrossEntropyLoss(mean, label_smoothing, ignore_index) ->
        backward -> gradient all-reduce -> AdamW) with no autograd graph; returns the loss as a device scalar (no host sync).
        Equivalent to utils/trainers/supervised_trainer.py:33-40 of the reference.  Leaves `last_logits` ([B, C] view of the
        padded GEMM output) and `last_pred` (i64 [B]) on the model; `counters` (i64 [2] on the device, default: the
        runtime's own) accumulates (correct, valid) rows.
        `mix` (data.MixParams, from data.GPUMixup.draw): Mixup / CutMix.  The batch is mixed into a workspace buffer
        (vitssl_mix_batch) and the loss is taken against the two-label targets lam s(y[i]) + (1 - lam) s(y[partner])
        (vitssl_classify_loss_mix); a row of an invalid table counts as a bad label (`check_labels`).  The counters then
        compare the prediction with the row's own label.  Without `mix` nothing of this is launched.
        `loss="bce"`: binary cross-entropy (timm's BinaryCrossEntropy, the DeiT III loss; utils.losses.BinaryCrossEntropy is
        its torch module) instead of softmax cross-entropy, in one launch of vitssl_classify_bce: a sigmoid per class against
        the targets smoothed by `label_smoothing` (with `mix`: the two-label targets), set to (t > target_threshold) when a
        threshold is given; a row's loss is the mean over its classes, their sum with `sum_classes`.  With "ce" (the default)
        nothing of this is launched; any other value is a ValueError."""
        R.require_gpu(x, "ViT.train_step")
        bce = loss_spec(loss, target_threshold, sum_classes)
        rt = self.runtime(x.device)
        st = rt.store
        with R.fused_step(self, st, optimizer, reducer) as apply:
            sched = rt.schedule()
            if sched == "head":                        # nothing below the head trains: no activations are kept
                rt.bb.forget("a")
            if mix is not None:
                mixed = rt.ws.get("mix.x", tuple(x.shape), F32, x.device)
                ops.mix_batch(R.as_f32(x), mixed, mix.iparams, mix.lam)
                x = mixed
            logits, _ = rt.forward(x, True, save=True, save_backbone=sched != "head")
            dlb = rt.ws.get("head.dlogits", tuple(logits.shape), BF16, x.device)
            value, pred = rt.loss(logits, labels, "head.", label_smoothing, ignore_index, counters, dlogits=dlb,
                                  dbias=st.gview("classification_head.linear.bias"), mix=mix, bce=bce)
            rt.backward(dlb, sched, reducer)
            apply()
            self.last_logits, self.last_pred = logits[:, :self.num_classes], pred
            return value

    @torch.no_grad()
    def eval_step(self, x: torch.Tensor, labels: torch.Tensor, label_smoothing: float = 0.0, ignore_index: int = -100,
                  counters=None, loss: str = "ce", target_threshold=None, sum_classes: bool = False) -> torch.Tensor:
        """The no-grad half of train_step: forward in eval mode (no dropout) and the loss kernel without a gradient.  Saves
        nothing and leaves the buffers of a pending backward alone; same `last_logits`, `last_pred` and counters; `loss`,
        `target_threshold` and `sum_classes` as there."""
        R.require_gpu(x, "ViT.eval_step")
        bce = loss_spec(loss, target_threshold, sum_classes)
        rt = self.runtime(x.device)
        logits, _ = rt.forward(x, False, save=False)
        value, pred = rt.loss(logits, labels, "head.tmp.", label_smoothing, ignore_index, counters, bce=bce)
        self.last_logits, self.last_pred = logits[:, :self.num_classes], pred
        return value
