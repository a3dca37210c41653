"""MAEViT: masked-autoencoder pre-training (He et al., "Masked Autoencoders Are Scalable Vision Learners") on the MI355X HIP
engine.  The encoder sees only the K visible patches of each image (plus CLS); a light decoder reconstructs the pixels of the
masked ones.

Per step: patchify (bf16) -> gather of the kept patch rows -> projection GEMM over B*K rows -> token assembly (CLS, fixed
sin-cos positions) -> encoder stack at K+1 tokens -> LayerNorm -> decoder_embed GEMM -> un-shuffle (mask tokens, decoder
positions) -> decoder stack at N+1 tokens -> gather of the B*(N-K) masked rows -> LayerNorm and decoder_pred GEMM on those rows
only -> mean squared error against the (per-patch normalised) pixels.  The token plumbing and the loss are
include_ext/vitssl_mae.h; everything else is the engine SimMIMViT runs on.

The patch features keep the project's unfold order (c, kh, kw), not the paper's (p, q, c): an official checkpoint would need
the rows of decoder_pred (and the columns of the patch projection) permuted; no import is built.

Public surface as SimMIMViT: `forward` (one autograd.Function; any torch loss and optimizer), `inference_forward`, and the
fused `train_step` (MSE, backward, overlapped all-reduce, flat AdamW / LAMB with no autograd graph).  bf16 operands only; no
dropout, drop path or LayerScale."""
import numpy as np
import torch
from torch import nn
from torch.autograd import Function

from vitssl_hip import engine as _engine

from ... import _runtime as R
from ..._runtime import BF16, F32, L, ops
from ...encoder_block import EncoderBlock
from .masking import MAEIndices, bool_mask, draw_keep, num_kept, restore_from_keep


def sincos_1d(dim: int, pos: np.ndarray) -> np.ndarray:
    """[len(pos), dim]: sin then cos of pos / 10000^(2 i / dim), i < dim / 2 (fp64)"""
    omega = 1.0 / 10000 ** (np.arange(dim // 2, dtype=np.float64) / (dim / 2.0))
    out = np.einsum("m,d->md", np.asarray(pos, dtype=np.float64).reshape(-1), omega)
    return np.concatenate([np.sin(out), np.cos(out)], axis=1)


def sincos_2d_table(dim: int, gh: int, gw: int) -> torch.Tensor:
    """The paper's fixed 2-D sin-cos table f32 [1, gh*gw + 1, dim]: row 0 (CLS) zero; the first half of a patch row encodes its
    column, the second half its row (the order of the published code), patches row-major."""
    if dim % 4 != 0:
        raise ValueError(f"the 2-D sin-cos table needs a width that is a multiple of 4, got {dim}")
    ww, hh = np.meshgrid(np.arange(gw, dtype=np.float64), np.arange(gh, dtype=np.float64))      # both [gh, gw]
    table = np.concatenate([sincos_1d(dim // 2, ww), sincos_1d(dim // 2, hh)], axis=1)
    return torch.from_numpy(np.concatenate([np.zeros((1, dim)), table], axis=0)).float().unsqueeze(0)


def _check_width(what, D, H, F):
    if D <= 0 or D % 64 != 0 or F <= 0 or F % 64 != 0:
        raise ValueError(f"MAEViT: {what} width {D} and mlp_dim {F} must be positive multiples of 64")
    if H <= 0 or D % H != 0:
        raise ValueError(f"MAEViT: {what} width {D} is not divisible by its {H} heads")
    dh = D // H
    if not (ops.HD_MIN <= dh <= ops.HD_MAX and dh % ops.HD_STEP == 0):
        raise ValueError(f"MAEViT: {what} head dim {D} / {H} = {dh} unsupported: supported are {ops.HD_SUPPORTED}")


class _MAERuntime:
    """Flat store, the two encoder stacks and the step workspaces of one MAEViT on one device."""

    def __init__(self, model: "MAEViT", device):
        if _engine.linear_operands() == "fp8":
            raise L.VitsslError("MAEViT is built for bf16 linear operands only: use bf16 operands (set_linear_operands('bf16') or "
                                "VITSSL_LINEAR_OPERANDS=bf16)")
        self.model, self.device = model, device
        C, H, W = model.input_shape
        self.C, self.H, self.W, self.P = C, H, W, model.patch_size
        self.gh, self.gw = H // self.P, W // self.P
        self.N, self.K = self.gh * self.gw, model.num_kept
        self.geo = R.PatchGeometry(C, self.P)
        self.Pd, self.Pdp, self.Np = self.geo.Pd, self.geo.Pdp, self.geo.Np
        self.D, self.Dd = model.embed_dim, model.decoder_embed_dim
        self.store = R.FlatStore(model, device)
        st, D, Dd = self.store, self.D, self.Dd
        self.enc = R.EncoderStack(st, [f"encoder_blocks.{i}." for i in range(len(model.encoder_blocks))], D, model.num_heads,
                                  model.mlp_dim, 0.0)
        self.dec = R.EncoderStack(st, [f"decoder_blocks.{i}." for i in range(len(model.decoder_blocks))], Dd, model.decoder_heads,
                                  model.decoder_mlp_dim, 0.0, site_base=3 * len(model.encoder_blocks))
        st.register_weight("dembed", lambda: st.view("decoder_embed.weight", (Dd, D)))
        self.ws = R.Workspace()
        self.geo.register_proj(st, "proj", lambda: st.view("projection.weight", (D, self.Pd)), D)
        self.head = R.PatchHead(st, self.geo, "dpred", "decoder_pred.weight", "decoder_pred.bias", Dd, self.ws)
        self.stage = R.HostStage()
        self.rec = None
        self.save_gen = 0      # id of the forward whose activations `rec` / the stacks hold

    def valid_for(self, device) -> bool:
        return device == self.device and self.store.is_attached()

    # the fixed position tables are buffers of the module (they move and load with it), read where they are
    @property
    def pos(self):
        return self.model.pos_embed.view(self.N + 1, self.D)

    @property
    def dpos(self):
        return self.model.decoder_pos_embed.view(self.N + 1, self.Dd)

    # ------------------------------------------------------------------ index tables
    def prepare(self, keep_cpu, restore_cpu, dev):
        """Host tables -> dict of int32 device views (MAEIndices.NAMES) plus B, Mm, staged as one copy through the runtime's ring
        of pinned buffers (engine.HostStage: they stay valid until the fourth later call)."""
        idx = MAEIndices(keep_cpu, restore_cpu, self.K)
        if idx.N != self.N:
            raise L.VitsslError(f"MAEViT: index tables are for {idx.N} patches, the model has {self.N}")
        return dict(zip(idx.NAMES, self.stage.upload(idx.tables(), dev)), B=idx.B, Mm=idx.Mm)

    # ------------------------------------------------------------------ forward
    def forward(self, x, save: bool, keep_cpu=None, prepared=None, training: bool = True):
        """-> (pred f32 [Mm, Pd], raw pixel targets f32 [Mm, Pd] (fresh tensor), bool mask [B, N, 1])"""
        st, ws = self.store, self.ws
        if x.dim() != 4 or tuple(x.shape[1:]) != (self.C, self.H, self.W):
            raise L.VitsslError(f"MAEViT: expected input [B,{self.C},{self.H},{self.W}], got {tuple(x.shape)}")
        N, K, D, Dd = self.N, self.K, self.D, self.Dd
        self.enc.check_tokens(K + 1)
        self.dec.check_tokens(N + 1)
        x = R.as_f32(x)
        B, dev = x.shape[0], x.device
        if prepared is None:
            if keep_cpu is None:
                keep_cpu, restore_cpu = draw_keep(B, N, K)          # host RNG first: the noise is the step's first draw
            else:
                restore_cpu = restore_from_keep(keep_cpu, N)
            prepared = self.prepare(keep_cpu, restore_cpu, dev)
        p = prepared
        if p["B"] != B:
            raise L.VitsslError(f"MAEViT: index tables are for {p['B']} images, the batch has {B}")
        Mm, M1, M2 = p["Mm"], B * (K + 1), B * (N + 1)
        st.refresh_weights()
        tag = "" if save else "tmp."
        g = lambda name, shape, dtype: ws.get(tag + name, shape, dtype, dev)      # noqa: E731

        targets = torch.empty(Mm, self.Pd, dtype=F32, device=dev)
        self.geo.gather_targets(x, p["midx"], targets)
        # encoder on the visible patches
        patches = g("patches", (B * N, self.Pdp), BF16)
        self.geo.patchify(x, patches)
        kept = g("kept", (B * K, self.Pdp), BF16)
        ops.mae_gather_rows_bf16(patches, p["keep_rows"], kept)
        xk = g("xk", (B * K, D), F32)
        ops.gemm_nt(kept, st.w("proj"), xk, L.EPI_F32, bias=st.view("projection.bias"))
        x0 = g("x0", (M1, D), F32)
        ops.mae_tokens_fwd(xk, p["keep"].view(B, K), self.pos, st.view("cls_token"), x0, B, N, K)
        xL, _ = self.enc.forward(x0, B, K + 1, training, 0, save=save, slot="a")
        h = g("h", (M1, D), BF16)
        mean, rstd = g("mean", (M1,), F32), g("rstd", (M1,), F32)
        ops.layernorm_fwd(xL, st.view("norm.weight"), st.view("norm.bias"), h, mean, rstd)
        # decoder on all tokens
        y = g("y", (M1, Dd), F32)
        ops.gemm_nt(h, st.w("dembed"), y, L.EPI_F32, bias=st.view("decoder_embed.bias"))
        x1 = g("x1", (M2, Dd), F32)
        ops.mae_unshuffle_fwd(y, p["restore"].view(B, N), st.view("mask_token"), self.dpos, x1, B, N, K)
        xD, _ = self.dec.forward(x1, B, N + 1, training, 0, save=save, slot="a")
        # prediction head on the masked rows only (LayerNorm is row-wise)
        xs = g("xs", (Mm, Dd), F32)
        ops.mae_gather_rows_f32(xD, p["mrows"], xs)
        hs = g("hs", (Mm, Dd), BF16)
        smean, srstd = g("smean", (Mm,), F32), g("srstd", (Mm,), F32)
        ops.layernorm_fwd(xs, st.view("decoder_norm.weight"), st.view("decoder_norm.bias"), hs, smean, srstd)
        pred = self.head.forward(hs)
        if save:
            self.save_gen += 1
            self.rec = dict(B=B, Mm=Mm, p=p, kept=kept, xL=xL, h=h, mean=mean, rstd=rstd, xs=xs, hs=hs, smean=smean, srstd=srstd)
        return pred, targets, bool_mask(p["restore"].view(B, N, 1), K)

    def encode_all(self, x):
        """The unmasked encode through `norm`: tokens bf16 [B, N+1, D], the LayerNorm kernel's output (K = N, identity order;
        saves nothing)."""
        st, ws, N, D = self.store, self.ws, self.N, self.D
        x = R.as_f32(x)
        B, dev = x.shape[0], x.device
        self.enc.check_tokens(N + 1)
        st.refresh_weights()
        patches = ws.get("inf.patches", (B * N, self.Pdp), BF16, dev)
        self.geo.patchify(x, patches)
        x0 = ws.get("inf.x0", (B * (N + 1), D), F32, dev)
        ops.gemm_nt(patches, st.w("proj"), x0, L.EPI_EMBED, bias=st.view("projection.bias"), embed=(None, None, self.pos, N, N + 1, 1))
        x0.view(B, N + 1, D)[:, 0] = st.view("cls_token") + self.pos[0]
        xL, _ = self.enc.forward(x0, B, N + 1, False, 0, save=False, slot="inf")
        h = ws.get("inf.h", (B * (N + 1), D), BF16, dev)
        mean, rstd = ws.get("inf.mean", (B * (N + 1),), F32, dev), ws.get("inf.rstd", (B * (N + 1),), F32, dev)
        ops.layernorm_fwd(xL, st.view("norm.weight"), st.view("norm.bias"), h, mean, rstd)
        return h.view(B, N + 1, D)

    # ------------------------------------------------------------------ backward
    def backward(self, dpred_bf16, reducer=None):
        """dpred_bf16: bf16 [Mm, Pdp] (pad columns zero).  Accumulates every parameter gradient into the store's flat gradient
        buffer (the caller zeroes it) and hands every parameter range to the reducer as it becomes final."""
        st, ws, rec = self.store, self.ws, self.rec
        B, Mm, p = rec["B"], rec["Mm"], rec["p"]
        N, K, D, Dd = self.N, self.K, self.D, self.Dd
        M1, M2 = B * (K + 1), B * (N + 1)
        dev = dpred_bf16.device
        gv = st.gview
        ready = (lambda *names: reducer.ready(*st.span(names[0], names[-1]))) if reducer is not None else (lambda *names: None)
        # prediction head
        self.head.wgrad(dpred_bf16, rec["hs"])
        ready("decoder_pred.weight", "decoder_pred.bias")
        dhs = ws.get("dhs", (Mm, Dd), BF16, dev)
        self.head.dgrad(dpred_bf16, dhs)
        gxs = ws.get("gxs", (Mm, Dd), F32, dev)
        ops.layernorm_bwd(dhs, rec["xs"], rec["smean"], rec["srstd"], st.view("decoder_norm.weight"), None, gxs, None,
                          gv("decoder_norm.weight"), gv("decoder_norm.bias"))
        ready("decoder_norm.weight", "decoder_norm.bias")
        # decoder
        gD = ws.get("gD", (M2, Dd), F32, dev)
        ops.mae_scatter_rows_f32(gxs, p["inv"], gD)
        gD = self.dec.backward(gD, slot="a", reducer=reducer)
        dy = ws.get("dy", (M1, Dd), BF16, dev)
        ops.mae_unshuffle_bwd(gD, p["restore"].view(B, N), dy, gv("decoder_embed.bias"), gv("mask_token"), B, N, K)
        ops.gemm_tn(dy, rec["h"], gv("decoder_embed.weight", (Dd, D)))
        ready("decoder_embed.weight", "decoder_embed.bias")
        dh = ws.get("dh", (M1, D), BF16, dev)
        ops.gemm_nt(dy, st.w("dembed.T"), dh, L.EPI_BF16)
        g = ws.get("g", (M1, D), F32, dev)
        ops.layernorm_bwd(dh, rec["xL"], rec["mean"], rec["rstd"], st.view("norm.weight"), None, g, None, gv("norm.weight"), gv("norm.bias"))
        ready("norm.weight", "norm.bias")
        # encoder and the embedding of the kept patches
        g = self.enc.backward(g, slot="a", reducer=reducer)
        dproj = ws.get("dproj", (B * K, D), BF16, dev)
        ops.mae_tokens_bwd(g, dproj, gv("projection.bias"), gv("cls_token"), B, N, K)
        self.geo.proj_wgrad(dproj, rec["kept"], gv("projection.weight", (D, self.Pd)), ws)      # over the B*K kept rows only
        ready("projection.weight", "projection.bias")
        ready("cls_token", "mask_token")      # the module's own parameters lead the store, next to each other

    def loss(self, pred, targets, dpred=None, gscale=0.0, norm_pix=True):
        """The sum of the row losses as a 1-element device tensor (targets normalised in place when `norm_pix`)."""
        loss_sum = self.ws.get("loss_sum", (1,), F32, pred.device)
        loss_sum.zero_()
        ops.mae_loss(pred, targets, loss_sum, dpred, gscale=gscale, norm_pix=norm_pix)
        return loss_sum


class _MAEFn(Function):
    @staticmethod
    def forward(ctx, rt, x, training, need, keep_cpu, *params):
        pred, targets, mask = rt.forward(x, save=need, keep_cpu=keep_cpu, training=training)
        if rt.model.norm_pix_loss:      # the loss kernel's normalisation, in place; its loss output is not used here
            rt.loss(pred, targets, None, norm_pix=True)
        ctx.rt, ctx.gen = rt, rt.save_gen
        ctx.mark_non_differentiable(targets, mask)
        return pred, targets, mask

    @staticmethod
    def backward(ctx, dpred, _dt, _dm):
        rt = ctx.rt
        return (None, None, None, None, None, *R.backward_grads("MAEViT", ctx.gen, rt.save_gen, rt.store,
                                                                lambda: rt.backward(rt.geo.widen_grad(dpred))))      # the engine reads the padded width


class MAEViT(nn.Module):
    def __init__(
        self,
        num_blocks: int,
        input_shape,
        embed_dim: int,
        patch_size: int,
        num_heads: int = 8,
        mlp_dim: int = 3072,
        dropout: float = 0.0,
        mask_ratio: float = 0.75,
        *,
        decoder_embed_dim: int = 512,
        decoder_blocks: int = 8,
        decoder_heads: int = 16,
        decoder_mlp_dim=None,
        norm_pix_loss: bool = True,
    ):
        super().__init__()
        if float(dropout) != 0.0:
            raise ValueError(f"MAEViT: dropout must be 0 (got {dropout}); dropout, drop path and LayerScale are not built for this model")
        C, Hi, Wi = (int(v) for v in input_shape)
        if Hi % patch_size != 0 or Wi % patch_size != 0:
            raise ValueError(f"Image dimensions H={Hi}, W={Wi} must be divisible by patch_size={patch_size}")
        decoder_mlp_dim = 4 * decoder_embed_dim if decoder_mlp_dim is None else int(decoder_mlp_dim)
        _check_width("encoder", embed_dim, num_heads, mlp_dim)
        _check_width("decoder", decoder_embed_dim, decoder_heads, decoder_mlp_dim)
        gh, gw = Hi // patch_size, Wi // patch_size
        N = gh * gw
        self.num_patches, self.num_kept = N, num_kept(N, mask_ratio)
        if not 1 <= self.num_kept <= N - 1:
            raise ValueError(f"MAEViT: mask_ratio={mask_ratio} keeps K = int({N} * (1 - mask_ratio)) = {self.num_kept} of {N} patches; "
                             f"K must lie in [1, {N - 1}]")
        Pd = C * patch_size * patch_size
        self.encoder_blocks = nn.ModuleList([EncoderBlock(embed_dim, num_heads, mlp_dim, 0.0) for _ in range(num_blocks)])
        self.projection = nn.Linear(Pd, embed_dim)                       # over the unfold layout (c, kh, kw), as SimMIMViT
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.norm = nn.LayerNorm(embed_dim)
        self.decoder_embed = nn.Linear(embed_dim, decoder_embed_dim)
        self.mask_token = nn.Parameter(torch.zeros(1, 1, decoder_embed_dim))
        self.decoder_blocks = nn.ModuleList([EncoderBlock(decoder_embed_dim, decoder_heads, decoder_mlp_dim, 0.0) for _ in range(decoder_blocks)])
        self.decoder_norm = nn.LayerNorm(decoder_embed_dim)
        self.decoder_pred = nn.Linear(decoder_embed_dim, Pd)
        nn.init.normal_(self.cls_token, std=0.02)
        nn.init.normal_(self.mask_token, std=0.02)
        # the fixed 2-D sin-cos tables of the paper: persistent buffers (in the state dict, no gradient)
        self.register_buffer("pos_embed", sincos_2d_table(embed_dim, gh, gw))
        self.register_buffer("decoder_pos_embed", sincos_2d_table(decoder_embed_dim, gh, gw))

        self.mask_ratio = mask_ratio
        self.input_shape = (C, Hi, Wi)
        self.embed_dim, self.patch_size = embed_dim, patch_size
        self.num_heads, self.mlp_dim, self.dropout_p = num_heads, mlp_dim, 0.0
        self.decoder_embed_dim, self.decoder_heads, self.decoder_mlp_dim = decoder_embed_dim, decoder_heads, decoder_mlp_dim
        self.norm_pix_loss = bool(norm_pix_loss)
        self._rt = None

    # ------------------------------------------------------------------ runtime
    def runtime(self, device=None) -> _MAERuntime:
        return R.model_runtime(self, "MAEViT", _MAERuntime, self.mask_token, device)

    def flat_store(self):
        return self.runtime().store

    # ------------------------------------------------------------------ reference-style API
    def forward(self, x: torch.Tensor, return_bool_mask=False, keep_cpu=None):
        """-> (pred [Mm, Pd], targets [Mm, Pd]), rows in ascending (b, n) order of the masked patches; the targets are already
        normalised per patch when `norm_pix_loss`, so `nn.MSELoss()(pred, targets)` is the paper's loss.  `keep_cpu` [B, K]
        (optional): the kept patch indices instead of a draw."""
        R.require_gpu(x, "MAEViT")
        rt = self.runtime(x.device)
        need = torch.is_grad_enabled() and any(p.requires_grad for p in rt.store.params)
        pred, targets, mask = _MAEFn.apply(rt, x, self.training, need, keep_cpu, *rt.store.params)
        if return_bool_mask:
            return pred, targets, mask
        return pred, targets

    @torch.no_grad()
    def inference_forward(self, x: torch.Tensor, return_patch_features=False):
        """Unmasked encode through `norm`: the mean over the patch tokens [B, D], or the patch tokens [B, N, D]; switches the
        module to eval (as SimMIMViT.inference_forward)."""
        self.eval()
        R.require_gpu(x, "MAEViT")
        tokens = self.runtime(x.device).encode_all(x)[:, 1:].float()
        return tokens if return_patch_features else tokens.mean(dim=1)

    # ------------------------------------------------------------------ fused step
    def train_step(self, x: torch.Tensor, optimizer, reducer=None, keep_cpu=None, prepared=None) -> torch.Tensor:
        """One full optimisation step (zero_grad -> forward -> MSE(mean) on the (normalised) pixels of the masked patches ->
        backward -> gradient all-reduce -> flat optimizer) with no autograd graph; returns the loss as a device scalar (no host
        sync) and leaves `last_pred` / `last_targets` on the model."""
        R.require_gpu(x, "MAEViT.train_step")
        rt = self.runtime(x.device)
        with R.fused_step(self, rt.store, optimizer, reducer) as apply:
            pred, targets, _ = rt.forward(x, save=True, keep_cpu=keep_cpu, prepared=prepared)
            Mm = pred.shape[0]
            dpb = rt.ws.get("dpred", (Mm, rt.Pdp), BF16, x.device)
            loss_sum = rt.loss(pred, targets, dpb, gscale=1.0 / Mm, norm_pix=self.norm_pix_loss)
            rt.backward(dpb, reducer)
            apply()
            self.last_pred, self.last_targets = pred, targets
            return loss_sum[0] / Mm
