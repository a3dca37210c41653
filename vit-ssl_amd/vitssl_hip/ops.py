"""Tensor-level wrappers over the C ABI: validate device/dtype/shape/contiguity on the
host (a wrong shape must never reach a hand-written kernel), then enqueue on torch's
current stream.  No computation happens in Python and there is no fallback path."""
import collections
import ctypes as C
import operator

import torch

from . import _lib as L
from ._lib import Dropout, Embed, Fp8Gemm, Gemm, call

BF16 = torch.bfloat16
F32 = torch.float32
FP8 = torch.float8_e4m3fn      # OCP e4m3fn: what gfx950's conversion and MFMA instructions implement


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk(t, dtype, name, shape=None):
    if t is None:
        raise L.VitsslError(f"{name}: tensor is None")
    if not t.is_cuda:
        raise L.VitsslError(f"{name}: expected a CUDA (HIP) tensor, got {t.device}; there is no CPU fallback")
    if t.device.index != torch.cuda.current_device():
        # launches go to the CURRENT device's current stream: a tensor of another GPU would be
        # touched by a kernel enqueued on the wrong device
        raise L.VitsslError(f"{name}: tensor lives on {t.device} but the current device is cuda:{torch.cuda.current_device()}; "
                            "call torch.cuda.set_device (one process per GPU) before using the engine")
    if t.dtype != dtype:
        raise L.VitsslError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise L.VitsslError(f"{name}: tensor must be contiguous")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise L.VitsslError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return C.c_void_p(t.data_ptr())


def _opt(t, dtype, name, shape=None):
    return C.c_void_p(0) if t is None else _chk(t, dtype, name, shape)


def make_dropout(p=0.0, seed=0, site=0):
    return Dropout(float(p), int(site) & 0xFFFFFFFF, int(seed) & 0xFFFFFFFFFFFFFFFF)


NO_DROP = make_dropout()

# Optional live kernel timing (bench.py): when PROFILE is a list, every GEMM / attention launch and
# the HBM-bound kernels (LayerNorm, AdamW) are bracketed by HIP events ON THE LAUNCH STREAM and
# (label, flops, start, end, algorithmic_bytes) appended.
PROFILE = None


def _prof_begin():
    if PROFILE is None:
        return None
    ev = torch.cuda.Event(enable_timing=True)
    ev.record(torch.cuda.current_stream())
    return ev


def _prof_end(ev0, label, flops, nbytes=0):
    if ev0 is None:
        return
    ev1 = torch.cuda.Event(enable_timing=True)
    ev1.record(torch.cuda.current_stream())
    PROFILE.append((label, flops, ev0, ev1, nbytes))


def dropout_mask(rows, cols, drop, device):
    keep = torch.empty(rows, cols, dtype=torch.uint8, device=device)
    call("vitssl_dropout_mask", _chk(keep, torch.uint8, "keep"), rows, cols, drop, _stream())
    return keep


def layernorm_fwd(x, gamma, beta, y, mean, rstd, eps=1e-5):
    rows, cols = x.shape
    ev = _prof_begin()
    call("vitssl_layernorm_fwd", _chk(x, F32, "x"), _chk(gamma, F32, "gamma", (cols,)), _chk(beta, F32, "beta", (cols,)),
         _chk(y, BF16, "y", (rows, cols)), _chk(mean, F32, "mean", (rows,)), _chk(rstd, F32, "rstd", (rows,)),
         rows, cols, float(eps), _stream())
    _prof_end(ev, "ln_fwd", 0.0, rows * (6 * cols + 8))          # x fp32 in, y bf16 out, mean / rstd


def layernorm_fwd_fp8(x, gamma, beta, y, y8, mean, rstd, eps=1e-5):
    """LayerNorm forward that writes the e4m3 image `y8` of its output (fp8 operand path); the bf16 image `y` is optional."""
    rows, cols = x.shape
    ev = _prof_begin()
    call("vitssl_layernorm_fwd_fp8", _chk(x, F32, "x"), _chk(gamma, F32, "gamma", (cols,)), _chk(beta, F32, "beta", (cols,)),
         _opt(y, BF16, "y", (rows, cols)), _chk(y8, FP8, "y8", (rows, cols)), _chk(mean, F32, "mean", (rows,)),
         _chk(rstd, F32, "rstd", (rows,)), rows, cols, float(eps), _stream())
    _prof_end(ev, "ln_fwd", 0.0, rows * ((7 if y is not None else 5) * cols + 8))


def _scalar(t, name):
    if t is None:
        return C.c_void_p(0)
    if t.numel() != 1:
        raise L.VitsslError(f"{name}: expected a 1-element fp32 device tensor")
    return _chk(t, F32, name)


def quantize_fp8(x, y8, scale=None, amax=None):
    """y8 = e4m3(clamp(x * scale, +-448)) of a bf16 tensor; `scale` / `amax` are optional 1-element device tensors
    (amax receives max(amax, max|x|)).  NaN maps to NaN (0x7F | sign, as torch's conversion), +-inf and overflow map to +-448;
    the recorded maximum ignores NaN (an infinity makes it +inf)."""
    call("vitssl_quantize_fp8_scaled", _chk(x, BF16, "x"), _chk(y8, FP8, "y8", x.shape), x.numel(), _scalar(scale, "scale"),
         _scalar(amax, "amax"), _stream())


def droppath_table(pairs, B, seed, out):
    """out f32 [len(pairs), B] = the per-sample branch scales (include/vitssl_droppath.h) of the (rate, site) pairs for `seed`:
    1 / (1 - r_eff) where the dropout stream keeps the sample, 0 where it drops it; a rate of 0 gives a row of ones."""
    n = len(pairs)
    if not 1 <= n <= L.DROPPATH_MAX_SITES:
        raise L.VitsslError(f"droppath_table: {n} (rate, site) pairs outside [1, {L.DROPPATH_MAX_SITES}]")
    rates = (C.c_float * n)(*[float(r) for r, _ in pairs])
    sites = (C.c_uint32 * n)(*[int(s) & 0xFFFFFFFF for _, s in pairs])
    call("vitssl_droppath_table", _chk(out, F32, "scale", (n, B)), rates, sites, n, int(B), C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF),
         _stream())
    return out


def _rowscale(rows, M, name):
    """vitssl_rowscale_t of rows = (scale f32 [groups], rows_per_group): row m of the [M, *] operand takes scale[m // rows_per_group]."""
    scale, rpg = rows
    rpg = int(rpg)
    if rpg <= 0 or M % rpg != 0:
        raise L.VitsslError(f"{name}: rows_per_group {rpg} does not divide the {M} rows")
    r = L.RowScale()
    r.scale = _chk(scale, F32, name + " rows.scale", (M // rpg,))
    r.groups, r.rows_per_group = M // rpg, rpg
    return r


def _colscale(cols, N, name):
    """vitssl_colscale_t of cols = gamma f32 [N]: column n of the [*, N] operand takes gamma[n] (LayerScale)."""
    c = L.ColScale()
    c.gamma = _chk(cols, F32, name + " cols(gamma)", (N,))
    c.cols = N
    return c


# LayerNorm backward has one launch path for all its forms (csrc/layernorm.hip); what differs is listed here: the suffix of the
# entry point and the sizing function its workspace is held to.
_LnForm = collections.namedtuple("_LnForm", "sfx query")
_LN_PLAIN = _LnForm("", "vitssl_sum_workspace_floats")
_LN_FP8 = _LnForm("_fp8", "vitssl_sum_workspace_floats")
_LN_ROWS = _LnForm("_rows", "vitssl_sum_workspace_floats")
_LN_LS = _LnForm("_ls", "vitssl_layerscale_workspace_floats")


def _ln_bwd(who, ln, g_res, gm, gm_colsum, drop, fp8=None, rows=None, cols=None, branch=None, dls=None):
    """The launch behind layernorm_bwd / grad_mask_cast and their fp8 forms.  ln = (dy, x, mean, rstd, gamma, g_out, dgamma, dbeta),
    or None for the mask + cast form, whose input is g_res; fp8 = (gm8, scale, amax)."""
    M, N = (ln[1] if ln else g_res).shape
    if cols is not None:
        if (branch is None) != (dls is None):
            raise L.VitsslError(f"{who}: branch= and dls= are given together (gamma's gradient) or both left out")
        form = _LN_LS
        extra = (C.byref(_rowscale(rows, M, who)) if rows is not None else None, C.byref(_colscale(cols, N, who)),
                 _opt(branch, BF16, who + " branch", (M, N)), _opt(dls, F32, who + " dls", (N,)))
    else:
        if branch is not None or dls is not None:
            raise L.VitsslError(f"{who}: branch= / dls= belong to cols= (LayerScale)")
        form = _LN_FP8 if fp8 else (_LN_PLAIN if rows is None else _LN_ROWS)
        extra = () if rows is None else (C.byref(_rowscale(rows, M, who)),)
    if ln:
        dy, x, mean, rstd, gamma, g_out, dgamma, dbeta = ln
        head = (_chk(dy, BF16, "dy", (M, N)), _chk(x, F32, "x"), _chk(mean, F32, "mean", (M,)), _chk(rstd, F32, "rstd", (M,)),
                _chk(gamma, F32, "gamma", (N,)), _opt(g_res, F32, "g_res", (M, N)), _chk(g_out, F32, "g_out", (M, N)))
    else:
        head = (_chk(g_res, F32, "g"),)
    # (a missing gm: the library refuses it where the form needs it; the mask + cast and LayerScale forms refuse it here)
    gm_p = (_opt if fp8 or (ln and form is not _LN_LS) else _chk)(gm, BF16, "gm", (M, N))
    q8 = (_chk(fp8[0], FP8, "gm8", (M, N)), _scalar(fp8[1], "scale"), _scalar(fp8[2], "amax")) if fp8 else ()
    sums = (_chk(dgamma, F32, "dgamma", (N,)), _chk(dbeta, F32, "dbeta", (N,))) if ln else ()
    ws = _tn_workspace((ln[1] if ln else g_res).device, int(getattr(L.lib(), form.query)(M, N)))
    ev = _prof_begin() if ln else None
    call("vitssl_" + ("layernorm_bwd" if ln else "grad_mask_cast") + form.sfx, *head, gm_p, *q8, *sums,
         _opt(gm_colsum, F32, "gm_colsum", (N,)), drop, *extra, M, N, C.c_void_p(ws.data_ptr()), ws.numel(), _stream())
    # dy bf16 + x fp32 (+ residual gradient fp32) in, gradient fp32 (+ masked bf16 / e4m3 operand) out (+ the bf16 branch image in)
    _prof_end(ev, "ln_bwd", 0.0, M * (N * (2 + 4 + (4 if g_res is not None else 0) + 4 + (2 if gm is not None else 0) + (1 if fp8 else 0)
                                           + (2 if branch is not None else 0)) + 8))


def layernorm_bwd(dy, x, mean, rstd, gamma, g_res, g_out, gm, dgamma, dbeta, gm_colsum=None, drop=NO_DROP, rows=None, cols=None,
                  branch=None, dls=None):
    """rows=(scale, rows_per_group): vitssl_layernorm_bwd_rows, the bf16 operand `gm` scaled per row (drop path).
    cols=gamma f32 [cols]: vitssl_layernorm_bwd_ls (LayerScale), `gm` also scaled per column; with branch= (the forward's bf16
    image of the branch) and dls= (f32 [cols]) gamma's gradient is accumulated into dls.  Composes with rows=."""
    _ln_bwd("layernorm_bwd", (dy, x, mean, rstd, gamma, g_out, dgamma, dbeta), g_res, gm, gm_colsum, drop, rows=rows, cols=cols,
            branch=branch, dls=dls)


def layernorm_bwd_fp8(dy, x, mean, rstd, gamma, g_res, g_out, gm, gm8, scale, amax, dgamma, dbeta, gm_colsum=None, drop=NO_DROP):
    """layernorm_bwd that also writes gm8 = e4m3(gm * scale) and records max|gm| in amax."""
    _ln_bwd("layernorm_bwd_fp8", (dy, x, mean, rstd, gamma, g_out, dgamma, dbeta), g_res, gm, gm_colsum, drop, fp8=(gm8, scale, amax))


def grad_mask_cast(g, gm, gm_colsum=None, drop=NO_DROP, rows=None, cols=None, branch=None, dls=None):
    """rows=(scale, rows_per_group): vitssl_grad_mask_cast_rows, `gm` scaled per row (drop path).
    cols=gamma (with branch= and dls= for gamma's gradient): vitssl_grad_mask_cast_ls (LayerScale); composes with rows=."""
    _ln_bwd("grad_mask_cast", None, g, gm, gm_colsum, drop, rows=rows, cols=cols, branch=branch, dls=dls)


def grad_mask_cast_fp8(g, gm, gm8, scale, amax, gm_colsum=None, drop=NO_DROP):
    _ln_bwd("grad_mask_cast_fp8", None, g, gm, gm_colsum, drop, fp8=(gm8, scale, amax))


_OUT0_DTYPE = {L.EPI_BF16: BF16, L.EPI_F32: F32, L.EPI_GELU: BF16, L.EPI_RESID: F32, L.EPI_DGELU: BF16, L.EPI_EMBED: F32}


def _nt_desc(who, sfx, dtype, A, B, epilogue, bias, set_out0, aux, dgelu_aux, out1, colsum, drop, epilogues=None):
    """The vitssl_gemm_t of gemm_nt / gemm_fp8_nt: operands of `dtype` (named "A" + sfx, "B" + sfx in error texts), M / N / K, bias,
    out0 (set_out0(g, M, N): the entry points' rules differ), aux by epilogue, out1, colsum with its workspace, dropout.
    -> (g, M, N, K)"""
    M, K = A.shape
    N, K2 = B.shape
    if K != K2:
        raise L.VitsslError(f"{who}: K mismatch {K} vs {K2}")
    if epilogues is not None and epilogue not in epilogues:
        raise L.VitsslError(f"{who}: epilogue {epilogue} has no fp8-operand form")
    g = Gemm()
    g.A = _chk(A, dtype, "A" + sfx)
    g.B = _chk(B, dtype, "B" + sfx)
    g.M, g.N, g.K = M, N, K
    g.epilogue = epilogue
    g.bias = _opt(bias, F32, "bias", (N,))
    set_out0(g, M, N)
    if epilogue == L.EPI_RESID:
        g.aux = _chk(aux, F32, "aux(residual)", (M, N))
    elif epilogue == L.EPI_DGELU:
        g.aux = _chk(aux, BF16, dgelu_aux, (M, N))
    g.out1 = _opt(out1, BF16, "out1", (M, N))
    g.colsum = _opt(colsum, F32, "colsum", (N,))
    if colsum is not None:
        g.workspace, g.workspace_floats = _sum_ws(colsum.device, M, N)
    g.drop = drop
    return g, M, N, K


def gemm_nt(A, B, out0, epilogue, bias=None, aux=None, out1=None, colsum=None, drop=NO_DROP, embed=None, rows=None, cols=None,
            branch=None):
    """out = A[M,K] @ B[N,K]^T with the fused epilogue (see include/vitssl_hip.h).  rows=(scale, rows_per_group) selects
    vitssl_gemm_bf16_nt_rows (EPI_RESID only): out0 = aux + scale[row // rows_per_group] * drop(acc + bias).
    cols=gamma f32 [N] selects vitssl_gemm_bf16_nt_ls (EPI_RESID only; LayerScale, composes with rows=):
    out0 = aux + scale[row // rows_per_group] * gamma[col] * drop(acc + bias), and branch= (bf16 [M, N], optional) receives
    drop(acc + bias), what the backward multiplies gamma's gradient from."""
    def set_out0(g, M, N):
        if epilogue != L.EPI_EMBED:
            g.out0 = _chk(out0, _OUT0_DTYPE[epilogue], "out0", (M, N))
            return
        if embed is None:
            raise L.VitsslError("gemm_nt: EPI_EMBED needs embed=(mask, mask_token, pos, tokens, out_tokens, tok_offset)")
        mask, mask_token, pos, tokens, out_tokens, tok_offset = embed
        if M % tokens != 0:
            raise L.VitsslError("gemm_nt: M must be a multiple of tokens")
        e = Embed()
        e.mask = _opt(mask, torch.uint8, "mask", (M,))
        e.mask_token = _opt(mask_token, F32, "mask_token", (N,))
        e.pos = _chk(pos, F32, "pos", (out_tokens, N))
        e.tokens, e.out_tokens, e.tok_offset = tokens, out_tokens, tok_offset
        g.embed = e
        g.out0 = _chk(out0, F32, "out0", ((M // tokens) * out_tokens, N))

    g, M, N, K = _nt_desc("gemm_nt", "", BF16, A, B, epilogue, bias, set_out0, aux, "aux(u)", out1, colsum, drop)
    ev = _prof_begin()
    if cols is not None:
        if epilogue != L.EPI_RESID:
            raise L.VitsslError(f"gemm_nt: cols= belongs to EPI_RESID, got epilogue {epilogue}")
        call("vitssl_gemm_bf16_nt_ls", C.byref(g), C.byref(_colscale(cols, N, "gemm_nt")),
             C.byref(_rowscale(rows, M, "gemm_nt")) if rows is not None else None, _opt(branch, BF16, "branch", (M, N)), _stream())
    elif branch is not None:
        raise L.VitsslError("gemm_nt: branch= belongs to cols= (LayerScale)")
    elif rows is not None:
        if epilogue != L.EPI_RESID:
            raise L.VitsslError(f"gemm_nt: rows= belongs to EPI_RESID, got epilogue {epilogue}")
        call("vitssl_gemm_bf16_nt_rows", C.byref(g), C.byref(_rowscale(rows, M, "gemm_nt")), _stream())
    else:
        call("vitssl_gemm_bf16_nt", C.byref(g), _stream())
    _prof_end(ev, f"gemm_nt[epi{epilogue}] {M}x{N}x{K}", 2.0 * M * N * K)


def gemm_fp8_nt(A8, B8, out0, epilogue, alpha=None, bias=None, aux=None, out1=None, out_fp8=None, drop=NO_DROP,
                alpha2=None, colsum=None, out_scale=None, out_amax=None):
    """out = alpha * alpha2 * (A8[M,K] @ B8[N,K]^T) with the fused epilogue; A8 / B8 are e4m3 operands, `alpha` /
    `alpha2` 1-element device tensors (dequantisation factors of the two operands).  `out_fp8`: optional e4m3 image of
    out1 (EPI_GELU) or of out0 (EPI_DGELU), written as e4m3(value * out_scale) with max|value| recorded in out_amax.
    Forward and input-gradient GEMMs (include/vitssl_hip.h)."""
    def set_out0(g, M, N):
        if out0 is None and not (epilogue == L.EPI_DGELU and out_fp8 is not None):
            raise L.VitsslError("gemm_fp8_nt: out0 may only be omitted for EPI_DGELU with out_fp8")
        g.out0 = _opt(out0, _OUT0_DTYPE[epilogue], "out0", (M, N))

    g, M, N, K = _nt_desc("gemm_fp8_nt", "8", FP8, A8, B8, epilogue, bias, set_out0, aux, "aux(g')", out1, colsum, drop,
                          epilogues=(L.EPI_BF16, L.EPI_F32, L.EPI_GELU, L.EPI_RESID, L.EPI_DGELU))
    q = Fp8Gemm()
    q.alpha = _scalar(alpha, "alpha")
    q.alpha2 = _scalar(alpha2, "alpha2")
    q.out_fp8 = _opt(out_fp8, FP8, "out_fp8", (M, N))
    q.out_scale = _scalar(out_scale, "out_scale")
    q.out_amax = _scalar(out_amax, "out_amax")
    if out_fp8 is not None and epilogue not in (L.EPI_GELU, L.EPI_DGELU):
        raise L.VitsslError("gemm_fp8_nt: out_fp8 belongs to EPI_GELU / EPI_DGELU")
    ev = _prof_begin()
    call("vitssl_gemm_fp8_nt", C.byref(g), C.byref(q), _stream())
    _prof_end(ev, f"gemm_fp8_nt[epi{epilogue}] {M}x{N}x{K}", 2.0 * M * N * K)


_TN_WS = {}


def _tn_workspace(device, floats):
    """Per-device slab workspace for the split-M wgrad combine (grown on demand, reused by
    every launch: launches on one stream are ordered, the reduce kernel drains the slabs
    before the next wgrad writes them)."""
    key = (device, torch.cuda.current_stream().cuda_stream)
    ws = _TN_WS.get(key)
    if ws is None or ws.numel() < floats:
        ws = torch.empty(max(floats, 1 << 20), dtype=F32, device=device)
        _TN_WS[key] = ws
    return ws


def _sum_ws(device, rows, cols):
    """(pointer, floats) of scratch for the library's fixed-order sums of a [rows, cols] matrix (include/vitssl_hip.h,
    vitssl_sum_workspace_floats); the TN slab workspace is reused: launches on one stream are ordered."""
    ws = _tn_workspace(device, int(L.lib().vitssl_sum_workspace_floats(rows, cols)))
    return C.c_void_p(ws.data_ptr()), ws.numel()


# The weight-gradient GEMM has one launch path for its two operand kinds (csrc/gemm_tn.hip); what differs is listed here.
_TnKind = collections.namedtuple("_TnKind", "label dtype sfx scalars entry query batch_entry batch_query Job")
_TN_BF16 = _TnKind("gemm_tn", BF16, "", (), "vitssl_gemm_bf16_tn", "vitssl_gemm_tn_workspace_floats",
                   "vitssl_gemm_bf16_tn_batch", "vitssl_gemm_tn_batch_workspace_floats", L.TnJob)
_TN_FP8 = _TnKind("gemm_fp8_tn", FP8, "8", ("alpha", "alpha2"), "vitssl_gemm_fp8_tn", "vitssl_gemm_fp8_tn_workspace_floats",
                  "vitssl_gemm_fp8_tn_batch", "vitssl_gemm_fp8_tn_batch_workspace_floats", L.Fp8TnJob)


def _tn_single(k, A, B, Cacc, scalars, atomic):
    M, N1 = A.shape
    M2, N2 = B.shape
    if M != M2:
        raise L.VitsslError(f"{k.label}: M mismatch {M} vs {M2}")
    a, b, c = _chk(A, k.dtype, "A" + k.sfx), _chk(B, k.dtype, "B" + k.sfx), _chk(Cacc, F32, "C", (N1, N2))
    if atomic:                    # NULL workspace: the partial tiles are added into C with atomics
        wsp, wsn = C.c_void_p(0), 0
    else:
        ws = _tn_workspace(A.device, int(getattr(L.lib(), k.query)(M, N1, N2)))
        wsp, wsn = C.c_void_p(ws.data_ptr()), ws.numel()
    ev = _prof_begin()
    call(k.entry, a, b, c, M, N1, N2, *scalars, wsp, wsn, _stream())
    _prof_end(ev, f"{k.label} {N1}x{N2}x{M}", 2.0 * M * N1 * N2)


def _tn_batch(k, jobs):
    if not jobs:
        return
    M = jobs[0][0].shape[0]
    arr = (k.Job * len(jobs))()
    flops = 0.0
    for j, (A, B, Cacc, *scalars) in enumerate(jobs):
        if len(scalars) != len(k.scalars):
            raise L.VitsslError(f"{k.label}_batch: job {j}: expected (A, B, C{''.join(', ' + n for n in k.scalars)})")
        if A.shape[0] != M or B.shape[0] != M:
            raise L.VitsslError(f"{k.label}_batch: job {j}: row counts {A.shape[0]} / {B.shape[0]} differ from {M}")
        N1, N2 = A.shape[1], B.shape[1]
        q = arr[j]
        setattr(q, "A" + k.sfx, _chk(A, k.dtype, "A" + k.sfx).value)
        setattr(q, "B" + k.sfx, _chk(B, k.dtype, "B" + k.sfx).value)
        q.C, q.N1, q.N2 = _chk(Cacc, F32, "C", (N1, N2)).value, N1, N2
        for name, t in zip(k.scalars, scalars):
            setattr(q, name, _scalar(t, name).value)
        flops += 2.0 * M * N1 * N2
    ws = _tn_workspace(jobs[0][0].device, int(getattr(L.lib(), k.batch_query)(arr, len(jobs), M)))
    ev = _prof_begin()
    call(k.batch_entry, arr, len(jobs), M, C.c_void_p(ws.data_ptr()), ws.numel(), _stream())
    _prof_end(ev, f"{k.label} batch{len(jobs)}x{M}", flops)


def gemm_tn(A, B, Cacc, atomic=False):
    """Cacc[N1,N2] (fp32) += A[M,N1]^T @ B[M,N2].  `atomic`: no slab workspace, the partial tiles are added into Cacc with atomics."""
    _tn_single(_TN_BF16, A, B, Cacc, (), atomic)


def gemm_fp8_tn(A8, B8, Cacc, alpha=None, alpha2=None, atomic=False):
    """Cacc[N1,N2] (fp32) += alpha * alpha2 * A8[M,N1]^T @ B8[M,N2] on e4m3 operands (weight gradient of the fp8 path);
    `atomic` as in gemm_tn."""
    _tn_single(_TN_FP8, A8, B8, Cacc, (_scalar(alpha, "alpha"), _scalar(alpha2, "alpha2")), atomic)


def gemm_tn_batch(jobs):
    """For every (A, B, Cacc) of `jobs` (at most 8, all with the same row count M): Cacc[N1,N2] (fp32) += A[M,N1]^T @ B[M,N2], in
    one launch with one shared split count and one reduce pass (vitssl_gemm_bf16_tn_batch)."""
    _tn_batch(_TN_BF16, jobs)


def gemm_fp8_tn_batch(jobs):
    """For every (A8, B8, Cacc, alpha, alpha2) of `jobs` (at most 8, same row count M): Cacc += alpha * alpha2 * A8^T @ B8 on e4m3
    operands, in one launch (vitssl_gemm_fp8_tn_batch)."""
    _tn_batch(_TN_FP8, jobs)


def attn_fwd(qkv, out, lse, B, N, H, dh, probs=None, out_fp8=None):
    """`out_fp8` (fp8 path): also the e4m3 image of the fp32 values `out` is rounded from, at unit scale.  NaN maps to NaN (a NaN
    byte; its sign is not kept), +-inf and overflow map to +-448."""
    ev = _prof_begin()
    _attn_fwd(qkv, out, lse, B, N, H, dh, probs, out_fp8)
    _prof_end(ev, f"attn_fwd B{B} N{N} H{H}", 4.0 * B * H * N * N * dh)


def _attn_fwd(qkv, out, lse, B, N, H, dh, probs=None, out_fp8=None):
    if out_fp8 is not None:       # fp8 operand path: also the e4m3 image of `out`
        call("vitssl_attn_fwd_fp8", _chk(qkv, BF16, "qkv", (B * N, 3 * H * dh)), _chk(out, BF16, "out", (B * N, H * dh)),
             _chk(out_fp8, FP8, "out_fp8", (B * N, H * dh)), _chk(lse, F32, "lse", (B, H, N)),
             _opt(probs, F32, "probs", (B, H, N, N)), B, N, H, dh, _stream())
        return
    call("vitssl_attn_fwd", _chk(qkv, BF16, "qkv", (B * N, 3 * H * dh)), _chk(out, BF16, "out", (B * N, H * dh)),
         _chk(lse, F32, "lse", (B, H, N)), _opt(probs, F32, "probs", (B, H, N, N)), B, N, H, dh, _stream())


def attn_bwd(qkv, out, dout, lse, dqkv, delta_ws, B, N, H, dh, dqkv_fp8=None, scale=None, amax=None):
    """`dqkv_fp8` (fp8 path): also the e4m3 image e4m3(dqkv * scale), with max|dqkv| recorded in `amax`.  NaN maps to NaN (a NaN
    byte; its sign is not kept), +-inf and overflow map to +-448; the recorded maximum ignores NaN."""
    ev = _prof_begin()
    if dqkv_fp8 is not None:
        call("vitssl_attn_bwd_fp8", _chk(qkv, BF16, "qkv", (B * N, 3 * H * dh)), _chk(out, BF16, "out", (B * N, H * dh)),
             _chk(dout, BF16, "dout", (B * N, H * dh)), _chk(lse, F32, "lse", (B, H, N)), _opt(dqkv, BF16, "dqkv", (B * N, 3 * H * dh)),
             _chk(dqkv_fp8, FP8, "dqkv_fp8", (B * N, 3 * H * dh)), _scalar(scale, "scale"), _scalar(amax, "amax"), B, N, H, dh, _stream())
    else:
        _attn_bwd(qkv, out, dout, lse, dqkv, delta_ws, B, N, H, dh)
    _prof_end(ev, f"attn_bwd B{B} N{N} H{H}", 8.0 * B * H * N * N * dh)


def _attn_bwd(qkv, out, dout, lse, dqkv, delta_ws, B, N, H, dh):
    call("vitssl_attn_bwd", _chk(qkv, BF16, "qkv", (B * N, 3 * H * dh)), _chk(out, BF16, "out", (B * N, H * dh)),
         _chk(dout, BF16, "dout", (B * N, H * dh)), _chk(lse, F32, "lse", (B, H, N)),
         _chk(dqkv, BF16, "dqkv", (B * N, 3 * H * dh)), _chk(delta_ws, F32, "delta_ws", (B, H, N)), B, N, H, dh, _stream())


# ---- head dims other than 64 (include/vitssl_attention_hd.h) and the dispatch between the two families
HD_MIN, HD_MAX, HD_STEP = 8, 128, 8
HD_SUPPORTED = "head dims 8, 16, ..., 128 (multiples of 8; 64 runs the dh = 64 kernels)"


def attn_hd_fwd(qkv, out, lse, B, N, H, dh, probs=None):
    ev = _prof_begin()
    call("vitssl_attn_hd_fwd", _chk(qkv, BF16, "qkv", (B * N, 3 * H * dh)), _chk(out, BF16, "out", (B * N, H * dh)),
         _chk(lse, F32, "lse", (B, H, N)), _opt(probs, F32, "probs", (B, H, N, N)), B, N, H, dh, _stream())
    _prof_end(ev, f"attn_hd_fwd B{B} N{N} H{H} dh{dh}", 4.0 * B * H * N * N * dh)


def attn_hd_bwd(qkv, out, dout, lse, dqkv, delta_ws, B, N, H, dh):
    ev = _prof_begin()
    call("vitssl_attn_hd_bwd", _chk(qkv, BF16, "qkv", (B * N, 3 * H * dh)), _chk(out, BF16, "out", (B * N, H * dh)),
         _chk(dout, BF16, "dout", (B * N, H * dh)), _chk(lse, F32, "lse", (B, H, N)),
         _chk(dqkv, BF16, "dqkv", (B * N, 3 * H * dh)), _chk(delta_ws, F32, "delta_ws", (B, H, N)), B, N, H, dh, _stream())
    _prof_end(ev, f"attn_hd_bwd B{B} N{N} H{H} dh{dh}", 8.0 * B * H * N * N * dh)


def attn_family(dh):
    """-> (attn_fwd, attn_bwd) of the kernel family that serves head dim `dh` with bf16 operands: the dh = 64 kernels for 64,
    the head-dim-templated streaming kernels for every other supported value.  Raises before anything is launched."""
    try:
        d = operator.index(dh)        # Python, numpy and symbolic integers alike
    except TypeError:
        d = None
    if d == 64:
        return attn_fwd, attn_bwd
    if d is not None and HD_MIN <= d <= HD_MAX and d % HD_STEP == 0:
        return attn_hd_fwd, attn_hd_bwd
    raise L.VitsslError(f"head dim {dh} (embed_dim / num_heads) unsupported by the attention kernels: supported are {HD_SUPPORTED}")


def attn_fwd_any(qkv, out, lse, B, N, H, dh, probs=None):
    attn_family(dh)[0](qkv, out, lse, B, N, H, dh, probs=probs)


def attn_bwd_any(qkv, out, dout, lse, dqkv, delta_ws, B, N, H, dh):
    attn_family(dh)[1](qkv, out, dout, lse, dqkv, delta_ws, B, N, H, dh)


def patchify_bf16(img, patches, P):
    B, Cc, H, W = img.shape
    call("vitssl_patchify_bf16", _chk(img, F32, "img"), _chk(patches, BF16, "patches", (B * (H // P) * (W // P), Cc * P * P)),
         B, Cc, H, W, P, _stream())


def gather_patches_f32(img, idx, out, P):
    B, Cc, H, W = img.shape
    n = idx.numel()
    call("vitssl_gather_patches_f32", _chk(img, F32, "img"), _chk(idx, torch.int32, "idx"), _chk(out, F32, "out", (n, Cc * P * P)),
         n, Cc, H, W, P, _stream())


def gather_rows_bf16(x, idx, out):
    rows, cols = x.shape
    n = idx.numel()
    call("vitssl_gather_rows_bf16", _chk(x, F32, "x"), _chk(idx, torch.int32, "idx"), _chk(out, BF16, "out", (n, cols)), n, cols, _stream())


def scatter_rows_f32(src, inv, g):
    rows, cols = g.shape
    call("vitssl_scatter_rows_f32", _chk(src, BF16, "src"), _chk(inv, torch.int32, "inv", (rows,)), _chk(g, F32, "g"), rows, cols, _stream())


def gather_cls_f32(x, out, B, T, D):
    call("vitssl_gather_cls_f32", _chk(x, F32, "x", (B * T, D)), _chk(out, F32, "out", (B, D)), B, T, D, _stream())


def scatter_cls_f32(gcls, g, B, T, D):
    call("vitssl_scatter_cls_f32", _chk(gcls, F32, "gcls", (B, D)), _chk(g, F32, "g", (B * T, D)), B, T, D, _stream())


def pool_tokens_fwd(x, out, B, T, D):
    """out[b] = the fp32 mean of image b's patch rows x[b*T + 1 .. b*T + T-1] (global average pooling; the CLS row is not read)."""
    call("vitssl_pool_tokens_fwd", _chk(x, F32, "x", (B * T, D)), _chk(out, F32, "out", (B, D)), B, T, D, _stream())


def pool_tokens_bwd(dout, g, B, T, D):
    """g[b*T] = 0 and g[b*T + t] = dout[b] / (T - 1) for t >= 1: every element of g is written."""
    call("vitssl_pool_tokens_bwd", _chk(dout, F32, "dout", (B, D)), _chk(g, F32, "g", (B * T, D)), B, T, D, _stream())


def embed_bwd(dtok, mask, dproj, dpos, dmask_token, dbias, dcls, B, tokens, tok_offset, D):
    T_out = tokens + tok_offset
    wsn = int(L.lib().vitssl_embed_bwd_workspace_floats(B, tokens, tok_offset, D))
    ws = _tn_workspace(dtok.device, wsn)       # shared scratch: launches on one stream are ordered
    call("vitssl_embed_bwd", _chk(dtok, F32, "dtok", (B * T_out, D)), _opt(mask, torch.uint8, "mask", (B * tokens,)),
         _chk(dproj, BF16, "dproj", (B * tokens, D)), _opt(dpos, F32, "dpos", (T_out, D)),
         _opt(dmask_token, F32, "dmask_token", (D,)), _opt(dbias, F32, "dbias", (D,)), _opt(dcls, F32, "dcls", (D,)),
         B, tokens, tok_offset, D, C.c_void_p(ws.data_ptr()), ws.numel(), _stream())


def l1_loss(pred, target, loss_sum, dpred=None, gscale=0.0):
    n = pred.numel()
    call("vitssl_l1_loss", _chk(pred, F32, "pred"), _chk(target, F32, "target", pred.shape), _chk(loss_sum, F32, "loss_sum", (1,)),
         _opt(dpred, BF16, "dpred", pred.shape), float(gscale), n, *_sum_ws(pred.device, n, 1), _stream())


def cross_entropy(logits, labels, loss_sum, dlogits=None, gscale=0.0):
    B, Cn = logits.shape
    call("vitssl_cross_entropy", _chk(logits, F32, "logits"), _chk(labels, torch.int64, "labels", (B,)),
         _chk(loss_sum, F32, "loss_sum", (1,)), _opt(dlogits, BF16, "dlogits", (B, Cn)), float(gscale), B, Cn, _stream())


def colsum_bf16(x, out):
    rows, cols = x.shape
    call("vitssl_colsum_bf16", _chk(x, BF16, "x"), _chk(out, F32, "out", (cols,)), rows, cols, *_sum_ws(x.device, rows, cols), _stream())


def cast_bf16(src, dst):
    call("vitssl_cast_bf16", _chk(src, F32, "src"), _chk(dst, BF16, "dst", src.shape), src.numel(), _stream())


def cast_transpose_bf16(src, dst, dst_t):
    R, Cn = src.shape
    call("vitssl_cast_transpose_bf16", _chk(src, F32, "src"), _opt(dst, BF16, "dst", (R, Cn)), _opt(dst_t, BF16, "dst_t", (Cn, R)),
         R, Cn, _stream())


class _JobTablePlan:
    """Device-resident job table of a batched (source -> image, transposed image) launch: built once per set of
    (source, destination) pointers, re-uploaded only when a pointer or shape changes.  A plan names its record struct (`Job`,
    the mirror of the C struct: the host records take their layout from it), its entry point and the dtype of its destinations."""
    Job = entry = dst_dtype = None

    def __init__(self):
        self.key = None
        self.jobs_dev = None
        self.starts_dev = None
        self.njobs = 0
        self.total = 0
        self.keep = None

    def _record(self, s, d, t):
        """one job as the fields of `Job`, in order; the tuple of all records is the key of the uploaded table"""
        return (s.data_ptr(), 0 if d is None else d.data_ptr(), 0 if t is None else t.data_ptr(), s.shape[0], s.shape[1])

    def _check(self, s, d, t):
        R, Cn = s.shape
        _chk(s, F32, "src"); _opt(d, self.dst_dtype, "dst", (R, Cn)); _opt(t, self.dst_dtype, "dst_t", (Cn, R))

    def _rebuilt(self, dev):
        """per-table device state behind the job table (none here)"""

    def _extra(self):
        """launch arguments between total_tiles and the stream (none here)"""
        return ()

    def run(self, jobs):
        """jobs: list of (src f32 [R,C], dst [R,C] | None, dst_t [C,R] | None)."""
        import numpy as np
        key = tuple(self._record(s, d, t) for s, d, t in jobs)
        if key != self.key:
            for s, d, t in jobs:
                self._check(s, d, t)
            dev = jobs[0][0].device
            rec = np.zeros(len(jobs), dtype=np.dtype(self.Job))
            starts = np.zeros(len(jobs) + 1, dtype=np.int32)
            for i, k in enumerate(key):
                rec[i] = k
                starts[i + 1] = starts[i] + ((k[3] + 63) // 64) * ((k[4] + 63) // 64)
            self.jobs_dev = torch.from_numpy(rec.view(np.uint8).copy()).to(dev)
            self.starts_dev = torch.from_numpy(starts).to(dev)
            self.njobs, self.total, self.key = len(jobs), int(starts[-1]), key
            self._rebuilt(dev)
        self.keep = jobs        # the sources must outlive the launch
        call(self.entry, C.c_void_p(self.jobs_dev.data_ptr()), C.c_void_p(self.starts_dev.data_ptr()), self.njobs, self.total,
             *self._extra(), _stream())


class CastPlan(_JobTablePlan):
    """Job table of `vitssl_cast_transpose_batch`: dst bf16 [R,C], dst_t bf16 [C,R]."""
    Job, entry, dst_dtype = L.CastJob, "vitssl_cast_transpose_batch", BF16


# ---- the patch path for any patch side and channel count (include/vitssl_patch.h) ----
def _chk_ld(t, dtype, name, rows, cols):
    """A [rows, cols] matrix with unit column stride whose rows lie `ld` >= cols elements apart (a contiguous matrix or the
    column prefix of a wider one) -> (pointer, ld)."""
    if t is None:
        raise L.VitsslError(f"{name}: tensor is None")
    if not t.is_cuda or t.device.index != torch.cuda.current_device():
        raise L.VitsslError(f"{name}: expected a tensor of the current CUDA (HIP) device, got {t.device}; there is no CPU fallback")
    if t.dtype != dtype:
        raise L.VitsslError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if tuple(t.shape) != (rows, cols):
        raise L.VitsslError(f"{name}: expected shape {(rows, cols)}, got {tuple(t.shape)}")
    ld = t.stride(0) if rows > 1 else max(t.stride(0), cols)
    if t.stride(1) != 1 or ld < cols:
        raise L.VitsslError(f"{name}: expected unit column stride and a row stride >= {cols}, got strides {tuple(t.stride())}")
    return C.c_void_p(t.data_ptr()), int(ld)


def patchify_ld_bf16(img, patches, P):
    """img f32 [B,C,H,W] -> patches bf16 [B*gh*gw, ld], ld >= C*P*P, any P; columns C*P*P .. ld-1 are written as zeros"""
    B, Cc, H, W = img.shape
    if P <= 0 or H % P != 0 or W % P != 0:
        raise L.VitsslError(f"patchify_ld: image {H}x{W} not divisible by patch {P}")
    rows = B * (H // P) * (W // P)
    if patches is None or patches.dim() != 2 or patches.shape[1] < Cc * P * P:
        raise L.VitsslError(f"patchify_ld: expected patches [{rows}, ld >= {Cc * P * P}], got {None if patches is None else tuple(patches.shape)}")
    call("vitssl_patchify_ld_bf16", _chk(img, F32, "img"), _chk(patches, BF16, "patches", (rows, patches.shape[1])), B, Cc, H, W, P,
         patches.shape[1], _stream())


def gather_patches_any_f32(img, idx, out, P):
    B, Cc, H, W = img.shape
    n = idx.numel()
    call("vitssl_gather_patches_any_f32", _chk(img, F32, "img"), _chk(idx, torch.int32, "idx"), _chk(out, F32, "out", (n, Cc * P * P)),
         n, Cc, H, W, P, _stream())


def l1_loss_ld(pred, target, loss_sum, dpred=None, gscale=0.0):
    """L1 loss of pred / target f32 [rows, cols] (each contiguous or a column prefix of a wider matrix); dpred bf16 [rows, ld_d]
    contiguous, ld_d >= cols: +-gscale / 0 in the first cols columns, zeros behind them."""
    rows, cols = pred.shape
    pp, ld_p = _chk_ld(pred, F32, "pred", rows, cols)
    tp, ld_t = _chk_ld(target, F32, "target", rows, cols)
    ld_d = 0
    if dpred is not None:
        if dpred.dim() != 2 or dpred.shape[0] != rows or dpred.shape[1] < cols:
            raise L.VitsslError(f"l1_loss_ld: dpred must be [{rows}, ld_d >= {cols}], got {tuple(dpred.shape)}")
        ld_d = dpred.shape[1]
    call("vitssl_l1_loss_ld", pp, ld_p, tp, ld_t, _chk(loss_sum, F32, "loss_sum", (1,)), _opt(dpred, BF16, "dpred"), ld_d, float(gscale),
         rows, cols, *_sum_ws(pred.device, rows * cols, 1), _stream())


def accumulate_ld_f32(dst, src, cols=None):
    """dst f32 [rows, cols] (contiguous) += src[:, :cols] of src f32 [rows, ld] (contiguous)"""
    rows, c = dst.shape
    if src is None or src.dim() != 2 or src.shape[0] != rows or src.shape[1] < c:
        raise L.VitsslError(f"accumulate_ld: src must be [{rows}, ld >= {c}], got {None if src is None else tuple(src.shape)}")
    call("vitssl_accumulate_ld_f32", _chk(dst, F32, "dst"), _chk(src, F32, "src"), rows, c, src.shape[1], _stream())


class CastPlanLd(CastPlan):
    """CastPlan whose destinations may be wider / taller than the source (`vitssl_cast_transpose_batch_ld`): dst bf16
    [>= R, ld >= C], dst_t bf16 [>= C, ld >= R].  Only the image of the source is written; the destinations are allocated
    zeroed, so their pad stays zero through every refresh."""
    Job, entry = L.CastLdJob, "vitssl_cast_transpose_batch_ld"

    def _record(self, s, d, t):
        return super()._record(s, d, t) + (0 if d is None else d.shape[1], 0 if t is None else t.shape[1])

    def _check(self, s, d, t):
        R, Cn = s.shape
        _chk(s, F32, "src"); _opt(d, BF16, "dst"); _opt(t, BF16, "dst_t")
        if d is not None and (d.dim() != 2 or d.shape[0] < R or d.shape[1] < Cn):
            raise L.VitsslError(f"cast plan: dst {tuple(d.shape)} does not hold the [{R}, {Cn}] source")
        if t is not None and (t.dim() != 2 or t.shape[0] < Cn or t.shape[1] < R):
            raise L.VitsslError(f"cast plan: dst_t {tuple(t.shape)} does not hold the transposed [{R}, {Cn}] source")


class Fp8WeightPlan(_JobTablePlan):
    """Job table of `vitssl_fp8_quantize_weights` (per-tensor power-of-two scales computed on the device, no host
    synchronisation): dst e4m3 [R,C], dst_t e4m3 [C,R]; `alpha` holds one dequantisation factor per job."""
    Job, entry, dst_dtype = L.Fp8WeightJob, "vitssl_fp8_quantize_weights", FP8

    def __init__(self):
        super().__init__()
        self.amax = self.alpha = None

    def _rebuilt(self, dev):
        self.amax = torch.zeros(self.njobs, dtype=F32, device=dev)
        self.alpha = torch.ones(self.njobs, dtype=F32, device=dev)

    def _extra(self):
        return C.c_void_p(self.amax.data_ptr()), C.c_void_p(self.alpha.data_ptr())


def adamw(p, g, m, v, lr, beta1, beta2, eps, wd, step, gscale=1.0):
    n = p.numel()
    ev = _prof_begin()
    call("vitssl_adamw", _chk(p, F32, "p"), _chk(g, F32, "g", p.shape), _chk(m, F32, "m", p.shape), _chk(v, F32, "v", p.shape),
         n, float(lr), float(beta1), float(beta2), float(eps), float(wd), int(step), float(gscale), _stream())
    _prof_end(ev, "adamw", 0.0, 28 * n)                          # p, m, v read + written, g read


class AdamWPlan:
    """Device-resident segment table of `vitssl_adamw_segments` / `vitssl_grad_sumsq` (include/vitssl_optim.h) over a flat
    store of `numel` floats, with the workspace of the norm and its one-float result slot.  `segments`: (offset, n, lr_scale,
    weight_decay) per parameter that takes part, in ascending order; checked on the host by the library when the plan is
    built (offsets multiples of 4 floats, no overlap, inside the store).  Built once and kept until the set of parameters changes.
    `lamb_buffers()` adds, on first use, what `vitssl_lamb_segments` (include/vitssl_lamb.h) needs: its workspace and the
    `trust` tensor [nseg]; a plan that only AdamW uses never allocates them."""

    def __init__(self, segments, numel, device):
        segments = [(int(o), int(n), float(s), float(w)) for o, n, s, w in segments]
        l = L.lib()
        self.nseg, self.numel = len(segments), int(numel)
        nbytes = int(l.vitssl_optim_table_bytes(self.nseg))
        host = torch.zeros(max(nbytes, 8), dtype=torch.uint8)
        arr = (L.OptimSegment * max(self.nseg, 1))(*[L.OptimSegment(*s) for s in segments])
        call("vitssl_optim_table_build", arr, self.nseg, self.numel, C.c_void_p(host.data_ptr()), nbytes)
        self.elements = sum(s[1] for s in segments)
        self.table = host.to(device)
        self.workspace = torch.empty(int(l.vitssl_grad_sumsq_workspace_bytes(self.nseg)), dtype=torch.uint8, device=device)
        self.sumsq = torch.zeros(1, dtype=F32, device=device)
        self._rows, self.lamb_workspace, self.trust = arr, None, None

    def lamb_buffers(self):
        """(workspace, trust) of lamb_segments, allocated on the first call"""
        if self.trust is None:
            nbytes = int(L.lib().vitssl_lamb_workspace_bytes(self._rows, self.nseg))
            if nbytes <= 0:
                raise L.VitsslError(f"vitssl_lamb_workspace_bytes refused a table of {self.nseg} segments")
            self.lamb_workspace = torch.empty(nbytes, dtype=torch.uint8, device=self.table.device)
            self.trust = torch.ones(self.nseg, dtype=F32, device=self.table.device)
        return self.lamb_workspace, self.trust


def _flat(t, name, plan):
    if t.dim() != 1 or t.numel() != plan.numel:
        raise L.VitsslError(f"{name}: expected the flat buffer of {plan.numel} floats the plan was built for, got {tuple(t.shape)}")
    return _chk(t, F32, name)


def grad_sumsq(g, plan, out=None, workspace=None):
    """out[0] (default: plan.sumsq) = sum of g^2 over the plan's segments; deterministic, no host synchronisation."""
    out = plan.sumsq if out is None else out
    ws = plan.workspace if workspace is None else workspace
    ev = _prof_begin()
    call("vitssl_grad_sumsq", _flat(g, "g", plan), _chk(plan.table, torch.uint8, "table"), plan.nseg, _chk(out, F32, "out", (1,)),
         _chk(ws, torch.uint8, "workspace"), ws.numel(), _stream())
    _prof_end(ev, "grad_sumsq", 0.0, 4 * plan.elements)
    return out


def adamw_segments(p, g, m, v, plan, lr, beta1, beta2, eps, step, gscale=1.0, sumsq=None, max_norm=0.0):
    """One launch of AdamW over the plan's segments (lr * lr_scale and the weight decay of each).  With `sumsq` (the result
    of grad_sumsq) the gradient is scaled by min(1, max_norm / (gscale * sqrt(sumsq) + 1e-6)) on the device; g is not written."""
    ev = _prof_begin()
    call("vitssl_adamw_segments", _flat(p, "p", plan), _flat(g, "g", plan), _flat(m, "m", plan), _flat(v, "v", plan),
         _chk(plan.table, torch.uint8, "table"), plan.nseg, float(lr), float(beta1), float(beta2), float(eps), int(step), float(gscale),
         _opt(sumsq, F32, "sumsq", (1,)), float(max_norm), _stream())
    _prof_end(ev, "adamw_segments", 0.0, 28 * plan.elements)


def lamb_segments(p, g, m, v, plan, lr, beta1, beta2, eps, step, gscale=1.0, sumsq=None, max_norm=0.0, always_adapt=False,
                  trust_clip=False, trust=None, workspace=None):
    """One LAMB step over the plan's segments (include/vitssl_lamb.h): the moment pass, the per-segment trust ratios and the
    apply pass, three launches.  `sumsq` clips as in adamw_segments; g is not written.  The ratios land in `trust`
    (default: the plan's tensor [nseg]), which is returned; reading it is the caller's synchronisation."""
    ws0, trust0 = (None, None) if (trust is not None and workspace is not None) else plan.lamb_buffers()
    trust = trust0 if trust is None else trust
    ws = ws0 if workspace is None else workspace
    flags = (L.LAMB_ALWAYS_ADAPT if always_adapt else 0) | (L.LAMB_TRUST_CLIP if trust_clip else 0)
    ev = _prof_begin()
    call("vitssl_lamb_segments", _flat(p, "p", plan), _flat(g, "g", plan), _flat(m, "m", plan), _flat(v, "v", plan),
         _chk(plan.table, torch.uint8, "table"), plan.nseg, float(lr), float(beta1), float(beta2), float(eps), int(step), float(gscale),
         _opt(sumsq, F32, "sumsq", (1,)), float(max_norm), flags, _chk(trust, F32, "trust", (plan.nseg,)),
         _chk(ws, torch.uint8, "workspace"), ws.numel(), _stream())
    _prof_end(ev, "lamb_segments", 0.0, 40 * plan.elements)        # moments: p, g, m, v read, m, v written; apply: p, m, v read, p written
    return trust


def ema(teacher, student, m):
    ev = _prof_begin()
    call("vitssl_ema", _chk(teacher, F32, "teacher"), _chk(student, F32, "student", teacher.shape), teacher.numel(), float(m), _stream())
    _prof_end(ev, "ema", 0.0, 12 * teacher.numel())               # teacher read + written, student read


# ---- DINO ----------------------------------------------------------------------------
def rownorm_fwd(z, zn, inv_norm):
    rows, cols = z.shape
    call("vitssl_rownorm_fwd", _chk(z, F32, "z"), _chk(zn, BF16, "zn", (rows, cols)), _chk(inv_norm, F32, "inv_norm", (rows,)), rows, cols, _stream())


def rownorm_bwd(dzn, zn, inv_norm, dz):
    rows, cols = dzn.shape
    call("vitssl_rownorm_bwd", _chk(dzn, F32, "dzn"), _chk(zn, BF16, "zn", (rows, cols)), _chk(inv_norm, F32, "inv_norm", (rows,)),
         _chk(dz, BF16, "dz", (rows, cols)), rows, cols, _stream())


def weightnorm_fold(g, v, w_f32, inv_vnorm):
    K, D = v.shape
    call("vitssl_weightnorm_fold", _chk(g, F32, "g"), _chk(v, F32, "v"), _chk(w_f32, F32, "w", (K, D)), _chk(inv_vnorm, F32, "inv_vnorm", (K,)),
         K, D, _stream())


def weightnorm_bwd(dw, g, v, inv_vnorm, dg, dv):
    K, D = v.shape
    call("vitssl_weightnorm_bwd", _chk(dw, F32, "dw", (K, D)), _chk(g, F32, "g"), _chk(v, F32, "v"), _chk(inv_vnorm, F32, "inv_vnorm", (K,)),
         _chk(dg, F32, "dg"), _chk(dv, F32, "dv", (K, D)), K, D, _stream())


def dino_tws_floats(G, B, K):
    """size of vitssl_dino_loss's scratch: [B, K] teacher probabilities + VITSSL_DINO_TWS_EXTRA(G, B) statistics"""
    return int(L.lib().vitssl_dino_loss_workspace_floats(G, B, K))


def dino_loss(teacher, student, center, t_ws, loss_sum, dstudent, G, V, B, K, teacher_temp, student_temp, gscale=1.0):
    ev = _prof_begin()
    _dino_loss(teacher, student, center, t_ws, loss_sum, dstudent, G, V, B, K, teacher_temp, student_temp, gscale)
    # teacher / student logits read (fp32), teacher-probability scratch written + read, bf16 gradient written
    _prof_end(ev, "dino_loss", 0.0, B * K * (4 * (G + V) + 8 + (2 * V if dstudent is not None else 0)))


def _dino_loss(teacher, student, center, t_ws, loss_sum, dstudent, G, V, B, K, teacher_temp, student_temp, gscale=1.0):
    call("vitssl_dino_loss", _chk(teacher, F32, "teacher", (G * B, K)), _chk(student, F32, "student", (V * B, K)),
         _chk(center, F32, "center"), _chk(t_ws, F32, "t_ws"), t_ws.numel(), _chk(loss_sum, F32, "loss_sum", (1,)),
         _opt(dstudent, BF16, "dstudent", (V * B, K)), G, V, B, K, float(teacher_temp), float(student_temp), float(gscale), _stream())


def colsum_f32(x, out):
    rows, cols = x.shape
    ev = _prof_begin()
    call("vitssl_colsum_f32", _chk(x, F32, "x"), _chk(out, F32, "out", (cols,)), rows, cols, _stream())
    _prof_end(ev, "center_colsum", 0.0, 4 * rows * cols)


def center_ema(center, colsum, momentum, inv_rows):
    K = colsum.numel()
    call("vitssl_center_ema", _chk(center, F32, "center"), _chk(colsum, F32, "colsum"), K, float(momentum), float(inv_rows), _stream())


def bicubic_resize_fwd(src, dst, gh0, gw0, gh, gw):
    D = src.shape[1]
    call("vitssl_bicubic_resize_fwd", _chk(src, F32, "src", (gh0 * gw0, D)), _chk(dst, F32, "dst", (gh * gw, D)),
         gh0, gw0, gh, gw, D, _stream())


def bicubic_resize_bwd(ddst, dsrc, gh0, gw0, gh, gw):
    D = ddst.shape[1]
    call("vitssl_bicubic_resize_bwd", _chk(ddst, F32, "ddst", (gh * gw, D)), _chk(dsrc, F32, "dsrc", (gh0 * gw0, D)),
         gh0, gw0, gh, gw, D, _stream())


# ---- DINO multi-crop input pipeline (data/datasets.py:80-123) -------------------------------
AUG_IP, AUG_FP = 11, 10


def aug_resized_crop_u8(src, iparams, tmp, dst):
    B, H, W, Cc = src.shape
    S = dst.shape[1]
    if Cc != 3:
        raise L.VitsslError(f"aug_resized_crop: expected channel-last RGB [B,H,W,3], got {tuple(src.shape)}")
    call("vitssl_aug_resized_crop_u8", _chk(src, torch.uint8, "src"), _chk(iparams, torch.int32, "iparams", (B, AUG_IP)),
         _chk(tmp, torch.uint8, "tmp", (B, H, S, 3)), _chk(dst, torch.uint8, "dst", (B, S, S, 3)), B, H, W, S, _stream())


def aug_color_u8(img, iparams, fparams):
    B, S = img.shape[0], img.shape[1]
    call("vitssl_aug_color_u8", _chk(img, torch.uint8, "img", (B, S, S, 3)), _chk(iparams, torch.int32, "iparams", (B, AUG_IP)),
         _chk(fparams, F32, "fparams", (B, AUG_FP)), B, S, _stream())


def aug_blur_to_tensor(img, fparams, out, ksize=7):
    B, S = img.shape[0], img.shape[1]
    call("vitssl_aug_blur_to_tensor", _chk(img, torch.uint8, "img", (B, S, S, 3)), _chk(fparams, F32, "fparams", (B, AUG_FP)),
         _chk(out, F32, "out", (B, 3, S, S)), B, S, ksize, _stream())


# ---- SimMIM / supervised / eval transform lists (utils/train_utils.py:54-68; include/vitssl_transforms.h) ----
TF_IP = 5


def tf_tile_rows(H, W, SH, SW):
    """output rows per workgroup tile of `tf_resized_crop_to_tensor` for this shape; raises where the kernel refuses it"""
    l = L.lib()
    tr = l.vitssl_debug_tf_tile_rows(int(H), int(W), int(SH), int(SW))
    if tr <= 0:
        raise L.VitsslError(f"vitssl_debug_tf_tile_rows failed ({tr}): {l.vitssl_last_error().decode()}")
    return tr


def tf_resized_crop_to_tensor(src, iparams, out):
    """src u8 [B,H,W,3], iparams int32 [B,5] (top, left, h, w, flip; boxes inside the image), out f32 [B,3,SH,SW]"""
    if src is None or src.dim() != 4 or src.shape[3] != 3:
        raise L.VitsslError(f"tf_resized_crop_to_tensor: expected channel-last RGB [B,H,W,3], got {None if src is None else tuple(src.shape)}")
    if out is None or out.dim() != 4:
        raise L.VitsslError(f"tf_resized_crop_to_tensor: expected out [B,3,SH,SW], got {None if out is None else tuple(out.shape)}")
    B, H, W, _ = src.shape
    SH, SW = out.shape[2], out.shape[3]
    call("vitssl_tf_resized_crop_to_tensor", _chk(src, torch.uint8, "src"), _chk(iparams, torch.int32, "iparams", (B, TF_IP)),
         _chk(out, F32, "out", (B, 3, SH, SW)), B, H, W, SH, SW, _stream())


# ---- per-epoch training metrics (utils/metrics.py of the reference; include/vitssl_metrics.h) ----
F64 = torch.float64


def _vp(t):
    return C.c_void_p(t.data_ptr())


RECON_ACC = 4          # squared error, sum of per-patch SSIM, elements, patches
DINO_STATS = 8         # n, mean, M2 of the teacher; the same of the student; cosine sum; |center|^2


def recon_metrics(pred, target, acc, C, P):
    """acc f64 [4] += (sum((clamp(pred, 0, 1) - target)^2), sum over patches of the mean SSIM index, elements, patches) of
    pred / target f32 [n, C*P*P] whose rows are [C, P, P] patches; n == 0 leaves acc untouched."""
    if pred is None or pred.dim() != 2 or pred.shape[1] != C * P * P:
        raise L.VitsslError(f"recon_metrics: expected pred [n, {C}*{P}*{P}], got {None if pred is None else tuple(pred.shape)}")
    n = pred.shape[0]
    a, b, c = _chk(pred, F32, "pred"), _chk(target, F32, "target", (n, C * P * P)), _chk(acc, F64, "acc", (RECON_ACC,))
    ws = _tn_workspace(pred.device, int(L.lib().vitssl_recon_metrics_workspace_floats(n, C, P)))      # shared scratch: launches on one stream are ordered
    call("vitssl_recon_metrics", a, b, c, n, C, P, _vp(ws), ws.numel(), _stream())


def dino_stats(teacher, student, center, out):
    """out f64 [8] = (n, mean, sum((x - mean)^2)) of teacher f32 [G,B,K] and of student f32 [V,B,K], the sum over (g, v, b) of
    their rows' cosine similarities, and |center|^2 (center f32 [K] or None)."""
    if teacher is None or teacher.dim() != 3 or student is None or student.dim() != 3:
        raise L.VitsslError("dino_stats: expected teacher [G,B,K] and student [V,B,K], got "
                            f"{None if teacher is None else tuple(teacher.shape)} and {None if student is None else tuple(student.shape)}")
    G, B, K = teacher.shape
    V = student.shape[0]
    t, s = _chk(teacher, F32, "teacher"), _chk(student, F32, "student", (V, B, K))
    c, o = _opt(center, F32, "center", (K,)), _chk(out, F64, "out", (DINO_STATS,))
    ws = _tn_workspace(teacher.device, int(L.lib().vitssl_dino_stats_workspace_floats(G, V, B, K)))
    call("vitssl_dino_stats", t, s, c, o, G, V, B, K, _vp(ws), ws.numel(), _stream())


# ---- classification loss of the supervised / fine-tune step (include/vitssl_classify.h) ----
I64, I32 = torch.int64, torch.int32


def _classify(who, entry, sizing, between, logits, labels, C, loss_out, pred, counters, bad_labels, dlogits, dbias, label_smoothing,
              ignore_index, upstream, workspace, scalars=(), nullable=False):
    """the checks and the call shared by classify_loss, classify_loss_mix and classify_bce; `between`: the (tensor, dtype, name)
    arguments the entry point takes between `labels` and `B` (`nullable`: one that is None is passed on as NULL); `scalars`: those it
    takes between the smoothing and `ignore_index`"""
    if logits is None or logits.dim() != 2 or not 2 <= int(C) <= logits.shape[1]:
        raise L.VitsslError(f"{who}: expected logits [B, ld] with 2 <= C = {C} <= ld, got {None if logits is None else tuple(logits.shape)}")
    B, ld = logits.shape
    ld_out = 0
    if dlogits is not None:
        if dlogits.dim() != 2 or dlogits.shape[0] != B or dlogits.shape[1] % 64 != 0 or dlogits.shape[1] < C:
            raise L.VitsslError(f"{who}: dlogits must be [{B}, ld_out] with ld_out % 64 == 0 and ld_out >= {C}, got {tuple(dlogits.shape)}")
        ld_out = dlogits.shape[1]
    z, y = _chk(logits, F32, "logits"), _chk(labels, I64, "labels", (B,))
    extra = [(_opt if nullable else _chk)(t, dtype, name, (B,)) for t, dtype, name in between]
    lo, pr = _chk(loss_out, F32, "loss_out", (2,)), _chk(pred, I64, "pred", (B,))
    ct, bl = _chk(counters, I64, "counters", (2,)), _chk(bad_labels, I32, "bad_labels", (1,))
    dl, db = _opt(dlogits, BF16, "dlogits"), _opt(dbias, F32, "dbias", (C,))
    need = int(getattr(L.lib(), sizing)(B, C))
    ws = _tn_workspace(logits.device, need) if workspace is None else workspace      # shared scratch: launches on one stream are ordered
    if workspace is not None:
        _chk(ws, F32, "workspace")
    call(entry, z, y, *extra, B, int(C), ld, float(label_smoothing), *scalars, int(ignore_index), float(upstream), lo, dl, ld_out, db,
         pr, ct, bl, _vp(ws), ws.numel(), _stream())


def classify_loss(logits, labels, C, loss_out, pred, counters, bad_labels, dlogits=None, dbias=None, label_smoothing=0.0,
                  ignore_index=-100, upstream=1.0, workspace=None):
    """nn.CrossEntropyLoss(mean, ignore_index, label_smoothing) on the first C columns of logits f32 [B, ld] (the padded
    classifier GEMM output): loss_out f32 [2] = (sum of the valid rows' losses, n_valid), overwritten; pred i64 [B] = argmax;
    counters i64 [2] += (correct, valid); bad_labels i32 [1] += labels outside [0, C) that are not ignore_index.  With
    dlogits bf16 [B, ld_out] (ld_out % 64 == 0): the zero-padded gradient scaled by upstream / n_valid; dbias f32 [C] += its
    column sums.  `workspace`: f32, at least vitssl_classify_loss_workspace_floats(B, C) (default: the shared scratch)."""
    _classify("classify_loss", "vitssl_classify_loss", "vitssl_classify_loss_workspace_floats", (), logits, labels, C, loss_out, pred,
              counters, bad_labels, dlogits, dbias, label_smoothing, ignore_index, upstream, workspace)


# ---- Mixup / CutMix (include/vitssl_mixup.h) ----
MIX_IP = 6
MIX_COPY, MIX_BLEND, MIX_PASTE = 0, 1, 2


def mix_batch(x, out, iparams, lam):
    """out f32 [B,C,H,W] (another buffer than x) = x mixed row by row: iparams int32 [B,6] = (kind, partner, y0, y1, x0, x1),
    lam f32 [B].  kind 0: out[i] = x[i]; 1: fmaf(lam, x[i], (1 - lam) * x[partner]); 2: x[partner] inside the box, x[i]
    elsewhere.  A partner outside the batch is the row itself, a box is clamped to the image, any other kind copies."""
    if x is None or x.dim() != 4:
        raise L.VitsslError(f"mix_batch: expected x [B,C,H,W], got {None if x is None else tuple(x.shape)}")
    B, Cn, H, W = x.shape
    call("vitssl_mix_batch", _chk(x, F32, "x"), _chk(out, F32, "out", (B, Cn, H, W)), _chk(iparams, I32, "iparams", (B, MIX_IP)),
         _chk(lam, F32, "lam", (B,)), B, Cn, H, W, _stream())


def classify_loss_mix(logits, labels, partner, lam, C, loss_out, pred, counters, bad_labels, dlogits=None, dbias=None,
                      label_smoothing=0.0, ignore_index=-100, upstream=1.0, workspace=None):
    """`classify_loss` against the target lam[i] s(labels[i]) + (1 - lam[i]) s(labels[partner[i]]) of a mixed batch (s: the
    label-smoothed one-hot row): partner int32 [B], lam f32 [B], everything else as there.  A row is ignored when either
    label is ignore_index; it is ignored and counted in bad_labels when its partner is outside [0, B), a label is otherwise
    outside [0, C) or lam is outside [0, 1].  counters[0] counts pred == labels[i], the row's own label."""
    _classify("classify_loss_mix", "vitssl_classify_loss_mix", "vitssl_classify_loss_mix_workspace_floats",
              ((partner, I32, "partner"), (lam, F32, "lam")), logits, labels, C, loss_out, pred, counters, bad_labels, dlogits, dbias,
              label_smoothing, ignore_index, upstream, workspace)


# ---- binary cross-entropy (include/vitssl_bce.h) ----
def classify_bce(logits, labels, C, loss_out, pred, counters, bad_labels, partner=None, lam=None, dlogits=None, dbias=None,
                 smoothing=0.0, target_threshold=None, sum_classes=False, ignore_index=-100, upstream=1.0, workspace=None):
    """timm's BinaryCrossEntropy (the DeiT III loss) with the arguments and the outputs of `classify_loss`: a sigmoid per class
    against t = lam[i] s(labels[i]) + (1 - lam[i]) s(labels[partner[i]]) (s: the label-smoothed one-hot row; partner int32 [B]
    and lam f32 [B] both None: one label per row), t = (t > target_threshold) with a threshold (None: the soft target); a
    row's loss is the mean over its C classes, their sum with `sum_classes`.  Rows, counters and bad_labels as
    `classify_loss` / `classify_loss_mix`."""
    if (partner is None) != (lam is None):
        raise L.VitsslError("classify_bce: partner and lam are either both None (one label per row) or both given")
    thr = -1.0 if target_threshold is None else float(target_threshold)
    if not thr >= 0.0 and target_threshold is not None:
        raise L.VitsslError(f"classify_bce: target_threshold = {target_threshold!r} must be None or a number >= 0")
    _classify("classify_bce", "vitssl_classify_bce", "vitssl_classify_bce_workspace_floats",
              ((partner, I32, "partner"), (lam, F32, "lam")), logits, labels, C, loss_out, pred, counters, bad_labels, dlogits, dbias,
              smoothing, ignore_index, upstream, workspace, scalars=(thr, int(bool(sum_classes))), nullable=True)


# ---- MAE token plumbing and loss (include_ext/vitssl_mae.h) ----
def _mae_shape(who, B, N, K, D):
    B, N, K, D = int(B), int(N), int(K), int(D)
    if B <= 0 or N <= 0 or D <= 0 or D % 4 != 0:
        raise L.VitsslError(f"{who}: B={B}, N={N} must be positive and the width {D} a positive multiple of 4")
    if not 1 <= K <= N - 1:
        raise L.VitsslError(f"{who}: K={K} kept patches outside [1, N-1] with N={N}")
    return B, N, K, D


def mae_tokens_fwd(xk, keep, pos, cls, out, B, N, K):
    """out f32 [B*(K+1), D]: row (b, 0) = cls + pos[0], row (b, 1+j) = xk[b, j] + pos[1 + keep[b, j]]; keep int32 [B, K]"""
    B, N, K, D = _mae_shape("mae_tokens_fwd", B, N, K, xk.shape[-1])
    call("vitssl_mae_tokens_fwd", _chk(xk, F32, "xk", (B * K, D)), _chk(keep, I32, "keep", (B, K)), _chk(pos, F32, "pos", (N + 1, D)),
         _chk(cls, F32, "cls", (D,)), _chk(out, F32, "out", (B * (K + 1), D)), B, N, K, D, _stream())


def mae_tokens_bwd(g, dproj, dbias, dcls, B, N, K):
    """g f32 [B*(K+1), D] -> dproj bf16 [B*K, D] (the patch rows), dbias += their f32 column sum, dcls += that of the CLS rows"""
    B, N, K, D = _mae_shape("mae_tokens_bwd", B, N, K, g.shape[-1])
    call("vitssl_mae_tokens_bwd", _chk(g, F32, "g", (B * (K + 1), D)), _chk(dproj, BF16, "dproj", (B * K, D)), _chk(dbias, F32, "dbias", (D,)),
         _chk(dcls, F32, "dcls", (D,)), B, N, K, D, *_sum_ws(g.device, B * (K + 1), D), _stream())


def mae_unshuffle_fwd(y, restore, mask_token, dpos, out, B, N, K):
    """out f32 [B*(N+1), Dd]: row (b, 0) = y[b, 0] + dpos[0], row (b, 1+n) = (y[b, 1 + restore[b, n]] if restore[b, n] < K else
    mask_token) + dpos[1+n]; restore int32 [B, N]"""
    B, N, K, D = _mae_shape("mae_unshuffle_fwd", B, N, K, y.shape[-1])
    call("vitssl_mae_unshuffle_fwd", _chk(y, F32, "y", (B * (K + 1), D)), _chk(restore, I32, "restore", (B, N)),
         _chk(mask_token, F32, "mask_token", (D,)), _chk(dpos, F32, "dpos", (N + 1, D)), _chk(out, F32, "out", (B * (N + 1), D)),
         B, N, K, D, _stream())


def mae_unshuffle_bwd(g, restore, dy, dbias, dmask_token, B, N, K):
    """g f32 [B*(N+1), Dd] -> dy bf16 [B*(K+1), Dd] (CLS and kept rows, in shuffle order), dbias += their f32 column sum,
    dmask_token += the column sum of the masked rows"""
    B, N, K, D = _mae_shape("mae_unshuffle_bwd", B, N, K, g.shape[-1])
    call("vitssl_mae_unshuffle_bwd", _chk(g, F32, "g", (B * (N + 1), D)), _chk(restore, I32, "restore", (B, N)),
         _chk(dy, BF16, "dy", (B * (K + 1), D)), _chk(dbias, F32, "dbias", (D,)), _chk(dmask_token, F32, "dmask_token", (D,)),
         B, N, K, D, *_sum_ws(g.device, B * (N + 1), D), _stream())


def mae_loss(pred, target, loss_sum, dpred=None, gscale=0.0, norm_pix=True):
    """MSE of pred f32 [Mm, Pd] (contiguous or the column prefix of a wider matrix) against target f32 [Mm, Pd] (contiguous);
    norm_pix: target is first normalised per row, in place ((t - mean) / sqrt(var + 1e-6), unbiased var).  loss_sum f32 [1] += the
    sum of the row means; dpred bf16 [Mm, Pdp >= Pd] = 2 (pred - t) gscale / Pd, zeros behind column Pd."""
    if pred is None or pred.dim() != 2:
        raise L.VitsslError(f"mae_loss: pred must be a matrix, got {None if pred is None else tuple(pred.shape)}")
    rows, cols = pred.shape
    pp, ld = _chk_ld(pred, F32, "pred", rows, cols)
    Pdp = 0
    if dpred is not None:
        if dpred.dim() != 2 or dpred.shape[0] != rows or dpred.shape[1] < cols or dpred.shape[1] % 4 != 0:
            raise L.VitsslError(f"mae_loss: dpred must be [{rows}, Pdp >= {cols}] with Pdp % 4 == 0, got {tuple(dpred.shape)}")
        Pdp = dpred.shape[1]
    if norm_pix and cols < 2:
        raise L.VitsslError("mae_loss: norm_pix needs at least two columns (the unbiased variance of one value is undefined)")
    call("vitssl_mae_loss", pp, ld, _chk(target, F32, "target", (rows, cols)), _chk(loss_sum, F32, "loss_sum", (1,)),
         _opt(dpred, BF16, "dpred"), rows, cols, Pdp, int(bool(norm_pix)), float(gscale), *_sum_ws(pred.device, rows, cols), _stream())


def _mae_rows(entry, dtype, per, src, idx, out, scatter):
    if src is None or src.dim() != 2 or out is None or out.dim() != 2 or src.shape[1] != out.shape[1] or out.shape[1] % per != 0:
        raise L.VitsslError(f"{entry}: src / out must be matrices of one width that is a multiple of {per}, got "
                            f"{None if src is None else tuple(src.shape)} / {None if out is None else tuple(out.shape)}")
    rows, cols = out.shape
    if rows == 0 or (scatter and src.shape[0] == 0):
        raise L.VitsslError(f"{entry}: empty operand")
    call("vitssl_" + entry, _chk(src, dtype, "src"), _chk(idx, I32, "inv" if scatter else "idx", (rows,)), _chk(out, dtype, "out"),
         rows, cols, _stream())


def mae_gather_rows_bf16(src, idx, out):
    """out bf16 [n, cols] = rows idx[i] of src bf16 [*, cols] (cols % 8 == 0)"""
    _mae_rows("mae_gather_rows_bf16", BF16, 8, src, idx, out, False)


def mae_gather_rows_f32(src, idx, out):
    """out f32 [n, cols] = rows idx[i] of src f32 [*, cols] (cols % 4 == 0)"""
    _mae_rows("mae_gather_rows_f32", F32, 4, src, idx, out, False)


def mae_scatter_rows_f32(src, inv, g):
    """g f32 [rows, cols]: row r = row inv[r] of src f32 [*, cols] where inv[r] >= 0, else zeros"""
    _mae_rows("mae_scatter_rows_f32", F32, 4, src, inv, g, True)
