"""ctypes binding of libvitssl_hip.so (C ABI declared in include/vitssl_hip.h).

There is no CPU fallback: if the library is missing or a call fails, this raises."""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VITSSL_LIB") or os.path.join(_HERE, "libvitssl_hip.so")   # VITSSL_LIB: developer override (kernel A/B builds)
_INCLUDE = os.path.normpath(os.path.join(_HERE, "..", "..", "include"))
# header key -> file, in the order the headers were added; REGISTRY below has one table per key
HEADERS = {key: os.path.join(_INCLUDE, f"vitssl_{key}.h")
           for key in ("hip", "transforms", "metrics", "classify", "attention_hd", "patch", "optim", "mixup", "droppath", "layerscale",
                       "lamb", "bce")}
# extension tables: entry points of the same library declared outside include/ (HEADERS, REGISTRY and STRUCTS above stay the
# twelve-header ABI); EXT_REGISTRY below has one table per key
_INCLUDE_EXT = os.path.normpath(os.path.join(_HERE, "..", "..", "include_ext"))
EXT_HEADERS = {"mae": os.path.join(_INCLUDE_EXT, "vitssl_mae.h")}
# add-on tables: every vitssl_<key>.h under include_addons/, keys from the directory listing in sorted order (the two
# directories above are pinned by their tests; a new feature adds its header here and its table to _ADDON_ABI below);
# ADDON_REGISTRY below has one table per key
_INCLUDE_ADDONS = os.path.normpath(os.path.join(_HERE, "..", "..", "include_addons"))
ADDON_HEADERS = {m.group(1): os.path.join(_INCLUDE_ADDONS, m.group(0))
                 for m in (re.fullmatch(r"vitssl_(\w+)\.h", f) for f in sorted(os.listdir(_INCLUDE_ADDONS))) if m}


class VitsslError(RuntimeError):
    pass


class Dropout(C.Structure):
    _fields_ = [("p", C.c_float), ("site", C.c_uint32), ("seed", C.c_uint64)]


class Embed(C.Structure):
    _fields_ = [("mask", C.c_void_p), ("mask_token", C.c_void_p), ("pos", C.c_void_p),
                ("tokens", C.c_int), ("out_tokens", C.c_int), ("tok_offset", C.c_int)]


class TnJob(C.Structure):
    """vitssl_tn_job_t"""
    _fields_ = [("A", C.c_void_p), ("B", C.c_void_p), ("C", C.c_void_p), ("N1", C.c_int), ("N2", C.c_int)]


class Fp8TnJob(C.Structure):
    """vitssl_fp8_tn_job_t"""
    _fields_ = [("A8", C.c_void_p), ("B8", C.c_void_p), ("C", C.c_void_p), ("N1", C.c_int), ("N2", C.c_int),
                ("alpha", C.c_void_p), ("alpha2", C.c_void_p)]


class OptimSegment(C.Structure):
    """vitssl_optim_segment_t"""
    _fields_ = [("offset", C.c_int64), ("n", C.c_int64), ("lr_scale", C.c_float), ("weight_decay", C.c_float)]


class RowScale(C.Structure):
    """vitssl_rowscale_t"""
    _fields_ = [("scale", C.c_void_p), ("groups", C.c_int64), ("rows_per_group", C.c_int)]


class ColScale(C.Structure):
    """vitssl_colscale_t"""
    _fields_ = [("gamma", C.c_void_p), ("cols", C.c_int)]


class Gemm(C.Structure):
    _fields_ = [("A", C.c_void_p), ("B", C.c_void_p), ("M", C.c_int64), ("N", C.c_int), ("K", C.c_int),
                ("epilogue", C.c_int), ("bias", C.c_void_p), ("aux", C.c_void_p), ("out0", C.c_void_p),
                ("out1", C.c_void_p), ("colsum", C.c_void_p), ("drop", Dropout), ("embed", Embed),
                ("workspace", C.c_void_p), ("workspace_floats", C.c_int64)]


class Fp8Gemm(C.Structure):
    _fields_ = [("alpha", C.c_void_p), ("alpha2", C.c_void_p), ("out_fp8", C.c_void_p), ("out_scale", C.c_void_p),
                ("out_amax", C.c_void_p)]


class CastJob(C.Structure):
    """vitssl_cast_job_t"""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("dst_t", C.c_void_p), ("R", C.c_int), ("C", C.c_int)]


class CastLdJob(C.Structure):
    """vitssl_cast_ld_job_t"""
    _fields_ = CastJob._fields_ + [("ld_dst", C.c_int), ("ld_dst_t", C.c_int)]


class Fp8WeightJob(C.Structure):
    """vitssl_fp8_weight_job_t"""
    _fields_ = [("src", C.c_void_p), ("dst_fp8", C.c_void_p), ("dst_t_fp8", C.c_void_p), ("R", C.c_int), ("C", C.c_int)]


# C struct name -> its mirror (tests/test_abi_mirror_host.py compares every layout with the compiled headers)
STRUCTS = {"vitssl_dropout_t": Dropout, "vitssl_embed_t": Embed, "vitssl_gemm_t": Gemm, "vitssl_fp8_gemm_t": Fp8Gemm,
           "vitssl_fp8_weight_job_t": Fp8WeightJob, "vitssl_tn_job_t": TnJob, "vitssl_fp8_tn_job_t": Fp8TnJob,
           "vitssl_cast_job_t": CastJob, "vitssl_cast_ld_job_t": CastLdJob, "vitssl_optim_segment_t": OptimSegment,
           "vitssl_rowscale_t": RowScale, "vitssl_colscale_t": ColScale}

EPI_BF16, EPI_F32, EPI_GELU, EPI_RESID, EPI_DGELU, EPI_EMBED = range(6)

ABI_VERSION = 3          # vitssl_version(): 2 = vitssl_dino_loss takes the size of its scratch buffer; 3 = the deterministic sums take a workspace
_vp, _i, _i64, _f, _d = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_double
_pGemm, _pRows, _pCols = C.POINTER(Gemm), C.POINTER(RowScale), C.POINTER(ColScale)


def _returns(restype, *argtypes):
    return restype, list(argtypes)


# The whole C ABI: header key -> function name -> argtypes, for an entry point that returns a status (the common case), or
# _returns(restype, *argtypes) for one that returns something else: a count, a size, text.  One line per declaration of the
# header; lib() binds every entry and tests/test_abi_mirror_host.py compares every one with the header's declaration.
_ABI = {
    # include/vitssl_hip.h
    "hip": {
        "vitssl_last_error": _returns(C.c_char_p),
        "vitssl_version": _returns(_i),
        "vitssl_set_reserved_cus": [_i],
        "vitssl_get_reserved_cus": _returns(_i),
        "vitssl_debug_last_nt_grid": _returns(_i),
        "vitssl_debug_last_attn_fwd_grid": _returns(_i),
        "vitssl_dropout_mask": [_vp, _i64, _i64, Dropout, _vp],
        "vitssl_layernorm_fwd": [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i, _f, _vp],
        "vitssl_layernorm_bwd": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, Dropout, _i64, _i, _vp, _i64, _vp],
        "vitssl_grad_mask_cast": [_vp, _vp, _vp, Dropout, _i64, _i, _vp, _i64, _vp],
        "vitssl_gemm_bf16_nt": [_pGemm, _vp],
        "vitssl_gemm_fp8_nt": [_pGemm, C.POINTER(Fp8Gemm), _vp],
        "vitssl_attn_fwd_fp8": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
        "vitssl_gemm_fp8_tn_workspace_floats": _returns(_i64, _i64, _i, _i),
        "vitssl_gemm_fp8_tn": [_vp, _vp, _vp, _i64, _i, _i, _vp, _vp, _vp, _i64, _vp],
        "vitssl_attn_bwd_fp8": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
        "vitssl_quantize_fp8": [_vp, _vp, _i64, _vp],
        "vitssl_quantize_fp8_scaled": [_vp, _vp, _i64, _vp, _vp, _vp],
        "vitssl_layernorm_fwd_fp8": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i, _f, _vp],
        "vitssl_layernorm_bwd_fp8": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, Dropout, _i64, _i, _vp,
                                     _i64, _vp],
        "vitssl_grad_mask_cast_fp8": [_vp, _vp, _vp, _vp, _vp, _vp, Dropout, _i64, _i, _vp, _i64, _vp],
        "vitssl_fp8_quantize_weights": [_vp, _vp, _i, _i, _vp, _vp, _vp],
        "vitssl_gemm_tn_workspace_floats": _returns(_i64, _i64, _i, _i),
        "vitssl_gemm_bf16_tn": [_vp, _vp, _vp, _i64, _i, _i, _vp, _i64, _vp],
        "vitssl_gemm_tn_batch_workspace_floats": _returns(_i64, C.POINTER(TnJob), _i, _i64),
        "vitssl_gemm_bf16_tn_batch": [C.POINTER(TnJob), _i, _i64, _vp, _i64, _vp],
        "vitssl_gemm_fp8_tn_batch_workspace_floats": _returns(_i64, C.POINTER(Fp8TnJob), _i, _i64),
        "vitssl_gemm_fp8_tn_batch": [C.POINTER(Fp8TnJob), _i, _i64, _vp, _i64, _vp],
        "vitssl_attn_fwd": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
        "vitssl_attn_bwd": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
        "vitssl_patchify_bf16": [_vp, _vp, _i, _i, _i, _i, _i, _vp],
        "vitssl_gather_patches_f32": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp],
        "vitssl_gather_rows_bf16": [_vp, _vp, _vp, _i, _i, _vp],
        "vitssl_scatter_rows_f32": [_vp, _vp, _vp, _i64, _i, _vp],
        "vitssl_gather_cls_f32": [_vp, _vp, _i, _i, _i, _vp],
        "vitssl_scatter_cls_f32": [_vp, _vp, _i, _i, _i, _vp],
        "vitssl_embed_bwd_workspace_floats": _returns(_i64, _i, _i, _i, _i),
        "vitssl_embed_bwd": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _i64, _vp],
        "vitssl_l1_loss": [_vp, _vp, _vp, _vp, _f, _i64, _vp, _i64, _vp],
        "vitssl_cross_entropy": [_vp, _vp, _vp, _vp, _f, _i, _i, _vp],
        "vitssl_colsum_bf16": [_vp, _vp, _i64, _i, _vp, _i64, _vp],
        "vitssl_sum_workspace_floats": _returns(_i64, _i64, _i),
        "vitssl_cast_bf16": [_vp, _vp, _i64, _vp],
        "vitssl_cast_transpose_bf16": [_vp, _vp, _vp, _i, _i, _vp],
        "vitssl_cast_transpose_batch": [_vp, _vp, _i, _i, _vp],
        "vitssl_adamw": [_vp, _vp, _vp, _vp, _i64, _f, _f, _f, _f, _f, _i, _f, _vp],
        "vitssl_ema": [_vp, _vp, _i64, _f, _vp],
        "vitssl_rownorm_fwd": [_vp, _vp, _vp, _i64, _i, _vp],
        "vitssl_rownorm_bwd": [_vp, _vp, _vp, _vp, _i64, _i, _vp],
        "vitssl_weightnorm_fold": [_vp, _vp, _vp, _vp, _i, _i, _vp],
        "vitssl_weightnorm_bwd": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp],
        "vitssl_dino_loss_workspace_floats": _returns(_i64, _i, _i, _i),
        "vitssl_dino_loss": [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _i, _i, _i, _i, _f, _f, _f, _vp],
        "vitssl_colsum_f32": [_vp, _vp, _i64, _i, _vp],
        "vitssl_center_ema": [_vp, _vp, _i, _f, _f, _vp],
        "vitssl_bicubic_resize_fwd": [_vp, _vp, _i, _i, _i, _i, _i, _vp],
        "vitssl_bicubic_resize_bwd": [_vp, _vp, _i, _i, _i, _i, _i, _vp],
        "vitssl_aug_resized_crop_u8": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
        "vitssl_aug_color_u8": [_vp, _vp, _vp, _i, _i, _vp],
        "vitssl_aug_blur_to_tensor": [_vp, _vp, _vp, _i, _i, _i, _vp],
    },
    # include/vitssl_transforms.h: the fused transform-list kernel and its introspection getter
    "transforms": {
        "vitssl_tf_resized_crop_to_tensor": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp],
        "vitssl_debug_tf_tile_rows": _returns(_i, _i, _i, _i, _i),
    },
    # include/vitssl_metrics.h: per-epoch training metrics
    "metrics": {
        "vitssl_recon_metrics_workspace_floats": _returns(_i64, _i64, _i, _i),
        "vitssl_recon_metrics": [_vp, _vp, _vp, _i64, _i, _i, _vp, _i64, _vp],
        "vitssl_dino_stats_workspace_floats": _returns(_i64, _i, _i, _i, _i),
        "vitssl_dino_stats": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _i64, _vp],
    },
    # include/vitssl_classify.h: classification loss of the supervised / fine-tune step
    "classify": {
        "vitssl_classify_loss_workspace_floats": _returns(_i64, _i, _i),
        "vitssl_classify_loss": [_vp, _vp, _i, _i, _i, _d, _i64, _f, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i64, _vp],
    },
    # include/vitssl_attention_hd.h: attention for head dims 8 .. 128 other than the dh = 64 family of vitssl_hip.h; argument
    # order as vitssl_attn_fwd / vitssl_attn_bwd
    "attention_hd": {
        "vitssl_attn_hd_fwd": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
        "vitssl_attn_hd_bwd": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
    },
    # include/vitssl_patch.h: the patch path for any patch side and channel count (matrices with a row stride whose pad columns
    # stay zero)
    "patch": {
        "vitssl_patchify_ld_bf16": [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp],
        "vitssl_gather_patches_any_f32": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp],
        "vitssl_l1_loss_ld": [_vp, _i64, _vp, _i64, _vp, _vp, _i64, _f, _i64, _i, _vp, _i64, _vp],
        "vitssl_accumulate_ld_f32": [_vp, _vp, _i64, _i, _i64, _vp],
        "vitssl_cast_transpose_batch_ld": [_vp, _vp, _i, _i, _vp],
    },
    # include/vitssl_optim.h: segmented AdamW (per-parameter lr / weight decay, global-norm clipping) and its host-side table builder
    "optim": {
        "vitssl_optim_table_bytes": _returns(_i64, _i),
        "vitssl_optim_table_build": [C.POINTER(OptimSegment), _i, _i64, _vp, _i64],
        "vitssl_grad_sumsq_workspace_bytes": _returns(_i64, _i),
        "vitssl_grad_sumsq": [_vp, _vp, _i, _vp, _vp, _i64, _vp],
        "vitssl_adamw_segments": [_vp, _vp, _vp, _vp, _vp, _i, _f, _f, _f, _f, _i, _f, _vp, _f, _vp],
    },
    # include/vitssl_mixup.h: Mixup / CutMix (the mix kernel and the classification loss against two-label targets)
    "mixup": {
        "vitssl_mix_batch": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
        "vitssl_classify_loss_mix_workspace_floats": _returns(_i64, _i, _i),
        "vitssl_classify_loss_mix": [_vp, _vp, _vp, _vp, _i, _i, _i, _d, _i64, _f, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i64, _vp],
    },
    # include/vitssl_droppath.h: stochastic depth (the table of per-sample branch scales and the row-scaled forms of the residual
    # GEMM and of the two kernels that emit the masked gradient operand)
    "droppath": {
        "vitssl_droppath_table": [_vp, C.POINTER(C.c_float), C.POINTER(C.c_uint32), _i, _i, C.c_uint64, _vp],
        "vitssl_gemm_bf16_nt_rows": [_pGemm, _pRows, _vp],
        "vitssl_layernorm_bwd_rows": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, Dropout, _pRows, _i64, _i, _vp, _i64, _vp],
        "vitssl_grad_mask_cast_rows": [_vp, _vp, _vp, Dropout, _pRows, _i64, _i, _vp, _i64, _vp],
    },
    # include/vitssl_layerscale.h: LayerScale (the column-scaled forms of the same three, which also sum gamma's gradient)
    "layerscale": {
        "vitssl_gemm_bf16_nt_ls": [_pGemm, _pCols, _pRows, _vp, _vp],
        "vitssl_layerscale_workspace_floats": _returns(_i64, _i64, _i),
        "vitssl_layernorm_bwd_ls": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, Dropout, _pRows, _pCols, _vp, _vp, _i64, _i,
                                    _vp, _i64, _vp],
        "vitssl_grad_mask_cast_ls": [_vp, _vp, _vp, Dropout, _pRows, _pCols, _vp, _vp, _i64, _i, _vp, _i64, _vp],
    },
    # include/vitssl_lamb.h: segmented LAMB over the table of vitssl_optim.h
    "lamb": {
        "vitssl_lamb_workspace_bytes": _returns(_i64, C.POINTER(OptimSegment), _i),
        "vitssl_lamb_segments": [_vp, _vp, _vp, _vp, _vp, _i, _f, _f, _f, _f, _i, _f, _vp, _f, _i, _vp, _vp, _i64, _vp],
    },
    # include/vitssl_bce.h: binary cross-entropy of the supervised / fine-tune step, one- and two-label targets
    "bce": {
        "vitssl_classify_bce_workspace_floats": _returns(_i64, _i, _i),
        "vitssl_classify_bce": [_vp, _vp, _vp, _vp, _i, _i, _i, _d, _d, _i, _i64, _f, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i64, _vp],
    },
}
# header key -> function name -> (restype, argtypes)
REGISTRY = {key: {name: p if isinstance(p, tuple) else (C.c_int, p) for name, p in table.items()} for key, table in _ABI.items()}

_EXT_ABI = {
    # include_ext/vitssl_mae.h: MAE token assembly, un-shuffle, normalised-pixel MSE loss, rows by index
    "mae": {
        "vitssl_mae_tokens_fwd": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
        "vitssl_mae_tokens_bwd": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _i64, _vp],
        "vitssl_mae_unshuffle_fwd": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
        "vitssl_mae_unshuffle_bwd": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _i64, _vp],
        "vitssl_mae_loss": [_vp, _i64, _vp, _vp, _vp, _i64, _i, _i, _i, _f, _vp, _i64, _vp],
        "vitssl_mae_gather_rows_bf16": [_vp, _vp, _vp, _i64, _i, _vp],
        "vitssl_mae_gather_rows_f32": [_vp, _vp, _vp, _i64, _i, _vp],
        "vitssl_mae_scatter_rows_f32": [_vp, _vp, _vp, _i64, _i, _vp],
    },
}
# extension key -> function name -> (restype, argtypes), the form of REGISTRY
EXT_REGISTRY = {key: {name: p if isinstance(p, tuple) else (C.c_int, p) for name, p in table.items()} for key, table in _EXT_ABI.items()}

_ADDON_ABI = {
    # include_addons/vitssl_pool.h: global average pooling of the patch tokens on the fp32 stream, forward and backward
    "pool": {
        "vitssl_pool_tokens_fwd": [_vp, _vp, _i, _i, _i, _vp],
        "vitssl_pool_tokens_bwd": [_vp, _vp, _i, _i, _i, _vp],
    },
}
# add-on key -> function name -> (restype, argtypes), the form of REGISTRY; a header without a table in _ADDON_ABI is a KeyError
ADDON_REGISTRY = {key: {name: p if isinstance(p, tuple) else (C.c_int, p) for name, p in _ADDON_ABI[key].items()} for key in ADDON_HEADERS}

DROPPATH_SITE_BIT = 0x80000000          # VITSSL_DROPPATH_SITE_BIT
DROPPATH_MAX_SITES = 128                # VITSSL_DROPPATH_MAX_SITES
LAMB_ALWAYS_ADAPT, LAMB_TRUST_CLIP = 1, 2          # VITSSL_LAMB_ALWAYS_ADAPT, VITSSL_LAMB_TRUST_CLIP

_lib = None


def header_path(key):
    """include/vitssl_<key>.h, include_ext/vitssl_<key>.h for an extension key, include_addons/vitssl_<key>.h for an add-on key."""
    for table in (HEADERS, EXT_HEADERS):
        if key in table:
            return table[key]
    return ADDON_HEADERS[key]


def header_text(key):
    """The header without its block comments, line comments and preprocessor lines: what is left are declarations."""
    with open(header_path(key)) as f:
        txt = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)        # the comments name functions of other headers in running text
    return re.sub(r"//.*$|^\s*#.*$", "", txt, flags=re.M)            # and so do the macros


def declarations(key="hip"):
    """Functions declared in include/vitssl_<key>.h: name -> (return type, [parameter types]), C types spelled as in the
    header with the parameter names dropped and no space before a `*`."""
    def ctype(s):
        return re.sub(r"\s*\*", "*", " ".join(s.split()))
    decls = {}
    for ret, name, params in re.findall(r"(?<=[;{}])\s*([A-Za-z_][\w\s*]*?)\b(vitssl_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", header_text(key)):
        params = [] if params.strip() == "void" else [ctype(re.sub(r"\w+\s*$", "", p)) for p in params.split(",")]
        decls[name] = (ctype(ret), params)
    return decls


def header_symbols(key="hip"):
    """Names of the functions declared in include/vitssl_<key>.h."""
    return sorted(declarations(key))


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise VitsslError(
            f"{LIB_PATH} not found: the HIP library is not built. Run `python __graft_entry__.py` "
            "(or __graft_entry__.build()). There is no CPU fallback for the vit_core hot path.")
    # PyTorch-ROCm bundles its own libamdhip64; the process must end up with ONE HIP runtime
    # (device pointers and streams cross this boundary).  Loading torch first makes the
    # dynamic loader satisfy this library's libamdhip64.so.7 dependency with torch's copy;
    # the other order pulls in /opt/rocm's runtime as a second instance and every launch fails
    # with "no ROCm-capable device is detected" (seen with build() followed by smoke()).
    import torch  # noqa: F401
    l = C.CDLL(LIB_PATH)
    if l.vitssl_version() != ABI_VERSION:        # int vitssl_version(void): ctypes' defaults call it right before anything is bound
        raise VitsslError(f"{LIB_PATH} implements C-ABI version {l.vitssl_version()}, these bindings expect {ABI_VERSION}: "
                          "rebuild it (python __graft_entry__.py)")
    # the extension tables after the registry, the add-on tables after those
    for table in list(REGISTRY.values()) + list(EXT_REGISTRY.values()) + list(ADDON_REGISTRY.values()):
        for name, (restype, argtypes) in table.items():
            fn = getattr(l, name)  # AttributeError if the symbol is missing
            fn.restype, fn.argtypes = restype, argtypes
    _lib = l
    return l


def call(name, *args):
    l = lib()
    rc = getattr(l, name)(*args)
    if rc != 0:
        raise VitsslError(f"{name} failed ({rc}): {l.vitssl_last_error().decode()}")
