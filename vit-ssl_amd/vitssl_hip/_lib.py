"""ctypes binding of libvitssl_hip.so (C ABI declared in include/vitssl_hip.h).

There is no CPU fallback: if the library is missing or a call fails, this raises."""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VITSSL_LIB") or os.path.join(_HERE, "libvitssl_hip.so")   # VITSSL_LIB: developer override (kernel A/B builds)
HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "include", "vitssl_hip.h"))
TRANSFORMS_HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "include", "vitssl_transforms.h"))
METRICS_HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "include", "vitssl_metrics.h"))
CLASSIFY_HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "include", "vitssl_classify.h"))
ATTENTION_HD_HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "include", "vitssl_attention_hd.h"))
PATCH_HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "include", "vitssl_patch.h"))
OPTIM_HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "include", "vitssl_optim.h"))
MIXUP_HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "include", "vitssl_mixup.h"))
BCE_HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "include", "vitssl_bce.h"))
DROPPATH_HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "include", "vitssl_droppath.h"))
LAYERSCALE_HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "include", "vitssl_layerscale.h"))
LAMB_HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "include", "vitssl_lamb.h"))


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


EPI_BF16, EPI_F32, EPI_GELU, EPI_RESID, EPI_DGELU, EPI_EMBED = range(6)

ABI_VERSION = 3          # vitssl_version(): 2 = vitssl_dino_loss takes the size of its scratch buffer; 3 = the deterministic sums take a workspace
_vp, _i, _i64, _f = C.c_void_p, C.c_int, C.c_int64, C.c_float

# name -> argtypes (restype is always int except the two noted)
PROTOTYPES = {
    "vitssl_dropout_mask": [_vp, _i64, _i64, Dropout, _vp],
    "vitssl_layernorm_fwd": [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i, _f, _vp],
    "vitssl_layernorm_bwd": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, Dropout, _i64, _i, _vp, _i64, _vp],
    "vitssl_grad_mask_cast": [_vp, _vp, _vp, Dropout, _i64, _i, _vp, _i64, _vp],
    "vitssl_gemm_bf16_nt": [C.POINTER(Gemm), _vp],
    "vitssl_gemm_bf16_tn": [_vp, _vp, _vp, _i64, _i, _i, _vp, _i64, _vp],
    "vitssl_gemm_bf16_tn_batch": [C.POINTER(TnJob), _i, _i64, _vp, _i64, _vp],
    "vitssl_gemm_fp8_tn_batch": [C.POINTER(Fp8TnJob), _i, _i64, _vp, _i64, _vp],
    "vitssl_gemm_fp8_nt": [C.POINTER(Gemm), C.POINTER(Fp8Gemm), _vp],
    "vitssl_gemm_fp8_tn": [_vp, _vp, _vp, _i64, _i, _i, _vp, _vp, _vp, _i64, _vp],
    "vitssl_quantize_fp8": [_vp, _vp, _i64, _vp],
    "vitssl_attn_bwd_fp8": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
    "vitssl_quantize_fp8_scaled": [_vp, _vp, _i64, _vp, _vp, _vp],
    "vitssl_layernorm_bwd_fp8": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, Dropout, _i64, _i, _vp, _i64,
                                 _vp],
    "vitssl_grad_mask_cast_fp8": [_vp, _vp, _vp, _vp, _vp, _vp, Dropout, _i64, _i, _vp, _i64, _vp],
    "vitssl_attn_fwd_fp8": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
    "vitssl_layernorm_fwd_fp8": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i, _f, _vp],
    "vitssl_fp8_quantize_weights": [_vp, _vp, _i, _i, _vp, _vp, _vp],
    "vitssl_attn_fwd": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
    "vitssl_attn_bwd": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
    "vitssl_patchify_bf16": [_vp, _vp, _i, _i, _i, _i, _i, _vp],
    "vitssl_gather_patches_f32": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp],
    "vitssl_gather_rows_bf16": [_vp, _vp, _vp, _i, _i, _vp],
    "vitssl_scatter_rows_f32": [_vp, _vp, _vp, _i64, _i, _vp],
    "vitssl_gather_cls_f32": [_vp, _vp, _i, _i, _i, _vp],
    "vitssl_scatter_cls_f32": [_vp, _vp, _i, _i, _i, _vp],
    "vitssl_embed_bwd": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _i64, _vp],
    "vitssl_l1_loss": [_vp, _vp, _vp, _vp, _f, _i64, _vp, _i64, _vp],
    "vitssl_cross_entropy": [_vp, _vp, _vp, _vp, _f, _i, _i, _vp],
    "vitssl_colsum_bf16": [_vp, _vp, _i64, _i, _vp, _i64, _vp],
    "vitssl_cast_bf16": [_vp, _vp, _i64, _vp],
    "vitssl_cast_transpose_bf16": [_vp, _vp, _vp, _i, _i, _vp],
    "vitssl_cast_transpose_batch": [_vp, _vp, _i, _i, _vp],
    "vitssl_bicubic_resize_fwd": [_vp, _vp, _i, _i, _i, _i, _i, _vp],
    "vitssl_bicubic_resize_bwd": [_vp, _vp, _i, _i, _i, _i, _i, _vp],
    "vitssl_aug_resized_crop_u8": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
    "vitssl_aug_color_u8": [_vp, _vp, _vp, _i, _i, _vp],
    "vitssl_aug_blur_to_tensor": [_vp, _vp, _vp, _i, _i, _i, _vp],
    "vitssl_adamw": [_vp, _vp, _vp, _vp, _i64, _f, _f, _f, _f, _f, _i, _f, _vp],
    "vitssl_ema": [_vp, _vp, _i64, _f, _vp],
    "vitssl_rownorm_fwd": [_vp, _vp, _vp, _i64, _i, _vp],
    "vitssl_rownorm_bwd": [_vp, _vp, _vp, _vp, _i64, _i, _vp],
    "vitssl_weightnorm_fold": [_vp, _vp, _vp, _vp, _i, _i, _vp],
    "vitssl_weightnorm_bwd": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp],
    "vitssl_dino_loss": [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _i, _i, _i, _i, _f, _f, _f, _vp],
    "vitssl_colsum_f32": [_vp, _vp, _i64, _i, _vp],
    "vitssl_center_ema": [_vp, _vp, _i, _f, _f, _vp],
    "vitssl_set_reserved_cus": [_i],
}

# include/vitssl_transforms.h (the fused transform-list kernel): same library, a table of its own, so that PROTOTYPES stays
# the mirror of include/vitssl_hip.h.  Launching entry points only; the introspection getter
# vitssl_debug_tf_tile_rows (returns a count) is bound in lib() beside the other vitssl_debug_* getters.
PROTOTYPES_TRANSFORMS = {
    "vitssl_tf_resized_crop_to_tensor": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp],
}

# include/vitssl_metrics.h (per-epoch training metrics): launching entry points; their sizing functions
# vitssl_*_workspace_floats (return a count) are bound in lib() beside the other sizing functions.
PROTOTYPES_METRICS = {
    "vitssl_recon_metrics": [_vp, _vp, _vp, _i64, _i, _i, _vp, _i64, _vp],
    "vitssl_dino_stats": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _i64, _vp],
}

# include/vitssl_classify.h (classification loss of the supervised / fine-tune step): the launching entry point; its sizing
# function vitssl_classify_loss_workspace_floats (returns a count) is bound in lib() beside the other sizing functions.
PROTOTYPES_CLASSIFY = {
    "vitssl_classify_loss": [_vp, _vp, _i, _i, _i, C.c_double, _i64, _f, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i64, _vp],
}

# include/vitssl_attention_hd.h (attention for head dims 8 .. 128 other than the dh = 64 family of vitssl_hip.h): both entry
# points launch; argument order as vitssl_attn_fwd / vitssl_attn_bwd.
PROTOTYPES_ATTENTION_HD = {
    "vitssl_attn_hd_fwd": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
    "vitssl_attn_hd_bwd": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
}

# include/vitssl_patch.h (the patch path for any patch side and channel count: matrices with a row stride whose pad columns
# stay zero): every entry point launches.
PROTOTYPES_PATCH = {
    "vitssl_patchify_ld_bf16": [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp],
    "vitssl_gather_patches_any_f32": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp],
    "vitssl_l1_loss_ld": [_vp, _i64, _vp, _i64, _vp, _vp, _i64, _f, _i64, _i, _vp, _i64, _vp],
    "vitssl_accumulate_ld_f32": [_vp, _vp, _i64, _i, _i64, _vp],
    "vitssl_cast_transpose_batch_ld": [_vp, _vp, _i, _i, _vp],
}

# include/vitssl_optim.h (segmented AdamW: per-parameter lr / weight decay, global-norm clipping): the launching entry points
# and the host-side table builder; the sizing functions vitssl_optim_table_bytes / vitssl_grad_sumsq_workspace_bytes (return a
# count) are bound in lib() beside the other sizing functions.
PROTOTYPES_OPTIM = {
    "vitssl_optim_table_build": [C.POINTER(OptimSegment), _i, _i64, _vp, _i64],
    "vitssl_grad_sumsq": [_vp, _vp, _i, _vp, _vp, _i64, _vp],
    "vitssl_adamw_segments": [_vp, _vp, _vp, _vp, _vp, _i, _f, _f, _f, _f, _i, _f, _vp, _f, _vp],
}

# include/vitssl_mixup.h (Mixup / CutMix: the mix kernel and the classification loss against two-label targets): the launching
# entry points; the sizing function vitssl_classify_loss_mix_workspace_floats (returns a count) is bound in lib() beside the
# other sizing functions.
PROTOTYPES_MIXUP = {
    "vitssl_mix_batch": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
    "vitssl_classify_loss_mix": [_vp, _vp, _vp, _vp, _i, _i, _i, C.c_double, _i64, _f, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i64, _vp],
}

# include/vitssl_droppath.h (stochastic depth: the table of per-sample branch scales and the row-scaled forms of the residual
# GEMM and of the two kernels that emit the masked gradient operand): every entry point launches.
DROPPATH_SITE_BIT = 0x80000000          # VITSSL_DROPPATH_SITE_BIT
DROPPATH_MAX_SITES = 128                # VITSSL_DROPPATH_MAX_SITES
PROTOTYPES_DROPPATH = {
    "vitssl_droppath_table": [_vp, C.POINTER(C.c_float), C.POINTER(C.c_uint32), _i, _i, C.c_uint64, _vp],
    "vitssl_gemm_bf16_nt_rows": [C.POINTER(Gemm), C.POINTER(RowScale), _vp],
    "vitssl_layernorm_bwd_rows": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, Dropout, C.POINTER(RowScale), _i64, _i, _vp,
                                  _i64, _vp],
    "vitssl_grad_mask_cast_rows": [_vp, _vp, _vp, Dropout, C.POINTER(RowScale), _i64, _i, _vp, _i64, _vp],
}

# include/vitssl_layerscale.h (LayerScale: the column-scaled forms of the residual GEMM and of the two kernels that emit the masked
# gradient operand, which also sum gamma's gradient), and the workspace query of those two, which returns an int64 count instead of a status (lib() below).
PROTOTYPES_LAYERSCALE = {
    "vitssl_gemm_bf16_nt_ls": [C.POINTER(Gemm), C.POINTER(ColScale), C.POINTER(RowScale), _vp, _vp],
    "vitssl_layernorm_bwd_ls": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, Dropout, C.POINTER(RowScale), C.POINTER(ColScale),
                                _vp, _vp, _i64, _i, _vp, _i64, _vp],
    "vitssl_grad_mask_cast_ls": [_vp, _vp, _vp, Dropout, C.POINTER(RowScale), C.POINTER(ColScale), _vp, _vp, _i64, _i, _vp, _i64, _vp],
    "vitssl_layerscale_workspace_floats": [C.c_int64, C.c_int],
}

# include/vitssl_lamb.h (segmented LAMB over the table of vitssl_optim.h): the launching entry point, and the host-side sizing
# function of its workspace, which returns an int64 count instead of a status (lib() below).
LAMB_ALWAYS_ADAPT, LAMB_TRUST_CLIP = 1, 2          # VITSSL_LAMB_ALWAYS_ADAPT, VITSSL_LAMB_TRUST_CLIP
PROTOTYPES_LAMB = {
    "vitssl_lamb_workspace_bytes": [C.POINTER(OptimSegment), _i],
    "vitssl_lamb_segments": [_vp, _vp, _vp, _vp, _vp, _i, _f, _f, _f, _f, _i, _f, _vp, _f, _i, _vp, _vp, _i64, _vp],
}

# include/vitssl_bce.h (binary cross-entropy of the supervised / fine-tune step, one- and two-label targets): the launching
# entry point; the sizing function vitssl_classify_bce_workspace_floats (returns a count) is bound in lib() beside the other
# sizing functions.
PROTOTYPES_BCE = {
    "vitssl_classify_bce": [_vp, _vp, _vp, _vp, _i, _i, _i, C.c_double, C.c_double, _i, _i64, _f, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp,
                            _i64, _vp],
}

_lib = None


def header_symbols():
    """Entry points declared in include/vitssl_hip.h (int-returning `vitssl_*` functions)."""
    with open(HEADER_PATH) as f:
        txt = f.read()
    return sorted(set(re.findall(r"\b(vitssl_[a-z0-9_]+)\s*\(", txt)))


def transforms_header_symbols():
    """Entry points declared in include/vitssl_transforms.h."""
    with open(TRANSFORMS_HEADER_PATH) as f:
        txt = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)        # the comments name functions of vitssl_hip.h
    return sorted(set(re.findall(r"\b(vitssl_[a-z0-9_]+)\s*\(", txt)))


def metrics_header_symbols():
    """Entry points and sizing functions declared in include/vitssl_metrics.h."""
    with open(METRICS_HEADER_PATH) as f:
        txt = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)        # the comments name functions in running text
    return sorted(set(re.findall(r"\b(vitssl_[a-z0-9_]+)\s*\(", txt)))


def classify_header_symbols():
    """Entry points and sizing functions declared in include/vitssl_classify.h."""
    with open(CLASSIFY_HEADER_PATH) as f:
        txt = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)        # the comments name functions in running text
    return sorted(set(re.findall(r"\b(vitssl_[a-z0-9_]+)\s*\(", txt)))


def attention_hd_header_symbols():
    """Entry points declared in include/vitssl_attention_hd.h."""
    with open(ATTENTION_HD_HEADER_PATH) as f:
        txt = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)        # the comments name functions of vitssl_hip.h
    return sorted(set(re.findall(r"\b(vitssl_[a-z0-9_]+)\s*\(", txt)))


def patch_header_symbols():
    """Entry points declared in include/vitssl_patch.h."""
    with open(PATCH_HEADER_PATH) as f:
        txt = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)        # the comments name functions of vitssl_hip.h
    return sorted(set(re.findall(r"\b(vitssl_[a-z0-9_]+)\s*\(", txt)))


def optim_header_symbols():
    """Entry points and sizing functions declared in include/vitssl_optim.h."""
    with open(OPTIM_HEADER_PATH) as f:
        txt = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)        # the comments name functions of vitssl_hip.h
    return sorted(set(re.findall(r"\b(vitssl_[a-z0-9_]+)\s*\(", txt)))


def mixup_header_symbols():
    """Entry points and sizing functions declared in include/vitssl_mixup.h."""
    with open(MIXUP_HEADER_PATH) as f:
        txt = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)        # the comments name functions of vitssl_classify.h
    return sorted(set(re.findall(r"\b(vitssl_[a-z0-9_]+)\s*\(", txt)))


def droppath_header_symbols():
    """Entry points declared in include/vitssl_droppath.h."""
    with open(DROPPATH_HEADER_PATH) as f:
        txt = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)        # the comments name functions of vitssl_hip.h
    txt = re.sub(r"^\s*#.*$", "", txt, flags=re.M)                    # and so do the macros
    return sorted(set(re.findall(r"\b(vitssl_[a-z0-9_]+)\s*\(", txt)))


def layerscale_header_symbols():
    """Entry points declared in include/vitssl_layerscale.h (the launching ones and the workspace query)."""
    with open(LAYERSCALE_HEADER_PATH) as f:
        txt = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)        # the comments name functions of the other headers
    txt = re.sub(r"^\s*#.*$", "", txt, flags=re.M)
    return sorted(set(re.findall(r"\b(vitssl_[a-z0-9_]+)\s*\(", txt)))


def lamb_header_symbols():
    """Entry points declared in include/vitssl_lamb.h (the launching one and the workspace sizing function)."""
    with open(LAMB_HEADER_PATH) as f:
        txt = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)        # the comments name functions of the other headers
    txt = re.sub(r"^\s*#.*$", "", txt, flags=re.M)
    return sorted(set(re.findall(r"\b(vitssl_[a-z0-9_]+)\s*\(", txt)))


def bce_header_symbols():
    """Entry points and sizing functions declared in include/vitssl_bce.h."""
    with open(BCE_HEADER_PATH) as f:
        txt = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)        # the comments name functions of the other headers
    return sorted(set(re.findall(r"\b(vitssl_[a-z0-9_]+)\s*\(", txt)))


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
    l.vitssl_last_error.restype = C.c_char_p
    l.vitssl_last_error.argtypes = []
    l.vitssl_version.restype = C.c_int
    l.vitssl_version.argtypes = []
    if l.vitssl_version() != ABI_VERSION:
        raise VitsslError(f"{LIB_PATH} implements C-ABI version {l.vitssl_version()}, these bindings expect {ABI_VERSION}: "
                          "rebuild it (python __graft_entry__.py)")
    l.vitssl_gemm_tn_workspace_floats.restype = C.c_int64
    l.vitssl_gemm_tn_workspace_floats.argtypes = [C.c_int64, C.c_int, C.c_int]
    l.vitssl_gemm_tn_batch_workspace_floats.restype = C.c_int64
    l.vitssl_gemm_tn_batch_workspace_floats.argtypes = [C.POINTER(TnJob), C.c_int, C.c_int64]
    l.vitssl_gemm_fp8_tn_batch_workspace_floats.restype = C.c_int64
    l.vitssl_gemm_fp8_tn_batch_workspace_floats.argtypes = [C.POINTER(Fp8TnJob), C.c_int, C.c_int64]
    l.vitssl_gemm_fp8_tn_workspace_floats.restype = C.c_int64
    l.vitssl_gemm_fp8_tn_workspace_floats.argtypes = [C.c_int64, C.c_int, C.c_int]
    l.vitssl_dino_loss_workspace_floats.restype = C.c_int64
    l.vitssl_dino_loss_workspace_floats.argtypes = [C.c_int, C.c_int, C.c_int]
    l.vitssl_sum_workspace_floats.restype = C.c_int64
    l.vitssl_sum_workspace_floats.argtypes = [C.c_int64, C.c_int]
    l.vitssl_embed_bwd_workspace_floats.restype = C.c_int64
    l.vitssl_embed_bwd_workspace_floats.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    for getter in ("vitssl_get_reserved_cus", "vitssl_debug_last_nt_grid", "vitssl_debug_last_attn_fwd_grid"):
        getattr(l, getter).restype = C.c_int
        getattr(l, getter).argtypes = []
    l.vitssl_debug_tf_tile_rows.restype = C.c_int
    l.vitssl_debug_tf_tile_rows.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    l.vitssl_recon_metrics_workspace_floats.restype = C.c_int64
    l.vitssl_recon_metrics_workspace_floats.argtypes = [C.c_int64, C.c_int, C.c_int]
    l.vitssl_dino_stats_workspace_floats.restype = C.c_int64
    l.vitssl_dino_stats_workspace_floats.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    l.vitssl_classify_loss_workspace_floats.restype = C.c_int64
    l.vitssl_classify_loss_workspace_floats.argtypes = [C.c_int, C.c_int]
    l.vitssl_classify_loss_mix_workspace_floats.restype = C.c_int64
    l.vitssl_classify_loss_mix_workspace_floats.argtypes = [C.c_int, C.c_int]
    l.vitssl_classify_bce_workspace_floats.restype = C.c_int64
    l.vitssl_classify_bce_workspace_floats.argtypes = [C.c_int, C.c_int]
    for sizing in ("vitssl_optim_table_bytes", "vitssl_grad_sumsq_workspace_bytes"):
        getattr(l, sizing).restype = C.c_int64
        getattr(l, sizing).argtypes = [C.c_int]
    for name, args in (list(PROTOTYPES.items()) + list(PROTOTYPES_TRANSFORMS.items()) + list(PROTOTYPES_METRICS.items())
                       + list(PROTOTYPES_CLASSIFY.items()) + list(PROTOTYPES_ATTENTION_HD.items()) + list(PROTOTYPES_PATCH.items())
                       + list(PROTOTYPES_OPTIM.items()) + list(PROTOTYPES_MIXUP.items()) + list(PROTOTYPES_DROPPATH.items())
                       + list(PROTOTYPES_LAYERSCALE.items()) + list(PROTOTYPES_LAMB.items()) + list(PROTOTYPES_BCE.items())):
        fn = getattr(l, name)  # AttributeError if the symbol is missing
        fn.restype = C.c_int
        fn.argtypes = args
    l.vitssl_layerscale_workspace_floats.restype = C.c_int64
    l.vitssl_lamb_workspace_bytes.restype = C.c_int64
    _lib = l
    return l


def call(name, *args):
    l = lib()
    rc = getattr(l, name)(*args)
    if rc != 0:
        raise VitsslError(f"{name} failed ({rc}): {l.vitssl_last_error().decode()}")
