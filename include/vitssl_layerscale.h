/*
 * vitssl_layerscale.h -- C ABI of LayerScale (a learnable per-channel scale gamma on a residual branch; timm's init_values,
 * ls1 / ls2) in libvitssl_hip.so (MI355X, gfx950): the form of the residual GEMM epilogue that multiplies the branch by gamma
 * per column, and the forms of the two kernels that emit the masked bf16 gradient operand that do the same and also sum
 * gamma's gradient.
 *
 * Same library, same conventions as vitssl_hip.h (0 on success, <0 on error with vitssl_last_error(); no allocation;
 * device pointers and workspaces owned by the caller; enqueued on `stream`, never synchronised; every check is made before
 * anything is launched).  Kept in a header of its own so that vitssl_hip.h, vitssl_gemm_t, vitssl_droppath.h and
 * vitssl_version() stay what they are; the Python mirror binds it through vitssl_hip._lib.REGISTRY["layerscale"].
 *
 * Semantics (timm's order, x + drop_path(ls(branch))), in every mode:
 *   x_out = aux + s[row] * gamma[col] * u,      u = drop(acc + bias)       (element dropout: keep ? (acc + bias) / (1 - p) : 0)
 * with s the optional drop-path row scale of vitssl_droppath.h (1 without it).  gamma is a parameter, so the backward needs
 *   d gamma[c] = sum_r s[r] * g_out[r, c] * u[r, c];
 * u exists nowhere once it is fused into the residual store (at gamma = 1e-5 the difference x_out - aux is below the fp32
 * spacing of the residual stream), so a forward that will be followed by a backward also writes u as a bf16 image.
 */
#ifndef VITSSL_LAYERSCALE_H
#define VITSSL_LAYERSCALE_H

#include <stdint.h>

#include "vitssl_droppath.h"
#include "vitssl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Column scales: column c of an [*, cols] matrix is multiplied by gamma[c]. */
typedef struct {
  const float* gamma;   /* f32 [cols], device memory */
  int cols;
} vitssl_colscale_t;

/* vitssl_gemm_bf16_nt for VITSSL_EPI_RESID (any other epilogue: VITSSL_ERR_ARG) with the branch scaled per column, and per row
 * when `rows` is given (NULL: no drop path); cols->cols must equal N:
 *   out0(f32) = fma(keep ? acc + bias : 0, (rs * 1 / (1 - p)) * gamma[c], aux)
 * rs * 1 / (1 - p) is formed exactly as vitssl_gemm_bf16_nt_rows forms it (rs alone with dropout off, 1 / (1 - p) alone without
 * rows, 1 with neither), then rounded once more in its product with gamma[c]: a gamma of ones gives the bits of the _rows launch
 * (or of the plain launch).  A row with rs == 0 stores aux unchanged, bit for bit.
 *   branch_bf16 [M, N] = bf16(keep ? (acc + bias) * 1 / (1 - p) : 0)     written only when the pointer is given (NULL: a forward
 * without a backward); independent of rs and gamma.  An own instantiation of the residual epilogue: the code of the plain and
 * of the _rows launch is what it was. */
int vitssl_gemm_bf16_nt_ls(const vitssl_gemm_t* g, const vitssl_colscale_t* cols, const vitssl_rowscale_t* rows,
                           void* branch_bf16, void* stream);

/* Workspace of the two entry points below, in floats: they write one more column sum than vitssl_layernorm_bwd, so rows of up
 * to 512 columns need more than vitssl_sum_workspace_floats(rows, cols).  Never smaller than that count. */
int64_t vitssl_layerscale_workspace_floats(int64_t rows, int cols);

/* vitssl_layernorm_bwd_rows / vitssl_grad_mask_cast_rows (same arguments; `rowscale` may be NULL here) with the bf16 operand
 * also scaled per column, and gamma's gradient:
 *   gm_bf16 = bf16(gamma[c] * (rs * (keepmask(drop) * g_out / (1 - p))))      (the fp32 operand of the _rows entry, one more fp32
 *   multiply, one bf16 rounding: a gamma of ones gives the _rows bits), gm_colsum summed from those values (the bias sits
 *   inside gamma);
 *   dls[c] += sum over rows with rs != 0 of rs * g_out[r, c] * float(branch_bf16[r, c])      (fp32; a dropped sample contributes
 *   exact zeros, by select), through the same slot rows and the same fixed-order reduce as dgamma, dbeta and gm_colsum, and
 *   accumulated into its target as gm_colsum is.
 * g_out, dgamma and dbeta are untouched by either scale (the same bits as the plain entry).  branch_bf16 and dls are given
 * together or both NULL (no gradient of gamma wanted: a frozen stack).  colscale->cols must equal cols; rows < 2^31; gm_bf16 is
 * required.  The workspace holds at least vitssl_layerscale_workspace_floats(rows, cols) floats (checked before the launch).
 * At 384 columns the LayerNorm form keeps the two-rows-per-wave layout of the plain entry. */
int vitssl_layernorm_bwd_ls(const void* dy_bf16, const float* x, const float* mean, const float* rstd, const float* gamma,
                            const float* g_res, float* g_out, void* gm_bf16, float* dgamma, float* dbeta, float* gm_colsum,
                            vitssl_dropout_t drop, const vitssl_rowscale_t* rowscale, const vitssl_colscale_t* colscale,
                            const void* branch_bf16, float* dls, int64_t rows, int cols, float* workspace,
                            int64_t workspace_floats, void* stream);
int vitssl_grad_mask_cast_ls(const float* g, void* gm_bf16, float* gm_colsum, vitssl_dropout_t drop,
                             const vitssl_rowscale_t* rowscale, const vitssl_colscale_t* colscale, const void* branch_bf16,
                             float* dls, int64_t rows, int cols, float* workspace, int64_t workspace_floats, void* stream);

#ifdef __cplusplus
}
#endif
#endif
