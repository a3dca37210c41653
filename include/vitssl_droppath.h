/*
 * vitssl_droppath.h -- C ABI of stochastic depth (drop path) in libvitssl_hip.so (MI355X, gfx950): the table of per-sample
 * branch scales, and the forms of the residual GEMM epilogue and of the two kernels that emit the masked bf16 gradient
 * operand that multiply a whole row by its sample's scale.
 *
 * Same library, same conventions as vitssl_hip.h (0 on success, <0 on error with vitssl_last_error(); no allocation;
 * device pointers and workspaces owned by the caller; enqueued on `stream`, never synchronised; every check is made before
 * anything is launched).  Kept in a header of its own so that vitssl_hip.h, vitssl_gemm_t and vitssl_version() stay what they
 * are; the Python mirror binds it through vitssl_hip._lib.REGISTRY["droppath"].
 *
 * Semantics (timm's DropPath, per sample, scale_by_keep): in training mode a residual branch of block i is multiplied, for
 * every sample b of the batch, by s[b] = keep[b] ? 1 / (1 - r_eff) : 0, with r_eff = round(r * 65536) / 65536 (the dropout
 * stream's rule) and the scale its exact fp32 reciprocal 65536 / (65536 - round(r * 65536)).  keep[b] is the keep bit of the
 * dropout stream of vitssl_hip.h (vitssl_dropout_t) for element b of a [1, B] tensor at (seed, site).
 *
 * Sites.  Element dropout of an encoder stack uses the sites site_base + 3 * block + which (which = 0, 1, 2), small numbers.
 * Drop path uses VITSSL_DROPPATH_SITE(block, branch) = 0x80000000 | (2 * block + branch), branch 0 = attention, 1 = MLP:
 * the high bit is set in no dropout site of any stack, so the two families never share a stream.  (A caller that runs several
 * stacks in one model adds each stack's site_base to the low bits of both families: engine.EncoderStack does.)  Two passes of
 * one stack in one step (DINO's student) differ in their seed, as their dropout does.
 */
#ifndef VITSSL_DROPPATH_H
#define VITSSL_DROPPATH_H

#include <stdint.h>

#include "vitssl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VITSSL_DROPPATH_SITE_BIT 0x80000000u
#define VITSSL_DROPPATH_SITE(block, branch) (VITSSL_DROPPATH_SITE_BIT | (uint32_t)(2 * (block) + (branch)))

/* scale f32 [sites, B]: row j holds the scales of the B samples for (rates[j], site_ids[j], seed):
 *   scale[j][b] = keep(seed, site_ids[j], element b of [1, B], rates[j]) ? 65536 / (65536 - round(rates[j] * 65536)) : 0
 * A rate of 0 (or below) gives a row of ones.  `rates` (f32 [sites]) and `site_ids` (u32 [sites]) are HOST arrays read
 * during the call (sites <= VITSSL_DROPPATH_MAX_SITES; they travel as kernel arguments): one launch, no host read of device
 * memory.  Rates must be < 1; B >= 1. */
#define VITSSL_DROPPATH_MAX_SITES 128
int vitssl_droppath_table(float* scale, const float* rates, const uint32_t* site_ids, int sites, int B, uint64_t seed,
                          void* stream);

/* Row scales: row m of an [M, *] matrix is multiplied by scale[m / rows_per_group]; scale holds `groups` floats and
 * groups * rows_per_group == M is checked.  (One row of the table above with rows_per_group = tokens per sample.) */
typedef struct {
  const float* scale;   /* f32 [groups], device memory */
  int64_t groups;
  int rows_per_group;
} vitssl_rowscale_t;

/* vitssl_gemm_bf16_nt for VITSSL_EPI_RESID (any other epilogue: VITSSL_ERR_ARG) with the branch scaled per row:
 *   out0(f32) = aux + scale[row / rows_per_group] * drop(acc + bias)
 * computed as fma(keep ? acc + bias : 0, scale * 1 / (1 - p), aux): one rounding of the product of the two scales, one of the
 * fma; a table of ones gives the bits of vitssl_gemm_bf16_nt.  A row whose scale is 0 stores aux unchanged, bit for bit
 * (whatever acc holds).  An own instantiation of the residual epilogue: the code of the plain launch is what it was. */
int vitssl_gemm_bf16_nt_rows(const vitssl_gemm_t* g, const vitssl_rowscale_t* rows, void* stream);

/* vitssl_layernorm_bwd / vitssl_grad_mask_cast (same arguments, same workspace) with the bf16 operand scaled per row:
 *   gm_bf16 = bf16(scale[row / rows_per_group] * (keepmask(drop) * g_out / (1 - p)))     (the fp32 operand of the plain entry,
 *   then one more fp32 multiply), gm_colsum summed from those values;
 * g_out, dgamma and dbeta are untouched by the scale (the same bits as the plain entry).  rows < 2^31.  gm_bf16 is required. */
int vitssl_layernorm_bwd_rows(const void* dy_bf16, const float* x, const float* mean, const float* rstd, const float* gamma,
                              const float* g_res, float* g_out, void* gm_bf16, float* dgamma, float* dbeta, float* gm_colsum,
                              vitssl_dropout_t drop, const vitssl_rowscale_t* rowscale, int64_t rows, int cols,
                              float* workspace, int64_t workspace_floats, void* stream);
int vitssl_grad_mask_cast_rows(const float* g, void* gm_bf16, float* gm_colsum, vitssl_dropout_t drop,
                               const vitssl_rowscale_t* rowscale, int64_t rows, int cols, float* workspace,
                               int64_t workspace_floats, void* stream);

#ifdef __cplusplus
}
#endif
#endif
