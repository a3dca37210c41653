/*
 * vitssl_mae.h -- C ABI of the MAE (masked autoencoder) token plumbing and loss in libvitssl_hip.so (MI355X, gfx950): the
 * assembly of the encoder's visible tokens, the un-shuffle in front of the decoder, both backwards, the normalised-pixel MSE
 * loss, and three row gathers / scatters that have no counterpart in vitssl_hip.h.
 *
 * An EXTENSION table: same library, same conventions as vitssl_hip.h (0 on success, -1 on an argument error with
 * vitssl_last_error() set; no allocation; device pointers and workspaces owned by the caller; enqueued on `stream`, never
 * synchronised; every check is made before anything is launched, so a refused call writes nothing).  It lives outside include/
 * so that the twelve headers there, their symbol lists and vitssl_version() stay what they are; the Python mirror binds it
 * through vitssl_hip._lib.EXT_REGISTRY["mae"].
 *
 * Shapes: B images, N patches per image, K kept patches per image (1 <= K <= N - 1), D / Dd the encoder / decoder width.
 *   keep     i32 [B, K]   the kept patch indices in shuffle order, each in [0, N)
 *   restore  i32 [B, N]   position of patch n in the shuffle (a permutation of 0 .. N-1 per image); < K means kept
 * INDEX VALUES ARE THE CALLER'S: no entry point validates an index on the device.  A value outside its range reads or writes
 * outside the operand.
 * Every f32 operand is read and written as 16-byte pieces, every bf16 result as 8-byte pieces (16 in the bf16 gather): widths
 * must be multiples of 4 (8 there) and the pointers aligned to the piece; a misaligned pointer is refused.
 * "+=" ACCUMULATES into the target (a slot of the flat gradient buffer, zeroed by the step); everything else is OVERWRITTEN.
 * Column sums follow the deterministic-sum rule of vitssl_hip.h: contiguous runs of at least 32 rows are summed top to bottom,
 * one slot row each in `workspace` (at least vitssl_sum_workspace_floats(rows of the summed matrix, width) floats), and the slots
 * are added in a fixed order.  No float atomics: the same inputs give the same bits.
 */
#ifndef VITSSL_MAE_H
#define VITSSL_MAE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- token assembly ----------------------------------------------------------------------------------------------------------
 * forward   xk f32 [B*K, D] (projection of the kept patches, bias included), pos f32 [N+1, D], cls f32 [D]
 *           out f32 [B*(K+1), D]:  out[b, 0] = cls + pos[0],  out[b, 1+j] = xk[b, j] + pos[1 + keep[b, j]]
 * backward  g f32 [B*(K+1), D]
 *           dproj bf16 [B*K, D] = the patch rows g[b, 1+j] rounded to nearest even
 *           dbias f32 [D] += column sum of the f32 patch rows,  dcls f32 [D] += column sum of the CLS rows g[b, 0]
 *           workspace: vitssl_sum_workspace_floats(B*(K+1), D) floats.  (N only bounds K.) */
int vitssl_mae_tokens_fwd(const float* xk, const int32_t* keep, const float* pos, const float* cls, float* out, int B, int N, int K,
                          int D, void* stream);
int vitssl_mae_tokens_bwd(const float* g, void* dproj_bf16, float* dbias, float* dcls, int B, int N, int K, int D, float* workspace,
                          int64_t workspace_floats, void* stream);

/* ---- un-shuffle ----------------------------------------------------------------------------------------------------------------
 * forward   y f32 [B*(K+1), Dd], mask_token f32 [Dd], dpos f32 [N+1, Dd]
 *           out f32 [B*(N+1), Dd]:  out[b, 0] = y[b, 0] + dpos[0];
 *           out[b, 1+n] = (restore[b, n] < K ? y[b, 1 + restore[b, n]] : mask_token) + dpos[1+n]
 * backward  g f32 [B*(N+1), Dd], read once in its own order through `restore` (row (b, 1+j) of dy is g[b, 1 + keep[b, j]])
 *           dy bf16 [B*(K+1), Dd]:  dy[b, 0] = g[b, 0],  dy[b, 1 + restore[b, n]] = g[b, 1+n] where restore[b, n] < K
 *           dbias f32 [Dd] += column sum of those f32 rows (CLS rows included),
 *           dmask_token f32 [Dd] += column sum of the B*(N-K) other rows of g
 *           workspace: vitssl_sum_workspace_floats(B*(N+1), Dd) floats. */
int vitssl_mae_unshuffle_fwd(const float* y, const int32_t* restore, const float* mask_token, const float* dpos, float* out, int B,
                             int N, int K, int Dd, void* stream);
int vitssl_mae_unshuffle_bwd(const float* g, const int32_t* restore, void* dy_bf16, float* dbias, float* dmask_token, int B, int N,
                             int K, int Dd, float* workspace, int64_t workspace_floats, void* stream);

/* ---- loss: mean squared error against (optionally per-patch normalised) pixels ---------------------------------------------------
 * pred f32 [Mm, Pd] with row stride ld >= Pd; target f32 [Mm, Pd] contiguous, raw pixel patches
 * norm_pix != 0:  mu = mean_c t,  var = sum_c (t - mu)^2 / (Pd - 1) (unbiased, as torch.var),  t <- (t - mu) / sqrt(var + 1e-6);
 *                 `target` is REWRITTEN in place with the fp32 rounding of that value; the loss and the gradient are taken
 *                 against the fp64 value before that rounding.  Pd = 1 is refused then
 * row loss   = mean_c (pred - t)^2;  loss_out f32 [1] += sum of the row losses (the caller divides by Mm)
 * dpred bf16 [Mm, Pdp] (NULL: no gradient) = 2 (pred - t) * gscale / Pd, columns [Pd, Pdp) zero; Pdp >= Pd, Pdp % 4 == 0,
 *                 8-byte aligned
 * One wave per row; rows of up to 4096 columns are read once and kept in registers, longer ones are swept again.  Row
 * arithmetic is fp64.  With Pd % 4 == 0 and ld % 4 == 0 rows move as 16-byte pieces and pred / target must be 16-byte aligned;
 * any other width moves element by element.  workspace: vitssl_sum_workspace_floats(Mm, Pd) floats. */
int vitssl_mae_loss(const float* pred, int64_t ld, float* target, float* loss_out, void* dpred_bf16, int64_t Mm, int Pd, int Pdp,
                    int norm_pix, float gscale, float* workspace, int64_t workspace_floats, void* stream);

/* ---- rows by index ---------------------------------------------------------------------------------------------------------------
 * gather_rows_bf16   out bf16 [n_idx, cols] = src bf16 [*, cols] rows idx[i]     (cols % 8 == 0, 16-byte aligned)
 * gather_rows_f32    out f32  [n_idx, cols] = src f32  [*, cols] rows idx[i]     (cols % 4 == 0, 16-byte aligned)
 * scatter_rows_f32   g   f32  [rows, cols]:  g[r] = inv[r] >= 0 ? src f32 [*, cols] row inv[r] : 0   (every row of g is written) */
int vitssl_mae_gather_rows_bf16(const void* src_bf16, const int32_t* idx, void* out_bf16, int64_t n_idx, int cols, void* stream);
int vitssl_mae_gather_rows_f32(const float* src, const int32_t* idx, float* out, int64_t n_idx, int cols, void* stream);
int vitssl_mae_scatter_rows_f32(const float* src, const int32_t* inv, float* g, int64_t rows, int cols, void* stream);

#ifdef __cplusplus
}
#endif
#endif
