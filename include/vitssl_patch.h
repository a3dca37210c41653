/*
 * vitssl_patch.h -- C ABI of the patch path for any patch side and channel count of libvitssl_hip.so (MI355X, gfx950).
 *
 * Same library, same conventions as vitssl_hip.h (0 on success, <0 on error with vitssl_last_error() naming the offending
 * argument; no allocation; device pointers and workspaces owned by the caller; enqueued on `stream`, never synchronised;
 * every limit is checked before anything is launched).  Kept in a header of its own so that the symbol list of vitssl_hip.h
 * and vitssl_version() stay what they are; the Python mirror binds these through vitssl_hip._lib.REGISTRY["patch"].
 *
 * vitssl_patchify_bf16 / vitssl_gather_patches_f32 of vitssl_hip.h serve patch sides that are multiples of 4, and the bf16
 * GEMMs take a contraction length that is a multiple of 64 and an output width that is a multiple of 4.  A patch width
 * Pd = C * P * P that is neither (patch 14: 588, 1-channel patch 7: 49) is run at a PADDED width ld >= Pd inside the engine:
 * the entry points below write and read matrices with a row stride, keep the pad columns at zero, and bring gradients
 * computed at the padded width back to the contiguous [.., Pd] shapes of the parameters.  Zero pad columns contribute exact
 * zeros to the fp32 accumulators of the GEMMs, so padding changes no result.
 */
#ifndef VITSSL_PATCH_H
#define VITSSL_PATCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* img f32 [B, C, H, W] -> patches bf16 [B * (H/P) * (W/P), ld], any P >= 1 that divides H and W.  Feature order (c, kh, kw),
 * patches row-major over the grid, round to nearest even (the layout and rounding of vitssl_patchify_bf16).  Columns
 * Pd .. ld-1 of every row are written as +0 on EVERY call.  ld >= Pd and ld % 2 == 0 (rows are written as 4-byte pairs);
 * `patches` 4-byte aligned; no alignment is assumed of the image rows.  Image rows are read coalesced and reordered through
 * LDS; the channel rows of one patch, padded, must fit 64 KiB of LDS: C * P * (P + 31) <= 16000. */
int vitssl_patchify_ld_bf16(const float* img, void* patches, int B, int C, int H, int W, int P, int ld, void* stream);

/* out f32 [n_idx, C * P * P] (contiguous) = patches[idx] gathered straight from the image, exact fp32 copies, any P >= 1
 * (the layout of vitssl_gather_patches_f32).  idx int32 [n_idx], values in [0, B * (H/P) * (W/P)) of the caller's image
 * batch.  Same LDS limit as above. */
int vitssl_gather_patches_any_f32(const float* img, const int32_t* idx, float* out, int n_idx, int C, int H, int W, int P,
                                  void* stream);

/* nn.L1Loss(mean) on matrices with row strides: pred f32 (row stride ld_p), target f32 (row stride ld_t), rows x cols with
 * any cols >= 1.  loss_sum += sum |pred - target| over the first `cols` columns (caller zeroes it and divides by
 * rows * cols); each workgroup parks its partial in a slot of the workspace and the slots are added in order, as
 * vitssl_l1_loss does: the same inputs give the same bits.  dpred_bf16 (row stride ld_d, or NULL): sign(pred - target) *
 * gscale in the first `cols` columns, +0 in columns cols .. ld_d-1, every element written.  ld_p, ld_t >= cols; with dpred:
 * ld_d >= cols, ld_d % 2 == 0, dpred 4-byte aligned.  workspace: at least vitssl_sum_workspace_floats(rows * cols, 1). */
int vitssl_l1_loss_ld(const float* pred, int64_t ld_p, const float* target, int64_t ld_t, float* loss_sum, void* dpred_bf16,
                      int64_t ld_d, float gscale, int64_t rows, int cols, float* workspace, int64_t workspace_floats,
                      void* stream);

/* dst f32 [rows, cols] (contiguous) += src f32 [rows, ld] restricted to its first `cols` columns: brings a weight gradient
 * computed at the padded width back into the flat gradient buffer.  One fp32 add per element.  ld >= cols. */
int vitssl_accumulate_ld_f32(float* dst, const float* src, int64_t rows, int cols, int64_t ld, void* stream);

/* vitssl_cast_transpose_batch with destination row strides: dst bf16 [R, ld_dst] and dst_t bf16 [C, ld_dst_t] receive the
 * image and the transposed image of src f32 [R, C] in their first C / R columns.  Nothing else of the destinations is
 * touched: the caller zeroes them once, and the pad columns (and pad rows of a taller destination) stay zero through every
 * refresh.  `jobs` and `tile_start` live in DEVICE memory, tile_start as for vitssl_cast_transpose_batch. */
typedef struct {
  const float* src; /* f32 [R, C] */
  void* dst;        /* bf16 [R, ld_dst] or NULL */
  void* dst_t;      /* bf16 [C, ld_dst_t] or NULL */
  int R, C;
  int ld_dst, ld_dst_t; /* >= C, >= R */
} vitssl_cast_ld_job_t;
int vitssl_cast_transpose_batch_ld(const vitssl_cast_ld_job_t* jobs, const int* tile_start, int njobs, int total_tiles,
                                   void* stream);

#ifdef __cplusplus
}
#endif
#endif
