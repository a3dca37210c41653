/*
 * vitssl_optim.h -- C ABI of the segmented AdamW step of libvitssl_hip.so (MI355X, gfx950): per-parameter learning-rate
 * multipliers and weight decay, and clipping of the global gradient norm without a host read.
 *
 * Same library, same conventions as vitssl_hip.h (0 on success, <0 on error with vitssl_last_error() naming the offending
 * argument; no allocation; device pointers and workspaces owned by the caller; enqueued on `stream`, never synchronised).
 * Kept in a header of its own so that the symbol list of vitssl_hip.h and vitssl_version() stay what they are; the Python
 * mirror binds these through vitssl_hip._lib.REGISTRY["optim"].  vitssl_adamw of vitssl_hip.h is untouched.
 *
 * The segment table.  A flat fp32 store (parameters p, gradient g, moments m and v, each `numel` floats) is described by
 * `nseg` segments in ascending order, one per parameter that takes part in the step:
 *   offset        first float of the segment, a multiple of 4 (16-byte loads and stores); offset + n <= numel
 *   n             its length, any positive number (1, 3, 65, ...); segments do not overlap
 *   lr_scale      the segment steps with lr * lr_scale
 *   weight_decay  its decoupled weight decay
 * Floats between segments (alignment pads, frozen parameters, parameters without a gradient) belong to no segment: no
 * kernel here reads or writes them, in any of the buffers -- they may hold anything, NaN included.
 * The kernels walk the table in units of 1024 floats that never straddle a segment.  vitssl_optim_table_build checks the
 * segments ON THE HOST and writes the image the kernels read (the entries followed by every segment's first unit), which
 * the caller copies to the device once and keeps until the set of segments changes.
 * THE CALLER'S CONTRACT: `table` of the launching entry points is the DEVICE copy of an image that vitssl_optim_table_build
 * accepted, and `nseg` is the nseg that image was built with.  The launching entry points cannot look into device memory:
 * they check nseg's range only and trust both.  Another nseg, or an image the builder did not write, makes the kernels read
 * unit starts from the wrong place and address the buffers out of bounds.
 *
 * vitssl_grad_sumsq: out[0] = sum of g[i]^2 over the table's segments.  Deterministic (ABI paragraph "deterministic sums" of
 * vitssl_hip.h): every workgroup stores one double-precision partial in the workspace, a second launch adds the partials
 * in a fixed order; no float atomics; the same inputs give the same bits.  `out` is overwritten, not accumulated into.
 * The workspace holds vitssl_grad_sumsq_workspace_bytes(nseg) bytes, 8-byte aligned, and is written before it is read.
 *
 * vitssl_adamw_segments: one launch over all segments.  Per element exactly the update of vitssl_adamw,
 *   gr = g * (gscale * coef);  p *= 1 - lr_s * weight_decay;  m = b1 m + (1 - b1) gr;  v = b2 v + (1 - b2) gr^2;
 *   p -= (lr_s / (1 - b1^step)) * m / (sqrt(v) / sqrt(1 - b2^step) + eps),      lr_s = lr * lr_scale
 * with coef = 1 when `sumsq` is NULL, else coef = min(1, max_norm / (gscale * sqrt(sumsq[0]) + 1e-6)), read on the device:
 * torch.nn.utils.clip_grad_norm_ applied to the averaged gradient g * gscale, with no host read of the norm.  One segment
 * {0, n, 1, wd} with sumsq == NULL gives the bits of vitssl_adamw(p, g, m, v, n, ..., wd, ...).
 * g is never written: after a clipped step the gradient buffer still holds the UNCLIPPED gradient.
 * p, g, m, v must be 16-byte aligned.  VITSSL_ERR_ARG before anything is launched for a NULL pointer, nseg <= 0, step < 1,
 * max_norm <= 0 with sumsq given, or a workspace below the sizing function's answer.
 */
#ifndef VITSSL_OPTIM_H
#define VITSSL_OPTIM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  int64_t offset;
  int64_t n;
  float lr_scale;
  float weight_decay;
} vitssl_optim_segment_t;

/* bytes of the table image of nseg segments (0 for nseg <= 0) */
int64_t vitssl_optim_table_bytes(int nseg);
/* host only: checks `segments` against a store of `numel` floats and writes the image into `image` (host memory of at least
 * vitssl_optim_table_bytes(nseg) bytes).  Launches nothing. */
int vitssl_optim_table_build(const vitssl_optim_segment_t* segments, int nseg, int64_t numel, void* image, int64_t image_bytes);

int64_t vitssl_grad_sumsq_workspace_bytes(int nseg);
int vitssl_grad_sumsq(const float* g, const void* table, int nseg, float* out, void* workspace, int64_t workspace_bytes,
                      void* stream);
int vitssl_adamw_segments(float* p, const float* g, float* m, float* v, const void* table, int nseg, float lr, float beta1,
                          float beta2, float eps, int step, float gscale, const float* sumsq, float max_norm, void* stream);

#ifdef __cplusplus
}
#endif
#endif
