/*
 * vitssl_lamb.h -- C ABI of the segmented LAMB step of libvitssl_hip.so (MI355X, gfx950): Adam moments, decoupled weight decay
 * inside the update, and one trust ratio |p| / |update| per parameter, over the segment table of vitssl_optim.h.
 *
 * Same library, same conventions as vitssl_hip.h (0 on success, <0 on error with vitssl_last_error() naming the offending
 * argument; no allocation; device pointers and workspaces owned by the caller; enqueued on `stream`, never synchronised).
 * Kept in a header of its own so that the symbol lists of the other headers stay what they are; the Python mirror binds these
 * through vitssl_hip._lib.REGISTRY["lamb"].  Nothing of vitssl_optim.h changes: the table is the image vitssl_optim_table_build
 * writes (same vitssl_optim_segment_t, same units of 1024 floats that never straddle a segment), and THE CALLER'S CONTRACT of
 * that header holds here too: `table` is the device copy of an image the builder accepted, `nseg` the nseg it was built with.
 *
 * The step (timm's Lamb restated).  For each element of segment s, with lr_s = lr * lr_scale and wd = weight_decay of s:
 *   gr = g * (gscale * coef)            coef exactly as vitssl_adamw_segments: 1 when sumsq == NULL, else
 *                                       min(1, max_norm / (gscale * sqrt(sumsq[0]) + 1e-6)), read on the device
 *   m  = b1 m + (1 - b1) gr;   v = b2 v + (1 - b2) gr^2
 *   r  = (m / (1 - b1^step)) / (sqrt(v) / sqrt(1 - b2^step) + eps) + wd * p
 *   trust_s = 1                                                 if wd == 0 and not always_adapt
 *           = (|p_s| > 0 and |r_s| > 0) ? |p_s| / |r_s| : 1     otherwise, then min(., 1) with trust_clip
 *   p -= lr_s * trust_s * r
 * |.| is the 2-norm over the whole segment, of the OLD p and of r formed from the NEW m and v.
 *
 * vitssl_lamb_segments is three launches on `stream`:
 *   (a) moments: writes m and v and stores, per UNIT of the table, the fp64 sums of p^2 and r^2 in the workspace
 *       (slot 2u and 2u + 1 of unit u; squares of fp32 values are exact in fp64).  Slots are per unit, not per workgroup:
 *       a segment's sums do not depend on the grid;
 *   (b) reduce: one wave per segment adds the segment's slots in a fixed order in fp64 (lane l adds the slots of units
 *       l, l + 64, ... in ascending order, then the 64 lanes are added in a fixed tree), forms the ratio in double and
 *       rounds it to fp32 once into trust[s];
 *   (c) apply: recomputes r from the new m, v and the old p with the expression of (a), and writes p.
 * No float atomics; the same inputs give the same bits.  g is never written (after a clipped step it still holds the
 * UNCLIPPED gradient).  Floats between the segments are neither read nor written, in any buffer.  Per element the step moves
 * 40 bytes (a: p, g, m, v read, m, v written; c: p, m, v read, p written) and needs no store-sized scratch.
 *
 * Workspace: vitssl_lamb_workspace_bytes(segments, nseg) bytes (16 per unit), 8-byte aligned, every slot written before it
 * is read.  The sizing function runs on the HOST over the segments the table was built from (the launching entry cannot look
 * into the device table); it returns 0 for nseg outside 1 .. 2^20, a NULL pointer or a segment with n <= 0.
 * The launching entry checks what it can see: workspace_bytes >= 16 * nseg (every segment owns at least one unit) and the
 * alignment.  Beyond that the kernels compare the table's unit count with the slots the workspace holds: with too few slots
 * they write nothing but trust[s] = NaN for every s -- a loud no-op, never a write behind the workspace.
 *
 * flags: VITSSL_LAMB_ALWAYS_ADAPT (bit 0) adapts segments with wd == 0 too; VITSSL_LAMB_TRUST_CLIP (bit 1) caps the ratio at 1.
 * trust: nseg floats, required; after the step trust[s] is the ratio segment s stepped with.
 * VITSSL_ERR_ARG before anything is launched for: a NULL pointer (p, g, m, v, table, trust, workspace), nseg outside
 * 1 .. 2^20, step < 1, max_norm <= 0 with sumsq given, a workspace below 16 * nseg bytes or not 8-byte aligned, p / g / m / v
 * not 16-byte aligned (table: 8, trust: 4), flag bits other than the two above.
 */
#ifndef VITSSL_LAMB_H
#define VITSSL_LAMB_H

#include <stdint.h>

#include "vitssl_optim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VITSSL_LAMB_ALWAYS_ADAPT 1
#define VITSSL_LAMB_TRUST_CLIP 2

int64_t vitssl_lamb_workspace_bytes(const vitssl_optim_segment_t* segments, int nseg);
int vitssl_lamb_segments(float* p, const float* g, float* m, float* v, const void* table, int nseg, float lr, float beta1,
                         float beta2, float eps, int step, float gscale, const float* sumsq, float max_norm, int flags,
                         float* trust, void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
