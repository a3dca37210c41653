/*
 * vitssl_mixup.h -- C ABI of Mixup / CutMix in libvitssl_hip.so (MI355X, gfx950): the kernel that mixes a rendered batch with
 * its partner rows, and the classification loss of vitssl_classify.h against the two-label soft targets that go with it.
 *
 * Same library, same conventions as vitssl_hip.h (0 on success, <0 on error with vitssl_last_error(); no allocation;
 * device pointers and workspaces owned by the caller; enqueued on `stream`, never synchronised; every check is made before
 * anything is launched).  Kept in a header of its own so that the symbol lists of vitssl_hip.h and vitssl_classify.h,
 * vitssl_version() and vitssl_classify_loss stay what they are; the Python mirror binds it through
 * vitssl_hip._lib.REGISTRY["mixup"].
 */
#ifndef VITSSL_MIXUP_H
#define VITSSL_MIXUP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the mix kernel --------------------------------------------------------------------------------------------------
 * What timm's Mixup does to a batch between the transform list and the model, per row i with partner p = iparams[i][1]:
 *
 *   x        f32 [B, C, H, W]   the rendered batch (data.GPUTransform's output), 16-byte aligned, only read
 *   out      f32 [B, C, H, W]   a DIFFERENT buffer, 16-byte aligned; every element is written.  A byte range that overlaps
 *                               x's is refused on the host (rows read their partners: in place cannot work)
 *   iparams  i32 [B, 6]         kind, partner, y0, y1, x0, x1
 *   lam      f32 [B]
 *
 *   kind 0  copy    out[i] = x[i], exact bits; neither x[p] nor lam is read
 *   kind 1  blend   out[i] = fmaf(lam, x[i], (1 - lam) * x[p]) in fp32, 1 - lam formed in the kernel: three roundings,
 *                   whatever the compiler's contraction flags
 *   kind 2  paste   out[i] = x[p] where y0 <= y < y1 and x0 <= x < x1, x[i] elsewhere, exact bits; lam is not read, and
 *                   x[p] is read inside the box only
 *
 * The tables are device memory the kernel cannot trust and does not fault on: a partner outside [0, B) is the row itself,
 * a box is clamped to the image (an empty or inverted one pastes nothing), any other kind is a copy.
 *
 * Memory-bound: rows with W % 4 == 0 move as 16-byte pieces with a per-element select at the box's left and right edge,
 * any other W goes element by element; a capped grid strides over the batch.  Limits (VITSSL_ERR_ARG beyond them, named
 * in the message): B, C, H, W >= 1 and C * H * W < 2^31. */
int vitssl_mix_batch(const float* x, float* out, const int32_t* iparams, const float* lam, int B, int C, int H, int W,
                     void* stream);

/* ---- the loss against two-label targets -------------------------------------------------------------------------------
 * vitssl_classify_loss (vitssl_classify.h) with, per row i, the soft target of a mixed image.  Layouts, the OVERWRITTEN /
 * ACCUMULATED rules, the limits, the alignment rules, fp64 arithmetic, deterministic sums and one wave per row are exactly
 * those of vitssl_classify_loss; the sizing function returns what vitssl_classify_loss_workspace_floats returns.  New:
 *
 *   partner    i32 [B]          the row whose label is mixed in
 *   lam        f32 [B]          the weight of the row's own label
 *
 * With a = labels[i], b = labels[partner[i]], l = (double)lam[i], s(y) = (1 - eps) onehot(y) + eps / C, the target is
 * t = l s(a) + (1 - l) s(b):
 *   row loss = l (1 - eps)(lse - z[a]) + (1 - l)(1 - eps)(lse - z[b]) + eps (lse - zbar)
 *   gradient = (softmax - t) * upstream / n_valid
 * (what torch's cross_entropy gives for the probability target l onehot(a) + (1 - l) onehot(b) with label_smoothing = eps).
 * A row with a == b, l == 1 or l == 0 is a one-label row: the same code computes it as vitssl_classify_loss does, to the
 * same bits.  In a two-label row 1 - t[a] - p[a] and 1 - t[b] - p[b] are summed from the other columns, as there.
 *
 * Rows that contribute nothing (zero gradient, not counted in n_valid):
 *   - bad rows, which also add 1 to bad_labels: partner outside [0, B); lam outside [0, 1] or NaN; a label that is neither
 *     ignore_index nor in [0, C).  Nothing is ever read through a bad index;
 *   - otherwise, rows where either label equals ignore_index.
 * pred is the argmax of every row as before; counters[0] counts the valid rows with pred == labels[i], the row's OWN
 * label (what the trainer's confusion matrix is fed), counters[1] the valid rows. */
int64_t vitssl_classify_loss_mix_workspace_floats(int B, int C);
int vitssl_classify_loss_mix(const float* logits, const int64_t* labels, const int32_t* partner, const float* lam, int B, int C,
                             int ld, double label_smoothing, int64_t ignore_index, float upstream, float* loss_out,
                             void* dlogits_bf16, int ld_out, float* dbias, int64_t* pred, int64_t* counters,
                             int32_t* bad_labels, float* workspace, int64_t workspace_floats, void* stream);

#ifdef __cplusplus
}
#endif
#endif
