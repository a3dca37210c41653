/*
 * vitssl_bce.h -- C ABI of the binary cross-entropy of the supervised / fine-tune step in libvitssl_hip.so (MI355X, gfx950):
 * the DeiT III loss (timm's BinaryCrossEntropy: a sigmoid per class against label-smoothed or mixed soft targets, with an
 * optional target threshold), the gradient head of the backward, the predictions and the epoch counters in one entry point.
 *
 * Same library, same conventions as vitssl_hip.h (0 on success, <0 on error with vitssl_last_error(); no allocation;
 * device pointers and workspaces owned by the caller; enqueued on `stream`, never synchronised; every check is made before
 * anything is launched).  Kept in a header of its own so that the symbol lists of vitssl_hip.h, vitssl_classify.h and
 * vitssl_mixup.h, vitssl_version(), vitssl_classify_loss and vitssl_classify_loss_mix stay what they are; the Python mirror
 * binds it through vitssl_hip._lib.REGISTRY["bce"].
 */
#ifndef VITSSL_BCE_H
#define VITSSL_BCE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- BinaryCrossEntropy(smoothing, target_threshold, sum_classes) with ignore_index ----------------------------------------
 * Layouts, the OVERWRITTEN / ACCUMULATED rules, the alignment rules, the limits (1 <= B <= 2^22, 2 <= C <= 65536,
 * 0 <= smoothing <= 1), the row states (valid / ignored / bad, as vitssl_classify_loss without tables and as
 * vitssl_classify_loss_mix with them), pred (argmax, first-NaN rule), counters (the row's OWN label) and bad_labels are
 * exactly those of vitssl_classify.h and vitssl_mixup.h; the sizing function returns what
 * vitssl_classify_loss_workspace_floats returns.  What differs is the loss:
 *
 *   partner           i32 [B] or NULL   the row whose label is mixed in
 *   lam               f32 [B] or NULL   the weight of the row's own label.  Both NULL (one label per row) or both given
 *   target_threshold  < 0: none.  NaN is refused
 *   sum_classes       0: a row's loss is the MEAN over its C classes; else their SUM
 *
 * With a = labels[i], b = labels[partner[i]], l = (double)lam[i] (without tables b = a, l = 1) and
 * s(y) = (1 - eps) onehot(y) + eps / C (so timm's on = 1 - eps + eps / C, off = eps / C):
 *   target        t = l s(a) + (1 - l) s(b);  with a threshold t = (t > target_threshold) ? 1 : 0, compared in fp64
 *   element loss  e(z, t) = max(z, 0) - z t + log1p(exp(-|z|))
 *   row loss      sum_c e(z[c], t[c]) / (sum_classes ? 1 : C)
 *   loss_out      [0] = sum of the row losses over the valid rows, [1] = n_valid (the caller divides on the device)
 *   gradient      (sigmoid(z) - t) * upstream / (n_valid * (sum_classes ? 1 : C)), the zero-padded bf16 dlogits; dbias
 *                 accumulates the column sums of the fp32 values before that rounding.  Where t == 1 exactly,
 *                 sigmoid(z) - 1 is formed as -sigmoid(-z)
 * With no ignored row this is torch's binary_cross_entropy_with_logits(z, t) (mean), with sum_classes its
 * (reduction="none").sum(-1).mean().  A two-label row with a == b, l == 1 or l == 0 runs the one-label statements: the same
 * bits as the call without tables.
 *
 * Arithmetic is fp64 throughout (log1p(exp(-|z|)) is evaluated as 2 atanh(u), u = exp(-|z|) / (2 + exp(-|z|)) <= 1/3, by a series
 * whose omitted terms lie below half an ulp).  One wave per row, rows read as 16-byte pieces, padding columns never read.  Neither the
 * loss nor the gradient of an element needs a sum over the row, so a row of ANY length is one pass (there is no
 * register-resident / re-read split at 1024 classes as in vitssl_classify_loss).  Sums over rows follow the deterministic-sum
 * rule of vitssl_hip.h: slots in the workspace added in a fixed order, no float atomics, the same bits on every run.  n_valid
 * is counted inside the launch. */
int64_t vitssl_classify_bce_workspace_floats(int B, int C);
int vitssl_classify_bce(const float* logits, const int64_t* labels, const int32_t* partner, const float* lam, int B, int C, int ld,
                        double smoothing, double target_threshold, int sum_classes, int64_t ignore_index, float upstream,
                        float* loss_out, void* dlogits_bf16, int ld_out, float* dbias, int64_t* pred, int64_t* counters,
                        int32_t* bad_labels, float* workspace, int64_t workspace_floats, void* stream);

#ifdef __cplusplus
}
#endif
#endif
