/*
 * vitssl_classify.h -- C ABI of the classification loss of libvitssl_hip.so (MI355X, gfx950): the loss, the gradient head
 * of the backward, the predictions and the epoch counters of a supervised / fine-tune step in one entry point.
 *
 * Same library, same conventions as vitssl_hip.h (0 on success, <0 on error with vitssl_last_error(); no allocation;
 * device pointers and workspaces owned by the caller; enqueued on `stream`, never synchronised).  Kept in a header of its
 * own so that the symbol list of vitssl_hip.h, vitssl_version() and vitssl_cross_entropy stay what they are; the Python
 * mirror binds it through vitssl_hip._lib.REGISTRY["classify"].
 */
#ifndef VITSSL_CLASSIFY_H
#define VITSSL_CLASSIFY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- nn.CrossEntropyLoss(weight=None, reduction="mean", ignore_index=i, label_smoothing=eps) -------------------------
 * What utils/trainers/supervised_trainer.py:34-38 of the reference evaluates per step (criterion of
 * configs/supervised/training.yaml), together with what follows it there: preds.argmax(1) (:46), the correct / total counts
 * of :53 and, in this engine, the top of the backward (the zero-padded bf16 d(logits) and the classifier's bias gradient).
 *
 *   logits     f32 [B, ld]      the padded output of the classifier GEMM: columns 0 .. C-1 of every row are read, the rest
 *                               is never touched.  ld >= C, ld % 4 == 0, 16-byte aligned (rows are read as 16-byte pieces)
 *   labels     i64 [B]
 *   loss_out   f32 [2]          OVERWRITTEN: [0] = sum over valid rows of the row loss, [1] = n_valid.  The caller forms the
 *                               quotient on the device: 0 / 0 = nan when every row is ignored, as torch gives
 *   dlogits    bf16 [B, ld_out] or NULL (evaluation).  ld_out % 64 == 0, ld_out >= C, 16-byte aligned: the operand layout the
 *                               head's gemm_nt / gemm_tn read.  Every element is written: columns < C of a valid row hold
 *                               (softmax - (1 - eps) onehot - eps / C) * upstream / n_valid, columns C .. ld_out-1 and
 *                               every ignored row hold zeros
 *   dbias      f32 [C] or NULL  ACCUMULATED: column sums of that gradient before its rounding to bf16
 *   pred       i64 [B]          argmax over the C valid columns of every row, ignored rows included.  A tie goes to the
 *                               lowest index.  NaN compares as the largest value, as in torch.argmax and numpy.argmax: a
 *                               row with a NaN answers the index of its first NaN
 *   counters   i64 [2]          ACCUMULATED: [0] += valid rows with pred == label, [1] += n_valid (one host read an epoch)
 *   bad_labels i32 [1]          ACCUMULATED: += rows whose label is neither ignore_index nor in [0, C).  Such a row is
 *                               treated as ignored (nothing is read or written through the label); the kernel never traps
 *   workspace  >= vitssl_classify_loss_workspace_floats(B, C) floats, 16-byte aligned; may hold anything
 *
 * A row with label == ignore_index contributes nothing.  With n_valid the number of other rows, lse = logsumexp(z) and
 * zbar the mean of the row's C logits:  row loss = (1 - eps)(lse - z[y]) + eps (lse - zbar).  n_valid is counted inside
 * the launch (every wave scans the B labels), not read by the host.
 *
 * Arithmetic is fp64 throughout (inputs are fp32, so z - max is exact): the bf16 gradient is the correctly rounded image of
 * the fp64 value up to the error of exp(), also where softmax - 1 cancels (1 - p[y] is summed from the other columns, not
 * subtracted).  Sums over rows follow the deterministic-sum rule of vitssl_hip.h: every row stores its loss (fp64) and its
 * fp32 gradient in a slot of the workspace and one launch each adds the slots in a fixed order; no float atomics, the same
 * inputs give the same bits on every run.
 *
 * One wave per row.  A row of up to 1024 classes stays in the wave's registers between the passes; a longer one is
 * re-read (three passes).  Limits (VITSSL_ERR_ARG beyond them, named in the message): 1 <= B <= 2^22, 2 <= C <= 65536,
 * 0 <= eps <= 1 (a double, as torch keeps it: eps / C is subtracted from probabilities of its own size).  Every check, a
 * NULL or too small workspace included, is made before anything is launched. */
int64_t vitssl_classify_loss_workspace_floats(int B, int C);
int vitssl_classify_loss(const float* logits, const int64_t* labels, int B, int C, int ld, double label_smoothing,
                         int64_t ignore_index, float upstream, float* loss_out, void* dlogits_bf16, int ld_out, float* dbias,
                         int64_t* pred, int64_t* counters, int32_t* bad_labels, float* workspace, int64_t workspace_floats,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif
