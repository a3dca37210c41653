/*
 * vitssl_metrics.h -- C ABI of the per-epoch training-metric kernels of libvitssl_hip.so (MI355X, gfx950).
 *
 * Same library, same conventions as vitssl_hip.h (0 on success, <0 on error with vitssl_last_error(); no allocation;
 * device pointers and workspaces owned by the caller; enqueued on `stream`, never synchronised).  Kept in a header of its
 * own so that the symbol list of vitssl_hip.h and vitssl_version() stay what they are; the Python mirror binds these
 * through vitssl_hip._lib.REGISTRY["metrics"].
 *
 * Both entry points are single-pass reductions without float atomics: every workgroup stores its fp64 partials in a slot
 * of the caller's workspace and ONE reduce launch adds the slots in a fixed order, so the same inputs give the same bits
 * on every run.  Every slot a reduce reads has been written by the launch before it: a workspace may hold anything.
 * Workspaces are sized in floats like every workspace of the library and must be 8-byte aligned (they hold doubles).
 */
#ifndef VITSSL_METRICS_H
#define VITSSL_METRICS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- SimMIM reconstruction metrics: PSNR and SSIM ---------------------------------------------
 * Replaces what utils/trainers/simmim_trainer.py:79-96 (and :116-133 in validate) does per epoch: keep every step's
 * clamp(pred, 0, 1) and target reshaped to [B * nm, C, P, P] alive, torch.cat them, and feed utils/metrics.py:159-187
 * (torcheval PeakSignalNoiseRatio(data_range=1.0), ignite SSIM(data_range=1.0)).  Here each step's tensors are reduced
 * where they lie into a 4-double accumulator that the host reads once per epoch:
 *   acc[0] += sum((clamp(pred, 0, 1) - target)^2)                                   PSNR = 10 log10(acc[2] / acc[0])
 *   acc[1] += sum over patches of mean over (C, P, P) of the SSIM index              SSIM = acc[1] / acc[3]
 *   acc[2] += n * C * P * P      (elements)
 *   acc[3] += n                  (patches)
 * SSIM index as ignite computes it: x = clamp(pred, 0, 1), y = target; each [P, P] plane reflect-padded by 5 and filtered
 * with the 11 x 11 Gaussian window of sigma 1.5 (outer product of exp(-d^2 / (2 sigma^2)) / sum, d = -5 .. 5); from the
 * five filtered maps of x, y, x^2, y^2, xy:  mu_x, mu_y, s_xx = E[x^2] - mu_x^2, s_yy, s_xy = E[xy] - mu_x mu_y,
 *   index = (2 mu_x mu_y + c1)(2 s_xy + c2) / ((mu_x^2 + mu_y^2 + c1)(s_xx + s_yy + c2)),  c1 = 0.01^2, c2 = 0.03^2.
 * The filter is separable and runs out of LDS in fp64 (the vector fp64 rate of gfx950 is half its fp32 rate, and the
 * kernel is bound by LDS reads either way), so the result carries no fp32 cancellation in E[x^2] - mu^2.
 *   pred, target  f32 [n, C * P * P]   feature order (c, kh, kw): a row is one [C, P, P] patch
 *   acc           f64 [4]              accumulated into (zero it at the start of an epoch)
 *   workspace     >= vitssl_recon_metrics_workspace_floats(n, C, P) floats
 * Limits (VITSSL_ERR_ARG beyond them, the message names the limit): 6 <= P <= 32 (a reflect padding of 5 needs P >= 6),
 * 1 <= C <= 4, n >= 0.  n == 0 launches nothing and leaves acc untouched.  A NULL or too small workspace is refused before
 * anything is launched. */
int64_t vitssl_recon_metrics_workspace_floats(int64_t n, int C, int P);
int vitssl_recon_metrics(const float* pred, const float* target, double* acc, int64_t n, int C, int P, float* workspace,
                         int64_t workspace_floats, void* stream);

/* ---- DINO output statistics --------------------------------------------------------------------
 * Replaces the eight metric classes of utils/metrics.py:58-156 that utils/trainers/dino_trainer.py:114-118 and :149-153
 * feed with the last batch's teacher and student outputs and the centre: CenterNorm (torch.linalg.norm), Teacher / Student
 * Mean, STD, Var over the flattened tensors, and CosineSim, whose body (:144-156) materialises a [G, V, B, K] product.
 * One pass over the two tensors (every element is read once per pair of teacher rows: once for G <= 2):
 *   out[0] = G * B * K     out[1] = mean of all teacher elements     out[2] = their centred second moment sum((t - mean)^2)
 *   out[3] = V * B * K     out[4], out[5] = the same for the student
 *   out[6] = sum over (g, v, b) of <t[g,b,:], s[v,b,:]> / (|t[g,b,:]| |s[v,b,:]| + 1e-8)   (a view paired with itself included)
 *   out[7] = |center|^2    (0 when center is NULL)
 * The host forms Var = out[2] / (out[0] - 1) (torch's unbiased default), STD = sqrt(Var), CosineSim = out[6] / (G V B),
 * CenterNorm = sqrt(out[7]).  Moments are accumulated in fp64 around the tensor's first element, so a large common offset
 * of the logits costs no precision.  `out` is overwritten, not accumulated into.
 *   teacher  f32 [G, B, K]     student  f32 [V, B, K]     center  f32 [K] or NULL     out  f64 [8]
 *   workspace >= vitssl_dino_stats_workspace_floats(G, V, B, K) floats
 * Limits (VITSSL_ERR_ARG beyond them, named in the message): K % 4 == 0, 1 <= G <= V <= 16, B >= 1; teacher, student and
 * center 16-byte aligned.  A NULL or too small workspace is refused before anything is launched. */
int64_t vitssl_dino_stats_workspace_floats(int G, int V, int B, int K);
int vitssl_dino_stats(const float* teacher, const float* student, const float* center, double* out, int G, int V, int B, int K,
                      float* workspace, int64_t workspace_floats, void* stream);

#ifdef __cplusplus
}
#endif
#endif
