/*
 * vitssl_attention_hd.h -- C ABI of the attention kernels for head dims other than 64 of libvitssl_hip.so (MI355X, gfx950).
 *
 * Same library, same conventions as vitssl_hip.h (0 on success, <0 on error with vitssl_last_error() naming the offending
 * argument; no allocation; device pointers and workspaces owned by the caller; enqueued on `stream`, never synchronised).
 * Kept in a header of its own so that the symbol list of vitssl_hip.h and vitssl_version() stay what they are; the Python
 * mirror binds these through vitssl_hip._lib.REGISTRY["attention_hd"].
 *
 * The attention entry points of vitssl_hip.h serve dh = 64 and refuse every other head dim; these two serve
 *   8 <= dh <= 128, dh % 8 == 0   (a head's slice of a row is a whole number of 16-byte chunks; dh = 64 included)
 *   1 <= N <= 2048 tokens
 * with one streaming design for every N (a workgroup owns 128 rows of one (image, head), the other operand streams through
 * LDS in 64-row tiles).  The kernels are instantiated for the head dim rounded up to 32, 64, 96 or 128 and read qkv in
 * place: nothing is padded or pre-scaled on the host.  Layouts are those of vitssl_attn_fwd / vitssl_attn_bwd:
 *   qkv    bf16 [B * N, 3 * H * dh]   q | k | v, each [H, dh] per token row
 *   out    bf16 [B * N, H * dh]       dout likewise
 *   lse    f32  [B, H, N]             log-sum-exp of the scaled scores
 *   probs  f32  [B, H, N, N] or NULL  softmax probabilities, written by a kernel of its own: `out` does not depend on it
 *   dqkv   bf16 [B * N, 3 * H * dh]   every element written exactly once (it may hold anything before)
 *   delta_ws f32 [B, H, N]            workspace of the backward: rowsum(dout * out), written before it is read
 * scores = q k^T / sqrt(dh), the scale applied in fp32; P is rounded to bf16 into P.V, dS to bf16 into the dQ / dK products.
 * The backward uses no atomics: the same inputs give the same bits.
 * qkv, out, dout and dqkv must be 16-byte aligned.  VITSSL_ERR_ARG beyond any limit, before anything is launched.
 */
#ifndef VITSSL_ATTENTION_HD_H
#define VITSSL_ATTENTION_HD_H

#ifdef __cplusplus
extern "C" {
#endif

int vitssl_attn_hd_fwd(const void* qkv, void* out, float* lse, float* probs, int B, int N, int H, int dh, void* stream);
int vitssl_attn_hd_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, float* delta_ws, int B,
                       int N, int H, int dh, void* stream);

#ifdef __cplusplus
}
#endif
#endif
