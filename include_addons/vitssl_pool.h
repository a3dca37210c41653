/*
 * vitssl_pool.h -- C ABI of the global-average-pooling head in libvitssl_hip.so (MI355X, gfx950): the mean of an image's patch
 * tokens on the fp32 residual stream, and its backward.
 *
 * An ADD-ON table: same library, same conventions as vitssl_hip.h (0 on success, -1 on an argument error with
 * vitssl_last_error() set; no allocation; device pointers owned by the caller; enqueued on `stream`, never synchronised; every
 * check is made before anything is launched, so a refused call writes nothing).  It lives under include_addons/ so that the
 * twelve headers of include/, the extension table of include_ext/, their symbol lists and vitssl_version() stay what they are;
 * the Python mirror binds every header of this directory through vitssl_hip._lib.ADDON_REGISTRY.
 *
 * Shapes: B images of T tokens each (T >= 2), D columns.  Row b*T of the stream is image b's CLS row, rows b*T+1 .. b*T+T-1
 * are its patch tokens.  r is the fp32 constant 1.0f / (float)(T - 1), computed once on the host.
 * Every operand moves as 16-byte pieces: D must be a multiple of 4 (D >= 4) and every pointer 16-byte aligned; a null or
 * misaligned pointer, B < 1, T < 2 or such a D is refused.  Index arithmetic is 64-bit.  No workspace, no float atomics.
 */
#ifndef VITSSL_POOL_H
#define VITSSL_POOL_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- forward -------------------------------------------------------------------------------------------------------------------
 * x f32 [B*T, D], read only; the CLS rows are never read
 * out f32 [B, D], every element OVERWRITTEN:  out[b, c] = r * sum_{t = 1 .. T-1} x[b*T + t, c]
 * The sum is taken in fp32 in an order that depends on (T, D) only -- not on B, the grid, the device's CU count or an
 * environment variable: token t belongs to part (t - 1) % 16, a part adds its tokens in ascending order starting from its
 * first, and the parts are added in ascending order starting from part 0.  The same inputs give the same bits, and image b of
 * a batch the bits of a launch on that image alone. */
int vitssl_pool_tokens_fwd(const float* x, float* out, int B, int T, int D, void* stream);

/* ---- backward ------------------------------------------------------------------------------------------------------------------
 * dout f32 [B, D], read only
 * g f32 [B*T, D], every element OVERWRITTEN:  g[b*T, c] = +0,  g[b*T + t, c] = r * dout[b, c] for t = 1 .. T-1 */
int vitssl_pool_tokens_bwd(const float* dout, float* g, int B, int T, int D, void* stream);

#ifdef __cplusplus
}
#endif
#endif
