// Global average pooling of the patch tokens on the fp32 residual stream, forward and backward (gfx950; C ABI in
// include_addons/vitssl_pool.h).  Both kernels are HBM-bound: 16 bytes per lane along D, one work item per (image, chunk of
// POOL_COLS columns), a capped grid that strides the items.  A workgroup's POOL_PARTS lane groups stride the tokens; the
// forward adds their partial sums through LDS in part order, so the summation order depends on T alone: no float atomics.
#include "common.h"
#include "../../include_addons/vitssl_pool.h"

namespace {

constexpr int POOL_THREADS = 256;
constexpr int POOL_LANES = 16;                              // lanes along D of one lane group: 16 * 16 bytes = 256 contiguous bytes of a row
constexpr int POOL_COLS = POOL_LANES * 4;                   // columns of one work item
constexpr int POOL_PARTS = POOL_THREADS / POOL_LANES;       // lane groups = partial sums per work item
constexpr int POOL_MAX_BLOCKS = 2048;                       // 256 CUs * 8 workgroups; the rest is strided

inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
inline unsigned pool_grid(long long items) { return (unsigned)(items < POOL_MAX_BLOCKS ? items : POOL_MAX_BLOCKS); }

// out[b, c] = r * sum_{t >= 1} x[b*T + t, c].  Part p = lane group p sums tokens 1 + p, 1 + p + POOL_PARTS, ... in ascending
// order (four loads in flight, added in token order); lane group 0 then adds parts 0 .. POOL_PARTS-1 in that order.
__global__ __launch_bounds__(POOL_THREADS) void pool_tokens_fwd_kernel(const float* __restrict__ x, float* __restrict__ out, long long items,
                                                                       int chunks, int T, int D, float r) {
  __shared__ f32x4 parts[POOL_PARTS][POOL_LANES];
  const int lane = threadIdx.x % POOL_LANES, part = threadIdx.x / POOL_LANES;
  for (long long item = blockIdx.x; item < items; item += gridDim.x) {      // uniform over the workgroup: the barriers below are safe
    const long long b = item / chunks;
    const int c = ((int)(item - b * chunks) * POOL_LANES + lane) * 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (c < D) {
      const float* src = x + b * T * D + c;                                   // the CLS row of image b: never dereferenced, t >= 1 below
      int t = 1 + part;
      for (; t + 3 * POOL_PARTS < T; t += 4 * POOL_PARTS) {
        const f32x4 v0 = *(const f32x4*)(src + (long long)t * D);
        const f32x4 v1 = *(const f32x4*)(src + (long long)(t + POOL_PARTS) * D);
        const f32x4 v2 = *(const f32x4*)(src + (long long)(t + 2 * POOL_PARTS) * D);
        const f32x4 v3 = *(const f32x4*)(src + (long long)(t + 3 * POOL_PARTS) * D);
        acc = acc + v0;
        acc = acc + v1;
        acc = acc + v2;
        acc = acc + v3;
      }
      for (; t < T; t += POOL_PARTS) acc = acc + *(const f32x4*)(src + (long long)t * D);
    }
    parts[part][lane] = acc;
    __syncthreads();
    if (part == 0 && c < D) {
      f32x4 s = parts[0][lane];
#pragma unroll
      for (int p = 1; p < POOL_PARTS; ++p) s = s + parts[p][lane];
      *(f32x4*)(out + b * D + c) = s * r;
    }
    __syncthreads();                                                          // parts is rewritten by the next item
  }
}

// g[b*T, c] = +0, g[b*T + t, c] = r * dout[b, c]: the same items; lane group p writes rows p, p + POOL_PARTS, ...
__global__ __launch_bounds__(POOL_THREADS) void pool_tokens_bwd_kernel(const float* __restrict__ dout, float* __restrict__ g, long long items,
                                                                       int chunks, int T, int D, float r) {
  const int lane = threadIdx.x % POOL_LANES, part = threadIdx.x / POOL_LANES;
  for (long long item = blockIdx.x; item < items; item += gridDim.x) {
    const long long b = item / chunks;
    const int c = ((int)(item - b * chunks) * POOL_LANES + lane) * 4;
    if (c >= D) continue;
    const f32x4 v = *(const f32x4*)(dout + b * D + c) * r;
    float* dst = g + b * T * D + c;
    int t = part;
    if (t == 0) {
      *(f32x4*)dst = f32x4{0.f, 0.f, 0.f, 0.f};
      t = POOL_PARTS;
    }
    for (; t < T; t += POOL_PARTS) *(f32x4*)(dst + (long long)t * D) = v;
  }
}

int pool_check(const char* who, const void* in, const void* out, int B, int T, int D) {
  VS_CHECK_ARG(in && out, "%s: null pointer", who);
  VS_CHECK_ARG(B >= 1 && T >= 2, "%s: B=%d must be at least 1 and T=%d at least 2 (one CLS row and one patch token)", who, B, T);
  VS_CHECK_ARG(D >= 4 && D % 4 == 0, "%s: D=%d must be a positive multiple of 4", who, D);
  VS_CHECK_ARG(aligned(in, 16) && aligned(out, 16), "%s: both pointers must be 16-byte aligned", who);
  return VITSSL_OK;
}

}  // namespace

extern "C" int vitssl_pool_tokens_fwd(const float* x, float* out, int B, int T, int D, void* stream) {
  if (int rc = pool_check("pool_tokens_fwd", x, out, B, T, D)) return rc;
  const int chunks = (D + POOL_COLS - 1) / POOL_COLS;
  const long long items = (long long)B * chunks;
  const float r = 1.0f / (float)(T - 1);
  hipLaunchKernelGGL(pool_tokens_fwd_kernel, dim3(pool_grid(items)), dim3(POOL_THREADS), 0, (hipStream_t)stream, x, out, items, chunks, T, D, r);
  VS_CHECK_LAUNCH("pool_tokens_fwd");
  return VITSSL_OK;
}

extern "C" int vitssl_pool_tokens_bwd(const float* dout, float* g, int B, int T, int D, void* stream) {
  if (int rc = pool_check("pool_tokens_bwd", dout, g, B, T, D)) return rc;
  const int chunks = (D + POOL_COLS - 1) / POOL_COLS;
  const long long items = (long long)B * chunks;
  const float r = 1.0f / (float)(T - 1);
  hipLaunchKernelGGL(pool_tokens_bwd_kernel, dim3(pool_grid(items)), dim3(POOL_THREADS), 0, (hipStream_t)stream, dout, g, items, chunks, T, D, r);
  VS_CHECK_LAUNCH("pool_tokens_bwd");
  return VITSSL_OK;
}
