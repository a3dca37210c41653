// MAE (masked autoencoder) token plumbing and loss (gfx950; C ABI in include_ext/vitssl_mae.h): assembly of the visible
// tokens, the un-shuffle in front of the decoder, both backwards, the normalised-pixel MSE loss and three row gathers /
// scatters.  All of it is HBM-bound: f32 moves as 16 bytes per lane, bf16 results as 8 (16 in the bf16 gather), coalesced along
// the row.  Column sums are two-stage and ordered (common.h, "deterministic sums"): no float atomics.
#include "common.h"
#include "../../include_ext/vitssl_mae.h"

namespace {

constexpr int MAE_THREADS = 256;
constexpr int MAE_SUM_ROWS = 32;        // rows of one slot row of a column sum (more once MAE_MAX_SPLITS blocks are in use)
constexpr int MAE_MAX_SPLITS = 512;
constexpr int MAE_LOSS_BLOCKS = 2048;   // the loss: one slot per block, four rows (waves) per block and trip

inline unsigned mae_grid(long long work_items) {
  long long g = (work_items + MAE_THREADS - 1) / MAE_THREADS;
  return (unsigned)(g < 1 ? 1 : g);
}
inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

__device__ __forceinline__ u32x2 pack4(const f32x4& v) { return u32x2{pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])}; }

// ------------------------------------------------------------------ forwards: one thread = 4 columns of one output row
__global__ void mae_tokens_fwd_kernel(const float* __restrict__ xk, const int* __restrict__ keep, const float* __restrict__ pos,
                                      const float* __restrict__ cls, float* __restrict__ out, long long rows, int K, int D) {
  const int d4n = D >> 2;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= rows * d4n) return;
  const long long r = t / d4n;
  const int c = (int)(t - r * d4n) * 4;
  const long long b = r / (K + 1);
  const int j = (int)(r - b * (K + 1));
  f32x4 v;
  if (j == 0) {
    v = *(const f32x4*)(cls + c) + *(const f32x4*)(pos + c);
  } else {
    const long long m = b * K + (j - 1);
    v = *(const f32x4*)(xk + m * D + c) + *(const f32x4*)(pos + (1LL + keep[m]) * D + c);
  }
  *(f32x4*)(out + r * D + c) = v;
}

__global__ void mae_unshuffle_fwd_kernel(const float* __restrict__ y, const int* __restrict__ restore, const float* __restrict__ mask_token,
                                         const float* __restrict__ dpos, float* __restrict__ out, long long rows, int N, int K, int D) {
  const int d4n = D >> 2;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= rows * d4n) return;
  const long long r = t / d4n;
  const int c = (int)(t - r * d4n) * 4;
  const long long b = r / (N + 1);
  const int n1 = (int)(r - b * (N + 1));
  const float* src = y + b * (K + 1) * D;                  // the CLS row of image b
  if (n1 > 0) {
    const int rs = restore[b * N + (n1 - 1)];
    src = rs < K ? src + (1LL + rs) * D : mask_token;
  }
  *(f32x4*)(out + r * D + c) = *(const f32x4*)(src + c) + *(const f32x4*)(dpos + (long long)n1 * D + c);
}

// ------------------------------------------------------------------ backwards: grid = (column chunks of 256 * 4, row splits)
// A block walks its contiguous run of rows of g top to bottom, four row loads in flight, and leaves its two column sums in
// slot rows parts[split][0 / 1][D]; the entry point adds the slot rows in order.
// UNSHUFFLE = false (token assembly): T = K + 1 rows per image; row 0 feeds sum 1 (d cls), the others sum 0 (d bias) and dst.
// UNSHUFFLE = true: T = N + 1 rows per image; a kept row (row 0, or restore < K) feeds sum 0 (d bias) and row
// (b, 1 + restore) of dst; the others feed sum 1 (d mask_token).
template <bool UNSHUFFLE>
__global__ void mae_bwd_kernel(const float* __restrict__ g, const int* __restrict__ restore, bf16_t* __restrict__ dst,
                               float* __restrict__ parts, long long rows, int T, int K, int D) {
  const int c = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (c >= D) return;
  const long long per = (rows + gridDim.y - 1) / gridDim.y;
  const long long r0 = blockIdx.y * per;
  const long long r1 = r0 + per < rows ? r0 + per : rows;
  f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0;
  long long b = r0 / T;
  int j = (int)(r0 - b * T);
  for (long long r = r0; r < r1; r += 4) {
    f32x4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (r + u < r1) v[u] = *(const f32x4*)(g + (r + u) * D + c);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (r + u >= r1) break;
      long long out_row;                    // < 0: the row feeds sum 1 only
      if constexpr (UNSHUFFLE) {
        const int rs = j == 0 ? -1 : restore[b * (T - 1) + (j - 1)];
        out_row = rs < K ? b * (K + 1) + (1 + rs) : -1;
      } else {
        out_row = j == 0 ? -1 : b * K + (j - 1);
      }
      if (out_row >= 0) {
        s0 += v[u];
        *(u32x2*)(dst + out_row * D + c) = pack4(v[u]);
      } else {
        s1 += v[u];
      }
      if (++j == T) j = 0, ++b;
    }
  }
  float* slot = parts + (long long)blockIdx.y * 2 * D + c;
  *(f32x4*)slot = s0;
  *(f32x4*)(slot + D) = s1;
}

// ------------------------------------------------------------------ rows by index: one thread = one 16-byte piece
template <typename V, bool SCATTER>
__global__ void mae_rows_kernel(const V* __restrict__ src, const int* __restrict__ idx, V* __restrict__ out, long long rows, int pieces) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= rows * pieces) return;
  const long long r = t / pieces;
  const int p = (int)(t - r * pieces);
  const int i = idx[r];
  V v = {};
  if (!SCATTER || i >= 0) v = src[(long long)i * pieces + p];
  out[r * pieces + p] = v;
}

// ------------------------------------------------------------------ loss
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// columns c .. c + 3 of a row of n columns (zeros behind the row's end); vec: as one 16-byte piece
__device__ __forceinline__ f32x4 row_ld4(const float* p, int c, int n, bool vec) {
  if (vec) return *(const f32x4*)(p + c);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (c + e < n) v[e] = p[c + e];
  return v;
}

// One wave per row, blocks stride over the rows; NV > 0: the wave keeps the target row (up to NV * 256 columns) in registers
// and reads it once; NV = 0: any length, the statistics sweep the row again (it comes back from the vector cache).
// parts[block] = sum of the block's row losses, added in row order per wave and then over the four waves.
template <int NV>
__global__ __launch_bounds__(MAE_THREADS) void mae_loss_kernel(const float* __restrict__ pred, long long ld, float* __restrict__ target,
                                                               float* __restrict__ parts, bf16_t* __restrict__ dpred, long long Mm,
                                                               int Pd, int Pdp, int norm_pix, double gs, int vec) {
  __shared__ double red[MAE_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nch = (Pd + 3) >> 2;                                  // 4-column chunks of a row, the last one may be partial
  const int iters = NV > 0 ? NV : (nch + 63) >> 6;
  double acc = 0.0;
  for (long long row = (long long)blockIdx.x * (MAE_THREADS / 64) + wave; row < Mm; row += (long long)gridDim.x * (MAE_THREADS / 64)) {
    const float* pr = pred + row * ld;
    float* tr = target + row * Pd;
    f32x4 tv[NV > 0 ? NV : 1];
    auto get = [&](int i, int c4) -> f32x4 { return NV > 0 ? tv[NV > 0 ? i : 0] : row_ld4(tr, 4 * c4, Pd, vec); };
    if (NV > 0) {
#pragma unroll(NV > 0 ? NV : 1)
      for (int i = 0; i < iters; ++i) {
        const int c4 = lane + 64 * i;
        tv[NV > 0 ? i : 0] = c4 < nch ? row_ld4(tr, 4 * c4, Pd, vec) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
    double mu = 0.0, rs = 1.0;
    if (norm_pix) {
      double s = 0.0;
#pragma unroll(NV > 0 ? NV : 1)
      for (int i = 0; i < iters; ++i) {
        const int c4 = lane + 64 * i;
        if (c4 < nch) {
          const f32x4 t = get(i, c4);                            // (zeros behind the row's end add nothing)
          s += ((double)t[0] + (double)t[1]) + ((double)t[2] + (double)t[3]);
        }
      }
      mu = wave_sum_d(s) / (double)Pd;
      double q = 0.0;
#pragma unroll(NV > 0 ? NV : 1)
      for (int i = 0; i < iters; ++i) {
        const int c4 = lane + 64 * i;
        if (c4 < nch) {
          const f32x4 t = get(i, c4);
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (4 * c4 + e < Pd) {
              const double d = (double)t[e] - mu;
              q = fma(d, d, q);
            }
        }
      }
      rs = 1.0 / sqrt(wave_sum_d(q) / (double)(Pd - 1) + 1e-6);
    }
    double l = 0.0;
#pragma unroll(NV > 0 ? NV : 1)
    for (int i = 0; i < iters; ++i) {
      const int c4 = lane + 64 * i;
      if (c4 < nch) {
        const int c = 4 * c4;
        f32x4 t = get(i, c4);
        const f32x4 p = row_ld4(pr, c, Pd, vec);
        double td[4];                                            // the target in fp64: what the loss and the gradient see
#pragma unroll
        for (int e = 0; e < 4; ++e) td[e] = ((double)t[e] - mu) * rs;      // (mu = 0, rs = 1 without norm_pix: the value itself)
        if (norm_pix) {
#pragma unroll
          for (int e = 0; e < 4; ++e) t[e] = (float)td[e];
          if (vec) {
            *(f32x4*)(tr + c) = t;
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (c + e < Pd) tr[c + e] = t[e];
          }
        }
        f32x4 gq = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (c + e < Pd) {
            const double d = (double)p[e] - td[e];
            l = fma(d, d, l);
            gq[e] = (float)(d * gs);
          }
        if (dpred) *(u32x2*)(dpred + row * Pdp + c) = pack4(gq);
      }
    }
    if (dpred)                                                    // the pad columns behind the last chunk of the row
      for (int c4 = nch + lane; c4 < (Pdp >> 2); c4 += 64) *(u32x2*)(dpred + row * Pdp + 4 * c4) = u32x2{0u, 0u};
    acc += wave_sum_d(l) / (double)Pd;
  }
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) parts[blockIdx.x] = (float)(((red[0] + red[1]) + red[2]) + red[3]);
}

int check_shape(const char* who, int B, int N, int K, int D) {
  VS_CHECK_ARG(B > 0 && N > 0 && D > 0, "%s: B=%d, N=%d and the width %d must be positive", who, B, N, D);
  VS_CHECK_ARG(K >= 1 && K <= N - 1, "%s: K=%d kept patches outside [1, N-1] with N=%d", who, K, N);
  VS_CHECK_ARG(D % 4 == 0, "%s: the width %d must be a multiple of 4", who, D);
  VS_CHECK_ARG((long long)B * (N + 1) * (D / 4) < (1LL << 40), "%s: B * (N + 1) * width too large", who);
  return VITSSL_OK;
}

int column_sum_splits(long long rows) {
  long long s = (rows + MAE_SUM_ROWS - 1) / MAE_SUM_ROWS;
  return (int)(s > MAE_MAX_SPLITS ? MAE_MAX_SPLITS : s);
}

template <bool UNSHUFFLE>
int launch_bwd(const char* who, const float* g, const int32_t* restore, void* dst, float* sum0, float* sum1, long long rows, int T, int K,
               int D, float* workspace, int64_t workspace_floats, hipStream_t s) {
  const int splits = column_sum_splits(rows);
  float* parts = vs_sum_parts(workspace, workspace_floats, 2LL * splits * D, rows, D, who);
  if (!parts) return VITSSL_ERR_ARG;
  VS_CHECK_ARG(aligned(parts, 16), "%s: workspace must be 16-byte aligned", who);
  hipLaunchKernelGGL((mae_bwd_kernel<UNSHUFFLE>), dim3((D / 4 + MAE_THREADS - 1) / MAE_THREADS, splits), dim3(MAE_THREADS), 0, s, g,
                     (const int*)restore, (bf16_t*)dst, parts, rows, T, K, D);
  VS_CHECK_LAUNCH(who);
  return vs_reduce_parts(VsSums{{sum0, sum1, nullptr, nullptr}, {parts, parts + D, nullptr, nullptr}}, splits, D, 2LL * D, s);
}

template <typename V, bool SCATTER>
int launch_rows(const char* who, const void* src, const int32_t* idx, void* out, int64_t rows, int cols, int per_piece, void* stream) {
  VS_CHECK_ARG(src && idx && out, "%s: null pointer", who);
  VS_CHECK_ARG(rows > 0 && cols > 0, "%s: rows=%lld and cols=%d must be positive", who, (long long)rows, cols);
  VS_CHECK_ARG(cols % per_piece == 0, "%s: cols=%d must be a multiple of %d", who, cols, per_piece);
  VS_CHECK_ARG(rows < (1LL << 31) && rows * (cols / per_piece) < (1LL << 40), "%s: rows=%lld too large", who, (long long)rows);
  VS_CHECK_ARG(aligned(src, 16) && aligned(out, 16), "%s: src / out must be 16-byte aligned", who);
  hipLaunchKernelGGL((mae_rows_kernel<V, SCATTER>), dim3(mae_grid(rows * (cols / per_piece))), dim3(MAE_THREADS), 0, (hipStream_t)stream,
                     (const V*)src, (const int*)idx, (V*)out, (long long)rows, cols / per_piece);
  VS_CHECK_LAUNCH(who);
  return VITSSL_OK;
}

}  // namespace

extern "C" int vitssl_mae_tokens_fwd(const float* xk, const int32_t* keep, const float* pos, const float* cls, float* out, int B, int N,
                                     int K, int D, void* stream) {
  VS_CHECK_ARG(xk && keep && pos && cls && out, "mae_tokens_fwd: null pointer");
  if (int rc = check_shape("mae_tokens_fwd", B, N, K, D)) return rc;
  VS_CHECK_ARG(aligned(xk, 16) && aligned(pos, 16) && aligned(cls, 16) && aligned(out, 16), "mae_tokens_fwd: xk / pos / cls / out must be 16-byte aligned");
  const long long rows = (long long)B * (K + 1);
  hipLaunchKernelGGL(mae_tokens_fwd_kernel, dim3(mae_grid(rows * (D / 4))), dim3(MAE_THREADS), 0, (hipStream_t)stream, xk,
                     (const int*)keep, pos, cls, out, rows, K, D);
  VS_CHECK_LAUNCH("mae_tokens_fwd");
  return VITSSL_OK;
}

extern "C" int vitssl_mae_tokens_bwd(const float* g, void* dproj_bf16, float* dbias, float* dcls, int B, int N, int K, int D,
                                     float* workspace, int64_t workspace_floats, void* stream) {
  VS_CHECK_ARG(g && dproj_bf16 && dbias && dcls, "mae_tokens_bwd: null pointer");
  if (int rc = check_shape("mae_tokens_bwd", B, N, K, D)) return rc;
  VS_CHECK_ARG(aligned(g, 16) && aligned(dproj_bf16, 8), "mae_tokens_bwd: g must be 16-byte and dproj 8-byte aligned");
  return launch_bwd<false>("mae_tokens_bwd", g, nullptr, dproj_bf16, dbias, dcls, (long long)B * (K + 1), K + 1, K, D, workspace,
                           workspace_floats, (hipStream_t)stream);
}

extern "C" int vitssl_mae_unshuffle_fwd(const float* y, const int32_t* restore, const float* mask_token, const float* dpos, float* out,
                                        int B, int N, int K, int Dd, void* stream) {
  VS_CHECK_ARG(y && restore && mask_token && dpos && out, "mae_unshuffle_fwd: null pointer");
  if (int rc = check_shape("mae_unshuffle_fwd", B, N, K, Dd)) return rc;
  VS_CHECK_ARG(aligned(y, 16) && aligned(mask_token, 16) && aligned(dpos, 16) && aligned(out, 16),
               "mae_unshuffle_fwd: y / mask_token / dpos / out must be 16-byte aligned");
  const long long rows = (long long)B * (N + 1);
  hipLaunchKernelGGL(mae_unshuffle_fwd_kernel, dim3(mae_grid(rows * (Dd / 4))), dim3(MAE_THREADS), 0, (hipStream_t)stream, y,
                     (const int*)restore, mask_token, dpos, out, rows, N, K, Dd);
  VS_CHECK_LAUNCH("mae_unshuffle_fwd");
  return VITSSL_OK;
}

extern "C" int vitssl_mae_unshuffle_bwd(const float* g, const int32_t* restore, void* dy_bf16, float* dbias, float* dmask_token, int B,
                                        int N, int K, int Dd, float* workspace, int64_t workspace_floats, void* stream) {
  VS_CHECK_ARG(g && restore && dy_bf16 && dbias && dmask_token, "mae_unshuffle_bwd: null pointer");
  if (int rc = check_shape("mae_unshuffle_bwd", B, N, K, Dd)) return rc;
  VS_CHECK_ARG(aligned(g, 16) && aligned(dy_bf16, 8), "mae_unshuffle_bwd: g must be 16-byte and dy 8-byte aligned");
  return launch_bwd<true>("mae_unshuffle_bwd", g, restore, dy_bf16, dbias, dmask_token, (long long)B * (N + 1), N + 1, K, Dd, workspace,
                          workspace_floats, (hipStream_t)stream);
}

extern "C" int vitssl_mae_loss(const float* pred, int64_t ld, float* target, float* loss_out, void* dpred_bf16, int64_t Mm, int Pd,
                               int Pdp, int norm_pix, float gscale, float* workspace, int64_t workspace_floats, void* stream) {
  VS_CHECK_ARG(pred && target && loss_out, "mae_loss: null pointer");
  VS_CHECK_ARG(Mm > 0 && Mm < (1LL << 31) && Pd > 0, "mae_loss: Mm=%lld (below 2^31) and Pd=%d must be positive", (long long)Mm, Pd);
  VS_CHECK_ARG(ld >= Pd && ld < (1LL << 31), "mae_loss: ld=%lld smaller than Pd=%d (or above 2^31)", (long long)ld, Pd);
  VS_CHECK_ARG(!norm_pix || Pd > 1, "mae_loss: norm_pix needs Pd > 1 (the unbiased variance of one value divides by zero)");
  if (dpred_bf16) {
    VS_CHECK_ARG(Pdp >= Pd && Pdp % 4 == 0, "mae_loss: Pdp=%d must be a multiple of 4 that is at least Pd=%d", Pdp, Pd);
    VS_CHECK_ARG(aligned(dpred_bf16, 8), "mae_loss: dpred must be 8-byte aligned");
  }
  const int vec = Pd % 4 == 0 && ld % 4 == 0;
  VS_CHECK_ARG(!vec || (aligned(pred, 16) && aligned(target, 16)), "mae_loss: pred / target must be 16-byte aligned when Pd and ld are multiples of 4");
  long long grid = (Mm + MAE_THREADS / 64 - 1) / (MAE_THREADS / 64);
  if (grid > MAE_LOSS_BLOCKS) grid = MAE_LOSS_BLOCKS;
  float* parts = vs_sum_parts(workspace, workspace_floats, grid, Mm, Pd, "mae_loss");
  if (!parts) return VITSSL_ERR_ARG;
  const double gs = 2.0 * (double)gscale / (double)Pd;
  const dim3 g((unsigned)grid), b(MAE_THREADS);
  hipStream_t s = (hipStream_t)stream;
  bf16_t* dp = (bf16_t*)dpred_bf16;
  if (Pd <= 1024) hipLaunchKernelGGL(mae_loss_kernel<4>, g, b, 0, s, pred, (long long)ld, target, parts, dp, (long long)Mm, Pd, Pdp, norm_pix, gs, vec);
  else if (Pd <= 4096) hipLaunchKernelGGL(mae_loss_kernel<16>, g, b, 0, s, pred, (long long)ld, target, parts, dp, (long long)Mm, Pd, Pdp, norm_pix, gs, vec);
  else hipLaunchKernelGGL(mae_loss_kernel<0>, g, b, 0, s, pred, (long long)ld, target, parts, dp, (long long)Mm, Pd, Pdp, norm_pix, gs, vec);
  VS_CHECK_LAUNCH("mae_loss");
  return vs_reduce_parts(loss_out, parts, (int)grid, 1, 1, s);
}

extern "C" int vitssl_mae_gather_rows_bf16(const void* src_bf16, const int32_t* idx, void* out_bf16, int64_t n_idx, int cols, void* stream) {
  return launch_rows<u32x4, false>("mae_gather_rows_bf16", src_bf16, idx, out_bf16, n_idx, cols, 8, stream);
}

extern "C" int vitssl_mae_gather_rows_f32(const float* src, const int32_t* idx, float* out, int64_t n_idx, int cols, void* stream) {
  return launch_rows<f32x4, false>("mae_gather_rows_f32", src, idx, out, n_idx, cols, 4, stream);
}

extern "C" int vitssl_mae_scatter_rows_f32(const float* src, const int32_t* inv, float* g, int64_t rows, int cols, void* stream) {
  return launch_rows<f32x4, true>("mae_scatter_rows_f32", src, inv, g, rows, cols, 4, stream);
}
