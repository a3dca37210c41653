// The patch path for any patch side and channel count (include/vitssl_patch.h): patchify / target gather through LDS, the L1
// loss, the gradient accumulate and the weight cast on matrices with a row stride.  A patch width C*P*P that the GEMMs do not
// take is run at a padded width whose pad columns these kernels keep at zero.
#include "common.h"
#include "../../include/vitssl_patch.h"

namespace {

constexpr int PT_THREADS = 256;
constexpr int PT_TILE_FLOATS = 8192;      // preferred LDS tile (32 KiB: four workgroups per CU)
constexpr int PT_MAX_FLOATS = 16000;      // hard limit: 64 KiB of LDS less the patch-base table
constexpr int PT_MAX_NPX = 48;

// One workgroup = `npx` consecutive output rows (patches).  Load phase: the tile is filled in (c, kh, patch, kw) order, so that
// with neighbouring patches of one grid row consecutive lanes read consecutive floats of an image row (dword loads: a patch
// row starts at any 4-byte offset when P is 14 or 7).  Store phase: every output row is written left to right, bf16 as
// 4-byte pairs, the pad columns as zeros.
// LDS layout: tile[(c * P + kh) * rs + j * P + kw], j = patch within the workgroup.  Feature f = (c * P + kh) * P + kw of a
// patch sits at (f / P) * rs + j * P + f % P.  rs = npx * P + pad with rs % 32 == P % 32: stepping to the next kh moves the
// bank by P, exactly as if the features were contiguous, so the lanes of a store-phase read fall on consecutive banks (an
// unpadded stride such as 224 = 7 * 32 would put every kh segment of a patch on the same 14 banks).
template <bool GATHER, typename OutT>
__global__ void __launch_bounds__(PT_THREADS)
patch_rows_kernel(const float* __restrict__ img, const int* __restrict__ idx, OutT* __restrict__ out, long long nrows, int C,
                  int H, int W, int P, int ld, int npx, int rs) {
  extern __shared__ __align__(16) float pt_lds[];
  long long* base = (long long*)pt_lds;                 // [npx] image offset of each patch's (c = 0, kh = 0, kw = 0)
  float* tile = pt_lds + 2 * npx;
  const int gw = W / P, gh = H / P;
  const long long r0 = (long long)blockIdx.x * npx;
  const int nj = (int)(nrows - r0 < npx ? nrows - r0 : npx);
  for (int j = threadIdx.x; j < nj; j += PT_THREADS) {
    const long long m = GATHER ? (long long)idx[r0 + j] : r0 + j;
    const long long b = m / (gh * gw);
    const int pi = (int)(m - b * gh * gw);
    const int py = pi / gw, px = pi - py * gw;
    base[j] = (b * C * H + (long long)py * P) * W + (long long)px * P;
  }
  __syncthreads();
  const int seg = nj * P;                               // floats of one (c, kh) row of the tile
  const int rows = C * P;
  for (int i = threadIdx.x; i < rows * seg; i += PT_THREADS) {
    const int ckh = i / seg, rem = i - ckh * seg;
    const int j = rem / P, kw = rem - j * P;
    const int c = ckh / P, kh = ckh - c * P;
    tile[ckh * rs + rem] = img[base[j] + ((long long)c * H + kh) * W + kw];
  }
  __syncthreads();
  const int Pd = rows * P;
  if constexpr (sizeof(OutT) == 2) {
    const int hp = ld >> 1;
    for (int i = threadIdx.x; i < nj * hp; i += PT_THREADS) {
      const int j = i / hp, f = (i - j * hp) * 2;
      float v0 = 0.f, v1 = 0.f;
      if (f < Pd) {
        const int q = f / P;
        v0 = tile[q * rs + j * P + (f - q * P)];
      }
      if (f + 1 < Pd) {
        const int q = (f + 1) / P;
        v1 = tile[q * rs + j * P + (f + 1 - q * P)];
      }
      *(unsigned*)((bf16_t*)out + (r0 + j) * ld + f) = pack_bf2(v0, v1);
    }
  } else {
    for (int i = threadIdx.x; i < nj * Pd; i += PT_THREADS) {
      const int j = i / Pd, f = i - j * Pd;
      const int q = f / P;
      ((float*)out)[(r0 + j) * Pd + f] = tile[q * rs + j * P + (f - q * P)];
    }
  }
}

// patches per workgroup and the LDS row stride for (C, P); false where one patch does not fit
bool patch_tile(int C, int P, long long nrows, int* npx_out, int* rs_out) {
  const long long rows = (long long)C * P;
  if (rows * (P + 31) > PT_MAX_FLOATS) return false;
  long long npx = (PT_TILE_FLOATS / rows - 31) / P;
  if (npx < 1) npx = 1;
  if (npx > PT_MAX_NPX) npx = PT_MAX_NPX;
  if (npx > nrows) npx = nrows;
  const int seg = (int)npx * P;
  *npx_out = (int)npx;
  *rs_out = seg + (((P - seg) % 32) + 32) % 32;
  return true;
}

int check_geometry(const char* who, int B, int C, int H, int W, int P) {
  VS_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0, "%s: empty image batch B=%d C=%d H=%d W=%d", who, B, C, H, W);
  VS_CHECK_ARG(P > 0, "%s: patch size %d must be positive", who, P);
  VS_CHECK_ARG(H % P == 0 && W % P == 0, "%s: image %dx%d not divisible by patch %d", who, H, W, P);
  VS_CHECK_ARG((long long)C * P * (P + 31) <= PT_MAX_FLOATS, "%s: C * P * (P + 31) = %lld exceeds %d (the channel rows of one patch must fit the LDS tile)", who,
               (long long)C * P * (P + 31), PT_MAX_FLOATS);
  VS_CHECK_ARG((long long)C * P * P < (1 << 24), "%s: patch width C * P * P exceeds 2^24", who);
  return VITSSL_OK;
}

template <bool GATHER, typename OutT>
int launch_patch_rows(const char* who, const float* img, const int* idx, OutT* out, long long nrows, int C, int H, int W, int P, int ld,
                      hipStream_t s) {
  int npx, rs;
  if (!patch_tile(C, P, nrows, &npx, &rs)) {
    vitssl_set_error("%s: patch does not fit the LDS tile", who);
    return VITSSL_ERR_ARG;
  }
  const long long blocks = (nrows + npx - 1) / npx;
  VS_CHECK_ARG(blocks < (1LL << 31), "%s: %lld patches exceed the grid limit", who, nrows);
  const size_t lds = (size_t)npx * 8 + (size_t)C * P * rs * 4;
  hipLaunchKernelGGL((patch_rows_kernel<GATHER, OutT>), dim3((unsigned)blocks), dim3(PT_THREADS), lds, s, img, idx, out, nrows, C, H, W, P,
                     ld, npx, rs);
  VS_CHECK_LAUNCH(who);
  return VITSSL_OK;
}

// ------------------------------------------------------------------ L1 loss on rows with strides
// one thread = one pair of columns of dpred's width (of `cols` without dpred)
__global__ void l1_loss_ld_kernel(const float* __restrict__ pred, long long ld_p, const float* __restrict__ target, long long ld_t,
                                  float* __restrict__ loss_parts, bf16_t* __restrict__ dpred, long long ld_d, float gscale,
                                  long long rows, int cols, int hp) {
  __shared__ float part[PT_THREADS / 64];
  float acc = 0.f;
  const long long n = rows * hp;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / hp;
    const int c = (int)(i - r * hp) * 2;
    float s[2] = {0.f, 0.f};
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (c + u < cols) {
        const float d = pred[r * ld_p + c + u] - target[r * ld_t + c + u];
        acc += fabsf(d);
        s[u] = d > 0.f ? gscale : (d < 0.f ? -gscale : 0.f);
      }
    }
    if (dpred) *(unsigned*)(dpred + r * ld_d + c) = pack_bf2(s[0], s[1]);
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int w = 0; w < PT_THREADS / 64; ++w) t += part[w];
    loss_parts[blockIdx.x] = t;                   // this block's slot; vitssl_l1_loss_ld sums the slots in order
  }
}

__global__ void accumulate_ld_kernel(float* __restrict__ dst, const float* __restrict__ src, long long rows, int cols, long long ld) {
  const long long n = rows * cols;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / cols;
    const int c = (int)(i - r * cols);
    dst[i] += src[r * ld + c];
  }
}

// cast_transpose_batch_kernel of elementwise.hip with destination row strides
__global__ void cast_transpose_batch_ld_kernel(const vitssl_cast_ld_job_t* __restrict__ jobs, const int* __restrict__ tile_start,
                                               int njobs) {
  __shared__ bf16_t tile[64][66];
  const int b = blockIdx.x;
  int lo = 0, hi = njobs;              // tile_start[lo] <= b < tile_start[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tile_start[mid] <= b) lo = mid; else hi = mid;
  }
  const vitssl_cast_ld_job_t j = jobs[lo];
  const int t = b - tile_start[lo];
  const int tx_n = (j.C + 63) >> 6;
  const int r0 = (t / tx_n) * 64, c0 = (t % tx_n) * 64;
  const int R = j.R, C = j.C;
  bf16_t* dst = (bf16_t*)j.dst;
  bf16_t* dst_t = (bf16_t*)j.dst_t;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int rr = ty; rr < 64; rr += 4) {
    const int r = r0 + rr, c = c0 + tx;
    bf16_t h = 0;
    if (r < R && c < C) {
      h = f2bf(j.src[(long long)r * C + c]);
      if (dst) dst[(long long)r * j.ld_dst + c] = h;
    }
    tile[rr][tx] = h;
  }
  __syncthreads();
  if (dst_t) {
    for (int cc = ty; cc < 64; cc += 4) {
      const int c = c0 + cc, r = r0 + tx;
      if (c < C && r < R) dst_t[(long long)c * j.ld_dst_t + r] = tile[tx][cc];
    }
  }
}

unsigned pt_stream_grid(long long items) {
  long long g = (items + PT_THREADS - 1) / PT_THREADS;
  if (g > 2048) g = 2048;
  if (g < 1) g = 1;
  return (unsigned)g;
}

}  // namespace

extern "C" int vitssl_patchify_ld_bf16(const float* img, void* patches, int B, int C, int H, int W, int P, int ld, void* stream) {
  VS_CHECK_ARG(img && patches, "patchify_ld: null pointer");
  if (int rc = check_geometry("patchify_ld", B, C, H, W, P)) return rc;
  const int Pd = C * P * P;
  VS_CHECK_ARG(ld >= Pd, "patchify_ld: ld=%d is smaller than the patch width C * P * P = %d", ld, Pd);
  VS_CHECK_ARG(ld % 2 == 0, "patchify_ld: ld=%d must be a multiple of 2 (rows are written as 4-byte pairs)", ld);
  VS_CHECK_ARG(ld <= (1 << 24), "patchify_ld: ld=%d exceeds 2^24", ld);
  VS_CHECK_ARG(((uintptr_t)patches & 3) == 0, "patchify_ld: patches must be 4-byte aligned");
  const long long nrows = (long long)B * (H / P) * (W / P);
  return launch_patch_rows<false, bf16_t>("patchify_ld", img, nullptr, (bf16_t*)patches, nrows, C, H, W, P, ld, (hipStream_t)stream);
}

extern "C" int vitssl_gather_patches_any_f32(const float* img, const int32_t* idx, float* out, int n_idx, int C, int H, int W, int P,
                                             void* stream) {
  VS_CHECK_ARG(img && idx && out, "gather_patches_any: null pointer");
  VS_CHECK_ARG(n_idx > 0, "gather_patches_any: n_idx=%d must be positive", n_idx);
  if (int rc = check_geometry("gather_patches_any", 1, C, H, W, P)) return rc;
  return launch_patch_rows<true, float>("gather_patches_any", img, idx, out, (long long)n_idx, C, H, W, P, C * P * P, (hipStream_t)stream);
}

extern "C" int vitssl_l1_loss_ld(const float* pred, int64_t ld_p, const float* target, int64_t ld_t, float* loss_sum, void* dpred_bf16,
                                 int64_t ld_d, float gscale, int64_t rows, int cols, float* workspace, int64_t workspace_floats,
                                 void* stream) {
  VS_CHECK_ARG(pred && target && loss_sum, "l1_loss_ld: null pointer");
  VS_CHECK_ARG(rows > 0 && cols > 0, "l1_loss_ld: empty problem rows=%lld cols=%d", (long long)rows, cols);
  VS_CHECK_ARG(ld_p >= cols && ld_t >= cols, "l1_loss_ld: ld_p=%lld / ld_t=%lld smaller than cols=%d", (long long)ld_p, (long long)ld_t, cols);
  if (dpred_bf16) {
    VS_CHECK_ARG(ld_d >= cols, "l1_loss_ld: ld_d=%lld smaller than cols=%d", (long long)ld_d, cols);
    VS_CHECK_ARG(ld_d % 2 == 0, "l1_loss_ld: ld_d=%lld must be a multiple of 2 (dpred is written as 4-byte pairs)", (long long)ld_d);
    VS_CHECK_ARG(((uintptr_t)dpred_bf16 & 3) == 0, "l1_loss_ld: dpred must be 4-byte aligned");
    VS_CHECK_ARG(ld_d < (1LL << 31), "l1_loss_ld: ld_d=%lld exceeds 2^31", (long long)ld_d);
  }
  const int hp = dpred_bf16 ? (int)(ld_d / 2) : (cols + 1) / 2;
  const unsigned grid = pt_stream_grid(rows * hp);
  float* parts = vs_sum_parts(workspace, workspace_floats, grid, rows * cols, 1, "l1_loss_ld");
  if (!parts) return VITSSL_ERR_ARG;
  hipLaunchKernelGGL(l1_loss_ld_kernel, dim3(grid), dim3(PT_THREADS), 0, (hipStream_t)stream, pred, (long long)ld_p, target, (long long)ld_t,
                     parts, (bf16_t*)dpred_bf16, (long long)ld_d, gscale, (long long)rows, cols, hp);
  VS_CHECK_LAUNCH("l1_loss_ld");
  return vs_reduce_parts(loss_sum, parts, (int)grid, 1, 1, (hipStream_t)stream);
}

extern "C" int vitssl_accumulate_ld_f32(float* dst, const float* src, int64_t rows, int cols, int64_t ld, void* stream) {
  VS_CHECK_ARG(dst && src, "accumulate_ld: null pointer");
  VS_CHECK_ARG(rows > 0 && cols > 0, "accumulate_ld: empty problem rows=%lld cols=%d", (long long)rows, cols);
  VS_CHECK_ARG(ld >= cols, "accumulate_ld: ld=%lld smaller than cols=%d", (long long)ld, cols);
  hipLaunchKernelGGL(accumulate_ld_kernel, dim3(pt_stream_grid(rows * cols)), dim3(PT_THREADS), 0, (hipStream_t)stream, dst, src,
                     (long long)rows, cols, (long long)ld);
  VS_CHECK_LAUNCH("accumulate_ld");
  return VITSSL_OK;
}

extern "C" int vitssl_cast_transpose_batch_ld(const vitssl_cast_ld_job_t* jobs, const int* tile_start, int njobs, int total_tiles,
                                              void* stream) {
  VS_CHECK_ARG(jobs && tile_start, "cast_transpose_batch_ld: null pointer");
  VS_CHECK_ARG(njobs > 0 && total_tiles > 0, "cast_transpose_batch_ld: njobs=%d and total_tiles=%d must be positive", njobs, total_tiles);
  hipLaunchKernelGGL(cast_transpose_batch_ld_kernel, dim3(total_tiles), dim3(PT_THREADS), 0, (hipStream_t)stream, jobs, tile_start,
                     njobs);
  VS_CHECK_LAUNCH("cast_transpose_batch_ld");
  return VITSSL_OK;
}
