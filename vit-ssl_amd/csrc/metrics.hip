// Per-epoch training metrics as single-pass reductions (gfx950): PSNR / SSIM of the SimMIM reconstruction and the DINO
// output statistics (utils/metrics.py of the reference, fed by utils/trainers/simmim_trainer.py:79-96 and
// dino_trainer.py:114-118).  include/vitssl_metrics.h declares the entry points and states what each replaces.
//
// Both follow the library's rule for sums fed by many workgroups (common.h, "deterministic sums"), with fp64 partials: a
// workgroup stores its partial sums in its own slot of the caller's workspace, one reduce launch adds the slots in a fixed
// order.  All accumulation is fp64: inputs are fp32, so products and differences are exact and the results carry rounding
// of the sums only; gfx950 issues vector fp64 at half the fp32 rate, which neither kernel is bound by.
#include "../../include/vitssl_metrics.h"
#include "common.h"
#include <math.h>
#include <utility>

namespace {

constexpr int MT_THREADS = 256;
constexpr int MT_WAVES = MT_THREADS / 64;

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ================================================================ reconstruction metrics
// A plane is one [P, P] channel of one patch; the planes of the whole input are contiguous runs of P * P floats.  A workgroup
// owns RM_PASSES * pl consecutive planes and takes them pl at a time through LDS:
//   load        clamp(pred), target -> X, Y (f32), 16-byte pieces where P * P % 4 == 0; the squared error is summed here
//   horizontal  11 taps along the row with reflected indices over x, y, x^2, y^2, xy -> H[5] (f64)
//   vertical    11 taps down the column of H -> the five means of a pixel in registers -> its SSIM index
// Lanes map to consecutive pixels, so every LDS access of a wave is to consecutive addresses.
constexpr int RM_PASSES = 4;
constexpr int RM_PIX = 512;            // pixels per pass aimed at: 24 KiB of LDS
constexpr int RM_MAX_PLANES = 8;
constexpr int RM_TAPS = 11, RM_PAD = 5;
constexpr int RM_PX_BYTES = 2 * (int)sizeof(float) + 5 * (int)sizeof(double);

struct RmTaps {
  double w[RM_TAPS];
};

struct RmPlan {
  int pl;             // planes per pass
  int plw;            // planes per workgroup
  long long groups;   // workgroups = partial slots (2 doubles each)
  int lds;            // bytes
};

RmPlan rm_plan(long long n, int C, int P) {
  RmPlan p;
  const int pp = P * P;
  p.pl = RM_PIX / pp;
  if (p.pl < 1) p.pl = 1;
  if (p.pl > RM_MAX_PLANES) p.pl = RM_MAX_PLANES;
  p.plw = p.pl * RM_PASSES;
  p.groups = (n * C + p.plw - 1) / p.plw;
  p.lds = p.pl * pp * RM_PX_BYTES;     // <= 48 KiB at P = 32
  return p;
}

__device__ __forceinline__ int reflect(int i, int P) { return i < 0 ? -i : (i >= P ? 2 * (P - 1) - i : i); }

// grid = plan.groups; parts[2 * blockIdx.x] = {squared error, sum of SSIM indices} of the workgroup's planes
template <bool VEC>
__global__ __launch_bounds__(MT_THREADS) void recon_metrics_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                                   double* __restrict__ parts, long long planes, int P, int pl,
                                                                   RmTaps taps) {
  extern __shared__ __attribute__((aligned(16))) double rm_lds[];
  const int pp = P * P, npx = pl * pp;
  double* H = rm_lds;
  float* X = (float*)(H + 5 * npx);
  float* Y = X + npx;
  const int tid = threadIdx.x;
  const long long q0 = (long long)blockIdx.x * (pl * RM_PASSES);
  constexpr double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
  double sse = 0.0, ssim = 0.0;

  for (int pass = 0; pass < RM_PASSES; ++pass) {
    const long long q = q0 + (long long)pass * pl;
    if (q >= planes) break;                                      // uniform over the workgroup
    const int nv = (int)(planes - q < pl ? planes - q : pl) * pp;   // valid pixels of this pass
    const float* ps = pred + q * pp;
    const float* ts = target + q * pp;
    if constexpr (VEC) {
      for (int i = tid * 4; i < nv; i += MT_THREADS * 4) {
        f32x4 a = *(const f32x4*)(ps + i);
        const f32x4 b = *(const f32x4*)(ts + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          a[e] = fminf(fmaxf(a[e], 0.f), 1.f);
          const double d = (double)a[e] - (double)b[e];
          sse = fma(d, d, sse);
        }
        *(f32x4*)(X + i) = a;
        *(f32x4*)(Y + i) = b;
      }
    } else {
      for (int i = tid; i < nv; i += MT_THREADS) {
        const float a = fminf(fmaxf(ps[i], 0.f), 1.f), b = ts[i];
        const double d = (double)a - (double)b;
        sse = fma(d, d, sse);
        X[i] = a;
        Y[i] = b;
      }
    }
    __syncthreads();
    for (int i = tid; i < nv; i += MT_THREADS) {
      const int pix = i % pp, c = pix % P;
      const float* xr = X + (i - c);
      const float* yr = Y + (i - c);
      double h0 = 0.0, h1 = 0.0, h2 = 0.0, h3 = 0.0, h4 = 0.0;
#pragma unroll
      for (int t = 0; t < RM_TAPS; ++t) {
        const int cc = reflect(c + t - RM_PAD, P);
        const double x = xr[cc], y = yr[cc], w = taps.w[t];
        h0 = fma(w, x, h0);
        h1 = fma(w, y, h1);
        h2 = fma(w, x * x, h2);
        h3 = fma(w, y * y, h3);
        h4 = fma(w, x * y, h4);
      }
      H[i] = h0;
      H[npx + i] = h1;
      H[2 * npx + i] = h2;
      H[3 * npx + i] = h3;
      H[4 * npx + i] = h4;
    }
    __syncthreads();
    for (int i = tid; i < nv; i += MT_THREADS) {
      const int pix = i % pp, r = pix / P, c = pix - r * P;
      const double* hc = H + (i - pix) + c;
      double mx = 0.0, my = 0.0, exx = 0.0, eyy = 0.0, exy = 0.0;
#pragma unroll
      for (int t = 0; t < RM_TAPS; ++t) {
        const double* h = hc + reflect(r + t - RM_PAD, P) * P;
        const double w = taps.w[t];
        mx = fma(w, h[0], mx);
        my = fma(w, h[npx], my);
        exx = fma(w, h[2 * npx], exx);
        eyy = fma(w, h[3 * npx], eyy);
        exy = fma(w, h[4 * npx], exy);
      }
      const double mxx = mx * mx, myy = my * my, mxy = mx * my;
      const double a1 = 2.0 * mxy + C1, a2 = 2.0 * (exy - mxy) + C2;
      const double b1 = mxx + myy + C1, b2 = (exx - mxx) + (eyy - myy) + C2;
      ssim += (a1 * a2) / (b1 * b2);
    }
    __syncthreads();                                             // X, Y and H are rewritten by the next pass
  }
  // (the last pass ended with a barrier: the front of the LDS image is free for the workgroup's two sums)
  sse = wave_sum_d(sse);
  ssim = wave_sum_d(ssim);
  if ((tid & 63) == 0) {
    H[2 * (tid >> 6)] = sse;
    H[2 * (tid >> 6) + 1] = ssim;
  }
  __syncthreads();
  if (tid < 2) parts[2 * (long long)blockIdx.x + tid] = ((H[tid] + H[2 + tid]) + H[4 + tid]) + H[6 + tid];
}

// one workgroup: acc += the slots, added in a fixed order
__global__ __launch_bounds__(MT_THREADS) void recon_metrics_reduce_kernel(const double* __restrict__ parts, long long groups,
                                                                          double* __restrict__ acc, double inv_cpp, double elements,
                                                                          double patches) {
  __shared__ double red[2 * MT_WAVES];
  const int tid = threadIdx.x;
  double a = 0.0, b = 0.0;
  for (long long g = tid; g < groups; g += MT_THREADS) {
    a += parts[2 * g];
    b += parts[2 * g + 1];
  }
  a = wave_sum_d(a);
  b = wave_sum_d(b);
  if ((tid & 63) == 0) {
    red[2 * (tid >> 6)] = a;
    red[2 * (tid >> 6) + 1] = b;
  }
  __syncthreads();
  if (tid == 0) {
    acc[0] += ((red[0] + red[2]) + red[4]) + red[6];
    acc[1] += (((red[1] + red[3]) + red[5]) + red[7]) * inv_cpp;
    acc[2] += elements;
    acc[3] += patches;
  }
}

// false: the geometry is refused (error set)
bool rm_geometry(long long n, int C, int P, const char* who) {
  if (P < 6 || P > 32) {
    vitssl_set_error("%s: patch size P = %d is outside 6 <= P <= 32 (the reflect padding of 5 needs P >= 6)", who, P);
    return false;
  }
  if (C < 1 || C > 4) {
    vitssl_set_error("%s: C = %d channels is outside 1 <= C <= 4", who, C);
    return false;
  }
  if (n < 0 || n > (1LL << 40)) {
    vitssl_set_error("%s: n = %lld patches is outside 0 <= n <= 2^40", who, n);
    return false;
  }
  return true;
}

// ================================================================ DINO output statistics
// grid = (B, K slices of DS_KL, pairs of teacher rows); one instantiation per student count V, so that the V row loads, the
// 2 V dot products and the V norms of a thread are registers without a condition between them.  For image b a thread reads 4 consecutive k of the pair's teacher rows and
// of all V student rows, and forms the 2 V dot products, the squared norms and the shifted moment sums from registers.
// Slot of a workgroup, DS_SLOT doubles:
//   [16 g + v] <t_g, s_v>   [32 + v] |s_v|^2   [48 + g] |t_g|^2   [50] sum(t - t0)   [51] sum((t - t0)^2)
//   [52] sum(s - s0)   [53] sum((s - s0)^2)   [54] |center slice|^2 (image 0 only)   [55] 0
// t0, s0: the first element of the tensor.  Student entries are the same for every teacher pair; the reduce reads pair 0's.
constexpr int DS_GT = 2;
constexpr int DS_VMAX = 16;
constexpr int DS_KL = 8192;
constexpr int DS_SLOT = 56;
constexpr int DS_NS = 32, DS_NT = 48, DS_TSUM = 50, DS_TSQ = 51, DS_SSUM = 52, DS_SSQ = 53, DS_CSQ = 54;

__device__ __forceinline__ void ds_put(double v, int idx, double* red, int tid) {
  v = wave_sum_d(v);
  if ((tid & 63) == 0) red[(tid >> 6) * DS_SLOT + idx] = v;
}

template <int V>
__global__ __launch_bounds__(MT_THREADS) void dino_stats_kernel(const float* __restrict__ teacher, const float* __restrict__ student,
                                                                const float* __restrict__ center, double* __restrict__ parts, int G,
                                                                int B, int K) {
  __shared__ double red[MT_WAVES * DS_SLOT];
  const int tid = threadIdx.x;
  const int b = blockIdx.x, ks = blockIdx.y, z = blockIdx.z;
  const int g0 = z * DS_GT;
  const bool two = g0 + 1 < G;
  const bool with_center = center != nullptr && b == 0 && z == 0;
  if (tid < MT_WAVES * DS_SLOT) red[tid] = 0.0;
  __syncthreads();
  const double t0 = teacher[0], s0 = student[0];
  const float* tp0 = teacher + ((long long)g0 * B + b) * K;
  const float* tp1 = tp0 + (long long)B * K;                     // dereferenced only if `two`
  const float* sp = student + (long long)b * K;
  const long long vstride = (long long)B * K;

  double dot[DS_GT][V], ns[V], nt[DS_GT] = {0.0, 0.0};
  double tsum = 0.0, tsq = 0.0, ssum = 0.0, ssq = 0.0, csq = 0.0;
#pragma unroll
  for (int v = 0; v < V; ++v) dot[0][v] = dot[1][v] = ns[v] = 0.0;

  const int k_end = min(K, (ks + 1) * DS_KL);
  for (int k = ks * DS_KL + tid * 4; k < k_end; k += MT_THREADS * 4) {
    f32x4 sv[V];
#pragma unroll
    for (int v = 0; v < V; ++v) sv[v] = *(const f32x4*)(sp + v * vstride + k);
    const f32x4 ta = *(const f32x4*)(tp0 + k);
    f32x4 tb = {0.f, 0.f, 0.f, 0.f};
    if (two) tb = *(const f32x4*)(tp1 + k);
    double a[4], bb[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      a[e] = ta[e];
      bb[e] = tb[e];
      nt[0] = fma(a[e], a[e], nt[0]);
      const double d = a[e] - t0;
      tsum += d;
      tsq = fma(d, d, tsq);
    }
    if (two) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        nt[1] = fma(bb[e], bb[e], nt[1]);
        const double d = bb[e] - t0;
        tsum += d;
        tsq = fma(d, d, tsq);
      }
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double x = sv[v][e];
        ns[v] = fma(x, x, ns[v]);
        dot[0][v] = fma(a[e], x, dot[0][v]);
        dot[1][v] = fma(bb[e], x, dot[1][v]);
        const double d = x - s0;
        ssum += d;
        ssq = fma(d, d, ssq);
      }
    }
    if (with_center) {
      const f32x4 c = *(const f32x4*)(center + k);
#pragma unroll
      for (int e = 0; e < 4; ++e) csq = fma((double)c[e], (double)c[e], csq);
    }
  }

#pragma unroll
  for (int v = 0; v < V; ++v) {
    ds_put(dot[0][v], v, red, tid);
    ds_put(dot[1][v], DS_VMAX + v, red, tid);
    ds_put(ns[v], DS_NS + v, red, tid);
  }
  ds_put(nt[0], DS_NT, red, tid);
  ds_put(nt[1], DS_NT + 1, red, tid);
  ds_put(tsum, DS_TSUM, red, tid);
  ds_put(tsq, DS_TSQ, red, tid);
  ds_put(ssum, DS_SSUM, red, tid);
  ds_put(ssq, DS_SSQ, red, tid);
  ds_put(csq, DS_CSQ, red, tid);
  __syncthreads();
  if (tid < DS_SLOT) {
    const long long slot = ((long long)b * gridDim.y + ks) * gridDim.z + z;
    parts[slot * DS_SLOT + tid] = ((red[tid] + red[DS_SLOT + tid]) + red[2 * DS_SLOT + tid]) + red[3 * DS_SLOT + tid];
  }
}

// one workgroup: the slots -> out[8], every sum in a fixed order
__global__ __launch_bounds__(MT_THREADS) void dino_stats_reduce_kernel(const double* __restrict__ parts, const float* __restrict__ teacher,
                                                                       const float* __restrict__ student, double* __restrict__ out, int G,
                                                                       int V, int B, int K, int KS, int Z) {
  __shared__ double red[MT_WAVES * 6];
  const int tid = threadIdx.x;
  double v6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};                 // cosine sum, tsum, tsq, ssum, ssq, csq
  const int gv = G * V;
  for (long long i = tid; i < (long long)B * gv; i += MT_THREADS) {
    const long long b = i / gv;
    const int r = (int)(i - b * gv), g = r / V, v = r - g * V, z = g / DS_GT, gi = g - z * DS_GT;
    double dot = 0.0, nt = 0.0, ns = 0.0;
    for (int ks = 0; ks < KS; ++ks) {
      const double* s0 = parts + ((b * KS + ks) * Z) * DS_SLOT;
      const double* sz = s0 + (long long)z * DS_SLOT;
      dot += sz[gi * DS_VMAX + v];
      nt += sz[DS_NT + gi];
      ns += s0[DS_NS + v];
    }
    v6[0] += dot / (sqrt(nt) * sqrt(ns) + 1e-8);
  }
  const long long slots = (long long)B * KS * Z;
  for (long long s = tid; s < slots; s += MT_THREADS) {
    const double* p = parts + s * DS_SLOT;
    v6[1] += p[DS_TSUM];
    v6[2] += p[DS_TSQ];
    if (s % Z == 0) {
      v6[3] += p[DS_SSUM];
      v6[4] += p[DS_SSQ];
      v6[5] += p[DS_CSQ];
    }
  }
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const double w = wave_sum_d(v6[j]);
    if ((tid & 63) == 0) red[(tid >> 6) * 6 + j] = w;
  }
  __syncthreads();
  if (tid == 0) {
    double t[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) t[j] = ((red[j] + red[6 + j]) + red[12 + j]) + red[18 + j];
    const double nT = (double)G * B * K, nS = (double)V * B * K;
    out[0] = nT;
    out[1] = (double)teacher[0] + t[1] / nT;
    out[2] = t[2] - t[1] * t[1] / nT;
    out[3] = nS;
    out[4] = (double)student[0] + t[3] / nS;
    out[5] = t[4] - t[3] * t[3] / nS;
    out[6] = t[0];
    out[7] = t[5];
  }
}

// false: the geometry is refused (error set)
bool ds_geometry(int G, int V, int B, int K, const char* who) {
  if (K < 4 || K % 4 != 0) {
    vitssl_set_error("%s: K = %d must be a positive multiple of 4 (rows are read as 16-byte pieces)", who, K);
    return false;
  }
  if (!(1 <= G && G <= V && V <= DS_VMAX)) {
    vitssl_set_error("%s: G = %d teacher and V = %d student views are outside 1 <= G <= V <= %d", who, G, V, DS_VMAX);
    return false;
  }
  if (B < 1 || B > (1 << 22)) {
    vitssl_set_error("%s: B = %d images is outside 1 <= B <= 2^22", who, B);
    return false;
  }
  return true;
}

typedef void (*DsKernel)(const float*, const float*, const float*, double*, int, int, int);
template <int... Vm1>
DsKernel ds_kernel_of(int V, std::integer_sequence<int, Vm1...>) {
  static const DsKernel table[] = {dino_stats_kernel<Vm1 + 1>...};
  return table[V - 1];
}

}  // namespace

extern "C" int64_t vitssl_recon_metrics_workspace_floats(int64_t n, int C, int P) {
  if (n <= 0 || C < 1 || C > 4 || P < 6 || P > 32 || n > (1LL << 40)) return 0;
  return 2 * 2 * rm_plan(n, C, P).groups;                       // 2 doubles a workgroup
}

extern "C" int vitssl_recon_metrics(const float* pred, const float* target, double* acc, int64_t n, int C, int P, float* workspace,
                                    int64_t workspace_floats, void* stream) {
  if (!rm_geometry(n, C, P, "recon_metrics")) return VITSSL_ERR_ARG;
  if (n == 0) return VITSSL_OK;
  VS_CHECK_ARG(pred && target && acc, "recon_metrics: null pointer");
  VS_CHECK_ARG(((uintptr_t)acc & 7) == 0 && ((uintptr_t)workspace & 7) == 0, "recon_metrics: acc and workspace must be 8-byte aligned");
  const RmPlan p = rm_plan(n, C, P);
  VS_CHECK_ARG(p.groups <= INT_MAX, "recon_metrics: %lld patches need %lld workgroups, above the grid limit", (long long)n, p.groups);
  if (!vs_parts(workspace, workspace_floats, 4 * p.groups, "recon_metrics", "vitssl_recon_metrics_workspace_floats")) return VITSSL_ERR_ARG;
  double* parts = (double*)workspace;
  RmTaps taps;
  double sum = 0.0;
  for (int t = 0; t < RM_TAPS; ++t) sum += taps.w[t] = exp(-0.5 * ((t - RM_PAD) / 1.5) * ((t - RM_PAD) / 1.5));
  for (int t = 0; t < RM_TAPS; ++t) taps.w[t] /= sum;
  const long long planes = (long long)n * C;
  const dim3 grid((unsigned)p.groups), block(MT_THREADS);
  hipStream_t s = (hipStream_t)stream;
  if ((P * P) % 4 == 0 && (((uintptr_t)pred | (uintptr_t)target) & 15) == 0)
    hipLaunchKernelGGL(recon_metrics_kernel<true>, grid, block, (size_t)p.lds, s, pred, target, parts, planes, P, p.pl, taps);
  else
    hipLaunchKernelGGL(recon_metrics_kernel<false>, grid, block, (size_t)p.lds, s, pred, target, parts, planes, P, p.pl, taps);
  VS_CHECK_LAUNCH("recon_metrics");
  hipLaunchKernelGGL(recon_metrics_reduce_kernel, dim3(1), block, 0, s, parts, p.groups, acc, 1.0 / (double)(C * P * P),
                     (double)n * C * P * P, (double)n);
  VS_CHECK_LAUNCH("recon_metrics (reduce)");
  return VITSSL_OK;
}

extern "C" int64_t vitssl_dino_stats_workspace_floats(int G, int V, int B, int K) {
  if (G < 1 || V < G || V > DS_VMAX || B < 1 || B > (1 << 22) || K < 4 || K % 4 != 0) return 0;
  const long long KS = (K + DS_KL - 1) / DS_KL, Z = (G + DS_GT - 1) / DS_GT;
  return 2 * (long long)B * KS * Z * DS_SLOT;
}

extern "C" int vitssl_dino_stats(const float* teacher, const float* student, const float* center, double* out, int G, int V, int B,
                                 int K, float* workspace, int64_t workspace_floats, void* stream) {
  VS_CHECK_ARG(teacher && student && out, "dino_stats: null pointer");
  if (!ds_geometry(G, V, B, K, "dino_stats")) return VITSSL_ERR_ARG;
  VS_CHECK_ARG((((uintptr_t)teacher | (uintptr_t)student | (uintptr_t)center) & 15) == 0,
               "dino_stats: teacher, student and center must be 16-byte aligned");
  VS_CHECK_ARG(((uintptr_t)out & 7) == 0 && ((uintptr_t)workspace & 7) == 0, "dino_stats: out and workspace must be 8-byte aligned");
  const int KS = (K + DS_KL - 1) / DS_KL, Z = (G + DS_GT - 1) / DS_GT;
  VS_CHECK_ARG(KS <= 65535, "dino_stats: K = %d needs %d slices of %d, above the grid limit 65535", K, KS, DS_KL);
  if (!vs_parts(workspace, workspace_floats, vitssl_dino_stats_workspace_floats(G, V, B, K), "dino_stats",
                "vitssl_dino_stats_workspace_floats"))
    return VITSSL_ERR_ARG;
  double* parts = (double*)workspace;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ds_kernel_of(V, std::make_integer_sequence<int, DS_VMAX>{}), dim3((unsigned)B, (unsigned)KS, (unsigned)Z),
                     dim3(MT_THREADS), 0, s, teacher, student, center, parts, G, B, K);
  VS_CHECK_LAUNCH("dino_stats");
  hipLaunchKernelGGL(dino_stats_reduce_kernel, dim3(1), dim3(MT_THREADS), 0, s, (const double*)parts, teacher, student, out, G, V, B, K, KS, Z);
  VS_CHECK_LAUNCH("dino_stats (reduce)");
  return VITSSL_OK;
}
