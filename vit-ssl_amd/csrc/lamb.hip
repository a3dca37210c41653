// Segmented LAMB (gfx950): Adam moments, weight decay inside the update and one trust ratio per parameter, over the segment
// table of include/vitssl_optim.h.  include/vitssl_lamb.h declares the entry points and states the formulas; optim.hip is
// untouched (its table helpers are file-local, so the three small ones this file needs are restated here).
//
// Three launches.  The moment and the apply pass are HBM-bound streams shaped like adamw_segments_kernel: 256 threads, one
// 16-byte group per thread and iteration, a grid capped at 2048 workgroups that strides the rest, the work unit 1024 floats
// of ONE segment, found by a binary search over the table's unit starts on wave-uniform values.  The moment pass leaves two
// fp64 partial sums per unit; the reduce adds a segment's slots with one wave; the apply pass recomputes the update from the
// new moments and the old parameter with the same inlined expression, so the step needs no store-sized scratch.
#include "../../include/vitssl_lamb.h"
#include "common.h"
#include <math.h>

namespace {

constexpr int LB_THREADS = 256;
constexpr int LB_WAVES = LB_THREADS / 64;
constexpr int LB_UNIT = 4 * LB_THREADS;     // floats of a work unit: the unit of vitssl_optim_table_build
constexpr int LB_GRID = 2048;               // 256 CUs x 8 workgroups, as optim.hip
constexpr int LB_REDUCE_GRID = 256;         // workgroups of the reduce: 4 segments (waves) each, striding the rest
constexpr int LB_MAX_SEGMENTS = 1 << 20;

static_assert(sizeof(vitssl_optim_segment_t) == 24, "the table image is 24 bytes a segment");

// the table image: nseg entries, then nseg + 1 unit starts (starts[s] = first unit of segment s, starts[nseg] = units)
__device__ __forceinline__ const int* unit_starts(const vitssl_optim_segment_t* segs, int nseg) { return (const int*)(segs + nseg); }

// the segment of unit u: the largest s with starts[s] <= u
__device__ __forceinline__ int find_segment(const int* __restrict__ starts, int nseg, int u) {
  int lo = 0, hi = nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (starts[mid] <= u) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the update r of one element.  Both passes call this one function; the only multiply-add is spelled as an fma, so there is
// no contraction left to the compiler and both passes see the same bits.
__device__ __forceinline__ float lamb_update(float m, float v, float p, float wd, float bc1, float bc2_sqrt, float eps) {
  return fmaf(wd, p, (m / bc1) / (sqrtf(v) / bc2_sqrt + eps));
}

// (a) new m and v, and slots[2u], slots[2u + 1] = sum of p^2, of r^2 over unit u.  cap: units the workspace has slots for.
__global__ __launch_bounds__(LB_THREADS) void lamb_moments_kernel(const float* __restrict__ p, const float* __restrict__ g,
                                                                  float* __restrict__ m, float* __restrict__ v,
                                                                  const vitssl_optim_segment_t* __restrict__ segs, int nseg,
                                                                  float b1, float b2, float eps, float bc1, float bc2_sqrt,
                                                                  float gscale0, const float* __restrict__ sumsq, float max_norm,
                                                                  double* __restrict__ slots, long long cap) {
  __shared__ double red[2][LB_WAVES][2];      // two copies, used by alternate units: one barrier a unit
  const int* __restrict__ starts = unit_starts(segs, nseg);
  const int units = starts[nseg];
  if (units > cap) return;
  float gscale = gscale0;
  if (sumsq) gscale = gscale0 * fminf(1.f, max_norm / (gscale0 * sqrtf(sumsq[0]) + 1e-6f));     // clip_grad_norm_'s coefficient
  int parity = 0;
  for (int u = blockIdx.x; u < units; u += gridDim.x, parity ^= 1) {
    const int s = find_segment(starts, nseg, u);
    const vitssl_optim_segment_t sg = segs[s];
    const long long done = (long long)(u - starts[s]) * LB_UNIT;
    const long long left = sg.n - done;
    const int cnt = left < LB_UNIT ? (int)left : LB_UNIT;
    const long long base = sg.offset + done;
    const float wd = sg.weight_decay;
    double sp = 0.0, sr = 0.0;
    if (4 * (int)threadIdx.x + 4 <= cnt) {
      const long long i = base + 4 * threadIdx.x;
      const f32x4 pv = *(const f32x4*)(p + i);
      const f32x4 gv = *(const f32x4*)(g + i) * gscale;
      f32x4 mv = *(const f32x4*)(m + i);
      f32x4 vv = *(const f32x4*)(v + i);
      mv = mv * b1 + gv * (1.f - b1);
      vv = vv * b2 + gv * gv * (1.f - b2);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double x = pv[r], y = lamb_update(mv[r], vv[r], pv[r], wd, bc1, bc2_sqrt, eps);
        sp = fma(x, x, sp);
        sr = fma(y, y, sr);
      }
      *(f32x4*)(m + i) = mv;
      *(f32x4*)(v + i) = vv;
    }
    if ((int)threadIdx.x < (cnt & 3)) {          // the segment's last, partial group: one element a thread
      const long long i = base + (cnt & ~3) + threadIdx.x;
      const float pv = p[i];
      const float gv = g[i] * gscale;
      const float mv = m[i] * b1 + gv * (1.f - b1);
      const float vv = v[i] * b2 + gv * gv * (1.f - b2);
      const double x = pv, y = lamb_update(mv, vv, pv, wd, bc1, bc2_sqrt, eps);
      sp = fma(x, x, sp);
      sr = fma(y, y, sr);
      m[i] = mv; v[i] = vv;
    }
    sp = wave_sum_d(sp);
    sr = wave_sum_d(sr);
    if ((threadIdx.x & 63) == 0) {
      red[parity][threadIdx.x >> 6][0] = sp;
      red[parity][threadIdx.x >> 6][1] = sr;
    }
    __syncthreads();
    if (threadIdx.x < 2)                         // every unit writes both of its slots
      slots[2 * (long long)u + threadIdx.x] =
          ((red[parity][0][threadIdx.x] + red[parity][1][threadIdx.x]) + red[parity][2][threadIdx.x]) + red[parity][3][threadIdx.x];
  }
}

// (b) one wave per segment: trust[s] from the segment's slots, added in a fixed order
__global__ __launch_bounds__(LB_THREADS) void lamb_trust_kernel(const vitssl_optim_segment_t* __restrict__ segs, int nseg,
                                                                const double* __restrict__ slots, long long cap, int flags,
                                                                float* __restrict__ trust) {
  const int* __restrict__ starts = unit_starts(segs, nseg);
  const int lane = threadIdx.x & 63;
  const bool fits = starts[nseg] <= cap;
  for (int s = blockIdx.x * LB_WAVES + (threadIdx.x >> 6); s < nseg; s += gridDim.x * LB_WAVES) {
    double t = 1.0;
    if (!fits) {
      t = (double)NAN;
    } else if (segs[s].weight_decay != 0.f || (flags & VITSSL_LAMB_ALWAYS_ADAPT)) {
      double sp = 0.0, sr = 0.0;
      for (int u = starts[s] + lane; u < starts[s + 1]; u += 64) {
        sp += slots[2 * (long long)u];
        sr += slots[2 * (long long)u + 1];
      }
      const double pn = sqrt(wave_sum_d(sp)), rn = sqrt(wave_sum_d(sr));
      if (pn > 0.0 && rn > 0.0) t = pn / rn;
      if ((flags & VITSSL_LAMB_TRUST_CLIP) && t > 1.0) t = 1.0;
    }
    if (lane == 0) trust[s] = (float)t;
  }
}

// (c) p -= lr_s * trust_s * r, with r recomputed from the new m, v and the old p
__global__ __launch_bounds__(LB_THREADS) void lamb_apply_kernel(float* __restrict__ p, const float* __restrict__ m,
                                                                const float* __restrict__ v,
                                                                const vitssl_optim_segment_t* __restrict__ segs, int nseg,
                                                                float lr0, float eps, float bc1, float bc2_sqrt,
                                                                const float* __restrict__ trust, long long cap) {
  const int* __restrict__ starts = unit_starts(segs, nseg);
  const int units = starts[nseg];
  if (units > cap) return;
  for (int u = blockIdx.x; u < units; u += gridDim.x) {
    const int s = find_segment(starts, nseg, u);
    const vitssl_optim_segment_t sg = segs[s];
    const long long done = (long long)(u - starts[s]) * LB_UNIT;
    const long long left = sg.n - done;
    const int cnt = left < LB_UNIT ? (int)left : LB_UNIT;
    const long long base = sg.offset + done;
    const float wd = sg.weight_decay;
    const float neg_step = -(lr0 * sg.lr_scale * trust[s]);
    if (4 * (int)threadIdx.x + 4 <= cnt) {
      const long long i = base + 4 * threadIdx.x;
      f32x4 pv = *(const f32x4*)(p + i);
      const f32x4 mv = *(const f32x4*)(m + i);
      const f32x4 vv = *(const f32x4*)(v + i);
#pragma unroll
      for (int r = 0; r < 4; ++r) pv[r] = fmaf(neg_step, lamb_update(mv[r], vv[r], pv[r], wd, bc1, bc2_sqrt, eps), pv[r]);
      *(f32x4*)(p + i) = pv;
    }
    if ((int)threadIdx.x < (cnt & 3)) {
      const long long i = base + (cnt & ~3) + threadIdx.x;
      const float pv = p[i];
      p[i] = fmaf(neg_step, lamb_update(m[i], v[i], pv, wd, bc1, bc2_sqrt, eps), pv);
    }
  }
}

}  // namespace

extern "C" int64_t vitssl_lamb_workspace_bytes(const vitssl_optim_segment_t* segments, int nseg) {
  if (!segments || nseg <= 0 || nseg > LB_MAX_SEGMENTS) return 0;
  int64_t units = 0;
  for (int s = 0; s < nseg; ++s) {
    if (segments[s].n <= 0) return 0;
    units += (segments[s].n + LB_UNIT - 1) / LB_UNIT;
  }
  return units * 2 * (int64_t)sizeof(double);            // sum of p^2 and of r^2 per unit
}

extern "C" int vitssl_lamb_segments(float* p, const float* g, float* m, float* v, const void* table, int nseg, float lr, float beta1,
                                    float beta2, float eps, int step, float gscale, const float* sumsq, float max_norm, int flags,
                                    float* trust, void* workspace, int64_t workspace_bytes, void* stream) {
  VS_CHECK_ARG(p && g && m && v, "lamb_segments: p, g, m or v is NULL");
  VS_CHECK_ARG(step >= 1, "lamb_segments: step = %d must be at least 1", step);
  VS_CHECK_ARG(table, "lamb_segments: table is NULL (the device copy of a vitssl_optim_table_build image)");
  VS_CHECK_ARG(trust, "lamb_segments: trust is NULL (nseg floats, required)");
  VS_CHECK_ARG(nseg > 0 && nseg <= LB_MAX_SEGMENTS, "lamb_segments: nseg = %d is outside 1 .. %d", nseg, LB_MAX_SEGMENTS);
  VS_CHECK_ARG((flags & ~(VITSSL_LAMB_ALWAYS_ADAPT | VITSSL_LAMB_TRUST_CLIP)) == 0, "lamb_segments: flags = 0x%x has unknown bits", flags);
  VS_CHECK_ARG((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0 && ((uintptr_t)table & 7) == 0 &&
                   ((uintptr_t)trust & 3) == 0,
               "lamb_segments: p, g, m, v must be 16-byte, table 8-byte, trust 4-byte aligned");
  VS_CHECK_ARG(!sumsq || max_norm > 0.f, "lamb_segments: max_norm = %g must be positive when sumsq is given", (double)max_norm);
  const int64_t least = (int64_t)nseg * 2 * (int64_t)sizeof(double);
  VS_CHECK_ARG(workspace && workspace_bytes >= least,
               "lamb_segments: workspace of %lld bytes, %d segments need at least %lld (vitssl_lamb_workspace_bytes)",
               (long long)(workspace ? workspace_bytes : 0), nseg, (long long)least);
  VS_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "lamb_segments: workspace must be 8-byte aligned");
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  const float bc1f = (float)bc1, bc2_sqrt = (float)sqrt(bc2);
  const vitssl_optim_segment_t* segs = (const vitssl_optim_segment_t*)table;
  double* slots = (double*)workspace;
  const long long cap = (long long)(workspace_bytes / (2 * (int64_t)sizeof(double)));
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(lamb_moments_kernel, dim3(LB_GRID), dim3(LB_THREADS), 0, s, p, g, m, v, segs, nseg, beta1, beta2, eps, bc1f,
                     bc2_sqrt, gscale, sumsq, max_norm, slots, cap);
  VS_CHECK_LAUNCH("lamb_segments (moments)");
  const int rgrid = (nseg + LB_WAVES - 1) / LB_WAVES < LB_REDUCE_GRID ? (nseg + LB_WAVES - 1) / LB_WAVES : LB_REDUCE_GRID;
  hipLaunchKernelGGL(lamb_trust_kernel, dim3(rgrid), dim3(LB_THREADS), 0, s, segs, nseg, (const double*)slots, cap, flags, trust);
  VS_CHECK_LAUNCH("lamb_segments (trust)");
  hipLaunchKernelGGL(lamb_apply_kernel, dim3(LB_GRID), dim3(LB_THREADS), 0, s, p, (const float*)m, (const float*)v, segs, nseg, lr, eps,
                     bc1f, bc2_sqrt, (const float*)trust, cap);
  VS_CHECK_LAUNCH("lamb_segments (apply)");
  return VITSSL_OK;
}
