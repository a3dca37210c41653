// Segmented AdamW (gfx950): per-parameter learning-rate multipliers and weight decay over the flat store, and the sum of
// squares of the gradient for clipping its global norm on the device.  include/vitssl_optim.h declares the entry points
// and the segment table; vitssl_adamw (elementwise.hip) is untouched and stays the default step.
//
// Both kernels are HBM-bound streams shaped like adamw_kernel: 256 threads, one 16-byte group per thread and iteration,
// a grid capped at 2048 workgroups that strides the rest.  The work unit is 1024 floats of ONE segment (the last unit of
// a segment is short; its last group may be partial and is done one element a thread), so unit u of a one-segment table
// covers the floats adamw_kernel's workgroup u covers.  A workgroup finds the segment of its unit by a binary search over
// the table's unit starts: one search per 1024 floats, on wave-uniform values (scalar loads of a table that stays cached);
// there is no per-element search.
#include "../../include/vitssl_optim.h"
#include "common.h"
#include <math.h>

namespace {

constexpr int OP_THREADS = 256;
constexpr int OP_WAVES = OP_THREADS / 64;
constexpr int OP_UNIT = 4 * OP_THREADS;     // floats of a work unit
constexpr int OP_GRID = 2048;               // 256 CUs x 8 workgroups, as stream_grid of elementwise.hip
constexpr int OP_MAX_SEGMENTS = 1 << 20;

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

// the update of adamw_kernel (elementwise.hip), expression for expression: the same contraction gives the same bits
__global__ __launch_bounds__(OP_THREADS) void adamw_segments_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                                    float* __restrict__ m, float* __restrict__ v,
                                                                    const vitssl_optim_segment_t* __restrict__ segs, int nseg,
                                                                    float lr0, float b1, float b2, float eps, float bc1,
                                                                    float bc2_sqrt, float gscale0, const float* __restrict__ sumsq,
                                                                    float max_norm) {
  const int* __restrict__ starts = unit_starts(segs, nseg);
  const int units = starts[nseg];
  float gscale = gscale0;
  if (sumsq) gscale = gscale0 * fminf(1.f, max_norm / (gscale0 * sqrtf(sumsq[0]) + 1e-6f));     // clip_grad_norm_'s coefficient
  for (int u = blockIdx.x; u < units; u += gridDim.x) {
    const int s = find_segment(starts, nseg, u);
    const vitssl_optim_segment_t sg = segs[s];
    const long long done = (long long)(u - starts[s]) * OP_UNIT;
    const long long left = sg.n - done;
    const int cnt = left < OP_UNIT ? (int)left : OP_UNIT;
    const long long base = sg.offset + done;
    const float lr = lr0 * sg.lr_scale, wd = sg.weight_decay;
    const float step_size = lr / bc1;
    if (4 * (int)threadIdx.x + 4 <= cnt) {
      const long long i = base + 4 * threadIdx.x;
      f32x4 pv = *(const f32x4*)(p + i);
      const f32x4 gv = *(const f32x4*)(g + i) * gscale;
      f32x4 mv = *(const f32x4*)(m + i);
      f32x4 vv = *(const f32x4*)(v + i);
      pv *= (1.f - lr * wd);
      mv = mv * b1 + gv * (1.f - b1);
      vv = vv * b2 + gv * gv * (1.f - b2);
#pragma unroll
      for (int r = 0; r < 4; ++r) pv[r] -= step_size * mv[r] / (sqrtf(vv[r]) / bc2_sqrt + eps);
      *(f32x4*)(p + i) = pv;
      *(f32x4*)(m + i) = mv;
      *(f32x4*)(v + i) = vv;
    }
    if ((int)threadIdx.x < (cnt & 3)) {          // the segment's last, partial group: one element a thread, as adamw_kernel's tail
      const long long i = base + (cnt & ~3) + threadIdx.x;
      float pv = p[i] * (1.f - lr * wd);
      const float gv = g[i] * gscale;
      const float mv = m[i] * b1 + gv * (1.f - b1);
      const float vv = v[i] * b2 + gv * gv * (1.f - b2);
      pv -= step_size * mv / (sqrtf(vv) / bc2_sqrt + eps);
      p[i] = pv; m[i] = mv; v[i] = vv;
    }
  }
}

// parts[workgroup] = sum of g^2 over the workgroup's units, in fp64 (the squares of fp32 values are exact there)
__global__ __launch_bounds__(OP_THREADS) void grad_sumsq_kernel(const float* __restrict__ g,
                                                                const vitssl_optim_segment_t* __restrict__ segs, int nseg,
                                                                double* __restrict__ parts) {
  __shared__ double red[OP_WAVES];
  const int* __restrict__ starts = unit_starts(segs, nseg);
  const int units = starts[nseg];
  double acc = 0.0;
  for (int u = blockIdx.x; u < units; u += gridDim.x) {
    const int s = find_segment(starts, nseg, u);
    const long long done = (long long)(u - starts[s]) * OP_UNIT;
    const long long left = segs[s].n - done;
    const int cnt = left < OP_UNIT ? (int)left : OP_UNIT;
    const long long base = segs[s].offset + done;
    const int e = 4 * threadIdx.x;
    if (e + 4 <= cnt) {
      const f32x4 x = *(const f32x4*)(g + base + e);
#pragma unroll
      for (int r = 0; r < 4; ++r) acc = fma((double)x[r], (double)x[r], acc);
    } else {
      for (int j = e; j < cnt; ++j) {
        const double x = g[base + j];
        acc = fma(x, x, acc);
      }
    }
  }
  acc = wave_sum_d(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) parts[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];      // every workgroup writes its slot
}

// one workgroup: out[0] = the slots added in a fixed order
__global__ __launch_bounds__(OP_THREADS) void grad_sumsq_reduce_kernel(const double* __restrict__ parts, int nparts,
                                                                       float* __restrict__ out) {
  __shared__ double red[OP_WAVES];
  double a = 0.0;
  for (int i = threadIdx.x; i < nparts; i += OP_THREADS) a += parts[i];
  a = wave_sum_d(a);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = (float)(((red[0] + red[1]) + red[2]) + red[3]);
}

}  // namespace

extern "C" int64_t vitssl_optim_table_bytes(int nseg) {
  if (nseg <= 0 || nseg > OP_MAX_SEGMENTS) return 0;
  return (int64_t)nseg * (int64_t)sizeof(vitssl_optim_segment_t) + ((int64_t)nseg + 1) * (int64_t)sizeof(int);
}

extern "C" int vitssl_optim_table_build(const vitssl_optim_segment_t* segments, int nseg, int64_t numel, void* image,
                                        int64_t image_bytes) {
  VS_CHECK_ARG(segments && image, "optim_table_build: null pointer");
  VS_CHECK_ARG(nseg > 0 && nseg <= OP_MAX_SEGMENTS, "optim_table_build: nseg = %d is outside 1 .. %d", nseg, OP_MAX_SEGMENTS);
  VS_CHECK_ARG(image_bytes >= vitssl_optim_table_bytes(nseg),
               "optim_table_build: image of %lld bytes, %d segments need %lld (vitssl_optim_table_bytes)", (long long)image_bytes, nseg,
               (long long)vitssl_optim_table_bytes(nseg));
  int64_t end = 0, units = 0;
  for (int s = 0; s < nseg; ++s) {
    const vitssl_optim_segment_t& sg = segments[s];
    VS_CHECK_ARG(sg.n > 0, "optim_table_build: segment %d has n = %lld", s, (long long)sg.n);
    VS_CHECK_ARG(sg.offset >= 0 && sg.offset % 4 == 0,
                 "optim_table_build: segment %d starts at float %lld, not a non-negative multiple of 4 (16-byte loads)", s,
                 (long long)sg.offset);
    VS_CHECK_ARG(sg.offset >= end, "optim_table_build: segment %d starts at float %lld, before the end %lld of the one before it", s,
                 (long long)sg.offset, (long long)end);
    VS_CHECK_ARG(sg.n <= numel && sg.offset <= numel - sg.n, "optim_table_build: segment %d (%lld + %lld) ends behind the store's %lld floats",
                 s, (long long)sg.offset, (long long)sg.n, (long long)numel);
    VS_CHECK_ARG(isfinite(sg.lr_scale) && isfinite(sg.weight_decay), "optim_table_build: segment %d has a non-finite lr_scale or weight_decay", s);
    end = sg.offset + sg.n;
    units += (sg.n + OP_UNIT - 1) / OP_UNIT;
    VS_CHECK_ARG(units <= INT_MAX, "optim_table_build: more than 2^31 units of %d floats", OP_UNIT);
  }
  memcpy(image, segments, (size_t)nseg * sizeof(vitssl_optim_segment_t));
  int* starts = (int*)((char*)image + (size_t)nseg * sizeof(vitssl_optim_segment_t));
  int u = 0;
  for (int s = 0; s < nseg; ++s) {
    starts[s] = u;
    u += (int)((segments[s].n + OP_UNIT - 1) / OP_UNIT);
  }
  starts[nseg] = u;
  return VITSSL_OK;
}

extern "C" int64_t vitssl_grad_sumsq_workspace_bytes(int nseg) {
  if (nseg <= 0 || nseg > OP_MAX_SEGMENTS) return 0;
  return (int64_t)OP_GRID * (int64_t)sizeof(double);         // one slot a workgroup; the grid does not depend on the table
}

extern "C" int vitssl_grad_sumsq(const float* g, const void* table, int nseg, float* out, void* workspace, int64_t workspace_bytes,
                                 void* stream) {
  VS_CHECK_ARG(g && out, "grad_sumsq: null pointer");
  VS_CHECK_ARG(table, "grad_sumsq: table is NULL (the device copy of a vitssl_optim_table_build image)");
  VS_CHECK_ARG(nseg > 0 && nseg <= OP_MAX_SEGMENTS, "grad_sumsq: nseg = %d is outside 1 .. %d", nseg, OP_MAX_SEGMENTS);
  VS_CHECK_ARG(((uintptr_t)g & 15) == 0 && ((uintptr_t)table & 7) == 0, "grad_sumsq: g must be 16-byte, table 8-byte aligned");
  const int64_t need = vitssl_grad_sumsq_workspace_bytes(nseg);
  VS_CHECK_ARG(workspace && workspace_bytes >= need, "grad_sumsq: workspace of %lld bytes, need %lld (vitssl_grad_sumsq_workspace_bytes)",
               (long long)(workspace ? workspace_bytes : 0), (long long)need);
  VS_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "grad_sumsq: workspace must be 8-byte aligned");
  double* parts = (double*)workspace;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(OP_GRID), dim3(OP_THREADS), 0, s, g, (const vitssl_optim_segment_t*)table, nseg, parts);
  VS_CHECK_LAUNCH("grad_sumsq");
  hipLaunchKernelGGL(grad_sumsq_reduce_kernel, dim3(1), dim3(OP_THREADS), 0, s, parts, OP_GRID, out);
  VS_CHECK_LAUNCH("grad_sumsq (reduce)");
  return VITSSL_OK;
}

extern "C" int vitssl_adamw_segments(float* p, const float* g, float* m, float* v, const void* table, int nseg, float lr, float beta1,
                                     float beta2, float eps, int step, float gscale, const float* sumsq, float max_norm, void* stream) {
  VS_CHECK_ARG(p && g && m && v && step >= 1, "adamw_segments: bad args");
  VS_CHECK_ARG(table, "adamw_segments: table is NULL (the device copy of a vitssl_optim_table_build image)");
  VS_CHECK_ARG(nseg > 0 && nseg <= OP_MAX_SEGMENTS, "adamw_segments: nseg = %d is outside 1 .. %d", nseg, OP_MAX_SEGMENTS);
  VS_CHECK_ARG((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0 && ((uintptr_t)table & 7) == 0,
               "adamw_segments: p, g, m, v must be 16-byte, table 8-byte aligned");
  VS_CHECK_ARG(!sumsq || max_norm > 0.f, "adamw_segments: max_norm = %g must be positive when sumsq is given", (double)max_norm);
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  hipLaunchKernelGGL(adamw_segments_kernel, dim3(OP_GRID), dim3(OP_THREADS), 0, (hipStream_t)stream, p, g, m, v,
                     (const vitssl_optim_segment_t*)table, nseg, lr, beta1, beta2, eps, (float)bc1, (float)sqrt(bc2), gscale, sumsq,
                     max_norm);
  VS_CHECK_LAUNCH("adamw_segments");
  return VITSSL_OK;
}
