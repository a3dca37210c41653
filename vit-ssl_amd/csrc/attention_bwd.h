// Parts that the backward kernels of attention.hip share (fused: up to 128 tokens, persistent: 129-224, pipelined: 225-256).
// Only arithmetic and LDS reads live here; which loads are requested when, every wait on a DMA or a store and every barrier stay in
// the kernel that owns the schedule.  Every helper here leaves the generated code of all three kernels as it was with the code
// written out; the pieces for which no such helper was found stay in the kernels (profiles/attn_bwd_refactor_isa.txt lists them).
// Naming as in attention.hip: wave w owns keys 32 w .. 32 w + 31 (key tiles kt = 0, 1), a step sweeps 32 queries,
// g = lane >> 4, li = lane & 15.  The kernels pass their own g / li: recomputed from `lane` in here, the same values moved registers.
#pragma once
#include "attention_tiles.h"

namespace vitssl_attn {

// exchange-image row in bytes (Np keys as bf16); + 16 makes the 8-byte column reads of the dQ product conflict-free
template <int NS>
constexpr int SX_ROW = 32 * NS * 2 + 16;

__device__ __forceinline__ bf16x8 join_tr(const s16x4& lo, const s16x4& hi) {
  typedef __attribute__((ext_vector_type(8))) short s16x8;
  const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, v);
}

// score accumulators of one key tile start at -inf for a masked key (>= N): p = dS = 0 there
__device__ __forceinline__ f32x4 key_mask_init1(int key, int N) {
  const float mi = key < N ? 0.f : -INFINITY;
  return f32x4{mi, mi, mi, mi};
}
__device__ __forceinline__ void zero_dkdv(f32x4 (&dk)[4][2], f32x4 (&dv)[4][2]) {
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      dv[dt][kt] = f32x4{0.f, 0.f, 0.f, 0.f};
      dk[dt][kt] = dv[dt][kt];
    }
}

// delta (pre-multiplied by 1/sqrt(dh)) of slice s = rows 32 s .. 32 s + 31, by ONE wave, 2 lanes per row; O from ring slot s % 3 of Or
__device__ __forceinline__ void delta_slice(float* del_s, const char* Or, const char* Dt, int s, int N, int lane) {
  const int rl = lane >> 1, half = lane & 1;
  const int row = 32 * s + rl;
  const char* orow = Or + (s % 3) * 32 * ROWB;
  float part = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const u32x4 ov = *(const u32x4*)(orow + tile_off(rl, half * 4 + j));
    const u32x4 dv = *(const u32x4*)(Dt + tile_off(row, half * 4 + j));
#pragma unroll
    for (int w = 0; w < 4; ++w) part += bf_lo(ov[w]) * bf_lo(dv[w]) + bf_hi(ov[w]) * bf_hi(dv[w]);
  }
  part += __shfl_xor(part, 1, 64);
  if (half == 0) del_s[row] = row < N ? part * SCALE : 0.f;
}

// The K^T fragments of a wave's dQ tile (16 head dimensions x all keys) are the same in every step: read once, 4 NS registers
// (re-reading them in every step instead: 223 against 218 us at B = 256, H = 12, N = 196).  The caller waits (lgkmcnt).
template <int NS>
__device__ __forceinline__ void load_kt(s16x4 (&klo)[NS], s16x4 (&khi)[NS], unsigned kaddr) {
  static_for<NS>([&](auto st_c) {
    constexpr int st = decltype(st_c)::value;
    ds_read_tr16<4096 * st>(klo[st], kaddr);
    ds_read_tr16<4096 * st + 2048>(khi[st], kaddr);
  });
}
// dQ^T[d][q] = sum_key K[key][d] dS[q][key] for one wave's (query tile qt_w, column slice) of a step, from exchange image sx and
// the held K^T fragments.  Two accumulators halve the dependent-MFMA chain.
template <int NS>
__device__ __forceinline__ f32x4 dq_product(const char* sx, int qt_w, int g, int li, const s16x4 (&klo)[NS], const s16x4 (&khi)[NS]) {
  const char* rowp = sx + (16 * qt_w + li) * SX_ROW<NS> + 8 * g;
  u32x2 dlo[NS], dhi[NS];
#pragma unroll
  for (int st = 0; st < NS; ++st) {
    dlo[st] = *(const u32x2*)(rowp + 64 * st);        // keys 32st + 4g .. +3
    dhi[st] = *(const u32x2*)(rowp + 64 * st + 32);   // keys 32st + 16 + 4g .. +3
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
#pragma unroll
  for (int st = 0; st < NS; ++st) {
    const u32x4 w = {dlo[st][0], dlo[st][1], dhi[st][0], dhi[st][1]};
    if (st & 1) acc1 = MFMA16(join_tr(klo[st], khi[st]), __builtin_bit_cast(bf16x8, w), acc1);
    else acc0 = MFMA16(join_tr(klo[st], khi[st]), __builtin_bit_cast(bf16x8, w), acc0);
  }
  return acc0 + acc1;
}

// the launch's max |dqkv| joins *qamax (non-negative floats order like their bit patterns)
__device__ __forceinline__ void publish_amax(float qmax, float* qamax, int lane) {
  qmax = wave_max(qmax);
  unsigned* slot = (unsigned*)qamax;
  if (lane == 0 && __float_as_uint(qmax) > __builtin_nontemporal_load(slot)) atomicMax(slot, __float_as_uint(qmax));
}

}  // namespace vitssl_attn
