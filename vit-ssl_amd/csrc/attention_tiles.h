// Tile layout, fragment reads and row stores shared by the attention kernels (attention.hip: up to 256 tokens, one
// workgroup per (image, head)), and the fragment packing, row stores and constants that the streaming kernels of
// attention_hd.hip take from here too.
#pragma once
#include "common.h"

namespace vitssl_attn {

constexpr int DH = 64;
constexpr int ROWB = DH * 2;  // bytes per tile row

__device__ __forceinline__ int tile_off(int row, int ch16) { return row * ROWB + ((ch16 ^ (((row >> 1) & 3) << 1)) << 4); }

// cooperative load of X[n][0..63] (n < N, row stride `stride` elements) into a swizzled LDS tile of Np rows
__device__ __forceinline__ void load_tile(char* lds, const bf16_t* g, long long stride, int N, int Np, int tid, int nthreads) {
  for (int idx = tid; idx < Np * 8; idx += nthreads) {
    const int row = idx >> 3, ch = idx & 7;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (row < N) v = *(const u32x4*)(g + (long long)row * stride + ch * 8);
    *(u32x4*)(lds + tile_off(row, ch)) = v;
  }
}

// asynchronous version: LDS-DMA (buffer_load ... lds), 1 KiB = 8 tile rows per wave
// instruction, the swizzle applied on the SOURCE chunk (same involution as tile_off);
// rows >= N fall outside the buffer descriptor and are zero-filled by the hardware.
// Completion = this wave's vmcnt, then a workgroup barrier.  Np/8 instructions in total,
// spread over NWAVES waves; returns how many this wave issued.
template <int NWAVES>
__device__ __forceinline__ int dma_tile(char* lds, const bf16_t* g, long long stride, int N, int Np, int wave, int lane) {
  const unsigned bytes = (unsigned)((long long)(N - 1) * stride * 2 + ROWB);
  __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)g, 0, (int)bytes, 0x00020000);
  int n = 0;
  for (int i = wave; i < Np / 8; i += NWAVES) {
    const int row = i * 8 + (lane >> 3);
    const int c = lane & 7;
    const int sc = c ^ (((row >> 1) & 3) << 1);
    const unsigned voff = (unsigned)((long long)row * stride * 2 + sc * 16);
    dma16_to_lds(rs, lds + i * 1024, voff);
    ++n;
  }
  return n;
}

// natural fragment (8 consecutive d) of row `row`, k-step kk, from an LDS tile
__device__ __forceinline__ bf16x8 lds_frag(const char* tile, int row, int kk, int lane) {
  return *(const bf16x8*)(tile + tile_off(row, 4 * kk + (lane >> 4)));
}
// natural fragment straight from global (zero past N)
__device__ __forceinline__ bf16x8 glb_frag(const bf16_t* g, long long stride, int row, int kk, int N, int lane) {
  u32x4 v = {0u, 0u, 0u, 0u};
  if (row < N) v = *(const u32x4*)(g + (long long)row * stride + 32 * kk + 8 * (lane >> 4));
  return __builtin_bit_cast(bf16x8, v);
}
// transposed fragment for contraction step s (rows 32s..32s+31, permuted order), columns d0..d0+15
__device__ __forceinline__ bf16x8 tr_frag(const char* tile, int s, int dt, int lane) {
  const int g = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;
  const int r0 = 32 * s + 4 * g + q;
  const int r1 = r0 + 16;
  const int ch = 2 * dt;  // 16-B chunk of column d0 = 16*dt; lanes pp>=2 use the odd chunk
  const char* a0 = tile + tile_off(r0, ch + (pp >> 1)) + 8 * (pp & 1);
  const char* a1 = tile + tile_off(r1, ch + (pp >> 1)) + 8 * (pp & 1);
  s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)a0);
  s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)a1);
  typedef __attribute__((ext_vector_type(8))) short s16x8;
  s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, v);
}
// accumulator tiles (2s, 2s+1) -> B-operand fragment of contraction step s
__device__ __forceinline__ bf16x8 pack_frag(const f32x4& a, const f32x4& b) {
  u32x4 w = {pack_bf2(a[0], a[1]), pack_bf2(a[2], a[3]), pack_bf2(b[0], b[1]), pack_bf2(b[2], b[3])};
  return __builtin_bit_cast(bf16x8, w);
}

#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0)

// One 128-byte row of 64 bf16 outputs.  A lane holds columns 16 dt + 4g .. +3 of the tiles
// dt = 2p, 2p+1; exchanging halves between lane rows (g, g^1) with v_permlane16_swap gives every
// lane 8 contiguous columns, i.e. one 16-byte store instead of two 8-byte ones (64-byte
// segments per row per instruction; HBM writes are sensitive to this).
// Both lanes of an exchanging pair share lane&15, so a row predicate on lane&15 is safe.
__device__ __forceinline__ void store_row_pair16(bf16_t* row, int p, int g, const u32x2& w0, const u32x2& w1) {
  auto lo = __builtin_amdgcn_permlane16_swap(w0[0], w1[0], false, false);
  auto hi = __builtin_amdgcn_permlane16_swap(w0[1], w1[1], false, false);
  const int odd = g & 1;
  const u32x4 v = {lo[0], hi[0], lo[1], hi[1]};
  *(u32x4*)(row + (2 * p + odd) * 16 + 4 * (g - odd)) = v;
}
// d[t] of lane row g = dword t*4 + g of a 16-dword row  ->  lane row g gets dwords 4g .. 4g+3 (v_permlane32_swap trades
// the wave halves, v_permlane16_swap the odd / even lane rows)
__device__ __forceinline__ u32x4 lane_rows_transpose4(const unsigned (&d)[4]) {
  auto s02 = __builtin_amdgcn_permlane32_swap(d[0], d[2], false, false);
  auto s13 = __builtin_amdgcn_permlane32_swap(d[1], d[3], false, false);
  auto e = __builtin_amdgcn_permlane16_swap(s02[0], s13[0], false, false);
  auto f = __builtin_amdgcn_permlane16_swap(s02[1], s13[1], false, false);
  return u32x4{e[0], e[1], f[0], f[1]};
}
__device__ __forceinline__ void store_row_pair16_if(bool ok, bf16_t* row, int p, int g, const u32x2& w0, const u32x2& w1) {
  auto lo = __builtin_amdgcn_permlane16_swap(w0[0], w1[0], false, false);
  auto hi = __builtin_amdgcn_permlane16_swap(w0[1], w1[1], false, false);
  const int odd = g & 1;
  const u32x4 v = {lo[0], hi[0], lo[1], hi[1]};
  if (ok) *(u32x4*)(row + (2 * p + odd) * 16 + 4 * (g - odd)) = v;
}
__device__ __forceinline__ u32x2 pack4(const f32x4& o) { return u32x2{pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3])}; }

constexpr float LOG2E = 1.4426950408889634f;
constexpr float SCALE = 0.125f;                  // 1/sqrt(64)
constexpr float SCALE_LOG2E = SCALE * LOG2E;

// attention_hd.hip: launches of the streaming kernels at dh = 64 for 257 .. ATTN_LONG_MAX_N tokens (bf16 operands)
constexpr int ATTN_LONG_MAX_N = 2048;
int attn_long_fwd(const bf16_t* qkv, bf16_t* out, float* lse, float* probs, int B, int N, int H, hipStream_t s, int* grid);
int attn_long_bwd(const bf16_t* qkv, const bf16_t* out, const bf16_t* dout, const float* lse, bf16_t* dqkv, float* delta_ws,
                  int B, int N, int H, hipStream_t s);

}  // namespace vitssl_attn
