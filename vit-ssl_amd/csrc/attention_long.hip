// Streaming multi-head self-attention for 257-2048 tokens (dh = 64, bf16 operands), gfx950.
//
// attention.hip keeps all keys and values of one (image, head) item in LDS, which ends at 256 tokens.  Here a
// workgroup owns one TILE of an item and the other side of the product streams through LDS in 64-row tiles, two
// buffers, the next tile arriving by LDS-DMA while the current one is multiplied:
//   forward   one workgroup per (item, 128 queries): K / V tiles stream, online softmax (running maximum and running sum
//             in fp32, the output accumulators rescaled whenever the maximum moves), writes out and lse;
//   probs     (return_attn only) a separate kernel recomputes S per (item, 128 queries) and writes exp(S - lse); the
//             forward itself never sees the probs pointer, so `out` cannot depend on it;
//   backward  three launches, no atomics, every output element written once by one workgroup in a fixed order:
//             delta = rowsum(dO * O) per row into the caller's workspace; dK / dV, one workgroup per (item, 128 keys)
//             sweeping Q / dO tiles; dQ, one workgroup per (item, 128 queries) sweeping K / V tiles.  Both recompute
//             P = exp(S - lse): 7 matrix products of N^2 x 64 instead of the fused backward's 5.
// Four waves per workgroup, a wave owns 32 rows of the workgroup's tile as two 16-row MFMA tiles, so that every fragment
// read from LDS feeds two MFMAs.  Orientations, tile image and fragment maps are those of attention.hip
// (attention_tiles.h).  Workgroups are numbered item-major and remapped so that one XCD gets a contiguous run: the tiles
// of an item, and the heads of an image, re-read their streamed operands from one L2.
#include "common.h"
#include "attention_tiles.h"

namespace {

using namespace vitssl_attn;

constexpr int LW = 4;                 // waves per workgroup
constexpr int WG_ROWS = 32 * LW;      // rows of the stationary tile (queries; keys in the dK / dV kernel)
constexpr int ST_ROWS = 64;           // rows of a streamed tile
constexpr int ST_BYTES = ST_ROWS * ROWB;

struct Item {
  const bf16_t *q, *k, *v;
  long long row0;     // first token row of the image, in rows of [B*N]
  long long lse0;     // item * N
};
__device__ __forceinline__ Item item_of(const bf16_t* qkv, int item, int N, int H) {
  const int b = item / H, h = item - b * H;
  Item it;
  it.row0 = (long long)b * N;
  it.q = qkv + it.row0 * (3LL * H * DH) + h * DH;
  it.k = it.q + (long long)H * DH;
  it.v = it.k + (long long)H * DH;
  it.lse0 = (long long)item * N;
  return it;
}

// rows [row0, row0 + 64) of X[n][0..63] (n < N) into a streamed-tile buffer; rows >= N arrive as zeros
__device__ __forceinline__ void dma_stream_tile(char* lds, const bf16_t* g, long long stride, int row0, int N, int wave, int lane) {
  dma_tile<LW>(lds, g + (long long)row0 * stride, stride, N - row0, ST_ROWS, wave, lane);
}
// 64 consecutive floats x[row0 ..] (zeros past N) into LDS: one wave instruction
__device__ __forceinline__ void dma_row_scalars(float* lds, const float* x, int row0, int N, int lane) {
  __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, N * 4, 0x00020000);
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, LDS_PTR((char*)lds), 4, (unsigned)(row0 + lane) * 4u, 0, 0, 0);
}
// this wave's share of the tile requested last has landed, and (behind the barrier) everybody's; every wave is done with the other buffer
__device__ __forceinline__ void stream_sync() {
  __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0) alone, as a builtin: hipcc then knows the earlier ordinary loads are complete too
  raw_barrier();
}

// tile-relative byte address of this lane's transposed reads (tr_frag of attention_tiles.h: row 4g + q of a 32-row step,
// column slice dt); the step and the second 16 rows are immediates (4096 st, + 2048): the swizzle ignores both
__device__ __forceinline__ void tr_lane_offsets(unsigned (&rel)[4], int lane) {
  const int g = lane >> 4, tq = (lane >> 2) & 3, tpp = lane & 3;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) rel[dt] = (unsigned)(tile_off(4 * g + tq, 2 * dt + (tpp >> 1)) + 8 * (tpp & 1));
}
// the four transposed fragments (column slices dt) of contraction step ST of the tile at LDS address `base`.  Inline asm
// reads (common.h, ds_read_tr16): the builtin would drain the next tile's LDS-DMA in front of every read.
template <int ST>
__device__ __forceinline__ void tr_frags(bf16x8 (&f)[4], unsigned base, const unsigned (&rel)[4]) {
  s16x4 lo[4], hi[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    ds_read_tr16<4096 * ST>(lo[dt], base + rel[dt]);
    ds_read_tr16<4096 * ST + 2048>(hi[dt], base + rel[dt]);
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  typedef __attribute__((ext_vector_type(8))) short s16x8;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    const s16x8 v = {lo[dt][0], lo[dt][1], lo[dt][2], lo[dt][3], hi[dt][0], hi[dt][1], hi[dt][2], hi[dt][3]};
    f[dt] = __builtin_bit_cast(bf16x8, v);
  }
}

// -inf for the keys >= N of the 16-key tile that starts at key0 (lane holds keys key0 + 4g + r), else 0
__device__ __forceinline__ f32x4 key_mask(int key0, int g, int N) {
  f32x4 v;
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = (key0 + 4 * g + r < N) ? 0.f : -INFINITY;
  return v;
}

__device__ __forceinline__ float max4(const f32x4& a) { return fmaxf(fmaxf(a[0], a[1]), fmaxf(a[2], a[3])); }

// ------------------------------------------------------------------ forward
// grid = items x ceil(N / 128).  LDS: 2 x (K tile, V tile) = 32 KiB.  S^T[key][q] = K.Q^T puts a query on the lane
// (column lane & 15, replicated over the four lane rows) and its 64 keys of the tile in 16 registers: running maximum, running
// sum and the rescale factor are lane scalars, and the accumulators of S^T are directly the B operand of O^T = V^T.P^T.
// The row sum stays a per-lane partial (each lane row sums its own keys; the rescale factor is common to them) and is
// reduced across the lane rows once, in the epilogue.  Keys >= N of the last tile start at -inf.  Rows >= N of the last
// query tile compute on zeros and are not stored.
__global__ __launch_bounds__(64 * LW, 2) void attn_long_fwd_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out,
                                                                 float* __restrict__ lse, int N, int H, int nqt) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, li = lane & 15;
  const int bid = xcd_remap(blockIdx.x, (int)gridDim.x);
  const int item = bid / nqt, qt = bid - item * nqt;
  const Item it = item_of(qkv, item, N, H);
  const long long stride = 3LL * H * DH;
  const int q0 = qt * WG_ROWS + wave * 32;
  const int nkt = (N + ST_ROWS - 1) / ST_ROWS;
  unsigned rel[4];
  tr_lane_offsets(rel, lane);

  bf16x8 qf[2][2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) qf[t][kk] = glb_frag(it.q, stride, q0 + t * 16 + li, kk, N, lane);
  dma_stream_tile(smem, it.k, stride, 0, N, wave, lane);
  dma_stream_tile(smem + ST_BYTES, it.v, stride, 0, N, wave, lane);

  float m_run[2] = {-INFINITY, -INFINITY}, l_run[2] = {0.f, 0.f};
  f32x4 o[2][4];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[t][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const f32x4 c4 = {SCALE_LOG2E, SCALE_LOG2E, SCALE_LOG2E, SCALE_LOG2E};

#pragma unroll 1
  for (int j = 0; j < nkt; ++j) {
    const char* Kt = smem + (j & 1) * 2 * ST_BYTES;
    const char* Vt = Kt + ST_BYTES;
    stream_sync();
    if (j + 1 < nkt) {
      char* Kn = smem + ((j + 1) & 1) * 2 * ST_BYTES;
      dma_stream_tile(Kn, it.k, stride, (j + 1) * ST_ROWS, N, wave, lane);
      dma_stream_tile(Kn + ST_BYTES, it.v, stride, (j + 1) * ST_ROWS, N, wave, lane);
    }
    const bool last = j + 1 == nkt;       // the only tile that can hold keys >= N
    f32x4 s[2][4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      const bf16x8 k0 = lds_frag(Kt, kt * 16 + li, 0, lane);
      const bf16x8 k1 = lds_frag(Kt, kt * 16 + li, 1, lane);
      const f32x4 init = last ? key_mask(j * ST_ROWS + kt * 16, g, N) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < 2; ++t) s[t][kt] = MFMA16(k0, qf[t][0], init);
#pragma unroll
      for (int t = 0; t < 2; ++t) s[t][kt] = MFMA16(k1, qf[t][1], s[t][kt]);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      float mx = fmaxf(fmaxf(max4(s[t][0]), max4(s[t][1])), fmaxf(max4(s[t][2]), max4(s[t][3])));
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m_run[t], mx);           // finite: every tile holds at least one key < N
      const float alpha = __builtin_amdgcn_exp2f((m_run[t] - m_new) * SCALE_LOG2E);   // 0 on the first tile (m_run = -inf)
      m_run[t] = m_new;
      const float mc = -m_new * SCALE_LOG2E;
      const f32x4 m4 = {mc, mc, mc, mc};
      f32x4 part = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        const f32x4 e = __builtin_elementwise_fma(s[t][kt], c4, m4);
#pragma unroll
        for (int r = 0; r < 4; ++r) s[t][kt][r] = __builtin_amdgcn_exp2f(e[r]);
        part += s[t][kt];
      }
      l_run[t] = l_run[t] * alpha + ((part[0] + part[1]) + (part[2] + part[3]));
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) o[t][dt] *= alpha;
    }
    const unsigned vbase = (unsigned)(size_t)LDS_PTR(Vt);
    static_for<2>([&](auto st_c) {
      constexpr int st = decltype(st_c)::value;
      bf16x8 pf[2], vf[4];
#pragma unroll
      for (int t = 0; t < 2; ++t) pf[t] = pack_frag(s[t][2 * st], s[t][2 * st + 1]);
      tr_frags<st>(vf, vbase, rel);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int t = 0; t < 2; ++t) o[t][dt] = MFMA16(vf[dt], pf[t], o[t][dt]);
    });
  }

#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int q = q0 + t * 16 + li;
    float sum = l_run[t];
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.0f / sum;
    if (g == 0 && q < N) lse[it.lse0 + q] = m_run[t] * SCALE + __logf(sum);
    bf16_t* og = out + (it.row0 + q) * ((long long)H * DH) + (item - (item / H) * H) * DH;
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) store_row_pair16_if(q < N, og, pr, g, pack4(o[t][2 * pr] * inv), pack4(o[t][2 * pr + 1] * inv));
  }
}

// ------------------------------------------------------------------ probs (return_attn)
// grid = items x ceil(N / 128); K tiles stream (2 x 8 KiB).  S[q][key] = Q.K^T: the key sits on the lane, so one store
// instruction covers 16 consecutive keys (64 bytes) of four query rows.  probs = exp(S / 8 - lse) with the lse the forward wrote.
__global__ __launch_bounds__(64 * LW, 2) void attn_long_probs_kernel(const bf16_t* __restrict__ qkv, const float* __restrict__ lse,
                                                                   float* __restrict__ probs, int N, int H, int nqt) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, li = lane & 15;
  const int bid = xcd_remap(blockIdx.x, (int)gridDim.x);
  const int item = bid / nqt, qt = bid - item * nqt;
  const Item it = item_of(qkv, item, N, H);
  const long long stride = 3LL * H * DH;
  const int q0 = qt * WG_ROWS + wave * 32;
  const int nkt = (N + ST_ROWS - 1) / ST_ROWS;

  bf16x8 qf[2][2];
  f32x4 nl[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) qf[t][kk] = glb_frag(it.q, stride, q0 + t * 16 + li, kk, N, lane);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q = q0 + t * 16 + 4 * g + r;
      nl[t][r] = q < N ? -lse[it.lse0 + q] * LOG2E : 0.f;
    }
  }
  dma_stream_tile(smem, it.k, stride, 0, N, wave, lane);
  const f32x4 c4 = {SCALE_LOG2E, SCALE_LOG2E, SCALE_LOG2E, SCALE_LOG2E};
#pragma unroll 1
  for (int j = 0; j < nkt; ++j) {
    const char* Kt = smem + (j & 1) * ST_BYTES;
    stream_sync();
    if (j + 1 < nkt) dma_stream_tile(smem + ((j + 1) & 1) * ST_BYTES, it.k, stride, (j + 1) * ST_ROWS, N, wave, lane);
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      const bf16x8 k0 = lds_frag(Kt, kt * 16 + li, 0, lane);
      const bf16x8 k1 = lds_frag(Kt, kt * 16 + li, 1, lane);
      const int key = j * ST_ROWS + kt * 16 + li;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
        a = MFMA16(qf[t][0], k0, a);
        a = MFMA16(qf[t][1], k1, a);
        const f32x4 e = __builtin_elementwise_fma(a, c4, nl[t]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int q = q0 + t * 16 + 4 * g + r;
          if (q < N && key < N) probs[(it.lse0 + q) * N + key] = __builtin_amdgcn_exp2f(e[r]);
        }
      }
    }
  }
}

// ------------------------------------------------------------------ backward: delta = rowsum(dO * O)
// eight lanes per (token, head) row of 64 values; delta f32 [B, H, N]
__global__ __launch_bounds__(256) void attn_long_delta_kernel(const bf16_t* __restrict__ outp, const bf16_t* __restrict__ dout,
                                                             float* __restrict__ delta, long long rows, int N, int H) {
  const long long row = ((long long)blockIdx.x * 256 + threadIdx.x) >> 3;   // = token * H + head
  const int c = threadIdx.x & 7;
  float part = 0.f;
  if (row < rows) {
    const u32x4 ov = *(const u32x4*)(outp + row * DH + c * 8);
    const u32x4 dv = *(const u32x4*)(dout + row * DH + c * 8);
#pragma unroll
    for (int w = 0; w < 4; ++w) part += bf_lo(ov[w]) * bf_lo(dv[w]) + bf_hi(ov[w]) * bf_hi(dv[w]);
  }
  part += __shfl_xor(part, 1, 64);
  part += __shfl_xor(part, 2, 64);
  part += __shfl_xor(part, 4, 64);
  if (c == 0 && row < rows) {
    const long long tok = row / H;
    const int h = (int)(row - tok * H);
    const long long b = tok / N;
    const int n = (int)(tok - b * N);
    delta[(b * H + h) * N + n] = part;
  }
}

// ------------------------------------------------------------------ backward: dK / dV
// grid = items x ceil(N / 128).  Wave w owns keys 32 w .. + 31 of the workgroup's 128: their K / V row fragments stay in
// registers, the accumulators are dK^T / dV^T [d][key].  Q and dO stream in 64-query tiles together with the tile's 64
// lse and delta values (LDS: 2 x (Q tile, dO tile) + 2 x 2 x 64 floats = 33 KiB).  Per 32 queries, as in the fused
// backward: S = Q.K^T and dP = dO.V^T (key on the lane, queries in registers), P = exp(S / 8 - lse),
// dS = P (dP - delta) / 8, dV^T += dO^T.P, dK^T += Q^T.dS.  Queries >= N arrive as zero rows of Q and dO (with lse =
// delta = 0: P = 1, dS = 0) and add nothing; keys >= N start S at -inf (P = dS = 0) and are not stored.
__global__ __launch_bounds__(64 * LW, 2) void attn_long_dkv_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dout,
                                                                 const float* __restrict__ lse, const float* __restrict__ delta,
                                                                 bf16_t* __restrict__ dqkv, int N, int H, int nkt_wg) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* scal = (float*)(smem + 4 * ST_BYTES);       // [buffer][lse | delta][64]
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, li = lane & 15;
  const int bid = xcd_remap(blockIdx.x, (int)gridDim.x);
  const int item = bid / nkt_wg, ktile = bid - item * nkt_wg;
  const int h = item - (item / H) * H;
  const Item it = item_of(qkv, item, N, H);
  const long long stride = 3LL * H * DH, ostride = (long long)H * DH;
  const bf16_t* dog = dout + it.row0 * ostride + h * DH;
  const int key0 = ktile * WG_ROWS + wave * 32;
  const int nqt = (N + ST_ROWS - 1) / ST_ROWS;
  unsigned rel[4];
  tr_lane_offsets(rel, lane);

  auto issue = [&](int j) {
    char* Qn = smem + (j & 1) * 2 * ST_BYTES;
    dma_stream_tile(Qn, it.q, stride, j * ST_ROWS, N, wave, lane);
    dma_stream_tile(Qn + ST_BYTES, dog, ostride, j * ST_ROWS, N, wave, lane);
    if (wave == 0) dma_row_scalars(scal + (j & 1) * 128, lse + it.lse0, j * ST_ROWS, N, lane);
    if (wave == 1) dma_row_scalars(scal + (j & 1) * 128 + 64, delta + it.lse0, j * ST_ROWS, N, lane);
  };

  bf16x8 kf[2][2], vf[2][2];
  f32x4 kinit[2];
#pragma unroll
  for (int kt = 0; kt < 2; ++kt) {
    const int key = key0 + kt * 16 + li;
    const float mi = key < N ? 0.f : -INFINITY;
    kinit[kt] = f32x4{mi, mi, mi, mi};
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      kf[kt][kk] = glb_frag(it.k, stride, key, kk, N, lane);
      vf[kt][kk] = glb_frag(it.v, stride, key, kk, N, lane);
    }
  }
  issue(0);

  f32x4 dv[4][2], dk[4][2];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      dv[dt][kt] = f32x4{0.f, 0.f, 0.f, 0.f};
      dk[dt][kt] = dv[dt][kt];
    }
  const f32x4 c4 = {SCALE_LOG2E, SCALE_LOG2E, SCALE_LOG2E, SCALE_LOG2E}, sc4 = {SCALE, SCALE, SCALE, SCALE};
  const f32x4 nl2e = {-LOG2E, -LOG2E, -LOG2E, -LOG2E}, nsc4 = {-SCALE, -SCALE, -SCALE, -SCALE};

#pragma unroll 1
  for (int j = 0; j < nqt; ++j) {
    const char* Qt = smem + (j & 1) * 2 * ST_BYTES;
    const char* Dt = Qt + ST_BYTES;
    const float* lse_s = scal + (j & 1) * 128;
    const float* del_s = lse_s + 64;
    stream_sync();
    if (j + 1 < nqt) issue(j + 1);
    const unsigned qbase = (unsigned)(size_t)LDS_PTR(Qt), dbase = (unsigned)(size_t)LDS_PTR(Dt);
    static_for<2>([&](auto qs_c) {
      constexpr int qs = decltype(qs_c)::value;
      f32x4 p[2][2], ds[2][2];   // [query tile in step][key tile]
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int qrow = qs * 32 + t * 16 + li;
        const bf16x8 qa0 = lds_frag(Qt, qrow, 0, lane), qa1 = lds_frag(Qt, qrow, 1, lane);
        const bf16x8 da0 = lds_frag(Dt, qrow, 0, lane), da1 = lds_frag(Dt, qrow, 1, lane);
        const f32x4 nl = *(const f32x4*)(lse_s + qs * 32 + t * 16 + 4 * g) * nl2e;
        const f32x4 nd = *(const f32x4*)(del_s + qs * 32 + t * 16 + 4 * g) * nsc4;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
          f32x4 a = kinit[kt], c = {0.f, 0.f, 0.f, 0.f};
          a = MFMA16(qa0, kf[kt][0], a);
          a = MFMA16(qa1, kf[kt][1], a);
          c = MFMA16(da0, vf[kt][0], c);
          c = MFMA16(da1, vf[kt][1], c);
          const f32x4 e = __builtin_elementwise_fma(a, c4, nl);
#pragma unroll
          for (int r = 0; r < 4; ++r) p[t][kt][r] = __builtin_amdgcn_exp2f(e[r]);
          ds[t][kt] = p[t][kt] * __builtin_elementwise_fma(c, sc4, nd);
        }
      }
      bf16x8 dof[4], qtf[4];
      tr_frags<qs>(dof, dbase, rel);
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        const bf16x8 pf = pack_frag(p[0][kt], p[1][kt]);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) dv[dt][kt] = MFMA16(dof[dt], pf, dv[dt][kt]);
      }
      tr_frags<qs>(qtf, qbase, rel);
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        const bf16x8 sf = pack_frag(ds[0][kt], ds[1][kt]);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) dk[dt][kt] = MFMA16(qtf[dt], sf, dk[dt][kt]);
      }
    });
  }

#pragma unroll
  for (int kt = 0; kt < 2; ++kt) {
    const int key = key0 + kt * 16 + li;
    bf16_t* dkg = dqkv + (it.row0 + key) * stride + (long long)H * DH + h * DH;
    bf16_t* dvg = dkg + (long long)H * DH;
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) store_row_pair16_if(key < N, dkg, pr, g, pack4(dk[2 * pr][kt]), pack4(dk[2 * pr + 1][kt]));
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) store_row_pair16_if(key < N, dvg, pr, g, pack4(dv[2 * pr][kt]), pack4(dv[2 * pr + 1][kt]));
  }
}

// ------------------------------------------------------------------ backward: dQ
// grid = items x ceil(N / 128); the forward's structure (K / V tiles stream, the query on the lane) with the Q and dO
// fragments, lse and delta of the wave's 32 queries in registers: S^T = K.Q^T, dP^T = V.dO^T, dS^T = P^T (dP^T - delta) / 8,
// dQ^T[d][q] += K^T.dS^T.
__global__ __launch_bounds__(64 * LW, 2) void attn_long_dq_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dout,
                                                                const float* __restrict__ lse, const float* __restrict__ delta,
                                                                bf16_t* __restrict__ dqkv, int N, int H, int nqt) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, li = lane & 15;
  const int bid = xcd_remap(blockIdx.x, (int)gridDim.x);
  const int item = bid / nqt, qt = bid - item * nqt;
  const int h = item - (item / H) * H;
  const Item it = item_of(qkv, item, N, H);
  const long long stride = 3LL * H * DH, ostride = (long long)H * DH;
  const bf16_t* dog = dout + it.row0 * ostride + h * DH;
  const int q0 = qt * WG_ROWS + wave * 32;
  const int nkt = (N + ST_ROWS - 1) / ST_ROWS;
  unsigned rel[4];
  tr_lane_offsets(rel, lane);

  bf16x8 qf[2][2], dof[2][2];
  float nl[2], nd[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int q = q0 + t * 16 + li;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      qf[t][kk] = glb_frag(it.q, stride, q, kk, N, lane);
      dof[t][kk] = glb_frag(dog, ostride, q, kk, N, lane);
    }
    nl[t] = q < N ? -lse[it.lse0 + q] * LOG2E : 0.f;
    nd[t] = q < N ? -delta[it.lse0 + q] * SCALE : 0.f;
  }
  dma_stream_tile(smem, it.k, stride, 0, N, wave, lane);
  dma_stream_tile(smem + ST_BYTES, it.v, stride, 0, N, wave, lane);

  f32x4 dq[2][4];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dq[t][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const f32x4 c4 = {SCALE_LOG2E, SCALE_LOG2E, SCALE_LOG2E, SCALE_LOG2E}, sc4 = {SCALE, SCALE, SCALE, SCALE};

#pragma unroll 1
  for (int j = 0; j < nkt; ++j) {
    const char* Kt = smem + (j & 1) * 2 * ST_BYTES;
    const char* Vt = Kt + ST_BYTES;
    stream_sync();
    if (j + 1 < nkt) {
      char* Kn = smem + ((j + 1) & 1) * 2 * ST_BYTES;
      dma_stream_tile(Kn, it.k, stride, (j + 1) * ST_ROWS, N, wave, lane);
      dma_stream_tile(Kn + ST_BYTES, it.v, stride, (j + 1) * ST_ROWS, N, wave, lane);
    }
    const bool last = j + 1 == nkt;
    f32x4 ds[2][4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      const bf16x8 k0 = lds_frag(Kt, kt * 16 + li, 0, lane), k1 = lds_frag(Kt, kt * 16 + li, 1, lane);
      const bf16x8 v0 = lds_frag(Vt, kt * 16 + li, 0, lane), v1 = lds_frag(Vt, kt * 16 + li, 1, lane);
      const f32x4 init = last ? key_mask(j * ST_ROWS + kt * 16, g, N) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        f32x4 a = init, c = {0.f, 0.f, 0.f, 0.f};
        a = MFMA16(k0, qf[t][0], a);
        a = MFMA16(k1, qf[t][1], a);
        c = MFMA16(v0, dof[t][0], c);
        c = MFMA16(v1, dof[t][1], c);
        const f32x4 l4 = {nl[t], nl[t], nl[t], nl[t]}, d4 = {nd[t], nd[t], nd[t], nd[t]};
        const f32x4 e = __builtin_elementwise_fma(a, c4, l4);
        f32x4 p;
#pragma unroll
        for (int r = 0; r < 4; ++r) p[r] = __builtin_amdgcn_exp2f(e[r]);
        ds[t][kt] = p * __builtin_elementwise_fma(c, sc4, d4);
      }
    }
    const unsigned kbase = (unsigned)(size_t)LDS_PTR(Kt);
    static_for<2>([&](auto st_c) {
      constexpr int st = decltype(st_c)::value;
      bf16x8 sf[2], ktf[4];
#pragma unroll
      for (int t = 0; t < 2; ++t) sf[t] = pack_frag(ds[t][2 * st], ds[t][2 * st + 1]);
      tr_frags<st>(ktf, kbase, rel);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int t = 0; t < 2; ++t) dq[t][dt] = MFMA16(ktf[dt], sf[t], dq[t][dt]);
    });
  }

#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int q = q0 + t * 16 + li;
    bf16_t* dqg = dqkv + (it.row0 + q) * stride + h * DH;
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) store_row_pair16_if(q < N, dqg, pr, g, pack4(dq[t][2 * pr]), pack4(dq[t][2 * pr + 1]));
  }
}

constexpr int LDS_FWD = 4 * ST_BYTES;
constexpr int LDS_PROBS = 2 * ST_BYTES;
constexpr int LDS_DKV = 4 * ST_BYTES + 2 * 2 * 64 * 4;
static_assert(LDS_DKV <= 48 * 1024, "within the default dynamic-LDS limit");

}  // namespace

namespace vitssl_attn {

int attn_long_fwd(const bf16_t* qkv, bf16_t* out, float* lse, float* probs, int B, int N, int H, hipStream_t s, int* grid) {
  const int nqt = (N + WG_ROWS - 1) / WG_ROWS;
  const int wgs = B * H * nqt;
  hipLaunchKernelGGL(attn_long_fwd_kernel, dim3(wgs), dim3(64 * LW), LDS_FWD, s, qkv, out, lse, N, H, nqt);
  VS_CHECK_LAUNCH("attn_long_fwd");
  if (probs) {
    hipLaunchKernelGGL(attn_long_probs_kernel, dim3(wgs), dim3(64 * LW), LDS_PROBS, s, qkv, (const float*)lse, probs, N, H, nqt);
    VS_CHECK_LAUNCH("attn_long_probs");
  }
  if (grid) *grid = wgs;
  return VITSSL_OK;
}

int attn_long_bwd(const bf16_t* qkv, const bf16_t* out, const bf16_t* dout, const float* lse, bf16_t* dqkv, float* delta_ws,
                  int B, int N, int H, hipStream_t s) {
  const int nt = (N + WG_ROWS - 1) / WG_ROWS;
  const int wgs = B * H * nt;
  const long long rows = (long long)B * N * H;
  hipLaunchKernelGGL(attn_long_delta_kernel, dim3((unsigned)((rows * 8 + 255) / 256)), dim3(256), 0, s, out, dout, delta_ws, rows, N, H);
  VS_CHECK_LAUNCH("attn_long_delta");
  hipLaunchKernelGGL(attn_long_dkv_kernel, dim3(wgs), dim3(64 * LW), LDS_DKV, s, qkv, dout, lse, (const float*)delta_ws, dqkv, N, H, nt);
  VS_CHECK_LAUNCH("attn_long_dkv");
  hipLaunchKernelGGL(attn_long_dq_kernel, dim3(wgs), dim3(64 * LW), LDS_FWD, s, qkv, dout, lse, (const float*)delta_ws, dqkv, N, H, nt);
  VS_CHECK_LAUNCH("attn_long_dq");
  return VITSSL_OK;
}

}  // namespace vitssl_attn
