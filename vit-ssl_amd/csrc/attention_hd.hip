// Streaming multi-head self-attention (bf16 operands), gfx950: the one implementation behind two entry points.
//   * head dims 8 .. 128 (dh % 8 == 0), 1 .. 2048 tokens: vitssl_attn_hd_fwd / _bwd, C ABI in include/vitssl_attention_hd.h;
//   * dh = 64 at 257 .. 2048 tokens: attn_long_fwd / _bwd (attention_tiles.h), reached from vitssl_attn_fwd / _bwd.  Below
//     that, attention.hip keeps all keys and values of an (image, head) item in LDS, which ends at 256 tokens.
//
// A workgroup of four waves owns 128 rows of one (image, head) item and the other side of the product streams through LDS in
// 64-row tiles, two buffers, the next tile arriving by LDS-DMA while the current one is multiplied.  A wave owns 32 of the
// rows as two 16-row MFMA tiles, so that every fragment read from LDS feeds two MFMAs.  Forward (online softmax in fp32: running
// maximum and running sum, the output accumulators rescaled whenever the maximum moves), a separate probs kernel (`out`
// cannot depend on the probs pointer), and a backward of three launches without atomics, every output element written once
// by one workgroup in a fixed order: delta = rowsum(dO * O) into the caller's workspace, dK / dV sweeping Q / dO tiles, dQ
// sweeping K / V tiles.  Both recompute P = exp(S - lse): 7 matrix products of N^2 x dh instead of the fused backward's 5.
// Workgroups are numbered item-major and remapped so that one XCD gets a contiguous run: the tiles of an item, and the heads
// of an image, re-read their streamed operands from one L2.
//
// The kernels are templated on DP, the head dim padded to a whole number of v_mfma_f32_16x16x32_bf16 contraction steps: 32,
// 64, 96 or 128 columns, i.e. DP / 8 16-byte chunks per tile row, and on DHC: 0 takes dh and the scale from the launch (the hd
// entry points, dh = 64 included), 64 makes them constants (the <64, 64> instantiations behind attn_long_*).  They read qkv in
// place: a head's slice of a row is dh / 8 chunks, and only those are fetched.
//   * LDS tiles: the chunks >= dh / 8 of every row are zeroed ONCE, before the first tile is requested, and the LDS-DMA
//     lanes that would land on them are switched off, so they stay zero for every tile of the sweep.  (A lane's LDS
//     destination is fixed by its lane number, its source is free: the lane computes which logical chunk its slot holds and
//     fetches that chunk, or nothing.)
//   * register fragments read straight from global memory take zeros for those chunks, stores skip them.
// The scale 1 / sqrt(dh) multiplies the fp32 score accumulators inside the exp2 argument.  Rounding points: bf16 P into P.V,
// delta from the stored bf16 O, bf16 dS.  At dh = 64 the two instantiations give the same bits.
#include "common.h"
#include "attention_tiles.h"
#include "../../include/vitssl_attention_hd.h"

namespace {

using namespace vitssl_attn;   // fragment packing, row stores, MFMA16, LOG2E (nothing of the 64-wide tile image is used)

constexpr int LW = 4;                 // waves per workgroup
constexpr int WG_ROWS = 32 * LW;      // rows of the stationary tile (queries; keys in the dK / dV kernel)
constexpr int ST_ROWS = 64;           // rows of a streamed tile
constexpr int HD_MAX_N = ATTN_LONG_MAX_N;

// Tile image of width DP: row pitch DP * 2 bytes, the 16-byte chunk index xor-ed with a function of the row so that the 16 lanes
// a ds_read_b128 serves together, and the 32 lanes of a transposed read, fall on distinct slots of the 256-byte bank row:
//   pitch  64 B (DP 32) and 192 B (DP 96): four rows already tile the bank row; rows 4 .. 7 of eight move by two chunks;
//   pitch 128 B (DP 64): the image of attention_tiles.h;
//   pitch 256 B (DP 128): every row starts on bank 0; eight consecutive rows move by 0, 2, .. 14 chunks.
// The xor never leaves the row (DP 96: it touches bit 1 of the chunk only, 12 chunks = 3 groups of 4) and ignores row bits
// >= 3, so that + 16 and + 32 rows are immediates of the transposed reads.
template <int DP>
struct TL {
  static_assert(DP == 32 || DP == 64 || DP == 96 || DP == 128, "padded head dims");
  static constexpr int CH = DP / 8;      // 16-byte chunks per row
  static constexpr int ROWB = DP * 2;    // bytes per row
  static constexpr int KK = DP / 32;     // contraction steps over the head dim
  static constexpr int DT = DP / 16;     // 16-column slices of an output row
  static constexpr int SH = DP == 64 ? 1 : (DP == 128 ? 0 : 2);
  static constexpr int MASK = DP == 64 ? 3 : (DP == 128 ? 7 : 1);
  static constexpr int ST_BYTES = ST_ROWS * ROWB;
  static __device__ __forceinline__ int swz(int row) { return ((row >> SH) & MASK) << 1; }
  static __device__ __forceinline__ int off(int row, int ch) { return row * ROWB + ((ch ^ swz(row)) << 4); }
};

struct Item {
  const bf16_t *q, *k, *v;
  long long row0;     // first token row of the image, in rows of [B*N]
  long long lse0;     // item * N
  int h;
};
__device__ __forceinline__ Item item_of(const bf16_t* qkv, int item, int N, int H, int dh) {
  const int b = item / H, h = item - b * H;
  Item it;
  it.row0 = (long long)b * N;
  it.q = qkv + it.row0 * (3LL * H * dh) + h * dh;
  it.k = it.q + (long long)H * dh;
  it.v = it.k + (long long)H * dh;
  it.lse0 = (long long)item * N;
  it.h = h;
  return it;
}

// The head dim as a kernel sees it.  DHC == 0: dh and scale = 1 / sqrt(dh) are the launch's arguments.  DHC == 64: they are the
// constants 64 and 1 / 8 whatever was passed, so chr = dh / 8 = TL<64>::CH, every test against it folds (no pad chunks, no
// zeroing, no switched-off DMA lanes) and no register holds either.
template <int DHC>
__device__ __forceinline__ void fix_head_dim(int& dh) {
  static_assert(DHC == 0 || DHC == 64, "run-time head dim, or dh = 64");
  if constexpr (DHC == 64) dh = 64;
}
template <int DHC>
__device__ __forceinline__ void fix_head_dim(int& dh, float& scale) {
  fix_head_dim<DHC>(dh);
  if constexpr (DHC == 64) scale = 0.125f;
}

// rows [row0, row0 + 64) of X[n][0 .. 8 chr) (n < N) into a streamed-tile buffer: CH wave instructions of 64 chunks each.  Slot
// `idx` of the tile holds chunk pc ^ swz(row) of row idx / CH; lanes whose chunk is >= chr fetch nothing (their slot keeps
// the zeros written by zero_tiles), rows >= N fall outside the buffer descriptor and are zero-filled by the hardware.
template <int DP>
__device__ __forceinline__ void dma_stream_tile(char* lds, const bf16_t* g, long long stride, int row0, int N, int chr, int wave, int lane) {
  using T = TL<DP>;
  const bf16_t* base = g + (long long)row0 * stride;
  const unsigned bytes = (unsigned)((long long)(N - row0 - 1) * stride * 2 + chr * 16);
  __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, (int)bytes, 0x00020000);
  for (int i = wave; i < T::CH; i += LW) {
    const int idx = i * 64 + lane;
    const int row = idx / T::CH, pc = idx - row * T::CH;
    const int c = pc ^ T::swz(row);
    const unsigned voff = (unsigned)((long long)row * stride * 2 + c * 16);
    if (c < chr) dma16_to_lds(rs, lds + i * 1024, voff);
  }
}
// the pad chunks of every tile buffer are zeroed once per workgroup (the whole tile area is: simpler, and as cheap)
__device__ __forceinline__ void zero_tiles(char* smem, int bytes, int tid) {
  const u32x4 z = {0u, 0u, 0u, 0u};
  for (int o = tid * 16; o < bytes; o += 64 * LW * 16) *(u32x4*)(smem + o) = z;
  __syncthreads();
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

// natural fragment (8 consecutive d) of row `row`, contraction step kk, from an LDS tile
template <int DP>
__device__ __forceinline__ bf16x8 lds_frag(const char* tile, int row, int kk, int lane) {
  return *(const bf16x8*)(tile + TL<DP>::off(row, 4 * kk + (lane >> 4)));
}
// natural fragment straight from global: zero past N and in the pad chunks
__device__ __forceinline__ bf16x8 glb_frag(const bf16_t* g, long long stride, int row, int kk, int N, int chr, int lane) {
  u32x4 v = {0u, 0u, 0u, 0u};
  const int ch = 4 * kk + (lane >> 4);
  if (row < N && ch < chr) v = *(const u32x4*)(g + (long long)row * stride + 8 * ch);
  return __builtin_bit_cast(bf16x8, v);
}
// tile-relative byte address of this lane's transposed reads (row 4g + q of a 32-row step, column slice dt)
template <int DP>
__device__ __forceinline__ void tr_lane_offsets(unsigned (&rel)[TL<DP>::DT], int lane) {
  const int g = lane >> 4, tq = (lane >> 2) & 3, tpp = lane & 3;
#pragma unroll
  for (int dt = 0; dt < TL<DP>::DT; ++dt) rel[dt] = (unsigned)(TL<DP>::off(4 * g + tq, 2 * dt + (tpp >> 1)) + 8 * (tpp & 1));
}
// the DT transposed fragments of contraction step ST (rows 32 ST .. + 31) of the tile at LDS address `base`.  Inline asm reads
// (common.h, ds_read_tr16): the builtin would drain the next tile's LDS-DMA in front of every read.
template <int DP, int ST>
__device__ __forceinline__ void tr_frags(bf16x8 (&f)[TL<DP>::DT], unsigned base, const unsigned (&rel)[TL<DP>::DT]) {
  constexpr int DT = TL<DP>::DT, STEP = 32 * TL<DP>::ROWB;
  s16x4 lo[DT], hi[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) {
    ds_read_tr16<STEP * ST>(lo[dt], base + rel[dt]);
    ds_read_tr16<STEP * ST + STEP / 2>(hi[dt], base + rel[dt]);
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  typedef __attribute__((ext_vector_type(8))) short s16x8;
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) {
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
__device__ __forceinline__ f32x4 splat(float x) { return f32x4{x, x, x, x}; }

// column slices (2 pr, 2 pr + 1) of one output row: the 16-byte store of attention_tiles.h, skipped where its eight columns
// are pad (they start at a multiple of 8, so they are pad together).  Every lane takes part in the exchange.
__device__ __forceinline__ void store_pair_hd(bool row_ok, bf16_t* row, int pr, int g, int dh, const f32x4& a, const f32x4& b) {
  const int odd = g & 1;
  const int col = (2 * pr + odd) * 16 + 4 * (g - odd);
  store_row_pair16_if(row_ok && col < dh, row, pr, g, pack4(a), pack4(b));
}

// ------------------------------------------------------------------ forward
// grid = items x ceil(N / 128).  LDS: 2 x (K tile, V tile).  S^T[key][q] = K.Q^T puts a query on the lane and its 64 keys of the
// tile in 16 registers: running maximum, running sum and the rescale factor are lane scalars, and the accumulators of S^T are
// directly the B operand of O^T = V^T.P^T.  Keys >= N of the last tile start at -inf.  Rows >= N of the last query tile
// compute on zeros and are not stored.
template <int DP, int DHC, int MINW>
__global__ __launch_bounds__(64 * LW, MINW) void attn_hd_fwd_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out,
                                                                  float* __restrict__ lse, int N, int H, int dh, int nqt, float scale) {
  using T = TL<DP>;
  constexpr int KK = T::KK, DT = T::DT, STB = T::ST_BYTES;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  fix_head_dim<DHC>(dh, scale);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, li = lane & 15;
  const int bid = xcd_remap(blockIdx.x, (int)gridDim.x);
  const int item = bid / nqt, qt = bid - item * nqt;
  const Item it = item_of(qkv, item, N, H, dh);
  const long long stride = 3LL * H * dh;
  const int chr = dh >> 3;
  const int q0 = qt * WG_ROWS + wave * 32;
  const int nkt = (N + ST_ROWS - 1) / ST_ROWS;
  const float scale_l2 = scale * LOG2E;
  unsigned rel[DT];
  tr_lane_offsets<DP>(rel, lane);

  bf16x8 qf[2][KK];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) qf[t][kk] = glb_frag(it.q, stride, q0 + t * 16 + li, kk, N, chr, lane);
  if (chr < T::CH) zero_tiles(smem, 4 * STB, threadIdx.x);
  dma_stream_tile<DP>(smem, it.k, stride, 0, N, chr, wave, lane);
  dma_stream_tile<DP>(smem + STB, it.v, stride, 0, N, chr, wave, lane);

  float m_run[2] = {-INFINITY, -INFINITY}, l_run[2] = {0.f, 0.f};
  f32x4 o[2][DT];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[t][dt] = splat(0.f);
  const f32x4 c4 = splat(scale_l2);

#pragma unroll 1
  for (int j = 0; j < nkt; ++j) {
    const char* Kt = smem + (j & 1) * 2 * STB;
    const char* Vt = Kt + STB;
    stream_sync();
    if (j + 1 < nkt) {
      char* Kn = smem + ((j + 1) & 1) * 2 * STB;
      dma_stream_tile<DP>(Kn, it.k, stride, (j + 1) * ST_ROWS, N, chr, wave, lane);
      dma_stream_tile<DP>(Kn + STB, it.v, stride, (j + 1) * ST_ROWS, N, chr, wave, lane);
    }
    const bool last = j + 1 == nkt;       // the only tile that can hold keys >= N
    f32x4 s[2][4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      const f32x4 init = last ? key_mask(j * ST_ROWS + kt * 16, g, N) : splat(0.f);
#pragma unroll
      for (int t = 0; t < 2; ++t) s[t][kt] = init;
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
        const bf16x8 kf = lds_frag<DP>(Kt, kt * 16 + li, kk, lane);
#pragma unroll
        for (int t = 0; t < 2; ++t) s[t][kt] = MFMA16(kf, qf[t][kk], s[t][kt]);
      }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      float mx = fmaxf(fmaxf(max4(s[t][0]), max4(s[t][1])), fmaxf(max4(s[t][2]), max4(s[t][3])));
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m_run[t], mx);           // finite: every tile holds at least one key < N
      const float alpha = __builtin_amdgcn_exp2f((m_run[t] - m_new) * scale_l2);   // 0 on the first tile (m_run = -inf)
      m_run[t] = m_new;
      const f32x4 m4 = splat(-m_new * scale_l2);
      f32x4 part = splat(0.f);
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        const f32x4 e = __builtin_elementwise_fma(s[t][kt], c4, m4);
#pragma unroll
        for (int r = 0; r < 4; ++r) s[t][kt][r] = __builtin_amdgcn_exp2f(e[r]);
        part += s[t][kt];
      }
      l_run[t] = l_run[t] * alpha + ((part[0] + part[1]) + (part[2] + part[3]));
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) o[t][dt] *= alpha;
    }
    const unsigned vbase = (unsigned)(size_t)LDS_PTR(Vt);
    static_for<2>([&](auto st_c) {
      constexpr int st = decltype(st_c)::value;
      bf16x8 pf[2], vf[DT];
#pragma unroll
      for (int t = 0; t < 2; ++t) pf[t] = pack_frag(s[t][2 * st], s[t][2 * st + 1]);
      tr_frags<DP, st>(vf, vbase, rel);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
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
    if (g == 0 && q < N) lse[it.lse0 + q] = m_run[t] * scale + __logf(sum);
    bf16_t* og = out + (it.row0 + q) * ((long long)H * dh) + it.h * dh;
#pragma unroll
    for (int pr = 0; pr < DT / 2; ++pr) store_pair_hd(q < N, og, pr, g, dh, o[t][2 * pr] * inv, o[t][2 * pr + 1] * inv);
  }
}

// ------------------------------------------------------------------ probs (return_attn)
// grid = items x ceil(N / 128); K tiles stream.  S[q][key] = Q.K^T: the key sits on the lane, so one store instruction covers
// 16 consecutive keys (64 bytes) of four query rows.  probs = exp(S / sqrt(dh) - lse) with the lse the forward wrote.
template <int DP, int DHC>
__global__ __launch_bounds__(64 * LW, 2) void attn_hd_probs_kernel(const bf16_t* __restrict__ qkv, const float* __restrict__ lse,
                                                                 float* __restrict__ probs, int N, int H, int dh, int nqt, float scale) {
  using T = TL<DP>;
  constexpr int KK = T::KK, STB = T::ST_BYTES;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  fix_head_dim<DHC>(dh, scale);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, li = lane & 15;
  const int bid = xcd_remap(blockIdx.x, (int)gridDim.x);
  const int item = bid / nqt, qt = bid - item * nqt;
  const Item it = item_of(qkv, item, N, H, dh);
  const long long stride = 3LL * H * dh;
  const int chr = dh >> 3;
  const int q0 = qt * WG_ROWS + wave * 32;
  const int nkt = (N + ST_ROWS - 1) / ST_ROWS;

  bf16x8 qf[2][KK];
  f32x4 nl[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) qf[t][kk] = glb_frag(it.q, stride, q0 + t * 16 + li, kk, N, chr, lane);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q = q0 + t * 16 + 4 * g + r;
      nl[t][r] = q < N ? -lse[it.lse0 + q] * LOG2E : 0.f;
    }
  }
  if (chr < T::CH) zero_tiles(smem, 2 * STB, threadIdx.x);
  dma_stream_tile<DP>(smem, it.k, stride, 0, N, chr, wave, lane);
  const f32x4 c4 = splat(scale * LOG2E);
#pragma unroll 1
  for (int j = 0; j < nkt; ++j) {
    const char* Kt = smem + (j & 1) * STB;
    stream_sync();
    if (j + 1 < nkt) dma_stream_tile<DP>(smem + ((j + 1) & 1) * STB, it.k, stride, (j + 1) * ST_ROWS, N, chr, wave, lane);
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      bf16x8 kf[KK];
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) kf[kk] = lds_frag<DP>(Kt, kt * 16 + li, kk, lane);
      const int key = j * ST_ROWS + kt * 16 + li;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        f32x4 a = splat(0.f);
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) a = MFMA16(qf[t][kk], kf[kk], a);
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
// eight lanes per (token, head) row of dh values (one or two 16-byte chunks each, exactly one at DHC = 64); delta f32 [B, H, N]
template <int DHC>
__global__ __launch_bounds__(256) void attn_hd_delta_kernel(const bf16_t* __restrict__ outp, const bf16_t* __restrict__ dout,
                                                           float* __restrict__ delta, long long rows, int N, int H, int dh) {
  fix_head_dim<DHC>(dh);
  const long long row = ((long long)blockIdx.x * 256 + threadIdx.x) >> 3;   // = token * H + head
  const int c = threadIdx.x & 7;
  float part = 0.f;
  if (row < rows) {
    for (int ch = c; ch < (dh >> 3); ch += 8) {
      const u32x4 ov = *(const u32x4*)(outp + row * dh + ch * 8);
      const u32x4 dv = *(const u32x4*)(dout + row * dh + ch * 8);
#pragma unroll
      for (int w = 0; w < 4; ++w) part += bf_lo(ov[w]) * bf_lo(dv[w]) + bf_hi(ov[w]) * bf_hi(dv[w]);
    }
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
// lse and delta values.  Per 32 queries: S = Q.K^T and dP = dO.V^T (key on the lane, queries in registers),
// P = exp(S scale - lse), dS = P (dP - delta) scale, dV^T += dO^T.P, dK^T += Q^T.dS.  Queries >= N arrive as zero rows of Q and
// dO (with lse = delta = 0: P = 1, dS = 0) and add nothing; keys >= N start S at -inf (P = dS = 0) and are not stored.
template <int DP, int DHC, int MINW>
__global__ __launch_bounds__(64 * LW, MINW) void attn_hd_dkv_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dout,
                                                                  const float* __restrict__ lse, const float* __restrict__ delta,
                                                                  bf16_t* __restrict__ dqkv, int N, int H, int dh, int nkt_wg, float scale) {
  using T = TL<DP>;
  constexpr int KK = T::KK, DT = T::DT, STB = T::ST_BYTES;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  fix_head_dim<DHC>(dh, scale);
  float* scal = (float*)(smem + 4 * STB);       // [buffer][lse | delta][64]
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, li = lane & 15;
  const int bid = xcd_remap(blockIdx.x, (int)gridDim.x);
  const int item = bid / nkt_wg, ktile = bid - item * nkt_wg;
  const Item it = item_of(qkv, item, N, H, dh);
  const int h = it.h;
  const long long stride = 3LL * H * dh, ostride = (long long)H * dh;
  const int chr = dh >> 3;
  const bf16_t* dog = dout + it.row0 * ostride + h * dh;
  const int key0 = ktile * WG_ROWS + wave * 32;
  const int nqt = (N + ST_ROWS - 1) / ST_ROWS;
  unsigned rel[DT];
  tr_lane_offsets<DP>(rel, lane);

  auto issue = [&](int j) {
    char* Qn = smem + (j & 1) * 2 * STB;
    dma_stream_tile<DP>(Qn, it.q, stride, j * ST_ROWS, N, chr, wave, lane);
    dma_stream_tile<DP>(Qn + STB, dog, ostride, j * ST_ROWS, N, chr, wave, lane);
    if (wave == 0) dma_row_scalars(scal + (j & 1) * 128, lse + it.lse0, j * ST_ROWS, N, lane);
    if (wave == 1) dma_row_scalars(scal + (j & 1) * 128 + 64, delta + it.lse0, j * ST_ROWS, N, lane);
  };

  bf16x8 kf[2][KK], vf[2][KK];
  f32x4 kinit[2];
#pragma unroll
  for (int kt = 0; kt < 2; ++kt) {
    const int key = key0 + kt * 16 + li;
    kinit[kt] = splat(key < N ? 0.f : -INFINITY);
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      kf[kt][kk] = glb_frag(it.k, stride, key, kk, N, chr, lane);
      vf[kt][kk] = glb_frag(it.v, stride, key, kk, N, chr, lane);
    }
  }
  if (chr < T::CH) zero_tiles(smem, 4 * STB, threadIdx.x);
  issue(0);

  f32x4 dv[DT][2], dk[DT][2];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      dv[dt][kt] = splat(0.f);
      dk[dt][kt] = dv[dt][kt];
    }
  const f32x4 c4 = splat(scale * LOG2E), sc4 = splat(scale);
  const f32x4 nl2e = splat(-LOG2E), nsc4 = splat(-scale);

#pragma unroll 1
  for (int j = 0; j < nqt; ++j) {
    const char* Qt = smem + (j & 1) * 2 * STB;
    const char* Dt = Qt + STB;
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
        f32x4 a[2] = {kinit[0], kinit[1]}, c[2] = {splat(0.f), splat(0.f)};
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
          const bf16x8 qa = lds_frag<DP>(Qt, qrow, kk, lane), da = lds_frag<DP>(Dt, qrow, kk, lane);
#pragma unroll
          for (int kt = 0; kt < 2; ++kt) {
            a[kt] = MFMA16(qa, kf[kt][kk], a[kt]);
            c[kt] = MFMA16(da, vf[kt][kk], c[kt]);
          }
        }
        const f32x4 nl = *(const f32x4*)(lse_s + qs * 32 + t * 16 + 4 * g) * nl2e;
        const f32x4 nd = *(const f32x4*)(del_s + qs * 32 + t * 16 + 4 * g) * nsc4;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
          const f32x4 e = __builtin_elementwise_fma(a[kt], c4, nl);
#pragma unroll
          for (int r = 0; r < 4; ++r) p[t][kt][r] = __builtin_amdgcn_exp2f(e[r]);
          ds[t][kt] = p[t][kt] * __builtin_elementwise_fma(c[kt], sc4, nd);
        }
      }
      bf16x8 tf[DT];
      tr_frags<DP, qs>(tf, dbase, rel);
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        const bf16x8 pf = pack_frag(p[0][kt], p[1][kt]);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) dv[dt][kt] = MFMA16(tf[dt], pf, dv[dt][kt]);
      }
      tr_frags<DP, qs>(tf, qbase, rel);
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        const bf16x8 sf = pack_frag(ds[0][kt], ds[1][kt]);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) dk[dt][kt] = MFMA16(tf[dt], sf, dk[dt][kt]);
      }
    });
  }

#pragma unroll
  for (int kt = 0; kt < 2; ++kt) {
    const int key = key0 + kt * 16 + li;
    bf16_t* dkg = dqkv + (it.row0 + key) * stride + (long long)H * dh + h * dh;
    bf16_t* dvg = dkg + (long long)H * dh;
#pragma unroll
    for (int pr = 0; pr < DT / 2; ++pr) store_pair_hd(key < N, dkg, pr, g, dh, dk[2 * pr][kt], dk[2 * pr + 1][kt]);
#pragma unroll
    for (int pr = 0; pr < DT / 2; ++pr) store_pair_hd(key < N, dvg, pr, g, dh, dv[2 * pr][kt], dv[2 * pr + 1][kt]);
  }
}

// ------------------------------------------------------------------ backward: dQ
// grid = items x ceil(N / 128); the forward's structure (K / V tiles stream, the query on the lane) with the Q and dO
// fragments, lse and delta of the wave's 32 queries in registers: S^T = K.Q^T, dP^T = V.dO^T, dS^T = P^T (dP^T - delta) scale,
// dQ^T[d][q] += K^T.dS^T.
template <int DP, int DHC, int MINW>
__global__ __launch_bounds__(64 * LW, MINW) void attn_hd_dq_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dout,
                                                                 const float* __restrict__ lse, const float* __restrict__ delta,
                                                                 bf16_t* __restrict__ dqkv, int N, int H, int dh, int nqt, float scale) {
  using T = TL<DP>;
  constexpr int KK = T::KK, DT = T::DT, STB = T::ST_BYTES;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  fix_head_dim<DHC>(dh, scale);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, li = lane & 15;
  const int bid = xcd_remap(blockIdx.x, (int)gridDim.x);
  const int item = bid / nqt, qt = bid - item * nqt;
  const Item it = item_of(qkv, item, N, H, dh);
  const int h = it.h;
  const long long stride = 3LL * H * dh, ostride = (long long)H * dh;
  const int chr = dh >> 3;
  const bf16_t* dog = dout + it.row0 * ostride + h * dh;
  const int q0 = qt * WG_ROWS + wave * 32;
  const int nkt = (N + ST_ROWS - 1) / ST_ROWS;
  unsigned rel[DT];
  tr_lane_offsets<DP>(rel, lane);

  bf16x8 qf[2][KK], dof[2][KK];
  float nl[2], nd[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int q = q0 + t * 16 + li;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      qf[t][kk] = glb_frag(it.q, stride, q, kk, N, chr, lane);
      dof[t][kk] = glb_frag(dog, ostride, q, kk, N, chr, lane);
    }
    nl[t] = q < N ? -lse[it.lse0 + q] * LOG2E : 0.f;
    nd[t] = q < N ? -delta[it.lse0 + q] * scale : 0.f;
  }
  if (chr < T::CH) zero_tiles(smem, 4 * STB, threadIdx.x);
  dma_stream_tile<DP>(smem, it.k, stride, 0, N, chr, wave, lane);
  dma_stream_tile<DP>(smem + STB, it.v, stride, 0, N, chr, wave, lane);

  f32x4 dq[2][DT];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) dq[t][dt] = splat(0.f);
  const f32x4 c4 = splat(scale * LOG2E), sc4 = splat(scale);

#pragma unroll 1
  for (int j = 0; j < nkt; ++j) {
    const char* Kt = smem + (j & 1) * 2 * STB;
    const char* Vt = Kt + STB;
    stream_sync();
    if (j + 1 < nkt) {
      char* Kn = smem + ((j + 1) & 1) * 2 * STB;
      dma_stream_tile<DP>(Kn, it.k, stride, (j + 1) * ST_ROWS, N, chr, wave, lane);
      dma_stream_tile<DP>(Kn + STB, it.v, stride, (j + 1) * ST_ROWS, N, chr, wave, lane);
    }
    const bool last = j + 1 == nkt;
    f32x4 ds[2][4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      const f32x4 init = last ? key_mask(j * ST_ROWS + kt * 16, g, N) : splat(0.f);
      f32x4 a[2] = {init, init}, c[2] = {splat(0.f), splat(0.f)};
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
        const bf16x8 kfr = lds_frag<DP>(Kt, kt * 16 + li, kk, lane), vfr = lds_frag<DP>(Vt, kt * 16 + li, kk, lane);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          a[t] = MFMA16(kfr, qf[t][kk], a[t]);
          c[t] = MFMA16(vfr, dof[t][kk], c[t]);
        }
      }
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const f32x4 e = __builtin_elementwise_fma(a[t], c4, splat(nl[t]));
        f32x4 p;
#pragma unroll
        for (int r = 0; r < 4; ++r) p[r] = __builtin_amdgcn_exp2f(e[r]);
        ds[t][kt] = p * __builtin_elementwise_fma(c[t], sc4, splat(nd[t]));
      }
    }
    const unsigned kbase = (unsigned)(size_t)LDS_PTR(Kt);
    static_for<2>([&](auto st_c) {
      constexpr int st = decltype(st_c)::value;
      bf16x8 sf[2], ktf[DT];
#pragma unroll
      for (int t = 0; t < 2; ++t) sf[t] = pack_frag(ds[t][2 * st], ds[t][2 * st + 1]);
      tr_frags<DP, st>(ktf, kbase, rel);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int t = 0; t < 2; ++t) dq[t][dt] = MFMA16(ktf[dt], sf[t], dq[t][dt]);
    });
  }

#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int q = q0 + t * 16 + li;
    bf16_t* dqg = dqkv + (it.row0 + q) * stride + h * dh;
#pragma unroll
    for (int pr = 0; pr < DT / 2; ++pr) store_pair_hd(q < N, dqg, pr, g, dh, dq[t][2 * pr], dq[t][2 * pr + 1]);
  }
}

// ------------------------------------------------------------------ launches
// One workgroup per 128-row tile, none of them persistent: nothing here is sized by the CU count, so the CUs reserved for a
// collective library (vitssl_set_reserved_cus) are free again as soon as the tiles that happened to run there retire.
constexpr int HD_LDS_LIMIT = 160 * 1024;
// registers: the dK / dV kernel at DP = 128 keeps 2 x 64 accumulators and 64 operand registers per lane and runs at one wave per
// SIMD; everything else fits two
template <int DP>
constexpr int dkv_minw() { return DP > 96 ? 1 : 2; }

template <int DP, int DHC>
int launch_fwd_hd(const bf16_t* qkv, bf16_t* out, float* lse, float* probs, int B, int N, int H, int dh, float scale, hipStream_t s) {
  constexpr int lds_fwd = 4 * TL<DP>::ST_BYTES, lds_probs = 2 * TL<DP>::ST_BYTES;
  static_assert(lds_probs <= 48 * 1024, "the probs kernel stays within the default dynamic-LDS limit");
  const int nqt = (N + WG_ROWS - 1) / WG_ROWS;
  const int wgs = B * H * nqt;
  if constexpr (lds_fwd > 48 * 1024) {
    static VsOnce done{false};
    if (int rc = ensure_lds(attn_hd_fwd_kernel<DP, DHC, 2>, HD_LDS_LIMIT, done, "attn_hd_fwd")) return rc;
  }
  hipLaunchKernelGGL((attn_hd_fwd_kernel<DP, DHC, 2>), dim3(wgs), dim3(64 * LW), lds_fwd, s, qkv, out, lse, N, H, dh, nqt, scale);
  VS_CHECK_LAUNCH("attn_hd_fwd");
  if (probs) {
    hipLaunchKernelGGL((attn_hd_probs_kernel<DP, DHC>), dim3(wgs), dim3(64 * LW), lds_probs, s, qkv, (const float*)lse, probs, N, H, dh, nqt, scale);
    VS_CHECK_LAUNCH("attn_hd_probs");
  }
  return VITSSL_OK;
}

template <int DP, int DHC>
int launch_bwd_hd(const bf16_t* qkv, const bf16_t* out, const bf16_t* dout, const float* lse, bf16_t* dqkv, float* delta_ws,
                  int B, int N, int H, int dh, float scale, hipStream_t s) {
  constexpr int lds_dq = 4 * TL<DP>::ST_BYTES, lds_dkv = lds_dq + 2 * 2 * 64 * 4;
  constexpr int MW = dkv_minw<DP>();
  const int nt = (N + WG_ROWS - 1) / WG_ROWS;
  const int wgs = B * H * nt;
  const long long rows = (long long)B * N * H;
  if constexpr (lds_dkv > 48 * 1024) {
    static VsOnce done_kv{false};
    if (int rc = ensure_lds(attn_hd_dkv_kernel<DP, DHC, MW>, HD_LDS_LIMIT, done_kv, "attn_hd_dkv")) return rc;
  }
  if constexpr (lds_dq > 48 * 1024) {
    static VsOnce done_q{false};
    if (int rc = ensure_lds(attn_hd_dq_kernel<DP, DHC, 2>, HD_LDS_LIMIT, done_q, "attn_hd_dq")) return rc;
  }
  hipLaunchKernelGGL(attn_hd_delta_kernel<DHC>, dim3((unsigned)((rows * 8 + 255) / 256)), dim3(256), 0, s, out, dout, delta_ws, rows, N, H, dh);
  VS_CHECK_LAUNCH("attn_hd_delta");
  hipLaunchKernelGGL((attn_hd_dkv_kernel<DP, DHC, MW>), dim3(wgs), dim3(64 * LW), lds_dkv, s, qkv, dout, lse, (const float*)delta_ws, dqkv, N, H,
                     dh, nt, scale);
  VS_CHECK_LAUNCH("attn_hd_dkv");
  hipLaunchKernelGGL((attn_hd_dq_kernel<DP, DHC, 2>), dim3(wgs), dim3(64 * LW), lds_dq, s, qkv, dout, lse, (const float*)delta_ws, dqkv, N, H, dh,
                     nt, scale);
  VS_CHECK_LAUNCH("attn_hd_dq");
  return VITSSL_OK;
}

#define VS_DP_SWITCH(DHV, CALL)              \
  switch (((DHV) + 31) / 32) {               \
    case 1: return CALL(32);                 \
    case 2: return CALL(64);                 \
    case 3: return CALL(96);                 \
    default: return CALL(128);               \
  }

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int check_hd_shape(const char* who, int B, int N, int H, int dh) {
  VS_CHECK_ARG(B > 0, "%s: B=%d must be positive", who, B);
  VS_CHECK_ARG(N > 0, "%s: N=%d must be positive", who, N);
  VS_CHECK_ARG(H > 0, "%s: H=%d must be positive", who, H);
  VS_CHECK_ARG(dh >= 8 && dh <= 128 && dh % 8 == 0, "%s: head dim dh=%d unsupported (supported: multiples of 8 from 8 to 128)", who, dh);
  VS_CHECK_ARG(N <= HD_MAX_N, "%s: sequence length N=%d > %d unsupported", who, N, HD_MAX_N);
  // byte offsets inside one image are 32-bit in the buffer descriptors; the workgroup count is an int
  VS_CHECK_ARG(6LL * H * dh * N < (1LL << 31), "%s: H=%d x dh=%d x N=%d: one image's qkv rows exceed 2 GiB", who, H, dh, N);
  VS_CHECK_ARG((long long)B * H * ((N + WG_ROWS - 1) / WG_ROWS) < (1LL << 31) && (long long)B * N * H * 8 < (1LL << 40),
               "%s: B=%d x H=%d x N=%d: too many workgroups for one launch", who, B, H, N);
  return VITSSL_OK;
}

}  // namespace

// dh = 64 at 257 .. ATTN_LONG_MAX_N tokens, for vitssl_attn_fwd / _bwd (attention.hip, which has checked the arguments): the
// DP = 64 kernels with the head dim folded.  32 KiB (forward, dQ), 16 KiB (probs) and 33 KiB (dK / dV) of dynamic LDS.
namespace vitssl_attn {

int attn_long_fwd(const bf16_t* qkv, bf16_t* out, float* lse, float* probs, int B, int N, int H, hipStream_t s, int* grid) {
  if (grid) *grid = B * H * ((N + WG_ROWS - 1) / WG_ROWS);
  return launch_fwd_hd<64, 64>(qkv, out, lse, probs, B, N, H, 64, 0.125f, s);
}

int attn_long_bwd(const bf16_t* qkv, const bf16_t* out, const bf16_t* dout, const float* lse, bf16_t* dqkv, float* delta_ws,
                  int B, int N, int H, hipStream_t s) {
  return launch_bwd_hd<64, 64>(qkv, out, dout, lse, dqkv, delta_ws, B, N, H, 64, 0.125f, s);
}

}  // namespace vitssl_attn

extern "C" int vitssl_attn_hd_fwd(const void* qkv, void* out, float* lse, float* probs, int B, int N, int H, int dh, void* stream) {
  VS_CHECK_ARG(qkv, "attn_hd_fwd: qkv is NULL");
  VS_CHECK_ARG(out, "attn_hd_fwd: out is NULL");
  VS_CHECK_ARG(lse, "attn_hd_fwd: lse is NULL");
  if (int rc = check_hd_shape("attn_hd_fwd", B, N, H, dh)) return rc;
  VS_CHECK_ARG(aligned16(qkv), "attn_hd_fwd: qkv must be 16-byte aligned");
  VS_CHECK_ARG(aligned16(out), "attn_hd_fwd: out must be 16-byte aligned");
  const float scale = 1.0f / sqrtf((float)dh);
#define VS_CALL(DP) launch_fwd_hd<DP, 0>((const bf16_t*)qkv, (bf16_t*)out, lse, probs, B, N, H, dh, scale, (hipStream_t)stream)
  VS_DP_SWITCH(dh, VS_CALL)
#undef VS_CALL
}

extern "C" int vitssl_attn_hd_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, float* delta_ws,
                                  int B, int N, int H, int dh, void* stream) {
  VS_CHECK_ARG(qkv, "attn_hd_bwd: qkv is NULL");
  VS_CHECK_ARG(out, "attn_hd_bwd: out is NULL");
  VS_CHECK_ARG(dout, "attn_hd_bwd: dout is NULL");
  VS_CHECK_ARG(lse, "attn_hd_bwd: lse is NULL");
  VS_CHECK_ARG(dqkv, "attn_hd_bwd: dqkv is NULL");
  VS_CHECK_ARG(delta_ws, "attn_hd_bwd: delta_ws is NULL (the backward keeps delta [B, H, N] there)");
  if (int rc = check_hd_shape("attn_hd_bwd", B, N, H, dh)) return rc;
  VS_CHECK_ARG(aligned16(qkv), "attn_hd_bwd: qkv must be 16-byte aligned");
  VS_CHECK_ARG(aligned16(out), "attn_hd_bwd: out must be 16-byte aligned");
  VS_CHECK_ARG(aligned16(dout), "attn_hd_bwd: dout must be 16-byte aligned");
  VS_CHECK_ARG(aligned16(dqkv), "attn_hd_bwd: dqkv must be 16-byte aligned");
  const float scale = 1.0f / sqrtf((float)dh);
#define VS_CALL(DP)                                                                                                                   \
  launch_bwd_hd<DP, 0>((const bf16_t*)qkv, (const bf16_t*)out, (const bf16_t*)dout, lse, (bf16_t*)dqkv, delta_ws, B, N, H, dh, scale, \
                    (hipStream_t)stream)
  VS_DP_SWITCH(dh, VS_CALL)
#undef VS_CALL
}
