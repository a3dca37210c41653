// bf16 MFMA GEMM  C[M,N] = A[M,K] . B[N,K]^T  with fused epilogues (gfx950).
//
// Tile 256x256x64, 512 threads = 8 waves as 2(M) x 4(N), each wave owns a 128x64
// sub-tile = 8x4 accumulators of v_mfma_f32_16x16x32_bf16.  The MFMA is issued with
// the B-tile fragment as its A operand and the A-tile fragment as its B operand, so a
// lane ends up holding 4 CONSECUTIVE output columns of one output row
// (D[n = 4*(lane>>4)+r][m = lane&15]) -> 8-byte bf16 / 16-byte fp32 row-contiguous
// epilogue accesses with no LDS transpose.
//
// Operand staging is LDS-DMA (buffer_load_dwordx4 ... lds): each wave-instruction lands
// 1 KiB = 8 tile rows x 128 B linearly in LDS; the 16-byte chunk a lane FETCHES is
// XOR-swizzled on the SOURCE side (chunk ^ ((row>>1)&7)) and the same XOR is applied
// when fragments are read, which makes every 16-lane ds_read_b128 group hit 16
// distinct 16-byte slots of the 256-byte bank row (conflict-free).  The hardware
// bounds check of the buffer descriptor zero-fills rows past the end of A / B, so
// ragged M and N need no special staging code.
//
// Pipeline: 2 LDS buffers; the stage of k-tile t+1 is issued before the MFMAs of
// k-tile t (A before the first 32-MFMA cluster, B before the second) and retired
// (vmcnt(0) + barrier) after them.
//
// Persistent mode (short contractions only by default -- see launch_cfg): the grid
// is one workgroup per CU slot, each workgroup walks tiles b, b + G, ... and the first stage
// of the NEXT tile is issued during the last K-step of the current one, so it lands behind
// the epilogue.  With one tile per workgroup the same loop simply runs once.
//
// Two tile configurations share this code (every wave always owns 128x64 outputs):
//   BIG   256x256x64, 8 waves, 128 KiB LDS, one workgroup per CU: best main loop;
//   SMALL 256x128x32, 4 waves,  48 KiB LDS, two workgroups per CU: tiny grids only.
// Tried and dropped in round 1: 4-slot 32-deep LDS ring, split-half
// and quarter-step DMA schedules, start-up stagger, L2 warm-up loads, global_load_lds,
// peeling the under-filled last round into a SMALL-tile launch.
//
// Here: tile configurations, staging, the two main loops, the launch chain, the entry points.  Epilogues: csrc/nt_epilogue.h.
#include "nt_epilogue.h"

namespace {

template <int BK_, int WM_, int WN_, int MI_ = 8>
struct NtCfg {
  static constexpr int BK = BK_, WM = WM_, WN = WN_;
  static constexpr int MI = MI_;                              // 16-row MFMA tiles per wave along M
  static constexpr int WROWS = 16 * MI_;                      // rows per wave
  static constexpr int BM = WROWS * WM_, BN = 64 * WN_;
  static constexpr int WAVES = WM_ * WN_, THREADS = 64 * WM_ * WN_;
  static constexpr int ROWB = BK_ * 2;                       // bytes per tile row
  static constexpr int A_BYTES = BM * ROWB, B_BYTES = BN * ROWB;
  static constexpr int BUF_BYTES = A_BYTES + B_BYTES;
  static constexpr int LDS_BYTES = 2 * BUF_BYTES;
  static constexpr int MIN_WAVES_PER_SIMD = 2;
  static constexpr int WG_PER_CU = (WAVES == 8) ? 1 : 2;     // what registers + LDS allow
};
using NtBig = NtCfg<64, 2, 4>;
using NtSmall = NtCfg<32, 2, 2>;
// 224x256x64 and 192x256x64: fewer rows per tile when that needs fewer tile-rounds of the 256
// CUs than the 256-row tiling (see launch_nt)
using NtBig224 = NtCfg<64, 2, 4, 7>;
using NtBig192 = NtCfg<64, 2, 4, 6>;

// XOR applied to the 16-byte chunk index of tile row r (source side for the DMA, and on
// the fragment reads): BK=64 (128-B rows) chunk ^ ((r>>1)&7); BK=32 (64-B rows)
// chunk ^ 3*((r>>3)&1).  Both make every 16-lane ds_read_b128 group conflict-free.
template <int BK_>
__device__ __forceinline__ int nt_swz(int r) {
  return BK_ == 64 ? ((r >> 1) & 7) : 3 * ((r >> 3) & 1);
}

template <int BK_, int ROWS, int WAVES>
__device__ __forceinline__ void stage_tile(__amdgpu_buffer_rsrc_t rsrc, char* lds_tile, long long row0, int k0,
                                           int K, int wave, int lane) {
  constexpr int ROWB = BK_ * 2;
  constexpr int RPI = 1024 / ROWB;              // tile rows per 1-KiB wave-instruction
  constexpr int LPR = ROWB / 16;                // lanes per row
  constexpr int SLOTS = ROWS / RPI;
  constexpr int PER = (SLOTS + WAVES - 1) / WAVES;   // uneven for 224-row tiles: the last wave issues fewer
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = wave * PER + j;               // wave-uniform instruction slot
    if (SLOTS % WAVES != 0 && i >= SLOTS) break;
    const int r = i * RPI + lane / LPR;         // tile row this lane fetches for
    const int c = lane % LPR;                   // 16-B chunk position in the LDS row
    const int sc = c ^ nt_swz<BK_>(r);          // chunk fetched from global
    const unsigned voff = (unsigned)(((row0 + r) * (long long)K + k0) * 2 + sc * 16);
    dma16_to_lds(rsrc, lds_tile + i * 1024, voff);
  }
}

// s_waitcnt vmcnt(N rounded down to 16, 8 or 0): waits at least as long as the exact count (common.h, wait_vmcnt)
template <int N>
__device__ __forceinline__ void wait_vmcnt_round_down() {
  if constexpr (N >= 16) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
  else if constexpr (N >= 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// Tile of workgroup `bid` (of G) in round r, or false.  Within a round the `cnt` live workgroups
// get an XCD-aware bijective remap: blocks b, b+8, ... share an XCD (round-robin
// dispatch), so each XCD takes a contiguous run of tiles and neighbouring tiles (same A
// row-panel, same weight panels) hit the same L2.  Tiles are ordered column-group-major:
// all tile rows of a group of `group_n` tile columns, then the next group, so a group's
// weight panels are re-used from L2 by every tile row.  Speed only, never correctness.
template <int BM, int BN>
__device__ __forceinline__ bool nt_tile_of(const NtParams& p, const int ntiles, const int G, const int bid, int r, long long& m0, int& n0) {
  const int base = r * G;
  const int cnt = min(G, ntiles - base);
  if (bid >= cnt) return false;
  const int wgid = base + xcd_remap(bid, cnt);
  const int full = p.tiles_m * p.group_n;
  const int cg = wgid / full;
  const int rem = wgid - cg * full;
  const int gw = min(p.group_n, p.tiles_n - cg * p.group_n);
  const int tile_m = rem / gw;
  m0 = (long long)tile_m * BM;
  n0 = (cg * p.group_n + (rem - tile_m * gw)) * BN;
  return true;
}

template <int EPI, typename CFG>
__global__ __launch_bounds__(CFG::THREADS, CFG::MIN_WAVES_PER_SIMD) void gemm_nt_kernel(NtParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int BM = CFG::BM, BN = CFG::BN, BK = CFG::BK;

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave / CFG::WN, wn = wave % CFG::WN;

  const int ntiles = p.tiles_m * p.tiles_n;
  const int G = gridDim.x;
  const int bid = blockIdx.x;
  auto tile_of = [&](int r, long long& m0, int& n0) { return nt_tile_of<BM, BN>(p, ntiles, G, bid, r, m0, n0); };

  const unsigned long long a_bytes = (unsigned long long)p.M * p.K * 2ull;
  const unsigned long long b_bytes = (unsigned long long)p.N * p.K * 2ull;
  __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)p.A, 0, (int)a_bytes, 0x00020000);
  __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc((void*)p.B, 0, (int)b_bytes, 0x00020000);

  const int kb = p.k_chunk ? (int)blockIdx.y * p.k_chunk : 0;                       // this slice's K range
  const int nk = (p.k_chunk ? min(p.K - kb, p.k_chunk) : p.K) / BK;
  const int swz = nt_swz<BK>(lane & 15);           // rows are 16*x + (lane&15)
  const int frag_row = lane & 15;
  const int kq = lane >> 4;

  constexpr int MI = CFG::MI;
  f32x4 acc[4][MI];

  // 32-MFMA cluster of k-step kk (a compile-time constant: a runtime index pushes acc[] to scratch); the BK = 64 loop, which
  // issues DMA between its two clusters, raises the wave's priority over them
  auto compute_half = [&](const char* bufA, const char* bufB, auto kk_c) {
    constexpr int kk = decltype(kk_c)::value;
    const int coff = ((kk * 4 + kq) ^ swz) << 4;
    bf16x8 fb[4], fa[MI];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      fb[j] = *(const bf16x8*)(bufB + (wn * 64 + j * 16 + frag_row) * CFG::ROWB + coff);
#pragma unroll
    for (int i = 0; i < MI; ++i)
      fa[i] = *(const bf16x8*)(bufA + (wm * CFG::WROWS + i * 16 + frag_row) * CFG::ROWB + coff);
    if constexpr (BK == 64) __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < MI; ++i)
        acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j], fa[i], acc[j][i], 0, 0, 0);
    if constexpr (BK == 64) __builtin_amdgcn_s_setprio(0);
  };

  long long m0 = 0, m0n = 0;
  int n0 = 0, n0n = 0;
  if (!tile_of(0, m0, n0)) return;                 // workgroup-uniform
  int par = 0;                                     // LDS buffer of the stage consumed next
  stage_tile<BK, BM, CFG::WAVES>(rsA, smem, m0, kb, p.K, wave, lane);
  stage_tile<BK, BN, CFG::WAVES>(rsB, smem + CFG::A_BYTES, n0, kb, p.K, wave, lane);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  for (int round = 0;; ++round) {
    const bool has_next = tile_of(round + 1, m0n, n0n);
    // stage 0 of this tile has landed for this wave; the barrier makes every wave's share
    // visible and fences the previous tile's last LDS reads from this tile's first DMA
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < MI; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int t = 0; t < nk; ++t) {
      char* bufA = smem + par * CFG::BUF_BYTES;
      char* nA = smem + (par ^ 1) * CFG::BUF_BYTES;
      const bool more = t + 1 < nk;
      // what to prefetch into the other buffer: this tile's next K-step, or the first
      // K-step of the next tile of this workgroup (lands behind the epilogue)
      const bool fetch = more || has_next;
      const long long sm = more ? m0 : m0n;
      const int sn = more ? n0 : n0n;
      const int sk = kb + (more ? (t + 1) * BK : 0);
      if constexpr (BK == 64) {
        // spread the DMA over the step: A before the first MFMA cluster, B between the
        // two (a single 64-KiB burst right after the barrier queues in the TA)
        if (fetch) stage_tile<BK, BM, CFG::WAVES>(rsA, nA, sm, sk, p.K, wave, lane);
        compute_half(bufA, bufA + CFG::A_BYTES, IC<0>{});
        if (fetch) stage_tile<BK, BN, CFG::WAVES>(rsB, nA + CFG::A_BYTES, sn, sk, p.K, wave, lane);
        compute_half(bufA, bufA + CFG::A_BYTES, IC<1>{});
      } else {
        if (fetch) {
          stage_tile<BK, BM, CFG::WAVES>(rsA, nA, sm, sk, p.K, wave, lane);
          stage_tile<BK, BN, CFG::WAVES>(rsB, nA + CFG::A_BYTES, sn, sk, p.K, wave, lane);
        }
        compute_half(bufA, bufA + CFG::A_BYTES, IC<0>{});
      }
      par ^= 1;
      if (more) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
      }
    }

    nt_epilogue<EPI, CFG>(p, acc, m0, n0, wm, wn, lane);

    if (!has_next) break;
    // The next tile's first stage was issued before every store above; vector-memory
    // operations retire in issue order, so "at most <the stores of the last half> still in
    // flight" implies that DMA has landed, without waiting for the stores themselves.
    constexpr int TAIL = nt_epi_tail_stores<EPI>();
    static_assert(TAIL <= nt_epi_row_ops<EPI, false>(true) * MI, "more than this epilogue is certain to store");
    wait_vmcnt_round_down<TAIL>();
    m0 = m0n;
    n0 = n0n;
  }
}

// ====================================================================================
// Ping-pong main loop (BK = 64 tiles, 8 waves): the K-step is cut into 4 phases of one
// 64x32 accumulator quadrant each (16 MFMAs); every phase is {LOAD: fragment ds_reads + the
// LDS-DMA of one half-tile "unit" ; s_barrier ; COMPUTE: 16 MFMAs ; s_barrier}.  Waves 4-7
// (the second wave of every SIMD: tile rows 128..255) run ONE barrier behind waves 0-3, so on
// each SIMD one wave is in its MFMA cluster while its partner reads LDS / issues DMA -- the
// matrix pipe never waits for a fragment read and the two waves never contend for it.
//
// Staging never drains: operands are DMA'd in units of 128 tile rows x 64 k (16 KiB = 2
// wave-instructions per wave): A0/A1 = m-half 0/1 of BOTH wave rows, B0/B1 = n-half 0/1 of all
// four wave columns.  The unit issued in phase p of K-tile t is
//     p0: B1(t+1)   p1: A1(t+1)   p2: B0(t+2)   p3: A0(t+2)
// i.e. a region is refilled two phases after its last fragment read (B0/A0 are read in p0, B1 in
// p1, A1 in p2) and every unit is issued 5-6 phases before its first read.  Waits are counted:
// p0, p1 and p3 end their LOAD part with s_waitcnt vmcnt(8) = "everything but the 4 newest units
// has landed", which is exactly what the NEXT phase reads; p2 needs no wait.  Rules this obeys
// (MI355X guide, "Read a staged buffer one phase AFTER the wait that retires it"): the wait that
// covers a unit sits before the first barrier of the phase preceding its first read (one extra
// barrier because the two wave groups are staggered), and a region is re-issued no earlier
// than two phases after its last read.
//
// The K-tile stream is continuous across OUTPUT tiles (persistent workgroups): while the last
// K-tiles of one output tile are multiplied, the first units of the workgroup's next output tile
// are already in flight, so there is no prologue bubble after the first tile; the epilogue runs
// with ~80 KiB of the next tile staged.  The vector-memory operations of the epilogue sit in the
// same in-order counter, so the first K-tile after an epilogue waits with vmcnt(8 + S), S = a
// lower bound of the epilogue's operations per wave (a smaller count only waits longer).
// Past the last tile the stream issues out-of-range DMA (zero fill, no memory traffic) so every
// count stays uniform.
// two 16-byte fragments of one tile row -> the 32-byte operand of the K = 128 fp8 MFMA
__device__ __forceinline__ i32x8 join_frags(const bf16x8& lo, const bf16x8& hi) {
  const u32x4 a = __builtin_bit_cast(u32x4, lo), b = __builtin_bit_cast(u32x4, hi);
  return i32x8{(int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)b[0], (int)b[1], (int)b[2], (int)b[3]};
}

template <int EPI, typename CFG, bool F8 = false>
__global__ __launch_bounds__(CFG::THREADS, 2) void gemm_nt_pp_kernel(NtParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  static_assert(CFG::BK == 64 && CFG::WM == 2 && CFG::WN == 4, "ping-pong loop is written for 8 waves, BK = 64");
  constexpr int BM = CFG::BM, BN = CFG::BN, MI = CFG::MI;
  constexpr int MH1 = MI - 4;                          // 16-row tiles in the second m-half (first has 4)
  constexpr int BUF = CFG::BUF_BYTES;
  constexpr int DUMMY = 2 * BUF;                       // 1 KiB sink for the slots a short A1 unit does not need
  constexpr unsigned OOBV = 0x80000000u;
  // EPI_GELU (bf16 operands): the 18 KiB GELU table sits behind the sink (see "GELU by table" above nt_epilogue)
  constexpr bool USE_GLUT = EPI == VITSSL_EPI_GELU;
  constexpr int GLUT_BASE = 2 * BUF + 1024;
  constexpr int GLUT_IMM = USE_GLUT ? GLUT_BASE - (int)GLUT_LO8 : -1;
  static_assert(!USE_GLUT || (GLUT_IMM >= 0 && GLUT_IMM < 65536), "the table's offset must fit the ds_read immediate");

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int ntiles = p.tiles_m * p.tiles_n;
  const int G = gridDim.x;
  const int bid = blockIdx.x;

  auto tile_of = [&](int r, long long& m0, int& n0) { return nt_tile_of<BM, BN>(p, ntiles, G, bid, r, m0, n0); };

  long long m0 = 0;
  int n0 = 0;
  if (!tile_of(0, m0, n0)) return;                     // workgroup-uniform, before any barrier

  // Start-up stagger.  Every workgroup runs the same program on equal tiles, so left alone the
  // whole chip alternates between "all CUs in the K loop" (HBM nearly idle) and "all CUs in the
  // epilogue" (a 32-128 MB burst at the HBM rate with the matrix pipes idle): measured 9-23 us of
  // epilogue per tile for the two-image / residual epilogues against 2-4 us of issue time.  With
  // the static tile assignment the workgroups b >= ntiles % G own one tile fewer than the others:
  // they can start up to one tile time late for free.  Spreading their start over that window
  // puts their epilogues beside other CUs' K loops.
  if (p.stagger > 0) {
    const int rem = ntiles % G;
    if (rem != 0 && bid >= rem && wave == 0) {
      const unsigned long long delay = (unsigned long long)p.stagger * (unsigned)(bid - rem) / (unsigned)(G - rem);
      const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
      while (__builtin_amdgcn_s_memrealtime() - t0 < delay) __builtin_amdgcn_s_sleep(8);
    }   // the other waves are held by the prologue's barrier
  }

  // A K-tile is 128 BYTES of every operand row: 64 bf16 or 128 e4m3 elements.  Staging, LDS layout and
  // fragment reads are byte-identical for the two operand types; the fp8 form hands the two 16-byte
  // fragments of a row to ONE v_mfma_f32_16x16x128_f8f6f4 (its k order inside the tile is a permutation
  // applied to both operands alike, which a contraction does not see).
  constexpr unsigned ESZ = F8 ? 1u : 2u;
  const unsigned long long a_bytes = (unsigned long long)p.M * p.K * ESZ;
  const unsigned long long b_bytes = (unsigned long long)p.N * p.K * ESZ;
  const int nk = F8 ? p.K / 128 : p.K / 64;
  const unsigned rowb = (unsigned)p.K * ESZ;           // bytes per operand row

  // ---- staging slots: every wave issues exactly 2 DMA instructions per unit (8 rows x 128 B each)
  // unit A_h: rows g*WROWS + 64 h + 8 q (+ lane/8); unit B_h: rows 64 c + 32 h + 8 q
  unsigned voffA[2][2], voffB[2][2];                   // tile-relative byte offsets of this lane's 16-byte chunk
  int ldsA[2][2], ldsB[2][2];                          // wave-uniform LDS byte offsets inside a buffer
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int s = 2 * wave + e;
      {
        const int per_g = h == 0 ? 8 : 2 * MH1;        // slots per wave row in this unit
        const bool ok = s < 2 * per_g;
        const int g = s / per_g, q = s - g * per_g;
        const int r = g * CFG::WROWS + 64 * h + 8 * q;
        const int rl = r + (lane >> 3);
        const int sc = (lane & 7) ^ ((rl >> 1) & 7);
        voffA[h][e] = ok ? (unsigned)rl * rowb + (unsigned)sc * 16u : OOBV;
        ldsA[h][e] = ok ? r * 128 : DUMMY;
      }
      {
        const int c = s >> 2, q = s & 3;
        const int r = 64 * c + 32 * h + 8 * q;
        const int rl = r + (lane >> 3);
        const int sc = (lane & 7) ^ ((rl >> 1) & 7);
        voffB[h][e] = (unsigned)rl * rowb + (unsigned)sc * 16u;
        ldsB[h][e] = CFG::A_BYTES + r * 128;
      }
    }

  // ---- staging stream: K-tiles in the order they will be multiplied, across output tiles
  struct Cur {
    int round, kt;
    unsigned a, b;          // byte offset of (tile row 0, k0) in A / B; OOBV once the stream has ended
  };
  auto cur_at = [&](int round) {
    Cur c;
    c.round = round;
    c.kt = 0;
    long long mm;
    int nn;
    if (tile_of(round, mm, nn)) {
      c.a = (unsigned)((unsigned long long)mm * rowb);
      c.b = (unsigned)((unsigned long long)nn * rowb);
    } else {
      c.a = c.b = OOBV;
    }
    return c;
  };
  auto cur_next = [&](const Cur& c) {
    if (c.a == OOBV) return c;
    if (c.kt + 1 < nk) {
      Cur n = c;
      n.kt += 1;
      n.a += 128u;
      n.b += 128u;
      return n;
    }
    return cur_at(c.round + 1);
  };
  // DMA of one unit: 2 wave-instructions.  bufsel = LDS buffer (0/1) of the unit's K-tile.
  auto stage_a = [&](const Cur& c, int bufsel, auto h_c) {
    constexpr int h = decltype(h_c)::value;
    // The K-tile's position goes into the DESCRIPTOR (scalar arithmetic: window = operand bytes from (tile row 0, k0) on; an ended
    // stream gets an empty window -> zero fill, no traffic), not into the lanes' offsets: the LOAD parts of this loop share their SIMD
    // with the partner wave's MFMA cluster and vector-ALU instructions there cost issue slots (csrc/gemm_tn.hip).
    __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)p.A + c.a), 0, c.a == OOBV ? 0 : (int)(a_bytes - c.a), 0x00020000);
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const bool live = ldsA[h][e] != DUMMY;
      // (an ended stream has c.a = OOBV: out of range for every live slot -> zero fill)
      dma16_to_lds(rs, smem + (live ? bufsel * BUF : 0) + ldsA[h][e], voffA[h][e]);
    }
  };
  auto stage_b = [&](const Cur& c, int bufsel, auto h_c) {
    constexpr int h = decltype(h_c)::value;
    __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)p.B + c.b), 0, c.b == OOBV ? 0 : (int)(b_bytes - c.b), 0x00020000);
#pragma unroll
    for (int e = 0; e < 2; ++e)
      dma16_to_lds(rs, smem + bufsel * BUF + ldsB[h][e], voffB[h][e]);
  };

  // ---- fragment addressing (as in gemm_nt_kernel)
  const int frag_row = lane & 15;
  const int kq = lane >> 4;
  const int swz = nt_swz<64>(frag_row);
  const int offA0 = (wm * CFG::WROWS + frag_row) * 128 + (((0 + kq) ^ swz) << 4);
  const int offA1 = (wm * CFG::WROWS + frag_row) * 128 + (((4 + kq) ^ swz) << 4);
  const int offB0 = CFG::A_BYTES + (wn * 64 + frag_row) * 128 + (((0 + kq) ^ swz) << 4);
  const int offB1 = CFG::A_BYTES + (wn * 64 + frag_row) * 128 + (((4 + kq) ^ swz) << 4);

  f32x4 acc[4][MI];
  bf16x8 fa[2][4];          // A fragments of the current m-half: [kk][tile]
  bf16x8 fb[2][2][2];       // B fragments: [n-half][kk][tile]

  auto read_a = [&](const char* buf, auto mh_c) {
    constexpr int mh = decltype(mh_c)::value;
    constexpr int cnt = mh == 0 ? 4 : MH1;
#pragma unroll
    for (int ii = 0; ii < cnt; ++ii) {
      fa[0][ii] = *(const bf16x8*)(buf + offA0 + (4 * mh + ii) * 2048);
      fa[1][ii] = *(const bf16x8*)(buf + offA1 + (4 * mh + ii) * 2048);
    }
  };
  auto read_b = [&](const char* buf, auto nh_c) {
    constexpr int nh = decltype(nh_c)::value;
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      fb[nh][0][jj] = *(const bf16x8*)(buf + offB0 + (2 * nh + jj) * 2048);
      fb[nh][1][jj] = *(const bf16x8*)(buf + offB1 + (2 * nh + jj) * 2048);
    }
  };
  // (s_setprio 1 around these clusters was neutral in round 2 and cost 0.5-1.5 % with the leaner loops of round 3: 8 more scalar
  // instructions per K-tile in LOAD parts that are bound by issue slots; profiles/r03_tls_ab.txt)
  auto mma_quad = [&](auto mh_c, auto nh_c) {
    constexpr int mh = decltype(mh_c)::value, nh = decltype(nh_c)::value;
    constexpr int cnt = mh == 0 ? 4 : MH1;
    if constexpr (F8) {
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const i32x8 bq = join_frags(fb[nh][0][jj], fb[nh][1][jj]);
#pragma unroll
        for (int ii = 0; ii < cnt; ++ii)
          acc[2 * nh + jj][4 * mh + ii] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
              bq, join_frags(fa[0][ii], fa[1][ii]), acc[2 * nh + jj][4 * mh + ii], 0, 0, 0, 0, 0, 0);   // e4m3 x e4m3, scales 0 = unscaled form
      }
    } else {
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
#pragma unroll
          for (int ii = 0; ii < cnt; ++ii)
            acc[2 * nh + jj][4 * mh + ii] =
                __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[nh][kk][jj], fa[kk][ii], acc[2 * nh + jj][4 * mh + ii], 0, 0, 0);
    }
  };
  // One K-tile = 4 phases.  NW = counted wait of p0 / p1 / p3 (8, or 8 + S right after an epilogue).
  auto ktile = [&](int buf, const Cur& c1, const Cur& c2, bool last_of_round, auto nw_c) {
    constexpr int NW = decltype(nw_c)::value;
    const char* cur = smem + buf * BUF;
    // p0: quadrant (m0, n0)
    read_b(cur, IC<0>{});
    read_a(cur, IC<0>{});
    stage_b(c1, buf ^ 1, IC<1>{});
    wait_vmcnt<NW>();
    raw_barrier();
    mma_quad(IC<0>{}, IC<0>{});
    raw_barrier();
    // p1: quadrant (m0, n1)
    read_b(cur, IC<1>{});
    stage_a(c1, buf ^ 1, IC<1>{});
    wait_vmcnt<NW>();
    raw_barrier();
    mma_quad(IC<0>{}, IC<1>{});
    raw_barrier();
    // p2: quadrant (m1, n1)
    read_a(cur, IC<1>{});
    stage_b(c2, buf, IC<0>{});
    raw_barrier();
    mma_quad(IC<1>{}, IC<1>{});
    raw_barrier();
    // p3: quadrant (m1, n0)
    stage_a(c2, buf, IC<0>{});
    wait_vmcnt<NW>();
    raw_barrier();
    mma_quad(IC<1>{}, IC<0>{});
    // waves 4-7 leave the stagger at the end of an output tile (they re-enter it with the
    // barrier at the top of the next one): both wave groups then run their epilogues together
    if (!(last_of_round && wm == 1)) raw_barrier();
  };

  // ---- prologue: K-tiles 0 and (B0, A0 of) 1 of the stream
  Cur c0 = cur_at(0);
  Cur c1 = cur_next(c0);
  stage_b(c0, 0, IC<0>{});
  stage_a(c0, 0, IC<0>{});
  stage_b(c0, 0, IC<1>{});
  stage_a(c0, 0, IC<1>{});
  stage_b(c1, 1, IC<0>{});
  stage_a(c1, 1, IC<0>{});
  Cur c2 = cur_next(c1);
  if constexpr (USE_GLUT) {
    if ((unsigned)(unsigned long long)LDS_PTR(smem) != 0u) __builtin_trap();      // glut_read addresses the table by raw LDS offsets
    // fill the table while the first K-tiles are in flight: entry (magnitude index, sign) = the two bf16 results for that
    // bf16 input, from the SAME function the arithmetic path evaluates.  Every wave passes the K loop's barriers before
    // the first epilogue reads it.
    const float hs = p.drop_on ? 0.5f * p.dk.scale : 0.5f;
    const float cs = p.drop_on ? 0.3989422804014327f * p.dk.scale : 0.3989422804014327f;
    unsigned* tab = (unsigned*)(smem + GLUT_BASE);
    for (int e = threadIdx.x; e < GLUT_ENTRIES; e += CFG::THREADS) {
      const unsigned h = (unsigned)((e >> 1) + (GLUT_E_LO << 7)) | ((unsigned)(e & 1) << 15);
      float y, dy;
      gelu_both_scaled(bf2f((bf16_t)h), hs, cs, y, dy);
      if constexpr (F8) {
        const float qs = p.qscale ? *p.qscale : 1.0f;
        tab[e] = (unsigned)f2bf(dy) | ((pack_fp8x4(y * qs, 0.f, 0.f, 0.f) & 0xffu) << 16);
      } else {
        tab[e] = (unsigned)f2bf(y) | ((unsigned)f2bf(dy) << 16);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
  wait_vmcnt<8>();                               // B0, A0 of K-tile 0 have landed
  raw_barrier();

  constexpr int S = nt_epi_vmem_ops<EPI, MI, F8>();
  constexpr int NW = 8;                                // "all but the 4 newest units have landed"
  constexpr int NW_POST = (NW + S) > 63 ? 63 : (NW + S);
  int buf = 0;
#ifdef VITSSL_NT_STAMPS
  auto stamp = [&](int round, int which) {
    if (!(p.stamps && (wave & 3) == 0 && lane == 0 && round < 16)) return;
    p.stamps[(((size_t)bid * 2 + wm) * 16 + round) * 4 + which] = __builtin_amdgcn_s_memrealtime();
    // second half of the buffer: the same points in shader clocks (in-kernel clock = d s_memtime / d s_memrealtime x 100 MHz)
    p.stamps[(size_t)256 * 2 * 16 * 4 + (((size_t)bid * 2 + wm) * 16 + round) * 4 + which] = __builtin_amdgcn_s_memtime();
  };
#else
  auto stamp = [&](int, int) {};
#endif
  for (int round = 0;; ++round) {
    stamp(round, 0);
    if (wm == 1) raw_barrier();                        // waves 4-7 run one barrier behind waves 0-3
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < MI; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < nk; ++t) {
      const bool last = t + 1 == nk;
      if (t == 0 && round > 0) ktile(buf, c1, c2, last, IC<NW_POST>{});
      else ktile(buf, c1, c2, last, IC<NW>{});
      c1 = c2;
      c2 = cur_next(c2);
      buf ^= 1;
    }
    stamp(round, 1);
    if constexpr (F8) {
      if (p.alpha || p.alpha2) {
        const float al = (p.alpha ? *p.alpha : 1.0f) * (p.alpha2 ? *p.alpha2 : 1.0f);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int i = 0; i < MI; ++i) acc[j][i] *= al;
      }
    }
    // the wave's LDS window for line-shaped stores: its own two B1 staging slots (2 KiB, contiguous) of the buffer whose B1 / A1
    // units are not in flight -- K-tile (last) read them two barriers ago, and this wave itself re-issues them in p0 of the
    // next K-tile, after its epilogue in program order; no other wave ever writes there
    nt_epilogue<EPI, CFG, F8, GLUT_IMM, true>(p, acc, m0, n0, wm, wn, lane, smem, smem + (buf ^ 1) * BUF + ldsB[1][0]);
    stamp(round, 2);
#ifdef VITSSL_NT_STAMPS
    if (p.stamps) {                                    // diagnostic: when have this wave's stores been acknowledged?
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      stamp(round, 3);
    }
#endif
    if (!tile_of(round + 1, m0, n0)) break;
  }
  // the stream's trailing (out-of-range, zero-filling) DMA must have retired before the LDS is released
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

int cu_count() { return vitssl_persistent_cus(); }

template <int EPI, typename CFG, bool F8 = false>
int launch_pp(NtParams p, hipStream_t s) {
  constexpr int LDS = 2 * CFG::BUF_BYTES + 1024 + (EPI == VITSSL_EPI_GELU ? GLUT_BYTES : 0);
  static VsOnce attr_done{false};
  if (int rc = ensure_lds(gemm_nt_pp_kernel<EPI, CFG, F8>, LDS, attr_done, "gemm_nt")) return rc;
  const long long ntiles = (long long)p.tiles_m * p.tiles_n;
  const long long slots = cu_count();
  const long long grid = ntiles < slots ? ntiles : slots;
  // tile-time estimate for the start-up stagger (us): K loop ~1.45 us per 256-row K-tile + an uncontended epilogue.
  // Round 2 measured the stagger time-neutral: in the accumulator layout a CU's stores were bound inside the CU (55 GB/s) whether or
  // not the other CUs stored at the same moment.  With line-shaped epilogue accesses a CU alone stores 180+ GB/s but only ~55 when
  // all 256 burst together, so spreading the epilogues pays: interleaved A/B, M = 50176: dGELU 281 -> 262 us (N = 3072, K = 768),
  // residual 241 -> 231 (K = 3072), plain stores -1.5..-3 %, never slower; whole step 34.29 -> 34.05 ms.
  // VITSSL_NT_STAGGER (developer knob): scale of the window, 0 = off
  constexpr float STAGGER_SCALE = 1.0f;
  static VsEnvMilli stagger_knob;
  const float stagger_scale = stagger_knob.get("VITSSL_NT_STAGGER", STAGGER_SCALE);
  // Which epilogues stagger (bit = VITSSL_EPI_* value; VITSSL_NT_STAGGER_EPIS overrides).  Spreading the workgroups in time costs L2
  // sharing (the workgroups of a raster group are no longer at the same k): FETCH_SIZE per launch with / without stagger
  // (tools/fetch_ab.sh): plain bf16, 224-row tiles 415 / 282 MB, residual 547 / 412, dGELU 692 / 645, GELU 347 / 344.  Whole step
  // (same box, alternating, ms): all 33.12, residual + dGELU 33.13, dGELU only 33.26, none 33.42 -> only the two epilogues that are
  // bound by their own traffic stagger.
  constexpr int STAGGER_EPIS = (1 << VITSSL_EPI_RESID) | (1 << VITSSL_EPI_DGELU);
  static VsEnvInt stagger_mask_knob;
  const int stagger_mask = stagger_mask_knob.get("VITSSL_NT_STAGGER_EPIS", STAGGER_EPIS);
  const float tile_us = (float)(p.K * p.esz / 128) * 1.45f * (float)CFG::MI / 8.f + nt_epi(EPI).epi_us;
  p.stagger = ((stagger_mask >> nt_epi(EPI).stagger_bit) & 1) ? (int)(stagger_scale * tile_us * 100.f) : 0;
  vitssl_note_nt_grid((int)grid);
  hipLaunchKernelGGL((gemm_nt_pp_kernel<EPI, CFG, F8>), dim3((unsigned)grid), dim3(CFG::THREADS), LDS, s, p);
  VS_CHECK_LAUNCH("gemm_nt_pp");
  return VITSSL_OK;
}

template <int EPI, typename CFG>
int launch_cfg_parts(NtParams p, hipStream_t s) {
  if constexpr (CFG::LDS_BYTES > 48 * 1024) {
    static VsOnce attr_done{false};
    if (int rc = ensure_lds(gemm_nt_kernel<EPI, CFG>, CFG::LDS_BYTES, attr_done, "gemm_nt")) return rc;
  }
  p.tiles_m = (int)ceil_div64(p.M, CFG::BM);
  p.tiles_n = (int)ceil_div64(p.N, CFG::BN);
  const int want = (int)((2 * 1024 * 1024) / ((long long)CFG::BN * p.K * p.esz));   // panels of a group <= ~2 MiB of L2
  static VsEnvInt group_env;                           // VITSSL_NT_GROUPN: force the raster group width (developer knob)
  const int group_knob = group_env.get("VITSSL_NT_GROUPN", 0);
  if (group_knob > 0) p.group_n = group_knob < p.tiles_n ? group_knob : p.tiles_n;
  else if (p.tiles_n <= 4) p.group_n = p.tiles_n;
  else if (want <= 2) p.group_n = 2;
  else if (p.tiles_n % 6 == 0 && want >= 6) p.group_n = 6;
  else if (p.tiles_n % 4 == 0) p.group_n = 4;
  else if (p.tiles_n % 3 == 0) p.group_n = 3;
  else p.group_n = want < 4 ? want : 4;
  if (p.esz == 1) {
    if ((p.N & 7) != 0) {
      vitssl_set_error("gemm_fp8_nt: N=%d must be a multiple of 8", p.N);
      return VITSSL_ERR_ARG;
    }
    // fp8 operands exist for the ping-pong loop and the epilogues nt_epi() marks only
    if constexpr (CFG::WAVES == 8 && CFG::BK == 64 && nt_epi(EPI).fp8) {
      return launch_pp<EPI, CFG, true>(p, s);
    } else {
      vitssl_set_error("gemm_fp8_nt: epilogue %d / tile configuration not built for fp8 operands", EPI);
      return VITSSL_ERR_ARG;
    }
  }
  if constexpr (CFG::WAVES == 8 && CFG::BK == 64 && EPI != EPI_F32_SPLITK) {
    if (p.k_chunk == 0 && (p.N & 7) == 0) return launch_pp<EPI, CFG>(p, s);   // (its line-shaped stores move 8 columns per lane)
  }
  // Persistent workgroups.  Measured on MI355X (bench.py, same box, alternating runs): with
  // K = 768 / 3072 (ViT-B) the NT family takes 23.12 ms per step either way and the whole step
  // is 0.2-0.5 ms slower persistent; with K = 384 (ViT-S: 6 K-steps per tile, the fixed
  // per-tile cost dominates) the step drops 21.75 -> 20.83 ms.  Default: persistent for
  // K <= 512 only; VITSSL_NT_PERSIST=0/1 forces it (developer knob).
  static VsEnvInt persist_env;
  const int knob = persist_env.get("VITSSL_NT_PERSIST", -1);
  const bool persist = knob >= 0 ? knob != 0 : p.K <= 512;
  const long long ntiles = (long long)p.tiles_m * p.tiles_n;
  long long grid = ntiles;
  if (persist) {
    const long long slots = (long long)cu_count() * CFG::WG_PER_CU;
    if (grid > slots) grid = slots;
  }
  const unsigned slices = p.k_chunk ? (unsigned)ceil_div64(p.K, p.k_chunk) : 1u;
  hipLaunchKernelGGL((gemm_nt_kernel<EPI, CFG>), dim3((unsigned)grid, slices), dim3(CFG::THREADS), CFG::LDS_BYTES, s, p);
  VS_CHECK_LAUNCH("gemm_nt");
  return VITSSL_OK;
}

// 0 = auto, 1 = always BIG, 2 = always SMALL, 3 = always 192x256 (VITSSL_NT_TILE, developer knob)
int nt_tile_override() {
  static VsEnvInt knob;
  return knob.get("VITSSL_NT_TILE", 0);
}

// Split-K for fp32 outputs whose grid cannot fill the chip but whose contraction is long
// (DINO head: dX[640,256] = dY[640,65536] . W[65536,256] is 6 SMALL tiles x 2048 K-steps:
// 483 us on 6 CUs).  The K range is cut into slices that accumulate with fp32 atomics into a
// zeroed output.
int launch_splitk_f32(NtParams p, hipStream_t s, bool* done) {
  *done = false;
  const long long tiles = ceil_div64(p.M, NtSmall::BM) * ceil_div64(p.N, NtSmall::BN);
  if (tiles >= 64 || p.K < 4096) return VITSSL_OK;
  // about half a workgroup per CU: more slices mean more colliding fp32 atomics on the small
  // output (M = 512: 128 slices 253 us, 64: 147 us, 32: 103 us, 16: 114 us, 8: 178 us)
  long long slices = (cu_count() / 2 + tiles - 1) / tiles;
  const long long max_slices = p.K / 512;            // at least 16 K-steps of 32 per slice
  if (slices > max_slices) slices = max_slices;
  if (slices < 2) return VITSSL_OK;
  long long chunk = ceil_div64(ceil_div64(p.K, slices), 64) * 64;
  p.k_chunk = (int)chunk;
  hipError_t e = hipMemsetAsync(p.out0, 0, (size_t)p.M * p.N * sizeof(float), s);
  if (e != hipSuccess) {
    vitssl_set_error("gemm_nt: split-K memset failed: %s", hipGetErrorString(e));
    return VITSSL_ERR_LAUNCH;
  }
  *done = true;
  return launch_cfg_parts<EPI_F32_SPLITK, NtSmall>(p, s);      // no column sums here
}


// Column sums (bias gradients): every wave stores its sums in the slot row of its row group (tile row x waves along M, rows past M
// included, as zeros), and the slot rows are added to p.colsum in a fixed order (common.h, deterministic sums).
template <int EPI, typename CFG>
int launch_cfg(NtParams p, hipStream_t s) {
  float* colsum = p.colsum;
  if (!colsum) return launch_cfg_parts<EPI, CFG>(p, s);
  const int groups = (int)ceil_div64(p.M, CFG::BM) * (CFG::BM / CFG::WROWS);
  p.colsum = vs_sum_parts(p.workspace, p.workspace_floats, (long long)groups * p.N, p.M, p.N, "gemm_nt column sums");
  if (!p.colsum) return VITSSL_ERR_ARG;
  const int rc = launch_cfg_parts<EPI, CFG>(p, s);
  if (rc != VITSSL_OK) return rc;
  return vs_reduce_parts(colsum, p.colsum, groups, p.N, p.N, s);
}

template <int EPI>
int launch_nt(const NtParams& p, hipStream_t s) {
  if constexpr (EPI == VITSSL_EPI_F32) {
    if (!p.colsum && p.esz == 2) {
      bool done = false;
      const int rc = launch_splitk_f32(p, s, &done);
      if (rc != VITSSL_OK || done) return rc;
    }
  }
  const int mode = p.esz == 1 ? 0 : nt_tile_override();
  if (mode == 1) return launch_cfg<EPI, NtBig>(p, s);
  if (mode == 2) return launch_cfg<EPI, NtSmall>(p, s);
  if (mode == 3) return launch_cfg<EPI, NtBig192>(p, s);
  if (mode == 4) return launch_cfg<EPI, NtBig224>(p, s);
  // Measured on MI355X (tools/bench_gemm.py, round 1): SMALL loses 10-25 % on every ViT-B
  // shape, heavy epilogues included; it only pays for grids too small to fill the chip.
  const long long big_tiles = ceil_div64(p.M, 256) * ceil_div64(p.N, 256);
  if (big_tiles < 64 && p.esz == 2) return launch_cfg<EPI, NtSmall>(p, s);
  // (N = 384, ViT-S: three exact 128-wide SMALL columns instead of two 256-wide ones with the
  // second half empty were measured too: 21.1 vs 20.9 ms per step, not worth it.)
  //
  // Row counts whose 256-row tiling is "one round and a bit" (DINO global crops: M = 25216,
  // N = 768 -> 297 tiles = 2 rounds for 1.16 rounds of work) are re-tiled with 192-row tiles
  // when that needs fewer tile-rounds: cost model = rounds x (1 for 256x256, 0.78 for 192x256,
  // measured ratio of the two main loops).
  const long long slots = cu_count();
  const long long tn = ceil_div64(p.N, 256);
  const double c256 = (double)ceil_div64(ceil_div64(p.M, 256) * tn, slots);
  const double c224 = 0.90 * (double)ceil_div64(ceil_div64(p.M, 224) * tn, slots);
  const double c192 = 0.78 * (double)ceil_div64(ceil_div64(p.M, 192) * tn, slots);
  double best = c256;
  if (c192 < 0.9 * c256 && c192 <= c224) best = c192;
  else if (c224 < 0.95 * c256) best = c224;
  // (Two launches over disjoint row ranges -- whole rounds of one tile height, then one round of another -- were built and
  // measured in round 2: 0.3 % of a ViT-B step, because the ping-pong loop is bound by the bytes it stages, (rows + 256) per
  // K-tile, so the smaller tiles give the tail back; removed in round 4, DESIGN.md section 12b keeps the numbers.)
  if (best == c192 && best != c256) return launch_cfg<EPI, NtBig192>(p, s);
  if (best == c224 && best != c256) return launch_cfg<EPI, NtBig224>(p, s);
  return launch_cfg<EPI, NtBig>(p, s);
}

}  // namespace

#ifdef VITSSL_NT_STAMPS
static unsigned long long* g_nt_stamps = nullptr;
extern "C" void vitssl_debug_nt_stamps(void* buf) { g_nt_stamps = (unsigned long long*)buf; }
#endif

// the facts of the epilogue a caller names (the internal ids are not the caller's to name: they read as "not an epilogue")
static NtEpiFacts caller_epi(int epi) { return nt_epi(epi >= EPI_F32_SPLITK ? -1 : epi); }

static int check_rowscale(const char* who, const vitssl_rowscale_t* rows, int64_t M) {
  VS_CHECK_ARG(rows->scale && rows->groups > 0 && rows->rows_per_group > 0, "%s: row scales need scale, groups > 0 and rows_per_group > 0", who);
  VS_CHECK_ARG(rows->groups * (int64_t)rows->rows_per_group == M, "%s: groups (%lld) * rows_per_group (%d) must equal M (%lld)", who,
               (long long)rows->groups, rows->rows_per_group, (long long)M);
  return VITSSL_OK;
}

static int gemm_nt_entry(const vitssl_gemm_t* g, int esz, const vitssl_fp8_gemm_t* q, void* stream, const vitssl_rowscale_t* rows = nullptr,
                         const vitssl_colscale_t* cols = nullptr, void* branch = nullptr) {
  const char* who = cols ? "gemm_nt_ls" : rows ? "gemm_nt_rows" : esz == 1 ? "gemm_fp8_nt" : "gemm_nt";
  VS_CHECK_ARG(g && g->A && g->B && (g->out0 || (esz == 1 && caller_epi(g->epilogue).q8_of == 0 && q && q->out_fp8)), "%s: null operand", who);
  VS_CHECK_ARG(g->M > 0 && g->N > 0 && g->K > 0, "%s: empty problem M=%lld N=%d K=%d", who, (long long)g->M, g->N, g->K);
  VS_CHECK_ARG(g->K % (128 / esz) == 0, "%s: K=%d must be a multiple of %d", who, g->K, 128 / esz);
  VS_CHECK_ARG(g->N % 4 == 0, "%s: N=%d must be a multiple of 4", who, g->N);
  VS_CHECK_ARG(g->N <= (1 << 20), "%s: N=%d exceeds 2^20 (epilogue windows use 32-bit byte offsets)", who, g->N);
  VS_CHECK_ARG((unsigned long long)g->M * g->K * (unsigned)esz < (1ull << 31) && (unsigned long long)g->N * g->K * (unsigned)esz < (1ull << 31),
               "%s: operand larger than 2 GiB (M=%lld N=%d K=%d)", who, (long long)g->M, g->N, g->K);
  // the leading fields in declaration order, the rest zero (tiles_m .. stagger are set down the launch chain)
  NtParams p{(const bf16_t*)g->A, (const bf16_t*)g->B, g->M, g->N, g->K, g->bias, g->aux, g->out0, g->out1, g->colsum, g->workspace,
             g->workspace_floats, make_drop_key(g->drop)};
  p.drop_on = p.dk.thr != 0;
  p.embed = g->embed;
  p.esz = esz;
  if (q) {
    p.alpha = q->alpha;
    p.alpha2 = q->alpha2;
    p.out2 = q->out_fp8;
    p.qscale = q->out_scale;
    p.qamax = q->out_amax;
  }
  p.rows_per_group = 1;
#ifdef VITSSL_NT_STAMPS
  p.stamps = g_nt_stamps;
#endif
  hipStream_t s = (hipStream_t)stream;
  VS_CHECK_ARG(!g->colsum || caller_epi(g->epilogue).colsum, "%s: column sums are built for the BF16 / F32 / DGELU epilogues only", who);
  VS_CHECK_ARG(!p.drop_on || (unsigned long long)g->M * (unsigned long long)g->N < (1ull << 34),
               "%s: dropout over %lld x %d elements: the stream's group counter is 32 bits (M * N < 2^34)", who, (long long)g->M, g->N);
  if (rows || cols) {
    // vitssl_gemm_bf16_nt_rows / _ls: the residual epilogue with a per-row scale of the branch, or a per-column one (+ optional row scales)
    VS_CHECK_ARG(g->epilogue == VITSSL_EPI_RESID, "%s: %s scales are built for VITSSL_EPI_RESID only, got epilogue %d", who,
                 cols ? "column" : "row", g->epilogue);
    VS_CHECK_ARG(g->aux, "%s: EPI_RESID needs aux (residual)", who);
    if (cols) {
      VS_CHECK_ARG(cols->gamma, "%s: null gamma", who);
      VS_CHECK_ARG(cols->cols == g->N, "%s: cols (%d) must equal N (%d)", who, cols->cols, g->N);
    }
    if (rows) {
      if (int rc = check_rowscale(who, rows, g->M)) return rc;
      p.rowscale = rows->scale;
      p.rows_per_group = (unsigned)rows->rows_per_group;
    }
    if (!cols) return launch_nt<EPI_RESID_ROWS>(p, s);
    p.colscale = cols->gamma;
    p.out1 = branch;
    return launch_nt<EPI_RESID_LS>(p, s);
  }
  switch (g->epilogue) {
    case VITSSL_EPI_BF16: return launch_nt<VITSSL_EPI_BF16>(p, s);
    case VITSSL_EPI_F32: return launch_nt<VITSSL_EPI_F32>(p, s);
    case VITSSL_EPI_GELU:
      VS_CHECK_ARG(g->out1 || p.out2, "%s: EPI_GELU needs out1 (or, with fp8 operands, out_fp8)", who);
      return launch_nt<VITSSL_EPI_GELU>(p, s);
    case VITSSL_EPI_RESID:
      VS_CHECK_ARG(g->aux, "%s: EPI_RESID needs aux (residual)", who);
      return launch_nt<VITSSL_EPI_RESID>(p, s);
    case VITSSL_EPI_DGELU:
      VS_CHECK_ARG(g->aux, "%s: EPI_DGELU needs aux (pre-activation)", who);
      return launch_nt<VITSSL_EPI_DGELU>(p, s);
    case VITSSL_EPI_EMBED:
      VS_CHECK_ARG(g->embed.pos && g->embed.tokens > 0 && g->embed.out_tokens >= g->embed.tokens + g->embed.tok_offset,
                   "%s: EPI_EMBED needs pos/tokens", who);
      VS_CHECK_ARG(!g->embed.mask || g->embed.mask_token, "%s: EPI_EMBED mask without mask_token", who);
      return launch_nt<VITSSL_EPI_EMBED>(p, s);
    default:
      vitssl_set_error("%s: unknown epilogue %d", who, g->epilogue);
      return VITSSL_ERR_ARG;
  }
}

extern "C" int vitssl_gemm_bf16_nt(const vitssl_gemm_t* g, void* stream) { return gemm_nt_entry(g, 2, nullptr, stream); }

extern "C" int vitssl_gemm_bf16_nt_rows(const vitssl_gemm_t* g, const vitssl_rowscale_t* rows, void* stream) {
  VS_CHECK_ARG(rows, "gemm_nt_rows: null row scales (vitssl_gemm_bf16_nt is the launch without them)");
  return gemm_nt_entry(g, 2, nullptr, stream, rows);
}

extern "C" int vitssl_gemm_bf16_nt_ls(const vitssl_gemm_t* g, const vitssl_colscale_t* cols, const vitssl_rowscale_t* rows,
                                      void* branch_bf16, void* stream) {
  VS_CHECK_ARG(cols, "gemm_nt_ls: null column scales (vitssl_gemm_bf16_nt / vitssl_gemm_bf16_nt_rows are the launches without them)");
  return gemm_nt_entry(g, 2, nullptr, stream, rows, cols, branch_bf16);
}

extern "C" int vitssl_gemm_fp8_nt(const vitssl_gemm_t* g, const vitssl_fp8_gemm_t* q, void* stream) {
  VS_CHECK_ARG(g && caller_epi(g->epilogue).fp8, "gemm_fp8_nt: fp8 operands are built for the BF16 / F32 / GELU / RESID / DGELU epilogues");
  VS_CHECK_ARG(!(q && q->out_fp8) || caller_epi(g->epilogue).q8_of >= 0, "gemm_fp8_nt: out_fp8 belongs to EPI_GELU / EPI_DGELU");
  return gemm_nt_entry(g, 1, q, stream);
}
