// LayerNorm forward / backward for the fp32 residual stream (gfx950, HBM-bound).
//
// One 64-lane wave per row; the row lives in registers as V float4 per lane
// (cols <= 256*V), statistics are two-pass in fp32 via wavefront shuffles, the
// output is emitted as bf16 (the operand of the next MFMA GEMM).
//
// Backward fuses, per row: LN input-gradient, + residual-branch gradient, fp32 store
// of the new residual gradient, and the dropout-masked bf16 copy the next
// (reverse-order) GEMM consumes; per column: dgamma, dbeta and the bias-gradient
// column sum are accumulated in registers across the rows a wave visits, reduced
// across the block's 4 waves in LDS and added to global with one atomic per column
// per block.
#include "../../include/vitssl_droppath.h"
#include "../../include/vitssl_layerscale.h"
#include "common.h"

namespace {

constexpr int LN_THREADS = 256;  // 4 waves = 4 rows in flight per block

// Q8: also emit the e4m3 image of the output (fp8 operand path, unit scale)
template <int V, bool Q8 = false>
__global__ __launch_bounds__(LN_THREADS) void ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, bf16_t* __restrict__ y,
                                                            float* __restrict__ mean, float* __restrict__ rstd,
                                                            long long rows, int cols, float eps, unsigned char* __restrict__ y8 = nullptr) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int c4n = cols >> 2;
  f32x4 g[V], b[V];
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const int c4 = lane + 64 * v;
    if (c4 < c4n) {
      g[v] = *(const f32x4*)(gamma + 4 * c4);
      b[v] = *(const f32x4*)(beta + 4 * c4);
    }
  }
  const float inv = 1.0f / (float)cols;
  const long long row_step = (long long)gridDim.x * 4;
  f32x4 nxt[V];                                   // the next row of this wave, requested before the current one is reduced
  auto fetch = [&](long long row) {
    if (row >= rows) return;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const int c4 = lane + 64 * v;
      if (c4 < c4n) nxt[v] = *(const f32x4*)(x + row * cols + 4 * c4);
    }
  };
  fetch((long long)blockIdx.x * 4 + wave);
  for (long long row = (long long)blockIdx.x * 4 + wave; row < rows; row += row_step) {
    f32x4 xv[V];
    float s = 0.f;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const int c4 = lane + 64 * v;
      if (c4 < c4n) {
        xv[v] = nxt[v];
        s += xv[v][0] + xv[v][1] + xv[v][2] + xv[v][3];
      }
    }
    fetch(row + row_step);                        // the next row's load flies under the reductions and the stores
    const float mu = wave_sum(s) * inv;
    float ss = 0.f;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const int c4 = lane + 64 * v;
      if (c4 < c4n) {
        xv[v] -= mu;
        ss += xv[v][0] * xv[v][0] + xv[v][1] * xv[v][1] + xv[v][2] * xv[v][2] + xv[v][3] * xv[v][3];
      }
    }
    const float rs = rsqrtf(wave_sum(ss) * inv + eps);
    if (lane == 0) {
      mean[row] = mu;
      rstd[row] = rs;
    }
    bf16_t* yr = y + row * cols;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const int c4 = lane + 64 * v;
      if (c4 < c4n) {
        const f32x4 o = xv[v] * rs * g[v] + b[v];
        if (!Q8 || y) {                         // fp8 path: the bf16 image is optional (kernel-argument uniform)
          u32x2 w = {pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3])};
          *(u32x2*)(yr + 4 * c4) = w;
        }
        if constexpr (Q8) *(unsigned*)(y8 + row * cols + 4 * c4) = pack_fp8x4(o[0], o[1], o[2], o[3]);
      }
    }
  }
}

// workgroups per CU the register budget is sized for.  The prefetching form holds two rows of operands; where that
// spills, fewer resident waves win (MI355X, interleaved A/B, M = 50176, D = 768: with column sums + dropout
// 134 us without prefetch, 154 at 3 workgroups (spills), 125 at 2; without column sums 132 -> 118 at 3)
constexpr int ln_bwd_blocks(int V, bool has_ln, bool has_cs) {
  if (!has_ln) return (V <= 2 || (V == 3 && !has_cs)) ? 4 : (V <= 4 ? 3 : 1);
  return V <= 1 ? 4 : (V == 2 ? (has_cs ? 3 : 4) : (V == 3 ? (has_cs ? 2 : 3) : (V == 4 ? 2 : 1)));
}

// HAS_LN = false turns the kernel into the plain "mask + cast + column-sum" of g_res.
// Q8: also write the e4m3 image gm8 = e4m3(gm * *qscale) and record max |gm| in *qamax (fp8 dgrad operand).
// PAIR (rows of 384 columns, ViT-S): a wave takes two consecutive rows = one contiguous run of 192 float4 = three full
// 64-lane vectors, the access shape of a 768-column row.  One row per wave leaves half the lanes of the second vector idle
// (96 float4 = 64 + 32) and half as many bytes per wave in flight: 57.8 us against 52.2 for M = 50176 (5.3 -> 5.9 TB/s; 33.8 ->
// 28.9 us at M = 25088; interleaved A/B, MI355X).  The caller passes rows = row pairs and cols = 2 x the row length; a slot
// (lane, v) belongs to the pair's second row where lane + 64 v >= cols / 8, and the row statistics are reduced per row.  (The
// same form of the FORWARD kernel was 17 % slower than one row per wave, 24.5 against 21.0 us, and is not built.)
// ROWS (drop path, include/vitssl_droppath.h): the bf16 operand of row r is multiplied once more, by rowscale[r / rows_per_group];
// g_out, dgamma and dbeta are not.  An instantiation of its own: the plain kernels are what they were.  (The row-pair form without
// column sums spills at 3 workgroups per CU once it also holds the pair's two scales: it takes the budget of the form with them.)
// LS (LayerScale, include/vitssl_layerscale.h; built with ROWS and HAS_CS, rowscale and gm_colsum may be NULL at run time): the
// bf16 operand is multiplied once more, by lsgamma[column], and where dls is given a fourth column sum, of sc * g_out * branch, is
// kept; the branch image is requested with the row's other operands so that the prefetch stays one round trip.
struct LnLsArgs {                                   // the arguments only the LayerScale form takes
  const float* gamma;                               // f32 [cols]
  const bf16_t* branch;                             // bf16 [rows, cols] or NULL
  float* dls;                                       // slot rows of gamma's gradient or NULL (with branch)
};
__device__ __forceinline__ const LnLsArgs& ln_first(const LnLsArgs& a) { return a; }
// (1024 columns with LayerNorm: the four sums and the branch image do not fit the two-workgroup budget without scratch; rows above
// 512 columns run one workgroup per CU anyway, ln_grid)
constexpr int ln_bwd_ls_blocks(int V, bool has_ln) { return has_ln && V == 4 ? 1 : ln_bwd_blocks(V, has_ln, true); }

// (the LayerScale arguments travel as a parameter pack, empty in every other instantiation: those keep the argument list, and so
// the code, they had)
template <int V, bool HAS_LN, bool HAS_CS, bool Q8 = false, bool PAIR = false, bool ROWS = false, typename... LSARGS>
__global__ __launch_bounds__(LN_THREADS, sizeof...(LSARGS) ? ln_bwd_ls_blocks(V, HAS_LN) : ln_bwd_blocks(V, HAS_LN, HAS_CS || (ROWS && PAIR))) void ln_bwd_kernel(const bf16_t* __restrict__ dy, const float* __restrict__ x,
                                                            const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            const float* __restrict__ gamma, const float* g_res,
                                                            float* g_out, bf16_t* __restrict__ gm, float* __restrict__ dgamma,
                                                            float* __restrict__ dbeta, float* __restrict__ gm_colsum,
                                                            DropKey dk, int drop_on, long long rows, int cols,
                                                            unsigned char* __restrict__ gm8 = nullptr,
                                                            const float* __restrict__ qscale = nullptr, float* qamax = nullptr,
                                                            const float* __restrict__ rowscale = nullptr, unsigned rows_per_group = 1,
                                                            LSARGS... lsargs) {
  constexpr bool LS = sizeof...(LSARGS) > 0;
  const float* __restrict__ lsgamma = nullptr;
  const bf16_t* __restrict__ branch = nullptr;
  float* __restrict__ dls = nullptr;
  if constexpr (LS) {
    const LnLsArgs& a = ln_first(lsargs...);
    lsgamma = a.gamma;
    branch = a.branch;
    dls = a.dls;
  }
  __shared__ __attribute__((aligned(16))) float red[4][V * 256];   // [wave][col]
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int c4n = cols >> 2;
  const int c4h = PAIR ? c4n >> 1 : c4n;            // float4 per row
  static_assert(!PAIR || (HAS_LN && !Q8), "row pairs are built for the LayerNorm form with a bf16 image");
  static_assert(!ROWS || !Q8, "row scales are built for the bf16 image");
  static_assert(!LS || (ROWS && HAS_CS), "LayerScale is built on the form with row scales and column sums");
  f32x4 g[V], acc_dg[V], acc_db[V], acc_cs[V];
  f32x4 lsg[V], acc_ls[V];                          // LS: gamma of the slot's four columns, running sum of its gradient
  bool hi[V];                                       // PAIR: the slot holds columns of the pair's second row
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const int c4 = lane + 64 * v;
    hi[v] = PAIR && c4 >= c4h;
    acc_dg[v] = f32x4{0.f, 0.f, 0.f, 0.f};
    acc_db[v] = acc_dg[v];
    acc_cs[v] = acc_dg[v];
    if (HAS_LN && c4 < c4n) g[v] = *(const f32x4*)(gamma + 4 * (c4 - (hi[v] ? c4h : 0)));
    if constexpr (LS) {
      acc_ls[v] = acc_dg[v];
      if (c4 < c4n) lsg[v] = *(const f32x4*)(lsgamma + 4 * (c4 - (hi[v] ? c4h : 0)));
    }
  }
  const float inv = 1.0f / (float)(PAIR ? cols >> 1 : cols);
  const float qs = (Q8 && qscale) ? *qscale : 1.0f;
  float qmax = 0.f;
  // raw operands of one row (HAS_LN): x, residual gradient, packed dy, statistics
  f32x4 nx[V], ngr[V];
  u32x2 ndy[V];
  u32x2 nbr[V];                                     // LS: the row's packed branch image
  float nmu = 0.f, nrs = 0.f, nmuB = 0.f, nrsB = 0.f;
  float nsc = 1.f, nscB = 1.f;                      // ROWS: scale of the row (PAIR: of the pair's two rows); rows < 2^31
  auto fetch = [&](long long row) {
    if (!HAS_LN || row >= rows) return;
    if constexpr (ROWS && !LS) {
      nsc = rowscale[(PAIR ? 2u * (unsigned)row : (unsigned)row) / rows_per_group];
      if constexpr (PAIR) nscB = rowscale[(2u * (unsigned)row + 1u) / rows_per_group];
    }
    if constexpr (LS) {
      if (rowscale) {                               // kernel-argument uniform: LayerScale without drop path keeps the ones
        nsc = rowscale[(PAIR ? 2u * (unsigned)row : (unsigned)row) / rows_per_group];
        if constexpr (PAIR) nscB = rowscale[(2u * (unsigned)row + 1u) / rows_per_group];
      }
    }
    if constexpr (PAIR) {
      nmu = mean[2 * row];
      nrs = rstd[2 * row];
      nmuB = mean[2 * row + 1];
      nrsB = rstd[2 * row + 1];
    } else {
      nmu = mean[row];
      nrs = rstd[row];
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const int c4 = lane + 64 * v;
      if (c4 < c4n) {
        if (g_res) ngr[v] = *(const f32x4*)(g_res + row * cols + 4 * c4);
        ndy[v] = *(const u32x2*)(dy + row * cols + 4 * c4);
        if constexpr (LS) {
          if (dls) nbr[v] = *(const u32x2*)(branch + row * cols + 4 * c4);
        }
        nx[v] = *(const f32x4*)(x + row * cols + 4 * c4);
      }
    }
  };
  const long long row_step = (long long)gridDim.x * 4;
  fetch((long long)blockIdx.x * 4 + wave);
  for (long long row = (long long)blockIdx.x * 4 + wave; row < rows; row += row_step) {
    f32x4 dx[V];
    u32x2 brp[V];                                   // LS: the branch image of this row (taken before the next row's fetch)
    float sc = 1.f, scB = 1.f;
    // (mask + cast form: no prefetch to ride on.  A row belongs to one wave, so the index is made wave-uniform and the scale comes
    // through the scalar cache: as a vector load at the loop head it made every row wait for the previous row's stores first,
    // +16 us at 50432 x 768)
    if constexpr (ROWS && !HAS_LN && !LS) sc = rowscale[__builtin_amdgcn_readfirstlane((unsigned)row / rows_per_group)];
    if constexpr (LS && !HAS_LN) {
      if (rowscale) sc = rowscale[__builtin_amdgcn_readfirstlane((unsigned)row / rows_per_group)];
    }
    if constexpr (ROWS && HAS_LN) {
      sc = nsc;
      scB = nscB;
    }
    if constexpr (HAS_LN) {
      const float mu = nmu, rs = nrs, muB = nmuB, rsB = nrsB;
      f32x4 xh[V], gr[V];
      u32x2 dyp[V];
#pragma unroll
      for (int v = 0; v < V; ++v) {
        xh[v] = nx[v];
        gr[v] = ngr[v];
        dyp[v] = ndy[v];
      }
      if constexpr (LS) {
#pragma unroll
        for (int v = 0; v < V; ++v) brp[v] = nbr[v];
      }
      fetch(row + row_step);                      // in flight during everything below
      float s1 = 0.f, s2 = 0.f, s1B = 0.f, s2B = 0.f;
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const int c4 = lane + 64 * v;
        if (c4 < c4n) {
          const f32x4 d = {bf_lo(dyp[v][0]), bf_hi(dyp[v][0]), bf_lo(dyp[v][1]), bf_hi(dyp[v][1])};
          xh[v] = (xh[v] - (hi[v] ? muB : mu)) * (hi[v] ? rsB : rs);
          const f32x4 dyg = d * g[v];
          acc_dg[v] += d * xh[v];
          acc_db[v] += d;
          const float t1 = dyg[0] + dyg[1] + dyg[2] + dyg[3];
          const f32x4 t = dyg * xh[v];
          const float t2 = t[0] + t[1] + t[2] + t[3];
          if (hi[v]) {
            s1B += t1;
            s2B += t2;
          } else {
            s1 += t1;
            s2 += t2;
          }
        }
      }
      const float m1 = wave_sum(s1) * inv;
      const float m2 = wave_sum(s2) * inv;
      const float m1B = PAIR ? wave_sum(s1B) * inv : 0.f;
      const float m2B = PAIR ? wave_sum(s2B) * inv : 0.f;
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const int c4 = lane + 64 * v;
        if (c4 < c4n) {
          const f32x4 d = {bf_lo(dyp[v][0]), bf_hi(dyp[v][0]), bf_lo(dyp[v][1]), bf_hi(dyp[v][1])};
          dx[v] = (d * g[v] - (hi[v] ? m1B : m1) - xh[v] * (hi[v] ? m2B : m2)) * (hi[v] ? rsB : rs);
          if (g_res) dx[v] += gr[v];
          *(f32x4*)(g_out + row * cols + 4 * c4) = dx[v];
        }
      }
    } else {
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const int c4 = lane + 64 * v;
        if (c4 < c4n) dx[v] = *(const f32x4*)(g_res + row * cols + 4 * c4);
        if constexpr (LS) {
          if (dls && c4 < c4n) brp[v] = *(const u32x2*)(branch + row * cols + 4 * c4);
        }
      }
    }
    if (gm || (Q8 && gm8)) {
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const int c4 = lane + 64 * v;
        if (c4 < c4n) {
          f32x4 o = dx[v];
          if (drop_on) {
            bool keep[4];
            drop_keep4(dk, drop_words(dk, (unsigned)row * (unsigned)c4n + (unsigned)c4), keep);
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = keep[r] ? o[r] * dk.scale : 0.f;
          }
          if constexpr (ROWS) o *= hi[v] ? scB : sc;
          if constexpr (LS) {
            o *= lsg[v];
            if (dls) {                             // d gamma: rs * g_out * u; a dropped sample (rs == 0) adds exact zeros
              const float rsv = hi[v] ? scB : sc;
              const f32x4 u = {bf_lo(brp[v][0]), bf_hi(brp[v][0]), bf_lo(brp[v][1]), bf_hi(brp[v][1])};
#pragma unroll
              for (int r = 0; r < 4; ++r) acc_ls[v][r] += rsv == 0.f ? 0.f : rsv * dx[v][r] * u[r];
            }
          }
          if (gm) {                              // fp8 path: the bf16 image is optional
            u32x2 w = {pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3])};
            *(u32x2*)(gm + row * cols + 4 * c4) = w;
          }
          if constexpr (Q8) {
            *(unsigned*)(gm8 + row * cols + 4 * c4) = pack_fp8x4(o[0] * qs, o[1] * qs, o[2] * qs, o[3] * qs);
            qmax = fmaxf(qmax, fmaxf(fmaxf(fabsf(o[0]), fabsf(o[1])), fmaxf(fabsf(o[2]), fabsf(o[3]))));
          }
          if (HAS_CS) acc_cs[v] += o;
        }
      }
    }
  }
  if constexpr (Q8) {
    if (qamax) {
      qmax = wave_max(qmax);
      unsigned* slot = (unsigned*)qamax;
      if (lane == 0 && __float_as_uint(qmax) > __builtin_nontemporal_load(slot)) atomicMax(slot, __float_as_uint(qmax));
    }
  }
  // cross-wave column reduction into this block's slot row of each sum (LDS buffer reused); launch_ln_bwd sums the slots
#pragma unroll
  for (int qty = 0; qty < (LS ? 4 : 3); ++qty) {
    if (qty < 2 && !HAS_LN) continue;
    if (qty == 2 && !HAS_CS) continue;
    float* target = qty == 0 ? dgamma : (qty == 1 ? dbeta : gm_colsum);
    if constexpr (LS) {
      if (qty == 3) target = dls;
    }
    if (!target) continue;   // kernel-argument uniform
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const int c4 = lane + 64 * v;
      if (c4 < c4n) {
        f32x4 a = qty == 0 ? acc_dg[v] : (qty == 1 ? acc_db[v] : acc_cs[v]);
        if constexpr (LS) {
          if (qty == 3) a = acc_ls[v];
        }
        *(f32x4*)&red[wave][4 * c4] = a;
      }
    }
    __syncthreads();
    if constexpr (PAIR) {                            // a column's two slots: columns c and c + cols / 2 of the pair
      const int ch = cols >> 1;
      for (int c = threadIdx.x; c < ch; c += LN_THREADS)
        target[(long long)blockIdx.x * ch + c] = (red[0][c] + red[1][c] + red[2][c] + red[3][c]) +
                                                 (red[0][c + ch] + red[1][c + ch] + red[2][c + ch] + red[3][c + ch]);
    } else {
      for (int c = threadIdx.x; c < cols; c += LN_THREADS)
        target[(long long)blockIdx.x * cols + c] = red[0][c] + red[1][c] + red[2][c] + red[3][c];
    }
    __syncthreads();
  }
}

// Blocks of 4 rows, grid-stride.  Backward: every block ends with one slot row per accumulated vector (summed in order by a
// reduce launch; the measurements below were taken when it was one atomic per column), and
// the register budget admits 2-4 blocks per CU, so a grid larger than what is resident at once only adds such tails:
// one block per CU (two for rows of <= 512 columns) is fastest now that the next row is prefetched (MI355X, interleaved
// A/B against the former cap of 2048: M = 50176, D = 768: 123 -> 110 us, with column sums 126 -> 111; D = 1024,
// M = 25088: 89 -> 75; D = 384: 79 -> 58; DINO local crops, M = 18944, D = 768: 65 -> 37).  Forward has no such tail:
// 4096 blocks give 43.5-43.6 ms per ViT-B step against 43.8 with 2048 (uncapped: 43.7).
constexpr long long LN_FWD_GRID_CAP = 4096;
inline int ln_grid(long long rows, bool fwd = false, int cols = 1024) {
  long long g = (rows + 3) / 4;
  long long cap = fwd ? LN_FWD_GRID_CAP : (long long)vitssl_persistent_cus() * (cols <= 512 ? 2 : 1);
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

// The launches of launch_ln_bwd_parts below for the ROWS instantiations: the same column-count paths, the 384-column row pairs
// included, the same grids (so the slot rows of the sums are laid out as launch_ln_bwd expects).
template <bool HAS_LN>
int launch_ln_bwd_rows(const void* dy, const float* x, const float* mean, const float* rstd, const float* gamma, const float* g_res,
                       float* g_out, void* gm, float* dgamma, float* dbeta, float* gm_colsum, DropKey dk, int on, int64_t rows, int cols,
                       hipStream_t s, vitssl_rowscale_t rsc) {
  const unsigned rpg = (unsigned)rsc.rows_per_group;
#define VS_LNR(V, CS, PAIR, GRID, ROWS_, COLS_)                                                                                     \
  hipLaunchKernelGGL((ln_bwd_kernel<V, HAS_LN, CS, false, PAIR, true>), dim3(GRID), dim3(LN_THREADS), 0, s, (const bf16_t*)dy, x, mean, \
                     rstd, gamma, g_res, g_out, (bf16_t*)gm, dgamma, dbeta, gm_colsum, dk, on, (long long)(ROWS_), COLS_,             \
                     (unsigned char*)nullptr, (const float*)nullptr, (float*)nullptr, rsc.scale, rpg)
  if constexpr (HAS_LN) {
    if (cols == 384 && (rows & 1) == 0) {            // two rows per wave (PAIR)
      const int pgrid = ln_grid(rows / 2, false, 768);
      if (gm_colsum) VS_LNR(3, true, true, pgrid, rows / 2, 768);
      else VS_LNR(3, false, true, pgrid, rows / 2, 768);
      VS_CHECK_LAUNCH("layernorm_bwd_rows");
      return VITSSL_OK;
    }
  }
  const int grid = ln_grid(rows, false, cols);
#define VS_LNRV(V)                                          \
  do {                                                      \
    if (gm_colsum) VS_LNR(V, true, false, grid, rows, cols); \
    else VS_LNR(V, false, false, grid, rows, cols);          \
  } while (0)
  if (cols <= 256) VS_LNRV(1);
  else if (cols <= 512) VS_LNRV(2);
  else if (cols <= 768) VS_LNRV(3);
  else if (cols <= 1024) VS_LNRV(4);
  else VS_LNRV(8);
#undef VS_LNRV
#undef VS_LNR
  VS_CHECK_LAUNCH("layernorm_bwd_rows");
  return VITSSL_OK;
}

// LayerScale (include/vitssl_layerscale.h): the launches of launch_ln_bwd_rows for the LS instantiations (always built with the
// column sums; gm_colsum, the row scales and dls may be absent at run time), then the four sums' slot rows added in one pass.
template <bool HAS_LN>
int launch_ln_bwd_ls(const char* who, const void* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                     const float* g_res, float* g_out, void* gm, float* dgamma, float* dbeta, float* gm_colsum, vitssl_dropout_t drop,
                     const vitssl_rowscale_t* rsc, const float* lsgamma, const void* branch, float* dls, int64_t rows, int cols,
                     float* workspace, int64_t workspace_floats, hipStream_t s) {
  DropKey dk = make_drop_key(drop);
  const int on = dk.thr != 0;
  VS_CHECK_ARG(!on || (unsigned long long)rows * (unsigned long long)cols < (1ull << 34),
               "%s: the dropout stream's group counter is 32 bits (rows * cols < 2^34)", who);
  const bool pair = HAS_LN && cols == 384 && (rows & 1) == 0;
  const int grid = pair ? ln_grid(rows / 2, false, 768) : ln_grid(rows, false, cols);
  const long long slab = (long long)grid * cols;
  const bool sums = (HAS_LN && (dgamma || dbeta)) || gm_colsum || dls;
  float *pg = nullptr, *pb = nullptr, *pc = nullptr, *pl = nullptr;
  if (sums) {
    const long long promised = vitssl_layerscale_workspace_floats(rows, cols);
    VS_CHECK_ARG(4 * slab <= promised, "%s: this launch needs %lld floats of workspace, vitssl_layerscale_workspace_floats(%lld, %d) promises %lld",
                 who, 4 * slab, (long long)rows, cols, promised);
    float* parts = vs_parts(workspace, workspace_floats, promised, who, "vitssl_layerscale_workspace_floats");
    if (!parts) return VITSSL_ERR_ARG;
    pg = HAS_LN && dgamma ? parts : nullptr;
    pb = HAS_LN && dbeta ? parts + slab : nullptr;
    pc = gm_colsum ? parts + 2 * slab : nullptr;
    pl = dls ? parts + 3 * slab : nullptr;
  }
  const float* rscale = rsc ? rsc->scale : nullptr;
  const unsigned rpg = rsc ? (unsigned)rsc->rows_per_group : 1u;
  const LnLsArgs lsa = {lsgamma, (const bf16_t*)branch, pl};
#define VS_LNL(V, PAIR, GRID, ROWS_, COLS_)                                                                                          \
  hipLaunchKernelGGL((ln_bwd_kernel<V, HAS_LN, true, false, PAIR, true, LnLsArgs>), dim3(GRID), dim3(LN_THREADS), 0, s,              \
                     (const bf16_t*)dy, x, mean, rstd, gamma, g_res, g_out, (bf16_t*)gm, pg, pb, pc, dk, on, (long long)(ROWS_), COLS_, \
                     (unsigned char*)nullptr, (const float*)nullptr, (float*)nullptr, rscale, rpg, lsa)
  if (pair) {
    if constexpr (HAS_LN) VS_LNL(3, true, grid, rows / 2, 768);      // two rows per wave, as the plain entry
  } else if (cols <= 256) VS_LNL(1, false, grid, rows, cols);
  else if (cols <= 512) VS_LNL(2, false, grid, rows, cols);
  else if (cols <= 768) VS_LNL(3, false, grid, rows, cols);
  else if (cols <= 1024) VS_LNL(4, false, grid, rows, cols);
  else VS_LNL(8, false, grid, rows, cols);
#undef VS_LNL
  VS_CHECK_LAUNCH(who);
  if (!sums) return VITSSL_OK;
  return vs_reduce_parts(VsSums{{pg ? dgamma : nullptr, pb ? dbeta : nullptr, pc ? gm_colsum : nullptr, pl ? dls : nullptr}, {pg, pb, pc, pl}},
                         grid, cols, cols, s);
}

template <bool HAS_LN, bool Q8 = false>
int launch_ln_bwd_parts(const void* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                  const float* g_res, float* g_out, void* gm, float* dgamma, float* dbeta, float* gm_colsum,
                  vitssl_dropout_t drop, int64_t rows, int cols, hipStream_t s, void* gm8 = nullptr,
                  const float* qscale = nullptr, float* qamax = nullptr, const vitssl_rowscale_t* rsc = nullptr) {
  DropKey dk = make_drop_key(drop);
  const int on = dk.thr != 0;
  VS_CHECK_ARG(!on || (unsigned long long)rows * (unsigned long long)cols < (1ull << 34),
               "layernorm_bwd / grad_mask_cast: the dropout stream's group counter is 32 bits (rows * cols < 2^34)");
  if constexpr (!Q8) {
    if (rsc) return launch_ln_bwd_rows<HAS_LN>(dy, x, mean, rstd, gamma, g_res, g_out, gm, dgamma, dbeta, gm_colsum, dk, on, rows, cols, s, *rsc);
  }
  if constexpr (HAS_LN && !Q8) {
    if (cols == 384 && (rows & 1) == 0) {            // two rows per wave (PAIR)
      const int pgrid = ln_grid(rows / 2, false, 768);
      if (gm_colsum)
        hipLaunchKernelGGL((ln_bwd_kernel<3, true, true, false, true>), dim3(pgrid), dim3(LN_THREADS), 0, s, (const bf16_t*)dy, x, mean,
                           rstd, gamma, g_res, g_out, (bf16_t*)gm, dgamma, dbeta, gm_colsum, dk, on, (long long)(rows / 2), 768,
                           (unsigned char*)nullptr, (const float*)nullptr, (float*)nullptr);
      else
        hipLaunchKernelGGL((ln_bwd_kernel<3, true, false, false, true>), dim3(pgrid), dim3(LN_THREADS), 0, s, (const bf16_t*)dy, x, mean,
                           rstd, gamma, g_res, g_out, (bf16_t*)gm, dgamma, dbeta, gm_colsum, dk, on, (long long)(rows / 2), 768,
                           (unsigned char*)nullptr, (const float*)nullptr, (float*)nullptr);
      VS_CHECK_LAUNCH("layernorm_bwd");
      return VITSSL_OK;
    }
  }
  const int grid = ln_grid(rows, false, cols);
#define VS_LNB(V)                                                                                                        \
  do {                                                                                                                   \
    if (gm_colsum)                                                                                                       \
      hipLaunchKernelGGL((ln_bwd_kernel<V, HAS_LN, true, Q8>), dim3(grid), dim3(LN_THREADS), 0, s, (const bf16_t*)dy, x, mean, \
                         rstd, gamma, g_res, g_out, (bf16_t*)gm, dgamma, dbeta, gm_colsum, dk, on, (long long)rows, cols,  \
                         (unsigned char*)gm8, qscale, qamax);                                                            \
    else                                                                                                                 \
      hipLaunchKernelGGL((ln_bwd_kernel<V, HAS_LN, false, Q8>), dim3(grid), dim3(LN_THREADS), 0, s, (const bf16_t*)dy, x, mean, \
                         rstd, gamma, g_res, g_out, (bf16_t*)gm, dgamma, dbeta, gm_colsum, dk, on, (long long)rows, cols,  \
                         (unsigned char*)gm8, qscale, qamax);                                                            \
  } while (0)
  if (cols <= 256) VS_LNB(1);
  else if (cols <= 512) VS_LNB(2);
  else if (cols <= 768) VS_LNB(3);
  else if (cols <= 1024) VS_LNB(4);
  else VS_LNB(8);
#undef VS_LNB
  VS_CHECK_LAUNCH("layernorm_bwd");
  return VITSSL_OK;
}

// The kernel writes one slot row per block for each column sum (dgamma, dbeta, gm_colsum); they are then added to the targets
// in a fixed order (common.h, deterministic sums).
template <bool HAS_LN, bool Q8 = false>
int launch_ln_bwd(const void* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                  const float* g_res, float* g_out, void* gm, float* dgamma, float* dbeta, float* gm_colsum,
                  vitssl_dropout_t drop, int64_t rows, int cols, float* workspace, int64_t workspace_floats, hipStream_t s,
                  void* gm8 = nullptr, const float* qscale = nullptr, float* qamax = nullptr, const vitssl_rowscale_t* rsc = nullptr) {
  const bool pair = HAS_LN && !Q8 && cols == 384 && (rows & 1) == 0;
  const int grid = pair ? ln_grid(rows / 2, false, 768) : ln_grid(rows, false, cols);
  const long long slab = (long long)grid * cols;
  if (!((HAS_LN && (dgamma || dbeta)) || gm_colsum))
    return launch_ln_bwd_parts<HAS_LN, Q8>(dy, x, mean, rstd, gamma, g_res, g_out, gm, nullptr, nullptr, nullptr, drop, rows, cols, s, gm8,
                                           qscale, qamax, rsc);
  float* parts = vs_sum_parts(workspace, workspace_floats, 3 * slab, rows, cols, "layernorm_bwd / grad_mask_cast");
  if (!parts) return VITSSL_ERR_ARG;
  float* pg = HAS_LN && dgamma ? parts : nullptr;
  float* pb = HAS_LN && dbeta ? parts + slab : nullptr;
  float* pc = gm_colsum ? parts + 2 * slab : nullptr;
  const int rc = launch_ln_bwd_parts<HAS_LN, Q8>(dy, x, mean, rstd, gamma, g_res, g_out, gm, pg, pb, pc, drop, rows, cols, s, gm8,
                                                 qscale, qamax, rsc);
  if (rc != VITSSL_OK) return rc;
  return vs_reduce_parts(VsSums{{pg ? dgamma : nullptr, pb ? dbeta : nullptr, pc ? gm_colsum : nullptr}, {pg, pb, pc}}, grid, cols,
                         cols, s);
}

}  // namespace

extern "C" int vitssl_layernorm_fwd(const float* x, const float* gamma, const float* beta, void* y_bf16, float* mean,
                                    float* rstd, int64_t rows, int cols, float eps, void* stream) {
  VS_CHECK_ARG(x && gamma && beta && y_bf16 && mean && rstd, "layernorm_fwd: null pointer");
  VS_CHECK_ARG(rows > 0 && cols > 0 && cols % 4 == 0 && cols <= 2048, "layernorm_fwd: cols=%d must be a multiple of 4 and <= 2048", cols);
  hipStream_t s = (hipStream_t)stream;
  const int grid = ln_grid(rows, true);
#define VS_LNF(V)                                                                                                   \
  hipLaunchKernelGGL((ln_fwd_kernel<V, false>), dim3(grid), dim3(LN_THREADS), 0, s, x, gamma, beta, (bf16_t*)y_bf16, mean, rstd, \
                     (long long)rows, cols, eps, (unsigned char*)nullptr)
  if (cols <= 256) VS_LNF(1);
  else if (cols <= 512) VS_LNF(2);
  else if (cols <= 768) VS_LNF(3);
  else if (cols <= 1024) VS_LNF(4);
  else VS_LNF(8);
#undef VS_LNF
  VS_CHECK_LAUNCH("layernorm_fwd");
  return VITSSL_OK;
}

extern "C" int vitssl_layernorm_fwd_fp8(const float* x, const float* gamma, const float* beta, void* y_bf16, void* y_fp8,
                                        float* mean, float* rstd, int64_t rows, int cols, float eps, void* stream) {
  VS_CHECK_ARG(x && gamma && beta && y_fp8 && mean && rstd, "layernorm_fwd_fp8: null pointer");   // y_bf16 may be NULL
  VS_CHECK_ARG(rows > 0 && cols > 0 && cols % 4 == 0 && cols <= 2048, "layernorm_fwd_fp8: cols=%d must be a multiple of 4 and <= 2048", cols);
  const int grid = ln_grid(rows, true);
  hipStream_t s = (hipStream_t)stream;
#define VS_LNF(V)                                                                                                         \
  hipLaunchKernelGGL((ln_fwd_kernel<V, true>), dim3(grid), dim3(LN_THREADS), 0, s, x, gamma, beta, (bf16_t*)y_bf16, mean, rstd, \
                     (long long)rows, cols, eps, (unsigned char*)y_fp8)
  if (cols <= 256) VS_LNF(1);
  else if (cols <= 512) VS_LNF(2);
  else if (cols <= 768) VS_LNF(3);
  else if (cols <= 1024) VS_LNF(4);
  else VS_LNF(8);
#undef VS_LNF
  VS_CHECK_LAUNCH("layernorm_fwd_fp8");
  return VITSSL_OK;
}

extern "C" int vitssl_layernorm_bwd(const void* dy_bf16, const float* x, const float* mean, const float* rstd,
                                    const float* gamma, const float* g_res, float* g_out, void* gm_bf16, float* dgamma,
                                    float* dbeta, float* gm_colsum, vitssl_dropout_t drop, int64_t rows, int cols,
                                    float* workspace, int64_t workspace_floats, void* stream) {
  VS_CHECK_ARG(dy_bf16 && x && mean && rstd && gamma && g_out && dgamma && dbeta, "layernorm_bwd: null pointer");
  VS_CHECK_ARG(rows > 0 && cols > 0 && cols % 4 == 0 && cols <= 2048, "layernorm_bwd: cols=%d must be a multiple of 4 and <= 2048", cols);
  VS_CHECK_ARG(!gm_colsum || gm_bf16, "layernorm_bwd: gm_colsum without gm_bf16");
  return launch_ln_bwd<true>(dy_bf16, x, mean, rstd, gamma, g_res, g_out, gm_bf16, dgamma, dbeta, gm_colsum, drop, rows,
                             cols, workspace, workspace_floats, (hipStream_t)stream);
}

extern "C" int vitssl_layernorm_bwd_fp8(const void* dy_bf16, const float* x, const float* mean, const float* rstd,
                                        const float* gamma, const float* g_res, float* g_out, void* gm_bf16, void* gm_fp8,
                                        const float* qscale, float* qamax, float* dgamma, float* dbeta, float* gm_colsum,
                                        vitssl_dropout_t drop, int64_t rows, int cols, float* workspace, int64_t workspace_floats, void* stream) {
  VS_CHECK_ARG(dy_bf16 && x && mean && rstd && gamma && g_out && dgamma && dbeta && gm_fp8, "layernorm_bwd_fp8: null pointer");   // gm_bf16 may be NULL
  VS_CHECK_ARG(rows > 0 && cols > 0 && cols % 4 == 0 && cols <= 2048, "layernorm_bwd_fp8: cols=%d must be a multiple of 4 and <= 2048", cols);
  return launch_ln_bwd<true, true>(dy_bf16, x, mean, rstd, gamma, g_res, g_out, gm_bf16, dgamma, dbeta, gm_colsum, drop, rows,
                                   cols, workspace, workspace_floats, (hipStream_t)stream, gm_fp8, qscale, qamax);
}

extern "C" int vitssl_grad_mask_cast_fp8(const float* g, void* gm_bf16, void* gm_fp8, const float* qscale, float* qamax,
                                         float* gm_colsum, vitssl_dropout_t drop, int64_t rows, int cols, float* workspace, int64_t workspace_floats, void* stream) {
  VS_CHECK_ARG(g && gm_fp8, "grad_mask_cast_fp8: null pointer");   // gm_bf16 may be NULL
  VS_CHECK_ARG(rows > 0 && cols > 0 && cols % 4 == 0 && cols <= 2048, "grad_mask_cast_fp8: cols=%d must be a multiple of 4 and <= 2048", cols);
  return launch_ln_bwd<false, true>(nullptr, nullptr, nullptr, nullptr, nullptr, g, nullptr, gm_bf16, nullptr, nullptr,
                                    gm_colsum, drop, rows, cols, workspace, workspace_floats, (hipStream_t)stream, gm_fp8, qscale, qamax);
}

extern "C" int vitssl_grad_mask_cast(const float* g, void* gm_bf16, float* gm_colsum, vitssl_dropout_t drop,
                                     int64_t rows, int cols, float* workspace, int64_t workspace_floats, void* stream) {
  VS_CHECK_ARG(g && gm_bf16, "grad_mask_cast: null pointer");
  VS_CHECK_ARG(rows > 0 && cols > 0 && cols % 4 == 0 && cols <= 2048, "grad_mask_cast: cols=%d must be a multiple of 4 and <= 2048", cols);
  return launch_ln_bwd<false>(nullptr, nullptr, nullptr, nullptr, nullptr, g, nullptr, gm_bf16, nullptr, nullptr,
                              gm_colsum, drop, rows, cols, workspace, workspace_floats, (hipStream_t)stream);
}

// ---- drop path: the same two contracts with the bf16 operand scaled per row (include/vitssl_droppath.h) ----------------------
static int check_rowscale(const char* who, const vitssl_rowscale_t* r, int64_t rows) {
  VS_CHECK_ARG(r && r->scale && r->groups > 0 && r->rows_per_group > 0, "%s: row scales need scale, groups > 0 and rows_per_group > 0", who);
  VS_CHECK_ARG(rows < (1ll << 31), "%s: rows = %lld outside rows < 2^31", who, (long long)rows);
  VS_CHECK_ARG(r->groups * (int64_t)r->rows_per_group == rows, "%s: groups (%lld) * rows_per_group (%d) must equal rows (%lld)", who,
               (long long)r->groups, r->rows_per_group, (long long)rows);
  return VITSSL_OK;
}

extern "C" int vitssl_layernorm_bwd_rows(const void* dy_bf16, const float* x, const float* mean, const float* rstd,
                                         const float* gamma, const float* g_res, float* g_out, void* gm_bf16, float* dgamma,
                                         float* dbeta, float* gm_colsum, vitssl_dropout_t drop, const vitssl_rowscale_t* rowscale,
                                         int64_t rows, int cols, float* workspace, int64_t workspace_floats, void* stream) {
  VS_CHECK_ARG(dy_bf16 && x && mean && rstd && gamma && g_out && dgamma && dbeta && gm_bf16, "layernorm_bwd_rows: null pointer");
  VS_CHECK_ARG(rows > 0 && cols > 0 && cols % 4 == 0 && cols <= 2048, "layernorm_bwd_rows: cols=%d must be a multiple of 4 and <= 2048", cols);
  if (int rc = check_rowscale("layernorm_bwd_rows", rowscale, rows)) return rc;
  return launch_ln_bwd<true>(dy_bf16, x, mean, rstd, gamma, g_res, g_out, gm_bf16, dgamma, dbeta, gm_colsum, drop, rows, cols,
                             workspace, workspace_floats, (hipStream_t)stream, nullptr, nullptr, nullptr, rowscale);
}

extern "C" int vitssl_grad_mask_cast_rows(const float* g, void* gm_bf16, float* gm_colsum, vitssl_dropout_t drop,
                                          const vitssl_rowscale_t* rowscale, int64_t rows, int cols, float* workspace,
                                          int64_t workspace_floats, void* stream) {
  VS_CHECK_ARG(g && gm_bf16, "grad_mask_cast_rows: null pointer");
  VS_CHECK_ARG(rows > 0 && cols > 0 && cols % 4 == 0 && cols <= 2048, "grad_mask_cast_rows: cols=%d must be a multiple of 4 and <= 2048", cols);
  if (int rc = check_rowscale("grad_mask_cast_rows", rowscale, rows)) return rc;
  return launch_ln_bwd<false>(nullptr, nullptr, nullptr, nullptr, nullptr, g, nullptr, gm_bf16, nullptr, nullptr, gm_colsum, drop,
                              rows, cols, workspace, workspace_floats, (hipStream_t)stream, nullptr, nullptr, nullptr, rowscale);
}

// ---- LayerScale: the same two contracts with the bf16 operand also scaled per column, and gamma's gradient (include/vitssl_layerscale.h)
static int check_ls(const char* who, const vitssl_rowscale_t* rowscale, const vitssl_colscale_t* colscale, const void* branch,
                    const float* dls, int64_t rows, int cols) {
  VS_CHECK_ARG(rows > 0 && cols > 0 && cols % 4 == 0 && cols <= 2048, "%s: cols=%d must be a multiple of 4 and <= 2048", who, cols);
  VS_CHECK_ARG(rows < (1ll << 31), "%s: rows = %lld outside rows < 2^31", who, (long long)rows);
  VS_CHECK_ARG(colscale && colscale->gamma, "%s: null column scales", who);
  VS_CHECK_ARG(colscale->cols == cols, "%s: column scales hold %d entries for %d columns", who, colscale->cols, cols);
  VS_CHECK_ARG((branch != nullptr) == (dls != nullptr), "%s: branch_bf16 and dls are given together or not at all", who);
  if (rowscale) return check_rowscale(who, rowscale, rows);
  return VITSSL_OK;
}

extern "C" int vitssl_layernorm_bwd_ls(const void* dy_bf16, const float* x, const float* mean, const float* rstd, const float* gamma,
                                       const float* g_res, float* g_out, void* gm_bf16, float* dgamma, float* dbeta, float* gm_colsum,
                                       vitssl_dropout_t drop, const vitssl_rowscale_t* rowscale, const vitssl_colscale_t* colscale,
                                       const void* branch_bf16, float* dls, int64_t rows, int cols, float* workspace,
                                       int64_t workspace_floats, void* stream) {
  VS_CHECK_ARG(dy_bf16 && x && mean && rstd && gamma && g_out && dgamma && dbeta && gm_bf16, "layernorm_bwd_ls: null pointer");
  if (int rc = check_ls("layernorm_bwd_ls", rowscale, colscale, branch_bf16, dls, rows, cols)) return rc;
  return launch_ln_bwd_ls<true>("layernorm_bwd_ls", dy_bf16, x, mean, rstd, gamma, g_res, g_out, gm_bf16, dgamma, dbeta, gm_colsum, drop,
                                rowscale, colscale->gamma, branch_bf16, dls, rows, cols, workspace, workspace_floats, (hipStream_t)stream);
}

extern "C" int vitssl_grad_mask_cast_ls(const float* g, void* gm_bf16, float* gm_colsum, vitssl_dropout_t drop,
                                        const vitssl_rowscale_t* rowscale, const vitssl_colscale_t* colscale, const void* branch_bf16,
                                        float* dls, int64_t rows, int cols, float* workspace, int64_t workspace_floats, void* stream) {
  VS_CHECK_ARG(g && gm_bf16, "grad_mask_cast_ls: null pointer");
  if (int rc = check_ls("grad_mask_cast_ls", rowscale, colscale, branch_bf16, dls, rows, cols)) return rc;
  return launch_ln_bwd_ls<false>("grad_mask_cast_ls", nullptr, nullptr, nullptr, nullptr, nullptr, g, nullptr, gm_bf16, nullptr, nullptr,
                                 gm_colsum, drop, rowscale, colscale->gamma, branch_bf16, dls, rows, cols, workspace, workspace_floats,
                                 (hipStream_t)stream);
}
