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
// across the block's 4 waves in LDS and stored to the block's slot row of the caller's
// workspace; a reduce launch then adds the slot rows to the targets in a fixed order
// (common.h, deterministic sums).  Every backward entry point goes through the one
// launch_ln_bwd below, which alone decides the grid and so the slot layout.
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

// One call of any backward entry point.  The form -- HAS_LN, Q8 (the fp8 triple), ROWS (row scales) and LS (the LayerScale triple) --
// is the entry point's compile-time choice; the members a form does not take stay null.
struct LnBwdCall {
  const char* who;                                  // the name the entry point's messages carry
  const void* dy;
  const float *x, *mean, *rstd, *gamma, *g_res;
  float* g_out;
  void* gm;
  float *dgamma, *dbeta, *gm_colsum;
  vitssl_dropout_t drop;
  int64_t rows;
  int cols;
  float* workspace;
  int64_t workspace_floats;
  hipStream_t s;
  void* gm8;                                        // Q8
  const float* qscale;
  float* qamax;
  const vitssl_rowscale_t* rowscale;                // ROWS (LS: or NULL)
  const float* lsgamma;                             // LS
  const void* branch;
  float* dls;
};

// The launch path of every backward form.  The kernel writes one slot row per block for each column sum (dgamma, dbeta, gm_colsum
// and, with LayerScale, dls); they are then added to the targets in a fixed order (common.h, deterministic sums).  The grid, and
// with it the layout of the slot rows, is decided here and nowhere else.  What is built: row pairs (PAIR) for the bf16 image of
// the LayerNorm form at V = 3 only; LayerScale with the column sums and the row scales only (gm_colsum, the row scales and dls may
// be absent at run time).
template <bool HAS_LN, bool Q8 = false, bool ROWS = false, bool LS = false>
int launch_ln_bwd(const LnBwdCall& c) {
  static_assert(!Q8 || !ROWS, "row scales are built for the bf16 image");
  static_assert(!LS || ROWS, "LayerScale is built on the form with row scales");
  const int64_t rows = c.rows;
  const int cols = c.cols;
  DropKey dk = make_drop_key(c.drop);
  const int on = dk.thr != 0;
  VS_CHECK_ARG(!on || (unsigned long long)rows * (unsigned long long)cols < (1ull << 34),
               "%s: the dropout stream's group counter is 32 bits (rows * cols < 2^34)", c.who);
  constexpr bool CAN_PAIR = HAS_LN && !Q8;
  const bool pair = CAN_PAIR && cols == 384 && (rows & 1) == 0;   // two rows per wave: the kernel sees rows / 2 rows of 768 columns
  const long long krows = pair ? rows / 2 : rows;
  const int kcols = pair ? 768 : cols;
  const int grid = ln_grid(krows, false, kcols);
  const long long slab = (long long)grid * cols;

  constexpr int NSUMS = LS ? 4 : 3;
  float* const target[4] = {HAS_LN ? c.dgamma : nullptr, HAS_LN ? c.dbeta : nullptr, c.gm_colsum, LS ? c.dls : nullptr};
  float* slot[4] = {nullptr, nullptr, nullptr, nullptr};
  const bool sums = target[0] || target[1] || target[2] || target[3];
  if (sums) {                                       // the documented promise is what the caller's workspace is held to (vs_sum_parts)
    const char* sizing = LS ? "vitssl_layerscale_workspace_floats" : "vitssl_sum_workspace_floats";
    const long long promised = LS ? vitssl_layerscale_workspace_floats(rows, cols) : vitssl_sum_workspace_floats(rows, cols);
    VS_CHECK_ARG(NSUMS * slab <= promised, "%s: this launch needs %lld floats of workspace, %s(%lld, %d) promises %lld", c.who,
                 NSUMS * slab, sizing, (long long)rows, cols, promised);
    float* parts = vs_parts(c.workspace, c.workspace_floats, promised, c.who, sizing);
    if (!parts) return VITSSL_ERR_ARG;
    for (int q = 0; q < NSUMS; ++q)
      if (target[q]) slot[q] = parts + q * slab;
  }

  const float* rscale = c.rowscale ? c.rowscale->scale : nullptr;
  const unsigned rpg = c.rowscale ? (unsigned)c.rowscale->rows_per_group : 1u;
#define VS_LN_BWD_ARGS                                                                                                              \
  dim3(grid), dim3(LN_THREADS), 0, c.s, (const bf16_t*)c.dy, c.x, c.mean, c.rstd, c.gamma, c.g_res, c.g_out, (bf16_t*)c.gm, slot[0], \
      slot[1], slot[2], dk, on, krows, kcols, (unsigned char*)c.gm8, c.qscale, c.qamax, rscale, rpg
  auto launch = [&](auto v, auto cs, auto pr) {
    constexpr int V = decltype(v)::value;
    constexpr bool CS = decltype(cs)::value, PAIR = decltype(pr)::value;
    static_assert(!PAIR || (CAN_PAIR && V == 3), "row pairs: the LayerNorm form with a bf16 image, 2 x 384 columns");
    static_assert(!LS || CS, "LayerScale is built with the column sums");
    if constexpr (LS)
      hipLaunchKernelGGL((ln_bwd_kernel<V, HAS_LN, CS, Q8, PAIR, ROWS, LnLsArgs>), VS_LN_BWD_ARGS,
                         LnLsArgs{c.lsgamma, (const bf16_t*)c.branch, slot[3]});
    else
      hipLaunchKernelGGL((ln_bwd_kernel<V, HAS_LN, CS, Q8, PAIR, ROWS>), VS_LN_BWD_ARGS);
  };
#undef VS_LN_BWD_ARGS
  auto with_cs = [&](auto v, auto pr) {
    if (LS || c.gm_colsum) launch(v, std::true_type{}, pr);
    else if constexpr (!LS) launch(v, std::false_type{}, pr);
  };
  using std::integral_constant;
  if (pair) {
    if constexpr (CAN_PAIR) with_cs(integral_constant<int, 3>{}, std::true_type{});
  } else if (cols <= 256) with_cs(integral_constant<int, 1>{}, std::false_type{});
  else if (cols <= 512) with_cs(integral_constant<int, 2>{}, std::false_type{});
  else if (cols <= 768) with_cs(integral_constant<int, 3>{}, std::false_type{});
  else if (cols <= 1024) with_cs(integral_constant<int, 4>{}, std::false_type{});
  else with_cs(integral_constant<int, 8>{}, std::false_type{});
  VS_CHECK_LAUNCH(LS ? c.who : (ROWS ? "layernorm_bwd_rows" : "layernorm_bwd"));
  if (!sums) return VITSSL_OK;
  return vs_reduce_parts(VsSums{{target[0], target[1], target[2], target[3]}, {slot[0], slot[1], slot[2], slot[3]}}, grid, cols, cols, c.s);
}

template <bool Q8>
int launch_ln_fwd(const char* who, const float* x, const float* gamma, const float* beta, void* y_bf16, void* y_fp8, float* mean,
                  float* rstd, int64_t rows, int cols, float eps, hipStream_t s) {
  const int grid = ln_grid(rows, true);
#define VS_LNF(V)                                                                                                                 \
  hipLaunchKernelGGL((ln_fwd_kernel<V, Q8>), dim3(grid), dim3(LN_THREADS), 0, s, x, gamma, beta, (bf16_t*)y_bf16, mean, rstd, \
                     (long long)rows, cols, eps, (unsigned char*)y_fp8)
  if (cols <= 256) VS_LNF(1);
  else if (cols <= 512) VS_LNF(2);
  else if (cols <= 768) VS_LNF(3);
  else if (cols <= 1024) VS_LNF(4);
  else VS_LNF(8);
#undef VS_LNF
  VS_CHECK_LAUNCH(who);
  return VITSSL_OK;
}

}  // namespace

extern "C" int vitssl_layernorm_fwd(const float* x, const float* gamma, const float* beta, void* y_bf16, float* mean,
                                    float* rstd, int64_t rows, int cols, float eps, void* stream) {
  VS_CHECK_ARG(x && gamma && beta && y_bf16 && mean && rstd, "layernorm_fwd: null pointer");
  VS_CHECK_ARG(rows > 0 && cols > 0 && cols % 4 == 0 && cols <= 2048, "layernorm_fwd: cols=%d must be a multiple of 4 and <= 2048", cols);
  return launch_ln_fwd<false>("layernorm_fwd", x, gamma, beta, y_bf16, nullptr, mean, rstd, rows, cols, eps, (hipStream_t)stream);
}

extern "C" int vitssl_layernorm_fwd_fp8(const float* x, const float* gamma, const float* beta, void* y_bf16, void* y_fp8,
                                        float* mean, float* rstd, int64_t rows, int cols, float eps, void* stream) {
  VS_CHECK_ARG(x && gamma && beta && y_fp8 && mean && rstd, "layernorm_fwd_fp8: null pointer");   // y_bf16 may be NULL
  VS_CHECK_ARG(rows > 0 && cols > 0 && cols % 4 == 0 && cols <= 2048, "layernorm_fwd_fp8: cols=%d must be a multiple of 4 and <= 2048", cols);
  return launch_ln_fwd<true>("layernorm_fwd_fp8", x, gamma, beta, y_bf16, y_fp8, mean, rstd, rows, cols, eps, (hipStream_t)stream);
}

// ---- backward.  The plain, fp8 and row-scale (drop path) forms share the name their workspace and dropout messages carry.
static const char* const LN_BWD_WHO = "layernorm_bwd / grad_mask_cast";

// (drop path: the _rows forms take the same contracts with the bf16 operand scaled per row, include/vitssl_droppath.h)
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
  return launch_ln_bwd<true, false, true>({LN_BWD_WHO, dy_bf16, x, mean, rstd, gamma, g_res, g_out, gm_bf16, dgamma, dbeta, gm_colsum, drop,
                                           rows, cols, workspace, workspace_floats, (hipStream_t)stream, nullptr, nullptr, nullptr, rowscale});
}

extern "C" int vitssl_layernorm_bwd(const void* dy_bf16, const float* x, const float* mean, const float* rstd,
                                    const float* gamma, const float* g_res, float* g_out, void* gm_bf16, float* dgamma,
                                    float* dbeta, float* gm_colsum, vitssl_dropout_t drop, int64_t rows, int cols,
                                    float* workspace, int64_t workspace_floats, void* stream) {
  VS_CHECK_ARG(dy_bf16 && x && mean && rstd && gamma && g_out && dgamma && dbeta, "layernorm_bwd: null pointer");
  VS_CHECK_ARG(rows > 0 && cols > 0 && cols % 4 == 0 && cols <= 2048, "layernorm_bwd: cols=%d must be a multiple of 4 and <= 2048", cols);
  VS_CHECK_ARG(!gm_colsum || gm_bf16, "layernorm_bwd: gm_colsum without gm_bf16");
  return launch_ln_bwd<true>({LN_BWD_WHO, dy_bf16, x, mean, rstd, gamma, g_res, g_out, gm_bf16, dgamma, dbeta, gm_colsum, drop, rows, cols,
                              workspace, workspace_floats, (hipStream_t)stream});
}

extern "C" int vitssl_layernorm_bwd_fp8(const void* dy_bf16, const float* x, const float* mean, const float* rstd,
                                        const float* gamma, const float* g_res, float* g_out, void* gm_bf16, void* gm_fp8,
                                        const float* qscale, float* qamax, float* dgamma, float* dbeta, float* gm_colsum,
                                        vitssl_dropout_t drop, int64_t rows, int cols, float* workspace, int64_t workspace_floats, void* stream) {
  VS_CHECK_ARG(dy_bf16 && x && mean && rstd && gamma && g_out && dgamma && dbeta && gm_fp8, "layernorm_bwd_fp8: null pointer");   // gm_bf16 may be NULL
  VS_CHECK_ARG(rows > 0 && cols > 0 && cols % 4 == 0 && cols <= 2048, "layernorm_bwd_fp8: cols=%d must be a multiple of 4 and <= 2048", cols);
  return launch_ln_bwd<true, true>({LN_BWD_WHO, dy_bf16, x, mean, rstd, gamma, g_res, g_out, gm_bf16, dgamma, dbeta, gm_colsum, drop, rows,
                                    cols, workspace, workspace_floats, (hipStream_t)stream, gm_fp8, qscale, qamax});
}

// ---- the mask + cast + column-sum form of the same launch (no LayerNorm)
extern "C" int vitssl_grad_mask_cast_fp8(const float* g, void* gm_bf16, void* gm_fp8, const float* qscale, float* qamax,
                                         float* gm_colsum, vitssl_dropout_t drop, int64_t rows, int cols, float* workspace, int64_t workspace_floats, void* stream) {
  VS_CHECK_ARG(g && gm_fp8, "grad_mask_cast_fp8: null pointer");   // gm_bf16 may be NULL
  VS_CHECK_ARG(rows > 0 && cols > 0 && cols % 4 == 0 && cols <= 2048, "grad_mask_cast_fp8: cols=%d must be a multiple of 4 and <= 2048", cols);
  return launch_ln_bwd<false, true>({LN_BWD_WHO, nullptr, nullptr, nullptr, nullptr, nullptr, g, nullptr, gm_bf16, nullptr, nullptr, gm_colsum,
                                     drop, rows, cols, workspace, workspace_floats, (hipStream_t)stream, gm_fp8, qscale, qamax});
}

extern "C" int vitssl_grad_mask_cast_rows(const float* g, void* gm_bf16, float* gm_colsum, vitssl_dropout_t drop,
                                          const vitssl_rowscale_t* rowscale, int64_t rows, int cols, float* workspace,
                                          int64_t workspace_floats, void* stream) {
  VS_CHECK_ARG(g && gm_bf16, "grad_mask_cast_rows: null pointer");
  VS_CHECK_ARG(rows > 0 && cols > 0 && cols % 4 == 0 && cols <= 2048, "grad_mask_cast_rows: cols=%d must be a multiple of 4 and <= 2048", cols);
  if (int rc = check_rowscale("grad_mask_cast_rows", rowscale, rows)) return rc;
  return launch_ln_bwd<false, false, true>({LN_BWD_WHO, nullptr, nullptr, nullptr, nullptr, nullptr, g, nullptr, gm_bf16, nullptr, nullptr,
                                            gm_colsum, drop, rows, cols, workspace, workspace_floats, (hipStream_t)stream, nullptr, nullptr,
                                            nullptr, rowscale});
}

extern "C" int vitssl_grad_mask_cast(const float* g, void* gm_bf16, float* gm_colsum, vitssl_dropout_t drop,
                                     int64_t rows, int cols, float* workspace, int64_t workspace_floats, void* stream) {
  VS_CHECK_ARG(g && gm_bf16, "grad_mask_cast: null pointer");
  VS_CHECK_ARG(rows > 0 && cols > 0 && cols % 4 == 0 && cols <= 2048, "grad_mask_cast: cols=%d must be a multiple of 4 and <= 2048", cols);
  return launch_ln_bwd<false>({LN_BWD_WHO, nullptr, nullptr, nullptr, nullptr, nullptr, g, nullptr, gm_bf16, nullptr, nullptr, gm_colsum, drop,
                               rows, cols, workspace, workspace_floats, (hipStream_t)stream});
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
  return launch_ln_bwd<true, false, true, true>({"layernorm_bwd_ls", dy_bf16, x, mean, rstd, gamma, g_res, g_out, gm_bf16, dgamma, dbeta,
                                                 gm_colsum, drop, rows, cols, workspace, workspace_floats, (hipStream_t)stream, nullptr, nullptr,
                                                 nullptr, rowscale, colscale->gamma, branch_bf16, dls});
}

extern "C" int vitssl_grad_mask_cast_ls(const float* g, void* gm_bf16, float* gm_colsum, vitssl_dropout_t drop,
                                        const vitssl_rowscale_t* rowscale, const vitssl_colscale_t* colscale, const void* branch_bf16,
                                        float* dls, int64_t rows, int cols, float* workspace, int64_t workspace_floats, void* stream) {
  VS_CHECK_ARG(g && gm_bf16, "grad_mask_cast_ls: null pointer");
  if (int rc = check_ls("grad_mask_cast_ls", rowscale, colscale, branch_bf16, dls, rows, cols)) return rc;
  return launch_ln_bwd<false, false, true, true>({"grad_mask_cast_ls", nullptr, nullptr, nullptr, nullptr, nullptr, g, nullptr, gm_bf16, nullptr,
                                                  nullptr, gm_colsum, drop, rows, cols, workspace, workspace_floats, (hipStream_t)stream,
                                                  nullptr, nullptr, nullptr, rowscale, colscale->gamma, branch_bf16, dls});
}
