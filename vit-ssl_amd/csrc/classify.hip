// Classification loss of the supervised / fine-tune step (gfx950): nn.CrossEntropyLoss(mean, ignore_index, label_smoothing)
// on the padded fp32 output of the classifier GEMM, the zero-padded bf16 d(logits) the head's backward GEMMs read, the bias
// gradient, the predictions and the epoch counters.  include/vitssl_classify.h declares the entry point and its contract.
//
// One wave per row, CL_WAVES rows a workgroup; lane l owns columns 4 l .. 4 l + 3 of every 256-column chunk, so a wave reads
// a chunk as 64 x 16 bytes and writes its bf16 gradient as 64 x 8 bytes.  All arithmetic is fp64 (the inputs are fp32, so
// z - max is exact; gfx950 issues vector fp64 at half the fp32 rate and a row of classes is far too short to be bound by
// it): the bf16 gradient is then the rounded image of the fp64 value and does not flip at rounding boundaries.
// Sums over rows follow the library's rule (common.h, "deterministic sums"): a row stores its loss and its fp32 gradient in
// its own slot of the caller's workspace; classify_finish_kernel and vs_reduce_parts add the slots in a fixed order.
//
// MIX (include/vitssl_mixup.h, vitssl_classify_loss_mix): the same kernels against the two-label target of a mixed image.  A
// row whose two labels coincide, or whose weight is 0 or 1, runs the one-label statements below unchanged; a genuine
// two-label row keeps the second label's term apart as well.  The one-label instantiation contains none of it.
//
// BCE (include/vitssl_bce.h, vitssl_classify_bce): binary cross-entropy on the same rows, labels and tables -- a kernel of its own
// (classify_bce_kernel, one pass over the row) that shares row_state, the argmax order, the workspace slots and the finish kernel.
#include "../../include/vitssl_classify.h"
#include "../../include/vitssl_mixup.h"
#include "../../include/vitssl_bce.h"
#include "common.h"
#include <math.h>

namespace {

constexpr int CL_THREADS = 256;
constexpr int CL_WAVES = CL_THREADS / 64;
constexpr int CL_CHUNK = 256;                 // columns a wave covers per step: 64 lanes x 4
constexpr int CL_NV = 4;                      // chunks a wave keeps in registers: rows of up to 1024 classes
constexpr int CL_MAX_C = 65536;
constexpr int CL_MAX_B = 1 << 22;

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// argmax order: NaN above everything, then the value, then the LOWER index (total, so every lane ends with the same answer)
__device__ __forceinline__ bool arg_better(float v, int i, float bv, int bi) {
  const bool vn = v != v, bn = bv != bv;
  if (vn != bn) return vn;
  if (!vn && v != bv) return v > bv;
  return i < bi;
}

struct ClArgs {
  const float* logits;
  const long long* labels;
  const int* partner;        // MIX: [B]
  const float* lam;          // MIX: [B]
  double* row_loss;          // workspace: [B]
  float* parts;              // workspace: [B, cp] fp32 gradient rows (read by the bias-gradient sum), or nullptr
  bf16_t* dlogits;           // or nullptr
  long long* pred;
  long long ignore_index;
  double eps, upstream;
  int B, C, ld, ld_out, cp;
};

__device__ __forceinline__ bool label_valid(long long l, long long ignore_index, int C) { return l != ignore_index && l >= 0 && l < C; }

// what a row contributes: ROW_VALID, ROW_IGNORED (nothing), ROW_BAD (nothing, and counted in bad_labels).  MIX: la / lb / lm
// are the row's two labels and its weight; nothing is read through a partner outside [0, B)
enum { ROW_VALID = 0, ROW_IGNORED = 1, ROW_BAD = 2 };
template <bool MIX>
__device__ __forceinline__ int row_state(const long long* labels, const int* partner, const float* lam, int i, int B, int C,
                                         long long ignore_index, long long& la, long long& lb, float& lm) {
  la = lb = labels[i];
  lm = 1.f;
  if constexpr (!MIX) {
    return label_valid(la, ignore_index, C) ? ROW_VALID : la == ignore_index ? ROW_IGNORED : ROW_BAD;
  } else {
    const int p = partner[i];
    lm = lam[i];
    const bool pok = p >= 0 && p < B;
    if (pok) lb = labels[p];
    const bool bad = !pok || !(lm >= 0.f && lm <= 1.f) || (la != ignore_index && (la < 0 || la >= C)) ||
                     (lb != ignore_index && (lb < 0 || lb >= C));
    return bad ? ROW_BAD : (la == ignore_index || lb == ignore_index) ? ROW_IGNORED : ROW_VALID;
  }
}

// REG: the row's chunks (C <= CL_NV * CL_CHUNK) stay in registers between the passes; otherwise every pass re-reads the row
template <bool REG, bool MIX>
__global__ __launch_bounds__(CL_THREADS) void classify_rows_kernel(ClArgs a) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * CL_WAVES + (threadIdx.x >> 6);
  if (row >= a.B) return;                                        // (no barrier below: waves are independent)
  const int C = a.C;
  // n_valid: every wave counts the B labels itself (B / 64 coalesced reads), so the gradient's 1 / n_valid needs neither a
  // launch of its own nor a host read
  int nv = 0;
  bool valid;
  int y, y2 = -1;                                                // y2: the second label of a two-label row (MIX), else no column
  double wa = 1.0, wb = 0.0;                                     // their weights
  if constexpr (!MIX) {
    for (int i = lane; i < a.B; i += 64) nv += label_valid(a.labels[i], a.ignore_index, C) ? 1 : 0;
    nv = wave_sum_i(nv);
    const long long lab = a.labels[row];
    valid = label_valid(lab, a.ignore_index, C);
    y = valid ? (int)lab : -1;                                   // -1 matches no column: nothing is indexed by a bad label
  } else {
    long long la, lb;
    float lm;
    for (int i = lane; i < a.B; i += 64) nv += row_state<true>(a.labels, a.partner, a.lam, i, a.B, C, a.ignore_index, la, lb, lm) == ROW_VALID ? 1 : 0;
    nv = wave_sum_i(nv);
    valid = row_state<true>(a.labels, a.partner, a.lam, row, a.B, C, a.ignore_index, la, lb, lm) == ROW_VALID;
    y = -1;
    if (valid) {
      if (la == lb || lm == 1.f) y = (int)la;                    // one-label rows: the statements of the one-label kernel
      else if (lm == 0.f) y = (int)lb;
      else y = (int)la, y2 = (int)lb, wa = (double)lm, wb = 1.0 - (double)lm;
    }
  }
  const bool two = MIX && y2 >= 0;                               // wave-uniform
  const float* zr = a.logits + (long long)row * a.ld;
  const int nk = (C + CL_CHUNK - 1) / CL_CHUNK;

  f32x4 zc[REG ? CL_NV : 1];
  double ec[REG ? CL_NV : 1][4];
  // f(k): chunk k holds a column < C (wave-uniform)
  auto chunks = [&](auto&& f) {
    if constexpr (REG) {
      static_for<CL_NV>([&](auto K) {
        if (K.value < nk) f(K);
      });
    } else {
      for (int k = 0; k < nk; ++k) f(k);
    }
  };
  auto load = [&](auto k) -> f32x4 {
    const int col = (int)k * CL_CHUNK + lane * 4;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (col < C) v = *(const f32x4*)(zr + col);                  // ld % 4 == 0 and col < C <= ld: the 16 bytes lie in the row
    return v;
  };

  // pass 1: max, argmax, sum of the logits
  float m = -INFINITY, bv = -INFINITY;
  int bi = INT_MAX;
  double zs = 0.0;
  chunks([&](auto k) {
    const f32x4 v = load(k);
    if constexpr (REG) zc[(int)k] = v;
    const int col = (int)k * CL_CHUNK + lane * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (col + e < C) {
        m = fmaxf(m, v[e]);
        zs += (double)v[e];
        if (arg_better(v[e], col + e, bv, bi)) bv = v[e], bi = col + e;
      }
  });
  m = wave_max(m);
  zs = wave_sum_d(zs);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (arg_better(ov, oi, bv, bi)) bv = ov, bi = oi;
  }

  // pass 2: exp(z - max); the label's term apart, so that 1 - p[y] is a sum and not a difference
  const double md = (double)m;
  double so = 0.0, ey = 0.0, zy = 0.0, e2 = 0.0, z2 = 0.0;
  chunks([&](auto k) {
    f32x4 v;
    if constexpr (REG) v = zc[(int)k]; else v = load(k);
    const int col = (int)k * CL_CHUNK + lane * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      double x = 0.0;
      if (col + e < C) {
        x = exp((double)v[e] - md);
        if constexpr (MIX) {
          if (col + e == y) ey = x, zy = (double)v[e]; else if (col + e == y2) e2 = x, z2 = (double)v[e]; else so += x;
        } else {
          if (col + e == y) ey = x, zy = (double)v[e]; else so += x;
        }
      }
      if constexpr (REG) ec[(int)k][e] = x;
    }
  });
  so = wave_sum_d(so);
  ey = wave_sum_d(ey);
  zy = wave_sum_d(zy);
  double s = so + ey;
  if (two) {
    e2 = wave_sum_d(e2);
    z2 = wave_sum_d(z2);
    s += e2;
  }
  if (lane == 0) {
    double loss = 0.0;
    if (two) {
      const double ls = log(s);
      loss = (1.0 - a.eps) * (wa * ((md - zy) + ls) + wb * ((md - z2) + ls));
      if (a.eps > 0.0) loss += a.eps * ((md + ls) - zs / (double)C);
    } else if (valid) {
      const double ls = ey == 1.0 ? log1p(so) : log(s);         // the label is the row's maximum: s = 1 + so
      loss = (1.0 - a.eps) * ((md - zy) + ls);
      if (a.eps > 0.0) loss += a.eps * ((md + log(s)) - zs / (double)C);
    }
    a.row_loss[row] = loss;
    a.pred[row] = bi;
  }
  if (!a.dlogits && !a.parts) return;

  // pass 3: the gradient, to the bf16 operand (every column below ld_out) and to the row's slot of the bias-gradient sum
  const double scale = a.upstream / (double)nv, inv_s = 1.0 / s, sm = a.eps / (double)C;
  double gy = (a.eps * (1.0 - 1.0 / (double)C) - so * inv_s) * scale;             // p[y] - (1 - eps) - eps / C
  double gy2 = 0.0;
  if (two) {                                                     // p[a] - wa (1 - eps) - eps / C, and the same for b
    gy = ((wb * (1.0 - a.eps) + a.eps * (1.0 - 1.0 / (double)C)) - (so + e2) * inv_s) * scale;
    gy2 = ((wa * (1.0 - a.eps) + a.eps * (1.0 - 1.0 / (double)C)) - (so + ey) * inv_s) * scale;
  }
  bf16_t* dr = a.dlogits ? a.dlogits + (long long)row * a.ld_out : nullptr;
  float* pr = a.parts ? a.parts + (long long)row * a.cp : nullptr;
  chunks([&](auto k) {
    const int col = (int)k * CL_CHUNK + lane * 4;
    if (col >= C) return;
    f32x4 g = {0.f, 0.f, 0.f, 0.f};
    if (valid) {
      f32x4 v;
      if constexpr (!REG) v = load(k);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (col + e < C) {
          double x;
          if constexpr (REG) x = ec[(int)k][e]; else x = exp((double)v[e] - md);
          if constexpr (MIX)
            g[e] = (float)(col + e == y ? gy : col + e == y2 ? gy2 : (x * inv_s - sm) * scale);
          else
            g[e] = (float)(col + e == y ? gy : (x * inv_s - sm) * scale);
        }
    }
    if (dr) {                                                    // col < C <= ld_out and ld_out % 4 == 0
      const u32x2 w = {pack_bf2(g[0], g[1]), pack_bf2(g[2], g[3])};
      *(u32x2*)(dr + col) = w;
    }
    if (pr) *(f32x4*)(pr + col) = g;                             // cp = C rounded up to 4
  });
  if (dr) {                                                      // the zero padding: columns cp .. ld_out-1 (both multiples of 4)
    const u32x2 z = {0u, 0u};
    for (int col = a.cp + lane * 4; col < a.ld_out; col += CL_CHUNK) *(u32x2*)(dr + col) = z;
  }
}

// one workgroup: loss_out = {sum of the row losses in a fixed order, n_valid}; counters and bad_labels accumulated
template <bool MIX>
__global__ __launch_bounds__(CL_THREADS) void classify_finish_kernel(const double* __restrict__ row_loss, const long long* __restrict__ labels,
                                                                     const int* __restrict__ partner, const float* __restrict__ lam,
                                                                     const long long* __restrict__ pred, long long ignore_index, int B, int C,
                                                                     float* __restrict__ loss_out, long long* __restrict__ counters,
                                                                     int* __restrict__ bad_labels) {
  __shared__ double red[CL_WAVES];
  __shared__ int cnt[CL_WAVES][3];
  const int tid = threadIdx.x;
  double sum = 0.0;
  int nvalid = 0, ncorrect = 0, nbad = 0;
  for (int i = tid; i < B; i += CL_THREADS) {
    long long l, lb;
    float lm;
    const int st = row_state<MIX>(labels, partner, lam, i, B, C, ignore_index, l, lb, lm);
    if (st == ROW_VALID) {
      sum += row_loss[i];
      ++nvalid;
      ncorrect += pred[i] == l ? 1 : 0;                          // MIX: the row's own label
    } else if (st == ROW_BAD) {
      ++nbad;
    }
  }
  sum = wave_sum_d(sum);
  nvalid = wave_sum_i(nvalid);
  ncorrect = wave_sum_i(ncorrect);
  nbad = wave_sum_i(nbad);
  if ((tid & 63) == 0) {
    red[tid >> 6] = sum;
    cnt[tid >> 6][0] = nvalid;
    cnt[tid >> 6][1] = ncorrect;
    cnt[tid >> 6][2] = nbad;
  }
  __syncthreads();
  if (tid == 0) {
    const int v = cnt[0][0] + cnt[1][0] + cnt[2][0] + cnt[3][0];
    loss_out[0] = (float)(((red[0] + red[1]) + red[2]) + red[3]);
    loss_out[1] = (float)v;
    counters[0] += cnt[0][1] + cnt[1][1] + cnt[2][1] + cnt[3][1];
    counters[1] += v;
    bad_labels[0] += cnt[0][2] + cnt[1][2] + cnt[2][2] + cnt[3][2];
  }
}

// BCE (include/vitssl_bce.h, vitssl_classify_bce): a sigmoid per class against the label-smoothed (MIX: two-label) target,
// optionally thresholded to {0, 1}.  Neither the loss nor the gradient of an element needs a sum over the row, so a row of any
// length is ONE pass: a chunk is read once, and its argmax candidates, its loss terms and its gradient leave with it.
struct BceArgs {
  ClArgs c;                  // eps: the smoothing
  double thr;                // < 0: the soft target as it is
  double div;                // what a row's sum over the classes is divided by: C, or 1 (sum_classes)
};

__device__ __forceinline__ double bce_target(double t, double thr) { return thr >= 0.0 ? (t > thr ? 1.0 : 0.0) : t; }

// One element: its loss max(z, 0) - z t + log1p(exp(-|z|)) is returned, d = sigmoid(z) - t.  One exponential and one division
// serve all of it: with ex = exp(-|z|) in [0, 1] and q = 1 / ((1 + ex)(2 + ex)),
//   sigmoid(|z|) = (2 + ex) q,  sigmoid(-|z|) = ex sigmoid(|z|)                  (no cancellation in either tail)
//   log1p(ex) = 2 atanh(u),  u = ex / (2 + ex) = ex (1 + ex) q <= 1/3:  2 u (1 + u^2/3 + u^4/5 + ... + u^34/35); the terms
//   left out sum to less than (1/9)^18 / 37 / (1 - 1/9) = 2e-19 of the bracket, below half an ulp of an fp64 number
// (the library's log1p spends about 80 fp64 additions an element on a range this argument never has).  Where t == 1 exactly
// sigmoid(z) - 1 is formed as -sigmoid(-z).  Branch-free, so that the four elements of a piece interleave.
__device__ __forceinline__ double bce_element(float zf, double t, double& d) {
  const double z = (double)zf, ex = exp(-fabs(z)), w = 1.0 + ex, v = 2.0 + ex;
  const double q = 1.0 / (w * v), r = v * q, er = ex * r, u = (ex * w) * q, u2 = u * u;
  double p = 1.0 / 35.0;
#pragma unroll
  for (int k = 33; k >= 1; k -= 2) p = fma(p, u2, 1.0 / (double)k);
  const bool pos = z >= 0.0;
  d = t == 1.0 ? -(pos ? er : r) : (pos ? r : er) - t;
  return (fmax(z, 0.0) - z * t) + 2.0 * u * p;
}

template <bool MIX>
__global__ __launch_bounds__(CL_THREADS) void classify_bce_kernel(BceArgs b) {
  const ClArgs& a = b.c;
  const int lane = threadIdx.x & 63;
  // (readfirstlane: the row is wave-uniform and the compiler is told so -- the row's state, labels and targets then live in
  // scalar registers and `valid` is a scalar branch around the arithmetic, not an execution mask inside it)
  const int row = __builtin_amdgcn_readfirstlane(blockIdx.x * CL_WAVES + (threadIdx.x >> 6));
  if (row >= a.B) return;                                        // (no barrier below: waves are independent)
  const int C = a.C;
  long long la, lb;
  float lm;
  int nv = 0;                                                    // n_valid, counted by every wave as in classify_rows_kernel
  for (int i = lane; i < a.B; i += 64) nv += row_state<MIX>(a.labels, a.partner, a.lam, i, a.B, C, a.ignore_index, la, lb, lm) == ROW_VALID ? 1 : 0;
  nv = wave_sum_i(nv);
  const bool valid = row_state<MIX>(a.labels, a.partner, a.lam, row, a.B, C, a.ignore_index, la, lb, lm) == ROW_VALID;
  // the targets of the row's (up to) three kinds of column: s(y)[y] = on, s(y)[c != y] = off
  const double off = a.eps / (double)C, on = (1.0 - a.eps) + off;
  int y = -1, y2 = -1;                                           // -1 matches no column: nothing is indexed by a bad label
  double ty = on, ty2 = off;
  if (valid) {
    y = (int)la;                                                 // one-label rows: a == b, l == 1 ...
    if constexpr (MIX) {
      if (la != lb && lm != 1.f) {
        if (lm == 0.f) {
          y = (int)lb;                                           // ... or l == 0
        } else {
          const double wa = (double)lm, wb = 1.0 - (double)lm;
          y2 = (int)lb, ty = wa * on + wb * off, ty2 = wa * off + wb * on;
        }
      }
    }
  }
  ty = bce_target(ty, b.thr), ty2 = bce_target(ty2, b.thr);
  const double to = bce_target(off, b.thr);
  const float* zr = a.logits + (long long)row * a.ld;
  const double scale = a.upstream / ((double)nv * b.div);
  bf16_t* dr = a.dlogits ? a.dlogits + (long long)row * a.ld_out : nullptr;
  float* pr = a.parts ? a.parts + (long long)row * a.cp : nullptr;

  float bv = -INFINITY;
  int bi = INT_MAX;
  double ls = 0.0;
  for (int col = lane * 4; col < C; col += CL_CHUNK) {
    const f32x4 v = *(const f32x4*)(zr + col);                   // ld % 4 == 0 and col < C <= ld: the 16 bytes lie in the row
    f32x4 g = {0.f, 0.f, 0.f, 0.f};
    const int n = min(C - col, 4);                               // 4 everywhere but in the row's last piece
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < n && arg_better(v[e], col + e, bv, bi)) bv = v[e], bi = col + e;
    if (valid) {
      double d[4], l[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) l[e] = bce_element(v[e], MIX && col + e == y2 ? ty2 : col + e == y ? ty : to, d[e]);
#pragma unroll
      for (int e = 0; e < 4; ++e)                                // (a column >= C holds anything, NaN included: computed, never used)
        if (e < n) ls += l[e], g[e] = (float)(d[e] * scale);
    }
    if (dr) {                                                    // col < C <= ld_out and ld_out % 4 == 0
      const u32x2 w = {pack_bf2(g[0], g[1]), pack_bf2(g[2], g[3])};
      *(u32x2*)(dr + col) = w;
    }
    if (pr) *(f32x4*)(pr + col) = g;                             // cp = C rounded up to 4
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (arg_better(ov, oi, bv, bi)) bv = ov, bi = oi;
  }
  ls = wave_sum_d(ls);
  if (lane == 0) {
    a.row_loss[row] = ls / b.div;
    a.pred[row] = bi;
  }
  if (dr) {                                                      // the zero padding: columns cp .. ld_out-1 (both multiples of 4)
    const u32x2 z = {0u, 0u};
    for (int col = a.cp + lane * 4; col < a.ld_out; col += CL_CHUNK) *(u32x2*)(dr + col) = z;
  }
}

inline long long cl_cp(int C) { return ((long long)C + 3) / 4 * 4; }
inline long long cl_loss_floats(int B) { return ((long long)2 * B + 3) / 4 * 4; }   // B doubles, the gradient rows behind them 16-byte aligned

}  // namespace

extern "C" int64_t vitssl_classify_loss_workspace_floats(int B, int C) {
  if (B < 1 || B > CL_MAX_B || C < 2 || C > CL_MAX_C) return 0;
  return cl_loss_floats(B) + (long long)B * cl_cp(C);
}

// every entry point: `who` names the caller in the messages; partner == nullptr is the one-label loss; bce: the sigmoid loss
// of include/vitssl_bce.h with its threshold and its sum_classes flag (nullptr: cross-entropy)
struct BceSpec {
  double thr;
  int sum_classes;
};
static int classify_launch(const char* who, const char* sizing, const float* logits, const int64_t* labels, const int32_t* partner, const float* lam,
                           int B, int C, int ld, double label_smoothing, int64_t ignore_index, float upstream, float* loss_out,
                           void* dlogits_bf16, int ld_out, float* dbias, int64_t* pred, int64_t* counters, int32_t* bad_labels,
                           float* workspace, int64_t workspace_floats, void* stream, const BceSpec* bce = nullptr) {
  VS_CHECK_ARG(logits && labels && loss_out && pred && counters && bad_labels, "%s: null pointer", who);
  VS_CHECK_ARG(B >= 1 && B <= CL_MAX_B, "%s: B = %d rows is outside 1 <= B <= 2^22", who, B);
  VS_CHECK_ARG(C >= 2 && C <= CL_MAX_C, "%s: C = %d classes is outside 2 <= C <= 65536", who, C);
  VS_CHECK_ARG(ld >= C && ld % 4 == 0, "%s: C = %d classes need a row length ld >= C that is a multiple of 4, got ld = %d", who, C, ld);
  VS_CHECK_ARG(label_smoothing >= 0.0 && label_smoothing <= 1.0, "%s: label_smoothing = %g is outside 0 <= eps <= 1", who, label_smoothing);
  if (dlogits_bf16)
    VS_CHECK_ARG(ld_out >= C && ld_out % 64 == 0, "%s: dlogits needs a row length ld_out >= C = %d that is a multiple of 64, got ld_out = %d", who,
                 C, ld_out);
  VS_CHECK_ARG((((uintptr_t)logits | (uintptr_t)dlogits_bf16 | (uintptr_t)workspace) & 15) == 0,
               "%s: logits, dlogits and workspace must be 16-byte aligned", who);
  VS_CHECK_ARG((((uintptr_t)labels | (uintptr_t)pred | (uintptr_t)counters) & 7) == 0, "%s: labels, pred and counters must be 8-byte aligned", who);
  VS_CHECK_ARG((((uintptr_t)partner | (uintptr_t)lam) & 3) == 0, "%s: partner and lam must be 4-byte aligned", who);
  if (!vs_parts(workspace, workspace_floats, vitssl_classify_loss_workspace_floats(B, C), who, sizing)) return VITSSL_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  ClArgs a;
  a.logits = logits;
  a.labels = (const long long*)labels;
  a.partner = partner;
  a.lam = lam;
  a.row_loss = (double*)workspace;
  a.parts = dbias ? workspace + cl_loss_floats(B) : nullptr;
  a.dlogits = (bf16_t*)dlogits_bf16;
  a.pred = (long long*)pred;
  a.ignore_index = ignore_index;
  a.eps = label_smoothing;
  a.upstream = (double)upstream;
  a.B = B, a.C = C, a.ld = ld, a.ld_out = ld_out, a.cp = (int)cl_cp(C);
  const dim3 grid((unsigned)((B + CL_WAVES - 1) / CL_WAVES)), block(CL_THREADS);
  const bool reg = C <= CL_NV * CL_CHUNK;
  if (bce) {
    BceArgs b;
    b.c = a;
    b.thr = bce->thr;
    b.div = bce->sum_classes ? 1.0 : (double)C;
    if (!partner)
      hipLaunchKernelGGL(classify_bce_kernel<false>, grid, block, 0, s, b);
    else
      hipLaunchKernelGGL(classify_bce_kernel<true>, grid, block, 0, s, b);
  } else if (!partner) {
    if (reg)
      hipLaunchKernelGGL((classify_rows_kernel<true, false>), grid, block, 0, s, a);
    else
      hipLaunchKernelGGL((classify_rows_kernel<false, false>), grid, block, 0, s, a);
  } else {
    if (reg)
      hipLaunchKernelGGL((classify_rows_kernel<true, true>), grid, block, 0, s, a);
    else
      hipLaunchKernelGGL((classify_rows_kernel<false, true>), grid, block, 0, s, a);
  }
  VS_CHECK_LAUNCH(who);
  if (!partner)
    hipLaunchKernelGGL(classify_finish_kernel<false>, dim3(1), block, 0, s, (const double*)a.row_loss, a.labels, a.partner, a.lam,
                       (const long long*)a.pred, (long long)ignore_index, B, C, loss_out, (long long*)counters, bad_labels);
  else
    hipLaunchKernelGGL(classify_finish_kernel<true>, dim3(1), block, 0, s, (const double*)a.row_loss, a.labels, a.partner, a.lam,
                       (const long long*)a.pred, (long long)ignore_index, B, C, loss_out, (long long*)counters, bad_labels);
  VS_CHECK_LAUNCH(who);
  if (dbias) return vs_reduce_parts(dbias, a.parts, B, C, a.cp, s);
  return VITSSL_OK;
}

extern "C" int vitssl_classify_loss(const float* logits, const int64_t* labels, int B, int C, int ld, double label_smoothing,
                                    int64_t ignore_index, float upstream, float* loss_out, void* dlogits_bf16, int ld_out,
                                    float* dbias, int64_t* pred, int64_t* counters, int32_t* bad_labels, float* workspace,
                                    int64_t workspace_floats, void* stream) {
  return classify_launch("classify_loss", "vitssl_classify_loss_workspace_floats", logits, labels, nullptr, nullptr, B, C, ld, label_smoothing,
                         ignore_index, upstream, loss_out, dlogits_bf16, ld_out, dbias, pred, counters, bad_labels, workspace, workspace_floats,
                         stream);
}

extern "C" int64_t vitssl_classify_loss_mix_workspace_floats(int B, int C) { return vitssl_classify_loss_workspace_floats(B, C); }

extern "C" int vitssl_classify_loss_mix(const float* logits, const int64_t* labels, const int32_t* partner, const float* lam, int B, int C,
                                        int ld, double label_smoothing, int64_t ignore_index, float upstream, float* loss_out,
                                        void* dlogits_bf16, int ld_out, float* dbias, int64_t* pred, int64_t* counters,
                                        int32_t* bad_labels, float* workspace, int64_t workspace_floats, void* stream) {
  VS_CHECK_ARG(partner && lam, "classify_loss_mix: null pointer");
  return classify_launch("classify_loss_mix", "vitssl_classify_loss_mix_workspace_floats", logits, labels, partner, lam, B, C, ld,
                         label_smoothing, ignore_index, upstream, loss_out, dlogits_bf16, ld_out, dbias, pred, counters, bad_labels, workspace,
                         workspace_floats, stream);
}

extern "C" int64_t vitssl_classify_bce_workspace_floats(int B, int C) { return vitssl_classify_loss_workspace_floats(B, C); }

extern "C" int vitssl_classify_bce(const float* logits, const int64_t* labels, const int32_t* partner, const float* lam, int B, int C, int ld,
                                   double smoothing, double target_threshold, int sum_classes, int64_t ignore_index, float upstream,
                                   float* loss_out, void* dlogits_bf16, int ld_out, float* dbias, int64_t* pred, int64_t* counters,
                                   int32_t* bad_labels, float* workspace, int64_t workspace_floats, void* stream) {
  VS_CHECK_ARG((partner == nullptr) == (lam == nullptr), "classify_bce: partner and lam are either both NULL (one label) or both given");
  VS_CHECK_ARG(target_threshold == target_threshold, "classify_bce: target_threshold is NaN (a negative value means no threshold)");
  const BceSpec bce = {target_threshold, sum_classes != 0};
  return classify_launch("classify_bce", "vitssl_classify_bce_workspace_floats", logits, labels, partner, lam, B, C, ld, smoothing, ignore_index,
                         upstream, loss_out, dlogits_bf16, ld_out, dbias, pred, counters, bad_labels, workspace, workspace_floats, stream, &bce);
}
