// Mixup / CutMix on a rendered batch (gfx950): out[i] = x[i], a blend of x[i] and x[partner], or x[i] with a box of x[partner]
// pasted in, per row of a device-side table.  include/vitssl_mixup.h declares the entry point and its contract.
//
// Memory-bound: 8 bytes (copy, paste) or 12 bytes (blend) of traffic per element and no reuse.  An image is cut into tiles of
// MX_TILE consecutive pieces (a piece = 16 bytes when W % 4 == 0, else one float); a workgroup takes a tile, so the image, its
// table row and its partner are uniform over the workgroup and sit in scalar registers, and a capped grid strides over the
// tiles.  A paste lane finds its image row and column from the piece index with two integer divisions; replacing them by
// multiplications with prepared reciprocals gained under 1 % at (256, 3, 224, 224) and was left out.
// Nothing is read that is not used: a copy row never touches its partner, a paste row only inside its box, where x[i] is
// not read in turn.
#include "../../include/vitssl_mixup.h"
#include "common.h"

namespace {

constexpr int MX_THREADS = 256;
constexpr int MX_UNROLL = 4;                          // pieces a lane has in flight
constexpr int MX_TILE = MX_THREADS * MX_UNROLL;
constexpr int MX_MAX_GRID = 2048;                     // 256 CUs x 8 workgroups: the rest is the grid-stride loop
enum { MIX_COPY = 0, MIX_BLEND = 1, MIX_PASTE = 2 };

struct MixArgs {
  const float* x;
  float* out;
  const int* iparams;        // [B, 6]
  const float* lam;          // [B]
  long long tiles;           // B * tiles_per_image
  int tiles_per_image, pieces;   // pieces of one image: C*H*W / 4 (VEC) or C*H*W
  int B, H, W, chw;
};

__device__ __forceinline__ float blend(float l, float om, float a, float b) { return fmaf(l, a, __fmul_rn(om, b)); }

// VEC: W % 4 == 0, so every image row starts on a 16-byte boundary and a piece never crosses a row
template <bool VEC>
__global__ __launch_bounds__(MX_THREADS) void mix_batch_kernel(MixArgs a) {
  constexpr int PW = VEC ? 4 : 1;                     // floats a piece
  const int wp = a.W / PW;                            // pieces a row
  for (long long t = blockIdx.x; t < a.tiles; t += gridDim.x) {
    const int i = (int)(t / a.tiles_per_image);
    const int first = (int)(t - (long long)i * a.tiles_per_image) * MX_TILE;
    // the table row, made safe: an unknown kind copies, a partner outside the batch is the row itself, the box is clamped
    const int* ip = a.iparams + (long long)i * 6;
    int kind = ip[0], p = ip[1];
    if (kind != MIX_BLEND && kind != MIX_PASTE) kind = MIX_COPY;
    if (p < 0 || p >= a.B) p = i;
    const int y0 = max(ip[2], 0), y1 = min(ip[3], a.H), x0 = max(ip[4], 0), x1 = min(ip[5], a.W);
    const float l = kind == MIX_BLEND ? a.lam[i] : 1.f;
    const float om = 1.f - l;
    const float* xa = a.x + (long long)i * a.chw;
    const float* xb = a.x + (long long)p * a.chw;
    float* o = a.out + (long long)i * a.chw;
#pragma unroll
    for (int u = 0; u < MX_UNROLL; ++u) {
      const unsigned v = (unsigned)first + u * MX_THREADS + threadIdx.x;   // first < pieces < 2^31: no wrap in 32 unsigned bits
      if (v >= (unsigned)a.pieces) continue;
      const long long off = (long long)v * PW;                    // < C*H*W
      if (kind == MIX_COPY) {
        if constexpr (VEC) *(f32x4*)(o + off) = *(const f32x4*)(xa + off); else o[off] = xa[off];
        continue;
      }
      if (kind == MIX_BLEND) {
        if constexpr (VEC) {
          const f32x4 va = *(const f32x4*)(xa + off), vb = *(const f32x4*)(xb + off);
          f32x4 r;
#pragma unroll
          for (int e = 0; e < 4; ++e) r[e] = blend(l, om, va[e], vb[e]);
          *(f32x4*)(o + off) = r;
        } else {
          o[off] = blend(l, om, xa[off], xb[off]);
        }
        continue;
      }
      // paste: the piece's image row and first column
      const unsigned row = v / (unsigned)wp;
      const int xc = (int)(v - row * (unsigned)wp) * PW;
      const int y = (int)(row % (unsigned)a.H);
      const bool yin = y >= y0 && y < y1;
      if constexpr (VEC) {
        int nin = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) nin += (yin && xc + e >= x0 && xc + e < x1) ? 1 : 0;
        // one load with a per-lane source (a wave straddles the box in nearly every row of it: two masked loads would cost twice)
        f32x4 r = *(const f32x4*)((nin == 4 ? xb : xa) + off);
        if (nin != 0 && nin != 4) {                               // the box's left or right edge lies in the piece: r holds x[i]
          const f32x4 vb = *(const f32x4*)(xb + off);
#pragma unroll
          for (int e = 0; e < 4; ++e) r[e] = (xc + e >= x0 && xc + e < x1) ? vb[e] : r[e];
        }
        *(f32x4*)(o + off) = r;
      } else {
        o[off] = (yin && xc >= x0 && xc < x1) ? xb[off] : xa[off];
      }
    }
  }
}

}  // namespace

extern "C" int vitssl_mix_batch(const float* x, float* out, const int32_t* iparams, const float* lam, int B, int C, int H, int W,
                                void* stream) {
  VS_CHECK_ARG(x && out && iparams && lam, "mix_batch: null pointer");
  VS_CHECK_ARG(B >= 1 && C >= 1 && H >= 1 && W >= 1, "mix_batch: B = %d, C = %d, H = %d, W = %d must all be >= 1", B, C, H, W);
  const long long chw = (long long)C * H * W;
  VS_CHECK_ARG(chw < (1ll << 31), "mix_batch: C * H * W = %lld elements an image is outside C * H * W < 2^31", chw);
  VS_CHECK_ARG((((uintptr_t)x | (uintptr_t)out) & 15) == 0, "mix_batch: x and out must be 16-byte aligned");
  VS_CHECK_ARG((((uintptr_t)iparams | (uintptr_t)lam) & 3) == 0, "mix_batch: iparams and lam must be 4-byte aligned");
  const uintptr_t bytes = (uintptr_t)B * (uintptr_t)chw * 4u, xa = (uintptr_t)x, oa = (uintptr_t)out;
  VS_CHECK_ARG(xa + bytes <= oa || oa + bytes <= xa, "mix_batch: out overlaps x (rows read their partner rows: the mix cannot run in place)");
  const bool vec = W % 4 == 0;
  MixArgs a;
  a.x = x, a.out = out, a.iparams = iparams, a.lam = lam;
  a.pieces = (int)(vec ? chw / 4 : chw);
  a.tiles_per_image = (int)(((long long)a.pieces + MX_TILE - 1) / MX_TILE);
  a.tiles = (long long)B * a.tiles_per_image;
  a.B = B, a.H = H, a.W = W, a.chw = (int)chw;
  const dim3 grid((unsigned)(a.tiles < MX_MAX_GRID ? a.tiles : MX_MAX_GRID)), block(MX_THREADS);
  if (vec)
    hipLaunchKernelGGL(mix_batch_kernel<true>, grid, block, 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(mix_batch_kernel<false>, grid, block, 0, (hipStream_t)stream, a);
  VS_CHECK_LAUNCH("mix_batch");
  return VITSSL_OK;
}
