// SimMIM / supervised / finetune / eval transform lists on the GPU (gfx950): RandomResizedCrop -> RandomHorizontalFlip ->
// ToTensor and Resize -> ToTensor (utils/train_utils.py:54-68 with configs/*/train_transforms.yaml, val_transforms.yaml,
// configs/*_eval/transforms.yaml) as ONE launch.  include/vitssl_transforms.h declares the entry points.
//
// One workgroup renders `tr` output rows of one image:
//   0. the horizontal taps of all SW output columns and the vertical taps of its rows go to LDS (Pillow's fixed-point
//      taps, csrc/resample_taps.h: the code the DINO kernels use; double precision, so they are computed once per
//      workgroup, not once per source row as aug_resize_h_kernel does);
//   1. horizontal pass over the source rows its output rows need, rounded to uint8 INTO LDS, flipped on the way;
//   2. vertical pass out of LDS + /255, each lane storing 4 pixels of the three planes as 16-byte pieces: for a plane
//      the tile's rows are one contiguous run of tr * SW floats, so a wave's stores are whole lines.
// HBM sees the crop box once (rows shared by neighbouring tiles come from L2) and the fp32 output once; there is no
// uint8 intermediate in device memory.  Arithmetic as in augment.hip: no FMA contraction (-ffp-contract=off).
#include "../../include/vitssl_transforms.h"
#include "common.h"
#include "resample_taps.h"

namespace {

constexpr int TF_IP = 5;
constexpr int TF_THREADS = 256;
constexpr int TF_LDS_AIM = 32 * 1024;   // tiles are sized to this where they can be (>= 4 workgroups per CU) ...
constexpr int TF_LDS_MAX = 64 * 1024;   // ... and never above this (the default dynamic-LDS limit of a launch)
constexpr int TF_MAX_RATIO = 127;       // taps per output position 2 * ratio + 1 <= 255 (count packed in 8 bits)

struct TfPlan {
  int tr;         // output rows per workgroup
  int kh, kv;     // tap capacity per output column / row: 2 * ceil(ratio) + 1
  int cap_rows;   // source rows a tile can need
  int rowb;       // bytes of one LDS row: SW * 3 rounded up to 4
  long long lds;  // dynamic LDS the tile needs, in bytes (64-bit: a wide SW times tall taps passes 2^31 before it is refused)
};

// LDS image: int hmeta[SW] (first source column << 8 | taps), int hk[kh][SW], int vmeta[tr], int vk[tr][kv], u8 rows[cap_rows][rowb]
// A tile's rows span less than (tr - 1) * s + 2 * max(s, 1) + 1 source rows for the vertical scale s = h / SH <= H / SH
// (first row > centre_0 - support - 0.5, end <= centre_last + support + 0.5).
void tf_fill(TfPlan& p, int H, int SH, int SW, int tr) {
  const double smax = (double)H / (double)SH;
  p.tr = tr;
  p.cap_rows = (int)((double)(tr - 1) * smax + 2.0 * (smax < 1.0 ? 1.0 : smax) + 1.0) + 1;
  if (p.cap_rows > H) p.cap_rows = H;
  p.rowb = (SW * 3 + 3) & ~3;
  p.lds = ((long long)SW * (1 + p.kh) + (long long)tr * (1 + p.kv)) * (long long)sizeof(int) + (long long)p.cap_rows * p.rowb;
}

// false: the shape is refused (error set)
bool tf_plan(TfPlan& p, int H, int W, int SH, int SW, const char* who) {
  if (!(H > 0 && W > 0 && SH > 0 && SW > 0 && H < (1 << 23) && W < (1 << 23) && SH < (1 << 23) && SW < (1 << 23))) {
    vitssl_set_error("%s: bad shape %dx%d -> %dx%d (sizes must be in [1, 2^23))", who, H, W, SH, SW);
    return false;
  }
  const int rh = (W + SW - 1) / SW, rv = (H + SH - 1) / SH;
  if (rh > TF_MAX_RATIO || rv > TF_MAX_RATIO) {
    vitssl_set_error("%s: source %dx%d is more than %dx the output size %dx%d", who, H, W, TF_MAX_RATIO, SH, SW);
    return false;
  }
  p.kh = 2 * rh + 1;
  p.kv = 2 * rv + 1;
  int best = 0;
  for (int tr = 32; tr >= 1 && !best; tr >>= 1) {
    if (tr > 1 && tr >= 2 * SH) continue;          // no taller than the output needs
    tf_fill(p, H, SH, SW, tr);
    if (p.lds <= TF_LDS_AIM) best = tr;
  }
  for (int tr = 32; tr >= 1 && !best; tr >>= 1) {
    if (tr > 1 && tr >= 2 * SH) continue;
    tf_fill(p, H, SH, SW, tr);
    if (p.lds <= TF_LDS_MAX) best = tr;
  }
  if (!best) {
    tf_fill(p, H, SH, SW, 1);
    vitssl_set_error("%s: %dx%d -> %dx%d needs %lld bytes of LDS for the %d rows of %d pixels behind one output row and its tap "
                     "tables; the limit is %d", who, H, W, SH, SW, p.lds, p.cap_rows, SW, TF_LDS_MAX);
    return false;
  }
  tf_fill(p, H, SH, SW, best);
  return true;
}

// grid = B * tiles.  VEC = 4: SW % 4 == 0 and `out` 16-byte aligned; VEC = 1: anything
template <int VEC>
__global__ __launch_bounds__(TF_THREADS) void tf_resized_crop_tensor_kernel(const unsigned char* __restrict__ src, const int* __restrict__ ip,
                                                                          float* __restrict__ out, int H, int W, int SH, int SW,
                                                                          TfPlan p, int tiles) {
  extern __shared__ __attribute__((aligned(16))) int tf_lds[];
  int* hmeta = tf_lds;
  int* hk = hmeta + SW;
  int* vmeta = hk + p.kh * SW;
  int* vk = vmeta + p.tr;
  unsigned char* rows = (unsigned char*)(vk + p.tr * p.kv);
  const int b = blockIdx.x / tiles, y0 = (blockIdx.x - b * tiles) * p.tr;
  const int* q = ip + b * TF_IP;
  const int top = q[0], left = q[1], h = q[2], w = q[3], flip = q[4];
  const int nout = min(p.tr, SH - y0);
  const int rowb = p.rowb;

  // 0. taps: columns tap-major (lane xx reads hk[x][xx]: no bank conflicts), rows row-major (a row's taps are broadcast)
  for (int i = threadIdx.x; i < SW + nout; i += TF_THREADS) {
    int n;
    if (i < SW) {
      const int xmin = resample_taps(w, SW, i, hk + i, p.kh, &n, SW);
      hmeta[i] = (xmin << 8) | n;
    } else {
      const int r = i - SW;
      const int ymin = resample_taps(h, SH, y0 + r, vk + r * p.kv, p.kv, &n);
      vmeta[r] = (ymin << 8) | n;
    }
  }
  __syncthreads();
  const int row0 = vmeta[0] >> 8;                      // first source row (of the box) this tile reads; ymin grows with the row
  const int mlast = vmeta[nout - 1];
  const int nrows = min((mlast >> 8) + (mlast & 255) - row0, p.cap_rows);     // (the min only binds for a box outside the contract)

  // 1. horizontal pass, uint8 into LDS, flipped
  const unsigned char* sbase = src + (((long long)b * H + top + row0) * W + left) * 3;
  for (int i = threadIdx.x; i < nrows * SW; i += TF_THREADS) {
    const int r = i / SW, xx = i - r * SW;
    const int m = hmeta[xx], n = m & 255;
    const unsigned char* px = sbase + ((long long)r * W + (m >> 8)) * 3;
    int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
    for (int x = 0; x < n; ++x, px += 3) {
      const int k = hk[x * SW + xx];                   // < 2^23: a 24-bit multiply is exact
      s0 += __mul24(px[0], k);
      s1 += __mul24(px[1], k);
      s2 += __mul24(px[2], k);
    }
    unsigned char* o = rows + r * rowb + (flip ? SW - 1 - xx : xx) * 3;
    o[0] = clip8(s0 >> PRECISION_BITS);
    o[1] = clip8(s1 >> PRECISION_BITS);
    o[2] = clip8(s2 >> PRECISION_BITS);
  }
  __syncthreads();

  // 2. vertical pass + ToTensor: an item is VEC pixels x 3 channels = VEC * 3 bytes of every LDS row it needs
  const int qw = SW / VEC;
  for (int i = threadIdx.x; i < nout * qw; i += TF_THREADS) {
    const int r = i / qw, xq = i - r * qw;
    const int m = vmeta[r];
    const int ymin = (m >> 8) - row0;
    const int n = min(m & 255, nrows - ymin);
    const unsigned char* col = rows + ymin * rowb + xq * (VEC * 3);
    const int* kr = vk + r * p.kv;
    int s[VEC * 3];
#pragma unroll
    for (int e = 0; e < VEC * 3; ++e) s[e] = 1 << (PRECISION_BITS - 1);
    for (int y = 0; y < n; ++y, col += rowb) {
      const int k = kr[y];
      if constexpr (VEC == 4) {
        const unsigned* c4 = (const unsigned*)col;     // 12-byte items in 4-byte-multiple rows: aligned
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          const unsigned v = c4[d];
#pragma unroll
          for (int e = 0; e < 4; ++e) s[d * 4 + e] += __mul24((int)((v >> (8 * e)) & 255u), k);
        }
      } else {
#pragma unroll
        for (int e = 0; e < 3; ++e) s[e] += __mul24(col[e], k);
      }
    }
    float* o = out + (((long long)b * 3) * SH + y0 + r) * SW + xq * VEC;
    const long long plane = (long long)SH * SW;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if constexpr (VEC == 4) {
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (float)clip8(s[e * 3 + c] >> PRECISION_BITS) / 255.0f;
        *(f32x4*)(o + c * plane) = v;
      } else {
        o[c * plane] = (float)clip8(s[c] >> PRECISION_BITS) / 255.0f;
      }
    }
  }
}

}  // namespace

extern "C" int vitssl_debug_tf_tile_rows(int H, int W, int SH, int SW) {
  TfPlan p;
  if (!tf_plan(p, H, W, SH, SW, "debug_tf_tile_rows")) return VITSSL_ERR_ARG;
  return p.tr;
}

extern "C" int vitssl_tf_resized_crop_to_tensor(const uint8_t* src, const int32_t* iparams, float* out, int B, int H, int W, int SH,
                                                int SW, void* stream) {
  VS_CHECK_ARG(src && iparams && out, "tf_resized_crop_to_tensor: null pointer");
  VS_CHECK_ARG(B > 0, "tf_resized_crop_to_tensor: empty batch (B = %d)", B);
  TfPlan p;
  if (!tf_plan(p, H, W, SH, SW, "tf_resized_crop_to_tensor")) return VITSSL_ERR_ARG;
  const int tiles = (SH + p.tr - 1) / p.tr;
  VS_CHECK_ARG((long long)B * tiles <= INT_MAX, "tf_resized_crop_to_tensor: %d images x %d tiles exceed the grid limit", B, tiles);
  const dim3 grid((unsigned)(B * tiles)), block(TF_THREADS);
  if (SW % 4 == 0 && ((uintptr_t)out & 15) == 0)
    hipLaunchKernelGGL(tf_resized_crop_tensor_kernel<4>, grid, block, (size_t)p.lds, (hipStream_t)stream, src, iparams, out, H, W, SH, SW, p, tiles);
  else
    hipLaunchKernelGGL(tf_resized_crop_tensor_kernel<1>, grid, block, (size_t)p.lds, (hipStream_t)stream, src, iparams, out, H, W, SH, SW, p, tiles);
  VS_CHECK_LAUNCH("tf_resized_crop_to_tensor");
  return VITSSL_OK;
}
