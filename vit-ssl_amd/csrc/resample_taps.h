// Pillow's 8-bit BILINEAR resampling taps (Resample.c: precompute_coeffs + normalize_coeffs_8bpc), shared by the DINO
// multi-crop kernels (augment.hip) and the fused transform-list kernel (transforms.hip) so that the two input pipelines
// cannot drift apart.  The arithmetic is double precision with every product and sum rounded separately: a file that
// includes this is compiled with -ffp-contract=off (__graft_entry__.py, PER_FILE_FLAGS).
#pragma once
#include "common.h"

constexpr int PRECISION_BITS = 32 - 8 - 2;   // Pillow Resample.c

__device__ __forceinline__ double bilinear_filter(double x) {
  x = x < 0.0 ? -x : x;
  return x < 1.0 ? 1.0 - x : 0.0;
}

// Taps of output position xx, evaluated on the fly (BILINEAR, support 1, widened by the scale when downscaling).  Returns
// the first source index; writes up to `cap` fixed-point taps to k[0], k[stride], ... and their number to *count.
__device__ __forceinline__ int resample_taps(int in_size, int out_size, int xx, int* k, int cap, int* count, int stride = 1) {
  const double scale = (double)in_size / (double)out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = filterscale;
  const double ss = 1.0 / filterscale;
  const double center = ((double)xx + 0.5) * scale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in_size) xmax = in_size;
  xmax -= xmin;
  if (xmax > cap) xmax = cap;          // cannot happen for cap >= 2*ceil(scale)+1 (checked on the host)
  double ww = 0.0;
  for (int x = 0; x < xmax; ++x) ww += bilinear_filter(((double)(x + xmin) - center + 0.5) * ss);
  for (int x = 0; x < xmax; ++x) {
    double w = bilinear_filter(((double)(x + xmin) - center + 0.5) * ss);
    if (ww != 0.0) w /= ww;
    k[x * stride] = w < 0.0 ? (int)(-0.5 + w * (double)(1 << PRECISION_BITS)) : (int)(0.5 + w * (double)(1 << PRECISION_BITS));
  }
  *count = xmax;
  return xmin;
}

__device__ __forceinline__ unsigned char clip8(int v) { return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v)); }
