// Stochastic depth (drop path): the table of per-sample branch scales (gfx950).  include/vitssl_droppath.h declares the entry
// point and the semantics.  scale[j][b] = keep ? 1 / (1 - r_eff) : 0 with the keep bit of the dropout stream (common.h) for
// element b of a [1, B] tensor at (seed, site_j).  A few hundred floats per step: one small launch whose (rate, site) lists
// travel as kernel arguments, so nothing is copied to the device and nothing is read back.
#include "../../include/vitssl_droppath.h"
#include "common.h"

namespace {

constexpr int DP_THREADS = 256;

struct DropPathArgs {
  float* scale;                                   // [sites, B]
  unsigned long long seed;
  int sites, B;
  float rate[VITSSL_DROPPATH_MAX_SITES];
  unsigned site[VITSSL_DROPPATH_MAX_SITES];
};

__global__ __launch_bounds__(DP_THREADS) void droppath_table_kernel(DropPathArgs a) {
  const int j = blockIdx.y;                       // < sites (grid.y == sites)
  const int b = blockIdx.x * DP_THREADS + threadIdx.x;
  if (b >= a.B) return;
  vitssl_dropout_t d;
  d.p = a.rate[j];
  d.site = a.site[j];
  d.seed = a.seed;
  const DropKey k = make_drop_key(d);
  float s = 1.0f;
  if (k.thr != 0) {
    bool keep[4];
    drop_keep4(k, drop_words(k, (unsigned)b >> 2), keep);     // element b of the group b / 4
    const int e = b & 3;
    const bool kept = e == 0 ? keep[0] : e == 1 ? keep[1] : e == 2 ? keep[2] : keep[3];
    s = kept ? k.scale : 0.f;
  }
  a.scale[(long long)j * a.B + b] = s;
}

}  // namespace

extern "C" int vitssl_droppath_table(float* scale, const float* rates, const uint32_t* site_ids, int sites, int B, uint64_t seed,
                                     void* stream) {
  VS_CHECK_ARG(scale && rates && site_ids, "droppath_table: null pointer");
  VS_CHECK_ARG(sites >= 1 && sites <= VITSSL_DROPPATH_MAX_SITES, "droppath_table: sites = %d outside [1, %d]", sites,
               VITSSL_DROPPATH_MAX_SITES);
  VS_CHECK_ARG(B >= 1, "droppath_table: B = %d must be >= 1", B);
  DropPathArgs a;
  a.scale = scale;
  a.seed = seed;
  a.sites = sites;
  a.B = B;
  for (int j = 0; j < VITSSL_DROPPATH_MAX_SITES; ++j) {
    a.rate[j] = 0.f;
    a.site[j] = 0u;
  }
  for (int j = 0; j < sites; ++j) {
    VS_CHECK_ARG(rates[j] < 1.0f, "droppath_table: rate %g of entry %d must be < 1 (a rate of 0 or below keeps every sample)",
                 (double)rates[j], j);
    a.rate[j] = rates[j] > 0.f ? rates[j] : 0.f;
    a.site[j] = site_ids[j];
  }
  const dim3 grid((unsigned)((B + DP_THREADS - 1) / DP_THREADS), (unsigned)sites), block(DP_THREADS);
  hipLaunchKernelGGL(droppath_table_kernel, grid, block, 0, (hipStream_t)stream, a);
  VS_CHECK_LAUNCH("droppath_table");
  return VITSSL_OK;
}
