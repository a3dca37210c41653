// LayerScale (include/vitssl_layerscale.h): the kernels live where the residual adds and their backward live -- the EPI_RESID_LS
// epilogue of csrc/nt_epilogue.h and the LS instantiations of ln_bwd_kernel in csrc/layernorm.hip.  What stands alone is the sizing
// of the workspace of the two backward entry points, which keep four column sums where vitssl_layernorm_bwd keeps three.
#include "../../include/vitssl_layerscale.h"
#include "common.h"

// One slot row per workgroup and sum: at most min(ceil(rows / 4), 2 x CUs) workgroups (csrc/layernorm.hip, ln_grid: two per CU for
// rows of up to 512 columns, one above).  Never below vitssl_sum_workspace_floats, so one buffer serves both families.
extern "C" int64_t vitssl_layerscale_workspace_floats(int64_t rows, int cols) {
  if (rows <= 0 || cols <= 0) return 0;
  long long ln = (rows + 3) / 4;
  const long long cap = 2LL * vitssl_persistent_cus();
  if (ln > cap) ln = cap;
  const long long need = 4 * ln * (long long)cols;
  const long long base = vitssl_sum_workspace_floats(rows, cols);
  return need > base ? need : base;
}
