// Host side of the implicit-GEMM launch: the process-wide settings the plan reads, and the switch from a ConvPlan to the
// kernel family that runs it (each family is one translation unit, igemm_*.hip).
#include "common.h"
#include "conv_plan.h"
#include "kernels.h"

namespace rgbm {

int g_debug_flags = 0;
long long g_ws_min_rows = 0;              // GEMM rows from which the persistent role-specialised implicit-GEMM kernels are used; 0 = per storage type (conv_plan.cpp: ws_min_rows), set by rgbm_set_tuning
int g_tuning_version = 0;                 // bumped by rgbm_debug_flags / rgbm_set_tuning: captured forward graphs of older settings are dropped
// kernel of the 256-channel x 128-pixel launches (layer3 / layer4 / up_1), rgbm_set_tuning("gemm_kernel"): 0 = conv_igemm_ws_kernel
// (16x16x32 MFMAs, 8 multiply waves, 256 x 128 tile), 1 = conv_igemm_m32_kernel<256 x 128>, 2 = conv_igemm_m32_kernel<256 x 256> (default)
int g_gemm_kernel = 2;

// process-wide settings of the decision (rgbm_debug_flags, rgbm_set_tuning) and the current device's persistent grid; n_cu > 0: plan for
// that many CUs instead (no HIP runtime call)
int conv_tuning(int n_cu, ConvTuning* t) {
  *t = ConvTuning{g_debug_flags, g_gemm_kernel, g_ws_min_rows, n_cu};
  return n_cu > 0 ? 0 : persistent_grid_cus(&t->n_cu);
}

int conv_no_kernel() { RGBM_REQUIRE(false, "conv plan names a kernel this storage type does not have"); }

int launch_conv(const ConvDesc& d, int dtype, const ConvPlan& p, hipStream_t s) {
  switch (p.kernel) {
    case CONV_GENERIC: return launch_igemm_generic(d, dtype, p, s);
    case CONV_V3: return launch_igemm_v3(d, dtype, p, s);
    case CONV_WS:
    case CONV_WS_WIDE:
    case CONV_WS_SLIM: return launch_igemm_ws(d, dtype, p, s);
    case CONV_WS64:
    case CONV_WS64_ROWHALO: return launch_igemm_ws64(d, dtype, p, s);
    case CONV_M32:
    case CONV_M32_SMALL: return launch_igemm_m32(d, dtype, p, s);
  }
  return conv_no_kernel();
}

}  // namespace rgbm
