// Which kernel, tile and K split an implicit-GEMM convolution runs on: the decision, and nothing else.  plan_conv is a pure function
// of its arguments (no HIP runtime call, no global read), so it can be asked without a GPU (rgbm_conv_plan in rgbm.h) and tested
// directly.  A launch asks it once: ConvLayer::run / run_then_1x1 (layers.cpp) gather the ConvTuning and call it, ConvLayer::launch binds what
// the plan needs on the device (K-split scratch, identity, border table) and launch_conv (conv_launch.cpp) launches what it says.
#pragma once
#include <vector>

#include "common.h"

namespace rgbm {

// everything outside the ConvDesc that the decision depends on
struct ConvTuning {
  int flags;               // rgbm_debug_flags word (DebugFlag, kernels.h)
  int gemm_kernel;         // rgbm_set_tuning "gemm_kernel"
  long long ws_min_rows;   // rgbm_set_tuning "ws_min_rows" (0 = the default)
  int n_cu;                // persistent_grid_cus()
};

// (the values are the kernel ids of rgbm_conv_plan, rgbm.h)
enum ConvKernel {
  CONV_GENERIC = 0,        // conv_igemm_glds_kernel, bch x bpix tile
  CONV_V3 = 1,             // conv_igemm_v3_kernel 128 x 256
  CONV_WS = 2,             // conv_igemm_ws_kernel 128 x 256
  CONV_WS_WIDE = 3,        // ... 256 x 128
  CONV_WS_SLIM = 4,        // ... 64 x 256, four multiply waves
  CONV_WS64 = 5,           // conv_igemm_ws64_kernel
  CONV_WS64_ROWHALO = 6,   // ... row-halo variant
  CONV_M32 = 7,            // conv_igemm_m32_kernel: main_rows on 256 x 256 tiles, the rest on tail_bch x 128 tiles
  CONV_M32_SMALL = 8,      // ... one launch of bch x 128 tiles that does not fill the grid, K loop cut into ksplit parts
};

struct ConvPlan {
  int kernel;              // ConvKernel
  int bch, bpix;           // tile (of the main launch for CONV_M32)
  bool uniform_taps;       // every K tile inside one tap (the UNI forms of the generic / v3 kernels)
  long long main_rows;     // CONV_M32: rows [0, main_rows) on 256 x 256 tiles
  int tail_bch;            // CONV_M32: channel tile of the 128-pixel launch of rows [main_rows, M) (0 = no tail)
  int ksplit;              // K parts the launch asks for (1 = none); ConvLayer::launch runs it unsplit where a capture finds the stream without scratch
  bool identity_residual;  // the m32 kernels add the residual through identity K steps (else in the epilogue)
  int korder, buf_ok;      // ConvDesc fields of the same names
  bool border;             // CONV_M32: the main launch's rows on class-pure 256 x 256 tiles from a row table (plan_border); ConvLayer::launch
                           // runs them row-major where a capture finds the layer without a table for this shape
};

// ---- border-class tiles of a dilated 2-D conv (CONV_M32, ConvPlan::border) ------------------------------------------------------------
// Output pixels whose set of in-range taps is the same form a border class (3 x 3, pad = dil: interior, four edges, four corners).  A
// tile is 256 rows of ONE class taken across views, so it walks only the class's taps: every K step of a tap that reads nothing but
// padding is gone, and every step that runs is the step the row-major tiles run.  The in-range taps of a class are a rectangle
// [kh0, kh1) x [kw0, kw1) of the kernel (in-range positions along an axis are an interval).
struct BorderClass {
  int kh0, kh1, kw0, kw1;  // in-range taps
  int mask;                // bit kh * KW + kw
  int n_pix;               // pixels of a view in this class
  int pix0;                // its first entry in BorderPlan::pix
  long long row0;          // its first table row; it owns its live rows rounded up to whole tiles, the last ones dead
};
struct BorderTile {
  int cls, ch;             // class, channel tile
  int mask;                // the class's tap mask
  int steps;               // K steps: popcount(mask) * Cin / BK, + the residual steps
  long long row0;          // first table row
};
struct BorderPlan {
  int n_wg, n_ch, kr, steps_per_tap;
  std::vector<BorderClass> classes;
  std::vector<int> pix;           // per class, the pixels h * Wq + w of a view in row-major order
  std::vector<BorderTile> tiles;  // class-major, rows ascending, channel tiles innermost
  std::vector<int> order;         // tile indices, workgroup-major: workgroup b runs order[wg_off[b] .. wg_off[b + 1]) in this order
  std::vector<int> wg_off;        // n_wg + 1
  std::vector<int> rows;          // table row -> GEMM row m = (view * Hq + h) * Wq + w < main_rows, -1 = dead
  long long total_steps, parent_steps, max_wg_steps;      // parent_steps: every 256-row tile of the row-major order walks every tap
};
// Whether the GEMM rows [0, main_rows) of d (the main launch of CONV_M32) run on border-class tiles: cheap (O(Hq + Wq)), called by
// plan_conv per launch.
bool border_applies(const ConvDesc& d, int dtype, int flags, long long main_rows);
// The whole table for n_wg workgroups.  false: declined (border_applies says no).  Pure: no HIP call, no global read.
bool plan_border(const ConvDesc& d, int dtype, int flags, long long main_rows, int n_wg, BorderPlan* out);

// K-split scratch of a stream: fp32 partial accumulators and arrival counters (ConvScratch, layers.h); a split that would not fit is not planned
constexpr size_t kM32SplitFloats = 8u << 20, kM32SplitCounters = 16384;

// 0, or -1 with the error set where no kernel takes d (a malformed descriptor)
int plan_conv(const ConvDesc& d, int dtype, const ConvTuning& t, ConvPlan* out);
// the process's current tuning (conv_launch.cpp); n_cu = 0: the current device's, else as given without a HIP runtime call
int conv_tuning(int n_cu, ConvTuning* t);

// One launcher per kernel family, each its own translation unit; launch_conv (conv_launch.cpp) picks by p.kernel:
//   CONV_GENERIC -> igemm_generic.hip        CONV_V3 -> igemm_generic.hip        CONV_WS / _WIDE / _SLIM -> igemm_ws.hip
//   CONV_WS64 / _ROWHALO -> igemm_ws64.hip   CONV_M32 / _SMALL -> igemm_m32.hip
int launch_igemm_generic(const ConvDesc& d, int dtype, const ConvPlan& p, hipStream_t s);
int launch_igemm_v3(const ConvDesc& d, int dtype, const ConvPlan& p, hipStream_t s);
int launch_igemm_ws(const ConvDesc& d, int dtype, const ConvPlan& p, hipStream_t s);
int launch_igemm_ws64(const ConvDesc& d, int dtype, const ConvPlan& p, hipStream_t s);
int launch_igemm_m32(const ConvDesc& d, int dtype, const ConvPlan& p, hipStream_t s);
int conv_no_kernel();      // -1 with the error set: the plan names a kernel the storage type does not have

}  // namespace rgbm
