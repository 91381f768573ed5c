// Float pixel -> 8-bit pixel, the one definition behind rgbm_quantize_frames (prepare.hip) and the 8-bit synthetic camera
// (synth_env.hip): q(x) = min(max(rint(x * 255), 0), 255) in float32 with rint = round half to even, NaN -> 0 (every comparison
// with NaN is false).  A single float32 product and a rounding: nothing a compiler could contract.
#pragma once
#include <hip/hip_runtime.h>

namespace rgbm {

__device__ inline unsigned quantize_px(float x) {
  const float r = rintf(x * 255.f);
  return r > 0.f ? (r < 255.f ? (unsigned)r : 255u) : 0u;
}

}  // namespace rgbm
