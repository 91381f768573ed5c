// Device functions of the plane-sweep warp (network_v5.py:378-430, network_v2.py:104-142), shared by the kernels that must agree on a
// voxel bit for bit: build_volume_kernel (misc_kernels.hip) and v2_point_rows_kernel (v2_head.hip).  Both files are built with
// -ffp-contract=off (build.sh), so the expressions below round the same way in both.
#pragma once
#include "common.h"

namespace rgbm {

// vol[v,d,y,x,:] = feat[v,y,x,:] + grid_sample(feat[partner(v)], homography(v,d,y,x))   (bilinear, zeros,
// align_corners=False fed with the align_corners=True normalisation, exactly as the reference does).
__device__ __forceinline__ void warp_coords(const float* __restrict__ hm, float x, float y, float depth, int H, int W,
                                            float& ix, float& iy) {
  // rot_xyz = rot @ [x,y,1]; * depth; + trans; perspective divide; normalise; un-normalise (grid_sample)
  const float rx = hm[0] * x + hm[1] * y + hm[2];
  const float ry = hm[3] * x + hm[4] * y + hm[5];
  const float rz = hm[6] * x + hm[7] * y + hm[8];
  const float px = rx * depth + hm[9], py = ry * depth + hm[10], pz = rz * depth + hm[11];
  const float u = px / pz, vv = py / pz;
  const float gx = u / ((float)(W - 1) / 2.f) - 1.f;
  const float gy = vv / ((float)(H - 1) / 2.f) - 1.f;
  ix = ((gx + 1.f) * (float)W - 1.f) / 2.f;
  iy = ((gy + 1.f) * (float)H - 1.f) / 2.f;
}

struct Bilin { int x0, y0; float w00, w01, w10, w11; bool nan; };
__device__ __forceinline__ Bilin bilin_setup(float ix, float iy) {
  Bilin b;
  b.nan = !(isfinite(ix) && isfinite(iy));
  if (b.nan) { b.x0 = b.y0 = -100; b.w00 = b.w01 = b.w10 = b.w11 = 0.f; return b; }
  // clamp far-out-of-range coordinates before the int conversion (all four taps are outside anyway)
  ix = fminf(fmaxf(ix, -4.f), 1.0e6f);
  iy = fminf(fmaxf(iy, -4.f), 1.0e6f);
  const float fx = floorf(ix), fy = floorf(iy);
  b.x0 = (int)fx; b.y0 = (int)fy;
  const float tx = ix - fx, ty = iy - fy;
  b.w00 = (1.f - tx) * (1.f - ty);   // (x0,y0)  "nw"
  b.w01 = tx * (1.f - ty);           // (x1,y0)  "ne"
  b.w10 = (1.f - tx) * ty;           // (x0,y1)  "sw"
  b.w11 = tx * ty;                   // (x1,y1)  "se"
  return b;
}

}  // namespace rgbm
