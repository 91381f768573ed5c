// Depth map of a crop -> world-frame points, gfx950: the per-pixel analogue of the simulator camera's `Position` image
// (collection.py:230-233) and of the back-projection `predict` applies to the chosen pixels (interface_v5.py:329-336):
//   cam = ((x - cx) z / fx, (y - cy) z / fy, z),   world = inv(E)[:3, :3] cam + inv(E)[:3, 3]
// with the cropped intrinsics (fx, fy, cx, cy of Kcrop; the crop step produces no skew) and inv(E) from the Gauss-Jordan inverse the
// box tail uses for ex_inv (bbox_emit.h: invert_extrinsic).  Arithmetic in fp64 on float32 depths, rounded once into the float32 result;
// compiled without mul + add contraction (build.sh), like postproc.hip, so it rounds like its numpy twin.  A pixel whose depth is not
// finite yields NaN (so does every pixel of a view whose E has no finite inverse); nothing is clamped.
#include "bbox_emit.h"
#include "common.h"
#include "kernels.h"

namespace rgbm {

__global__ __launch_bounds__(256) void depth_to_points_kernel(const float* __restrict__ depth, const double* __restrict__ Kc,
                                                              const double* __restrict__ E, float* __restrict__ points, int S) {
  __shared__ double inv[12];
  __shared__ int inv_ok;
  const long long v = blockIdx.y;
  if (threadIdx.x == 0) inv_ok = invert_extrinsic_rows(v, E, inv) ? 1 : 0;
  __syncthreads();
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= S * S) return;
  const int y = i / S, x = i - y * S;
  const double fx = Kc[v * 9 + 0], fy = Kc[v * 9 + 4], cx = Kc[v * 9 + 2], cy = Kc[v * 9 + 5];
  const float zf = depth[v * S * S + i];
  float* o = points + (v * S * S + i) * 3;
  if (!isfinite(zf) || !inv_ok) {
    const float qnan = __uint_as_float(0x7fc00000u);
    o[0] = qnan; o[1] = qnan; o[2] = qnan;
    return;
  }
  double w[3];
  backproject_world(inv, (double)x, (double)y, (double)zf, fx, fy, cx, cy, w);
#pragma unroll
  for (int r = 0; r < 3; ++r) o[r] = (float)w[r];
}

int launch_depth_to_points(const float* depth, const double* Kc, const double* E, int n, int S, float* points, hipStream_t s) {
  RGBM_REQUIRE(depth && Kc && E && points, "depth_to_points arguments");
  RGBM_REQUIRE(n > 0 && n <= 65535 && S > 0 && S <= 4096, "depth_to_points: 1 .. 65535 views of at most 4096 x 4096 pixels");
  hipLaunchKernelGGL(depth_to_points_kernel, dim3((unsigned)((S * S + 255) / 256), (unsigned)n), dim3(256), 0, s, depth, Kc, E, points, S);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace rgbm
