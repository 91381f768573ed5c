// Two-view geometric consistency of dense depth maps and the packed point cloud of the surviving pixels, gfx950.
//
// depth_consistency_kernel: the check every MVSNet-style pipeline runs between "depth maps" and "point cloud".  One thread per pixel
// (x, y) of view a with depth d:
//   1. d not finite, d <= 0, or E_a / E_b without a finite inverse                      -> keep 0, fused / reproj / rel NaN
//   2. X = inv(E_a) (d ((x - cx_a) / fx_a, (y - cy_a) / fy_a, 1)); (u, v, z) = the projection of X through Kcrop_b E_b[:3];
//      z <= 0 or u, v outside [0, S - 1]                                                -> as 1
//   3. depth_b sampled bilinearly at (u, v), taps x0 = floor(u), x1 = min(x0 + 1, S - 1) (y alike); a tap that is not finite or
//      <= 0                                                                             -> as 1 (a map never bleeds across its own NaN silhouette)
//   4. (u, v) at the sampled depth back-projected through view b and projected into view a: (x', y', d');
//      reproj = hypot(x' - x, y' - y), rel = |d' - d| / d                                  (written whatever 5 decides)
//   5. keep = reproj < px_max && rel < rel_max && (no conf_a || conf >= conf_min) && (no mask_a || mask != 0);
//      fused = keep ? (d + d') / 2 : NaN
// All of it in fp64 on the float32 maps, rounded once into the float32 results; built without mul + add contraction (build.sh) like
// depth_points.hip, whose back-projection expression it shares (bbox_emit.h: backproject_world).  Rules 2-4 are reproject_round_trip
// of cloud_geom.h, which depth_fusion_kernel calls once per source view; the kernel keeps rule 1, the thresholds and what is written.
//
// cloud_pack_kernel: deterministic ordered compaction of the kept pixels into [n][cap][3] world-frame points: for pose i the kept pixels
// of view 1 in row-major order, then those of view 2.  No atomics: the slot of a pixel is the number of kept pixels before it.  A pose is
// cut into PACK_BLOCKS contiguous pieces, one workgroup each.  A workgroup first counts the keep bytes of the whole pose (three integer
// sums: kept before its piece, kept in view 1, kept in view 2 — integer addition, so the order of the reduction does not matter), then
// walks its piece in chunks of PACK_THREADS pixels with a wave ballot / popcount and a 16-entry LDS table of wave totals.  Rows from
// min(cap, total) to cap are filled with NaN / -1 by the pose's workgroups together.  The walk, the row and the fill are pack_walk /
// pack_emit_row / pack_fill_unused of cloud_geom.h, which cloud_pack_views_kernel (depth_fusion.hip) calls from its own counting
// prologue; a view's camera comes into LDS through load_view_pose in all four kernels.
#include <cmath>

#include "cloud_geom.h"
#include "common.h"
#include "kernels.h"

namespace rgbm {

namespace {
constexpr int PACK_THREADS = 1024;      // 16 waves
constexpr int PACK_BLOCKS = 8;          // workgroups per pose
constexpr int PACK_WAVES = PACK_THREADS / 64;
}  // namespace

// (256, 5): the one-off 4 x 4 inversion of load_view_pose, not the per-pixel code, sets the register count; five waves per SIMD are what the
// kernel has run at, and the bound keeps the inversion from costing one of them
__global__ __launch_bounds__(256, 5) void depth_consistency_kernel(const float* __restrict__ depth_a, const float* __restrict__ conf_a,
                                                                const unsigned char* __restrict__ mask_a, const double* __restrict__ Ka,
                                                                const double* __restrict__ Ea, const float* __restrict__ depth_b,
                                                                const double* __restrict__ Kb, const double* __restrict__ Eb, int S,
                                                                double px_max, double rel_max, float conf_min, float* __restrict__ fused,
                                                                float* __restrict__ reproj, float* __restrict__ rel,
                                                                unsigned char* __restrict__ keep) {
  __shared__ ViewPose cam[2];      // a, b
  const long long f = blockIdx.y;
  if (threadIdx.x == 0 || threadIdx.x == 64) load_view_pose(f, threadIdx.x ? Eb : Ea, cam[threadIdx.x >> 6]);      // two different waves
  __syncthreads();
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= S * S) return;
  const long long o = f * S * S + i;
  const int y = i / S, x = i - y * S;
  const float qnan = __uint_as_float(0x7fc00000u);
  float r_fused = qnan, r_reproj = qnan, r_rel = qnan;
  unsigned char r_keep = 0;
  const float df = depth_a[o];
  if (isfinite(df) && df > 0.f && cam[0].ok && cam[1].ok) {
    const double d = (double)df;
    const ViewK ka = view_intrinsics(f, Ka), kb = view_intrinsics(f, Kb);
    double X[3], e_px, e_rel, dr;
    backproject_world(cam[0].inv, (double)x, (double)y, d, ka.fx, ka.fy, ka.cx, ka.cy, X);
    if (reproject_round_trip(X, (double)x, (double)y, d, cam[0], ka, cam[1], kb, depth_b + f * S * S, S, e_px, e_rel, dr)) {
      r_reproj = (float)e_px;
      r_rel = (float)e_rel;
      const bool k = e_px < px_max && e_rel < rel_max && (!conf_a || conf_a[o] >= conf_min) && (!mask_a || mask_a[o] != 0);
      r_keep = k ? 1 : 0;
      if (k) r_fused = (float)((d + dr) / 2.0);
    }
  }
  fused[o] = r_fused;
  keep[o] = r_keep;
  if (reproj) reproj[o] = r_reproj;
  if (rel) rel[o] = r_rel;
}

int launch_depth_consistency(const float* depth_a, const float* conf_a, const unsigned char* mask_a, const double* Ka, const double* Ea,
                             const float* depth_b, const double* Kb, const double* Eb, int n, int S, double px_max, double rel_max,
                             float conf_min, float* fused, float* reproj, float* rel, unsigned char* keep, hipStream_t s) {
  RGBM_REQUIRE(depth_a && Ka && Ea && depth_b && Kb && Eb && fused && keep, "depth_consistency arguments");
  RGBM_REQUIRE(n > 0 && n <= 65535 && S > 0 && S <= 4096, "depth_consistency: 1 .. 65535 poses of at most 4096 x 4096 pixels");
  RGBM_REQUIRE(std::isfinite(px_max) && px_max >= 0 && std::isfinite(rel_max) && rel_max >= 0 && std::isfinite(conf_min) && conf_min >= 0,
               "depth_consistency: px_max, rel_max and conf_min are finite and >= 0");
  hipLaunchKernelGGL(depth_consistency_kernel, dim3((unsigned)((S * S + 255) / 256), (unsigned)n), dim3(256), 0, s, depth_a, conf_a, mask_a,
                     Ka, Ea, depth_b, Kb, Eb, S, px_max, rel_max, conf_min, fused, reproj, rel, keep);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

// (PACK_THREADS, 5): as for depth_consistency_kernel
__global__ __launch_bounds__(PACK_THREADS, 5) void cloud_pack_kernel(const float* __restrict__ fused1, const unsigned char* __restrict__ keep1,
                                                                  const double* __restrict__ K1, const double* __restrict__ E1,
                                                                  const float* __restrict__ fused2, const unsigned char* __restrict__ keep2,
                                                                  const double* __restrict__ K2, const double* __restrict__ E2, int S,
                                                                  int cap, float* __restrict__ cloud, int* __restrict__ index,
                                                                  int* __restrict__ count) {
  __shared__ ViewPose cam[2];
  __shared__ int wsum[3][PACK_WAVES];
  const long long f = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int SS = S * S, views = keep2 ? 2 : 1, T = views * SS;      // T <= 2^25
  const int piece = (T + PACK_BLOCKS - 1) / PACK_BLOCKS;
  const int lo = min((int)blockIdx.x * piece, T), hi = min(lo + piece, T);      // blockIdx.x: uniform over the workgroup
  if (tid == 0 || (tid == 64 && views == 2)) load_view_pose(f, wave ? E2 : E1, cam[wave]);
  const unsigned char* k1 = keep1 + f * SS;
  const unsigned char* k2 = keep2 ? keep2 + f * SS : nullptr;
  auto kept = [&](int p) -> bool { return (p < SS ? k1[p] : k2[p - SS]) != 0; };

  // kept pixels before this piece, in view 1, in view 2
  int c[3] = {0, 0, 0};
  for (int p = tid; p < T; p += PACK_THREADS) {
    const int k = kept(p) ? 1 : 0;
    c[0] += p < lo ? k : 0;
    c[1] += p < SS ? k : 0;
    c[2] += p < SS ? 0 : k;
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    for (int m = 32; m > 0; m >>= 1) c[j] += __shfl_xor(c[j], m, 64);
    if (lane == 0) wsum[j][wave] = c[j];
  }
  __syncthreads();
  int base = 0, n1 = 0, n2 = 0;      // sums over all waves: the same in every thread
  for (int w = 0; w < PACK_WAVES; ++w) { base += wsum[0][w]; n1 += wsum[1][w]; n2 += wsum[2][w]; }
  __syncthreads();      // wsum[0] is the walk's table
  if (blockIdx.x == 0 && tid == 0) { count[f * 2 + 0] = n1; count[f * 2 + 1] = n2; }

  float* cl = cloud + f * (long long)cap * 3;
  int* ix = index + f * (long long)cap;
  pack_walk<PACK_THREADS>(lo, hi, base, cap, wsum[0], kept, [&](int slot, int p) {
    const int v = p < SS ? 0 : 1, q = p - v * SS;
    pack_emit_row(cl, ix, slot, p, cam[v], view_intrinsics(f, v ? K2 : K1), q, S, (v ? fused2 : fused1)[f * SS + q]);
  });
  pack_fill_unused(cl, ix, (long long)n1 + n2, cap, (long long)blockIdx.x * PACK_THREADS + tid, (long long)PACK_BLOCKS * PACK_THREADS);
}

int launch_cloud_pack(const float* fused1, const unsigned char* keep1, const double* K1, const double* E1, const float* fused2,
                      const unsigned char* keep2, const double* K2, const double* E2, int n, int S, int cap, float* cloud, int* index,
                      int* count, hipStream_t s) {
  RGBM_REQUIRE(fused1 && keep1 && K1 && E1 && count, "cloud_pack arguments");
  const bool any2 = fused2 || keep2 || K2 || E2, all2 = fused2 && keep2 && K2 && E2;
  RGBM_REQUIRE(any2 == all2, "cloud_pack: fused2, keep2, Kcrop2 and E2 are given together or not at all");
  RGBM_REQUIRE(n > 0 && n <= 65535 && S > 0 && S <= 4096, "cloud_pack: 1 .. 65535 poses of at most 4096 x 4096 pixels");
  RGBM_REQUIRE(cap >= 0, "cloud_pack: cap >= 0");
  RGBM_REQUIRE(cap == 0 || (cloud && index), "cloud_pack: cloud and index are NULL");
  hipLaunchKernelGGL(cloud_pack_kernel, dim3(PACK_BLOCKS, (unsigned)n), dim3(PACK_THREADS), 0, s, fused1, keep1, K1, E1, fused2, keep2, K2,
                     E2, S, cap, cloud, index, count);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace rgbm
