// What the dense-depth cloud kernels share (depth_consistency.hip: two views, depth_fusion.hip: V views; DESIGN.md sections 5k, 5n):
// a view's camera in LDS, the reprojection round trip of the consistency rules, and the ordered compaction of the pack kernels.  All
// fp64 on float32 maps; both files are built without mul + add contraction (build.sh), the pragma keeps that true for this text.
#pragma once
#include <hip/hip_runtime.h>

#include "bbox_emit.h"

#pragma clang fp contract(off)

namespace rgbm {

// A view's camera.  The pose half costs a 4 x 4 inversion and lives in LDS: one thread per view calls load_view_pose, a barrier follows
// before anyone reads it.  The intrinsics are four doubles at an address that is uniform over the workgroup: every thread reads them
// from Kcrop itself (scalar loads; a copy in LDS would come back through vector registers).
struct ViewPose {
  double inv[12];      // inv(E) as [R | t]
  double ext[12];      // E[:3]
  int ok;              // E has a finite inverse
};
struct ViewK { double fx, fy, cx, cy; };

__device__ inline void load_view_pose(long long f, const double* __restrict__ E /*[.][16]*/, ViewPose& c) {
  for (int j = 0; j < 12; ++j) c.ext[j] = E[f * 16 + j];
  c.ok = invert_extrinsic_rows(f, E, c.inv) ? 1 : 0;
}
__device__ inline ViewK view_intrinsics(long long f, const double* __restrict__ K /*[.][9]*/) {
  return ViewK{K[f * 9 + 0], K[f * 9 + 4], K[f * 9 + 2], K[f * 9 + 5]};
}

// Rules 2-4 of the consistency check (depth_consistency.hip) for pixel (x, y) of view a at depth d > 0 against view b, both with a
// finite inverse.  X = the pixel in the world frame, backproject_world(a.inv, x, y, d, ka ...): the caller computes it, so that a
// kernel with several sources does so once.  (u, v, z) = X in view b; depth_b [S][S] sampled bilinearly at (u, v) with taps
// x0 = floor(u), x1 = min(x0 + 1, S - 1) (y alike); (u, v) at the sampled depth taken back through view b into view a: (x', y', d').
// false: b does not witness the pixel (z <= 0, (u, v) outside [0, S - 1], or a tap that is not finite or <= 0: a map never bleeds
// across its own NaN silhouette).  true: e_px = hypot(x' - x, y' - y), e_rel = |d' - d| / d, dr = d'.
__device__ inline bool reproject_round_trip(const double X[3], double x, double y, double d, const ViewPose& a, const ViewK& ka,
                                            const ViewPose& b, const ViewK& kb, const float* __restrict__ depth_b, int S, double& e_px,
                                            double& e_rel, double& dr) {
  const double top = (double)(S - 1);
  double u, v, z;
  project_view(b.ext, X, kb.fx, kb.fy, kb.cx, kb.cy, u, v, z);
  if (!(z > 0.0 && u >= 0.0 && u <= top && v >= 0.0 && v <= top)) return false;      // true for NaN
  const int x0 = (int)floor(u), y0 = (int)floor(v);                                   // 0 .. S - 1
  const int x1 = min(x0 + 1, S - 1), y1 = min(y0 + 1, S - 1);
  const float t00 = depth_b[y0 * S + x0], t01 = depth_b[y0 * S + x1], t10 = depth_b[y1 * S + x0], t11 = depth_b[y1 * S + x1];
  if (!(isfinite(t00) && isfinite(t01) && isfinite(t10) && isfinite(t11) && t00 > 0.f && t01 > 0.f && t10 > 0.f && t11 > 0.f)) return false;
  const double ax = u - (double)x0, ay = v - (double)y0;
  const double db = ((double)t00 * (1.0 - ax) + (double)t01 * ax) * (1.0 - ay) + ((double)t10 * (1.0 - ax) + (double)t11 * ax) * ay;
  double Xb[3], xr, yr;
  backproject_world(b.inv, u, v, db, kb.fx, kb.fy, kb.cx, kb.cy, Xb);
  project_view(a.ext, Xb, ka.fx, ka.fy, ka.cx, ka.cy, xr, yr, dr);
  e_px = hypot(xr - x, yr - y);
  e_rel = fabs(dr - d) / d;
  return true;
}

// Ordered compaction without atomics: the kept pixels p of [lo, hi) get the slots base, base + 1, ... in increasing p, and emit(slot, p)
// runs for every slot < cap.  Chunks of THREADS pixels, a wave ballot / popcount and the LDS table wtab[THREADS / 64] of wave totals.
// Returns base + the kept pixels walked (the walk stops once base >= cap).
// BARRIERS INSIDE THE LOOP: every thread of the workgroup calls this, with the same lo, hi, base and cap; wtab is free on entry (a
// barrier since its last use) and on return.
template <int THREADS, class Kept, class Emit>
__device__ inline int pack_walk(int lo, int hi, int base, int cap, int* wtab, Kept kept, Emit emit) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int p0 = lo; p0 < hi && base < cap; p0 += THREADS) {      // base, p0: the same in every thread
    const int p = p0 + tid;
    const bool k = p < hi && kept(p);
    const unsigned long long b = __ballot(k);
    if (lane == 0) wtab[wave] = __popcll(b);
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < THREADS / 64; ++w) { const int t = wtab[w]; before += w < wave ? t : 0; all += t; }
    const int slot = base + before + __popcll(b & ((1ull << lane) - 1ull));
    if (k && slot < cap) emit(slot, p);
    base += all;
    __syncthreads();
  }
  return base;
}

// Row `slot` of a pose's packed cloud cl [cap][3] / ix [cap]: pixel q = y S + x of view c at fused depth zf in the world frame (NaN
// without a finite depth or inverse), and the index the gather kernels look it up by.
__device__ inline void pack_emit_row(float* __restrict__ cl, int* __restrict__ ix, int slot, int index, const ViewPose& c, const ViewK& k, int q, int S,
                                     float zf) {
  const float qnan = __uint_as_float(0x7fc00000u);
  const int y = q / S, x = q - y * S;
  float o[3] = {qnan, qnan, qnan};
  if (isfinite(zf) && c.ok) {
    double w3[3];
    backproject_world(c.inv, (double)x, (double)y, (double)zf, k.fx, k.fy, k.cx, k.cy, w3);
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = (float)w3[r];
  }
  cl[(long long)slot * 3 + 0] = o[0];
  cl[(long long)slot * 3 + 1] = o[1];
  cl[(long long)slot * 3 + 2] = o[2];
  ix[slot] = index;
}

// The rows no pixel fills, [min(cap, total), cap): NaN / -1, shared among the pose's `threads` threads of which this one is `me`
__device__ inline void pack_fill_unused(float* __restrict__ cl, int* __restrict__ ix, long long total, int cap, long long me, long long threads) {
  const float qnan = __uint_as_float(0x7fc00000u);
  for (long long r = (total < cap ? total : cap) + me; r < cap; r += threads) {
    cl[r * 3 + 0] = qnan; cl[r * 3 + 1] = qnan; cl[r * 3 + 2] = qnan;
    ix[r] = -1;
  }
}

}  // namespace rgbm
