// Tail of AdaPoseEstimator_v5.predict shared by the post-processing kernels (postproc.hip, align.hip, postproc_regressed.hip):
//   bbox corners of `size` (lib/utils.py:49-56), transformed by sRT = [R | t] held in float32 (interface_v5.py:357-361,
//   utils.py:58-74), then taken to the world frame with inv(view1_extrinsic), or default_bbox when anything is non-finite
//   (interface_v5.py:368-374).  Called by one thread per pose.
#pragma once
#include <hip/hip_runtime.h>

namespace rgbm {

// corner signs of get_3d_bbox (lib/utils.py:49-56)
__device__ inline double bbox_sign(int k, int axis) {
  const double sg[8][3] = {{1, 1, 1}, {1, 1, -1}, {-1, 1, 1}, {-1, 1, -1}, {1, -1, 1}, {1, -1, -1}, {-1, -1, 1}, {-1, -1, -1}};
  return sg[k][axis];
}

// a = [E1[b] | I] reduced by Gauss-Jordan with partial pivoting in fp64: columns 4..7 hold inv(E1[b]).  false: singular or non-finite.
__device__ inline bool invert_extrinsic(long long b, const double* __restrict__ E1, double a[4][8]) {
  bool ok = true;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) { a[i][j] = E1[b * 16 + i * 4 + j]; a[i][4 + j] = i == j ? 1.0 : 0.0; }
  for (int c = 0; c < 4; ++c) {
    int piv = c; double best = fabs(a[c][c]);
    for (int rr = c + 1; rr < 4; ++rr) if (fabs(a[rr][c]) > best) { best = fabs(a[rr][c]); piv = rr; }
    if (!(best > 0.0)) { ok = false; break; }
    if (piv != c) for (int k = 0; k < 8; ++k) { const double tmp = a[c][k]; a[c][k] = a[piv][k]; a[piv][k] = tmp; }
    const double inv = 1.0 / a[c][c];
    for (int k = 0; k < 8; ++k) a[c][k] *= inv;
    for (int rr = 0; rr < 4; ++rr) if (rr != c) { const double f = a[rr][c]; for (int k = 0; k < 8; ++k) a[rr][k] -= f * a[c][k]; }
  }
  for (int i = 0; i < 4 && ok; ++i) for (int j = 0; j < 4; ++j) if (!isfinite(a[i][4 + j])) ok = false;
  return ok;
}

// inv(E) of view b as the 3 x 4 matrix [R | t] (row-major, 12 doubles) the back-projection below applies; false: no finite inverse
__device__ inline bool invert_extrinsic_rows(long long b, const double* __restrict__ E, double* inv /*[12]*/) {
  double a[4][8];
  const bool ok = invert_extrinsic(b, E, a);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 4; ++j) inv[i * 4 + j] = a[i][4 + j];
  return ok;
}

// pixel (x, y) of a crop at camera depth z -> world frame: cam = ((x - cx) z / fx, (y - cy) z / fy, z), world = inv[:, :3] cam + inv[:, 3]
// (interface_v5.py:329-336, 369-372).  The ONE expression depth_points.hip and depth_consistency.hip evaluate (both built without
// contraction), so that a packed cloud point equals the point image's bit for bit.
__device__ inline void backproject_world(const double* inv /*[12]*/, double x, double y, double z, double fx, double fy, double cx, double cy,
                                         double out[3]) {
  const double c0 = (x - cx) * z / fx, c1 = (y - cy) * z / fy;
#pragma unroll
  for (int r = 0; r < 3; ++r) out[r] = inv[r * 4 + 0] * c0 + inv[r * 4 + 1] * c1 + inv[r * 4 + 2] * z + inv[r * 4 + 3];
}

// world X -> (u, v, z) of a view with rows E[0..11] of its extrinsic and fx, fy, cx, cy of its cropped intrinsics (cloud_geom.h:
// reproject_round_trip)
__device__ inline void project_view(const double* E /*[12]*/, const double X[3], double fx, double fy, double cx, double cy, double& u,
                                    double& v, double& z) {
  const double c0 = E[0] * X[0] + E[1] * X[1] + E[2] * X[2] + E[3];
  const double c1 = E[4] * X[0] + E[5] * X[1] + E[6] * X[2] + E[7];
  z = E[8] * X[0] + E[9] * X[1] + E[10] * X[2] + E[11];
  u = fx * c0 / z + cx;
  v = fy * c1 / z + cy;
}

// the corners of pose b as they are, or default_bbox (+10 cube) when !ok; valid = ok
__device__ inline void emit_corners(long long b, const double c[8][3], bool ok, double* __restrict__ bbox, int* __restrict__ valid) {
  const double dflt[8][3] = {{0, 0, 0}, {0, 0, 1}, {0, 1, 0}, {0, 1, 1}, {1, 0, 0}, {1, 0, 1}, {1, 1, 0}, {1, 1, 1}};
  for (int k = 0; k < 8; ++k)
    for (int i = 0; i < 3; ++i) bbox[(b * 8 + k) * 3 + i] = ok ? c[k][i] : dflt[k][i] + 10.0;
  valid[b] = ok ? 1 : 0;
}

// camera-frame corners -> world frame through `a` (invert_extrinsic), or default_bbox and valid = 0 when !ok or a corner is non-finite
__device__ inline void emit_corners_world(long long b, const double cam[8][3], bool ok, const double a[4][8], double* __restrict__ bbox,
                                          int* __restrict__ valid) {
  double out[8][3];
  for (int k = 0; k < 8 && ok; ++k)
    for (int i = 0; i < 3; ++i) {
      if (!isfinite(cam[k][i])) ok = false;
      out[k][i] = a[i][4] * cam[k][0] + a[i][5] * cam[k][1] + a[i][6] * cam[k][2] + a[i][7];
    }
  emit_corners(b, out, ok, bbox, valid);
}

// the corners of a box of `size` in the frame sRT = [R | t] maps to; R and t are the float32 values the reference's sRT holds
__device__ inline void bbox_corners_srt(const double R[9] /* float32 values */, const float tf[3], const double size[3], double c[8][3]) {
  for (int k = 0; k < 8; ++k) {
    const double p[3] = {bbox_sign(k, 0) * size[0] / 2, bbox_sign(k, 1) * size[1] / 2, bbox_sign(k, 2) * size[2] / 2};
    for (int i = 0; i < 3; ++i) c[k][i] = R[i * 3 + 0] * p[0] + R[i * 3 + 1] * p[1] + R[i * 3 + 2] * p[2] + (double)tf[i];
  }
}

__device__ inline void emit_bbox_world(long long b, const double R[9] /* float32 values */, const float tf[3], const double size[3],
                                       bool ok, const double* __restrict__ E1, double* __restrict__ bbox, int* __restrict__ valid) {
  double a[4][8];
  if (!invert_extrinsic(b, E1, a)) ok = false;
  double cam[8][3];
  if (ok) bbox_corners_srt(R, tf, size, cam);
  emit_corners_world(b, cam, ok, a, bbox, valid);
}

}  // namespace rgbm
