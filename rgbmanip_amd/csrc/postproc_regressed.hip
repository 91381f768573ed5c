// The `direct_regression: True` tail of AdaPoseEstimator_v4.predict on the GPU (gfx950):
//   models/pose_estimator/AdaPose/interface_v4.py:322-325  (tr = view1_r, tt = view1_t, ts = ||view1_s||)
//   models/pose_estimator/AdaPose/interface_v4.py:358-378  (bbox -> camera frame -> world frame, default_bbox)
//   models/pose_estimator/AdaPose/lib/utils.py:40-74       (get_3d_bbox, transform_coordinates_3d)
// The translation and the scale come from the network's own heads, so the pair median of postproc.hip is never needed: one
// workgroup per pose, whose only reduction is the per-axis max of |nocs| over the P points; no scratch, one launch for any batch.
//
// Arithmetic follows the reference's dtypes, which differ from v5's: ts is a float32 scalar here, so size, the corners and the
// camera-frame box stay float32 (v5's scale is a float64 median) and only the world transform is float64.
//  * ts = np.linalg.norm(s) = sqrt(s.dot(s)): numpy's float32 dot of a short vector (OpenBLAS sdot) rounds every product to float32 and
//    accumulates the products in double; the sum is rounded to float32 and the root taken in float32.
//  * size = 2 * half * ts and size / 2: float32 (the factor 2 is exact).
//  * sRT @ [bbox; 1] is a float32 matrix product (sgemm): per element one chain of fused multiply-adds over k = 0..3, starting from
//    the rounded first product; the last term t * 1 rounds acc + t.  Row 3 of sRT is (0, 0, 0, 1), so the division by the
//    homogeneous coordinate changes nothing finite and turns a non-finite corner into NaN, which is rejected either way.
// tests/golden/postproc_v4.npz pins all of it against the reference's own numpy calls.
// Built with -ffp-contract=off: only the fmaf calls below fuse.
#include "common.h"
#include "kernels.h"
#include "bbox_emit.h"

#pragma clang fp contract(off)

namespace rgbm {

namespace {

constexpr int PR_THREADS = 256;
constexpr int PR_WAVES = PR_THREADS / 64;

__global__ __launch_bounds__(PR_THREADS) void postprocess_regressed_kernel(
    const float* __restrict__ nocs /*[B,P,3]*/, const float* __restrict__ rot /*[B,9]*/, const float* __restrict__ tr /*[B,3]*/,
    const float* __restrict__ sv /*[B,3]*/, const double* __restrict__ E1 /*[B,16]*/, double* __restrict__ bbox /*[B,8,3]*/,
    double* __restrict__ ts_out /*[B,4]*/, int* __restrict__ valid, int P) {
  __shared__ float wmax[PR_WAVES][3];
  __shared__ int wnan[PR_WAVES];
  const long long b = blockIdx.x;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const float* n = nocs + b * P * 3;
  // half = np.max(abs(nocs), axis=0): np.max propagates NaN (fmaxf drops it: carried as a flag; a NaN on any axis rejects the box)
  float m[3] = {0.f, 0.f, 0.f};
  int nan = 0;
  for (int i = t; i < P; i += PR_THREADS) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float x = fabsf(n[(long long)i * 3 + c]);
      nan |= x != x;
      m[c] = fmaxf(m[c], x);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int c = 0; c < 3; ++c) m[c] = fmaxf(m[c], __shfl_xor(m[c], off));
    nan |= __shfl_xor(nan, off);
  }
  if (lane == 0) { wmax[wv][0] = m[0]; wmax[wv][1] = m[1]; wmax[wv][2] = m[2]; wnan[wv] = nan; }
  __syncthreads();
  if (t != 0) return;
  float half[3] = {wmax[0][0], wmax[0][1], wmax[0][2]};
  nan = wnan[0];
  for (int w = 1; w < PR_WAVES; ++w) {
    for (int c = 0; c < 3; ++c) half[c] = fmaxf(half[c], wmax[w][c]);
    nan |= wnan[w];
  }
  const float* s = sv + b * 3;
  const float q0 = s[0] * s[0], q1 = s[1] * s[1], q2 = s[2] * s[2];
  const float scale = sqrtf((float)(((double)q0 + (double)q1) + (double)q2));
  float R[9], tf[3], hs[3];
  for (int i = 0; i < 9; ++i) R[i] = rot[b * 9 + i];
  for (int i = 0; i < 3; ++i) {
    tf[i] = tr[b * 3 + i];
    hs[i] = nan ? __builtin_nanf("") : ((2.f * half[i]) * scale) / 2.f;
    ts_out[b * 4 + i] = (double)tf[i];
  }
  ts_out[b * 4 + 3] = (double)scale;
  double a[4][8], cam[8][3];
  const bool ok = invert_extrinsic(b, E1, a);
  for (int k = 0; k < 8; ++k) {
    const float p0 = (float)bbox_sign(k, 0) * hs[0], p1 = (float)bbox_sign(k, 1) * hs[1], p2 = (float)bbox_sign(k, 2) * hs[2];
    for (int i = 0; i < 3; ++i)
      cam[k][i] = (double)fmaf(tf[i], 1.f, fmaf(R[i * 3 + 2], p2, fmaf(R[i * 3 + 1], p1, R[i * 3 + 0] * p0)));
  }
  emit_corners_world(b, cam, ok, a, bbox, valid);
}

}  // namespace

int launch_postprocess_regressed(const float* nocs, const float* rot, const float* tr, const float* sv, const double* E1, double* bbox,
                                 double* ts_out, int* valid, int B, int P, hipStream_t s) {
  RGBM_REQUIRE(nocs && rot && tr && sv && E1 && bbox && ts_out && valid, "postprocess_regressed arguments");
  RGBM_REQUIRE(B >= 1 && P >= 1 && P <= 1024, "postprocess_regressed needs B >= 1 and 1 <= P <= 1024");
  hipLaunchKernelGGL(postprocess_regressed_kernel, dim3((unsigned)B), dim3(PR_THREADS), 0, s, nocs, rot, tr, sv, E1, bbox, ts_out, valid, P);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace rgbm
