// The `direct_regression: False`, `use_depth: True` tail of AdaPoseEstimator_v5.predict on the GPU:
//   /root/reference/models/pose_estimator/AdaPose/interface_v5.py:322-339  back-projection of the predicted depth
//   /root/reference/models/pose_estimator/AdaPose/lib/align.py:10-41       estimateSimilarityUmeyama
//   /root/reference/models/pose_estimator/AdaPose/lib/align.py:44-104      estimateSimilarityTransform (RANSAC)
//   /root/reference/models/pose_estimator/AdaPose/interface_v5.py:348-374  bbox from (s, R, t), world frame, default bbox
// One workgroup per pose.  The reference runs 128 RANSAC iterations one after the other, each a 5-point Umeyama fit and a
// residual pass over all P points, stopping early by a confidence rule.  Here the 128 hypotheses are fitted by 128 threads at
// once, the P x 128 residual tests are spread over the waves (ballot + popcount), and thread 0 then replays the
// reference's sequential "strictly better ratio / early break" scan over the 128 inlier counts, so the hypothesis chosen is
// the one the sequential loop would have kept.  The final fit over the inliers uses block-wide fp64 sums.
// The 5-point samples come from a seeded hash (sample k of iteration i of pose b = mix32(seed, 128 b + i, k) mod P) where
// the reference uses the global np.random.randint — the same distribution, reproducible, restated in oracle/align_ref.py.
// A NaN covariance makes the reference raise; here the pose is marked invalid (default bbox).
// The hypothesis, the inlier test and the scan are align_math.h's (ransac_hypothesis / ransac_inlier / ransac_scan), which cloud_fit.hip
// calls on streamed rows; the hash and the block sums are common.h's, the box is bbox_emit.h's.
#include "common.h"
#include "kernels.h"
#include "bbox_emit.h"
#include "align_math.h"

#pragma clang fp contract(off)

namespace rgbm {

namespace {

constexpr int AL_THREADS = 256;
constexpr int AL_MAXP = 1024;
constexpr int AL_ITERS = 128;

}  // namespace

__global__ __launch_bounds__(AL_THREADS) void umeyama_ransac_kernel(
    const float* __restrict__ nocs /*[B,P,3]*/, const float* __restrict__ depth /*[B,P]*/, const int* __restrict__ choose /*[B,P]*/,
    const double* __restrict__ Kc /*[B,9]*/, const double* __restrict__ E1 /*[B,16]*/, double* __restrict__ bbox /*[B,8,3]*/,
    double* __restrict__ srt /*[B,13]: s, R(9), t(3)*/, int* __restrict__ valid, int P, int img, unsigned seed) {
  __shared__ double sx[AL_MAXP], sy[AL_MAXP], sz[AL_MAXP], tx[AL_MAXP], ty[AL_MAXP], tz[AL_MAXP];
  __shared__ double hyp[AL_ITERS][13];          // s*R (9), t (3), threshold
  __shared__ int cnt[AL_ITERS];
  __shared__ double red[AL_THREADS];
  __shared__ int s_best, s_fail;
  __shared__ float hmax[3];
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const double fx = Kc[b * 9 + 0], cx = Kc[b * 9 + 2], fy = Kc[b * 9 + 4], cy = Kc[b * 9 + 5];
  if (t == 0) { s_best = -1; s_fail = 0; hmax[0] = hmax[1] = hmax[2] = 0.f; }
  __syncthreads();
  double ax = 0, ay = 0, az = 0;
  bool nan_in = false;
  for (int p = t; p < P; p += AL_THREADS) {
    const float* n = nocs + ((long long)b * P + p) * 3;
    sx[p] = n[0]; sy[p] = n[1]; sz[p] = n[2];
    const int ch = choose[(long long)b * P + p];
    const double z = (double)depth[(long long)b * P + p];
    tx[p] = ((double)(ch % img) - cx) * z / fx;
    ty[p] = ((double)(ch / img) - cy) * z / fy;
    tz[p] = z;
    ax += sx[p]; ay += sy[p]; az += sz[p];
    nan_in |= (n[0] != n[0]) || (n[1] != n[1]) || (n[2] != n[2]);
    atomicMax((int*)&hmax[0], __float_as_int(fabsf(n[0])));
    atomicMax((int*)&hmax[1], __float_as_int(fabsf(n[1])));
    atomicMax((int*)&hmax[2], __float_as_int(fabsf(n[2])));
  }
  // inlier threshold: a tenth of the source diameter (align.py:52-57)
  const double mx = block_sum<AL_THREADS>(ax, red) / P, my = block_sum<AL_THREADS>(ay, red) / P, mz = block_sum<AL_THREADS>(az, red) / P;
  double far = 0.0;
  for (int p = t; p < P; p += AL_THREADS) {
    const double dx = sx[p] - mx, dy = sy[p] - my, dz = sz[p] - mz;
    far = fmax(far, sqrt((dx * dx + dy * dy) + dz * dz));
  }
  const double inlier_t = 2 * block_max<AL_THREADS>(far, red) / 10.0;
  const auto inlier = [&](const double* m, int p) -> bool {
    const double s[3] = {sx[p], sy[p], sz[p]}, w[3] = {tx[p], ty[p], tz[p]};
    return ransac_inlier(m, s, w);
  };

  // ---- 128 five-point hypotheses, one per thread (align.py:66-70) ----
  if (t < AL_ITERS) {
    double sv[5][3], tv[5][3];
    for (int k = 0; k < 5; ++k) {
      const int i = (int)(mix32(seed, (unsigned)b * AL_ITERS + t, k) % (unsigned)P);
      sv[k][0] = sx[i]; sv[k][1] = sy[i]; sv[k][2] = sz[i];
      tv[k][0] = tx[i]; tv[k][1] = ty[i]; tv[k][2] = tz[i];
    }
    if (!ransac_hypothesis(sv, tv, inlier_t, hyp[t])) s_fail = 1;
  }
  __syncthreads();

  // ---- inlier counts of every hypothesis: wave w takes hypotheses w, w+4, ... (align.py:71-76) ----
  for (int h = wave; h < AL_ITERS; h += AL_THREADS / 64) {
    int c = 0;
    for (int p = lane; p < P; p += 64) c += __popcll(__ballot(inlier(hyp[h], p)));
    if (lane == 0) cnt[h] = c;
  }
  __syncthreads();

  // ---- the reference's sequential scan picks the hypothesis (align.py:77-87) ----
  if (t == 0) {
    int examined;
    s_best = ransac_scan(cnt, AL_ITERS, P, examined);
  }
  __syncthreads();
  const int best_h = s_best;
  const bool fail = s_fail != 0;

  // ---- final fit over the inliers of the kept hypothesis (align.py:93-95) ----
  double n_in = 0, a0 = 0, a1 = 0, a2 = 0, b0 = 0, b1 = 0, b2 = 0;
  if (best_h >= 0) {
    for (int p = t; p < P; p += AL_THREADS) {
      if (inlier(hyp[best_h], p)) {
        n_in += 1; a0 += sx[p]; a1 += sy[p]; a2 += sz[p]; b0 += tx[p]; b1 += ty[p]; b2 += tz[p];
      } else {
        sx[p] = __builtin_nan("");              // mark as outlier for the second pass (this thread owns p)
      }
    }
  }
  const double n = block_sum<AL_THREADS>(n_in, red);
  const double ms[3] = {block_sum<AL_THREADS>(a0, red) / n, block_sum<AL_THREADS>(a1, red) / n, block_sum<AL_THREADS>(a2, red) / n};
  const double mt[3] = {block_sum<AL_THREADS>(b0, red) / n, block_sum<AL_THREADS>(b1, red) / n, block_sum<AL_THREADS>(b2, red) / n};
  double cv[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, var = 0.0;
  if (best_h >= 0) {
    for (int p = t; p < P; p += AL_THREADS) {
      if (sx[p] != sx[p]) continue;
      const double cs[3] = {sx[p] - ms[0], sy[p] - ms[1], sz[p] - ms[2]};
      const double ct[3] = {tx[p] - mt[0], ty[p] - mt[1], tz[p] - mt[2]};
      for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) cv[i * 3 + j] += ct[i] * cs[j];
      var += (cs[0] * cs[0] + cs[1] * cs[1]) + cs[2] * cs[2];
    }
  }
  double cov[9];
  for (int i = 0; i < 9; ++i) cov[i] = block_sum<AL_THREADS>(cv[i], red) / n;
  var = block_sum<AL_THREADS>(var, red) / n;
  const double any_nan = block_sum<AL_THREADS>(nan_in ? 1.0 : 0.0, red);
  if (t == 0) {
    double scale = 0, R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, tr[3] = {0, 0, 0};
    bool ok = best_h >= 0 && !fail && any_nan == 0.0;
    if (ok) ok = umeyama_from_stats(cov, ms, mt, var, scale, R, tr);
    double* o = srt + (long long)b * 13;
    o[0] = ok ? scale : __builtin_nan("");
    for (int i = 0; i < 9; ++i) o[1 + i] = R[i];
    for (int i = 0; i < 3; ++i) o[10 + i] = tr[i];
    // sRT is a float32 matrix in the reference (interface_v5.py:357-361): R and t are rounded to float32 there
    double Rf[9];
    for (int i = 0; i < 9; ++i) Rf[i] = (double)(float)R[i];
    const float tf[3] = {(float)tr[0], (float)tr[1], (float)tr[2]};
    const double size[3] = {2.0 * (double)hmax[0] * scale, 2.0 * (double)hmax[1] * scale, 2.0 * (double)hmax[2] * scale};
    emit_bbox_world(b, Rf, tf, size, ok, E1, bbox, valid);
  }
}

int launch_umeyama_ransac(const float* nocs, const float* depth, const int* choose, const double* Kc, const double* E1,
                          double* bbox, double* srt, int* valid, int B, int P, int img, unsigned seed, hipStream_t s) {
  RGBM_REQUIRE(nocs && depth && choose && Kc && E1 && bbox && srt && valid, "umeyama_ransac arguments");
  RGBM_REQUIRE(B > 0 && P >= 5 && P <= AL_MAXP && img > 0, "umeyama_ransac needs 5 <= P <= 1024");
  hipLaunchKernelGGL(umeyama_ransac_kernel, dim3(B), dim3(AL_THREADS), 0, s, nocs, depth, choose, Kc, E1, bbox, srt, valid, P,
                     img, seed);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace rgbm
