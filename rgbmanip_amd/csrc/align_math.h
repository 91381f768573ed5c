// The similarity-fit arithmetic shared by align.hip (umeyama_ransac_kernel) and cloud_fit.hip (the fit over the two-view cloud):
// a 3 x 3 SVD by one-sided Jacobi, Umeyama's closed form from sufficient statistics (lib/align.py:10-41) and the three steps of the RANSAC
// around it (five-point hypothesis, inlier test, sequential scan; lib/align.py:44-104), fp64.  The sample hash is common.h's mix32.
// Both files are built without mul+add contraction; the pragma below keeps that true for this text wherever it is included.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace rgbm {

__device__ inline double det3(const double* m) {
  return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

// A (row-major 3x3) = U diag(S) V^T, S descending, by one-sided Jacobi on the columns of A.
__device__ inline void svd3(const double* A, double* U, double* S, double* V) {
  double W[9], Vm[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  for (int i = 0; i < 9; ++i) W[i] = A[i];
  for (int sweep = 0; sweep < 30; ++sweep) {
    double off = 0.0;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        double alpha = 0, beta = 0, gamma = 0;
        for (int r = 0; r < 3; ++r) { alpha += W[r * 3 + p] * W[r * 3 + p]; beta += W[r * 3 + q] * W[r * 3 + q]; gamma += W[r * 3 + p] * W[r * 3 + q]; }
        if (gamma == 0.0 || fabs(gamma) <= 1e-300) continue;
        off = fmax(off, fabs(gamma) / sqrt(alpha * beta));
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double tt = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + tt * tt), s = c * tt;
        for (int r = 0; r < 3; ++r) {
          const double wp = W[r * 3 + p], wq = W[r * 3 + q];
          W[r * 3 + p] = c * wp - s * wq; W[r * 3 + q] = s * wp + c * wq;
          const double vp = Vm[r * 3 + p], vq = Vm[r * 3 + q];
          Vm[r * 3 + p] = c * vp - s * vq; Vm[r * 3 + q] = s * vp + c * vq;
        }
      }
    if (off < 1e-15) break;
  }
  double sv[3];
  for (int j = 0; j < 3; ++j) sv[j] = sqrt(W[j] * W[j] + W[3 + j] * W[3 + j] + W[6 + j] * W[6 + j]);
  int ord[3] = {0, 1, 2};
  for (int a = 0; a < 2; ++a)
    for (int b = a + 1; b < 3; ++b)
      if (sv[ord[b]] > sv[ord[a]]) { const int tmp = ord[a]; ord[a] = ord[b]; ord[b] = tmp; }
  const double tiny = 1e-14 * fmax(sv[ord[0]], 1e-300);
  for (int j = 0; j < 3; ++j) {
    const int o = ord[j];
    S[j] = sv[o];
    for (int r = 0; r < 3; ++r) { V[r * 3 + j] = Vm[r * 3 + o]; U[r * 3 + j] = sv[o] > tiny ? W[r * 3 + o] / sv[o] : 0.0; }
  }
  // columns of U that belong to (numerically) zero singular values: complete to an orthonormal basis
  if (!(S[0] > tiny)) { U[0] = 1; U[3] = 0; U[6] = 0; }
  if (!(S[1] > tiny)) {
    const double ax = fabs(U[0]), ay = fabs(U[3]), az = fabs(U[6]);
    double e[3] = {0, 0, 0};
    e[(ax <= ay && ax <= az) ? 0 : (ay <= az ? 1 : 2)] = 1.0;
    const double d = e[0] * U[0] + e[1] * U[3] + e[2] * U[6];
    double v[3] = {e[0] - d * U[0], e[1] - d * U[3], e[2] - d * U[6]};
    const double n = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    U[1] = v[0] / n; U[4] = v[1] / n; U[7] = v[2] / n;
  }
  if (!(S[2] > tiny)) {
    U[2] = U[3] * U[7] - U[6] * U[4]; U[5] = U[6] * U[1] - U[0] * U[7]; U[8] = U[0] * U[4] - U[3] * U[1];
  }
}

// Umeyama from sufficient statistics: n, centroids ms / mt, Cov = sum (t - mt)(s - ms)^T / n, varP = sum_axis var(source).
// -> scale, R (row-major), t.  Returns false for a NaN covariance.
__device__ inline bool umeyama_from_stats(const double* cov, const double* ms, const double* mt, double varP, double& scale, double* R, double* t) {
  for (int i = 0; i < 9; ++i) if (cov[i] != cov[i]) return false;
  double U[9], S[3], V[9];
  svd3(cov, U, S, V);
  double Vh[9];
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Vh[i * 3 + j] = V[j * 3 + i];
  if (det3(U) * det3(Vh) < 0.0) { S[2] = -S[2]; U[2] = -U[2]; U[5] = -U[5]; U[8] = -U[8]; }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R[i * 3 + j] = U[i * 3] * Vh[j] + U[i * 3 + 1] * Vh[3 + j] + U[i * 3 + 2] * Vh[6 + j];
  scale = 1 / varP * ((S[0] + S[1]) + S[2]);
  for (int j = 0; j < 3; ++j) t[j] = mt[j] - ((ms[0] * (scale * R[j * 3]) + ms[1] * (scale * R[j * 3 + 1])) + ms[2] * (scale * R[j * 3 + 2]));
  return true;
}

// ---- the similarity RANSAC of lib/align.py:44-104, one piece per step --------------------------------------------------------------
// A hypothesis is 13 doubles: s R (row-major), t, and the inlier threshold s * inlier_t.

// Five-point hypothesis (align.py:66-70) from the sampled source rows s and target rows t.  false: NaN covariance (the reference
// raises), hyp is all zero then, so that no row is its inlier.
__device__ inline bool ransac_hypothesis(const double s[5][3], const double t[5][3], double inlier_t, double* hyp /*[13]*/) {
  double ms[3] = {0, 0, 0}, mt[3] = {0, 0, 0};
  for (int k = 0; k < 5; ++k)
    for (int j = 0; j < 3; ++j) { ms[j] += s[k][j]; mt[j] += t[k][j]; }
  for (int j = 0; j < 3; ++j) { ms[j] /= 5; mt[j] /= 5; }
  double cov[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, var = 0.0;
  for (int k = 0; k < 5; ++k) {
    const double cs[3] = {s[k][0] - ms[0], s[k][1] - ms[1], s[k][2] - ms[2]};
    const double ct[3] = {t[k][0] - mt[0], t[k][1] - mt[1], t[k][2] - mt[2]};
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) cov[i * 3 + j] += ct[i] * cs[j];
    var += (cs[0] * cs[0] + cs[1] * cs[1]) + cs[2] * cs[2];
  }
  for (int i = 0; i < 9; ++i) cov[i] /= 5;
  var /= 5;
  double scale, R[9], tr[3];
  const bool ok = umeyama_from_stats(cov, ms, mt, var, scale, R, tr);
  if (!ok) { scale = 0; for (int i = 0; i < 9; ++i) R[i] = 0; tr[0] = tr[1] = tr[2] = 0; }
  for (int i = 0; i < 9; ++i) hyp[i] = scale * R[i];
  hyp[9] = tr[0]; hyp[10] = tr[1]; hyp[11] = tr[2];
  hyp[12] = scale * inlier_t;
  return ok;
}

// Is row (s, t) an inlier of hypothesis m (align.py:71-76): the counting and every inlier pass evaluate this and nothing else
__device__ inline bool ransac_inlier(const double* m /*[13]*/, const double s[3], const double t[3]) {
  const double rx = t[0] - (((m[0] * s[0] + m[1] * s[1]) + m[2] * s[2]) + m[9]);
  const double ry = t[1] - (((m[3] * s[0] + m[4] * s[1]) + m[5] * s[2]) + m[10]);
  const double rz = t[2] - (((m[6] * s[0] + m[7] * s[1]) + m[8] * s[2]) + m[11]);
  return sqrt((rx * rx + ry * ry) + rz * rz) < m[12];
}

// The reference's sequential scan over the inlier counts of `iters` hypotheses among m rows (align.py:77-91): a strictly better ratio
// wins, the confidence rule breaks early, a best ratio < 0.1 keeps none.  Returns the kept hypothesis or -1; examined = the hypotheses
// the sequential loop would have run (0 when m < 5: the reference does not fit fewer than five rows).
__device__ inline int ransac_scan(const int* cnt, int iters, int m, int& examined) {
  double best = 0.0;
  int best_h = -1;
  examined = 0;
  if (m >= 5) {
    for (int i = 0; i < iters; ++i) {
      examined = i + 1;
      const double ratio = (double)cnt[i] / (double)m;
      if (ratio > best) { best = ratio; best_h = i; }
      const double b5 = (best * best) * (best * best) * best;
      if ((1 - pow(1 - b5, (double)i)) > 0.99) break;
    }
  }
  return best < 0.1 ? -1 : best_h;
}

}  // namespace rgbm
