// A box fitted to the two-view cloud: rgbm_cloud_gather looks the packed cloud's rows up in per-pixel maps (the
// dense NOCS map), rgbm_cloud_similarity runs the reference's similarity RANSAC
//   models/pose_estimator/AdaPose/lib/align.py:10-41    estimateSimilarityUmeyama
//   models/pose_estimator/AdaPose/lib/align.py:44-104   estimateSimilarityTransform (RANSAC)
//   models/pose_estimator/AdaPose/interface_v5.py:348-374  bbox from (s, R, t), default bbox
// on up to 2 S S rows per pose where align.hip runs it on 1024.  The rows (2.4 MB per pose at the cap) do not fit the LDS: every pass
// streams them from memory as fp32 and converts on the fly; a pose's rows are cut into CF_SLICES(cap) slices of whole workgroups, so that
// 8 poses fill the device.  What the slices produce is combined without floating-point atomics: inlier counts are integers (ballot +
// popcount, integer adds are order-free), fp64 partial sums go to scratch and are added in slice order by whoever needs them.  Results are
// bit-identical from run to run.
//   1 cf_sum         per slice: sum of the NOCS rows, max |nocs| per axis, NaN anywhere in the m rows of either array
//   2 cf_far         per slice: largest distance of a NOCS row to the centroid  (threshold = 2 max / 10, align.py:52-57)
//   3 cf_hypotheses  per pose: 128 five-point Umeyama fits, one per thread; sample k of hypothesis i = mix32(seed, 128 b + i, k) mod m
//   4 cf_count       per slice: inliers of every hypothesis among the slice's rows (hypothesis table in LDS)
//   5 cf_scan        per pose: the reference's sequential scan over the 128 counts (strictly better ratio, confidence break, < 0.1: none)
//   6 cf_inlier_sum  per slice: count and coordinate sums of the kept hypothesis's inliers
//   7 cf_inlier_cov  per slice: their covariance and source variance about the centroids
//   8 cf_finish      per pose: Umeyama over the inliers, the box (no world transform: the cloud is in the world frame), srt, info, valid
// Steps 3, 4 / 6 / 7 and 5 call align_math.h's ransac_hypothesis, ransac_inlier and ransac_scan, the ones umeyama_ransac_kernel (align.hip)
// runs on its 1024 rows in LDS; the box corners and the default box are bbox_emit.h's, the hash and the block reductions common.h's.
#include "common.h"
#include "kernels.h"
#include "bbox_emit.h"
#include "align_math.h"

#pragma clang fp contract(off)

namespace rgbm {

namespace {

constexpr int CF_THREADS = 256;
constexpr int CF_ITERS = 128;
constexpr int CF_SLICE_ROWS = 4096;      // rows of a slice: 16 per thread
constexpr int CF_MAX_SLICES = 64;

// per-pose scratch, in doubles: [sum NS*8][far NS][hyp 128*13][isum NS*8][icov NS*10][ints: cnt NS*128, sel 8]
struct CfLayout {
  int ns;
  size_t o_sum, o_far, o_hyp, o_isum, o_icov, o_int, per_pose;      // offsets in doubles
};
__host__ __device__ inline int cf_slices(int cap) {
  const int ns = (cap + CF_SLICE_ROWS - 1) / CF_SLICE_ROWS;
  return ns < 1 ? 1 : (ns > CF_MAX_SLICES ? CF_MAX_SLICES : ns);
}
__host__ __device__ inline CfLayout cf_layout(int cap) {
  CfLayout L;
  L.ns = cf_slices(cap);
  const size_t ns = (size_t)L.ns;
  L.o_sum = 0;
  L.o_far = L.o_sum + ns * 8;
  L.o_hyp = L.o_far + ns;
  L.o_isum = L.o_hyp + (size_t)CF_ITERS * 13;
  L.o_icov = L.o_isum + ns * 8;
  L.o_int = L.o_icov + ns * 10;
  L.per_pose = L.o_int + (ns * CF_ITERS + 8 + 1) / 2;
  return L;
}
// sel (ints behind the slices' counts): 0 m, 1 kept hypothesis or -1, 2 its inlier count, 3 hypotheses examined, 4 a hypothesis had a NaN covariance

__device__ inline int cf_rows(const int* __restrict__ count, int b, int cap) {
  const long long c = (long long)count[2 * b] + (long long)count[2 * b + 1];
  return (int)(c < 0 ? 0 : (c > cap ? cap : c));
}
// rows [r0, r1) of slice sl: the cut depends on cap alone
__device__ inline void cf_range(int cap, int ns, int sl, int m, int& r0, int& r1) {
  const int len = (cap + ns - 1) / ns;
  r0 = sl * len; r1 = r0 + len;
  if (r0 > m) r0 = m;
  if (r1 > m) r1 = m;
}

__device__ inline void cf_row(const float* __restrict__ a, long long row, double v[3]) {
  const float* p = a + row * 3;
  v[0] = (double)p[0]; v[1] = (double)p[1]; v[2] = (double)p[2];
}

}  // namespace

// ---------------------------------------------------------------- gather
// out[i][r][c] = map{1 + index / S2}[i][index % S2][c]; NaN rows for index < 0, index >= 2 S2, or view 2 without map2
__global__ __launch_bounds__(256) void cloud_gather_kernel(const float* __restrict__ map1, const float* __restrict__ map2,
                                                           const int* __restrict__ index, long long rows, int S2, int C, int cap,
                                                           float* __restrict__ out) {
  for (long long r = blockIdx.x * (long long)blockDim.x + threadIdx.x; r < rows; r += (long long)gridDim.x * blockDim.x) {
    const long long i = r / cap;
    const int ix = index[r];
    const float* src = nullptr;
    if (ix >= 0 && ix < S2) src = map1 + (i * S2 + ix) * C;
    else if (ix >= S2 && (long long)ix < 2ll * S2 && map2 != nullptr) src = map2 + (i * S2 + (ix - S2)) * C;
    for (int c = 0; c < C; ++c) out[r * C + c] = src ? src[c] : __builtin_nanf("");
  }
}

int launch_cloud_gather(const float* map1, const float* map2, const int* index, int n, int S2, int C, int cap, float* out, hipStream_t s) {
  RGBM_REQUIRE(n >= 0 && S2 > 0 && cap >= 0 && C >= 1 && C <= 4, "cloud_gather: n >= 0, S2 > 0, cap >= 0, 1 <= C <= 4");
  const long long rows = (long long)n * cap;
  if (rows == 0) return 0;
  RGBM_REQUIRE(map1 && index && out, "cloud_gather arguments");
  const long long g = (rows + 255) / 256;
  hipLaunchKernelGGL(cloud_gather_kernel, dim3((unsigned)(g < 65536 ? g : 65536)), dim3(256), 0, s, map1, map2, index, rows, S2, C, cap, out);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------- similarity fit
__global__ __launch_bounds__(CF_THREADS) void cf_sum_kernel(const float* __restrict__ nocs, const float* __restrict__ cloud,
                                                            const int* __restrict__ count, int cap, double* __restrict__ scratch) {
  __shared__ double red[CF_THREADS];
  const CfLayout L = cf_layout(cap);
  const int b = blockIdx.y, sl = blockIdx.x, t = threadIdx.x;
  const int m = cf_rows(count, b, cap);
  int r0, r1;
  cf_range(cap, L.ns, sl, m, r0, r1);
  double a[3] = {0, 0, 0}, h[3] = {0, 0, 0}, bad = 0;
  for (int p = r0 + t; p < r1; p += CF_THREADS) {
    double s[3], w[3];
    cf_row(nocs, (long long)b * cap + p, s);
    cf_row(cloud, (long long)b * cap + p, w);
    for (int j = 0; j < 3; ++j) {
      a[j] += s[j];
      h[j] = fmax(h[j], fabs(s[j]));      // fmax drops a NaN operand: NaN rows are caught by `bad`
      if (s[j] != s[j] || w[j] != w[j]) bad = 1;
    }
  }
  double* o = scratch + (size_t)b * L.per_pose + L.o_sum + (size_t)sl * 8;
  for (int j = 0; j < 3; ++j) {
    const double sj = block_sum<CF_THREADS>(a[j], red), hj = block_max<CF_THREADS>(h[j], red);
    if (t == 0) { o[j] = sj; o[3 + j] = hj; }
  }
  const double bd = block_max<CF_THREADS>(bad, red);
  if (t == 0) { o[6] = bd; o[7] = 0; }
}

// centroid of the m NOCS rows from the slices' sums, in slice order
__device__ inline void cf_centroid(const double* __restrict__ pose, const CfLayout& L, int m, double c[3]) {
  for (int j = 0; j < 3; ++j) {
    double a = 0;
    for (int sl = 0; sl < L.ns; ++sl) a += pose[L.o_sum + (size_t)sl * 8 + j];
    c[j] = a / m;
  }
}

__global__ __launch_bounds__(CF_THREADS) void cf_far_kernel(const float* __restrict__ nocs, const int* __restrict__ count, int cap,
                                                            double* __restrict__ scratch) {
  __shared__ double red[CF_THREADS];
  const CfLayout L = cf_layout(cap);
  const int b = blockIdx.y, sl = blockIdx.x, t = threadIdx.x;
  const int m = cf_rows(count, b, cap);
  double* pose = scratch + (size_t)b * L.per_pose;
  int r0, r1;
  cf_range(cap, L.ns, sl, m, r0, r1);
  double c[3] = {0, 0, 0};
  if (m > 0) cf_centroid(pose, L, m, c);
  double far = 0.0;
  for (int p = r0 + t; p < r1; p += CF_THREADS) {
    double s[3];
    cf_row(nocs, (long long)b * cap + p, s);
    const double dx = s[0] - c[0], dy = s[1] - c[1], dz = s[2] - c[2];
    far = fmax(far, sqrt((dx * dx + dy * dy) + dz * dz));
  }
  far = block_max<CF_THREADS>(far, red);
  if (t == 0) pose[L.o_far + sl] = far;
}

__global__ __launch_bounds__(CF_ITERS) void cf_hypotheses_kernel(const float* __restrict__ nocs, const float* __restrict__ cloud,
                                                                 const int* __restrict__ count, int cap, unsigned seed,
                                                                 double* __restrict__ scratch) {
  __shared__ int s_fail;
  const CfLayout L = cf_layout(cap);
  const int b = blockIdx.x, t = threadIdx.x;
  const int m = cf_rows(count, b, cap);
  double* pose = scratch + (size_t)b * L.per_pose;
  int* sel = reinterpret_cast<int*>(pose + L.o_int) + (size_t)L.ns * CF_ITERS;
  if (t == 0) s_fail = 0;
  __syncthreads();
  double* hy = pose + L.o_hyp + (size_t)t * 13;
  if (m >= 5) {
    double far = 0.0;
    for (int sl = 0; sl < L.ns; ++sl) far = fmax(far, pose[L.o_far + sl]);
    const double inlier_t = 2 * far / 10.0;
    double sv[5][3], tv[5][3];
    for (int k = 0; k < 5; ++k) {
      const int idx = (int)(mix32(seed, (unsigned)b * CF_ITERS + t, k) % (unsigned)m);
      cf_row(nocs, (long long)b * cap + idx, sv[k]);
      cf_row(cloud, (long long)b * cap + idx, tv[k]);
    }
    if (!ransac_hypothesis(sv, tv, inlier_t, hy)) atomicOr(&s_fail, 1);
  } else {
    for (int i = 0; i < 13; ++i) hy[i] = 0.0;
  }
  __syncthreads();
  if (t == 0) { sel[0] = m; sel[4] = s_fail; }
}

__global__ __launch_bounds__(CF_THREADS) void cf_count_kernel(const float* __restrict__ nocs, const float* __restrict__ cloud,
                                                              const int* __restrict__ count, int cap, double* __restrict__ scratch) {
  __shared__ double hyp[CF_ITERS * 13];
  __shared__ int cnt[CF_ITERS];
  const CfLayout L = cf_layout(cap);
  const int b = blockIdx.y, sl = blockIdx.x, t = threadIdx.x, lane = t & 63;
  const int m = cf_rows(count, b, cap);
  double* pose = scratch + (size_t)b * L.per_pose;
  for (int i = t; i < CF_ITERS * 13; i += CF_THREADS) hyp[i] = pose[L.o_hyp + i];
  if (t < CF_ITERS) cnt[t] = 0;
  __syncthreads();
  int r0, r1;
  cf_range(cap, L.ns, sl, m, r0, r1);
  // four rows per thread against every hypothesis: one broadcast read of a hypothesis serves 256 rows of the wave
  for (int base = r0; base < r1; base += 4 * CF_THREADS) {      // uniform over the workgroup
    double s[4][3], w[4][3];
    bool in[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int p = base + q * CF_THREADS + t;
      in[q] = p < r1;
      const long long row = (long long)b * cap + (in[q] ? p : r0);
      cf_row(nocs, row, s[q]);
      cf_row(cloud, row, w[q]);
    }
    for (int h = 0; h < CF_ITERS; ++h) {
      const double* mh = hyp + h * 13;
      int c = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) c += __popcll(__ballot(in[q] && ransac_inlier(mh, s[q], w[q])));
      if (lane == 0 && c) atomicAdd(&cnt[h], c);      // integer: order-free
    }
  }
  __syncthreads();
  int* cn = reinterpret_cast<int*>(pose + L.o_int) + (size_t)sl * CF_ITERS;
  if (t < CF_ITERS) cn[t] = cnt[t];
}

__global__ __launch_bounds__(CF_ITERS) void cf_scan_kernel(int cap, double* __restrict__ scratch) {
  __shared__ int cnt[CF_ITERS];
  const CfLayout L = cf_layout(cap);
  const int b = blockIdx.x, t = threadIdx.x;
  double* pose = scratch + (size_t)b * L.per_pose;
  const int* cn = reinterpret_cast<const int*>(pose + L.o_int);
  int* sel = reinterpret_cast<int*>(pose + L.o_int) + (size_t)L.ns * CF_ITERS;
  int c = 0;
  for (int sl = 0; sl < L.ns; ++sl) c += cn[(size_t)sl * CF_ITERS + t];
  cnt[t] = c;
  __syncthreads();
  if (t == 0) {
    int examined;
    const int best_h = ransac_scan(cnt, CF_ITERS, sel[0], examined);
    sel[1] = best_h;
    sel[2] = best_h >= 0 ? cnt[best_h] : 0;
    sel[3] = examined;
  }
}

__global__ __launch_bounds__(CF_THREADS) void cf_inlier_sum_kernel(const float* __restrict__ nocs, const float* __restrict__ cloud,
                                                                   const int* __restrict__ count, int cap, double* __restrict__ scratch) {
  __shared__ double red[CF_THREADS];
  __shared__ double mh[13];
  const CfLayout L = cf_layout(cap);
  const int b = blockIdx.y, sl = blockIdx.x, t = threadIdx.x;
  const int m = cf_rows(count, b, cap);
  double* pose = scratch + (size_t)b * L.per_pose;
  const int* sel = reinterpret_cast<const int*>(pose + L.o_int) + (size_t)L.ns * CF_ITERS;
  const int best_h = sel[1];
  if (t < 13) mh[t] = best_h >= 0 ? pose[L.o_hyp + (size_t)best_h * 13 + t] : 0.0;
  __syncthreads();
  int r0, r1;
  cf_range(cap, L.ns, sl, m, r0, r1);
  double acc[7] = {0, 0, 0, 0, 0, 0, 0};
  if (best_h >= 0) {
    for (int p = r0 + t; p < r1; p += CF_THREADS) {
      double s[3], w[3];
      cf_row(nocs, (long long)b * cap + p, s);
      cf_row(cloud, (long long)b * cap + p, w);
      if (ransac_inlier(mh, s, w)) { acc[0] += 1; for (int j = 0; j < 3; ++j) { acc[1 + j] += s[j]; acc[4 + j] += w[j]; } }
    }
  }
  double* o = pose + L.o_isum + (size_t)sl * 8;
  for (int j = 0; j < 7; ++j) {
    const double v = block_sum<CF_THREADS>(acc[j], red);
    if (t == 0) o[j] = v;
  }
  if (t == 0) o[7] = 0;
}

// n, centroids of the inliers from the slices' sums, in slice order
__device__ inline void cf_inlier_means(const double* __restrict__ pose, const CfLayout& L, double& n, double ms[3], double mt[3]) {
  double a[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int sl = 0; sl < L.ns; ++sl)
    for (int j = 0; j < 7; ++j) a[j] += pose[L.o_isum + (size_t)sl * 8 + j];
  n = a[0];
  for (int j = 0; j < 3; ++j) { ms[j] = a[1 + j] / n; mt[j] = a[4 + j] / n; }
}

__global__ __launch_bounds__(CF_THREADS) void cf_inlier_cov_kernel(const float* __restrict__ nocs, const float* __restrict__ cloud,
                                                                   const int* __restrict__ count, int cap, double* __restrict__ scratch) {
  __shared__ double red[CF_THREADS];
  __shared__ double mh[13];
  const CfLayout L = cf_layout(cap);
  const int b = blockIdx.y, sl = blockIdx.x, t = threadIdx.x;
  const int m = cf_rows(count, b, cap);
  double* pose = scratch + (size_t)b * L.per_pose;
  const int* sel = reinterpret_cast<const int*>(pose + L.o_int) + (size_t)L.ns * CF_ITERS;
  const int best_h = sel[1];
  if (t < 13) mh[t] = best_h >= 0 ? pose[L.o_hyp + (size_t)best_h * 13 + t] : 0.0;
  __syncthreads();
  int r0, r1;
  cf_range(cap, L.ns, sl, m, r0, r1);
  double acc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (best_h >= 0) {
    double n, ms[3], mt[3];
    cf_inlier_means(pose, L, n, ms, mt);
    for (int p = r0 + t; p < r1; p += CF_THREADS) {
      double s[3], w[3];
      cf_row(nocs, (long long)b * cap + p, s);
      cf_row(cloud, (long long)b * cap + p, w);
      if (!ransac_inlier(mh, s, w)) continue;
      const double cs[3] = {s[0] - ms[0], s[1] - ms[1], s[2] - ms[2]};
      const double ct[3] = {w[0] - mt[0], w[1] - mt[1], w[2] - mt[2]};
      for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) acc[i * 3 + j] += ct[i] * cs[j];
      acc[9] += (cs[0] * cs[0] + cs[1] * cs[1]) + cs[2] * cs[2];
    }
  }
  double* o = pose + L.o_icov + (size_t)sl * 10;
  for (int j = 0; j < 10; ++j) {
    const double v = block_sum<CF_THREADS>(acc[j], red);
    if (t == 0) o[j] = v;
  }
}

__global__ void cf_finish_kernel(int n, int cap, const double* __restrict__ scratch, double* __restrict__ bbox, double* __restrict__ srt,
                                 int* __restrict__ info, int* __restrict__ valid) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  const CfLayout L = cf_layout(cap);
  const double* pose = scratch + (size_t)b * L.per_pose;
  const int* sel = reinterpret_cast<const int*>(pose + L.o_int) + (size_t)L.ns * CF_ITERS;
  const int m = sel[0], best_h = sel[1];
  double bad = 0, hmax[3] = {0, 0, 0};
  for (int sl = 0; sl < L.ns; ++sl) {
    bad = fmax(bad, pose[L.o_sum + (size_t)sl * 8 + 6]);
    for (int j = 0; j < 3; ++j) hmax[j] = fmax(hmax[j], pose[L.o_sum + (size_t)sl * 8 + 3 + j]);
  }
  const bool usable = m >= 5 && bad == 0.0 && sel[4] == 0;      // (a hypothesis with a NaN covariance: the reference raises)
  double scale = 0, R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, tr[3] = {0, 0, 0};
  bool ok = usable && best_h >= 0;
  if (ok) {
    double nin, ms[3], mt[3], cov[9], var = 0;
    cf_inlier_means(pose, L, nin, ms, mt);
    for (int i = 0; i < 10; ++i) {
      double a = 0;
      for (int sl = 0; sl < L.ns; ++sl) a += pose[L.o_icov + (size_t)sl * 10 + i];
      if (i < 9) cov[i] = a / nin; else var = a / nin;
    }
    ok = umeyama_from_stats(cov, ms, mt, var, scale, R, tr);
  }
  double* o = srt + (long long)b * 13;
  o[0] = ok ? scale : __builtin_nan("");
  for (int i = 0; i < 9; ++i) o[1 + i] = R[i];
  for (int i = 0; i < 3; ++i) o[10 + i] = tr[i];
  info[4 * b + 0] = m;
  info[4 * b + 1] = usable ? best_h : -1;
  info[4 * b + 2] = usable ? sel[2] : 0;
  info[4 * b + 3] = usable ? sel[3] : 0;
  // sRT is a float32 matrix in the reference (interface_v5.py:357-361): R and t are rounded to float32 there
  double Rf[9], corner[8][3];
  for (int i = 0; i < 9; ++i) Rf[i] = (double)(float)R[i];
  const float tf[3] = {(float)tr[0], (float)tr[1], (float)tr[2]};
  const double size[3] = {2.0 * hmax[0] * scale, 2.0 * hmax[1] * scale, 2.0 * hmax[2] * scale};
  bbox_corners_srt(Rf, tf, size, corner);
  for (int k = 0; k < 8; ++k)
    for (int i = 0; i < 3; ++i)
      if (!isfinite(corner[k][i])) ok = false;
  if (!ok) o[0] = __builtin_nan("");
  emit_corners(b, corner, ok, bbox, valid);      // no world transform: the cloud is in the world frame
}

size_t cloud_similarity_scratch_bytes(int n, int cap) {
  return (size_t)(n > 0 ? n : 0) * cf_layout(cap).per_pose * sizeof(double);
}

int launch_cloud_similarity(const float* nocs, const float* cloud, const int* count, int n, int cap, unsigned seed, double* bbox, double* srt,
                            int* info, int* valid, void* scratch, size_t scratch_bytes, hipStream_t s) {
  RGBM_REQUIRE(n >= 0 && cap >= 1, "cloud_similarity: n >= 0, cap >= 1");
  if (n == 0) return 0;
  RGBM_REQUIRE(nocs && cloud && count && bbox && srt && info && valid && scratch, "cloud_similarity arguments");
  RGBM_REQUIRE(((uintptr_t)scratch & 7) == 0 && scratch_bytes >= cloud_similarity_scratch_bytes(n, cap),
               "cloud_similarity: scratch too small or not 8-byte aligned (rgbm_cloud_similarity_scratch_bytes)");
  RGBM_REQUIRE(n <= 65535, "cloud_similarity: at most 65535 poses per call");
  double* sc = reinterpret_cast<double*>(scratch);
  const dim3 gs((unsigned)cf_slices(cap), (unsigned)n), gp((unsigned)n);
  hipLaunchKernelGGL(cf_sum_kernel, gs, dim3(CF_THREADS), 0, s, nocs, cloud, count, cap, sc);
  hipLaunchKernelGGL(cf_far_kernel, gs, dim3(CF_THREADS), 0, s, nocs, count, cap, sc);
  hipLaunchKernelGGL(cf_hypotheses_kernel, gp, dim3(CF_ITERS), 0, s, nocs, cloud, count, cap, seed, sc);
  hipLaunchKernelGGL(cf_count_kernel, gs, dim3(CF_THREADS), 0, s, nocs, cloud, count, cap, sc);
  hipLaunchKernelGGL(cf_scan_kernel, gp, dim3(CF_ITERS), 0, s, cap, sc);
  hipLaunchKernelGGL(cf_inlier_sum_kernel, gs, dim3(CF_THREADS), 0, s, nocs, cloud, count, cap, sc);
  hipLaunchKernelGGL(cf_inlier_cov_kernel, gs, dim3(CF_THREADS), 0, s, nocs, cloud, count, cap, sc);
  hipLaunchKernelGGL(cf_finish_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, n, cap, sc, bbox, srt, info, valid);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace rgbm
