// Statistics over S Dropout2d samples per pose (gfx950): what AdaPoseEstimator_v5.estimate_samples makes of the S boxes and the S
// NOCS / depth rows that one AdaPoseNet.forward_samples gives for every pose.  float64 numpy twins:
// rgbmanip_amd/samples.py (box_stats_ref, point_stats_ref), which sum in the same order.
//
// sample_box_stats_kernel: one workgroup (one wavefront) per pose.  The pose's S boxes are staged in LDS; lane s decides whether sample
// s counts (ok set and its 24 coordinates finite) and derives the sample's centre, its three edge lengths and unit edge vectors; one
// ballot gives the set of counted samples.  Every statistic element then belongs to one lane, which walks the counted samples in
// ascending s twice (mean, then deviations from it): the summation order is fixed by the data layout alone - no atomics, and no
// order that depends on which lane finishes first.  count = 0 leaves 0 / 0 = NaN in every statistic; count = 1 gives deviations
// x - x / 1 = 0 exactly.
//   edges: the three that leave corner 0 of get_3d_bbox (lib/utils.py:49-56; bbox_emit.h: bbox_sign), in the order x, y, z of the
//   box frame, i.e. to corners 2, 4 and 1.
//   axis_spread_deg[e]: sqrt(mean_s angle_s^2) in degrees, angle_s = acos(clamp(u_s . m, -1, 1)), u_s the sample's unit edge vector
//   and m the normalised sum of the counted u_s.  One counted sample has no spread: 0 is written, not acos of a dot product that
//   rounding may leave an ulp under 1 (acos(1 - 2^-53) is 1.5e-8 rad).
// sample_point_stats_kernel: one element of [n][M] per thread and grid stride, the S values read twice with unit stride across lanes
// (4-byte loads, 256 B per wavefront instruction; the second pass is served from cache: S n M 4 bytes are a few MB in the estimator).
// Built with -ffp-contract=off: the twins round every product and sum.
#include "sample_stats.h"

#pragma clang fp contract(off)

namespace rgbm {

namespace {

constexpr int SB_THREADS = 64;

struct SampleBoxOut {
  int* count;
  double *bbox_mean, *bbox_std, *center_mean, *center_cov, *extent_mean, *extent_std, *axis_spread_deg;
};

// sum over the counted samples (bits of `mask`, ascending) of v[s * stride]
__device__ __forceinline__ double sum_counted(const double* v, int stride, unsigned long long mask) {
  double a = 0.0;
  for (unsigned long long m = mask; m; m &= m - 1) a += v[(__ffsll((long long)m) - 1) * stride];
  return a;
}
// ... and of (v - mv)(w - mw)
__device__ __forceinline__ double sum_dev2(const double* v, double mv, const double* w, double mw, int stride, unsigned long long mask) {
  double a = 0.0;
  for (unsigned long long m = mask; m; m &= m - 1) {
    const int s = __ffsll((long long)m) - 1;
    a += (v[s * stride] - mv) * (w[s * stride] - mw);
  }
  return a;
}

__global__ __launch_bounds__(SB_THREADS) void sample_box_stats_kernel(const double* __restrict__ boxes /*[S][n][24]*/,
                                                                      const unsigned char* __restrict__ ok /*[S][n]*/, int n, int S,
                                                                      const SampleBoxOut o) {
  __shared__ double box[kSampleMax][24];
  __shared__ double ctr[kSampleMax][3];
  __shared__ double len[kSampleMax][3];
  __shared__ double unit[kSampleMax][9];      // [edge][xyz]
  const long long b = blockIdx.x;
  const int t = threadIdx.x;
  for (int i = t; i < S * 24; i += SB_THREADS) {
    const int s = i / 24, k = i - s * 24;
    box[s][k] = boxes[((long long)s * n + b) * 24 + k];
  }
  __syncthreads();
  bool counted = false;
  if (t < S) {
    counted = ok[(long long)t * n + b] != 0;
    for (int k = 0; k < 24; ++k) counted = counted && isfinite(box[t][k]);
    for (int i = 0; i < 3; ++i) {
      double a = 0.0;
      for (int k = 0; k < 8; ++k) a += box[t][k * 3 + i];
      ctr[t][i] = a / 8.0;
    }
    const int far[3] = {2, 4, 1};      // the corner at the far end of edge e from corner 0
    for (int e = 0; e < 3; ++e) {
      const double v0 = box[t][far[e] * 3 + 0] - box[t][0], v1 = box[t][far[e] * 3 + 1] - box[t][1],
                   v2 = box[t][far[e] * 3 + 2] - box[t][2];
      const double l = sqrt(v0 * v0 + v1 * v1 + v2 * v2);
      len[t][e] = l;
      unit[t][e * 3 + 0] = v0 / l; unit[t][e * 3 + 1] = v1 / l; unit[t][e * 3 + 2] = v2 / l;
    }
  }
  const unsigned long long mask = __ballot(counted);
  const int cnt = __popcll(mask);
  const double dc = (double)cnt;
  __syncthreads();
  if (t == 0) o.count[b] = cnt;
  if (t < 24) {
    const double m = sum_counted(&box[0][t], 24, mask) / dc;
    o.bbox_mean[b * 24 + t] = m;
    o.bbox_std[b * 24 + t] = sqrt(sum_dev2(&box[0][t], m, &box[0][t], m, 24, mask) / dc);
  } else if (t < 27) {
    const int i = t - 24;
    o.center_mean[b * 3 + i] = sum_counted(&ctr[0][i], 3, mask) / dc;
  } else if (t < 36) {
    const int i = (t - 27) / 3, j = (t - 27) % 3;
    const double mi = sum_counted(&ctr[0][i], 3, mask) / dc, mj = sum_counted(&ctr[0][j], 3, mask) / dc;
    o.center_cov[b * 9 + (t - 27)] = sum_dev2(&ctr[0][i], mi, &ctr[0][j], mj, 3, mask) / dc;
  } else if (t < 39) {
    const int e = t - 36;
    const double m = sum_counted(&len[0][e], 3, mask) / dc;
    o.extent_mean[b * 3 + e] = m;
    o.extent_std[b * 3 + e] = sqrt(sum_dev2(&len[0][e], m, &len[0][e], m, 3, mask) / dc);
  } else if (t < 42) {
    const int e = t - 39;
    const double* u = &unit[0][e * 3];
    const double m0 = sum_counted(u + 0, 9, mask), m1 = sum_counted(u + 1, 9, mask), m2 = sum_counted(u + 2, 9, mask);
    double spread;
    if (cnt == 1) {
      spread = 0.0 * ((m0 + m1) + m2);      // 0, or NaN for an edge of no length
    } else {
      const double l = sqrt(m0 * m0 + m1 * m1 + m2 * m2);
      const double d0 = m0 / l, d1 = m1 / l, d2 = m2 / l;
      double a = 0.0;
      for (unsigned long long m = mask; m; m &= m - 1) {
        const int s = __ffsll((long long)m) - 1;
        double c = u[s * 9 + 0] * d0 + u[s * 9 + 1] * d1 + u[s * 9 + 2] * d2;
        c = c > 1.0 ? 1.0 : c < -1.0 ? -1.0 : c;      // NaN stays NaN
        const double ang = acos(c);
        a += ang * ang;
      }
      spread = sqrt(a / dc) * (180.0 / 3.14159265358979323846);
    }
    o.axis_spread_deg[b * 3 + e] = spread;
  }
}

constexpr int SP_THREADS = 256;

__global__ __launch_bounds__(SP_THREADS) void sample_point_stats_kernel(const float* __restrict__ x /*[S][N]*/, long long N, int S,
                                                                        float* __restrict__ mean, float* __restrict__ std) {
  const double dS = (double)S;
  for (long long i = blockIdx.x * (long long)SP_THREADS + threadIdx.x; i < N; i += (long long)gridDim.x * SP_THREADS) {
    double a = 0.0;
    for (int s = 0; s < S; ++s) a += (double)x[(long long)s * N + i];
    const double m = a / dS;
    double q = 0.0;
    for (int s = 0; s < S; ++s) {
      const double d = (double)x[(long long)s * N + i] - m;
      q += d * d;
    }
    mean[i] = (float)m;
    std[i] = (float)sqrt(q / dS);
  }
}

__global__ __launch_bounds__(256) void tile_words_kernel(const unsigned* __restrict__ src, unsigned* __restrict__ dst, long long words, int S) {
  const long long total = words * S;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) dst[i] = src[i % words];
}

unsigned stride_grid(long long items, int threads) {
  const long long g = (items + threads - 1) / threads;
  return (unsigned)(g < 1 ? 1 : g < 2048 ? g : 2048);
}

}  // namespace

int launch_sample_box_stats(const double* boxes, const unsigned char* ok, int n, int S, int* count, double* bbox_mean, double* bbox_std,
                            double* center_mean, double* center_cov, double* extent_mean, double* extent_std, double* axis_spread_deg,
                            hipStream_t s) {
  RGBM_REQUIRE(boxes && ok && count && bbox_mean && bbox_std && center_mean && center_cov && extent_mean && extent_std && axis_spread_deg,
               "sample_box_stats arguments");
  RGBM_REQUIRE(S >= 1 && S <= kSampleMax, "sample_box_stats: 1 <= S <= 64 samples");
  RGBM_REQUIRE(n >= 1 && n <= kSampleBoxPoses, "sample_box_stats: 1 <= n <= 65535 poses");
  const SampleBoxOut o{count, bbox_mean, bbox_std, center_mean, center_cov, extent_mean, extent_std, axis_spread_deg};
  hipLaunchKernelGGL(sample_box_stats_kernel, dim3((unsigned)n), dim3(SB_THREADS), 0, s, boxes, ok, n, S, o);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_sample_point_stats(const float* x, int n, int S, long long M, float* mean, float* std, hipStream_t s) {
  RGBM_REQUIRE(x && mean && std, "sample_point_stats arguments");
  RGBM_REQUIRE(S >= 1 && n >= 1 && M >= 1, "sample_point_stats: S, n and M must be positive");
  RGBM_REQUIRE((long long)n * M <= (1ll << 40) / S, "sample_point_stats: too many elements");
  const long long N = (long long)n * M;
  hipLaunchKernelGGL(sample_point_stats_kernel, dim3(stride_grid(N, SP_THREADS)), dim3(SP_THREADS), 0, s, x, N, S, mean, std);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_tile_words(const void* src, void* dst, long long words, int S, hipStream_t s) {
  RGBM_REQUIRE(src && dst && words >= 1 && S >= 1, "tile_words arguments");
  hipLaunchKernelGGL(tile_words_kernel, dim3(stride_grid(words * S, 256)), dim3(256), 0, s, (const unsigned*)src, (unsigned*)dst, words, S);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace rgbm
