// Multi-view fusion of dense depth maps and the packed point cloud of V views, gfx950.
//
// depth_fusion_kernel: the MVSNet fusion step over V >= 2 views of a pose.  One thread per pixel (x, y) of reference view a with depth
// d; the V views' inverses and extrinsic rows sit in LDS (cloud_geom.h: ViewPose):
//   0. d not finite, d <= 0, or E_a without a finite inverse                               -> keep 0, fused NaN, nviews 0, agree 0
//   1. for the sources b = 0 .. V - 1, b != a, in increasing order: a source whose E_b has no finite inverse does not agree; otherwise
//      rules 2-4 of depth_consistency.hip (cloud_geom.h: reproject_round_trip, the function depth_consistency_kernel calls) give
//      (x', y', d'_b), or no witness; b agrees iff hypot(x' - x, y' - y) < px_max && |d'_b - d| / d < rel_max
//   2. c = the agreeing sources; nviews = c, agree = their bit set                           (written whatever 3 decides)
//   3. keep = c >= n_min && (no conf || conf >= conf_min) && (no mask || mask != 0);
//      fused = keep ? (d + sum of d'_b over the agreeing b, in increasing b) / (1 + c) : NaN
// All in fp64 on the float32 maps, rounded once; built without mul + add contraction (build.sh).  At V = 2, n_min = 1 the sum is d + d'
// and the divisor 2: fused and keep are the bits depth_consistency_kernel writes for the same direction.
//
// cloud_pack_views: cloud_pack_kernel's ordered compaction over V views — view 0's kept pixels in row-major order, then view 1's, ...
// Two launches, no atomics: cloud_count_views_kernel writes count [n][V] (one workgroup per view of a pose), cloud_pack_views_kernel
// cuts every view into `pieces` contiguous pieces, one workgroup each, whose first slot is the counts of the views before its own plus
// the kept pixels of its own view before its piece — a workgroup reads at most one view's keep bytes, whatever V is (cloud_pack_kernel
// reads the whole pose in each of its 8 workgroups).  The walk of a piece, the row and the NaN / -1 fill are the functions
// cloud_pack_kernel calls (cloud_geom.h: pack_walk, pack_emit_row, pack_fill_unused).
//
// cloud_gather_views: cloud_gather_kernel for maps [n][V][S2][C] and indices view * S2 + pixel.
#include <cmath>

#include "cloud_geom.h"
#include "common.h"
#include "kernels.h"

namespace rgbm {

namespace {
constexpr int FUSE_MAX_VIEWS = 16;
constexpr int PACKV_THREADS = 1024;      // 16 waves
constexpr int PACKV_WAVES = PACKV_THREADS / 64;
constexpr int PACKV_PIECE = 16384;       // pixels of a view per workgroup, at least (S = 224: 4 pieces per view, cloud_pack's 8 per pair)
constexpr int PACKV_MAX_PIECES = 64;
}  // namespace

__global__ __launch_bounds__(256) void depth_fusion_kernel(const float* __restrict__ depth, const float* __restrict__ conf,
                                                           const unsigned char* __restrict__ mask, const double* __restrict__ Kc,
                                                           const double* __restrict__ E, int V, int S, double px_max, double rel_max,
                                                           float conf_min, int n_min, float* __restrict__ fused,
                                                           unsigned char* __restrict__ keep, unsigned char* __restrict__ nviews,
                                                           unsigned short* __restrict__ agree) {
  __shared__ ViewPose cam[FUSE_MAX_VIEWS];
  const int pose = blockIdx.y / V, a = blockIdx.y - pose * V;
  const long long v0 = (long long)pose * V;      // first view of the pose
  if ((int)threadIdx.x < V) load_view_pose(v0 + threadIdx.x, E, cam[threadIdx.x]);
  __syncthreads();
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int SS = S * S;
  if (i >= SS) return;
  const long long o = (v0 + a) * SS + i;
  const int y = i / S, x = i - y * S;
  float r_fused = __uint_as_float(0x7fc00000u);
  unsigned char r_keep = 0;
  int c = 0;
  unsigned bits = 0;
  const float df = depth[o];
  if (isfinite(df) && df > 0.f && cam[a].ok) {
    const double d = (double)df;
    const ViewK ka = view_intrinsics(v0 + a, Kc);
    double X[3], sum = d;
    backproject_world(cam[a].inv, (double)x, (double)y, d, ka.fx, ka.fy, ka.cx, ka.cy, X);
    for (int b = 0; b < V; ++b) {
      double e_px, e_rel, dr;
      if (b == a || !cam[b].ok) continue;
      if (!reproject_round_trip(X, (double)x, (double)y, d, cam[a], ka, cam[b], view_intrinsics(v0 + b, Kc), depth + (v0 + b) * SS, S, e_px, e_rel, dr)) continue;
      if (e_px < px_max && e_rel < rel_max) {
        sum += dr;
        ++c;
        bits |= 1u << b;
      }
    }
    const bool k = c >= n_min && (!conf || conf[o] >= conf_min) && (!mask || mask[o] != 0);
    r_keep = k ? 1 : 0;
    if (k) r_fused = (float)(sum / (double)(1 + c));
  }
  fused[o] = r_fused;
  keep[o] = r_keep;
  nviews[o] = (unsigned char)c;
  if (agree) agree[o] = (unsigned short)bits;
}

int launch_depth_fusion(const float* depth, const float* conf, const unsigned char* mask, const double* Kc, const double* E, int n, int V,
                        int S, double px_max, double rel_max, float conf_min, int n_min, float* fused, unsigned char* keep,
                        unsigned char* nviews, unsigned short* agree, hipStream_t s) {
  RGBM_REQUIRE(depth && Kc && E && fused && keep && nviews, "depth_fusion arguments");
  RGBM_REQUIRE(V >= 2 && V <= FUSE_MAX_VIEWS, "depth_fusion: 2 .. 16 views");
  RGBM_REQUIRE(n_min >= 1 && n_min <= V - 1, "depth_fusion: 1 <= n_min <= V - 1");
  RGBM_REQUIRE(n > 0 && (long long)n * V <= 65535 && S > 0 && S <= 4096,
               "depth_fusion: at least one pose, n V <= 65535 views of at most 4096 x 4096 pixels");
  RGBM_REQUIRE(std::isfinite(px_max) && px_max >= 0 && std::isfinite(rel_max) && rel_max >= 0 && std::isfinite(conf_min) && conf_min >= 0,
               "depth_fusion: px_max, rel_max and conf_min are finite and >= 0");
  hipLaunchKernelGGL(depth_fusion_kernel, dim3((unsigned)((S * S + 255) / 256), (unsigned)(n * V)), dim3(256), 0, s, depth, conf, mask, Kc,
                     E, V, S, px_max, rel_max, conf_min, n_min, fused, keep, nviews, agree);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

// count[pose][view] = the view's kept pixels; one workgroup per view (integer sums: the order of the reduction does not matter)
__global__ __launch_bounds__(PACKV_THREADS) void cloud_count_views_kernel(const unsigned char* __restrict__ keep, int SS,
                                                                          int* __restrict__ count) {
  __shared__ int wsum[PACKV_WAVES];
  const long long f = (long long)blockIdx.y * gridDim.x + blockIdx.x;      // pose * V + view
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned char* k = keep + f * SS;
  int c = 0;
  for (int p = tid; p < SS; p += PACKV_THREADS) c += k[p] != 0 ? 1 : 0;
  for (int m = 32; m > 0; m >>= 1) c += __shfl_xor(c, m, 64);
  if (lane == 0) wsum[wave] = c;
  __syncthreads();
  if (tid == 0) {
    int t = 0;
    for (int w = 0; w < PACKV_WAVES; ++w) t += wsum[w];
    count[f] = t;
  }
}

__global__ __launch_bounds__(PACKV_THREADS) void cloud_pack_views_kernel(const float* __restrict__ fused, const unsigned char* __restrict__ keep,
                                                                         const double* __restrict__ Kc, const double* __restrict__ E, int V,
                                                                         int S, int pieces, int cap, const int* __restrict__ count,
                                                                         float* __restrict__ cloud, int* __restrict__ index) {
  __shared__ ViewPose cam;
  __shared__ int wsum[PACKV_WAVES];
  const long long pose = blockIdx.y;
  const int v = blockIdx.x / pieces, j = blockIdx.x - v * pieces;      // blockIdx.x, pieces: uniform over the workgroup
  const long long f = pose * V + v;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int SS = S * S;
  const int piece = (SS + pieces - 1) / pieces;
  const int lo = min(j * piece, SS), hi = min(lo + piece, SS);
  if (tid == 0) load_view_pose(f, E, cam);
  const unsigned char* kv = keep + f * SS;

  // kept pixels of this view before the piece
  int c = 0;
  for (int p = tid; p < lo; p += PACKV_THREADS) c += kv[p] != 0 ? 1 : 0;
  for (int m = 32; m > 0; m >>= 1) c += __shfl_xor(c, m, 64);
  if (lane == 0) wsum[wave] = c;
  __syncthreads();
  int base = 0, total = 0;                          // V S S <= 2^28; sums over all waves and views: the same in every thread
  for (int w = 0; w < PACKV_WAVES; ++w) base += wsum[w];
  for (int w = 0; w < V; ++w) { const int t = count[pose * V + w]; base += w < v ? t : 0; total += t; }
  __syncthreads();      // wsum is the walk's table

  float* cl = cloud + pose * (long long)cap * 3;
  int* ix = index + pose * (long long)cap;
  const ViewK kc = view_intrinsics(f, Kc);
  pack_walk<PACKV_THREADS>(lo, hi, base, cap, wsum, [&](int p) -> bool { return kv[p] != 0; },
                           [&](int slot, int p) { pack_emit_row(cl, ix, slot, v * SS + p, cam, kc, p, S, fused[f * SS + p]); });
  pack_fill_unused(cl, ix, total, cap, (long long)blockIdx.x * PACKV_THREADS + tid, (long long)gridDim.x * PACKV_THREADS);
}

int launch_cloud_pack_views(const float* fused, const unsigned char* keep, const double* Kc, const double* E, int n, int V, int S, int cap,
                            float* cloud, int* index, int* count, hipStream_t s) {
  RGBM_REQUIRE(fused && keep && Kc && E && count, "cloud_pack_views arguments");
  RGBM_REQUIRE(V >= 1 && V <= FUSE_MAX_VIEWS, "cloud_pack_views: 1 .. 16 views");
  RGBM_REQUIRE(n > 0 && n <= 65535 && S > 0 && S <= 4096, "cloud_pack_views: 1 .. 65535 poses of at most 4096 x 4096 pixels");
  RGBM_REQUIRE(cap >= 0, "cloud_pack_views: cap >= 0");
  RGBM_REQUIRE(cap == 0 || (cloud && index), "cloud_pack_views: cloud and index are NULL");
  const int SS = S * S;
  int pieces = (SS + PACKV_PIECE - 1) / PACKV_PIECE;
  if (pieces > PACKV_MAX_PIECES) pieces = PACKV_MAX_PIECES;
  hipLaunchKernelGGL(cloud_count_views_kernel, dim3((unsigned)V, (unsigned)n), dim3(PACKV_THREADS), 0, s, keep, SS, count);
  RGBM_CHECK_HIP(hipGetLastError());
  if (cap > 0) {
    hipLaunchKernelGGL(cloud_pack_views_kernel, dim3((unsigned)(V * pieces), (unsigned)n), dim3(PACKV_THREADS), 0, s, fused, keep, Kc, E, V,
                       S, pieces, cap, count, cloud, index);
    RGBM_CHECK_HIP(hipGetLastError());
  }
  return 0;
}

// out[i][r][c] = maps[i][index / S2][index % S2][c]; NaN rows for an index outside [0, V S2)
__global__ __launch_bounds__(256) void cloud_gather_views_kernel(const float* __restrict__ maps, const int* __restrict__ index, long long rows,
                                                                 long long VS2, int C, int cap, float* __restrict__ out) {
  for (long long r = blockIdx.x * (long long)blockDim.x + threadIdx.x; r < rows; r += (long long)gridDim.x * blockDim.x) {
    const long long i = r / cap;
    const int ix = index[r];
    const float* src = ix >= 0 && (long long)ix < VS2 ? maps + (i * VS2 + ix) * C : nullptr;
    for (int c = 0; c < C; ++c) out[r * C + c] = src ? src[c] : __builtin_nanf("");
  }
}

int launch_cloud_gather_views(const float* maps, const int* index, int n, int V, int S2, int C, int cap, float* out, hipStream_t s) {
  RGBM_REQUIRE(n >= 0 && V >= 1 && V <= FUSE_MAX_VIEWS && S2 > 0 && S2 <= 4096 * 4096 && cap >= 0 && C >= 1 && C <= 4,
               "cloud_gather_views: n >= 0, 1 <= V <= 16, 0 < S2 <= 4096 x 4096, cap >= 0, 1 <= C <= 4");
  const long long rows = (long long)n * cap;
  if (rows == 0) return 0;
  RGBM_REQUIRE(maps && index && out, "cloud_gather_views arguments");
  const long long g = (rows + 255) / 256;
  hipLaunchKernelGGL(cloud_gather_views_kernel, dim3((unsigned)(g < 65536 ? g : 65536)), dim3(256), 0, s, maps, index, rows,
                     (long long)V * S2, C, cap, out);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace rgbm
