// Procedural camera for the synthetic MultiVecEnv stand-in: there is no simulator on the GPU box, so the
// controller benchmark / tests render what `MultiVecEnv.get_image()` (env/my_vec_env.py:266, base_manipulation.py:653-687)
// would hand over — a 480x640 colour frame, the handle mask, the intrinsic and the world->camera extrinsic per environment —
// directly into device memory.  The scene is one oriented box (the "handle") in front of a patterned background; the mask is
// exactly the set of pixels whose viewing ray hits the box, so mask, ground-truth corners, K and E are geometrically consistent.
//
// Everything is float64 with a fixed evaluation order and no fused multiply-adds (-ffp-contract=off): oracle/synth_env_ref.py
// restates the same expressions in numpy and the two agree BIT FOR BIT (tests/test_gpu_control.py), which is what lets the
// tests drive the reference-shaped host code and the device code with identical frames.
#include "common.h"
#include "kernels.h"
#include "control.h"
#include "quantize.h"

namespace rgbm {

// Per environment: K [3,3], E [4,4] (OpenCV camera: x right, y down, z forward; X_cam = E X_world) and the ray set-up
// rays [N,12] = camera centre in box coordinates (3) + A (9, row-major) with ray direction in box coordinates
// d = A (xn, yn, 1), xn = (u - cx) / fx, yn = (v - cy) / fy.
__global__ void synth_camera_kernel(const SynthScene sc, double* K, double* E, double* rays) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= sc.N) return;
  const double* cp = sc.cam_pose + (long long)i * 7;
  const double* rp = sc.robot_pose + (long long)i * 7;
  const double* bx = sc.box + (long long)i * 15;
  double qn = sqrt(cp[3] * cp[3] + cp[4] * cp[4] + cp[5] * cp[5] + cp[6] * cp[6]);
  const double w = cp[3] / qn, x = cp[4] / qn, y = cp[5] / qn, z = cp[6] / qn;
  // columns of R(q): forward f = R e_x, left l = R e_y, up u = R e_z
  const double f[3] = {1 - 2 * (y * y + z * z), 2 * (x * y + w * z), 2 * (x * z - w * y)};
  const double l[3] = {2 * (x * y - w * z), 1 - 2 * (x * x + z * z), 2 * (y * z + w * x)};
  const double u[3] = {2 * (x * z + w * y), 2 * (y * z - w * x), 1 - 2 * (x * x + y * y)};
  const double p[3] = {rp[0] + cp[0], rp[1] + cp[1], rp[2] + cp[2]};            // camera centre in the world frame
  double R[3][3];                                                               // rows: right, down, forward
  for (int k = 0; k < 3; ++k) { R[0][k] = -l[k]; R[1][k] = -u[k]; R[2][k] = f[k]; }
  double* Ei = E + (long long)i * 16;
  for (int r = 0; r < 3; ++r) {
    for (int k = 0; k < 3; ++k) Ei[r * 4 + k] = R[r][k];
    Ei[r * 4 + 3] = -(R[r][0] * p[0] + R[r][1] * p[1] + R[r][2] * p[2]);
  }
  Ei[12] = 0; Ei[13] = 0; Ei[14] = 0; Ei[15] = 1;
  double* Ki = K + (long long)i * 9;
  Ki[0] = sc.fx; Ki[1] = 0; Ki[2] = sc.cx; Ki[3] = 0; Ki[4] = sc.fy; Ki[5] = sc.cy; Ki[6] = 0; Ki[7] = 0; Ki[8] = 1;
  double* ry = rays + (long long)i * 12;
  for (int a = 0; a < 3; ++a) {                                                 // box axis a (row a of the box rotation)
    const double* ax = bx + 3 + a * 3;
    ry[a] = ax[0] * (p[0] - bx[0]) + ax[1] * (p[1] - bx[1]) + ax[2] * (p[2] - bx[2]);
    for (int c = 0; c < 3; ++c)                                                 // A = Rbox * R^T : A[a][c] = axis_a . (row c of R)
      ry[3 + a * 3 + c] = ax[0] * R[c][0] + ax[1] * R[c][1] + ax[2] * R[c][2];
  }
}

// Ray-box test and shading of pixel (row v, column uu) of env `env`, shared by the float32 and the 8-bit kernel so that the two
// cannot drift: rs = the 12 ray constants, hs = the 3 half extents of the box (both staged in LDS by the caller).  Writes the
// colour as the float32 the float kernel stores and returns whether the viewing ray hits the box.  (The helpers come first.)
// Background pattern: channel c of a pixel whose pattern index is m (m0 < 97, m1 < 89, m2 < 13).
__device__ __forceinline__ float synth_bg(int c, int m) {
  return c == 0 ? (float)(0.20 + 0.5 * ((double)m / 97.0)) : c == 1 ? (float)(0.25 + 0.4 * ((double)m / 89.0)) : (float)(0.15 + 0.6 * ((double)m / 13.0));
}
constexpr int SYNTH_BG_M0 = 97, SYNTH_BG_M1 = 89, SYNTH_BG_M2 = 13, SYNTH_BG_ENTRIES = SYNTH_BG_M0 + SYNTH_BG_M1 + SYNTH_BG_M2;

// BG_TABLE false: synth_bg is evaluated per pixel; true: bg is a table of its SYNTH_BG_ENTRIES values (channel 0, then 1, then 2) in LDS.
template <bool BG_TABLE = false>
__device__ __forceinline__ bool synth_shade_px(const SynthScene& sc, const double* rs, const double* hs, int env, int v, int uu, float rgb[3],
                                               const float* bg = nullptr) {
  const double xn = ((double)uu - sc.cx) / sc.fx, yn = ((double)v - sc.cy) / sc.fy;
  double tmin = -INFINITY, tmax = INFINITY;
  int face = 0;
  double o[3], d[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    o[a] = rs[a];
    d[a] = (rs[3 + a * 3] * xn + rs[4 + a * 3] * yn) + rs[5 + a * 3];
    double tn, tf;
    if (d[a] != 0.0) {
      const double t1 = (-hs[a] - o[a]) / d[a], t2 = (hs[a] - o[a]) / d[a];
      tn = fmin(t1, t2); tf = fmax(t1, t2);
    } else {
      const bool inside = fabs(o[a]) <= hs[a];
      tn = inside ? -INFINITY : INFINITY; tf = INFINITY;
    }
    if (tn > tmin) { tmin = tn; face = a; }
    tmax = fmin(tmax, tf);
  }
  const bool hit = tmax >= tmin && tmin > 0.0;
  if (hit) {
    const int a1 = face == 0 ? 1 : 0, a2 = face == 2 ? 1 : 2;
    const double p1 = o[a1] + tmin * d[a1], p2 = o[a2] + tmin * d[a2];
    const long long cell = (long long)floor(p1 * 50.0) + (long long)floor(p2 * 50.0);
    const double shade = (cell & 1) ? 1.0 : 0.6;
    const double base[3][3] = {{0.85, 0.30, 0.25}, {0.25, 0.80, 0.35}, {0.30, 0.40, 0.90}};
    for (int c = 0; c < 3; ++c) rgb[c] = (float)(base[face][c] * shade);
  } else {
    const int e = sc.env0 + env;
    const int m0 = (uu * 7 + v * 3 + e * 31) % 97, m1 = (uu * 2 + v * 5 + e * 17) % 89, m2 = ((uu >> 3) + (v >> 3) + e) % 13;
    if (BG_TABLE) { rgb[0] = bg[m0]; rgb[1] = bg[SYNTH_BG_M0 + m1]; rgb[2] = bg[SYNTH_BG_M0 + SYNTH_BG_M1 + m2]; }
    else { rgb[0] = synth_bg(0, m0); rgb[1] = synth_bg(1, m1); rgb[2] = synth_bg(2, m2); }
  }
  return hit;
}

// One thread per pixel; colour [N,H,W,3] f32 in [0,1], mask [N,H,W] u8.
__global__ __launch_bounds__(256) void synth_render_kernel(const SynthScene sc, const double* rays, float* color, unsigned char* mask) {
  const int env = blockIdx.y;
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= sc.H * sc.W) return;
  const int v = pix / sc.W, uu = pix - v * sc.W;
  __shared__ double rs[12], hs[3];
  if (threadIdx.x < 12) rs[threadIdx.x] = rays[(long long)env * 12 + threadIdx.x];
  if (threadIdx.x >= 16 && threadIdx.x < 19) hs[threadIdx.x - 16] = sc.box[(long long)env * 15 + 12 + threadIdx.x - 16];
  __syncthreads();
  float rgb[3];
  const bool hit = synth_shade_px(sc, rs, hs, env, v, uu, rgb);
  const long long off = (long long)env * sc.H * sc.W + pix;
  color[off * 3] = rgb[0]; color[off * 3 + 1] = rgb[1]; color[off * 3 + 2] = rgb[2];
  mask[off] = hit ? 1 : 0;
}

// ---- the same camera delivering bytes: what an 8-bit view queue stores, written where it is kept ----------------------------
// colour [N,H,W,3] u8 = quantize_px of the float32 the kernel above stores (rgbm_quantize_frames of its frame, bit for bit), mask
// [N,H,W] u8 0 / 1, and optionally the per-env mask extent [N,4] (row min, col min, row max, col max) and hit count [N] that
// rgbm_mask_extent computes from that mask.  A thread owns SYNTH_U8_PX consecutive pixels of a frame, a workgroup 1024.
// WIDE (H*W % 4 == 0, colour and mask 4-byte aligned): 12 colour bytes leave as three 32-bit stores and 4 mask bytes as one, a
// wave writes 768 + 256 contiguous bytes.  Otherwise every byte is stored on its own and the last thread of a frame stops at H*W.
// Extent / count: per thread in registers, per workgroup in LDS, then one set of integer global atomics by thread 0 of a workgroup
// that saw a hit — integer min / max / add, so the result does not depend on the order of arrival.  ext / count were initialised
// to (2H, 2W, 0, 0) / 0 by synth_extent_init_kernel earlier on the same stream.
constexpr int SYNTH_U8_PX = 4, SYNTH_U8_THREADS = 256;

__global__ void synth_extent_init_kernel(int* ext, int* count, int N, int H, int W) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  ext[i * 4 + 0] = 2 * H; ext[i * 4 + 1] = 2 * W; ext[i * 4 + 2] = 0; ext[i * 4 + 3] = 0;
  count[i] = 0;
}

template <bool WIDE, bool BG_TABLE>
__global__ __launch_bounds__(SYNTH_U8_THREADS) void synth_render_u8_kernel(const SynthScene sc, const double* rays, unsigned char* color,
                                                                           unsigned char* mask, int* ext, int* count) {
  __shared__ double rs[12], hs[3];
  __shared__ float bg[SYNTH_BG_ENTRIES];
  __shared__ int s_y1, s_x1, s_y2, s_x2, s_n;
  const int env = blockIdx.y, t = threadIdx.x, HW = sc.H * sc.W;
  if (t < 12) rs[t] = rays[(long long)env * 12 + t];
  if (t >= 16 && t < 19) hs[t - 16] = sc.box[(long long)env * 15 + 12 + t - 16];
  if (t == 32) { s_y1 = 2 * sc.H; s_x1 = 2 * sc.W; s_y2 = 0; s_x2 = 0; s_n = 0; }
  // the background takes 3 of a pixel's 11 float64 divisions and has only 199 values: one division per thread here instead of 12.
  // BG_TABLE is off where a pattern index could be negative (the launcher decides): then it is no table index
  static_assert(SYNTH_BG_ENTRIES <= SYNTH_U8_THREADS, "one background table entry per thread");
  if (BG_TABLE) {
    if (t < SYNTH_BG_M0) bg[t] = synth_bg(0, t);
    else if (t < SYNTH_BG_M0 + SYNTH_BG_M1) bg[t] = synth_bg(1, t - SYNTH_BG_M0);
    else if (t < SYNTH_BG_ENTRIES) bg[t] = synth_bg(2, t - SYNTH_BG_M0 - SYNTH_BG_M1);
  }
  __syncthreads();
  const int pix0 = (blockIdx.x * SYNTH_U8_THREADS + t) * SYNTH_U8_PX;      // first pixel of this thread; H*W + 1023 < 2^31 (launcher)
  const long long frame = (long long)env * HW;
  unsigned q[3 * SYNTH_U8_PX], m[SYNTH_U8_PX];
  int y1 = 2 * sc.H, x1 = 2 * sc.W, y2 = 0, x2 = 0, n = 0;
#pragma unroll
  for (int j = 0; j < SYNTH_U8_PX; ++j) {
    const int pix = pix0 + j;
    if (pix >= HW) break;                                                  // WIDE: all four pixels or none
    const int v = pix / sc.W, uu = pix - v * sc.W;
    float rgb[3];
    const bool hit = synth_shade_px<BG_TABLE>(sc, rs, hs, env, v, uu, rgb, bg);
    for (int c = 0; c < 3; ++c) q[j * 3 + c] = quantize_px(rgb[c]);
    m[j] = hit ? 1u : 0u;
    if (hit) { y1 = min(y1, v); y2 = max(y2, v); x1 = min(x1, uu); x2 = max(x2, uu); ++n; }
    if (!WIDE) {
      unsigned char* cp = color + (frame + pix) * 3;
      cp[0] = (unsigned char)q[j * 3]; cp[1] = (unsigned char)q[j * 3 + 1]; cp[2] = (unsigned char)q[j * 3 + 2];
      mask[frame + pix] = (unsigned char)m[j];
    }
  }
  if (WIDE && pix0 < HW) {
    unsigned* c4 = reinterpret_cast<unsigned*>(color + (frame + pix0) * 3);
    c4[0] = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
    c4[1] = q[4] | (q[5] << 8) | (q[6] << 16) | (q[7] << 24);
    c4[2] = q[8] | (q[9] << 8) | (q[10] << 16) | (q[11] << 24);
    *reinterpret_cast<unsigned*>(mask + frame + pix0) = m[0] | (m[1] << 8) | (m[2] << 16) | (m[3] << 24);
  }
  if (!ext) return;                                                        // uniform over the grid
  if (n) { atomicMin(&s_y1, y1); atomicMax(&s_y2, y2); atomicMin(&s_x1, x1); atomicMax(&s_x2, x2); atomicAdd(&s_n, n); }
  __syncthreads();
  if (t == 0 && s_n) {
    atomicMin(&ext[env * 4 + 0], s_y1); atomicMin(&ext[env * 4 + 1], s_x1);
    atomicMax(&ext[env * 4 + 2], s_y2); atomicMax(&ext[env * 4 + 3], s_x2);
    atomicAdd(&count[env], s_n);
  }
}

int launch_synth_camera(const SynthScene& sc, double* K, double* E, double* rays, hipStream_t s) {
  RGBM_REQUIRE(sc.cam_pose && sc.robot_pose && sc.box && K && E && rays && sc.N > 0, "synth_camera arguments");
  hipLaunchKernelGGL(synth_camera_kernel, dim3((sc.N + 63) / 64), dim3(64), 0, s, sc, K, E, rays);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_synth_render(const SynthScene& sc, const double* rays, float* color, unsigned char* mask, hipStream_t s) {
  RGBM_REQUIRE(sc.box && rays && color && mask && sc.N > 0 && sc.H > 0 && sc.W > 0 && sc.N < 65536, "synth_render arguments");
  hipLaunchKernelGGL(synth_render_kernel, dim3((sc.H * sc.W + 255) / 256, sc.N), dim3(256), 0, s, sc, rays, color, mask);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_synth_render_u8(const SynthScene& sc, const double* rays, unsigned char* color, unsigned char* mask, int* ext, int* count,
                           hipStream_t s) {
  RGBM_REQUIRE(sc.box && rays && color && mask && sc.N > 0 && sc.H > 0 && sc.W > 0 && sc.N < 65536, "synth_render_u8 arguments");
  RGBM_REQUIRE((ext == nullptr) == (count == nullptr), "synth_render_u8: extent and count are both given or both null");
  const long long HW = (long long)sc.H * sc.W;
  RGBM_REQUIRE(HW <= (1ll << 30), "synth_render_u8 frame size");
  if (ext) hipLaunchKernelGGL(synth_extent_init_kernel, dim3((sc.N + 63) / 64), dim3(64), 0, s, ext, count, sc.N, sc.H, sc.W);
  constexpr int per_block = SYNTH_U8_THREADS * SYNTH_U8_PX;
  const dim3 grid((unsigned)((HW + per_block - 1) / per_block), sc.N);
  const bool wide = HW % 4 == 0 && reinterpret_cast<uintptr_t>(color) % 4 == 0 && reinterpret_cast<uintptr_t>(mask) % 4 == 0;
  // pattern indices (u * 7 + v * 3 + e * 31) % 97, ...: non-negative, hence table indices, unless the env id is negative or the sum overflows
  const bool table = sc.env0 >= 0 && 7ll * sc.W + 5ll * sc.H + 31ll * ((long long)sc.env0 + sc.N) <= 0x7fffffffll;
  auto kernel = wide ? (table ? synth_render_u8_kernel<true, true> : synth_render_u8_kernel<true, false>)
                     : (table ? synth_render_u8_kernel<false, true> : synth_render_u8_kernel<false, false>);
  hipLaunchKernelGGL(kernel, grid, dim3(SYNTH_U8_THREADS), 0, s, sc, rays, color, mask, ext, count);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace rgbm
