// Dense head of the cost volume, gfx950: prob conv + softmax + expected depth + confidence at EVERY pixel of the crop
// (the depth map the reference's earlier generation returns, lib/network_v3.py:406-408), from the u11 that the dense cost
// regularisation materialises per view chunk.  The point kernel (head_kernels.hip: prob_softmax_depth_kernel) evaluates the same
// Conv3d(8 -> 1, 3^3, pad 1, no bias) (network_v5.py:280,290) only at the P chosen pixels; this one is its dense twin and keeps its
// arithmetic: fp32 sums, taps kd, kh, kw ascending, the eight channels of a tap as one expression, the softmax and the expectation
// written the same way — so that the map read at a chosen pixel is the point kernel's view1_depth.
//
// A workgroup of 256 threads owns a DD_TH x DD_TW = 8 x 32 pixel tile of one view, one pixel per thread, and walks the D depth planes
// once.  Plane z of the tile plus its one-pixel border (10 x 34 voxels x 8 channels) is staged in LDS as fp32 — whatever the storage
// type, so the conversion is paid once per voxel and not once per tap — and every thread adds the plane's nine in-plane taps to the
// three logits it feeds: kd = 0 of logit z + 1, kd = 1 of logit z, kd = 2 of logit z - 1.  Planes arrive in ascending order, so each
// logit still receives its 27 taps in the point kernel's order.  Two LDS slots: plane z + 1 is fetched into registers while plane z is
// consumed, one barrier per plane.  u11 is read 340 / 256 = 1.33 times (the border); the 216 weights sit in LDS in [kh][kw][kd][c] order
// (held in SGPRs they spill), from where the compiler keeps most of them in VGPRs across the plane loop.  Out-of-volume taps: border
// voxels outside the crop are staged as zeros, planes -1 and D are skipped; a zero tap adds +-0 to a sum that is never -0, which leaves it
// bit for bit what skipping the tap leaves.
#include "common.h"
#include "kernels.h"

namespace rgbm {

namespace {
constexpr int DD_TH = 8, DD_TW = 32, DD_C = 8;
constexpr int DD_HW = DD_TW + 2, DD_HH = DD_TH + 2, DD_NV = DD_HW * DD_HH;      // staged voxels of a plane: 340
constexpr int DD_MAXD = 24;
static_assert(DD_TH * DD_TW == 256 && DD_NV <= 512, "one pixel per thread, at most two staged voxels per thread");

// a voxel's eight channels as they lie in memory (16 bytes of a 16-bit type, 32 of a 4-byte one), and as floats: the values
// load4(p) / load4(p + 4) of the point kernel give
template <typename T> struct DDRaw { uint4 q[sizeof(T) / 2]; };
template <typename T> __device__ __forceinline__ void dd_fetch(const T* p, DDRaw<T>& r) {
#pragma unroll
  for (int i = 0; i < (int)sizeof(T) / 2; ++i) r.q[i] = reinterpret_cast<const uint4*>(p)[i];
}
template <typename T> __device__ __forceinline__ void dd_floats(const DDRaw<T>& r, float v[8]) {
  if (sizeof(T) == 2) {
    unpack_chunk(r.q[0], v, T());
  } else {
    unpack_chunk(r.q[0], v, T());
    unpack_chunk(r.q[sizeof(T) / 2 - 1], v + 4, T());
  }
}
}  // namespace

template <typename T>
__global__ __launch_bounds__(256) void dense_depth_kernel(const T* __restrict__ u11, const float* __restrict__ wprob,
                                                          const float* __restrict__ depths, float* __restrict__ depth_map,
                                                          float* __restrict__ conf_map, int v0, int Vc, int B, int D, int H, int W,
                                                          int classmajor) {
  constexpr int C = DD_C;
  __shared__ __attribute__((aligned(16))) float plane[2][DD_NV * C];
  __shared__ __attribute__((aligned(16))) float wl[9 * 3 * C];      // wprob as [kh][kw][kd][c]: the 24 weights of an in-plane tap side by side
  __shared__ float logit[DD_MAXD][256];      // a thread's own column: no barrier between its writes and its reads
  const int tid = threadIdx.x;
  if (tid < 27 * C) {
    const int c = tid % C, t = tid / C, kw = t % 3, kh = (t / 3) % 3, kd = t / 9;
    wl[((kh * 3 + kw) * 3 + kd) * C + c] = wprob[tid];      // read behind the first plane's barrier
  }
  const int tiles_x = (W + DD_TW - 1) / DD_TW;
  const int ty0 = (blockIdx.x / tiles_x) * DD_TH, tx0 = (blockIdx.x % tiles_x) * DD_TW;
  const int vl = blockIdx.y;                 // local view of the chunk
  const int v = v0 + vl;

  // the (at most two) border-tile voxels this thread stages per plane: their in-plane offset in u11, or -1 outside the crop
  long long voff[2];
  bool stage[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int i = tid + 256 * r;
    stage[r] = i < DD_NV;
    const int hy = i / DD_HW, hx = i - hy * DD_HW;
    const int yy = ty0 + hy - 1, xx = tx0 + hx - 1;
    voff[r] = -1;
    if (stage[r] && (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W)
      // class-major u11 (written by the halo-tiled conv11): class = parity bits (d,y,x), dense [8][Vc][D/2][H/2][W/2][C]; the depth
      // part of either index is added per plane below
      voff[r] = classmajor ? ((((long long)(((yy & 1) << 1) | (xx & 1)) * Vc + vl) * (D >> 1)) * (H >> 1) + (yy >> 1)) * (W >> 1) + (xx >> 1)
                           : (((long long)vl * D) * H + yy) * W + xx;
  }
  const long long cls_d = (long long)4 * Vc * (D >> 1) * (H >> 1) * (W >> 1);      // class-major: voxels between depth parities
  const long long zstep = classmajor ? (long long)(H >> 1) * (W >> 1) : (long long)H * W;
  auto fetch = [&](int z, DDRaw<T> regs[2]) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
#pragma unroll
      for (int i = 0; i < (int)sizeof(T) / 2; ++i) regs[r].q[i] = make_uint4(0u, 0u, 0u, 0u);      // all-zero bits are 0.0 in every storage type
      if (voff[r] >= 0) {
        const long long vidx = classmajor ? voff[r] + (z & 1) * cls_d + (long long)(z >> 1) * zstep : voff[r] + (long long)z * zstep;
        dd_fetch(u11 + vidx * C, regs[r]);
      }
    }
  };

  const int py = tid / DD_TW, px = tid - py * DD_TW;      // this thread's pixel inside the tile
  DDRaw<T> regs[2];      // plane z + 1 in flight while plane z is consumed: converted only when it is written to LDS
  fetch(0, regs);
  float a_lo = 0.f, a_mid = 0.f, a_hi = 0.f;              // the sums of logits z - 1, z, z + 1 while plane z is consumed
  for (int z = 0; z < D; ++z) {
    float* pl = plane[z & 1];
#pragma unroll
    for (int r = 0; r < 2; ++r)
      if (stage[r]) {
        float f[C];
        dd_floats(regs[r], f);
        store4(pl + (tid + 256 * r) * C, f);
        store4(pl + (tid + 256 * r) * C + 4, f + 4);
      }
    __syncthreads();      // slot z & 1 was last read while plane z - 2 was consumed: every thread has passed the barrier of plane z - 1 since
    if (z + 1 < D) fetch(z + 1, regs);
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        float a[4], b[4];
        const float* p = pl + ((py + kh) * DD_HW + (px + kw)) * C;
        load4(p, a);
        load4(p + 4, b);
        {                 // kd = 0 of logit z + 1
          const float* ww = wl + ((kh * 3 + kw) * 3 + 0) * C;
          a_hi += a[0] * ww[0] + a[1] * ww[1] + a[2] * ww[2] + a[3] * ww[3] + b[0] * ww[4] + b[1] * ww[5] + b[2] * ww[6] +
                  b[3] * ww[7];
        }
        {                 // kd = 1 of logit z
          const float* ww = wl + ((kh * 3 + kw) * 3 + 1) * C;
          a_mid += a[0] * ww[0] + a[1] * ww[1] + a[2] * ww[2] + a[3] * ww[3] + b[0] * ww[4] + b[1] * ww[5] + b[2] * ww[6] +
                   b[3] * ww[7];
        }
        {                 // kd = 2 of logit z - 1
          const float* ww = wl + ((kh * 3 + kw) * 3 + 2) * C;
          a_lo += a[0] * ww[0] + a[1] * ww[1] + a[2] * ww[2] + a[3] * ww[3] + b[0] * ww[4] + b[1] * ww[5] + b[2] * ww[6] +
                  b[3] * ww[7];
        }
      }
    }
    if (z >= 1) logit[z - 1][tid] = a_lo;      // (the sums of "logit -1" and "logit D" are formed and dropped: no branch in the tap loop)
    a_lo = a_mid; a_mid = a_hi; a_hi = 0.f;
  }
  logit[D - 1][tid] = a_lo;

  const int y = ty0 + py, x = tx0 + px;
  if (y >= H || x >= W) return;              // (no barrier behind this point)
  // softmax over depth, expectation, maximum: the point kernel's statements
  float m = -INFINITY;
  for (int dz = 0; dz < D; ++dz) m = fmaxf(m, logit[dz][tid]);
  float sum = 0.f;
  for (int dz = 0; dz < D; ++dz) { const float e = expf(logit[dz][tid] - m); logit[dz][tid] = e; sum += e; }
  const float inv = 1.f / sum;
  float dep = 0.f, conf = 0.f;
  const int b = v % B;
  for (int dz = 0; dz < D; ++dz) {
    const float pr = logit[dz][tid] * inv;
    dep += pr * depths[b * D + dz];
    conf = pr > conf || pr != pr ? pr : conf;      // NaN propagates, like torch.max
  }
  const long long o = ((long long)v * H + y) * W + x;
  depth_map[o] = dep;
  if (conf_map) conf_map[o] = conf;
}

int launch_dense_depth(int dtype, const void* u11, const float* wprob, const float* depths, float* depth_map, float* conf_map,
                       int v0, int Vc, int B, int D, int H, int W, int classmajor, hipStream_t s) {
  RGBM_REQUIRE(u11 && wprob && depths && depth_map, "dense depth arguments");
  RGBM_REQUIRE(D >= 1 && D <= DD_MAXD && Vc > 0 && Vc <= 65535 && H > 0 && W > 0, "dense depth supports up to 24 depth planes and 65535 views per chunk");
  RGBM_REQUIRE(!classmajor || (D % 2 == 0 && H % 2 == 0 && W % 2 == 0), "dense depth: class-major u11 needs even dimensions");
  const dim3 g((unsigned)(((W + DD_TW - 1) / DD_TW) * ((H + DD_TH - 1) / DD_TH)), (unsigned)Vc);
  if (dtype == BF16)
    hipLaunchKernelGGL(dense_depth_kernel<unsigned short>, g, dim3(256), 0, s, (const unsigned short*)u11, wprob, depths, depth_map, conf_map,
                       v0, Vc, B, D, H, W, classmajor);
  else if (dtype == F16)
    hipLaunchKernelGGL(dense_depth_kernel<f16_t>, g, dim3(256), 0, s, (const f16_t*)u11, wprob, depths, depth_map, conf_map,
                       v0, Vc, B, D, H, W, classmajor);
  else if (dtype == BF16X3)
    hipLaunchKernelGGL(dense_depth_kernel<bx3_t>, g, dim3(256), 0, s, (const bx3_t*)u11, wprob, depths, depth_map, conf_map,
                       v0, Vc, B, D, H, W, classmajor);
  else
    hipLaunchKernelGGL(dense_depth_kernel<float>, g, dim3(256), 0, s, (const float*)u11, wprob, depths, depth_map, conf_map,
                       v0, Vc, B, D, H, W, classmajor);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace rgbm
