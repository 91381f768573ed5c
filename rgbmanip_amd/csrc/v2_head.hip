// The per-point plane-sweep head of the v2 network (lib/network_v2.py:152-184): for a chosen pixel, ref + warped over the 24 planes,
// volume_conv (three 1x1x1 Conv3d + eval BatchNorm + ReLU, 32 -> 16 -> 8 -> 1), fuse_conv (1x1 Conv2d 24 -> 32, ReLU, 32 -> 64), the
// gather at `choose`, and pose_mlp1 (64 -> 64 -> 64, ReLU each).  Nothing in that chain mixes pixels, so the value at a chosen pixel
// depends on that pixel's 24 voxels alone: the kernel evaluates the 1024 chosen pixels of a view instead of its 50 176, and no volume
// exists in memory (the reference materialises 154 MB per view for it).
//
// Mapping, chosen for the tap gathers (12 KB per point from fp32 maps, which is what the kernel waits for): 8 lanes carry one point, lane
// c of them channels 4c .. 4c + 3, so that a tap's 32 channels are one contiguous row read by 8 neighbouring lanes (16 bytes per lane
// from fp32 maps, 8 from 16-bit maps); the four taps of a plane are read unconditionally at clamped addresses (four independent loads in
// flight) and an outside tap adds nothing, which is grid_sample's zero padding per tap.  The voxel is the arithmetic of
// build_volume_kernel (warp_device.h; both files are built with -ffp-contract=off).  volume_conv is split over the 8 lanes by input
// channel: a reduce-scatter (xor 4, 2, 1) leaves lane c with outputs 2c, 2c + 1 of layer 1, then with output c of layer 2, and a butterfly
// sum of layer 3's 8 products leaves the plane value, the same bits, in all 8 lanes: 24 exchanges per plane, no product computed twice.
// The 24 plane values go through a row of LDS; from there on lane c computes output channels 4c .. 4c + 3 and 32 + 4c .. 32 + 4c + 3 of
// every layer: weights are k-major in LDS (conflict-free 16-byte reads), the layer's input is a broadcast read of the point's row.
// All arithmetic is fp32 whatever the feature map's storage type.  512 threads = 64 points per pass; 47.6 KB of weights + 17.4 KB of rows.
#include "common.h"
#include "kernels.h"
#include "warp_device.h"

namespace rgbm {

// offsets into the table (floats); every block starts on a multiple of 4
constexpr int kV2W1 = 0;                          // volume_conv.0 x BN scale  [16][32] (output-major: lane c reads [o][4c .. 4c + 3])
constexpr int kV2B1 = kV2W1 + 16 * 32;            // its BN shift [16]
constexpr int kV2W2 = kV2B1 + 16;                 // volume_conv.1 [8][16], shift [8]
constexpr int kV2B2 = kV2W2 + 8 * 16;
constexpr int kV2W3 = kV2B2 + 8;                  // volume_conv.2 [8], shift [1] (+ 3 pad)
constexpr int kV2B3 = kV2W3 + 8;
constexpr int kV2FA = kV2B3 + 4;                  // fuse_conv.0 transposed [24][32], bias [32]
constexpr int kV2FAb = kV2FA + 24 * 32;
constexpr int kV2FB = kV2FAb + 32;                // fuse_conv.2 transposed [32][64], bias [64]
constexpr int kV2FBb = kV2FB + 32 * 64;
constexpr int kV2M0 = kV2FBb + 64;                // pose_mlp1.0 transposed [64][64], bias [64]
constexpr int kV2M0b = kV2M0 + 64 * 64;
constexpr int kV2M1 = kV2M0b + 64;                // pose_mlp1.2 transposed [64][64], bias [64]
constexpr int kV2M1b = kV2M1 + 64 * 64;
static_assert(kV2M1b + 64 == kV2HeadFloats, "kernels.h: kV2HeadFloats");
constexpr int kV2Row = 68;                        // floats per point row in LDS: 64 + 4, so the 8 rows of a wave start 4 banks apart
constexpr int kV2Points = 64;                     // points per pass of a 512-thread workgroup

void v2_head_pack(const V2HeadWeights& m, float* t) {
  for (int i = 0; i < kV2HeadFloats; ++i) t[i] = 0.f;
  for (int o = 0; o < 16; ++o) {
    for (int i = 0; i < 32; ++i) t[kV2W1 + o * 32 + i] = m.vc_w[0][o * 32 + i] * m.vc_scale[0][o];
    t[kV2B1 + o] = m.vc_shift[0][o];
  }
  for (int o = 0; o < 8; ++o) {
    for (int i = 0; i < 16; ++i) t[kV2W2 + o * 16 + i] = m.vc_w[1][o * 16 + i] * m.vc_scale[1][o];
    t[kV2B2 + o] = m.vc_shift[1][o];
  }
  for (int i = 0; i < 8; ++i) t[kV2W3 + i] = m.vc_w[2][i] * m.vc_scale[2][0];
  t[kV2B3] = m.vc_shift[2][0];
  for (int o = 0; o < 32; ++o) {
    for (int k = 0; k < 24; ++k) t[kV2FA + k * 32 + o] = m.fc_w[0][o * 24 + k];
    t[kV2FAb + o] = m.fc_b[0][o];
  }
  for (int o = 0; o < 64; ++o) {
    for (int k = 0; k < 32; ++k) t[kV2FB + k * 64 + o] = m.fc_w[1][o * 32 + k];
    t[kV2FBb + o] = m.fc_b[1][o];
    for (int k = 0; k < 64; ++k) {
      t[kV2M0 + k * 64 + o] = m.pm_w[0][o * 64 + k];
      t[kV2M1 + k * 64 + o] = m.pm_w[1][o * 64 + k];
    }
    t[kV2M0b + o] = m.pm_b[0][o];
    t[kV2M1b + o] = m.pm_b[1][o];
  }
}

__device__ __forceinline__ float relu_nan(float a) { return a < 0.f ? 0.f : a; }      // NaN propagates, like torch.relu

// a layer with 64 outputs on a point's row x [K] (LDS, read as a broadcast): lane c gets channels 4c .. 4c + 3 (lo) and 32 + 4c .. (hi)
template <int K, bool RELU>
__device__ __forceinline__ void v2_layer64(const float* __restrict__ wt, const float* __restrict__ bias, const float* __restrict__ x, int c,
                                           float4& lo, float4& hi) {
  lo = *reinterpret_cast<const float4*>(bias + c * 4);
  hi = *reinterpret_cast<const float4*>(bias + 32 + c * 4);
#pragma unroll 2
  for (int k0 = 0; k0 < K; k0 += 4) {
    const float4 xv = *reinterpret_cast<const float4*>(x + k0);
    const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float4 a = *reinterpret_cast<const float4*>(wt + (k0 + j) * 64 + c * 4);
      const float4 b = *reinterpret_cast<const float4*>(wt + (k0 + j) * 64 + 32 + c * 4);
      lo.x = fmaf(xs[j], a.x, lo.x); lo.y = fmaf(xs[j], a.y, lo.y); lo.z = fmaf(xs[j], a.z, lo.z); lo.w = fmaf(xs[j], a.w, lo.w);
      hi.x = fmaf(xs[j], b.x, hi.x); hi.y = fmaf(xs[j], b.y, hi.y); hi.z = fmaf(xs[j], b.z, hi.z); hi.w = fmaf(xs[j], b.w, hi.w);
    }
  }
  if (RELU) {
    lo.x = relu_nan(lo.x); lo.y = relu_nan(lo.y); lo.z = relu_nan(lo.z); lo.w = relu_nan(lo.w);
    hi.x = relu_nan(hi.x); hi.y = relu_nan(hi.y); hi.z = relu_nan(hi.z); hi.w = relu_nan(hi.w);
  }
}

template <typename T>
__global__ __launch_bounds__(512) void v2_point_rows_kernel(const float* __restrict__ table, const T* __restrict__ feat,
                                                            const float* __restrict__ homog, const float* __restrict__ depths,
                                                            const int* __restrict__ choose, float* __restrict__ rows,
                                                            float* __restrict__ fuse64, float* __restrict__ planes, int V, int B, int P,
                                                            int D, int H, int W, long long N) {
  constexpr int C = 32;
  __shared__ __attribute__((aligned(16))) float w[kV2HeadFloats];
  __shared__ __attribute__((aligned(16))) float xrows[kV2Points * kV2Row];
  for (int i = threadIdx.x; i < kV2HeadFloats; i += 512) w[i] = table[i];
  __syncthreads();
  const int c = threadIdx.x & 7;
  float* const xr = xrows + (threadIdx.x >> 3) * kV2Row;
  // every thread walks the same number of passes (the barriers below are the workgroup's); a thread past the last point computes
  // point N - 1 again and stores nothing
  for (long long base = (long long)blockIdx.x * kV2Points; base < N; base += (long long)gridDim.x * kV2Points) {
    const long long pt_raw = base + (threadIdx.x >> 3);
    const bool live = pt_raw < N;
    const long long pt = live ? pt_raw : N - 1;
    const int v = (int)(pt / P);
    const int partner = (v + B) % V;
    const int b = v % B;
    const int pix = min(max(choose[pt], 0), H * W - 1);      // an index outside the crop reads its nearest end, never outside the map
    const int y = pix / W, x = pix - y * W;
    float ref[4];
    load4(feat + (((long long)v * H + y) * W + x) * C + c * 4, ref);
    const T* src = feat + (long long)partner * H * W * C + c * 4;
    const float* hm = homog + (long long)v * 12;
#pragma unroll 1
    for (int dz = 0; dz < D; ++dz) {
      asm volatile("" ::: "memory");      // the plane loop re-reads its weights from LDS: hoisted out of it they fill 256 VGPRs and spill (120 with this)
      float ix, iy;
      warp_coords(hm, (float)x, (float)y, depths[b * D + dz], H, W, ix, iy);
      const Bilin bl = bilin_setup(ix, iy);
      const bool xin0 = (unsigned)bl.x0 < (unsigned)W, xin1 = (unsigned)(bl.x0 + 1) < (unsigned)W;
      const bool yin0 = (unsigned)bl.y0 < (unsigned)H, yin1 = (unsigned)(bl.y0 + 1) < (unsigned)H;
      const int xc0 = min(max(bl.x0, 0), W - 1), xc1 = min(max(bl.x0 + 1, 0), W - 1);
      const int yc0 = min(max(bl.y0, 0), H - 1), yc1 = min(max(bl.y0 + 1, 0), H - 1);
      float s00[4], s01[4], s10[4], s11[4];
      load4(src + ((long long)yc0 * W + xc0) * C, s00);
      load4(src + ((long long)yc0 * W + xc1) * C, s01);
      load4(src + ((long long)yc1 * W + xc0) * C, s10);
      load4(src + ((long long)yc1 * W + xc1) * C, s11);
      float f[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        // build_volume_kernel's sum: corners 00, 01, 10, 11, an absent corner adds nothing
        float acc = 0.f;
        if (xin0 && yin0) acc += s00[e] * bl.w00;
        if (xin1 && yin0) acc += s01[e] * bl.w01;
        if (xin0 && yin1) acc += s10[e] * bl.w10;
        if (xin1 && yin1) acc += s11[e] * bl.w11;
        f[e] = bl.nan ? __builtin_nanf("") : (ref[e] + acc);
      }
      // volume_conv.0: this lane's four input channels of all 16 outputs, then a reduce-scatter over the point's 8 lanes: each exchange
      // (xor 4, 2, 1) halves what a lane still carries, and lane c ends with the whole sums of outputs 2c and 2c + 1
      float p16[16];
#pragma unroll
      for (int o = 0; o < 16; ++o) {
        const float4 wv = *reinterpret_cast<const float4*>(w + kV2W1 + o * 32 + c * 4);
        float a = f[0] * wv.x;
        a = fmaf(f[1], wv.y, a); a = fmaf(f[2], wv.z, a); a = fmaf(f[3], wv.w, a);
        p16[o] = a;
      }
      const bool b2 = (c & 4) != 0, b1 = (c & 2) != 0, b0 = (c & 1) != 0;
      float p8[8], p4[4], p2[2];
#pragma unroll
      for (int o = 0; o < 8; ++o) p8[o] = (b2 ? p16[o + 8] : p16[o]) + __shfl_xor(b2 ? p16[o] : p16[o + 8], 4);
#pragma unroll
      for (int o = 0; o < 4; ++o) p4[o] = (b1 ? p8[o + 4] : p8[o]) + __shfl_xor(b1 ? p8[o] : p8[o + 4], 2);
#pragma unroll
      for (int o = 0; o < 2; ++o) p2[o] = (b0 ? p4[o + 2] : p4[o]) + __shfl_xor(b0 ? p4[o] : p4[o + 2], 1);
      const float2 bias1 = *reinterpret_cast<const float2*>(w + kV2B1 + 2 * c);
      const float h1a = relu_nan(p2[0] + bias1.x), h1b = relu_nan(p2[1] + bias1.y);
      // volume_conv.1: this lane's two inputs of all 8 outputs, the same exchange: lane c ends with output c
      float q8[8], q4[4], q2[2];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float2 wv = *reinterpret_cast<const float2*>(w + kV2W2 + j * 16 + 2 * c);
        q8[j] = fmaf(h1b, wv.y, h1a * wv.x);
      }
#pragma unroll
      for (int o = 0; o < 4; ++o) q4[o] = (b2 ? q8[o + 4] : q8[o]) + __shfl_xor(b2 ? q8[o] : q8[o + 4], 4);
#pragma unroll
      for (int o = 0; o < 2; ++o) q2[o] = (b1 ? q4[o + 2] : q4[o]) + __shfl_xor(b1 ? q4[o] : q4[o + 2], 2);
      const float q1 = (b0 ? q2[1] : q2[0]) + __shfl_xor(b0 ? q2[0] : q2[1], 1);
      const float h2 = relu_nan(q1 + w[kV2B2 + c]);
      // volume_conv.2: one product per lane and a butterfly sum, which leaves the same bits in all 8 lanes
      float pv = h2 * w[kV2W3 + c];
      pv += __shfl_xor(pv, 4);
      pv += __shfl_xor(pv, 2);
      pv += __shfl_xor(pv, 1);
      pv = relu_nan(pv + w[kV2B3]);
      if (c == (dz & 7)) {
        xr[dz] = pv;
        if (planes != nullptr && live) planes[pt * D + dz] = pv;
      }
    }
    __syncthreads();
    // fuse_conv.0 (24 -> 32, ReLU): channels 4c .. 4c + 3 into the row's second half
    {
      float4 a = *reinterpret_cast<const float4*>(w + kV2FAb + c * 4);
#pragma unroll
      for (int k0 = 0; k0 < 24; k0 += 4) {
        const float4 xv = *reinterpret_cast<const float4*>(xr + k0);
        const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float4 wv = *reinterpret_cast<const float4*>(w + kV2FA + (k0 + j) * 32 + c * 4);
          a.x = fmaf(xs[j], wv.x, a.x); a.y = fmaf(xs[j], wv.y, a.y); a.z = fmaf(xs[j], wv.z, a.z); a.w = fmaf(xs[j], wv.w, a.w);
        }
      }
      a.x = relu_nan(a.x); a.y = relu_nan(a.y); a.z = relu_nan(a.z); a.w = relu_nan(a.w);
      *reinterpret_cast<float4*>(xr + 32 + c * 4) = a;
    }
    __syncthreads();
    float4 lo, hi;
    v2_layer64<32, false>(w + kV2FB, w + kV2FBb, xr + 32, c, lo, hi);      // fuse_conv.2: no ReLU behind it
    __syncthreads();
    *reinterpret_cast<float4*>(xr + c * 4) = lo;
    *reinterpret_cast<float4*>(xr + 32 + c * 4) = hi;
    if (fuse64 != nullptr && live) {
      *reinterpret_cast<float4*>(fuse64 + pt * 64 + c * 4) = lo;
      *reinterpret_cast<float4*>(fuse64 + pt * 64 + 32 + c * 4) = hi;
    }
    __syncthreads();
    v2_layer64<64, true>(w + kV2M0, w + kV2M0b, xr, c, lo, hi);            // pose_mlp1.0
    __syncthreads();
    *reinterpret_cast<float4*>(xr + c * 4) = lo;
    *reinterpret_cast<float4*>(xr + 32 + c * 4) = hi;
    __syncthreads();
    v2_layer64<64, true>(w + kV2M1, w + kV2M1b, xr, c, lo, hi);            // pose_mlp1.2
    if (live) {
      *reinterpret_cast<float4*>(rows + pt * 64 + c * 4) = lo;
      *reinterpret_cast<float4*>(rows + pt * 64 + 32 + c * 4) = hi;
    }
    __syncthreads();      // the next pass writes the rows this one read
  }
}

int launch_v2_point_rows(int feat_dtype, const float* table, const void* feat, const float* homog, const float* depths, const int* choose,
                         float* rows, float* fuse64, float* planes, int V, int B, int P, int D, int H, int W, int Vh, hipStream_t s) {
  RGBM_REQUIRE(table && feat && homog && depths && choose && rows, "v2_point_rows arguments");
  RGBM_REQUIRE((((uintptr_t)feat | (uintptr_t)rows | (uintptr_t)fuse64) & 15) == 0 && ((uintptr_t)table & 3) == 0,
               "v2_point_rows: feat, rows and fuse64 must be 16-byte aligned (a lane moves 16-byte pieces of their rows)");
  RGBM_REQUIRE(feat_dtype == F32 || feat_dtype == BF16 || feat_dtype == F16, "v2_point_rows: fp32, bf16 or f16 feature maps (a split-pair net hands its fp32 copy)");
  RGBM_REQUIRE(B > 0 && V == 2 * B && (Vh == B || Vh == V) && P > 0 && D == 24 && H > 0 && W > 0 && (long long)H * W < (1ll << 31) / 32,
               "v2_point_rows: V = 2B views, heads for B or 2B of them, 24 planes");
  const long long N = (long long)Vh * P;
  int n_cu = 0;
  if (int rc = persistent_grid_cus(&n_cu)) return rc;
  const long long passes = (N + kV2Points - 1) / kV2Points;
  const long long cap = 2ll * n_cu;      // two workgroups fit a CU's LDS
  const unsigned grid = (unsigned)(passes < cap ? passes : cap);
  if (feat_dtype == BF16)
    hipLaunchKernelGGL(v2_point_rows_kernel<unsigned short>, dim3(grid), dim3(512), 0, s, table, (const unsigned short*)feat, homog, depths, choose,
                       rows, fuse64, planes, V, B, P, D, H, W, N);
  else if (feat_dtype == F16)
    hipLaunchKernelGGL(v2_point_rows_kernel<f16_t>, dim3(grid), dim3(512), 0, s, table, (const f16_t*)feat, homog, depths, choose, rows, fuse64,
                       planes, V, B, P, D, H, W, N);
  else
    hipLaunchKernelGGL(v2_point_rows_kernel<float>, dim3(grid), dim3(512), 0, s, table, (const float*)feat, homog, depths, choose, rows, fuse64,
                       planes, V, B, P, D, H, W, N);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace rgbm
