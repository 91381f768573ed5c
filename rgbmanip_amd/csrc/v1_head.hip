// Stage A of the v1 network's heads (lib/network.py:167-177): for a chosen pixel, ref + warped over the 24 planes, volume_conv (three
// 1x1x1 Conv3d + eval BatchNorm + ReLU, 32 -> 16 -> 8 -> 1), fuse_conv (1x1 Conv2d 24 -> 32, ReLU, 32 -> 32) and the residual
// relu(ref + fuse_conv(planes)), which replaces the pixel's feature row.  As in the v2 network nothing of the chain mixes pixels, and both
// warps read the ORIGINAL maps, so the new row of a chosen pixel depends on that pixel's 24 voxels alone: the kernel evaluates the chosen
// pixels, and neither a volume nor a second feature map exists in memory.
//
// The mapping is v2_point_rows_kernel's (v2_head.hip, which describes it): 8 lanes carry one point, lane c of them channels 4c .. 4c + 3.
// The plane loop below is a COPY of that kernel's, statement for statement, and not a shared function: with the loop moved into one
// __forceinline__ function of a common header the three instantiations of v2_point_rows_kernel no longer disassembled to their
// instructions (same count, another schedule), so v2_head.hip stays as it is and this file carries its own copy.
// Whoever changes one loop changes the other.  What differs is the tail behind the loop - two small layers and the residual on the
// lane's own four channels of `ref`, which it still holds from the plane sum - and the table: 10.1 KB against 47.6 KB.
// All arithmetic is fp32 whatever the feature map's storage type.  512 threads = 64 points per pass; 10.1 KB of weights + 17.4 KB of rows.
#include "common.h"
#include "kernels.h"
#include "warp_device.h"

namespace rgbm {

// offsets into the table (floats); every block starts on a multiple of 4.  The first 676 floats keep the layout of v2's table (kV2W1 .. kV2B3)
constexpr int kV1W1 = 0;                          // volume_conv.0 x BN scale  [16][32] (output-major: lane c reads [o][4c .. 4c + 3])
constexpr int kV1B1 = kV1W1 + 16 * 32;            // its BN shift [16]
constexpr int kV1W2 = kV1B1 + 16;                 // volume_conv.1 [8][16], shift [8]
constexpr int kV1B2 = kV1W2 + 8 * 16;
constexpr int kV1W3 = kV1B2 + 8;                  // volume_conv.2 [8], shift [1] (+ 3 pad)
constexpr int kV1B3 = kV1W3 + 8;
constexpr int kV1FA = kV1B3 + 4;                  // fuse_conv.0 transposed [24][32], bias [32]
constexpr int kV1FAb = kV1FA + 24 * 32;
constexpr int kV1FB = kV1FAb + 32;                // fuse_conv.2 transposed [32][32], bias [32]
constexpr int kV1FBb = kV1FB + 32 * 32;
static_assert(kV1FBb + 32 == kV1HeadFloats, "kernels.h: kV1HeadFloats");
constexpr int kV1Row = 68;                        // floats per point row in LDS (planes in 0 .. 23, fuse_conv.0's output in 32 .. 63): the 8 rows of a wave start 4 banks apart
constexpr int kV1Points = 64;                     // points per pass of a 512-thread workgroup
constexpr int kV1GroupsPerCu = 2;                 // resident workgroups per CU: 100 - 104 VGPRs leave 4 waves per SIMD = two 512-thread workgroups; the 27.5 KB of LDS would allow 5

void v1_head_pack(const V1HeadWeights& m, float* t) {
  for (int i = 0; i < kV1HeadFloats; ++i) t[i] = 0.f;
  for (int o = 0; o < 16; ++o) {
    for (int i = 0; i < 32; ++i) t[kV1W1 + o * 32 + i] = m.vc_w[0][o * 32 + i] * m.vc_scale[0][o];
    t[kV1B1 + o] = m.vc_shift[0][o];
  }
  for (int o = 0; o < 8; ++o) {
    for (int i = 0; i < 16; ++i) t[kV1W2 + o * 16 + i] = m.vc_w[1][o * 16 + i] * m.vc_scale[1][o];
    t[kV1B2 + o] = m.vc_shift[1][o];
  }
  for (int i = 0; i < 8; ++i) t[kV1W3 + i] = m.vc_w[2][i] * m.vc_scale[2][0];
  t[kV1B3] = m.vc_shift[2][0];
  for (int o = 0; o < 32; ++o) {
    for (int k = 0; k < 24; ++k) t[kV1FA + k * 32 + o] = m.fc_w[0][o * 24 + k];
    t[kV1FAb + o] = m.fc_b[0][o];
    for (int k = 0; k < 32; ++k) t[kV1FB + k * 32 + o] = m.fc_w[1][o * 32 + k];
    t[kV1FBb + o] = m.fc_b[1][o];
  }
}

__device__ __forceinline__ float relu_nan(float a) { return a < 0.f ? 0.f : a; }      // NaN propagates, like torch.relu

// a layer with 32 outputs on a point's row x [K] (LDS, read as a broadcast): lane c gets channels 4c .. 4c + 3; bias first, then k ascending
template <int K>
__device__ __forceinline__ float4 v1_layer32(const float* __restrict__ wt, const float* __restrict__ bias, const float* __restrict__ x, int c) {
  float4 a = *reinterpret_cast<const float4*>(bias + c * 4);
#pragma unroll
  for (int k0 = 0; k0 < K; k0 += 4) {
    const float4 xv = *reinterpret_cast<const float4*>(x + k0);
    const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float4 wv = *reinterpret_cast<const float4*>(wt + (k0 + j) * 32 + c * 4);
      a.x = fmaf(xs[j], wv.x, a.x); a.y = fmaf(xs[j], wv.y, a.y); a.z = fmaf(xs[j], wv.z, a.z); a.w = fmaf(xs[j], wv.w, a.w);
    }
  }
  return a;
}

template <typename T>
__global__ __launch_bounds__(512) void v1_fused_points_kernel(const float* __restrict__ table, const T* __restrict__ feat,
                                                              const float* __restrict__ homog, const float* __restrict__ depths,
                                                              const int* __restrict__ choose, float* __restrict__ fused32,
                                                              float* __restrict__ planes, int V, int B, int P, int D, int H, int W,
                                                              long long N) {
  constexpr int C = 32;
  __shared__ __attribute__((aligned(16))) float w[kV1HeadFloats];
  __shared__ __attribute__((aligned(16))) float xrows[kV1Points * kV1Row];
  for (int i = threadIdx.x; i < kV1HeadFloats; i += 512) w[i] = table[i];
  __syncthreads();
  const int c = threadIdx.x & 7;
  float* const xr = xrows + (threadIdx.x >> 3) * kV1Row;
  // every thread walks the same number of passes (the barriers below are the workgroup's); a thread past the last point computes
  // point N - 1 again and stores nothing
  for (long long base = (long long)blockIdx.x * kV1Points; base < N; base += (long long)gridDim.x * kV1Points) {
    const long long pt_raw = base + (threadIdx.x >> 3);
    const bool live = pt_raw < N;
    const long long pt = live ? pt_raw : N - 1;
    const int v = (int)(pt / P);
    const int partner = (v + B) % V;
    const int b = v % B;
    const int pix = min(max(choose[pt], 0), H * W - 1);      // an index outside the crop reads its nearest end, never outside the map
    const int y = pix / W, x = pix - y * W;
    float ref[4];      // the original row: it enters every plane's sum and, behind fuse_conv, the residual
    load4(feat + (((long long)v * H + y) * W + x) * C + c * 4, ref);
    const T* src = feat + (long long)partner * H * W * C + c * 4;
    const float* hm = homog + (long long)v * 12;
#pragma unroll 1
    for (int dz = 0; dz < D; ++dz) {
      asm volatile("" ::: "memory");      // the plane loop re-reads its weights from LDS: hoisted out of it they fill the VGPRs and spill (v2_head.hip)
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
        const float4 wv = *reinterpret_cast<const float4*>(w + kV1W1 + o * 32 + c * 4);
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
      const float2 bias1 = *reinterpret_cast<const float2*>(w + kV1B1 + 2 * c);
      const float h1a = relu_nan(p2[0] + bias1.x), h1b = relu_nan(p2[1] + bias1.y);
      // volume_conv.1: this lane's two inputs of all 8 outputs, the same exchange: lane c ends with output c
      float q8[8], q4[4], q2[2];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float2 wv = *reinterpret_cast<const float2*>(w + kV1W2 + j * 16 + 2 * c);
        q8[j] = fmaf(h1b, wv.y, h1a * wv.x);
      }
#pragma unroll
      for (int o = 0; o < 4; ++o) q4[o] = (b2 ? q8[o + 4] : q8[o]) + __shfl_xor(b2 ? q8[o] : q8[o + 4], 4);
#pragma unroll
      for (int o = 0; o < 2; ++o) q2[o] = (b1 ? q4[o + 2] : q4[o]) + __shfl_xor(b1 ? q4[o] : q4[o + 2], 2);
      const float q1 = (b0 ? q2[1] : q2[0]) + __shfl_xor(b0 ? q2[0] : q2[1], 1);
      const float h2 = relu_nan(q1 + w[kV1B2 + c]);
      // volume_conv.2: one product per lane and a butterfly sum, which leaves the same bits in all 8 lanes
      float pv = h2 * w[kV1W3 + c];
      pv += __shfl_xor(pv, 4);
      pv += __shfl_xor(pv, 2);
      pv += __shfl_xor(pv, 1);
      pv = relu_nan(pv + w[kV1B3]);
      if (c == (dz & 7)) {
        xr[dz] = pv;
        if (planes != nullptr && live) planes[pt * D + dz] = pv;
      }
    }
    __syncthreads();
    // fuse_conv.0 (24 -> 32, ReLU): channels 4c .. 4c + 3 into the row's second half
    float4 a = v1_layer32<24>(w + kV1FA, w + kV1FAb, xr, c);
    a.x = relu_nan(a.x); a.y = relu_nan(a.y); a.z = relu_nan(a.z); a.w = relu_nan(a.w);
    *reinterpret_cast<float4*>(xr + 32 + c * 4) = a;
    __syncthreads();
    // fuse_conv.2 (32 -> 32, no ReLU behind it), the residual, one ReLU
    a = v1_layer32<32>(w + kV1FB, w + kV1FBb, xr + 32, c);
    a.x = relu_nan(ref[0] + a.x); a.y = relu_nan(ref[1] + a.y); a.z = relu_nan(ref[2] + a.z); a.w = relu_nan(ref[3] + a.w);
    if (live) *reinterpret_cast<float4*>(fused32 + pt * 32 + c * 4) = a;
    // no barrier here: the next pass writes planes into 0 .. 23 of the rows, which nothing reads behind the first barrier above, and
    // writes 32 .. 63 only behind its own first barrier, which every thread reaches after this read
  }
}

int launch_v1_fused_points(int feat_dtype, const float* table, const void* feat, const float* homog, const float* depths, const int* choose,
                           float* fused32, float* planes, int V, int B, int P, int D, int H, int W, int Vh, hipStream_t s) {
  RGBM_REQUIRE(table && feat && homog && depths && choose && fused32, "v1_fused_points arguments");
  RGBM_REQUIRE((((uintptr_t)feat | (uintptr_t)fused32 | (uintptr_t)planes) & 15) == 0 && ((uintptr_t)table & 3) == 0,
               "v1_fused_points: feat, fused32 and planes must be 16-byte aligned (a lane moves 16-byte pieces of the rows)");
  RGBM_REQUIRE(feat_dtype == F32 || feat_dtype == BF16 || feat_dtype == F16, "v1_fused_points: fp32, bf16 or f16 feature maps (a split-pair net hands its fp32 copy)");
  RGBM_REQUIRE(B > 0 && V == 2 * B && (Vh == B || Vh == V) && P > 0 && D == 24 && H > 0 && W > 0 && (long long)H * W < (1ll << 31) / 32,
               "v1_fused_points: V = 2B views, heads for B or 2B of them, 24 planes");
  const long long N = (long long)Vh * P;
  int n_cu = 0;
  if (int rc = persistent_grid_cus(&n_cu)) return rc;
  const long long passes = (N + kV1Points - 1) / kV1Points;
  const long long cap = (long long)kV1GroupsPerCu * n_cu;
  const unsigned grid = (unsigned)(passes < cap ? passes : cap);
  if (feat_dtype == BF16)
    hipLaunchKernelGGL(v1_fused_points_kernel<unsigned short>, dim3(grid), dim3(512), 0, s, table, (const unsigned short*)feat, homog, depths, choose,
                       fused32, planes, V, B, P, D, H, W, N);
  else if (feat_dtype == F16)
    hipLaunchKernelGGL(v1_fused_points_kernel<f16_t>, dim3(grid), dim3(512), 0, s, table, (const f16_t*)feat, homog, depths, choose, fused32, planes,
                       V, B, P, D, H, W, N);
  else
    hipLaunchKernelGGL(v1_fused_points_kernel<float>, dim3(grid), dim3(512), 0, s, table, (const float*)feat, homog, depths, choose, fused32, planes,
                       V, B, P, D, H, W, N);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace rgbm
