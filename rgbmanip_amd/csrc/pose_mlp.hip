// The per-point layers of the pose MLP of a bf16 net in two kernels (network_v5.py:471-483), gfx950.
//   pose_mlp1_kernel: PF96 (fp32) -> f16 -> pose_mlp1.0 (96 -> 128, ReLU) -> pose_mlp1.2 (128 -> 128, ReLU) -> Q128b (f16) + the slices' column sums
//   pose_mlp2_kernel: Q128b -> pose_mlp2.0 (128 -> 256, per-view bias, ReLU) -> pose_mlp2.2 (256 -> 256, ReLU) -> the slices' column sums ONLY
// The mean of pose_mlp1's output over a view's points feeds pose_mlp2.0's bias: that dependency is the one kernel boundary.  As per-layer
// launches (four implicit GEMMs, a conversion, two mean kernels) the chain moved 1.9 GB per batch-256 step, 1.1 GB of it the two
// 256-channel per-point tensors whose only consumer is a mean over points; here the f16 copy of PF96, pose_mlp1.0's output and both
// 256-channel tensors stay in LDS.
// Both kernels: 8 waves, one persistent workgroup per CU walking (view, slice) units of P / kMeanSplit points in slabs of 128.  A wave owns
// 16 (pose_mlp1) or 32 (pose_mlp2) output channels of both layers and keeps their weights in registers as MFMA A operands for the whole
// launch, read straight from the layers' f16 weight arrays ([Cout][Kpad]: a lane's 8 consecutive K are one 16-byte load); the slab's
// activations lie in LDS as [point][channel] f16 rows, 16 bytes of padding per row (rows 4 banks apart: a ds_read_b128 of 16 rows is
// conflict-free), and are the B operands: 8 consecutive channels of a point are one ds_read_b128.  Y^T = W X^T: the accumulators hold
// 4 consecutive channels of one point, packed to f16 they are one 8-byte LDS write of the next layer's B rows.
// Rounding: to f16 (saturating, as pack_chunk does) exactly where the per-layer launches store a tensor - behind every ReLU, and the last
// layer's output before it is summed; sums over K ascend in fp32 in the MFMA.  The two paths differ by fp32 summation order only.
// Column sums: a lane adds its points in ascending slab / tile order, the lanes of a channel are added by a fixed butterfly: no atomics,
// the same bits on every run and for every grid size.  Layout [V][kMeanSplit][C], what launch_mean_points_partial writes.
#include "common.h"
#include "kernels.h"
#include "prof.h"

namespace rgbm {

typedef __attribute__((ext_vector_type(16))) float f32x16;

namespace pose {
constexpr int SLAB = kPoseMlpSlab;
constexpr int LD96 = 96 + 8, LD128 = 128 + 8, LD256 = 256 + 8;      // f16 elements per LDS row
constexpr size_t LDS1 = (size_t)SLAB * (LD96 + 2 * LD128) * sizeof(f16_t);
constexpr size_t LDS2 = (size_t)SLAB * (LD128 + LD256) * sizeof(f16_t) + 2 * 256 * sizeof(float);
static_assert(LDS1 <= 160 * 1024 && LDS2 <= 160 * 1024, "pose MLP: a slab's activations must fit the LDS");

// ReLU, then the saturating f16 rounding of pack_chunk: x < 0 -> 0, x > 65504 -> 65504, NaN stays NaN (both comparisons are false)
__device__ __forceinline__ float relu_sat(float x) {
  const float r = x < 0.f ? 0.f : x;
  return r > 65504.f ? 65504.f : r;
}
__device__ __forceinline__ f16x4 relu_f16x4(float a, float b, float c, float d) {
  f16x4 h;
  h[0] = (f16_t)relu_sat(a); h[1] = (f16_t)relu_sat(b); h[2] = (f16_t)relu_sat(c); h[3] = (f16_t)relu_sat(d);
  // the packed quad exists HERE: hipcc otherwise makes the comparisons of a whole tile first and keeps (then spills) their 64 masks
  unsigned long long bits = __builtin_bit_cast(unsigned long long, h);
  asm volatile("" : "+v"(bits));
  return __builtin_bit_cast(f16x4, bits);
}
}  // namespace pose

struct PoseMlpArgs {
  const float* pf96;            // [V * P][96] fp32
  const f16_t* w[4];            // the four layers' weights, [Cout][ldw[l]] f16 (pose_mlp2.0: its per-point half, 128 columns)
  int ldw[4];
  const float* b1; const float* b2; const float* b4;      // biases of pose_mlp1.0 / pose_mlp1.2 / pose_mlp2.2
  const float* vbias;           // [V][256]: pose_mlp2.0's bias + its global half applied to the view's mean
  f16_t* q128;                  // [V * P][128] f16: pose_mlp1's output
  float* part128;               // [V][kMeanSplit][128] column sums of q128
  float* part256;               // [V][kMeanSplit][256] column sums of pose_mlp2's (f16-rounded) output
  int P, units;                 // units = V * kMeanSplit
};

__global__ __launch_bounds__(512) void pose_mlp1_kernel(const PoseMlpArgs d) {
  using namespace pose;
  extern __shared__ __attribute__((aligned(16))) char pose_lds[];
  f16_t* xs = reinterpret_cast<f16_t*>(pose_lds);      // [SLAB][LD96]  the slab of PF96 in f16
  f16_t* hs = xs + SLAB * LD96;                        // [SLAB][LD128] pose_mlp1.0's output
  f16_t* os = hs + SLAB * LD128;                       // [SLAB][LD128] pose_mlp1.2's output, on its way to memory in whole rows
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lq = lane >> 4;            // 16x16x32: A row / B column lr, K = 8 lq + j; C column lr, rows 4 lq + i
  const int ch0 = wave * 16;
  if ((int)blockIdx.x >= d.units) return;
  f16x8 a1[3], a2[4];
#pragma unroll
  for (int ks = 0; ks < 3; ++ks) a1[ks] = *reinterpret_cast<const f16x8*>(d.w[0] + (long long)(ch0 + lr) * d.ldw[0] + ks * 32 + lq * 8);
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) a2[ks] = *reinterpret_cast<const f16x8*>(d.w[1] + (long long)(ch0 + lr) * d.ldw[1] + ks * 32 + lq * 8);
  const f32x4 bias1 = *reinterpret_cast<const f32x4*>(d.b1 + ch0 + lq * 4);
  const f32x4 bias2 = *reinterpret_cast<const f32x4*>(d.b2 + ch0 + lq * 4);
  const int slice = d.P / kMeanSplit, sps = slice / SLAB;      // points per slice, slabs per slice

  // a slab of PF96: SLAB x 24 float4, six per thread
  auto row0_of = [&](int unit, int sb) { return (long long)(unit / kMeanSplit) * d.P + (long long)(unit % kMeanSplit) * slice + sb * SLAB; };
  auto load_x = [&](long long row0, float4 (&pre)[6]) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const int idx = tid + 512 * i, r = idx / 24, c4 = idx % 24;
      pre[i] = *reinterpret_cast<const float4*>(d.pf96 + (row0 + r) * 96 + c4 * 4);
    }
  };
  auto store_x = [&](const float4 (&pre)[6]) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const int idx = tid + 512 * i, r = idx / 24, c4 = idx % 24;
      f16x4 h;
      h[0] = (f16_t)sat_f16(pre[i].x); h[1] = (f16_t)sat_f16(pre[i].y); h[2] = (f16_t)sat_f16(pre[i].z); h[3] = (f16_t)sat_f16(pre[i].w);
      *reinterpret_cast<f16x4*>(xs + r * LD96 + c4 * 4) = h;
    }
  };

  int unit = blockIdx.x, sb = 0;
  float4 pre[6];
  load_x(row0_of(unit, sb), pre);
  store_x(pre);
  float sum[4] = {0.f, 0.f, 0.f, 0.f};
  while (true) {
    const long long row0 = row0_of(unit, sb);
    __syncthreads();      // xs of this slab is complete; every wave is done with the previous slab's hs and os
    {
      f32x4 acc[8];
#pragma unroll
      for (int t = 0; t < 8; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 3; ++ks)
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          const f16x8 b = *reinterpret_cast<const f16x8*>(xs + (t * 16 + lr) * LD96 + ks * 32 + lq * 8);
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1[ks], b, acc[t], 0, 0, 0);
        }
#pragma unroll
      for (int t = 0; t < 8; ++t)
        *reinterpret_cast<f16x4*>(hs + (t * 16 + lr) * LD128 + ch0 + lq * 4) =
            relu_f16x4(acc[t][0] + bias1[0], acc[t][1] + bias1[1], acc[t][2] + bias1[2], acc[t][3] + bias1[3]);
    }
    __syncthreads();      // hs is complete; xs is free
    int nunit = unit, nsb = sb + 1;
    if (nsb == sps) { nsb = 0; nunit += gridDim.x; }
    const bool has_next = nunit < d.units;      // workgroup-uniform
    if (has_next) load_x(row0_of(nunit, nsb), pre);      // in flight under the second layer
    {
      f32x4 acc[8];
#pragma unroll
      for (int t = 0; t < 8; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          const f16x8 b = *reinterpret_cast<const f16x8*>(hs + (t * 16 + lr) * LD128 + ks * 32 + lq * 8);
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a2[ks], b, acc[t], 0, 0, 0);
        }
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const f16x4 h = relu_f16x4(acc[t][0] + bias2[0], acc[t][1] + bias2[1], acc[t][2] + bias2[2], acc[t][3] + bias2[3]);
        *reinterpret_cast<f16x4*>(os + (t * 16 + lr) * LD128 + ch0 + lq * 4) = h;
#pragma unroll
        for (int i = 0; i < 4; ++i) sum[i] += (float)h[i];
      }
    }
    if (has_next) store_x(pre);
    __syncthreads();      // os is complete
    // SLAB rows of 256 bytes out: 16 lanes per row
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = tid + 512 * i, r = idx >> 4, c = idx & 15;
      *reinterpret_cast<uint4*>(d.q128 + (row0 + r) * 128 + c * 8) = *reinterpret_cast<const uint4*>(os + r * LD128 + c * 8);
    }
    if (nsb == 0) {
      // the slice's column sums: the 16 lanes of a channel quad in a fixed butterfly
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float s = sum[i];
        s += __shfl_xor(s, 1); s += __shfl_xor(s, 2); s += __shfl_xor(s, 4); s += __shfl_xor(s, 8);
        sum[i] = s;
      }
      if (lr == 0) *reinterpret_cast<float4*>(d.part128 + (long long)unit * 128 + ch0 + lq * 4) = make_float4(sum[0], sum[1], sum[2], sum[3]);
#pragma unroll
      for (int i = 0; i < 4; ++i) sum[i] = 0.f;
    }
    if (!has_next) break;
    unit = nunit; sb = nsb;
  }
}

__global__ __launch_bounds__(512) void pose_mlp2_kernel(const PoseMlpArgs d) {
  using namespace pose;
  extern __shared__ __attribute__((aligned(16))) char pose_lds[];
  f16_t* xs = reinterpret_cast<f16_t*>(pose_lds);      // [SLAB][LD128] the slab of Q128b
  f16_t* hs = xs + SLAB * LD128;                       // [SLAB][LD256] pose_mlp2.0's output
  float* vb = reinterpret_cast<float*>(hs + SLAB * LD256);      // [256] the view's bias of pose_mlp2.0
  float* b4 = vb + 256;                                         // [256] pose_mlp2.2's bias
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 31, lh = lane >> 5;            // 32x32x16: A row / B column lr, K = 8 lh + j; C column lr, rows 8 g + 4 lh + i of register 4 g + i
  const int ch0 = wave * 32;
  if ((int)blockIdx.x >= d.units) return;
  // pose_mlp2.2's operands (64 registers) stay for the whole launch; pose_mlp2.0's (32) are fetched again for every slab behind the second
  // layer's last MFMA (8 KB per wave from L2, under the epilogue and the barrier): held across the second layer they left one B operand
  // in flight per MFMA.  The address passes through an empty asm so that hipcc does not hoist the loads back out of the slab loop
  f16x8 a3[8], a4[16];
  auto load_a3 = [&]() {
    const f16_t* p = d.w[2] + (long long)(ch0 + lr) * d.ldw[2] + lh * 8;
    asm volatile("" : "+v"(p));
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) a3[ks] = *reinterpret_cast<const f16x8*>(p + ks * 16);
  };
  load_a3();
#pragma unroll
  for (int ks = 0; ks < 16; ++ks) a4[ks] = *reinterpret_cast<const f16x8*>(d.w[3] + (long long)(ch0 + lr) * d.ldw[3] + ks * 16 + lh * 8);
  if (tid < 256) b4[tid] = d.b4[tid];
  const int slice = d.P / kMeanSplit, sps = slice / SLAB;

  // a slab of Q128b: SLAB x 16 chunks of 16 bytes, four per thread (chunk tid + 512 i: row (tid >> 4) + 32 i, chunk tid & 15 of the row)
  auto row0_of = [&](int unit, int sb) { return (long long)(unit / kMeanSplit) * d.P + (long long)(unit % kMeanSplit) * slice + sb * SLAB; };
  const int xr = tid >> 4, xc = (tid & 15) * 8;
  f32x4 pre0, pre1, pre2, pre3;      // (four named registers quads: as an array behind a reference hipcc kept them on the stack)
  auto load_x = [&](long long row0) {
    const f16_t* p = d.q128 + (row0 + xr) * 128 + xc;
    pre0 = *reinterpret_cast<const f32x4*>(p);
    pre1 = *reinterpret_cast<const f32x4*>(p + 32 * 128);
    pre2 = *reinterpret_cast<const f32x4*>(p + 64 * 128);
    pre3 = *reinterpret_cast<const f32x4*>(p + 96 * 128);
  };
  auto store_x = [&]() {
    f16_t* p = xs + xr * LD128 + xc;
    *reinterpret_cast<f32x4*>(p) = pre0;
    *reinterpret_cast<f32x4*>(p + 32 * LD128) = pre1;
    *reinterpret_cast<f32x4*>(p + 64 * LD128) = pre2;
    *reinterpret_cast<f32x4*>(p + 96 * LD128) = pre3;
  };

  int unit = blockIdx.x, sb = 0;
  load_x(row0_of(unit, sb));
  store_x();
  float sum[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) sum[i] = 0.f;
  while (true) {
    // (every wave is past the second barrier of the previous slab: nobody reads the previous view's vb any more)
    if (sb == 0 && tid < 256) vb[tid] = d.vbias[(long long)(unit / kMeanSplit) * 256 + tid];
    __syncthreads();      // xs, vb (and b4) are complete; every wave is done with the previous slab's hs
#pragma unroll
    for (int tp = 0; tp < 2; ++tp) {      // two 32-point tiles side by side: two independent accumulator chains
      f32x16 acc[2];
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[u][i] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 8; ++ks)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const f16x8 b = *reinterpret_cast<const f16x8*>(xs + ((tp * 2 + u) * 32 + lr) * LD128 + ks * 16 + lh * 8);
          acc[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a3[ks], b, acc[u], 0, 0, 0);
        }
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int c = ch0 + 8 * g + 4 * lh;
          const f32x4 bv = *reinterpret_cast<const f32x4*>(vb + c);
          *reinterpret_cast<f16x4*>(hs + ((tp * 2 + u) * 32 + lr) * LD256 + c) =
              relu_f16x4(acc[u][4 * g] + bv[0], acc[u][4 * g + 1] + bv[1], acc[u][4 * g + 2] + bv[2], acc[u][4 * g + 3] + bv[3]);
          __builtin_amdgcn_sched_barrier(0);      // one channel quad at a time: hipcc otherwise makes all 64 comparisons first and spills their masks
        }
    }
    __syncthreads();      // hs is complete; xs is free
    int nunit = unit, nsb = sb + 1;
    if (nsb == sps) { nsb = 0; nunit += gridDim.x; }
    const bool has_next = nunit < d.units;      // workgroup-uniform
    if (has_next) load_x(row0_of(nunit, nsb));      // in flight under the second layer
#pragma unroll
    for (int tp = 0; tp < 2; ++tp) {
      f32x16 acc[2];
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[u][i] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 16; ++ks)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const f16x8 b = *reinterpret_cast<const f16x8*>(hs + ((tp * 2 + u) * 32 + lr) * LD256 + ks * 16 + lh * 8);
          acc[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a4[ks], b, acc[u], 0, 0, 0);
        }
      // what the per-layer path stored as G256b and then averaged: bias, ReLU, f16 - summed here instead
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 bv = *reinterpret_cast<const f32x4*>(b4 + ch0 + 8 * g + 4 * lh);
          const f16x4 h = relu_f16x4(acc[u][4 * g] + bv[0], acc[u][4 * g + 1] + bv[1], acc[u][4 * g + 2] + bv[2], acc[u][4 * g + 3] + bv[3]);
#pragma unroll
          for (int i = 0; i < 4; ++i) sum[4 * g + i] += (float)h[i];
          __builtin_amdgcn_sched_barrier(0);
        }
    }
    if (has_next) { load_a3(); store_x(); }
    if (nsb == 0) {
      // the slice's column sums: the 32 lanes of a channel in a fixed butterfly
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        float s = sum[i];
        s += __shfl_xor(s, 1); s += __shfl_xor(s, 2); s += __shfl_xor(s, 4); s += __shfl_xor(s, 8); s += __shfl_xor(s, 16);
        sum[i] = s;
      }
      if (lr == 0) {
#pragma unroll
        for (int g = 0; g < 4; ++g)
          *reinterpret_cast<float4*>(d.part256 + (long long)unit * 256 + ch0 + 8 * g + 4 * lh) =
              make_float4(sum[4 * g], sum[4 * g + 1], sum[4 * g + 2], sum[4 * g + 3]);
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) sum[i] = 0.f;
    }
    if (!has_next) break;
    unit = nunit; sb = nsb;
  }
}

bool pose_mlp_fits(int P) { return P > 0 && P % (kMeanSplit * kPoseMlpSlab) == 0; }

static int pose_mlp_args(const PoseMlpDesc& d, PoseMlpArgs& a) {
  RGBM_REQUIRE(d.V > 0 && pose_mlp_fits(d.P), "pose MLP: points per view must be a multiple of 8 slabs of 128");
  RGBM_REQUIRE(d.pf96 && d.q128 && d.part128 && d.part256 && d.vbias && d.bias[0] && d.bias[1] && d.bias[3], "pose MLP: buffers");
  const int K[4] = {96, 128, 128, 256};
  for (int l = 0; l < 4; ++l) {
    RGBM_REQUIRE(d.w[l] != nullptr && d.ldw[l] >= K[l] && d.ldw[l] % 8 == 0 && ((uintptr_t)d.w[l] & 15) == 0, "pose MLP: weight rows of 16-byte chunks");
    a.w[l] = reinterpret_cast<const f16_t*>(d.w[l]);
    a.ldw[l] = d.ldw[l];
  }
  RGBM_REQUIRE((long long)d.V * kMeanSplit < (1ll << 31), "pose MLP: views");
  a.pf96 = d.pf96; a.b1 = d.bias[0]; a.b2 = d.bias[1]; a.b4 = d.bias[3]; a.vbias = d.vbias;
  a.q128 = reinterpret_cast<f16_t*>(d.q128); a.part128 = d.part128; a.part256 = d.part256;
  a.P = d.P; a.units = d.V * kMeanSplit;
  return 0;
}

// profiler rows 30 / 32; algorithmic flops: the two layers' multiply-adds; bytes: what has to move (PF96 in + Q128b out; Q128b in) + the sums
int launch_pose_mlp1(const PoseMlpDesc& d, hipStream_t s) {
  PoseMlpArgs a;
  if (int rc = pose_mlp_args(d, a)) return rc;
  int n_cu = 0;
  if (int rc = persistent_grid_cus(&n_cu)) return rc;
  if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(pose_mlp1_kernel), (int)pose::LDS1)) return rc;
  const double n = (double)d.V * d.P;
  prof_begin_launch(s, 30, 2.0 * n * (96.0 * 128 + 128.0 * 128), n * (96 * 4 + 128 * 2) + (double)a.units * 128 * 4);
  hipLaunchKernelGGL(pose_mlp1_kernel, dim3(a.units < n_cu ? a.units : n_cu), dim3(512), pose::LDS1, s, a);
  prof_end_launch(s);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_pose_mlp2(const PoseMlpDesc& d, hipStream_t s) {
  PoseMlpArgs a;
  if (int rc = pose_mlp_args(d, a)) return rc;
  int n_cu = 0;
  if (int rc = persistent_grid_cus(&n_cu)) return rc;
  if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(pose_mlp2_kernel), (int)pose::LDS2)) return rc;
  const double n = (double)d.V * d.P;
  prof_begin_launch(s, 32, 2.0 * n * (128.0 * 256 + 256.0 * 256), n * 128 * 2 + (double)a.units * 256 * 4);
  hipLaunchKernelGGL(pose_mlp2_kernel, dim3(a.units < n_cu ? a.units : n_cu), dim3(512), pose::LDS2, s, a);
  prof_end_launch(s);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace rgbm
