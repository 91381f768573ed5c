// Cross-view attention stack (lib/fusion.py: ViewFusion, embed_dim 32, 4 heads, depth 4) and the depth head of the baseline network
// (lib/network_baseline.py:553-562, 631-634), gfx950.  Everything here is fp32, whatever the handle's storage type.
//
// A block of the stack is two multi-head cross-attentions that both read the block's inputs:
//   y1 = W4a concat_h softmax_k((W1a x1 + b)(W2a x2 + b)^T / sqrt(8)) (W3a x2 + b) + b4a + x1       (fusion1: queries from view 1)
//   y2 = W4b concat_h softmax_k((W1b x2 + b)(W2b x1 + b)^T / sqrt(8)) (W3b x1 + b) + b4b + x2       (fusion2: queries from view 2)
// It runs as two launches: vf_proj_kernel writes q / k / v of both directions ([2][B][P][32]), vf_attn_kernel walks the keys flash-style
// and finishes with the output projection and the residual.  No score or probability ever reaches memory.
//
// vf_attn_kernel: a workgroup owns 64 queries of one (pose, direction); wave w owns head w.  Keys come in tiles of 32 through LDS (double
// buffered, the next tile's global loads in flight under the current tile's arithmetic).  A 32 key x 32 query score tile is four
// v_mfma_f32_32x32x2_f32 (d_k = 8) computed TRANSPOSED - A = the key tile, B = the queries - so that a lane holds the scores of ONE query
// (column l & 31) against 16 keys (rows 8 (r >> 2) + 4 (l >> 5) + (r & 3)): the running maximum, the running sum and the 8 output sums of a
// query live in its two lanes and the key walk needs no cross-lane step.  The two lanes of a query see disjoint halves of every tile; their
// states are merged once, behind the last tile, in a fixed order.  P V is 8 FMAs per score on the vector pipe, which is what bounds the
// kernel; the matrix pipe's quarter of the work runs beside it.  The softmax is exp2((s - m) log2(e) / sqrt(8)) with m the running maximum
// of the raw scores: the subtraction is done before the scaling, so a score of +-200 costs no accuracy in its probability.
#include "view_fusion.h"

namespace rgbm {

namespace vf {
constexpr int KT = 32;                 // keys per tile
constexpr int KLD = 33;                // row stride of the key tile in LDS: lane = key reads one dword per K step, conflict-free
constexpr int QB = 64;                 // queries per workgroup (two groups of 32 per wave)
constexpr int OLD = 36;                // row stride of the attention output staged for the output projection (16-byte rows, no 32-way conflict)
constexpr float kExpScale = 1.4426950408889634f * 0.35355339059327373f;      // log2(e) / sqrt(d_k)
}  // namespace vf

typedef __attribute__((ext_vector_type(16))) float f32x16;

__device__ __forceinline__ float vf_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// q / k / v of one block: view 0 rows (x1) feed fusion1's queries and fusion2's keys / values, view 1 rows (x2) the other way round.
// One thread per row; the weights are wave-uniform reads.
__global__ __launch_bounds__(256) void vf_proj_kernel(const float* __restrict__ x1, const float* __restrict__ x2, const float* __restrict__ w,
                                                      float* __restrict__ Q, float* __restrict__ K, float* __restrict__ V, long long n,
                                                      long long dir_stride) {
  const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
  if (row >= n) return;
  const int view = blockIdx.y;
  const float* xp = (view ? x2 : x1) + row * 32;
  float x[32];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float4 t = *reinterpret_cast<const float4*>(xp + 4 * i);
    x[4 * i] = t.x; x[4 * i + 1] = t.y; x[4 * i + 2] = t.z; x[4 * i + 3] = t.w;
  }
  for (int m = 0; m < 3; ++m) {
    const int dir = m == 0 ? view : 1 - view;
    const float* wm = w + (dir * 4 + m) * kVfLinearFloats;
    float* op = (m == 0 ? Q : m == 1 ? K : V) + dir * dir_stride + row * 32;
    for (int oc = 0; oc < 4; ++oc) {
      float acc[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) acc[c] = 0.f;
#pragma unroll
      for (int i = 0; i < 32; ++i)
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[c] = fmaf(wm[(oc * 8 + c) * 32 + i], x[i], acc[c]);
#pragma unroll
      for (int c = 0; c < 8; ++c) acc[c] += wm[1024 + oc * 8 + c];
      *reinterpret_cast<float4*>(op + oc * 8) = make_float4(acc[0], acc[1], acc[2], acc[3]);
      *reinterpret_cast<float4*>(op + oc * 8 + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
    }
  }
}

// grid (ceil(P / 64), directions, B), 256 threads.  w: the block's weights [2][4][kVfLinearFloats]; xa / ya: view 1's rows (direction 0),
// xb / yb: view 2's (direction 1); all [B][P][32].
__global__ __launch_bounds__(256) void vf_attn_kernel(const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ V,
                                                      const float* __restrict__ w, const float* __restrict__ xa, const float* __restrict__ xb,
                                                      float* __restrict__ ya, float* __restrict__ yb, int P, long long dir_stride) {
  using namespace vf;
  __shared__ float Ks[2][KT * KLD];
  __shared__ __attribute__((aligned(16))) float Vs[2][KT * 32];
  __shared__ __attribute__((aligned(16))) float Os[QB * OLD];
  const int t = threadIdx.x, lane = t & 63, hd = t >> 6, h = lane >> 5, c = lane & 31;
  const int dir = blockIdx.y, b = blockIdx.z, q0 = blockIdx.x * QB;
  const long long base = dir * dir_stride + (long long)b * P * 32;
  const float* Qp = Q + base;
  const float* Kp = K + base;
  const float* Vp = V + base;

  // B operand of the four K steps: Q[query][2 step + h] of this wave's head; a query past P reads the last row and is never stored
  float qb[2][4];
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const int q = q0 + g * 32 + c;
    const int qc = q < P ? q : P - 1;
#pragma unroll
    for (int st = 0; st < 4; ++st) qb[g][st] = Qp[(long long)qc * 32 + hd * 8 + 2 * st + h];
  }
  float mx[2], sum[2], acc[2][8];
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    mx[g] = -INFINITY; sum[g] = 0.f;
#pragma unroll
    for (int d = 0; d < 8; ++d) acc[g][d] = 0.f;
  }

  const int lr = t >> 3, lc = (t & 7) * 4;      // this thread's 16 bytes of a key / value tile: row lr (0..31), floats lc .. lc + 3
  const int nt = P / KT;
  float4 kr = *reinterpret_cast<const float4*>(Kp + (long long)lr * 32 + lc);
  float4 vr = *reinterpret_cast<const float4*>(Vp + (long long)lr * 32 + lc);
  {
    float* kd = &Ks[0][lr * KLD + lc];
    kd[0] = kr.x; kd[1] = kr.y; kd[2] = kr.z; kd[3] = kr.w;
    *reinterpret_cast<float4*>(&Vs[0][lr * 32 + lc]) = vr;
  }
  __syncthreads();
  for (int tile = 0; tile < nt; ++tile) {
    const int cur = tile & 1;
    const bool more = tile + 1 < nt;
    if (more) {
      const long long r = (long long)((tile + 1) * KT + lr) * 32 + lc;
      kr = *reinterpret_cast<const float4*>(Kp + r);
      vr = *reinterpret_cast<const float4*>(Vp + r);
    }
    // S^T = K_tile Q^T: A[i = key c][k = h] per step, B[k = h][j = query c]
    float a[4];
#pragma unroll
    for (int st = 0; st < 4; ++st) a[st] = Ks[cur][c * KLD + hd * 8 + 2 * st + h];
    f32x16 s[2];
#pragma unroll
    for (int g = 0; g < 2; ++g) {
#pragma unroll
      for (int r = 0; r < 16; ++r) s[g][r] = 0.f;
#pragma unroll
      for (int st = 0; st < 4; ++st) s[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[st], qb[g][st], s[g], 0, 0, 0);
    }
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      float tm = s[g][0];
#pragma unroll
      for (int r = 1; r < 16; ++r) tm = fmaxf(tm, s[g][r]);
      const float mn = fmaxf(mx[g], tm);
      const float corr = vf_exp2((mx[g] - mn) * kExpScale);      // first tile: exp2(-inf) = 0
      mx[g] = mn;
      sum[g] *= corr;
#pragma unroll
      for (int d = 0; d < 8; ++d) acc[g][d] *= corr;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s[g][r] = vf_exp2((s[g][r] - mn) * kExpScale);
        sum[g] += s[g][r];
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = 8 * (r >> 2) + 4 * h + (r & 3);      // the row of S^T this lane holds in register r
      const float4 v0 = *reinterpret_cast<const float4*>(&Vs[cur][key * 32 + hd * 8]);
      const float4 v1 = *reinterpret_cast<const float4*>(&Vs[cur][key * 32 + hd * 8 + 4]);
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const float p = s[g][r];
        acc[g][0] = fmaf(p, v0.x, acc[g][0]); acc[g][1] = fmaf(p, v0.y, acc[g][1]);
        acc[g][2] = fmaf(p, v0.z, acc[g][2]); acc[g][3] = fmaf(p, v0.w, acc[g][3]);
        acc[g][4] = fmaf(p, v1.x, acc[g][4]); acc[g][5] = fmaf(p, v1.y, acc[g][5]);
        acc[g][6] = fmaf(p, v1.z, acc[g][6]); acc[g][7] = fmaf(p, v1.w, acc[g][7]);
      }
    }
    if (more) {      // the other buffer was last read in the previous iteration, which every wave left through the barrier below
      float* kd = &Ks[cur ^ 1][lr * KLD + lc];
      kd[0] = kr.x; kd[1] = kr.y; kd[2] = kr.z; kd[3] = kr.w;
      *reinterpret_cast<float4*>(&Vs[cur ^ 1][lr * 32 + lc]) = vr;
    }
    __syncthreads();
  }

  // merge the two lanes of a query (lane c: keys 4h .. of every group of 8, lane c + 32 the others), lower half first in both lanes
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const float mo = __shfl_xor(mx[g], 32), so = __shfl_xor(sum[g], 32);
    const float m_lo = h ? mo : mx[g], m_hi = h ? mx[g] : mo;
    const float s_lo = h ? so : sum[g], s_hi = h ? sum[g] : so;
    const float mt = fmaxf(m_lo, m_hi);
    const float c_lo = vf_exp2((m_lo - mt) * kExpScale), c_hi = vf_exp2((m_hi - mt) * kExpScale);
    const float inv = 1.0f / (s_lo * c_lo + s_hi * c_hi);
#pragma unroll
    for (int d = 0; d < 8; ++d) {
      const float ao = __shfl_xor(acc[g][d], 32);
      const float a_lo = h ? ao : acc[g][d], a_hi = h ? acc[g][d] : ao;
      const float o = (a_lo * c_lo + a_hi * c_hi) * inv;
      if (h == 0) Os[(g * 32 + c) * OLD + hd * 8 + d] = o;
    }
  }
  __syncthreads();

  // output projection + bias + residual: lane = query, wave = 8 output channels
  const int wv = __builtin_amdgcn_readfirstlane(hd);
  const float* w4 = w + (dir * 4 + 3) * kVfLinearFloats;
  float o[32];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float4 tv = *reinterpret_cast<const float4*>(&Os[lane * OLD + 4 * i]);
    o[4 * i] = tv.x; o[4 * i + 1] = tv.y; o[4 * i + 2] = tv.z; o[4 * i + 3] = tv.w;
  }
  float y[8];
#pragma unroll
  for (int cc = 0; cc < 8; ++cc) y[cc] = 0.f;
#pragma unroll
  for (int i = 0; i < 32; ++i)
#pragma unroll
    for (int cc = 0; cc < 8; ++cc) y[cc] = fmaf(w4[(wv * 8 + cc) * 32 + i], o[i], y[cc]);
  const int q = q0 + lane;
  if (q < P) {
    const long long off = ((long long)b * P + q) * 32 + wv * 8;
    const float* xr = (dir ? xb : xa) + off;
    float* yr = (dir ? yb : ya) + off;
    const float4 r0 = *reinterpret_cast<const float4*>(xr), r1 = *reinterpret_cast<const float4*>(xr + 4);
    const float* b4 = w4 + 1024 + wv * 8;
    *reinterpret_cast<float4*>(yr) = make_float4(y[0] + b4[0] + r0.x, y[1] + b4[1] + r0.y, y[2] + b4[2] + r0.z, y[3] + b4[3] + r0.w);
    *reinterpret_cast<float4*>(yr + 4) = make_float4(y[4] + b4[4] + r1.x, y[5] + b4[5] + r1.y, y[6] + b4[6] + r1.z, y[7] + b4[7] + r1.w);
  }
}

size_t view_fusion_scratch_bytes(int B, int P) { return 10 * align_up((size_t)B * P * 32 * sizeof(float), 256); }

int launch_view_fusion(const float* w, const float* x1, const float* x2, int B, int P, float* y1, float* y2, void* scratch, size_t scratch_bytes,
                       int n_dirs_last, hipStream_t s) {
  RGBM_REQUIRE(w && x1 && x2 && y1 && scratch && (y2 || n_dirs_last == 1), "view_fusion arguments");
  RGBM_REQUIRE(B >= 1 && B <= 65535, "view_fusion: 1 <= B <= 65535 poses per call");
  RGBM_REQUIRE(P >= kVfMinPoints && P <= kVfMaxPoints && P % 32 == 0, "view_fusion: P must be a multiple of 32 in [32, 4096]");
  RGBM_REQUIRE(n_dirs_last == 1 || n_dirs_last == 2, "view_fusion: directions of the last block");
  RGBM_REQUIRE((((uintptr_t)x1 | (uintptr_t)x2 | (uintptr_t)y1 | (uintptr_t)y2 | (uintptr_t)scratch) & 15) == 0, "view_fusion: 16-byte aligned buffers");
  RGBM_REQUIRE(y1 != x1 && y1 != x2 && (y2 == nullptr || (y2 != x1 && y2 != x2)), "view_fusion: outputs may not alias inputs");
  RGBM_REQUIRE(scratch_bytes >= view_fusion_scratch_bytes(B, P), "view_fusion: scratch too small: need " + std::to_string(view_fusion_scratch_bytes(B, P)));
  const long long n = (long long)B * P;
  const size_t one = align_up((size_t)n * 32 * sizeof(float), 256);
  const long long dir_stride = n * 32;
  char* sp = (char*)scratch;
  float* Q = (float*)sp;      // [2][n][32]: the two directions dir_stride apart (the padding behind the pair is unused)
  float* K = (float*)(sp + 2 * one);
  float* V = (float*)(sp + 4 * one);
  float* pp[2][2] = {{(float*)(sp + 6 * one), (float*)(sp + 7 * one)}, {(float*)(sp + 8 * one), (float*)(sp + 9 * one)}};
  const float* in1 = x1;
  const float* in2 = x2;
  for (int blk = 0; blk < kVfBlocks; ++blk) {
    const bool last = blk == kVfBlocks - 1;
    float* o1 = last ? y1 : pp[blk & 1][0];
    float* o2 = last ? y2 : pp[blk & 1][1];
    const float* wb = w + (size_t)blk * 2 * 4 * kVfLinearFloats;
    hipLaunchKernelGGL(vf_proj_kernel, dim3((unsigned)((n + 255) / 256), 2), dim3(256), 0, s, in1, in2, wb, Q, K, V, n, dir_stride);
    RGBM_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(vf_attn_kernel, dim3((unsigned)((P + vf::QB - 1) / vf::QB), last ? n_dirs_last : 2, B), dim3(256), 0, s, Q, K, V, wb, in1,
                       in2, o1, o2, P, dir_stride);
    RGBM_CHECK_HIP(hipGetLastError());
    in1 = o1; in2 = o2;
  }
  return 0;
}

// ---------------------------------------------------------------- depth_head: 32 -> 64 ReLU -> 32 ReLU -> 1 ReLU, one thread per point
__global__ __launch_bounds__(256) void depth_head_kernel(const float* __restrict__ w, const float* __restrict__ x, long long n,
                                                         float* __restrict__ out, float* __restrict__ pf, int ldpf) {
  const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
  if (row >= n) return;
  float xi[32];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float4 t = *reinterpret_cast<const float4*>(x + row * 32 + 4 * i);
    xi[4 * i] = t.x; xi[4 * i + 1] = t.y; xi[4 * i + 2] = t.z; xi[4 * i + 3] = t.w;
    if (pf) *reinterpret_cast<float4*>(pf + row * ldpf + 4 * i) = t;
  }
  float h2[32];
#pragma unroll
  for (int j = 0; j < 32; ++j) h2[j] = 0.f;
  for (int oc = 0; oc < 8; ++oc) {      // eight of layer 0's outputs at a time, folded into layer 2's sums at once
    float h1[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) h1[c] = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i)
#pragma unroll
      for (int c = 0; c < 8; ++c) h1[c] = fmaf(w[kDhW0 + (oc * 8 + c) * 32 + i], xi[i], h1[c]);
#pragma unroll
    for (int c = 0; c < 8; ++c) h1[c] = fmaxf(h1[c] + w[kDhB0 + oc * 8 + c], 0.f);
#pragma unroll
    for (int j = 0; j < 32; ++j)
#pragma unroll
      for (int c = 0; c < 8; ++c) h2[j] = fmaf(w[kDhW1 + j * 64 + oc * 8 + c], h1[c], h2[j]);
  }
  float d = 0.f;
#pragma unroll
  for (int j = 0; j < 32; ++j) d = fmaf(w[kDhW2 + j], fmaxf(h2[j] + w[kDhB1 + j], 0.f), d);
  out[row] = fmaxf(d + w[kDhB2], 0.f);
}

int launch_depth_head(const float* w, const float* x, long long n, float* out, float* pf, int ldpf, hipStream_t s) {
  RGBM_REQUIRE(w && x && out && n > 0 && n <= (1ll << 31) * 256 - 256, "depth_head arguments");
  RGBM_REQUIRE(((uintptr_t)x & 15) == 0 && (pf == nullptr || (((uintptr_t)pf & 15) == 0 && ldpf >= 32 && ldpf % 4 == 0)), "depth_head: 16-byte aligned rows");
  hipLaunchKernelGGL(depth_head_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w, x, n, out, pf, ldpf);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

__global__ void fill_nan_kernel(float* __restrict__ p, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = __uint_as_float(0x7fc00000u);
}

int launch_fill_nan(float* p, long long n, hipStream_t s) {
  RGBM_REQUIRE(p && n > 0, "fill_nan arguments");
  hipLaunchKernelGGL(fill_nan_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p, n);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace rgbm
