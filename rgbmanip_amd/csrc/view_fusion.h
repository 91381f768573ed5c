// Host-side launchers of view_fusion.hip: the cross-view attention stack and the depth head of the baseline network
// (lib/network_baseline.py:553-562, lib/fusion.py).
#pragma once
#include "common.h"

namespace rgbm {

constexpr int kVfBlocks = 4, kVfDim = 32, kVfHeads = 4, kVfDk = 8;
// one nn.Linear(32, 32): weight [out][in] row-major, then the 32 biases
constexpr int kVfLinearFloats = kVfDim * kVfDim + kVfDim;
// the stack's weights on the device: [block 0..3][fusion1, fusion2][linears.0 .. linears.3][kVfLinearFloats]
constexpr int kVfWeightFloats = kVfBlocks * 2 * 4 * kVfLinearFloats;
// depth_head on the device: layer 0 (64 x 32 weights, 64 biases), layer 2 (32 x 64, 32), layer 4 (1 x 32, 1)
constexpr int kDhW0 = 0, kDhB0 = kDhW0 + 64 * 32, kDhW1 = kDhB0 + 64, kDhB1 = kDhW1 + 32 * 64, kDhW2 = kDhB1 + 32, kDhB2 = kDhW2 + 32;
constexpr int kDepthHeadFloats = kDhB2 + 1;
constexpr int kVfMinPoints = 32, kVfMaxPoints = 4096;

// ten [B][P][32] fp32 buffers: q / k / v of both directions and two ping-pong pairs
size_t view_fusion_scratch_bytes(int B, int P);
// x1 / x2 / y1 / y2 [B][P][32] fp32 (16-byte aligned; y may not alias x).  n_dirs_last = 1: the last block computes fusion1 only and y2 is
// not written.  Every pose is computed by its own workgroups in a fixed order: two calls give the same bytes, whatever B.
int launch_view_fusion(const float* w, const float* x1, const float* x2, int B, int P, float* y1, float* y2, void* scratch, size_t scratch_bytes,
                       int n_dirs_last, hipStream_t s);
// x [n][32] -> out [n] = relu(W2 relu(W1 relu(W0 x + b0) + b1) + b2); pf (optional): x copied into channels 0..31 of rows of stride ldpf
int launch_depth_head(const float* w, const float* x, long long n, float* out, float* pf, int ldpf, hipStream_t s);
int launch_fill_nan(float* p, long long n, hipStream_t s);

}  // namespace rgbm
