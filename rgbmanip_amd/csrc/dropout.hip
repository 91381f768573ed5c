// Seeded Dropout2d of PSPNet (pspnet.py:122,150,154: p = 0.15 after up_1 and after up_2, active in the reference as shipped, which
// never calls .eval()): one keep decision per (pose, view, site, channel), drawn here into a per-handle factor buffer that the
// up-sampling tap combination (upconv.hip) multiplies into its epilogue.
//
// Generator (DESIGN.md "Seeded Dropout2d"; restated in numpy by tests/test_dropout_host.py):
//   key   = pose << 10 | view << 9 | site << 8 | channel        (pose: global pose index, view 0/1, site 0 = up_1, 1 = up_2)
//   z     = mix64(mix64(seed) + key * 0x9E3779B97F4A7C15)       (mod 2^64; mix64 = the splitmix64 finaliser)
//   keep  = (z >> 40) >= thresh,  thresh = round(p * 2^24)
//   factor = keep ? scale : 0,    scale = fp32(1 / (1 - p))
// The pose index is the handle's device counter plus the pose's place in the batch: the counter is read by every workgroup and
// advanced by B by the last one to finish (a ticket), so consecutive forwards, graph replays included, continue one sequence.
#include "common.h"
#include "kernels.h"

namespace rgbm {

namespace {

__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// state[0]: pose counter, state[1]: ticket of the workgroups that have read it (0 between launches)
__global__ __launch_bounds__(256) void dropout_masks_kernel(float* __restrict__ masks, unsigned long long* __restrict__ state, int B,
                                                            unsigned thresh, float scale, unsigned long long seed_mixed, int advance) {
  __shared__ unsigned long long base_s;
  if (threadIdx.x == 0) base_s = __atomic_load_n(&state[0], __ATOMIC_RELAXED);
  __syncthreads();
  const unsigned long long base = base_s;
  const int total = 2 * B * kDropoutPerView;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int v = i / kDropoutPerView, r = i - v * kDropoutPerView;
    const int view = v >= B ? 1 : 0;
    const int site = r >= 256 ? 1 : 0;
    const int c = r - 256 * site;
    const unsigned long long pose = base + (unsigned long long)(v - view * B);
    const unsigned long long key = pose << 10 | (unsigned long long)view << 9 | (unsigned long long)site << 8 | (unsigned long long)c;
    const unsigned long long z = mix64(seed_mixed + key * 0x9E3779B97F4A7C15ull);
    masks[i] = (unsigned)(z >> 40) >= thresh ? scale : 0.f;
  }
  __syncthreads();      // every thread of this workgroup is past its read of base_s (and so the workgroup past its read of state[0])
  if (threadIdx.x == 0) {
    const unsigned long long t = atomicAdd(&state[1], 1ull);
    if (t == gridDim.x - 1) {       // the last workgroup: all others have read the counter
      state[1] = 0;
      if (advance) __atomic_store_n(&state[0], base + (unsigned long long)B, __ATOMIC_RELAXED);
    }
  }
}

unsigned long long mix64_host(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

}  // namespace

unsigned dropout_threshold(float p) { return (unsigned)llround((double)p * 16777216.0); }
float dropout_scale(float p) { return (float)(1.0 / (1.0 - (double)p)); }

int launch_dropout_masks(float* masks, unsigned long long* state, int B, float p, unsigned long long seed, int advance, hipStream_t s) {
  RGBM_REQUIRE(masks && state && B > 0 && (long long)B * 2 * kDropoutPerView < (1ll << 31), "dropout masks arguments");
  RGBM_REQUIRE(p > 0.f && p < 1.f, "dropout p must lie in (0, 1)");
  const int total = 2 * B * kDropoutPerView;
  const int blocks = (total + 255) / 256;
  const unsigned grid = (unsigned)(blocks < 1024 ? blocks : 1024);
  hipLaunchKernelGGL(dropout_masks_kernel, dim3(grid), dim3(256), 0, s, masks, state, B, dropout_threshold(p), dropout_scale(p),
                     mix64_host(seed), advance);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace rgbm
