// Feature-record cache of the PSPNet (DESIGN.md "Feature cache"): a view's 32-channel feature map depends on its frame alone, so a
// caller that meets the same frame in two forwards keeps the map in a pool of records and hands the stages behind the PSPNet a slot
// table instead of images.  Two streaming copies, 16 bytes per lane and access, every wave on consecutive 1 KiB pieces:
//   store:  workspace feature map of view v             -> pool record slots[v]
//   gather: pool record slot1[b] / slot2[b]             -> workspace feature map of view b / B + b  ([view1 batch ; view2 batch])
// and the kernel that turns the ten outputs of a pose whose slot lies outside the pool into NaN (the gather wrote zeros for it and
// read nothing).
// And the content key of a prepared crop ("content keys"): two 64-bit sums of a mixed (word, position) pair over
// the crop's 32-bit words, by which a caller that gets frames as fresh arrays recognises one it has kept the map of.
#include "kernels.h"

namespace rgbm {
namespace {

constexpr int kCopyThreads = 256;
constexpr int kCopyUnroll = 4;       // 16-byte loads in flight per lane

__device__ __forceinline__ void copy_part(const uint4* __restrict__ src, uint4* __restrict__ dst, long long n16, bool zero) {
  const long long step = (long long)gridDim.x * kCopyThreads;
  long long i = (long long)blockIdx.x * kCopyThreads + threadIdx.x;
  if (zero) {
    for (; i < n16; i += step) dst[i] = make_uint4(0u, 0u, 0u, 0u);
    return;
  }
  for (; i + (kCopyUnroll - 1) * step < n16; i += kCopyUnroll * step) {
    uint4 r[kCopyUnroll];
#pragma unroll
    for (int u = 0; u < kCopyUnroll; ++u) r[u] = src[i + u * step];
#pragma unroll
    for (int u = 0; u < kCopyUnroll; ++u) dst[i + u * step] = r[u];
  }
  for (; i < n16; i += step) dst[i] = src[i];
}

// grid (pieces of a view, V).  part16 / n16 / rec16: offset of this part inside a record, its length, the record's length, in 16-byte units
__global__ __launch_bounds__(kCopyThreads) void feat_store_kernel(const uint4* __restrict__ src, uint4* __restrict__ pool,
                                                                  const int* __restrict__ slots, int pool_records, long long part16,
                                                                  long long n16, long long rec16) {
  const int v = blockIdx.y;
  const int slot = slots[v];
  if ((unsigned)slot >= (unsigned)pool_records) return;      // outside the pool: nothing is written
  copy_part(src + (long long)v * n16, pool + (long long)slot * rec16 + part16, n16, false);
}

__global__ __launch_bounds__(kCopyThreads) void feat_gather_kernel(const uint4* __restrict__ pool, uint4* __restrict__ dst,
                                                                   const int* __restrict__ slot1, const int* __restrict__ slot2, int B,
                                                                   int pool_records, long long part16, long long n16, long long rec16) {
  const int v = blockIdx.y;
  const int slot = v < B ? slot1[v] : slot2[v - B];
  const bool bad = (unsigned)slot >= (unsigned)pool_records;      // outside the pool: zeros in, nothing read (the pose's outputs become NaN)
  copy_part(pool + (long long)(bad ? 0 : slot) * rec16 + part16, dst + (long long)v * n16, n16, bad);
}

struct OutPtrs { float* p[10]; int n[10]; };

// one workgroup per pose: every output of a pose with a slot outside the pool <- NaN
__global__ __launch_bounds__(256) void feat_bad_slot_nan_kernel(const int* __restrict__ slot1, const int* __restrict__ slot2,
                                                                int pool_records, OutPtrs o) {
  const int b = blockIdx.x;
  if ((unsigned)slot1[b] < (unsigned)pool_records && (unsigned)slot2[b] < (unsigned)pool_records) return;
  const float nan = __uint_as_float(0x7fc00000u);
#pragma unroll
  for (int k = 0; k < 10; ++k) {
    float* q = o.p[k] + (long long)b * o.n[k];
    for (int i = threadIdx.x; i < o.n[k]; i += 256) q[i] = nan;
  }
}

int copy_grid_x(int V, long long n16, unsigned* gx) {
  int n_cu = 0;
  if (int rc = persistent_grid_cus(&n_cu)) return rc;
  // about 16 workgroups per CU over all views, at least one full unrolled pass per workgroup
  const long long per_pass = (long long)kCopyThreads * kCopyUnroll;
  long long want = ((long long)n_cu * 16 + V - 1) / V;
  const long long cap = (n16 + per_pass - 1) / per_pass;
  if (want > cap) want = cap;
  if (want < 1) want = 1;
  *gx = (unsigned)want;
  return 0;
}

// ---- content key.  key[v][k] = sum over the words w_i of view v of mix((w_i | i << 32) ^ seed_k)  (mod 2^64), mix = the splitmix64
// finaliser.  Integer arithmetic only and the sum commutes: lane sums, wave shuffles, LDS partials and one 64-bit vector atomic per
// workgroup and key word give the same bits in any order.
constexpr int kKeyThreads = 256;
constexpr int kKeyUnroll = 4;        // 16-byte loads in flight per lane
constexpr unsigned long long kKeySeed0 = 0x9E3779B97F4A7C15ull, kKeySeed1 = 0xD1B54A32D192ED03ull;

__device__ __forceinline__ unsigned long long key_mix(unsigned long long x) {
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

__device__ __forceinline__ void key_add(unsigned w, unsigned i, unsigned long long& k0, unsigned long long& k1) {
  const unsigned long long x = (unsigned long long)w | ((unsigned long long)i << 32);
  k0 += key_mix(x ^ kKeySeed0);
  k1 += key_mix(x ^ kKeySeed1);
}

// grid (pieces of a view, V).  A row starts at any 4-byte address: up to three head words bring it to a 16-byte boundary, the body is
// read 16 bytes per lane, up to three tail words follow (head and tail: workgroup 0 of the view).  keys: zero on entry.
__global__ __launch_bounds__(kKeyThreads) void crop_fingerprint_kernel(const unsigned* __restrict__ img, int n_words,
                                                                       unsigned long long* __restrict__ keys) {
  const int v = blockIdx.y;
  const unsigned* row = img + (long long)v * n_words;
  int head = (int)(((16u - (unsigned)((uintptr_t)row & 15u)) & 15u) >> 2);
  if (head > n_words) head = n_words;
  const int n16 = (n_words - head) >> 2;
  const int tail0 = head + 4 * n16;                      // first tail word; n_words - tail0 in [0, 3]
  const uint4* body = reinterpret_cast<const uint4*>(row + head);
  unsigned long long k0 = 0, k1 = 0;
  const int step = (int)gridDim.x * kKeyThreads;
  int i = (int)blockIdx.x * kKeyThreads + (int)threadIdx.x;
  for (; i < n16 - (kKeyUnroll - 1) * step; i += kKeyUnroll * step) {      // (n16 < 2^29: the bound cannot wrap)
    uint4 r[kKeyUnroll];
#pragma unroll
    for (int u = 0; u < kKeyUnroll; ++u) r[u] = body[i + u * step];
#pragma unroll
    for (int u = 0; u < kKeyUnroll; ++u) {
      const unsigned w0 = (unsigned)(head + 4 * (i + u * step));
      key_add(r[u].x, w0, k0, k1); key_add(r[u].y, w0 + 1, k0, k1); key_add(r[u].z, w0 + 2, k0, k1); key_add(r[u].w, w0 + 3, k0, k1);
    }
  }
  for (; i < n16; i += step) {
    const uint4 r = body[i];
    const unsigned w0 = (unsigned)(head + 4 * i);
    key_add(r.x, w0, k0, k1); key_add(r.y, w0 + 1, k0, k1); key_add(r.z, w0 + 2, k0, k1); key_add(r.w, w0 + 3, k0, k1);
  }
  if (blockIdx.x == 0) {
    const int t = (int)threadIdx.x;
    if (t < head) key_add(row[t], (unsigned)t, k0, k1);
    if (t < n_words - tail0) key_add(row[tail0 + t], (unsigned)(tail0 + t), k0, k1);
  }
  for (int off = 32; off > 0; off >>= 1) {
    k0 += __shfl_down(k0, off, 64);
    k1 += __shfl_down(k1, off, 64);
  }
  __shared__ unsigned long long part[2][kKeyThreads / 64];
  const int wave = (int)threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { part[0][wave] = k0; part[1][wave] = k1; }
  __syncthreads();
  if (threadIdx.x < 2) {
    unsigned long long s = 0;
#pragma unroll
    for (int w = 0; w < kKeyThreads / 64; ++w) s += part[threadIdx.x][w];
    atomicAdd(&keys[2 * v + (int)threadIdx.x], s);
  }
}

}  // namespace

int launch_crop_fingerprint(const float* img, int V, int n_words, unsigned long long* keys_out, hipStream_t s) {
  RGBM_REQUIRE(img && keys_out && V > 0 && V < 65536 && n_words >= 1, "crop_fingerprint arguments");
  RGBM_REQUIRE((((uintptr_t)img) & 3) == 0 && (((uintptr_t)keys_out) & 7) == 0, "crop_fingerprint: 4-byte aligned words, 8-byte aligned keys");
  int n_cu = 0;
  if (int rc = persistent_grid_cus(&n_cu)) return rc;
  // about 8 workgroups per CU over all views; no more than one 16-byte load per lane would fill (a lone view still spreads over the CUs)
  long long want = ((long long)n_cu * 8 + V - 1) / V;
  const long long cap = ((long long)(n_words / 4) + kKeyThreads - 1) / kKeyThreads;
  if (want > cap) want = cap;
  if (want < 1) want = 1;
  RGBM_CHECK_HIP(hipMemsetAsync(keys_out, 0, (size_t)V * 2 * sizeof(unsigned long long), s));
  hipLaunchKernelGGL(crop_fingerprint_kernel, dim3((unsigned)want, (unsigned)V), dim3(kKeyThreads), 0, s,
                     reinterpret_cast<const unsigned*>(img), n_words, keys_out);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_feature_store(const void* src, void* pool, const int* slots, int V, int pool_records, size_t part_off, size_t part_bytes,
                         size_t record_bytes, hipStream_t s) {
  RGBM_REQUIRE(src && pool && slots && V > 0 && V < 65536 && pool_records > 0, "feature_store arguments");
  RGBM_REQUIRE(part_bytes > 0 && ((part_off | part_bytes | record_bytes) & 15) == 0 && part_off + part_bytes <= record_bytes &&
               (((uintptr_t)src | (uintptr_t)pool) & 15) == 0, "feature_store: 16-byte aligned buffers and sizes");
  unsigned gx = 0;
  if (int rc = copy_grid_x(V, (long long)(part_bytes / 16), &gx)) return rc;
  hipLaunchKernelGGL(feat_store_kernel, dim3(gx, (unsigned)V), dim3(kCopyThreads), 0, s, reinterpret_cast<const uint4*>(src),
                     reinterpret_cast<uint4*>(pool), slots, pool_records, (long long)(part_off / 16), (long long)(part_bytes / 16),
                     (long long)(record_bytes / 16));
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_feature_gather(const void* pool, void* dst, const int* slot1, const int* slot2, int B, int pool_records, size_t part_off,
                          size_t part_bytes, size_t record_bytes, hipStream_t s) {
  RGBM_REQUIRE(pool && dst && slot1 && slot2 && B > 0 && 2 * B < 65536 && pool_records > 0, "feature_gather arguments");
  RGBM_REQUIRE(part_bytes > 0 && ((part_off | part_bytes | record_bytes) & 15) == 0 && part_off + part_bytes <= record_bytes &&
               (((uintptr_t)dst | (uintptr_t)pool) & 15) == 0, "feature_gather: 16-byte aligned buffers and sizes");
  unsigned gx = 0;
  if (int rc = copy_grid_x(2 * B, (long long)(part_bytes / 16), &gx)) return rc;
  hipLaunchKernelGGL(feat_gather_kernel, dim3(gx, (unsigned)(2 * B)), dim3(kCopyThreads), 0, s, reinterpret_cast<const uint4*>(pool),
                     reinterpret_cast<uint4*>(dst), slot1, slot2, B, pool_records, (long long)(part_off / 16), (long long)(part_bytes / 16),
                     (long long)(record_bytes / 16));
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_feature_bad_slot_nan(const int* slot1, const int* slot2, int B, int pool_records, float* const out[10], const int per_pose[10],
                                hipStream_t s) {
  RGBM_REQUIRE(slot1 && slot2 && B > 0 && pool_records > 0, "feature_bad_slot_nan arguments");
  OutPtrs o;
  for (int k = 0; k < 10; ++k) {
    RGBM_REQUIRE(out[k] != nullptr && per_pose[k] > 0, "feature_bad_slot_nan outputs");
    o.p[k] = out[k]; o.n[k] = per_pose[k];
  }
  hipLaunchKernelGGL(feat_bad_slot_nan_kernel, dim3((unsigned)B), dim3(256), 0, s, slot1, slot2, pool_records, o);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace rgbm
