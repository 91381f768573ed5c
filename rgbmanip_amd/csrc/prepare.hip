// Device-side AdaPoseEstimator_v5.prepare_model_input, batched over frames:
//   /root/reference/models/pose_estimator/AdaPose/interface_v5.py:58-170  (mask bbox -> crop window -> resized mask ->
//     1024 `choose` indices -> resized + normalised RGB -> crop-adjusted intrinsics)
//   /root/reference/models/pose_estimator/AdaPose/lib/utils.py:10-38      (get_bbox: square window, multiple of 40, <= 440)
// The reference does this per sample on the host with numpy + cv2.resize (INTER_NEAREST for the mask, INTER_LINEAR for the
// float image); OpenCV is not available in the build container, so the resize arithmetic is OpenCV's documented one, the
// same as in oracle/postproc_ref.py (half-pixel centres, edge clamp, no antialias; sx = floor(dx*scale) for nearest) —
// "parity unpinned" at exactly this step, pinned (bit-exact) against the oracle restatement.
// The reference draws the 1024-subset with the global np.random.shuffle; here it is a seeded hash: candidate i of frame f
// gets key = mix32(seed, f, i) and the 1024 smallest (key, i) pairs are kept in index order — a uniformly random ordered
// subset like the reference's, but reproducible (oracle: postproc_ref.choose_subset_hash).
// Built with -ffp-contract=off: numpy rounds every elementwise op separately.
#include "common.h"
#include "kernels.h"
#include "quantize.h"

namespace rgbm {

namespace {

constexpr int PRE_THREADS = 1024;

// ---- cropped intrinsics of a window: interface_v5.py:153-168 (python floats = fp64), shared by the two kernels that write Kcrop ----
__device__ inline void crop_intrinsics(const double* __restrict__ Ki, int rmin, int rmax, int cmin, int cmax, int S, double* __restrict__ Ko) {
  const double ratio = (double)S / (double)(rmax - rmin);
  const double ccx = (double)(cmin + cmax) / 2.0, ccy = (double)(rmin + rmax) / 2.0;
  const double csx = (double)(cmax - cmin + 1), csy = (double)(rmax - rmin + 1);
  Ko[0] = Ki[0] * ratio; Ko[1] = 0.0; Ko[2] = (Ki[2] - (ccx - csx / 2.0)) * ratio;
  Ko[3] = 0.0; Ko[4] = Ki[4] * ratio; Ko[5] = (Ki[5] - (ccy - csy / 2.0)) * ratio;
  Ko[6] = 0.0; Ko[7] = 0.0; Ko[8] = 1.0;
}
// an empty mask (the reference returns None -> default bbox): the identity, so that what is computed from it stays finite
__device__ inline void identity_intrinsics(double* __restrict__ Ko) {
  for (int i = 0; i < 9; ++i) Ko[i] = (i % 4 == 0) ? 1.0 : 0.0;
}

// ---- 1. mask bounding box -> crop window (get_bbox) -> cropped intrinsics ------------------------------------------
// frame_map (optional): frame f reads image / mask number frame_map[f] of the arrays it is given (a view queue); a negative
// entry is a missing view and behaves like an all-zero mask.  K, the outputs and the subset hash stay indexed by f.
__global__ __launch_bounds__(PRE_THREADS) void mask_window_kernel(const unsigned char* __restrict__ mask, const double* __restrict__ K,
                                                                   const int* __restrict__ frame_map,
                                                                   int H, int W, int S, int* __restrict__ window /*[N,4]*/,
                                                                   double* __restrict__ Kcrop /*[N,9]*/, int* __restrict__ valid) {
  __shared__ int s_y1, s_x1, s_y2, s_x2;
  const int f = blockIdx.x, t = threadIdx.x;
  if (t == 0) { s_y1 = H; s_x1 = W; s_y2 = -1; s_x2 = -1; }
  __syncthreads();
  const int sf = frame_map ? frame_map[f] : f;
  const unsigned char* m = mask + (long long)(sf < 0 ? 0 : sf) * H * W;
  int y1 = H, x1 = W, y2 = -1, x2 = -1;
  for (int i = t; sf >= 0 && i < H * W; i += PRE_THREADS) {
    if (m[i]) {
      const int y = i / W, x = i - y * W;
      y1 = min(y1, y); y2 = max(y2, y); x1 = min(x1, x); x2 = max(x2, x);
    }
  }
  if (y2 >= 0) { atomicMin(&s_y1, y1); atomicMax(&s_y2, y2); atomicMin(&s_x1, x1); atomicMax(&s_x2, x2); }
  __syncthreads();
  if (t != 0) return;
  int* w = window + f * 4;
  double* Ko = Kcrop + f * 9;
  if (s_y2 < 0) {                                   // empty mask: the reference returns None -> default bbox
    w[0] = 0; w[1] = 40; w[2] = 0; w[3] = 40;
    identity_intrinsics(Ko);
    valid[f] = 0;
    return;
  }
  // lib/utils.py:10-38 (integer arithmetic of the reference; image fixed at 480 x 640 there, H x W here)
  int win = (max(s_y2 - s_y1, s_x2 - s_x1) / 40 + 1) * 40;
  win = min(win, 440);
  const int cy = (s_y1 + s_y2) / 2, cx = (s_x1 + s_x2) / 2;
  int rmin = cy - win / 2, rmax = cy + win / 2, cmin = cx - win / 2, cmax = cx + win / 2;
  if (rmin < 0) { rmax = rmax - rmin; rmin = 0; }
  if (cmin < 0) { cmax = cmax - cmin; cmin = 0; }
  if (rmax > H) { rmin = rmin - (rmax - H); rmax = H; }
  if (cmax > W) { cmin = cmin - (cmax - W); cmax = W; }
  w[0] = rmin; w[1] = rmax; w[2] = cmin; w[3] = cmax;
  crop_intrinsics(K + f * 9, rmin, rmax, cmin, cmax, S, Ko);
  valid[f] = 1;
}

// ---- 2. crop + resize: nearest mask, bilinear RGB, ToTensor [+ Normalize] -------------------------------------------
// NORM: ImageNet mean / std (interface_v5.py:52-54; interface_v4.py:52-55 for task "pots"); without it the resized crop itself is
// written (interface_v4.py:56-57: plain ToTensor for every other task).
// A frame pixel as the float32 the arithmetic below takes.  float frames: the value itself.  8-bit frames (a camera's bytes): byte b
// means fl32(b / 255), correctly rounded — numpy's float32(b) / float32(255) and what the upload path used to write as a float32
// frame.  The fp64 quotient rounded to float32 equals the correctly rounded float32 quotient for every byte value, b * (1 / 255.f)
// does not (126 of the 256 values are one ulp off, tools/check_div.py).
__device__ inline float pixel_value(float v) { return v; }
__device__ inline float pixel_value(unsigned char b) { return (float)((double)b / 255.0); }

// INTER_LINEAR on a float image, one output pixel (dy, dx) of an h x w source window resized to S x S, all three channels: f = (d + 0.5) *
// scale - 0.5, clamp at both edges, weights in fp32.  The window's pixel (y, x) is base[((row0 + y) * pitch + col0 + x) * 3 + c]: a window
// inside a whole frame (crop_resize_kernel: row0 / col0 = the window's corner, pitch = W) or a packed window (crop_resize_windows_kernel:
// row0 = col0 = 0, pitch = w).  The ONE body both crop kernels run, so that what they write cannot drift apart.
template <typename Px, bool NORM>
__device__ inline void crop_bilinear(const Px* __restrict__ base, int row0, int col0, int pitch, int h, int w, int S, int dy, int dx,
                                     float* __restrict__ img /*[N,3,S,S]*/, int f, int p) {
  const int rmin = row0, cmin = col0, W = pitch;
  auto taps = [](int d, int n_src, int n_dst, int& i0, int& i1, float& a) {
    const double fl = ((double)d + 0.5) * ((double)n_src / (double)n_dst) - 0.5;
    int j = (int)floor(fl);
    a = (float)(fl - (double)j);
    if (j < 0) { j = 0; a = 0.f; }
    if (j >= n_src - 1) { i0 = n_src - 1; i1 = n_src - 1; a = 0.f; }
    else { i0 = j; i1 = j + 1; }
  };
  int y0, y1, x0, x1;
  float ay, ax;
  taps(dy, h, S, y0, y1, ay);
  taps(dx, w, S, x0, x1, ax);
  const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float p00 = pixel_value(base[((long long)(rmin + y0) * W + cmin + x0) * 3 + c]), p01 = pixel_value(base[((long long)(rmin + y0) * W + cmin + x1) * 3 + c]);
    const float p10 = pixel_value(base[((long long)(rmin + y1) * W + cmin + x0) * 3 + c]), p11 = pixel_value(base[((long long)(rmin + y1) * W + cmin + x1) * 3 + c]);
    const float top = p00 * (1.f - ax) + p01 * ax;
    const float bot = p10 * (1.f - ax) + p11 * ax;
    const float v = top * (1.f - ay) + bot * ay;
    if constexpr (NORM) img[((long long)f * 3 + c) * S * S + p] = (v - mean[c]) / stdv[c];
    else img[((long long)f * 3 + c) * S * S + p] = v;
  }
}

// INTER_NEAREST: sx = min(floor(dx * (src/dst)), src-1), fp64 like numpy's python-float scale
__device__ inline int nearest_tap(int d, int n_src, int n_dst) { return min((int)floor((double)d * ((double)n_src / (double)n_dst)), n_src - 1); }

template <typename Px, bool NORM>
__global__ void crop_resize_kernel(const Px* __restrict__ rgb /*[N,H,W,3]*/, const unsigned char* __restrict__ mask,
                                   const int* __restrict__ frame_map, const int* __restrict__ window, int N, int H, int W, int S,
                                   float* __restrict__ img /*[N,3,S,S]*/, unsigned char* __restrict__ small /*[N,S,S]*/) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)N * S * S) return;
  const int f = (int)(i / (S * S)), p = (int)(i - (long long)f * S * S), dy = p / S, dx = p - dy * S;
  const int rmin = window[f * 4 + 0], rmax = window[f * 4 + 1], cmin = window[f * 4 + 2], cmax = window[f * 4 + 3];
  const int h = rmax - rmin, w = cmax - cmin;
  const int ny = nearest_tap(dy, h, S), nx = nearest_tap(dx, w, S);
  const int mf = frame_map ? frame_map[f] : f;
  const int sf = mf < 0 ? 0 : mf;
  small[i] = (mf >= 0 && mask[((long long)sf * H + rmin + ny) * W + cmin + nx]) ? 1 : 0;
  crop_bilinear<Px, NORM>(rgb + (long long)sf * H * W * 3, rmin, cmin, W, h, w, S, dy, dx, img, f, p);
}

// ---- 2b. the same from packed windows (estimate() with hip_upload: "windows") ------------------------------------------
// The host has cut every frame's crop window out of the frame and of the mask and stored the windows back to back: frame f's h x w x 3
// pixels row-major at element 3 * offset[f] of pix, its h x w mask bytes at mask_pix + offset[f]; window[f] is what mask_window_kernel
// derives from the whole mask (the host restates its integer arithmetic, upload.mask_windows).  Same taps, same values, same arithmetic as
// crop_resize_kernel on the whole frames: img and small are bit-identical.  A window with no pixels (h or w <= 0: not what the host
// packs) is written as zeros instead of being read.
template <typename Px, bool NORM>
__global__ void crop_resize_windows_kernel(const Px* __restrict__ pix, const unsigned char* __restrict__ mask_pix,
                                           const long long* __restrict__ offset /*[N]*/, const int* __restrict__ window /*[N,4]*/, int N, int S,
                                           float* __restrict__ img /*[N,3,S,S]*/, unsigned char* __restrict__ small /*[N,S,S]*/) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)N * S * S) return;
  const int f = (int)(i / (S * S)), p = (int)(i - (long long)f * S * S), dy = p / S, dx = p - dy * S;
  const int h = window[f * 4 + 1] - window[f * 4 + 0], w = window[f * 4 + 3] - window[f * 4 + 2];
  if (h <= 0 || w <= 0) {
    small[i] = 0;
    for (int c = 0; c < 3; ++c) img[((long long)f * 3 + c) * S * S + p] = 0.f;
    return;
  }
  const long long off = offset[f];
  const int ny = nearest_tap(dy, h, S), nx = nearest_tap(dx, w, S);
  small[i] = mask_pix[off + (long long)ny * w + nx] ? 1 : 0;
  crop_bilinear<Px, NORM>(pix + off * 3, 0, 0, w, h, w, S, dy, dx, img, f, p);
}

// Kcrop and valid of packed windows: what mask_window_kernel writes once it has found the window.  valid_in 0 = an empty mask.
__global__ void window_intrinsics_kernel(const int* __restrict__ window, const int* __restrict__ valid_in, const double* __restrict__ K, int N,
                                         int S, double* __restrict__ Kcrop /*[N,9]*/, int* __restrict__ valid) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= N) return;
  const int* w = window + f * 4;
  if (!valid_in[f] || w[1] <= w[0] || w[3] <= w[2]) {
    identity_intrinsics(Kcrop + f * 9);
    valid[f] = 0;
    return;
  }
  crop_intrinsics(K + f * 9, w[0], w[1], w[2], w[3], S, Kcrop + f * 9);
  valid[f] = 1;
}

// ---- 3. choose: nonzero indices of the resized mask, ordered random P-subset or wrap padding -------------------------
__global__ __launch_bounds__(PRE_THREADS) void choose_kernel(const unsigned char* __restrict__ small, const int* __restrict__ window,
                                                              int S, int P, unsigned seed, int* __restrict__ choose /*[N,P]*/,
                                                              float* __restrict__ pts2d /*[N,P,2] or null*/, int* __restrict__ valid,
                                                              int frame0 /*hash index of frame 0: a batch prepared in pieces*/) {
  extern __shared__ unsigned short idx[];           // candidate pixel indices, in order (S*S <= 65536)
  __shared__ int wsum[PRE_THREADS / 64];
  __shared__ int s_total, s_cnt;
  const int f = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const unsigned char* m = small + (long long)f * S * S;
  const int per = (S * S + PRE_THREADS - 1) / PRE_THREADS;
  const int lo = t * per, hi = min(lo + per, S * S);

  // block-wide exclusive scan of a per-thread count, thread ranges are contiguous so order is preserved
  auto excl_scan = [&](int mine, int& total) {
    int incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int o = __shfl_up(incl, off);
      if (lane >= off) incl += o;
    }
    __syncthreads();                                // wsum free to overwrite
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    int base = 0, tot = 0;
    for (int k = 0; k < PRE_THREADS / 64; ++k) { if (k < wv) base += wsum[k]; tot += wsum[k]; }
    total = tot;
    return base + incl - mine;
  };

  int cnt = 0;
  for (int i = lo; i < hi; ++i) cnt += m[i] ? 1 : 0;
  int n;
  int pos = excl_scan(cnt, n);
  for (int i = lo; i < hi; ++i) if (m[i]) idx[pos++] = (unsigned short)i;
  __syncthreads();
  int* out = choose + (long long)f * P;
  if (n == 0 || !valid[f]) {                        // reference: None -> default bbox; keep the tensors finite
    for (int i = t; i < P; i += PRE_THREADS) out[i] = 0;
    if (t == 0) valid[f] = 0;
  } else if (n <= P) {
    for (int i = t; i < P; i += PRE_THREADS) out[i] = idx[i % n];                   // np.pad(choose, ..., "wrap")
  } else {
    // smallest threshold T with count(key <= T) >= P, by bisection over the 32-bit key space
    unsigned tlo = 0u, thi = 0xFFFFFFFFu;
    while (tlo < thi) {
      const unsigned mid = tlo + ((thi - tlo) >> 1);
      int c = 0;
      for (int i = t; i < n; i += PRE_THREADS) c += mix32(seed, (unsigned)(f + frame0), (unsigned)idx[i]) <= mid ? 1 : 0;
      if (t == 0) s_cnt = 0;
      __syncthreads();
      atomicAdd(&s_cnt, c);
      __syncthreads();
      const int tot = s_cnt;
      __syncthreads();
      if (tot >= P) thi = mid; else tlo = mid + 1;
    }
    const unsigned T = tlo;
    // keep every key < T and, in index order, as many key == T as still fit; ordered compaction (contiguous ranges per thread)
    const int per2 = (n + PRE_THREADS - 1) / PRE_THREADS;
    const int a = min(t * per2, n), b = min(a + per2, n);
    int c_lt = 0, c_eq = 0;
    for (int i = a; i < b; ++i) { const unsigned k = mix32(seed, (unsigned)(f + frame0), (unsigned)idx[i]); c_lt += k < T; c_eq += k == T; }
    int n_lt, n_eq;
    int p_lt = excl_scan(c_lt, n_lt);
    int p_eq = excl_scan(c_eq, n_eq);
    const int eq_keep = P - n_lt;                   // ties kept (>= 1)
    // output position of element i = (#kept with smaller index): kept_lt before + min(eq before, eq_keep)
    for (int i = a; i < b; ++i) {
      const unsigned k = mix32(seed, (unsigned)(f + frame0), (unsigned)idx[i]);
      if (k < T) { out[p_lt + min(p_eq, eq_keep)] = idx[i]; ++p_lt; }
      else if (k == T) { if (p_eq < eq_keep) out[p_lt + p_eq] = idx[i]; ++p_eq; }
    }
    (void)n_eq;
  }
  if (pts2d) {                                      // interface_v5.py:140-147 (float32 / python-float ratio, then + int)
    __syncthreads();
    const int rmin = window[f * 4 + 0], rmax = window[f * 4 + 1], cmin = window[f * 4 + 2];
    const float ratio = (float)((double)S / (double)(rmax - rmin));     // float32 array / python float stays float32 in numpy
    for (int i = t; i < P; i += PRE_THREADS) {
      const int c = out[i];
      pts2d[((long long)f * P + i) * 2 + 0] = (float)(c % S) / ratio + (float)cmin;
      pts2d[((long long)f * P + i) * 2 + 1] = (float)(c / S) / ratio + (float)rmin;
    }
  }
}

// ---- 3b. choose at native resolution: the v2 interface's "sample, then resize" (interface_v2.py:74-98) -----------------------
// The candidates are the non-zero pixels of mask[rmin:rmax, cmin:cmax] itself, index i = row * crop_w + col: up to 440 x 440 = 193 600 of
// them, past what 16-bit indices or an index list in LDS can hold.  The window's mask is staged as a bit mask (a wave ballots 64
// neighbouring pixels into two words: 24.2 KB for the largest window); counts, the key threshold and the ordered compaction are derived
// from it, every thread owning a contiguous range of words so that order is index order.  The subset rule is choose_kernel's on the native
// index; the at most P kept indices go to LDS, and from them pts2d = (cmin + col, rmin + row) - whole pixels of the frame - and
// choose = floor(row * ratio) * S + floor(col * ratio) with ratio = S / crop_w in fp64 like the python float (duplicates when crop_w > S).
constexpr int kNativeMaxWin = 440;                                                  // get_bbox's largest window (mask_window_kernel)
constexpr int kNativeWords = (kNativeMaxWin * kNativeMaxWin + 63) / 64 * 2;         // 32-bit words of the bit mask

// A second copy of the scan choose_kernel holds as a lambda, on purpose: moving that lambda out would change choose_kernel's code, whose
// instructions are kept what they were (contiguous thread ranges keep order).
__device__ inline int block_excl_scan(int mine, int& total, int* wsum) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int incl = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(incl, off);
    if (lane >= off) incl += o;
  }
  __syncthreads();                                // wsum free to overwrite
  if (lane == 63) wsum[wv] = incl;
  __syncthreads();
  int base = 0, tot = 0;
  for (int k = 0; k < PRE_THREADS / 64; ++k) { if (k < wv) base += wsum[k]; tot += wsum[k]; }
  total = tot;
  return base + incl - mine;
}

__global__ __launch_bounds__(PRE_THREADS) void choose_native_kernel(const unsigned char* __restrict__ mask, const int* __restrict__ frame_map,
                                                                     const int* __restrict__ window, int H, int W, int S, int P, unsigned seed,
                                                                     int* __restrict__ choose /*[N,P]*/, float* __restrict__ pts2d /*[N,P,2] or null*/,
                                                                     int* __restrict__ valid, int frame0) {
  extern __shared__ int sel[];                      // the kept native indices, in order (P of them at most)
  __shared__ unsigned bits[kNativeWords];
  __shared__ int wsum[PRE_THREADS / 64];
  __shared__ int s_cnt;
  const int f = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int rmin = window[f * 4 + 0], rmax = window[f * 4 + 1], cmin = window[f * 4 + 2], cmax = window[f * 4 + 3];
  const int h = rmax - rmin, w = cmax - cmin;
  const int mf = frame_map ? frame_map[f] : f;
  // a window the frame does not hold, or one larger than the bit mask, is not read (mask_window_kernel writes neither)
  const bool ok = valid[f] != 0 && mf >= 0 && h > 0 && w > 0 && h <= kNativeMaxWin && w <= kNativeMaxWin && rmin >= 0 && cmin >= 0 && rmax <= H && cmax <= W;
  const int M = ok ? h * w : 0;
  const int nwords = (M + 63) / 64 * 2;
  const unsigned char* m = mask + (long long)(mf < 0 ? 0 : mf) * H * W;
  for (int c = wv; c < nwords / 2; c += PRE_THREADS / 64) {
    const int i = c * 64 + lane;
    bool on = false;
    if (i < M) {
      const int row = i / w, col = i - row * w;
      on = m[(long long)(rmin + row) * W + cmin + col] != 0;
    }
    const unsigned long long b = __ballot(on);
    if (lane == 0) { bits[2 * c] = (unsigned)b; bits[2 * c + 1] = (unsigned)(b >> 32); }
  }
  __syncthreads();
  const int per = (nwords + PRE_THREADS - 1) / PRE_THREADS;
  const int lo = min(t * per, nwords), hi = min(lo + per, nwords);
  int cnt = 0;
  for (int k = lo; k < hi; ++k) cnt += __popc(bits[k]);
  int n;
  const int pos0 = block_excl_scan(cnt, n, wsum);
  int* out = choose + (long long)f * P;
  const unsigned hf = (unsigned)(f + frame0);
  int kept = 0;                                     // entries of sel
  if (n == 0) {                                     // reference: None -> default bbox; keep the tensors finite
    for (int i = t; i < P; i += PRE_THREADS) {
      out[i] = 0;
      if (pts2d) { pts2d[((long long)f * P + i) * 2 + 0] = 0.f; pts2d[((long long)f * P + i) * 2 + 1] = 0.f; }
    }
    if (t == 0) valid[f] = 0;
    return;
  } else if (n <= P) {
    int pos = pos0;
    for (int k = lo; k < hi; ++k)
      for (unsigned b = bits[k]; b; b &= b - 1) sel[pos++] = k * 32 + (__ffs(b) - 1);
    kept = n;
  } else {
    // smallest threshold T with count(key <= T) >= P, by bisection over the 32-bit key space
    unsigned tlo = 0u, thi = 0xFFFFFFFFu;
    while (tlo < thi) {
      const unsigned mid = tlo + ((thi - tlo) >> 1);
      int c = 0;
      for (int k = lo; k < hi; ++k)
        for (unsigned b = bits[k]; b; b &= b - 1) c += mix32(seed, hf, (unsigned)(k * 32 + (__ffs(b) - 1))) <= mid ? 1 : 0;
      if (t == 0) s_cnt = 0;
      __syncthreads();
      atomicAdd(&s_cnt, c);
      __syncthreads();
      const int tot = s_cnt;
      __syncthreads();
      if (tot >= P) thi = mid; else tlo = mid + 1;
    }
    const unsigned T = tlo;
    // keep every key < T and, in index order, as many key == T as still fit
    int c_lt = 0, c_eq = 0;
    for (int k = lo; k < hi; ++k)
      for (unsigned b = bits[k]; b; b &= b - 1) {
        const unsigned key = mix32(seed, hf, (unsigned)(k * 32 + (__ffs(b) - 1)));
        c_lt += key < T; c_eq += key == T;
      }
    int n_lt, n_eq;
    int p_lt = block_excl_scan(c_lt, n_lt, wsum);
    int p_eq = block_excl_scan(c_eq, n_eq, wsum);
    const int eq_keep = P - n_lt;                   // ties kept (>= 1)
    for (int k = lo; k < hi; ++k)
      for (unsigned b = bits[k]; b; b &= b - 1) {
        const int i = k * 32 + (__ffs(b) - 1);
        const unsigned key = mix32(seed, hf, (unsigned)i);
        if (key < T) { sel[p_lt + min(p_eq, eq_keep)] = i; ++p_lt; }
        else if (key == T) { if (p_eq < eq_keep) sel[p_lt + p_eq] = i; ++p_eq; }
      }
    (void)n_eq;
    kept = P;
  }
  __syncthreads();
  const double ratio = (double)S / (double)h;       // crop_w = rmax - rmin (interface_v2.py:94-95)
  for (int j = t; j < P; j += PRE_THREADS) {
    const int i = sel[j % kept];                    // np.pad(choose, ..., "wrap") when fewer than P
    const int row = i / w, col = i - row * w;       // the window is square: crop_w == w
    out[j] = (int)(floor((double)row * ratio) * (double)S + floor((double)col * ratio));
    if (pts2d) {
      pts2d[((long long)f * P + j) * 2 + 0] = (float)(cmin + col);
      pts2d[((long long)f * P + j) * 2 + 1] = (float)(rmin + row);
    }
  }
}

// ---- float frames -> bytes: the write side of an 8-bit view queue whose environment hands over float frames -----------------
// q(x) = min(max(rint(x * 255), 0), 255) with rint = round half to even, NaN -> 0: quantize_px of quantize.h.

// A streaming kernel, 4 bytes in and 1 byte out per pixel.  `head` (< 4) scalar pixels bring dst to a 4-byte boundary, then every
// lane turns 4 consecutive floats into one 32-bit store (a wave: 1 KiB read, 256 B written, both contiguous), then `n - head - 4 *
// quads` (< 4) scalar pixels.  src + head is only known to be 4-byte aligned: the copy below says so, and hipcc makes one 16-byte
// load of it (global loads need dword alignment only).
__global__ __launch_bounds__(256) void quantize_frames_kernel(const float* __restrict__ src, unsigned char* __restrict__ dst, size_t n,
                                                              unsigned head, size_t quads) {
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
  if (gid < head) dst[gid] = (unsigned char)quantize_px(src[gid]);
  const size_t tail0 = (size_t)head + 4 * quads;
  if (gid < n - tail0) dst[tail0 + gid] = (unsigned char)quantize_px(src[tail0 + gid]);
  const float* s4 = src + head;
  unsigned* d4 = reinterpret_cast<unsigned*>(dst + head);
  for (size_t q = gid; q < quads; q += step) {
    float v[4];
    __builtin_memcpy(v, __builtin_assume_aligned(s4 + 4 * q, 4), sizeof(v));
    d4[q] = quantize_px(v[0]) | (quantize_px(v[1]) << 8) | (quantize_px(v[2]) << 16) | (quantize_px(v[3]) << 24);
  }
}

// ---- ControlInterface.add_view (rl_pose.py:130-149): per-env mask extent, in rows (dim 1) and columns (dim 2) -----------
__global__ __launch_bounds__(PRE_THREADS) void mask_extent_kernel(const unsigned char* __restrict__ mask, int H, int W,
                                                                   int* __restrict__ ext /*[N,4] rmin,cmin,rmax,cmax*/,
                                                                   int* __restrict__ count /*[N]*/) {
  __shared__ int s_y1, s_x1, s_y2, s_x2, s_n;
  const int f = blockIdx.x, t = threadIdx.x;
  if (t == 0) { s_y1 = 2 * H; s_x1 = 2 * W; s_y2 = 0; s_x2 = 0; s_n = 0; }      // the reference's defaults for "no pixel"
  __syncthreads();
  const unsigned char* m = mask + (long long)f * H * W;
  int y1 = 2 * H, x1 = 2 * W, y2 = 0, x2 = 0, n = 0;
  for (int i = t; i < H * W; i += PRE_THREADS) {
    if (m[i]) {
      const int y = i / W, x = i - y * W;
      y1 = min(y1, y); y2 = max(y2, y); x1 = min(x1, x); x2 = max(x2, x); ++n;
    }
  }
  if (n) { atomicMin(&s_y1, y1); atomicMax(&s_y2, y2); atomicMin(&s_x1, x1); atomicMax(&s_x2, x2); atomicAdd(&s_n, n); }
  __syncthreads();
  if (t == 0) { ext[f * 4 + 0] = s_y1; ext[f * 4 + 1] = s_x1; ext[f * 4 + 2] = s_y2; ext[f * 4 + 3] = s_x2; count[f] = s_n; }
}

}  // namespace

// P = eye(4); P[:3, :] = K' @ E[:3, :] in fp64 (interface_v5.py:264-267: numpy float64, dot products summed left to right), stored
// as the float32 the network takes (interface_v5.py:269-270).  One thread per matrix.
__global__ void projection_kernel(const double* __restrict__ Kc, const double* __restrict__ E, float* __restrict__ P, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double* k = Kc + (size_t)i * 9;
  const double* e = E + (size_t)i * 16;
  float* p = P + (size_t)i * 16;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) p[r * 4 + c] = (float)((k[r * 3 + 0] * e[c] + k[r * 3 + 1] * e[4 + c]) + k[r * 3 + 2] * e[8 + c]);
  p[12] = 0.f; p[13] = 0.f; p[14] = 0.f; p[15] = 1.f;
}

int launch_projection(const double* Kc, const double* E, float* P, int n, hipStream_t s) {
  RGBM_REQUIRE(Kc && E && P && n > 0, "projection arguments");
  hipLaunchKernelGGL(projection_kernel, dim3((n + 127) / 128), dim3(128), 0, s, Kc, E, P, n);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_mask_extent(const unsigned char* mask, int N, int H, int W, int* ext, int* count, hipStream_t s) {
  RGBM_REQUIRE(mask && ext && count && N > 0 && H > 0 && W > 0, "mask_extent arguments");
  hipLaunchKernelGGL(mask_extent_kernel, dim3(N), dim3(PRE_THREADS), 0, s, mask, H, W, ext, count);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

unsigned prepare_mix32(unsigned seed, unsigned frame, unsigned idx) { return mix32(seed, frame, idx); }

namespace {
template <typename Px, bool NORM = true>
int prepare_inputs_impl(const Px* rgb, const unsigned char* mask, const double* K, const int* frame_map, int N, int H, int W, int S, int P,
                        unsigned seed, float* img, int* choose, float* pts2d, double* Kcrop, int* window, int* valid,
                        unsigned char* small_scratch, hipStream_t s, int frame0, int sample_mode = 0) {
  RGBM_REQUIRE(rgb && mask && K && img && choose && Kcrop && window && valid && small_scratch, "prepare_inputs arguments");
  RGBM_REQUIRE(sample_mode == 0 || sample_mode == 1, "prepare_inputs: sample_mode 0 (resize the mask, then sample) or 1 (sample at native resolution)");
  // the crop window is a square of up to 440 pixels shifted back into the frame (lib/utils.py:10-38 does it for 480 x 640): a
  // smaller frame could not hold it and the shifted window would start at a negative row / column
  RGBM_REQUIRE(N > 0 && H >= 440 && W >= 440 && S > 0 && P > 0 && S * S <= 65536, "prepare_inputs sizes (frames must be at least 440 x 440)");
  hipLaunchKernelGGL(mask_window_kernel, dim3(N), dim3(PRE_THREADS), 0, s, mask, K, frame_map, H, W, S, window, Kcrop, valid);
  const long long tot = (long long)N * S * S;
  hipLaunchKernelGGL((crop_resize_kernel<Px, NORM>), dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, rgb, mask, frame_map, window, N, H, W, S, img, small_scratch);
  if (sample_mode == 1) {      // the image, Kcrop and the window are the kernels' above; only the points are drawn differently
    RGBM_REQUIRE(P <= 8192, "prepare_inputs: native sampling keeps its P chosen indices in LDS (P <= 8192)");
    hipLaunchKernelGGL(choose_native_kernel, dim3(N), dim3(PRE_THREADS), (size_t)P * sizeof(int), s, mask, frame_map, window, H, W, S, P, seed, choose,
                       pts2d, valid, frame0);
    RGBM_CHECK_HIP(hipGetLastError());
    return 0;
  }
  const size_t lds = (size_t)S * S * sizeof(unsigned short);
  if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(choose_kernel), 150 * 1024)) return rc;
  hipLaunchKernelGGL(choose_kernel, dim3(N), dim3(PRE_THREADS), lds, s, small_scratch, window, S, P, seed, choose, pts2d, valid, frame0);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}
}  // namespace

int launch_prepare_inputs(const float* rgb, const unsigned char* mask, const double* K, const int* frame_map, int N, int H, int W, int S, int P,
                          unsigned seed, float* img, int* choose, float* pts2d, double* Kcrop, int* window, int* valid,
                          unsigned char* small_scratch, hipStream_t s, int frame0) {
  return prepare_inputs_impl(rgb, mask, K, frame_map, N, H, W, S, P, seed, img, choose, pts2d, Kcrop, window, valid, small_scratch, s, frame0);
}

int launch_prepare_inputs_u8(const unsigned char* rgb, const unsigned char* mask, const double* K, const int* frame_map, int N, int H, int W,
                             int S, int P, unsigned seed, float* img, int* choose, float* pts2d, double* Kcrop, int* window, int* valid,
                             unsigned char* small_scratch, hipStream_t s, int frame0) {
  return prepare_inputs_impl(rgb, mask, K, frame_map, N, H, W, S, P, seed, img, choose, pts2d, Kcrop, window, valid, small_scratch, s, frame0);
}

// pixel_type 0: float32 frames, 1: 8-bit frames; normalize 1: the two entry points above, 0: the un-normalised crop
int launch_prepare_inputs_opt(const void* rgb, int pixel_type, int normalize, const unsigned char* mask, const double* K, const int* frame_map,
                              int N, int H, int W, int S, int P, unsigned seed, float* img, int* choose, float* pts2d, double* Kcrop,
                              int* window, int* valid, unsigned char* small_scratch, hipStream_t s, int frame0) {
  RGBM_REQUIRE((pixel_type == 0 || pixel_type == 1) && (normalize == 0 || normalize == 1), "prepare_inputs_opt: pixel_type and normalize are 0 or 1");
  const float* f32 = static_cast<const float*>(rgb);
  const unsigned char* u8 = static_cast<const unsigned char*>(rgb);
  if (normalize)
    return pixel_type ? launch_prepare_inputs_u8(u8, mask, K, frame_map, N, H, W, S, P, seed, img, choose, pts2d, Kcrop, window, valid, small_scratch, s, frame0)
                      : launch_prepare_inputs(f32, mask, K, frame_map, N, H, W, S, P, seed, img, choose, pts2d, Kcrop, window, valid, small_scratch, s, frame0);
  return pixel_type ? prepare_inputs_impl<unsigned char, false>(u8, mask, K, frame_map, N, H, W, S, P, seed, img, choose, pts2d, Kcrop, window, valid, small_scratch, s, frame0)
                    : prepare_inputs_impl<float, false>(f32, mask, K, frame_map, N, H, W, S, P, seed, img, choose, pts2d, Kcrop, window, valid, small_scratch, s, frame0);
}

// launch_prepare_inputs_opt with the points drawn at native resolution (sample_mode 1: choose_native_kernel)
int launch_prepare_inputs_native(const void* rgb, int pixel_type, int normalize, const unsigned char* mask, const double* K, const int* frame_map,
                                 int N, int H, int W, int S, int P, unsigned seed, float* img, int* choose, float* pts2d, double* Kcrop,
                                 int* window, int* valid, unsigned char* small_scratch, hipStream_t s, int frame0) {
  RGBM_REQUIRE((pixel_type == 0 || pixel_type == 1) && (normalize == 0 || normalize == 1), "prepare_inputs_native: pixel_type and normalize are 0 or 1");
  const float* f32 = static_cast<const float*>(rgb);
  const unsigned char* u8 = static_cast<const unsigned char*>(rgb);
  if (normalize)
    return pixel_type ? prepare_inputs_impl<unsigned char, true>(u8, mask, K, frame_map, N, H, W, S, P, seed, img, choose, pts2d, Kcrop, window, valid, small_scratch, s, frame0, 1)
                      : prepare_inputs_impl<float, true>(f32, mask, K, frame_map, N, H, W, S, P, seed, img, choose, pts2d, Kcrop, window, valid, small_scratch, s, frame0, 1);
  return pixel_type ? prepare_inputs_impl<unsigned char, false>(u8, mask, K, frame_map, N, H, W, S, P, seed, img, choose, pts2d, Kcrop, window, valid, small_scratch, s, frame0, 1)
                    : prepare_inputs_impl<float, false>(f32, mask, K, frame_map, N, H, W, S, P, seed, img, choose, pts2d, Kcrop, window, valid, small_scratch, s, frame0, 1);
}

namespace {
template <typename Px, bool NORM>
void launch_crop_windows(const void* pix, const unsigned char* mask_pix, const long long* offset, const int* window, int N, int S, float* img,
                         unsigned char* small, hipStream_t s) {
  const long long tot = (long long)N * S * S;
  hipLaunchKernelGGL((crop_resize_windows_kernel<Px, NORM>), dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, static_cast<const Px*>(pix),
                     mask_pix, offset, window, N, S, img, small);
}
}  // namespace

// prepare_inputs_opt from packed crop windows (include/rgbm.h: rgbm_prepare_inputs_windows)
int launch_prepare_inputs_windows(const void* pix, int pixel_type, int normalize, const unsigned char* mask_pix, const long long* offset,
                                  const int* window, const int* valid_in, const double* K, int frame0, int N, int H, int W, int S, int P,
                                  unsigned seed, float* img, int* choose, float* pts2d, double* Kcrop, int* valid, unsigned char* small_scratch,
                                  hipStream_t s) {
  RGBM_REQUIRE((pixel_type == 0 || pixel_type == 1) && (normalize == 0 || normalize == 1), "prepare_inputs_windows: pixel_type and normalize are 0 or 1");
  RGBM_REQUIRE(pix && mask_pix && offset && window && valid_in && K && img && choose && Kcrop && valid && small_scratch,
               "prepare_inputs_windows arguments");
  RGBM_REQUIRE(frame0 >= 0 && N > 0 && H >= 440 && W >= 440 && S > 0 && P > 0 && S * S <= 65536,
               "prepare_inputs_windows sizes (the windows' frames must be at least 440 x 440)");
  if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(choose_kernel), 150 * 1024)) return rc;
  hipLaunchKernelGGL(window_intrinsics_kernel, dim3((N + 127) / 128), dim3(128), 0, s, window, valid_in, K, N, S, Kcrop, valid);
  if (normalize) {
    if (pixel_type) launch_crop_windows<unsigned char, true>(pix, mask_pix, offset, window, N, S, img, small_scratch, s);
    else launch_crop_windows<float, true>(pix, mask_pix, offset, window, N, S, img, small_scratch, s);
  } else {
    if (pixel_type) launch_crop_windows<unsigned char, false>(pix, mask_pix, offset, window, N, S, img, small_scratch, s);
    else launch_crop_windows<float, false>(pix, mask_pix, offset, window, N, S, img, small_scratch, s);
  }
  hipLaunchKernelGGL(choose_kernel, dim3(N), dim3(PRE_THREADS), (size_t)S * S * sizeof(unsigned short), s, small_scratch, window, S, P, seed, choose,
                     pts2d, valid, frame0);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

// The chosen points' pixel coordinates as the real-world network reads them (interface_realworld.py:264-269): x / W, y / H.  A true
// IEEE float32 division: 640 and 480 are no powers of two, so a multiply by the reciprocal rounds differently.
__global__ void pts2d_to_coor_kernel(const float* __restrict__ pts2d, float* __restrict__ coor, long long n, float W, float H) {
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float2 p = *reinterpret_cast<const float2*>(pts2d + 2 * i);
  *reinterpret_cast<float2*>(coor + 2 * i) = make_float2(__fdiv_rn(p.x, W), __fdiv_rn(p.y, H));
}

int launch_pts2d_to_coor(const float* pts2d, float* coor, long long n, int W, int H, hipStream_t s) {
  RGBM_REQUIRE(pts2d && coor && n > 0 && W > 0 && H > 0, "pts2d_to_coor arguments");
  RGBM_REQUIRE((n + 255) / 256 < (1ll << 31), "pts2d_to_coor grid out of range");
  hipLaunchKernelGGL(pts2d_to_coor_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, pts2d, coor, n, (float)W, (float)H);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_quantize_frames(const float* src, unsigned char* dst, size_t n, hipStream_t s) {
  RGBM_REQUIRE(src && dst && n > 0, "quantize_frames arguments");
  RGBM_REQUIRE(reinterpret_cast<uintptr_t>(src) % 4 == 0, "quantize_frames: src must be 4-byte aligned");
  const unsigned head = (unsigned)std::min<size_t>(n, (4 - reinterpret_cast<uintptr_t>(dst) % 4) % 4);
  const size_t quads = (n - head) / 4;
  // a memory-bound stream: at most 8 blocks per CU's worth of blocks, the rest of the quads by grid stride
  const unsigned blocks = (unsigned)std::min<size_t>(2048, std::max<size_t>(1, (quads + 255) / 256));
  hipLaunchKernelGGL(quantize_frames_kernel, dim3(blocks), dim3(256), 0, s, src, dst, n, head, quads);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace rgbm
