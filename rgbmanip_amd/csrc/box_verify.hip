// Box verification without ground truth (gfx950): the silhouette of S boxes against the V masks of a pose, and the share of a packed
// cloud a box contains.  float64 numpy twins: rgbmanip_amd/verify.py (box_silhouette_ref, cloud_in_box_ref),
// which evaluate the same expressions in the same order; every output here is an integer, so kernel and twin are EQUAL.
//
// The box model is the one of box_overlap.hip: [8][3] corners read as o + a e0 + b e1 + c e2, 0 <= a, b, c <= 1, o = corner 0 and
// e0, e1, e2 the edges to corners 2, 4, 1.  In a frame (a camera's, or the world) the model's record is n_k = e_{k+1} x e_{k+2},
// det = e0 . n0, lo = min(0, det), hi = max(0, det): a point x is inside iff lo <= n_k . (x - o) <= hi for k = 0, 1, 2.
//
// Silhouette.  Camera-frame corners c = ((E_r0 x + E_r1 y) + E_r2 z) + E_r3.  Pixel (v, u) has the viewing ray t (xn, yn, 1),
// xn = (u - K02) / K00, yn = (v - K12) / K11 (integer pixel coordinates, as synth_shade_px).  Slab k: q0 = -(n_k . o),
// dq = (n_k.x xn + n_k.y yn) + n_k.z; dq != 0: tn / tf = min / max of (lo - q0) / dq, (hi - q0) / dq; dq == 0: tn = -inf inside the
// slab and +inf outside, tf = +inf.  The pixel is in the silhouette iff min_k tf >= max_k tn and max_k tn > 0, the renderer's rule.
//
// box_verify_setup_kernel, one thread per (pose, box, view): the 14-double record, the flags, a conservative pixel bound, and the
// initial value of every output of that (pose, box, view).  The bound: the silhouette is the set of pixels whose ray meets the
// parallelepiped at t > 0, that is at a point of positive depth; when all 8 corners of the model (o + a e0 + b e1 + c e2, not the
// four corners the model never reads) have z > 0 that point is a convex combination of them and its projection lies in the bounding
// rectangle of the projected corners.  That rectangle, widened by one pixel against the rounding of the slab arithmetic and clipped to
// the frame, is the bound; with a corner at z <= 0, a projection that is not finite, or a box so flat that its normals are mostly
// rounding (det^2 < 1e-18 |e0|^2 |e1|^2 |e2|^2), it is the whole frame.  The twin tests every
// pixel of the frame, so a bound that cuts a silhouette pixel off is a count mismatch in tests/test_gpu_verify.py.
//
// box_silhouette_kernel<WIDE>: a workgroup of 256 threads owns 1024 consecutive pixels (1.6 rows of a 640-wide frame) of one (pose,
// view); it stages that pair's S records and bounds in LDS, every thread keeps xn, yn and the mask bits of its 4 pixels in registers
// (WIDE: H W % 4 == 0 and a 4-byte aligned mask, one 32-bit load; otherwise 4 byte loads), and the boxes whose bound meets the tile's
// rows are walked with the mask read once.  Counts: ballot + popcount per wavefront, one LDS integer add per wavefront and box; extents:
// LDS integer min / max; then one set of global integer atomics per workgroup and box that saw a hit.  Integer sums, minima and maxima
// do not depend on the order of arrival: two calls give the same bytes.  The mask count of a tile is taken once, boxes or not.
//
// cloud_in_box_kernel: a workgroup takes 1024 rows of one pose's cloud; S lanes derive the world-frame records into LDS, every thread
// keeps 4 rows in registers and walks the S boxes; ballot + popcount, LDS adds, one global add per workgroup and box.
// Built with -ffp-contract=off: the twins round every product and sum.
#include "box_verify.h"

#pragma clang fp contract(off)

namespace rgbm {

namespace {

constexpr int BV_THREADS = 256;
constexpr int BV_PX = 4;                                  // pixels (cloud rows) per thread
constexpr int BV_TILE = BV_THREADS * BV_PX;               // per workgroup
constexpr unsigned BV_MAX_GRID = 8192;                    // workgroups per launch (32 per CU); more tiles than that are walked with a grid stride
constexpr int BV_REC = 14;                                // n[3][3], q0[3], lo, hi
enum { V_N = 0, V_Q = 9, V_LO = 12, V_HI = 13 };
enum { F_USABLE = 1, F_CAMERA_INSIDE = 2, F_BORDER = 4, F_BEHIND = 8 };

// the model of a box in the frame its four corners o, p2, p4, p1 are given in: edges, normals n_k = e_{k+1} x e_{k+2}, det = e0 . n0
__device__ __forceinline__ double derive_model(const double o[3], const double p2[3], const double p4[3], const double p1[3], double e[3][3],
                                               double nn[3][3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) { e[0][i] = p2[i] - o[i]; e[1][i] = p4[i] - o[i]; e[2][i] = p1[i] - o[i]; }
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const double* u = e[(d + 1) % 3];
    const double* v = e[(d + 2) % 3];
    nn[d][0] = u[1] * v[2] - u[2] * v[1];
    nn[d][1] = u[2] * v[0] - u[0] * v[2];
    nn[d][2] = u[0] * v[1] - u[1] * v[0];
  }
  return (e[0][0] * nn[0][0] + e[0][1] * nn[0][1]) + e[0][2] * nn[0][2];
}

__global__ __launch_bounds__(64) void box_verify_setup_kernel(const double* __restrict__ boxes, const unsigned char* __restrict__ ok,
                                                              const double* __restrict__ K, const double* __restrict__ E, int n, int S, int V,
                                                              int H, int W, const BoxSilhouetteOut out, double* __restrict__ rec,
                                                              int* __restrict__ bound) {
  const int g = blockIdx.x * 64 + threadIdx.x;              // (pose * S + box) * V + view, the index of the outputs
  if (g >= n * S * V) return;
  const int v = g % V, is = g / V, s = is % S, i = is / S;
  const int pv = i * V + v;
  const double* c = boxes + (long long)is * 24;
  const double* Ev = E + (long long)pv * 16;
  const double* Kv = K + (long long)pv * 9;
  const double fx = Kv[0], cx = Kv[2], fy = Kv[4], cy = Kv[5];
  bool fin = isfinite(fx) && isfinite(fy) && isfinite(cx) && isfinite(cy) && fx != 0.0 && fy != 0.0;
#pragma unroll
  for (int k = 0; k < 12; ++k) fin = fin && isfinite(Ev[k]);
  double cam[8][3];
  bool behind = false;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const double x = c[k * 3], y = c[k * 3 + 1], z = c[k * 3 + 2];
    fin = fin && isfinite(x) && isfinite(y) && isfinite(z);
#pragma unroll
    for (int r = 0; r < 3; ++r) cam[k][r] = ((Ev[r * 4] * x + Ev[r * 4 + 1] * y) + Ev[r * 4 + 2] * z) + Ev[r * 4 + 3];
    behind = behind || cam[k][2] <= 0.0;
  }
  double e[3][3], nn[3][3];
  const double det = derive_model(cam[0], cam[2], cam[4], cam[1], e, nn);
  const double lo = det < 0.0 ? det : 0.0, hi = det > 0.0 ? det : 0.0;
  const bool usable = fin && (ok ? ok[is] != 0 : true) && fabs(det) > 0.0;
  double* r = rec + ((long long)pv * S + s) * BV_REC;
  bool inside = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double q0 = -((nn[k][0] * cam[0][0] + nn[k][1] * cam[0][1]) + nn[k][2] * cam[0][2]);
    r[V_N + k * 3] = nn[k][0]; r[V_N + k * 3 + 1] = nn[k][1]; r[V_N + k * 3 + 2] = nn[k][2];
    r[V_Q + k] = q0;
    inside = inside && lo <= q0 && q0 <= hi;
  }
  r[V_LO] = lo; r[V_HI] = hi;
  // the pixel bound (rows r0..r1, columns c0..c1, inclusive); empty: (H, W, -1, -1)
  int b0 = H, b1 = W, b2 = -1, b3 = -1;
  if (usable) {
    double u0 = INFINITY, u1 = -INFINITY, v0 = INFINITY, v1 = -INFINITY;
    bool front = true;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      double p[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        p[a] = cam[0][a];
        if (j & 1) p[a] = p[a] + e[0][a];
        if (j & 2) p[a] = p[a] + e[1][a];
        if (j & 4) p[a] = p[a] + e[2][a];
      }
      front = front && p[2] > 0.0;
      const double uu = fx * (p[0] / p[2]) + cx, vv = fy * (p[1] / p[2]) + cy;
      u0 = fmin(u0, uu); u1 = fmax(u1, uu); v0 = fmin(v0, vv); v1 = fmax(v1, vv);
      front = front && isfinite(uu) && isfinite(vv);
    }
    // a box flattened to less than 1e-9 of the volume its edge lengths span has normals that are mostly rounding: its silhouette is
    // whatever the slab arithmetic makes of them, and only the whole frame bounds that
    double len2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) len2[k] = (e[k][0] * e[k][0] + e[k][1] * e[k][1]) + e[k][2] * e[k][2];
    front = front && det * det >= 1e-18 * ((len2[0] * len2[1]) * len2[2]);
    if (front) {      // all four limits are finite; they are clamped as doubles, so the conversions below see values within the frame
      const double c0 = fmax(floor(u0) - 1.0, 0.0), c1 = fmin(ceil(u1) + 1.0, (double)(W - 1));
      const double r0 = fmax(floor(v0) - 1.0, 0.0), r1 = fmin(ceil(v1) + 1.0, (double)(H - 1));
      if (c0 <= c1 && r0 <= r1) { b0 = (int)r0; b1 = (int)c0; b2 = (int)r1; b3 = (int)c1; }
    } else {
      b0 = 0; b1 = 0; b2 = H - 1; b3 = W - 1;
    }
  }
  int* b = bound + ((long long)pv * S + s) * 4;
  b[0] = b0; b[1] = b1; b[2] = b2; b[3] = b3;
  out.area_box[g] = 0;
  out.inter[g] = 0;
  out.rect[g * 4] = H; out.rect[g * 4 + 1] = W; out.rect[g * 4 + 2] = -1; out.rect[g * 4 + 3] = -1;
  out.flags[g] = usable ? F_USABLE | (inside ? F_CAMERA_INSIDE : 0) | (behind ? F_BEHIND : 0) : 0;
  if (s == 0) out.area_mask[pv] = 0;
}

// the renderer's hit rule for the viewing ray (xn, yn, 1) against the record r (LDS)
__device__ __forceinline__ bool silhouette_hit(const double* r, double xn, double yn) {
  const double lo = r[V_LO], hi = r[V_HI];
  double tmin = -INFINITY, tmax = INFINITY;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double q0 = r[V_Q + k];
    const double dq = (r[V_N + k * 3] * xn + r[V_N + k * 3 + 1] * yn) + r[V_N + k * 3 + 2];
    double tn, tf;
    if (dq != 0.0) {
      const double t1 = (lo - q0) / dq, t2 = (hi - q0) / dq;
      tn = fmin(t1, t2); tf = fmax(t1, t2);
    } else {
      tn = lo <= q0 && q0 <= hi ? -INFINITY : INFINITY; tf = INFINITY;
    }
    if (tn > tmin) tmin = tn;
    tmax = fmin(tmax, tf);
  }
  return tmax >= tmin && tmin > 0.0;
}

template <bool WIDE>
__global__ __launch_bounds__(BV_THREADS) void box_silhouette_kernel(const double* __restrict__ K, const unsigned char* __restrict__ mask, int n,
                                                                    int S, int V, int H, int W, const double* __restrict__ rec,
                                                                    const int* __restrict__ bound, const BoxSilhouetteOut out) {
  __shared__ double s_rec[kVerifyBoxesMax * BV_REC];
  __shared__ int s_bound[kVerifyBoxesMax * 4];
  __shared__ int s_area[kVerifyBoxesMax], s_inter[kVerifyBoxesMax], s_y1[kVerifyBoxesMax], s_x1[kVerifyBoxesMax], s_y2[kVerifyBoxesMax],
      s_x2[kVerifyBoxesMax];
  __shared__ int s_mask;
  const int t = threadIdx.x, lane = t & 63;
  const long long HW = (long long)H * W;
  const long long tiles = (HW + BV_TILE - 1) / BV_TILE;
  const long long works = (long long)n * V * tiles;
  for (long long w = blockIdx.x; w < works; w += gridDim.x) {
    const int pv = (int)(w / tiles);
    const long long tile = w - (long long)pv * tiles;
    for (int k = t; k < S * BV_REC; k += BV_THREADS) s_rec[k] = rec[(long long)pv * S * BV_REC + k];
    for (int k = t; k < S * 4; k += BV_THREADS) s_bound[k] = bound[(long long)pv * S * 4 + k];
    if (t < S) { s_area[t] = 0; s_inter[t] = 0; s_y1[t] = H; s_x1[t] = W; s_y2[t] = -1; s_x2[t] = -1; }
    if (t == BV_THREADS - 1) s_mask = 0;
    __syncthreads();
    const double* Kv = K + (long long)pv * 9;
    const double fx = Kv[0], cx = Kv[2], fy = Kv[4], cy = Kv[5];
    const long long first = tile * BV_TILE, pix0 = first + (long long)t * BV_PX;
    const long long last = first + BV_TILE - 1 < HW - 1 ? first + BV_TILE - 1 : HW - 1;
    const int row_first = (int)(first / W), row_last = (int)(last / W);
    const unsigned char* frame = mask + (long long)pv * HW;
    int py[BV_PX], px[BV_PX];
    bool live[BV_PX], fg[BV_PX];
    double xn[BV_PX], yn[BV_PX];
    unsigned word = 0;
    if (WIDE && pix0 < HW) word = *reinterpret_cast<const unsigned*>(frame + pix0);      // all four pixels or none
    int nfg = 0;
#pragma unroll
    for (int j = 0; j < BV_PX; ++j) {
      const long long pix = pix0 + j;
      live[j] = pix < HW;
      py[j] = live[j] ? (int)(pix / W) : 0;
      px[j] = live[j] ? (int)(pix - (long long)py[j] * W) : 0;
      xn[j] = ((double)px[j] - cx) / fx;
      yn[j] = ((double)py[j] - cy) / fy;
      fg[j] = WIDE ? ((word >> (8 * j)) & 0xffu) != 0 : live[j] && frame[pix] != 0;
      nfg += __popcll(__ballot(fg[j]));
    }
    if (lane == 0 && nfg) atomicAdd(&s_mask, nfg);
    for (int s = 0; s < S; ++s) {
      const int r0 = s_bound[s * 4], c0 = s_bound[s * 4 + 1], r1 = s_bound[s * 4 + 2], c1 = s_bound[s * 4 + 3];
      if (r0 > row_last || r1 < row_first) continue;      // uniform over the workgroup
      const double* r = s_rec + s * BV_REC;
      int area = 0, inter = 0, y1 = H, x1 = W, y2 = -1, x2 = -1;
#pragma unroll
      for (int j = 0; j < BV_PX; ++j) {
        bool hit = false;
        if (live[j] && py[j] >= r0 && py[j] <= r1 && px[j] >= c0 && px[j] <= c1) hit = silhouette_hit(r, xn[j], yn[j]);
        if (hit) { y1 = min(y1, py[j]); y2 = max(y2, py[j]); x1 = min(x1, px[j]); x2 = max(x2, px[j]); }
        area += __popcll(__ballot(hit));
        inter += __popcll(__ballot(hit && fg[j]));
      }
      if (lane == 0 && area) { atomicAdd(&s_area[s], area); if (inter) atomicAdd(&s_inter[s], inter); }
      if (y2 >= 0) { atomicMin(&s_y1[s], y1); atomicMax(&s_y2[s], y2); atomicMin(&s_x1[s], x1); atomicMax(&s_x2[s], x2); }
    }
    __syncthreads();
    if (t < S && s_area[t]) {
      const int i = pv / V, v = pv - i * V;
      const int g = (i * S + t) * V + v;
      atomicAdd(&out.area_box[g], s_area[t]);
      if (s_inter[t]) atomicAdd(&out.inter[g], s_inter[t]);
      atomicMin(&out.rect[g * 4], s_y1[t]); atomicMin(&out.rect[g * 4 + 1], s_x1[t]);
      atomicMax(&out.rect[g * 4 + 2], s_y2[t]); atomicMax(&out.rect[g * 4 + 3], s_x2[t]);
      if (s_y1[t] == 0 || s_x1[t] == 0 || s_y2[t] == H - 1 || s_x2[t] == W - 1) atomicOr(&out.flags[g], (int)F_BORDER);
    }
    if (t == BV_THREADS - 1 && s_mask) atomicAdd(&out.area_mask[pv], s_mask);
    __syncthreads();      // the next tile overwrites the LDS
  }
}

enum { C_O = 0, C_N = 3, C_LO = 12, C_HI = 13, C_OK = 14, C_SIZE = 15 };

__global__ __launch_bounds__(BV_THREADS) void cloud_in_box_kernel(const float* __restrict__ cloud, const int* __restrict__ count, int cols,
                                                                  const double* __restrict__ boxes, const unsigned char* __restrict__ ok, int n,
                                                                  int S, int cap, double inflate, int* __restrict__ inside,
                                                                  int* __restrict__ total) {
  __shared__ double s_rec[kVerifyBoxesMax * C_SIZE];
  __shared__ int s_in[kVerifyBoxesMax];
  const int t = threadIdx.x, lane = t & 63;
  const int tiles = cap > 0 ? (cap + BV_TILE - 1) / BV_TILE : 1;
  const long long works = (long long)n * tiles;
  for (long long w = blockIdx.x; w < works; w += gridDim.x) {
    const int pose = (int)(w / tiles);
    const int tile = (int)(w - (long long)pose * tiles);
    long long sum = 0;
    for (int c = 0; c < cols; ++c) { const int k = count[(long long)pose * cols + c]; sum += k > 0 ? k : 0; }
    const int rows = (int)(sum < (long long)cap ? sum : (long long)cap);      // the rows of this pose that hold points
    if (tile == 0 && t == 0) total[pose] = rows;
    const long long row0 = (long long)tile * BV_TILE;
    if (row0 >= rows) continue;      // uniform over the workgroup
    if (t < S) {
      const long long box = (long long)pose * S + t;
      const double* c = boxes + box * 24;
      bool fin = true;
#pragma unroll
      for (int k = 0; k < 24; ++k) fin = fin && isfinite(c[k]);
      double e[3][3], nn[3][3];
      const double det = derive_model(c, c + 6, c + 12, c + 3, e, nn);
      const double m = inflate * fabs(det);
      double* r = s_rec + t * C_SIZE;
      r[C_O] = c[0]; r[C_O + 1] = c[1]; r[C_O + 2] = c[2];
#pragma unroll
      for (int k = 0; k < 9; ++k) r[C_N + k] = nn[k / 3][k % 3];
      r[C_LO] = (det < 0.0 ? det : 0.0) - m;
      r[C_HI] = (det > 0.0 ? det : 0.0) + m;
      r[C_OK] = fin && (ok ? ok[box] != 0 : true) && fabs(det) > 0.0 ? 1.0 : 0.0;
      s_in[t] = 0;
    }
    __syncthreads();
    double p[BV_PX][3];
    bool live[BV_PX];
#pragma unroll
    for (int j = 0; j < BV_PX; ++j) {
      const long long row = row0 + j * BV_THREADS + t;
      live[j] = row < rows;
      const float* q = cloud + ((long long)pose * cap + (live[j] ? row : 0)) * 3;
#pragma unroll
      for (int a = 0; a < 3; ++a) p[j][a] = live[j] ? (double)q[a] : 0.0;
      live[j] = live[j] && isfinite(p[j][0]) && isfinite(p[j][1]) && isfinite(p[j][2]);
    }
    for (int s = 0; s < S; ++s) {
      const double* r = s_rec + s * C_SIZE;
      if (r[C_OK] == 0.0) continue;      // uniform over the workgroup
      const double lo = r[C_LO], hi = r[C_HI];
      int cnt = 0;
#pragma unroll
      for (int j = 0; j < BV_PX; ++j) {
        const double d0 = p[j][0] - r[C_O], d1 = p[j][1] - r[C_O + 1], d2 = p[j][2] - r[C_O + 2];
        bool in = live[j];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double a = (r[C_N + k * 3] * d0 + r[C_N + k * 3 + 1] * d1) + r[C_N + k * 3 + 2] * d2;
          in = in && lo <= a && a <= hi;
        }
        cnt += __popcll(__ballot(in));
      }
      if (lane == 0 && cnt) atomicAdd(&s_in[s], cnt);
    }
    __syncthreads();
    if (t < S && s_in[t]) atomicAdd(&inside[(long long)pose * S + t], s_in[t]);
    __syncthreads();      // the next tile overwrites the LDS
  }
}

unsigned capped_grid(long long blocks) { return (unsigned)(blocks < (long long)BV_MAX_GRID ? blocks : (long long)BV_MAX_GRID); }

}  // namespace

size_t box_silhouette_scratch_bytes(int n, int S, int V) {
  return (size_t)n * S * V * (BV_REC * sizeof(double) + 4 * sizeof(int));
}

int launch_box_silhouette(const double* boxes, const unsigned char* ok, const double* K, const double* E, const unsigned char* mask, int n,
                          int S, int V, int H, int W, const BoxSilhouetteOut& out, void* scratch, size_t scratch_bytes, hipStream_t s) {
  RGBM_REQUIRE(boxes && K && E && mask && out.area_box && out.inter && out.area_mask && out.rect && out.flags && scratch,
               "box_silhouette arguments");
  RGBM_REQUIRE(S >= 1 && S <= kVerifyBoxesMax, "box_silhouette: 1 <= S <= 64 boxes per pose");
  RGBM_REQUIRE(V >= 1 && V <= kVerifyViewsMax, "box_silhouette: 1 <= V <= 16 views per pose");
  RGBM_REQUIRE(n >= 1 && (long long)n * S * V <= (long long)kVerifyRecordsMax, "box_silhouette: n >= 1 and n * S * V <= 2^24");
  RGBM_REQUIRE(H >= 1 && W >= 1 && (long long)H * W < (1ll << 31), "box_silhouette: H, W >= 1 and H * W < 2^31");
  RGBM_REQUIRE(reinterpret_cast<uintptr_t>(scratch) % 8 == 0, "box_silhouette: the scratch must be 8-byte aligned");
  RGBM_REQUIRE(scratch_bytes >= box_silhouette_scratch_bytes(n, S, V), "box_silhouette: scratch smaller than rgbm_box_silhouette_scratch_bytes");
  const int records = n * S * V;
  double* rec = static_cast<double*>(scratch);
  int* bound = reinterpret_cast<int*>(rec + (size_t)records * BV_REC);
  hipLaunchKernelGGL(box_verify_setup_kernel, dim3((records + 63) / 64), dim3(64), 0, s, boxes, ok, K, E, n, S, V, H, W, out, rec, bound);
  RGBM_CHECK_HIP(hipGetLastError());
  const long long HW = (long long)H * W;
  const long long works = (long long)n * V * ((HW + BV_TILE - 1) / BV_TILE);
  const bool wide = HW % 4 == 0 && reinterpret_cast<uintptr_t>(mask) % 4 == 0;
  hipLaunchKernelGGL(wide ? box_silhouette_kernel<true> : box_silhouette_kernel<false>, dim3(capped_grid(works)), dim3(BV_THREADS), 0, s, K,
                     mask, n, S, V, H, W, rec, bound, out);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_cloud_in_box(const float* cloud, const int* count, int count_cols, const double* boxes, const unsigned char* ok, int n, int S,
                        int cap, double inflate, int* inside, int* total, hipStream_t s) {
  RGBM_REQUIRE(count && boxes && inside && total, "cloud_in_box arguments");
  RGBM_REQUIRE(S >= 1 && S <= kVerifyBoxesMax, "cloud_in_box: 1 <= S <= 64 boxes per pose");
  RGBM_REQUIRE(n >= 1 && (long long)n * S <= (long long)kVerifyRecordsMax, "cloud_in_box: n >= 1 and n * S <= 2^24");
  RGBM_REQUIRE(count_cols >= 1 && count_cols <= kVerifyCountColsMax, "cloud_in_box: 1 <= columns of count <= 16");
  RGBM_REQUIRE(cap >= 0 && cap <= (1 << 30) && (cap == 0 || cloud), "cloud_in_box: 0 <= cap <= 2^30, and a cloud where cap > 0");
  RGBM_REQUIRE(inflate >= 0.0 && inflate <= 1.7e308, "cloud_in_box: inflate must be finite and >= 0");
  RGBM_CHECK_HIP(hipMemsetAsync(inside, 0, (size_t)n * S * sizeof(int), s));
  const long long works = (long long)n * (cap > 0 ? (cap + BV_TILE - 1) / BV_TILE : 1);
  hipLaunchKernelGGL(cloud_in_box_kernel, dim3(capped_grid(works)), dim3(BV_THREADS), 0, s, cloud, count, count_cols, boxes, ok, n, S, cap,
                     inflate, inside, total);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace rgbm
