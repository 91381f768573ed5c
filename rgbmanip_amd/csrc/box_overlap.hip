// Agreement of two oriented boxes (gfx950): exact intersection volume and IoU of two parallelepipeds, and the centre, corner, extent
// and rotation errors between them.  float64 numpy twins: rgbmanip_amd/boxes.py (box_agreement_ref,
// box_iou_matrix_ref), which evaluate the same expressions in the same order.
//
// The box model.  A box is [8][3] corners in get_3d_bbox's order (bbox_emit.h: bbox_sign), read as the parallelepiped
// o + a ex + b ey + c ez, 0 <= a, b, c <= 1, with o = corner 0 and ex, ey, ez the edges to corners 2, 4 and 1 (the edges
// sample_stats.hip uses).  The other four corners enter the finiteness check, the centre (mean of the 8) and corner_dist only.
// volume = |det[ex ey ez]|; a box is unusable when a coordinate is not finite, its volume is not > 0 or its ok byte is 0.
// Range: the face normals are normalised through |u x v|^2, a product of four edge lengths, so edge lengths (and the coordinates that
// carry them) are meant to lie within 1e-60 .. 1e60; boxes are metres.  Outside that range products overflow or vanish and the results
// are not defined (no fault: every index comes from counts bounded by 10).
//
// derive_box makes a 27-double record of a box: centre, corner 0 relative to the centre, the three edges, the three unit normals
// of the faces a = 1, b = 1, c = 1 (pointing out of the box, also for a mirrored corner order), volume, the length of ex + ey + ez,
// and usability.
//
// The intersection volume of a pair is 1/3 sum_f d_f area(P_f) over the 12 faces of both boxes (divergence theorem), in coordinates
// relative to the centre of box A: the plane of face f is n_f . x <= d_f with the unit outward normal, and P_f is the face's quad
// clipped (Sutherland-Hodgman, closed half-spaces) by the other box's planes.  One lane per face, 12 lanes per pair, 5 pairs per
// wavefront (lanes 60..63 idle).  The two ping-pong polygons of a lane live in LDS as [buffer][vertex][coordinate][lane]: the lanes
// of one access are 8 bytes apart (no bank conflict), and the vertex index, which only the data knows, indexes LDS and never a
// per-thread array (that would be scratch memory).  A quad clipped by 6 planes has at most 10 vertices; the writes are bounded by
// that all the same.  The 12 face terms go through LDS and one lane adds them in face order (A's 0..5, then B's): no atomics and no
// order that depends on which lane finishes first.
//
// Faces are clipped independently of each other, so planes that coincide need a rule (without it identical boxes count their shared
// faces twice, and boxes that touch on a face count a face that bounds nothing).  With tau = 1e-12 and L the longer of the two
// lengths |ex + ey + ez|: a plane of B with n_A . n_B >= 1 - tau and |d_A - d_B| <= tau L against some plane of A is dropped (its
// face is not counted and A's faces are not clipped by it); a plane of B with n_A . n_B <= -(1 - tau) and |d_A + d_B| <= tau L makes
// the intersection volume 0.  inter = clamp(sum / 3, 0, min(vol_a, vol_b)), iou = inter / (vol_a + vol_b - inter).
//
// box_agreement_kernel: a workgroup (one wavefront) takes 5 pairs per pass; the corners are staged in LDS, 10 lanes derive the 10
// records, the 60 face lanes clip, then lanes 0..7 of each pair write one group of metrics each.
// box_iou_matrix_kernel: a workgroup takes up to 8 rows of one pose's [P][Q] matrix: it derives the records of its rows' boxes and
// of the pose's Q boxes once, then walks its rows * Q pairs 5 at a time.
// Built with -ffp-contract=off: the twins round every product and sum.
#include "box_overlap.h"

#pragma clang fp contract(off)

namespace rgbm {

namespace {

constexpr int BO_LANES = 64;
constexpr int BO_PAIRS = 5;       // pairs per pass of a wavefront
constexpr int BO_FACES = 12;      // face lanes per pair: A's faces 0..5, then B's
constexpr int BO_MAXV = 10;       // vertices of a quad clipped by 6 planes
constexpr int BO_ROWS = 8;        // rows of the IoU matrix per workgroup
constexpr unsigned BO_MAX_GRID = 8192;      // workgroups per launch (32 per CU); more work than that is walked with a grid stride
constexpr double BO_TAU = 1e-12;
constexpr double BO_DEG = 180.0 / 3.14159265358979323846;

// the record of a box (doubles)
enum { R_C = 0, R_O = 3, R_E = 6, R_N = 15, R_VOL = 24, R_DIAG = 25, R_OK = 26, R_SIZE = 27 };

struct PairLds {
  double poly[2][BO_MAXV][3][BO_LANES];
  double plane[BO_PAIRS][BO_FACES][4];      // n, d of every face, relative to the centre of A
  double part[BO_PAIRS][BO_FACES];          // d_f area(P_f)
  unsigned char drop[BO_PAIRS][6];          // B's plane coincides with one of A's
  unsigned char opposed[BO_PAIRS][6];       // B's plane lies on one of A's, facing it
};

__device__ __forceinline__ void derive_box(const double* __restrict__ c /*[8][3]*/, bool ok, double* rec) {
  bool fin = true;
#pragma unroll
  for (int k = 0; k < 24; ++k) fin = fin && isfinite(c[k]);
  double e[3][3];
  const int far[3] = {2, 4, 1};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    double a = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) a += c[k * 3 + i];
    const double ctr = a / 8.0;
    rec[R_C + i] = ctr;
    rec[R_O + i] = c[i] - ctr;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      e[d][i] = c[far[d] * 3 + i] - c[i];
      rec[R_E + d * 3 + i] = e[d][i];
    }
  }
  double nn[3][3];      // ey x ez, ez x ex, ex x ey
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const double* u = e[(d + 1) % 3];
    const double* v = e[(d + 2) % 3];
    nn[d][0] = u[1] * v[2] - u[2] * v[1];
    nn[d][1] = u[2] * v[0] - u[0] * v[2];
    nn[d][2] = u[0] * v[1] - u[1] * v[0];
  }
  const double det = e[0][0] * nn[0][0] + e[0][1] * nn[0][1] + e[0][2] * nn[0][2];
  const double vol = fabs(det);
  const double sg = det < 0.0 ? -1.0 : 1.0;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const double l = sqrt(nn[d][0] * nn[d][0] + nn[d][1] * nn[d][1] + nn[d][2] * nn[d][2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) rec[R_N + d * 3 + i] = sg * nn[d][i] / l;
  }
  const double g0 = e[0][0] + e[1][0] + e[2][0], g1 = e[0][1] + e[1][1] + e[2][1], g2 = e[0][2] + e[1][2] + e[2][2];
  rec[R_VOL] = vol;
  rec[R_DIAG] = sqrt(g0 * g0 + g1 * g1 + g2 * g2);
  rec[R_OK] = ok && fin && vol > 0.0 ? 1.0 : 0.0;
}

// The face terms of up to 5 pairs: lane 12 p + f clips face f of pair p (records ra, rb) and leaves d_f area(P_f) in L.part[p][f];
// the B lanes leave their coincidence flags in L.drop / L.opposed.  Every lane of the wavefront calls it (it holds barriers); a lane
// that is not `active` (lanes 60..63, a pair past the end, an unusable box) touches nothing.
__device__ __forceinline__ void pair_faces(PairLds& L, const double* ra, const double* rb, bool active, int lane) {
  const int p = lane / BO_FACES, f = lane - p * BO_FACES;
  const int side = f / 6, fi = f - side * 6, ax = fi >> 1, hi = fi & 1;
  double N0 = 0.0, N1 = 0.0, N2 = 0.0, D = 0.0;
  int cnt = 0;
  if (active) {
    const double* own = side ? rb : ra;
    double b0 = own[R_O + 0], b1 = own[R_O + 1], b2 = own[R_O + 2];
    if (side) {      // B's faces in A's frame
      b0 = b0 + (rb[R_C + 0] - ra[R_C + 0]);
      b1 = b1 + (rb[R_C + 1] - ra[R_C + 1]);
      b2 = b2 + (rb[R_C + 2] - ra[R_C + 2]);
    }
    const double* e = own + R_E + ax * 3;
    if (hi) { b0 = b0 + e[0]; b1 = b1 + e[1]; b2 = b2 + e[2]; }
    const double* nr = own + R_N + ax * 3;
    N0 = hi ? nr[0] : -nr[0];
    N1 = hi ? nr[1] : -nr[1];
    N2 = hi ? nr[2] : -nr[2];
    D = N0 * b0 + N1 * b1 + N2 * b2;
    double* pl = L.plane[p][f];
    pl[0] = N0; pl[1] = N1; pl[2] = N2; pl[3] = D;
    const double* u = own + R_E + ((ax + 1) % 3) * 3;
    const double* v = own + R_E + ((ax + 2) % 3) * 3;
    const double c0 = b0 + u[0], c1 = b1 + u[1], c2 = b2 + u[2];
    L.poly[0][0][0][lane] = b0; L.poly[0][0][1][lane] = b1; L.poly[0][0][2][lane] = b2;
    L.poly[0][1][0][lane] = c0; L.poly[0][1][1][lane] = c1; L.poly[0][1][2][lane] = c2;
    L.poly[0][2][0][lane] = c0 + v[0]; L.poly[0][2][1][lane] = c1 + v[1]; L.poly[0][2][2][lane] = c2 + v[2];
    L.poly[0][3][0][lane] = b0 + v[0]; L.poly[0][3][1][lane] = b1 + v[1]; L.poly[0][3][2][lane] = b2 + v[2];
    cnt = 4;
  }
  __syncthreads();
  if (active && side == 1) {
    const double tol = BO_TAU * fmax(ra[R_DIAG], rb[R_DIAG]);
    bool drop = false, opp = false;
    for (int i = 0; i < 6; ++i) {
      const double* q = L.plane[p][i];
      const double dot = q[0] * N0 + q[1] * N1 + q[2] * N2;
      if (dot >= 1.0 - BO_TAU && fabs(q[3] - D) <= tol) drop = true;
      if (dot <= -(1.0 - BO_TAU) && fabs(q[3] + D) <= tol) opp = true;
    }
    L.drop[p][fi] = drop ? 1 : 0;
    L.opposed[p][fi] = opp ? 1 : 0;
  }
  __syncthreads();
  if (active) {
    if (side == 1 && L.drop[p][fi]) cnt = 0;
    int cur = 0;
    for (int j = 0; j < 6 && cnt > 0; ++j) {
      if (side == 0 && L.drop[p][j]) continue;
      const double* q = L.plane[p][(1 - side) * 6 + j];
      const double q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
      const int nxt = cur ^ 1;
      double P0 = L.poly[cur][0][0][lane], P1 = L.poly[cur][0][1][lane], P2 = L.poly[cur][0][2][lane];
      double sP = (q0 * P0 + q1 * P1 + q2 * P2) - q3;
      int m = 0;
      for (int i = 0; i < cnt; ++i) {
        const int k = i + 1 == cnt ? 0 : i + 1;
        const double Q0 = L.poly[cur][k][0][lane], Q1 = L.poly[cur][k][1][lane], Q2 = L.poly[cur][k][2][lane];
        const double sQ = (q0 * Q0 + q1 * Q1 + q2 * Q2) - q3;
        const bool inP = sP <= 0.0, inQ = sQ <= 0.0;
        if (inP && m < BO_MAXV) {
          L.poly[nxt][m][0][lane] = P0; L.poly[nxt][m][1][lane] = P1; L.poly[nxt][m][2][lane] = P2;
          ++m;
        }
        if (inP != inQ && m < BO_MAXV) {
          const double t = sP / (sP - sQ);
          L.poly[nxt][m][0][lane] = P0 + t * (Q0 - P0);
          L.poly[nxt][m][1][lane] = P1 + t * (Q1 - P1);
          L.poly[nxt][m][2][lane] = P2 + t * (Q2 - P2);
          ++m;
        }
        P0 = Q0; P1 = Q1; P2 = Q2; sP = sQ;
      }
      cnt = m;
      cur = nxt;
    }
    double area = 0.0;
    if (cnt >= 3) {      // fan from vertex 0
      const double V0 = L.poly[cur][0][0][lane], V1 = L.poly[cur][0][1][lane], V2 = L.poly[cur][0][2][lane];
      double s0 = 0.0, s1 = 0.0, s2 = 0.0;
      double a0 = L.poly[cur][1][0][lane] - V0, a1 = L.poly[cur][1][1][lane] - V1, a2 = L.poly[cur][1][2][lane] - V2;
      for (int i = 2; i < cnt; ++i) {
        const double c0 = L.poly[cur][i][0][lane] - V0, c1 = L.poly[cur][i][1][lane] - V1, c2 = L.poly[cur][i][2][lane] - V2;
        s0 += a1 * c2 - a2 * c1;
        s1 += a2 * c0 - a0 * c2;
        s2 += a0 * c1 - a1 * c0;
        a0 = c0; a1 = c1; a2 = c2;
      }
      area = 0.5 * fabs(N0 * s0 + N1 * s1 + N2 * s2);
    }
    L.part[p][f] = D * area;
  }
  __syncthreads();
}

// after pair_faces: the intersection volume of pair p from its 12 face terms, in face order
__device__ __forceinline__ double pair_inter(const PairLds& L, int p, double va, double vb) {
  double s = 0.0;
  for (int f = 0; f < BO_FACES; ++f) s += L.part[p][f];
  s = s / 3.0;
  bool opp = false;
  for (int j = 0; j < 6; ++j) opp = opp || L.opposed[p][j] != 0;
  const double lim = fmin(va, vb);
  return opp ? 0.0 : s < 0.0 ? 0.0 : s > lim ? lim : s;
}

__device__ __forceinline__ double edge_length(const double* r, int e) {
  const double* v = r + R_E + e * 3;
  return sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
}

// u_a[e] . u_b[e], the unit edge vectors
__device__ __forceinline__ double unit_dot(const double* ra, const double* rb, int e) {
  const double la = edge_length(ra, e), lb = edge_length(rb, e);
  const double* v = ra + R_E + e * 3;
  const double* w = rb + R_E + e * 3;
  return (v[0] / la) * (w[0] / lb) + (v[1] / la) * (w[1] / lb) + (v[2] / la) * (w[2] / lb);
}

__device__ __forceinline__ double acos_deg(double c) {
  c = c > 1.0 ? 1.0 : c < -1.0 ? -1.0 : c;
  return acos(c) * BO_DEG;
}

__global__ __launch_bounds__(BO_LANES) void box_agreement_kernel(const double* __restrict__ a, const double* __restrict__ b,
                                                                 const unsigned char* __restrict__ ok_a,
                                                                 const unsigned char* __restrict__ ok_b, long long n,
                                                                 const BoxAgreementOut o) {
  __shared__ PairLds L;
  __shared__ double corner[BO_PAIRS][2][24];
  __shared__ double rec[BO_PAIRS][2][R_SIZE];
  const int lane = threadIdx.x;
  const long long groups = (n + BO_PAIRS - 1) / BO_PAIRS;
  const double nan = __builtin_nan("");
  for (long long g = blockIdx.x; g < groups; g += gridDim.x) {
    const long long first = g * BO_PAIRS;
    for (int i = lane; i < BO_PAIRS * 48; i += BO_LANES) {
      const int p = i / 48, r = i - p * 48, sd = r / 24, k = r - sd * 24;
      if (first + p < n) corner[p][sd][k] = (sd ? b : a)[(first + p) * 24 + k];
    }
    __syncthreads();
    if (lane < 2 * BO_PAIRS && first + (lane >> 1) < n) {
      const int p = lane >> 1, sd = lane & 1;
      const unsigned char* okp = sd ? ok_b : ok_a;
      derive_box(corner[p][sd], okp ? okp[first + p] != 0 : true, rec[p][sd]);
    }
    __syncthreads();
    const int p = lane / BO_FACES, f = lane - p * BO_FACES;
    const long long pair = first + p;
    const bool inrange = lane < BO_PAIRS * BO_FACES && pair < n;
    const double* ra = inrange ? rec[p][0] : nullptr;
    const double* rb = inrange ? rec[p][1] : nullptr;
    const bool usable = inrange && ra[R_OK] != 0.0 && rb[R_OK] != 0.0;
    pair_faces(L, ra, rb, usable, lane);
    if (inrange) {
      if (f == 0) {
        double inter = nan, iou = nan;
        if (usable) {
          inter = pair_inter(L, p, ra[R_VOL], rb[R_VOL]);
          iou = inter / ((ra[R_VOL] + rb[R_VOL]) - inter);
        }
        o.valid[pair] = usable ? 1 : 0;
        o.inter_volume[pair] = inter;
        o.iou[pair] = iou;
      } else if (f == 1) {
        const double d0 = rb[R_C + 0] - ra[R_C + 0], d1 = rb[R_C + 1] - ra[R_C + 1], d2 = rb[R_C + 2] - ra[R_C + 2];
        o.volume_a[pair] = usable ? ra[R_VOL] : nan;
        o.volume_b[pair] = usable ? rb[R_VOL] : nan;
        o.center_delta[pair * 3 + 0] = usable ? d0 : nan;
        o.center_delta[pair * 3 + 1] = usable ? d1 : nan;
        o.center_delta[pair * 3 + 2] = usable ? d2 : nan;
        o.center_dist[pair] = usable ? sqrt(d0 * d0 + d1 * d1 + d2 * d2) : nan;
      } else if (f == 2) {
        double s = 0.0;
        for (int k = 0; k < 8; ++k) {
          const double d0 = corner[p][0][k * 3 + 0] - corner[p][1][k * 3 + 0], d1 = corner[p][0][k * 3 + 1] - corner[p][1][k * 3 + 1],
                       d2 = corner[p][0][k * 3 + 2] - corner[p][1][k * 3 + 2];
          s += sqrt(d0 * d0 + d1 * d1 + d2 * d2);
        }
        o.corner_dist[pair] = usable ? s / 8.0 : nan;
      } else if (f == 3) {
        for (int e = 0; e < 3; ++e) {
          o.extent_a[pair * 3 + e] = usable ? edge_length(ra, e) : nan;
          o.extent_b[pair * 3 + e] = usable ? edge_length(rb, e) : nan;
        }
      } else if (f < 7) {
        const int e = f - 4;
        const double th = usable ? acos_deg(unit_dot(ra, rb, e)) : nan;
        o.axis_angle_deg[pair * 3 + e] = th;
        o.axis_fold_deg[pair * 3 + e] = fmin(th, 180.0 - th);      // NaN stays NaN
      } else if (f == 7) {
        double r = nan;
        if (usable) r = acos_deg((((unit_dot(ra, rb, 0) + unit_dot(ra, rb, 1)) + unit_dot(ra, rb, 2)) - 1.0) / 2.0);
        o.rot_deg[pair] = r;
      }
    }
    __syncthreads();      // the next pass overwrites corner, rec and L
  }
}

__global__ __launch_bounds__(BO_LANES) void box_iou_matrix_kernel(const double* __restrict__ a, const double* __restrict__ b,
                                                                  const unsigned char* __restrict__ ok_a,
                                                                  const unsigned char* __restrict__ ok_b, long long n, int P, int Q,
                                                                  double* __restrict__ iou) {
  __shared__ PairLds L;
  __shared__ double rec[BO_ROWS + kBoxMatrixMax][R_SIZE];      // the workgroup's rows of A, then the pose's boxes of B
  const int lane = threadIdx.x;
  const int tiles = (P + BO_ROWS - 1) / BO_ROWS;
  const long long works = n * tiles;
  const double nan = __builtin_nan("");
  for (long long w = blockIdx.x; w < works; w += gridDim.x) {
    const long long pose = w / tiles;
    const int row0 = (int)(w - pose * tiles) * BO_ROWS;
    const int rows = P - row0 < BO_ROWS ? P - row0 : BO_ROWS;
    for (int i = lane; i < rows + Q; i += BO_LANES) {
      if (i < rows) {
        const long long box = pose * P + row0 + i;
        derive_box(a + box * 24, ok_a ? ok_a[box] != 0 : true, rec[i]);
      } else {
        const long long box = pose * Q + (i - rows);
        derive_box(b + box * 24, ok_b ? ok_b[box] != 0 : true, rec[BO_ROWS + (i - rows)]);
      }
    }
    __syncthreads();
    const int pairs = rows * Q;
    const int p = lane / BO_FACES, f = lane - p * BO_FACES;
    for (int base = 0; base < pairs; base += BO_PAIRS) {
      const int idx = base + p;
      const bool inrange = lane < BO_PAIRS * BO_FACES && idx < pairs;
      const int r = inrange ? idx / Q : 0, c = inrange ? idx - r * Q : 0;
      const double* ra = rec[r];
      const double* rb = rec[BO_ROWS + c];
      const bool usable = inrange && ra[R_OK] != 0.0 && rb[R_OK] != 0.0;
      pair_faces(L, ra, rb, usable, lane);
      if (inrange && f == 0) {
        double v = nan;
        if (usable) {
          const double inter = pair_inter(L, p, ra[R_VOL], rb[R_VOL]);
          v = inter / ((ra[R_VOL] + rb[R_VOL]) - inter);
        }
        iou[((pose * P + row0 + r) * Q) + c] = v;
      }
      __syncthreads();      // the next pass overwrites L
    }
  }
}

unsigned capped_grid(long long blocks) { return (unsigned)(blocks < (long long)BO_MAX_GRID ? blocks : (long long)BO_MAX_GRID); }

}  // namespace

int launch_box_agreement(const double* a, const double* b, const unsigned char* ok_a, const unsigned char* ok_b, int n,
                         const BoxAgreementOut& o, hipStream_t s) {
  RGBM_REQUIRE(a && b && o.valid && o.iou && o.inter_volume && o.volume_a && o.volume_b && o.center_dist && o.center_delta &&
               o.corner_dist && o.extent_a && o.extent_b && o.axis_angle_deg && o.axis_fold_deg && o.rot_deg, "box_agreement arguments");
  RGBM_REQUIRE(n >= 1 && n <= kBoxPairsMax, "box_agreement: 1 <= n <= 2^24 pairs");
  const long long groups = ((long long)n + BO_PAIRS - 1) / BO_PAIRS;
  hipLaunchKernelGGL(box_agreement_kernel, dim3(capped_grid(groups)), dim3(BO_LANES), 0, s, a, b, ok_a, ok_b, (long long)n, o);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_box_iou_matrix(const double* a, const double* b, const unsigned char* ok_a, const unsigned char* ok_b, int n, int P, int Q,
                          double* iou, hipStream_t s) {
  RGBM_REQUIRE(a && b && iou, "box_iou_matrix arguments");
  RGBM_REQUIRE(P >= 1 && P <= kBoxMatrixMax && Q >= 1 && Q <= kBoxMatrixMax, "box_iou_matrix: 1 <= P, Q <= 64 boxes per pose");
  RGBM_REQUIRE(n >= 1 && (long long)n * P * Q <= 2147483647ll, "box_iou_matrix: n >= 1 and n * P * Q <= 2^31 - 1 pairs");
  const long long works = (long long)n * ((P + BO_ROWS - 1) / BO_ROWS);
  hipLaunchKernelGGL(box_iou_matrix_kernel, dim3(capped_grid(works)), dim3(BO_LANES), 0, s, a, b, ok_a, ok_b, (long long)n, P, Q, iou);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace rgbm
