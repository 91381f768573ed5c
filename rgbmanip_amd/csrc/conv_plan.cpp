#include "conv_plan.h"

#include <algorithm>
#include <functional>
#include <queue>
#include <utility>

#include "kernels.h"

namespace rgbm {

// channel tile of the generic kernel for Cout (the packed weights are padded to it)
int conv_ch_tile(int Cout) {
  if (Cout <= 16) return 16;
  if (Cout <= 32) return 32;
  if (Cout <= 64) return 64;
  return 128;
}
int conv_bk(int dtype) { return 8 * dtype_chunk(dtype); }      // 128 bytes per row

// parts to cut a small launch's K loop into: the tiles fill at most half the CUs, every part keeps at least eight K steps
#ifndef M32_KSPLIT_MAX
#define M32_KSPLIT_MAX 4
#endif
#ifndef M32_KSPLIT_MINSTEPS
#define M32_KSPLIT_MINSTEPS 8
#endif

namespace {

// every K tile inside one tap (see the UNI comment at the 2-stage kernel)
bool uniform_taps(const ConvDesc& d, int bk) {
  if (d.KD > 8 || d.KH > 8 || d.KW > 8) return false;
  if (d.lcin < 0) return d.ntaps == 1;
  return d.Cin % bk == 0;
}

// both operands addressable with 32-bit byte offsets from one buffer descriptor each (the request waves' blds16 form)
bool buffer_offsets_ok(const ConvDesc& d, int bch, long long esz) {
  const long long xbytes = ((long long)d.N * d.Di * d.Hi * d.Wi + (long long)(d.pd * d.Hi + d.ph) * d.Wi + d.pw) * d.Cin * esz;
  const long long wbytes = (long long)((d.Cout + bch - 1) / bch) * bch * d.Kpad * esz;
  return xbytes < (1ll << 32) - 65536 && wbytes < (1ll << 32) - 65536 && d.pd >= 0 && d.ph >= 0 && d.pw >= 0;
}

// row-halo variant of the 64-channel kernel: 2-D 3x3, stride 1, "same" padding, Cin a multiple of 64
bool rowhalo_ok(const ConvDesc& d) {
  return d.KD == 1 && d.KH == 3 && d.KW == 3 && d.sd == 1 && d.sh == 1 && d.sw == 1 && d.Dq == 1 && d.Di == 1 &&
         d.dilh == d.dilw && d.dilw >= 1 && d.dilw <= 4 && d.ph == d.dilh && d.pw == d.dilw && d.pd == 0 &&
         d.lcin >= 6 && d.Hq == d.Hi && d.Wq == d.Wi && d.Wi > 2 * d.dilw && d.osh == 1 && d.osw == 1;
}

// Small launches (round 6; the deployment shape: B = 1 .. 8 poses, cfg/task/open_cabinet.yaml:4 ships num_envs: 8): a layer whose tiles do not
// fill the persistent grid on the 256-pixel shapes.  Every tile walks the layer's whole K range at one K tile per (request-bound) step, so
// a launch costs  rounds x steps x (bytes requested per step)  and fewer bytes per tile win while the rounds do not grow: 128-pixel tiles of
// 64 / 128 / 256 channels (24 / 32 / 48 KB per step) against the 16x16x32 kernel's 64-channel x 256-pixel tile (40 KB).  Returns the channel
// tile to use (64 / 128 / 256), or 0 for "keep the 64 x 256 tile of conv_igemm_ws_kernel".
int m32_small_choice(const ConvDesc& d, int n_cu, bool slim_ok) {
  const long long p128 = (d.M + 127) / 128, p256 = (d.M + 255) / 256;
  auto cost = [&](long long tiles, int kb) { return (double)((tiles + n_cu - 1) / n_cu) * (double)(kb + 8); };      // + 8: the step's fixed part
  double best = slim_ok ? cost(p256 * (d.Cout / 64), 40) : 1e30;
  int pick = 0;
  const int bch[3] = {64, 128, 256}, kb[3] = {24, 32, 48};
  for (int i = 0; i < 3; ++i) {
    if (d.Cout % bch[i]) continue;
    const double c = cost(p128 * (d.Cout / bch[i]), kb[i]);
    if (c < best * 0.999) { best = c; pick = bch[i]; }
  }
  return pick;
}

int m32_ksplit_choice(const ConvDesc& d, int flags, long long tiles, int n_cu, int bch, int n_waves) {
  if ((flags & DBG_NO_KSPLIT) || tiles <= 0 || bch > 128) return 1;
  int n = (int)(n_cu / tiles);
  if (n > M32_KSPLIT_MAX) n = M32_KSPLIT_MAX;
  while (n > 1 && d.KT / n < M32_KSPLIT_MINSTEPS) --n;
  if (n < 2) return 1;
  if ((size_t)tiles * n * bch * 128 > kM32SplitFloats || (size_t)tiles * n_waves > kM32SplitCounters) return 1;
  return n;
}

// in-range taps [k0, k1) of output position q along one axis: 0 <= q - pad + k * dil < n
void tap_range(int q, int pad, int dil, int K, int n, int& k0, int& k1) {
  k0 = K; k1 = 0;
  for (int k = 0; k < K; ++k) {
    const int x = q - pad + k * dil;
    if (x >= 0 && x < n) { if (k < k0) k0 = k; k1 = k + 1; }
  }
  if (k0 > k1) k0 = k1 = 0;
}

// the classes of one axis: distinct tap ranges in order of first appearance; cls[q] = the class of position q
struct AxisClasses {
  std::vector<int> k0, k1, count, cls;
};
bool axis_classes(int nq, int pad, int dil, int K, int n, AxisClasses* a) {
  a->cls.resize(nq);
  for (int q = 0; q < nq; ++q) {
    int k0, k1;
    tap_range(q, pad, dil, K, n, k0, k1);
    if (k1 == k0) return false;                          // a position that reads padding only: a tile of it would have no K step
    for (int k = k0; k < k1; ++k) {                      // (an interval by construction; checked because the walker relies on it)
      const int x = q - pad + k * dil;
      if (x < 0 || x >= n) return false;
    }
    size_t c = 0;
    while (c < a->k0.size() && !(a->k0[c] == k0 && a->k1[c] == k1)) ++c;
    if (c == a->k0.size()) { a->k0.push_back(k0); a->k1.push_back(k1); a->count.push_back(0); }
    a->count[c] += 1;
    a->cls[q] = (int)c;
  }
  return true;
}

// the shapes the row table exists for: 2-D, stride 1, more than one tap, whole 256 x 256 interior tiles (what launch_m32's main launch takes)
bool border_shape_ok(const ConvDesc& d, int dtype) {
  return (dtype == BF16 || dtype == F16) && d.w_finite && d.KD == 1 && d.Di == 1 && d.Dq == 1 && d.pd == 0 && d.sd == 1 && d.sh == 1 && d.sw == 1 &&
         d.KH * d.KW > 1 && d.KH <= 4 && d.KW <= 4 && d.lcin >= 0 && d.Cin % conv_bk(dtype) == 0 && d.Cout % 256 == 0 && d.ph >= 0 && d.pw >= 0 &&
         d.dilh >= 1 && d.dilw >= 1 && d.N > 0 && d.M == (long long)d.N * d.Hq * d.Wq;
}

int popcount_int(int v) { int n = 0; for (; v; v &= v - 1) ++n; return n; }

}  // namespace

// rows of class (i, j) among the GEMM rows [0, main_rows): whole views, then the pixels of the last, partial view in front of its cut
static long long class_live_rows(const ConvDesc& d, const AxisClasses& ah, const AxisClasses& aw, long long main_rows, int i, int j) {
  const long long hw = (long long)d.Hq * d.Wq, whole = main_rows / hw, rem = main_rows % hw;
  const int hr = (int)(rem / d.Wq), wr = (int)(rem % d.Wq);
  long long h_below = 0, w_below = 0;
  for (int h = 0; h < hr; ++h) h_below += ah.cls[h] == i;
  for (int w = 0; w < wr; ++w) w_below += aw.cls[w] == j;
  return whole * ah.count[i] * aw.count[j] + h_below * aw.count[j] + (ah.cls[hr < d.Hq ? hr : 0] == i && hr < d.Hq ? w_below : 0);
}

bool border_applies(const ConvDesc& d, int dtype, int flags, long long main_rows) {
  if ((flags & (DBG_NO_BORDER_TILES | DBG_KORDER_TAPS_OUTER)) || !border_shape_ok(d, dtype)) return false;
  if (main_rows <= 0 || main_rows > d.M || main_rows % 256) return false;
  AxisClasses ah, aw;
  if (!axis_classes(d.Hq, d.ph, d.dilh, d.KH, d.Hi, &ah) || !axis_classes(d.Wq, d.pw, d.dilw, d.KW, d.Wi, &aw)) return false;
  long long tiles = 0, taps = 0;                         // pixel tiles, and taps summed over them
  for (size_t i = 0; i < ah.k0.size(); ++i)
    for (size_t j = 0; j < aw.k0.size(); ++j) {
      const long long t = (class_live_rows(d, ah, aw, main_rows, (int)i, (int)j) + 255) / 256;
      tiles += t;
      taps += t * (ah.k1[i] - ah.k0[i]) * (aw.k1[j] - aw.k0[j]);
    }
  // a tap saved: fewer K steps in all than the row-major tiles walk (dead rows of small classes can cost more than the classes save)
  return taps < (main_rows / 256) * (long long)d.ntaps && tiles < (1ll << 20);
}

bool plan_border(const ConvDesc& d, int dtype, int flags, long long main_rows, int n_wg, BorderPlan* out) {
  if (n_wg <= 0 || !border_applies(d, dtype, flags, main_rows)) return false;
  AxisClasses ah, aw;
  axis_classes(d.Hq, d.ph, d.dilh, d.KH, d.Hi, &ah);
  axis_classes(d.Wq, d.pw, d.dilw, d.KW, d.Wi, &aw);
  BorderPlan p;
  p.n_wg = n_wg;
  p.n_ch = d.Cout / 256;
  p.steps_per_tap = d.Cin / conv_bk(dtype);
  const bool dense_out = d.osd == 1 && d.osh == 1 && d.osw == 1 && d.opd == 0 && d.oph == 0 && d.opw == 0 && d.Dq == d.Do && d.Hq == d.Ho && d.Wq == d.Wo;
  p.kr = (dense_out && d.res_mode == RES_PRE_ACT && d.res != nullptr) ? 256 / conv_bk(dtype) : 0;      // (plan_conv's ident_ok: the main launch adds the residual by identity steps)
  const int nw = (int)aw.k0.size();
  std::vector<int> of_class(ah.k0.size() * nw, -1);
  for (int h = 0; h < d.Hq; ++h)                         // classes in order of first appearance, row-major
    for (int w = 0; w < d.Wq; ++w) {
      int& c = of_class[ah.cls[h] * nw + aw.cls[w]];
      if (c < 0) {
        c = (int)p.classes.size();
        BorderClass bc = {};
        bc.kh0 = ah.k0[ah.cls[h]]; bc.kh1 = ah.k1[ah.cls[h]]; bc.kw0 = aw.k0[aw.cls[w]]; bc.kw1 = aw.k1[aw.cls[w]];
        for (int kh = bc.kh0; kh < bc.kh1; ++kh)
          for (int kw = bc.kw0; kw < bc.kw1; ++kw) bc.mask |= 1 << (kh * d.KW + kw);
        bc.n_pix = ah.count[ah.cls[h]] * aw.count[aw.cls[w]];
        p.classes.push_back(bc);
      }
    }
  int pix0 = 0;
  for (BorderClass& bc : p.classes) { bc.pix0 = pix0; pix0 += bc.n_pix; }
  p.pix.assign((size_t)d.Hq * d.Wq, 0);
  {
    std::vector<int> fill(p.classes.size(), 0);
    for (int h = 0; h < d.Hq; ++h)
      for (int w = 0; w < d.Wq; ++w) {
        const int c = of_class[ah.cls[h] * nw + aw.cls[w]];
        p.pix[p.classes[c].pix0 + fill[c]++] = h * d.Wq + w;
      }
  }
  // Only the GEMM rows [0, main_rows) are taken: the rows behind them stay with the tail launch, whose 128-pixel tiles they ran on before
  // (its ReLU writes +0 where this kernel's writes -0: a row keeps its bits only on the tile shape it had).
  const long long hw = (long long)d.Hq * d.Wq;
  p.total_steps = 0;
  for (size_t c = 0; c < p.classes.size(); ++c) {
    BorderClass& bc = p.classes[c];
    bc.row0 = (long long)p.rows.size();
    for (long long v = 0; v * hw < main_rows; ++v)        // row r of a class: view r / n_pix, class pixel r % n_pix; the last view stops at the cut
      for (int i = 0; i < bc.n_pix; ++i) {
        const long long m = v * hw + p.pix[bc.pix0 + i];
        if (m < main_rows) p.rows.push_back((int)m);
      }
    const long long live = (long long)p.rows.size() - bc.row0;
    p.rows.resize((size_t)(bc.row0 + (live + 255) / 256 * 256), -1);
    if (p.rows.size() >= (1u << 30)) return false;
    const int steps = popcount_int(bc.mask) * p.steps_per_tap + p.kr;
    for (long long t = 0; t < (live + 255) / 256; ++t)
      for (int ch = 0; ch < p.n_ch; ++ch) {
        p.tiles.push_back(BorderTile{(int)c, ch, bc.mask, steps, bc.row0 + t * 256});
        p.total_steps += steps;
      }
  }
  p.parent_steps = (main_rows / 256) * p.n_ch * (long long)(d.ntaps * p.steps_per_tap + p.kr);
  // The tiles in the order of the views they cover (a tile's middle row: view (row - class row0 + 128) / n_pix), each to the workgroup
  // with the fewest steps so far; among equals the next in XCD-major order (workgroups b, b + 8, .. share an XCD), so that a pixel tile's
  // channel tiles and its neighbours run on one L2 at about the same time.  View order, because the classes of a view gather the same
  // input pixels: dealt longest first (all interior tiles, then the edges, then the corners) every class sweeps the whole input again,
  // long after the last one did (measured: profiles/border_tiles_ab.txt).  The last n_wg tiles go longest first, which evens the ends.
  std::vector<int> by_steps(p.tiles.size());
  for (size_t i = 0; i < by_steps.size(); ++i) by_steps[i] = (int)i;
  auto mid_view = [&](int i) { const BorderClass& bc = p.classes[p.tiles[i].cls]; return (double)(p.tiles[i].row0 - bc.row0 + 128) / bc.n_pix; };
  std::stable_sort(by_steps.begin(), by_steps.end(), [&](int a, int b) { return mid_view(a) < mid_view(b); });
  if ((int)by_steps.size() > n_wg)
    std::stable_sort(by_steps.end() - n_wg, by_steps.end(), [&](int a, int b) { return p.tiles[a].steps > p.tiles[b].steps; });
  typedef std::pair<long long, std::pair<int, int>> Load;      // (steps so far, (XCD-major rank, workgroup))
  std::priority_queue<Load, std::vector<Load>, std::greater<Load>> q;
  const int per_xcd = (n_wg + 7) / 8;
  for (int b = 0; b < n_wg; ++b) q.push(Load(0, std::make_pair((b & 7) * per_xcd + (b >> 3), b)));
  std::vector<std::vector<int>> mine(n_wg);
  for (int i : by_steps) {
    Load l = q.top();
    q.pop();
    mine[l.second.second].push_back(i);
    l.first += p.tiles[i].steps;
    q.push(l);
  }
  p.max_wg_steps = 0;
  p.wg_off.assign(1, 0);
  for (int b = 0; b < n_wg; ++b) {
    long long s = 0;
    for (int i : mine[b]) { p.order.push_back(i); s += p.tiles[i].steps; }
    p.wg_off.push_back((int)p.order.size());
    if (s > p.max_wg_steps) p.max_wg_steps = s;
  }
  *out = std::move(p);
  return true;
}

int plan_conv(const ConvDesc& d, int dtype, const ConvTuning& t, ConvPlan* out) {
  RGBM_REQUIRE(d.M > 0 && d.M < (1ll << 31), "conv M out of range");
  RGBM_REQUIRE(d.Cout % 4 == 0 && d.ldo % 4 == 0, "conv Cout/ldo must be multiples of 4");
  RGBM_REQUIRE(d.KT > 0 && d.Kpad == d.KT * conv_bk(dtype), "conv K padding mismatch");
  RGBM_REQUIRE(d.Cin % dtype_chunk(dtype) == 0, "conv Cin must be a multiple of the 16-byte chunk");
  if (d.lcin >= 0) {
    RGBM_REQUIRE((1 << d.lcin) == d.Cin, "conv lcin mismatch");
  } else {
    RGBM_REQUIRE(d.ntaps == 1, "linear-K mode needs a single tap");
  }
  const int f = t.flags, n_cu = t.n_cu;
  const long long esz = (long long)dtype_size(dtype);
  const bool bits16 = esz == 2, mfma32 = dtype != F32;      // mfma32: the storage types conv_igemm_m32_kernel exists for (16-bit, split pairs)
  const int ch_tile = conv_ch_tile(d.Cout);
  const bool uni = uniform_taps(d, conv_bk(dtype)) && !(f & DBG_NONUNIFORM_TAPS);
  const bool out16 = (((unsigned long long)d.out | (unsigned long long)(d.ldo * esz)) & 15ull) == 0ull;      // 16-byte aligned output rows
  const bool rows16 = out16 && ((unsigned long long)d.res & 15ull) == 0ull;                                  // ... and residual rows
  const bool dense_out = d.osd == 1 && d.osh == 1 && d.osw == 1 && d.opd == 0 && d.oph == 0 && d.opw == 0 && d.Dq == d.Do && d.Hq == d.Ho && d.Wq == d.Wo;
  // the m32 kernels can add a pre-activation residual on the matrix pipe (identity K steps): the same arithmetic whichever tile a row falls into
  const bool ident_ok = dense_out && d.res_mode == RES_PRE_ACT && d.res != nullptr && d.M * d.ldo * esz < (1ll << 32) - 65536;
  // GEMM rows (output pixels) from which the persistent role-specialised kernels replace the generic tiles.  Rounds 1-3 used 65 536
  // (one 256-pixel tile per CU).  Round 4, forward + post-processing latency at small batches on one box: with the 64 x 256 tile taken
  // for launches that fit one round of the grid the persistent kernels win from ~1000 rows on in every 16-bit and
  // split-pair case — bf16 B = 1 (1568 rows in layer3) 1.86 -> 1.54 ms, B = 8 2.65 -> 2.43 ms; split pairs B = 1 3.35 -> 2.51 ms, B = 2
  // 3.56 -> 2.83, B = 4 4.02 -> 3.36, B = 8 5.18 -> 4.62 ms — and fp32 does not care (7.1 / 8.3 / 11.0 / 17.6 ms either way).
  const bool ws_rows = d.M >= (t.ws_min_rows > 0 ? t.ws_min_rows : 1024);

  ConvPlan p = {};
  p.uniform_taps = uni;
  p.ksplit = 1;
  p.korder = (f & DBG_KORDER_TAPS_OUTER) ? 0 : 1;
  auto pick = [&](int kernel, int bch, int bpix) {
    p.kernel = kernel; p.bch = bch; p.bpix = bpix;
    p.buf_ok = buffer_offsets_ok(d, bch, esz) && !(f & DBG_GLOBAL_ADDR);
    *out = p;
    return 0;
  };
  auto generic = [&]() { return pick(CONV_GENERIC, ch_tile, ch_tile == 128 ? 128 : 256); };
  auto small = [&](int bch) {
    p.ksplit = m32_ksplit_choice(d, f, ((d.M + 127) / 128) * ((d.Cout + bch - 1) / bch), n_cu, bch, 4);
    // (layers of fewer than 256 channels — layer2 at one to four poses — add their residual in the epilogue: the identity steps turn an
    // infinite residual into NaN, and these layers' launches are held to the saturating-store contract of the kernels they replace)
    p.identity_residual = ident_ok && d.Cout % 256 == 0;
    return pick(CONV_M32_SMALL, bch, 128);
  };

  if (d.out_f32) {      // only the generic tile's epilogue knows the plain-fp32 output form
    RGBM_REQUIRE(dtype == BF16X3 && d.w2 == nullptr, "out_f32 is a bf16x3 option of the generic kernel");
    return generic();
  }
  // >= 128 output channels and enough pixel tiles to fill the chip: the 256x128 three-stage kernel
  if (ch_tile == 128 && !(f & DBG_NO_WS) && ws_rows) {
    // role-specialised (uniform taps, 16-byte aligned output / residual rows)
    if (!uni || (f & DBG_V3_FOR_WS) || !rows16) return pick(CONV_V3, 128, 256);
    // Small launches (B = 1 .. 8): the 256 x 128 / 128 x 256 tiles leave most CUs idle (layer3 at B = 1: 13 tiles), and every tile walks
    // the whole K range.  The 64-channel x 256-pixel shape of the same kernel makes 2-4x as many tiles of a quarter / half of the work;
    // taken while even those fit one round of the persistent grid (DBG_NO_SLIM_SMALL: never).
    if (!(f & DBG_NO_SLIM_SMALL) && d.Cout % 64 == 0) {
      const long long slim_tiles = ((d.M + 255) / 256) * (d.Cout / 64);
      if (mfma32) {
        // round 6: launches that do not fill the grid with 256-pixel tiles of the 256-channel layers pick their tile by requested bytes
        // (m32_small_choice; DBG_M32_TAILS_R5: as in round 5)
        if (d.Cout % 256 == 0 && ((d.M + 255) / 256) * (d.Cout / 256) < n_cu && t.gemm_kernel >= 1 && !(f & (DBG_M32_TAILS_R5 | DBG_WS_128x256)) &&
            buffer_offsets_ok(d, 256, esz)) {
          // (gemm_kernel = 1, the A/B reference: the same arithmetic on 256-channel x 128-pixel tiles - bit-identical results)
          const int bch = t.gemm_kernel == 1 ? 256 : m32_small_choice(d, n_cu, slim_tiles <= n_cu);
          if (bch) return small(bch);
        }
        // layer2's 128-channel layers at one to four poses (13-52 tiles of 64 x 256): 64-channel x 128-pixel tiles of the 32x32x16 kernel with
        // their K loop split (igemm_m32.hip) — taken only where the split applies, i.e. while twice the tiles still fit the grid
        if (d.Cout == 128 && ((d.M + 127) / 128) * 2 * 2 <= n_cu && t.gemm_kernel == 2 &&
            !(f & (DBG_M32_TAILS_R5 | DBG_WS_128x256 | DBG_NO_KSPLIT | DBG_L2_SLIM_TILE)) && d.w2 == nullptr && buffer_offsets_ok(d, 64, esz))
          return small(64);
      }
      if (slim_tiles <= n_cu) return pick(CONV_WS_SLIM, 64, 256);
    }
    if (d.Cout % 256 == 0 && !(f & DBG_WS_128x256)) {
      // conv_igemm_m32_kernel's request waves address both operands through 32-bit buffer offsets
      if (!(mfma32 && buffer_offsets_ok(d, 256, esz) && t.gemm_kernel >= 1)) return pick(CONV_WS_WIDE, 256, 128);
      // Whole rounds of 256 x 256 tiles over the persistent grid, the rest of the rows (a partial last round, a ragged last pixel tile) on
      // 128-pixel tiles in a second launch — cut in channels too (round 6) so that the rest gives every CU a tile: the smallest of 64 / 128 /
      // 256 channels whose tile count still fits one round (layer3's 8192 left-over rows: 64 tiles of 256 x 128 on a quarter of the chip
      // before, 256 tiles of 64 x 128 now).  gemm_kernel = 1: every row on 256 x 128 tiles.
      const bool big_ok = dense_out && (d.bias == nullptr || (d.bias_stride == 0 && d.Cout <= 2560)) && d.act != ACT_TANH &&
                          (d.res_mode == RES_NONE || (d.res_mode == RES_PRE_ACT && d.res != nullptr)) && d.M * d.ldo * esz < (1ll << 32) - 65536;
      const long long P = d.M / 256, n_ch = d.Cout / 256, tiles = P * n_ch;
      long long Pm = 0;
      if (t.gemm_kernel != 1 && big_ok && tiles >= n_cu) {
        const long long rem = tiles % n_cu;
        // a last round that fills less than ~60 % of the chip costs more on 256-pixel tiles than its rows cost on 128-pixel tiles afterwards
        Pm = (rem == 0 || rem * 10 >= (long long)n_cu * 6) ? P : (tiles - rem) / n_ch;
      }
      p.main_rows = Pm * 256;
      p.identity_residual = ident_ok;
      p.border = p.main_rows > 0 && p.korder == 1 && uni && border_applies(d, dtype, f, p.main_rows);
      p.tail_bch = p.main_rows == d.M ? 0 : 256;
      // the rest: 128-pixel tiles, channels cut so that the tiles fill (at most) one round of the grid (DBG_M32_TAILS_R5: 256 channels)
      const long long pt = (d.M - p.main_rows + 127) / 128;
      if (p.tail_bch && t.gemm_kernel != 1 && !(f & DBG_M32_TAILS_R5)) {
        if (pt * (d.Cout / 64) <= n_cu) p.tail_bch = 64;
        else if (pt * (d.Cout / 128) <= n_cu) p.tail_bch = 128;
      }
      return pick(CONV_M32, 256, 256);
    }
    // (round 6 measured layer2's 128-channel layers on 128 x 256 tiles of the 32x32x16 kernel: 0.122 against 0.119 ms per launch in bf16,
    // 0.293 against 0.291 in split pairs - a 128-channel tile needs 48 KB per 1024 cycles of MFMA and is request-bound in either kernel)
    return pick(CONV_WS, 128, 256);
  }
  // 33..64 output channels, 16-bit storage, no residual, >= 2 K tiles: the three-role persistent kernel, the only one that can fuse a
  // trailing 1x1 (then `out` is not written; else 16-byte aligned output rows)
  if (bits16 && uni && !(f & DBG_NO_WS64) && ch_tile == 64 && d.res_mode == RES_NONE && d.KT >= 2 && ws_rows &&
      (d.w2 ? d.Cout == 64 && d.kpad2 == 64 && (d.cout2 == 16 || d.cout2 == 32) && d.ldo2 % 4 == 0 : out16))
    return rowhalo_ok(d) && !(f & DBG_NO_ROWHALO) ? pick(CONV_WS64_ROWHALO, 64, 256) : pick(CONV_WS64, 64, 256);
  RGBM_REQUIRE(d.w2 == nullptr, "a fused 1x1 needs the ws64 kernel (ConvLayer::run_then_1x1 then runs the two layers)");
  // 33..64 output channels where there is no ws64 kernel (split pairs, fp32) or it does not apply (residual adds): the
  // role-specialised kernel with a 64 x 256 tile and four multiply waves
  // (round 6 measured 64-channel x 256-pixel tiles of the 32x32x16 kernel for layer1's 64-channel layers at batch 256: split pairs 0.542 ms
  // per launch against 0.475 on this tile, bf16 38.39 ms per forward against 38.10 with the row-halo ws64 kernel — not dispatched)
  if (ch_tile == 64 && uni && ws_rows && !(f & (DBG_NO_WS | DBG_V3_FOR_WS | DBG_NO_SLIM64)) && rows16) return pick(CONV_WS_SLIM, 64, 256);
  return generic();
}

}  // namespace rgbm
