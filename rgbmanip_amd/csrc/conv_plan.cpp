#include "conv_plan.h"

#include "kernels.h"

namespace rgbm {

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

}  // namespace

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
        // their K loop split (conv_igemm_m32.inc) — taken only where the split applies, i.e. while twice the tiles still fit the grid
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
  RGBM_REQUIRE(d.w2 == nullptr, "a fused 1x1 needs the ws64 kernel (check conv_ws64_eligible first)");
  // 33..64 output channels where there is no ws64 kernel (split pairs, fp32) or it does not apply (residual adds): the
  // role-specialised kernel with a 64 x 256 tile and four multiply waves
  // (round 6 measured 64-channel x 256-pixel tiles of the 32x32x16 kernel for layer1's 64-channel layers at batch 256: split pairs 0.542 ms
  // per launch against 0.475 on this tile, bf16 38.39 ms per forward against 38.10 with the row-halo ws64 kernel — not dispatched)
  if (ch_tile == 64 && uni && ws_rows && !(f & (DBG_NO_WS | DBG_V3_FOR_WS | DBG_NO_SLIM64)) && rows16) return pick(CONV_WS_SLIM, 64, 256);
  return generic();
}

}  // namespace rgbm
