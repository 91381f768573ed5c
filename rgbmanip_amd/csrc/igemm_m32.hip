// Implicit-GEMM tiles on v_mfma_f32_32x32x16 (gfx950): conv_igemm_m32_kernel, 16-bit storage types and split pairs.  Shared pieces: igemm_device.h.
// For the layers that carry the PSPNet backbone (lib/pspnet.py:11-30,42-43,59-62 of the reference: layer3 / layer4 BasicBlocks with
// dilation 2 / 4, residual + ReLU epilogue; :97-107 up_1 as a 1x1 GEMM).
//
// Round 5 measured what bounds conv_igemm_ws_kernel's K loop (timers in the request waves, tools/abl_m32_run*.sh): not the matrix pipe
// but the request waves' ISSUE of LDS-DMA pieces — 1780 cycles per 48 KB K tile with 64-bit global addresses, 64 cycles waiting for
// landings.  A CU takes at most ~60 bytes per clock out of L2 however it is asked (tools/micro/cu_fill_rate.hip: eight loader waves,
// any instruction form; four waves reach 42-46 B/clk with global_load_lds, 50-60 with buffer descriptors), and a 256 x 128 tile needs
// 48 KB per 1024 cycles of MFMA = 47 B/clk to run at the matrix rate.  So: (1) requests through buffer descriptors (blds16), (2) a
// tile with fewer bytes per flop.
//
//   BPIX = 256: 256 channels x 256 pixels, 64 KB per K tile for 2048 cycles of MFMA per SIMD (32 B/clk at the matrix rate), two
//               64 KB stages; 8 multiply waves (two per SIMD, 128 channels x 64 pixels = 4 x 2 fragments of 32 x 32 = 128 accumulators
//               each) + 4 request waves; the request of K tile g+1 goes out behind barrier g and has a whole K tile of MFMAs to land.
//   BPIX = 128: 256 x 128, three 48 KB stages, ONE multiply wave per SIMD (4 + 4 waves), fragment reads one 16-deep step ahead in two
//               register sets; the tile the 256-pixel launches leave over (launch_m32) and the A/B reference.  Round 6: 64 / 128-channel
//               variants of it (BCH) for the tails and for small batches, and for launches of at most half a grid of those a K split
//               (ConvDesc::ksplit: parts of a tile's K loop on separate workgroups, fixed-order sum by the last part to arrive).
// C layout: MFMA row i of fragment a carries channel a*32 + ((i>>2)&1)*16 + (i&3) + 4*(i>>3), so the 16 results of a lane are 16
// CONSECUTIVE channels of its pixel (two 16-byte stores; residual reads likewise), and with that permutation the plain (row>>1)&7
// chunk swizzle is conflict-free for the 16-lane groups ds_read_b128 is served in, for W and X rows alike.
// ---------------------------------------------------------------------------------------------------------
#include <atomic>
#include "igemm_device.h"

namespace rgbm {

#ifndef M32_SHIFT
#define M32_SHIFT 1   // 256-pixel tiles, 16-bit types: the K-tile barrier is passed in front of a K tile's LAST sub-step (see the multiply waves; 0 = at its head, for A/B)
#endif
#ifndef M32_RACE_PROBE
#define M32_RACE_PROBE 0   // 1 = a race probe with RIGHT results (tools/abl_flags.sh): multiply wave 5 sleeps ~4000 cycles behind the barrier of every
                           // tile's last K step, i.e. reads that step's fragments long after the other waves have gone on to their epilogues
                           // (the outputs must stay bit-identical)
#endif
typedef __attribute__((ext_vector_type(16))) float f32x16;

template <typename T> struct Mma32;
template <> struct Mma32<unsigned short> {
  __device__ static __forceinline__ void run(const uint4& a, const uint4& b, f32x16& c) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  }
};
template <> struct Mma32<f16_t> {
  __device__ static __forceinline__ void run(const uint4& a, const uint4& b, f32x16& c) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  }
};

// channel (within a 32-channel fragment) carried by MFMA row i
__device__ __forceinline__ int m32_row_channel(int i) { return ((i >> 2) & 1) * 16 + (i & 3) + 4 * (i >> 3); }

// BCH (round 6): output channels per tile.  256 = the tiles of rounds 5-6; 128 / 64 = the tail launches (the rows a partial last round
// leaves over, cut in channels too so that they give every CU a tile).  A multiply wave then owns BCH / 2 channels (BCH / 64 fragments
// of 32).  (128 x 256 tiles for layer2's 128-channel layers were measured and are level with conv_igemm_ws_kernel: request-bound.)
template <typename T, int BPIX, int BCH = 256>
__global__ __launch_bounds__(BPIX == 256 ? 768 : 512) void conv_igemm_m32_kernel(const ConvDesc d) {
  constexpr bool BIG = BPIX == 256;
  constexpr bool STAGED = BIG && BCH == 256;      // the output tile leaves through the ring stage of the last K step as whole 256-byte rows
  constexpr bool X3 = std::is_same<T, bx3_t>::value;      // split pairs: 4-byte slots, 32 channels per 128-byte row, three MFMAs per product
  constexpr int NMW = BIG ? 8 : 4;           // multiply waves; four request waves follow (eight for the 64 / 128-channel x 128-pixel tiles, i.e. half the
                                             // LDS-DMA pieces per wave: measured level at B = 1 / 2 / 8 in both storage types, round 6 — a one-tile launch's K step
                                             // costs ≈ 0.22 us + its bytes at ≈ 97 GB/s per CU (24 / 32 / 48 KB: 0.47 / 0.58 / 0.72 us), whoever requests them;
                                             // EIGHT MULTIPLY waves of 32 / 64 channels x 64 pixels on the 128 / 256-channel x 128-pixel tiles (two per SIMD covering
                                             // each other's step boundary; 150 registers and no spills where the 256-channel one has 256 and 124 bytes): level too
                                             // at B = 1 .. 16 — what a small batch's GEMM lacks is CUs fetching, not waves)
  constexpr int NTH = (NMW + 4) * 64;
  constexpr int NST = BIG ? 2 : 3;           // ring stages (128-pixel tiles with 4 / 6 stages of their 32 / 24 KB were measured at B = 1 / 8, round 6: bit-identical
                                             // and 3-5 % SLOWER at B = 1, level at B = 8 — a one-tile launch is bound by the multiply waves' own chain per K step
                                             // (barrier, first fragment reads, eight dependent MFMAs), not by requests in flight; the longer prologue only delays it)
  static_assert(BCH == 256 || BCH == 128 || BCH == 64, "channel tiles of 256 / 128 / 64");
  constexpr int E = 16 / sizeof(T);
  constexpr int BK = 8 * E;                  // 64 channels of a tap: 128-byte rows
  constexpr int XR = BPIX / 32;              // gathered rows per request thread
  constexpr int WL = BCH / 32;               // weight rows per request thread
  constexpr int NP = XR + WL;                // LDS-DMA pieces per request wave and K tile
  constexpr int FA = BCH / 64, FB = 2;       // 32 x 32 fragments of a multiply wave: BCH / 2 channels x 64 pixels
  constexpr int WCHW = FA * 32;              // channels of a multiply wave (two rows of waves share the tile's channels)
  constexpr int STAGE = (BCH + BPIX) * 8;    // uint4 slots per stage
  extern __shared__ __attribute__((aligned(16))) uint4 lds3[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // 0..NMW-1 multiply, then request
  // K split (128-pixel tiles, ConvDesc::ksplit > 1; launch_m32_range gives every (tile, part) its own workgroup): part p of a tile walks K steps
  // [p * KT / n, (p + 1) * KT / n); part 0 starts from the bias, the last part also runs the residual steps; see the reduction in front of the epilogue
  // (64 / 128-channel tiles only: in the 256-channel one the reduction's registers push 170 more bytes of accumulators into scratch)
  constexpr bool KSPLIT = !BIG && BCH <= 128;
  int KT = d.KT, kt0 = 0, part = 0, nsp = 1, vtile = -1;
  if constexpr (KSPLIT) {
    if (d.ksplit > 1) {
      nsp = d.ksplit;
      part = (int)blockIdx.x % nsp;
      vtile = (int)blockIdx.x / nsp;
      kt0 = (int)((long long)part * d.KT / nsp);
      KT = (int)((long long)(part + 1) * d.KT / nsp) - kt0;
    }
  }
  // d.ident set (launch_m32): a pre-activation residual rides the matrix pipe — KR extra K steps whose X operand is the residual tile (pixel rows, 64 channels
  // per step) and whose W operand is a 256 x 256 identity (d.ident): acc += 1.0 * r is exact, costs no register, no epilogue load (in the
  // in-order vmcnt queue of a multiply wave a load behind the output stores waits for their round trip) and uses the ring as it is.
  // 4 steps on top of 36 (layer3) or 72 (layer4).
  // Round 6, 256 x 256 tile: the identity is block diagonal, so an accumulator fragment (32 channels x 32 pixels) needs only its own 32
  // residual channels — in residual step r only the waves whose 128 channels contain the step's channel block multiply, with a CONSTANT
  // A fragment built in registers (one 1.0 per MFMA row; see the multiply waves), two MFMAs per fragment and 16-deep sub-step instead of
  // the full step's eight: 16 instead of 128 MFMAs per wave and tile, no identity rows through the ring.  acc + 1.0 * r + 0 * (15 other
  // residual values) is the same fp32 sum as before (finite values), so both tile sizes still agree bit for bit.
  const bool res_in_acc = d.ident != nullptr && d.res_mode == RES_PRE_ACT;      // the residual reaches the accumulators through KR identity steps (of the last K part)
  const int KR = (res_in_acc && part == nsp - 1) ? BCH / BK : 0;
  const int KTT = KT + KR;
  // Border-class tiles (256 x 256, d.btab set; conv_plan.h): this workgroup's tiles are the table entries [be0, be0 + n_my).  An entry
  // names the tile's 256 table rows, its K steps and the rectangle of taps they walk; EVERY wave takes a tile's step count from that one
  // entry (bsteps), so the multiply waves, the request waves and `total` count the same barriers.
  const bool bm = STAGED && !X3 && d.btab != nullptr;      // (16-bit types: with split pairs the table's registers push 390 bytes of accumulators into scratch)
  const int* __restrict__ bent = d.btab;
  int n_my = vtile >= 0 ? 1 : ((int)d.n_tiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
  int total = n_my * KTT;                    // K-tile steps of this workgroup; every wave passes `total` barriers
  if (bm) {
    const int be0 = d.btab[blockIdx.x];
    n_my = d.btab[blockIdx.x + 1] - be0;
    bent = d.btab + d.b_ent + 4 * be0;
    total = 0;
    for (int k = 0; k < n_my; ++k) total += bent[4 * k + 1] + KR;
  }
  auto bsteps = [&](int k) { return bm ? __builtin_amdgcn_readfirstlane(bent[4 * k + 1]) : KT; };      // K steps of tile k without the residual steps
  auto tile_of = [&](int k, int& pix_tile, int& ch_tile) {
    if (bm) { pix_tile = 0; ch_tile = __builtin_amdgcn_readfirstlane(bent[4 * k + 2]) >> 16; return; }
    const int v = vtile >= 0 ? vtile : (int)blockIdx.x + k * (int)gridDim.x;          // virtual workgroup id -> XCD-aware tile order
    const int nblk = d.n_tiles, bq = nblk >> 3, br = nblk & 7, xcd = v & 7, bidx = v >> 3;
    const int lid = (xcd < br ? xcd * (bq + 1) : br * (bq + 1) + (xcd - br) * bq) + bidx;
    pix_tile = lid / d.n_ch_tiles;
    ch_tile = lid - pix_tile * d.n_ch_tiles;
  };

  float* lbias = reinterpret_cast<float*>(lds3 + NST * STAGE);
  const bool bias_lds = d.bias != nullptr && d.bias_stride == 0 && d.Cout <= 2560;
  if (bias_lds)
    for (int i = tid; i < d.Cout; i += NTH) lbias[i] = d.bias[i];
  __syncthreads();

  if (wave >= NMW) {
    // ------------------------------------------------------------------ request waves (the tap walk of conv_igemm_ws_kernel)
    const int pw = wave - NMW;
    const int tp = tid - NMW * 64;
    const int j = tp & 7;
    const int r0 = tp >> 3;                  // 0..31
    const int js = j ^ ((r0 >> 1) & 7);      // rows r0 + 32*i share bits 1..3 with r0: one swizzle for all of a thread's rows (W and X)
    unsigned rmask[XR], xoff[XR], woff[WL], roff[XR];
    int tkd = 0, tkh = 0, tkw = 0, tc = 0;   // wave-uniform tap walker
    unsigned wko = 0;                        // byte offset of the walker's K index in a weight row
    const unsigned lds0 = __builtin_amdgcn_readfirstlane(lds_addr(lds3 + pw * 64));      // this wave's first piece, stage 0
    // Both operands through buffer descriptors (plan_conv checked that they fit 32-bit offsets).  X offsets are taken from
    // (input base - xbias) so that a row whose tap (0,0,0) lies in the padding still has a non-negative offset; a padded lane gets
    // an offset beyond num_records and lands as zeros.
    const long long xbias = ((long long)(d.pd * d.Hi + d.ph) * d.Wi + d.pw) * d.Cin * (long long)sizeof(T);
    const __amdgpu_buffer_rsrc_t rsrc_x = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(d.in)) - xbias, 0,
        (int)(unsigned)((long long)d.N * d.Di * d.Hi * d.Wi * d.Cin * (long long)sizeof(T) + xbias), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrc_w = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(d.wgt)), 0, (int)(unsigned)((long long)d.n_ch_tiles * BCH * d.Kpad * (long long)sizeof(T)), 0x00020000);

    const __amdgpu_buffer_rsrc_t rsrc_r = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(d.res)), 0, (int)(unsigned)(d.M * d.ldo * (long long)sizeof(T)), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrc_i = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(d.ident)), 0, (int)(unsigned)(256 * 256 * sizeof(T)), 0x00020000);
    long long mybase = 0;
    unsigned mymask = 0;
    int my_ch_tile = 0, my_pix_tile = 0;
    int ikt = 0, itile = 0;                  // K tile / tile index of the next request
    // border-class tiles: the request side's copy of the current tile's entry (K steps, tap rectangle) and this lane's GEMM row (-1: dead)
    int KTc = KT, KTTc = KTT, bkh0 = 0, bkh1 = 0, bkw0 = 0, bkw1 = 0, mym = -1;
    int* lrow = reinterpret_cast<int*>(lbias + 2560);      // [2][256]: the GEMM rows of tile k at (k & 1) * 256, for the multiply waves' epilogue
    auto decode_my = [&](long long m) {      // this lane's row: its first input pixel and which taps are in range (border-class tiles: all of the tile's)
      mybase = 0;
      mymask = 0;
      if (j < XR) {
        int xn = 0, xd0 = -(1 << 20), xh0 = 0, xw0 = 0;
        if (m >= 0 && m < d.M) {
          unsigned n, qd, qh, qw;
          decode_row(d, (unsigned)m, n, qd, qh, qw);
          xn = (int)n * d.Di;
          xd0 = (int)qd * d.sd - d.pd;
          xh0 = (int)qh * d.sh - d.ph;
          xw0 = (int)qw * d.sw - d.pw;
        }
        for (int kk = 0; kk < d.KD; ++kk) mymask |= (unsigned)((unsigned)(xd0 + kk * d.dild) < (unsigned)d.Di) << kk;
        for (int kk = 0; kk < d.KH; ++kk) mymask |= (unsigned)((unsigned)(xh0 + kk * d.dilh) < (unsigned)d.Hi) << (8 + kk);
        for (int kk = 0; kk < d.KW; ++kk) mymask |= (unsigned)((unsigned)(xw0 + kk * d.dilw) < (unsigned)d.Wi) << (16 + kk);
        if (bm) mymask = m >= 0 ? 0x00ffffffu : 0u;      // every tap the walker visits is in range for every live row
        const long long pix0 = ((long long)(xn + xd0) * d.Hi + xh0) * d.Wi + xw0;
        mybase = pix0 * d.Cin * (long long)sizeof(T);
      }
    };
    auto prepare_tile = [&](int k) {         // lane j of a row group decodes GEMM row r0 + 32*j; the group exchanges them (enter_tile)
      int pix_tile, ch_tile;
      tile_of(k, pix_tile, ch_tile);
      my_ch_tile = ch_tile;
      my_pix_tile = pix_tile;
      if (bm) {
        // the row comes from the table; it is decoded in enter_tile, behind the next counted wait (its load queues behind this step's pieces)
        const int tr = __builtin_amdgcn_readfirstlane(bent[4 * k + 2]);
        KTc = bsteps(k);
        KTTc = KTc + KR;
        bkh0 = tr & 15; bkh1 = (tr >> 4) & 15; bkw0 = (tr >> 8) & 15; bkw1 = (tr >> 12) & 15;
        mym = j < XR ? d.btab[d.b_rows + __builtin_amdgcn_readfirstlane(bent[4 * k]) + r0 + 32 * j] : -1;
        return;
      }
      decode_my(d.m0 + (long long)pix_tile * BPIX + r0 + 32 * j);
    };
    auto enter_tile = [&]() {
      const int grp = (tp & 63) & 56;
      if (bm) {
        decode_my(mym);
        if (j < XR) lrow[(itile & 1) * 256 + r0 + 32 * j] = mym;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // written before this wave's next barrier; read behind the tile's last one
      }
#pragma unroll
      for (int i = 0; i < XR; ++i) {
        const long long b = __shfl(mybase, grp | i, 64);
        rmask[i] = (unsigned)__shfl((int)mymask, grp | i, 64);
        xoff[i] = (unsigned)(b + xbias + (long long)(js * E) * (long long)sizeof(T));
        if (KR) {
          long long m = d.m0 + (long long)my_pix_tile * BPIX + r0 + 32 * i;      // residual row of GEMM row m (dense output: row m of [M][ldo])
          if (bm) { m = __shfl(mym, grp | i, 64); if (m < 0) m = d.M; }
          roff[i] = m < d.M ? (unsigned)((m * d.ldo + my_ch_tile * BCH + js * E) * (long long)sizeof(T)) : 0xffffffffu;
        }
      }
#pragma unroll
      for (int i = 0; i < WL; ++i) {
        const int row = r0 + 32 * i;
        woff[i] = (unsigned)(((long long)(my_ch_tile * BCH + row) * d.Kpad + js * E) * (long long)sizeof(T));
      }
      tkd = tkh = tkw = tc = 0;
      wko = 0;
      if (bm) {                                // the walker starts at the first tap of the tile's rectangle
        tkh = bkh0; tkw = bkw0;
        wko = (unsigned)((tkh * d.KW + tkw) * d.Cin) * (unsigned)sizeof(T);
      }
      if (kt0 > 0) {                           // K split: the walker starts at K step kt0 (the closed form of the advance at the end of issue())
        if (d.korder && d.lcin >= 0) {         // channel block outer, taps inner
          const int tap = kt0 % d.ntaps, cb = kt0 / d.ntaps;
          tkw = tap % d.KW; tkh = (tap / d.KW) % d.KH; tkd = tap / (d.KW * d.KH);
          tc = cb * BK;
          wko = (unsigned)(((long long)tap * d.Cin + tc) * (long long)sizeof(T));
        } else {
          wko = (unsigned)kt0 * (unsigned)(BK * sizeof(T));
          if (d.lcin >= 0) {                   // taps outer, channel blocks inner
            const int cpt = d.Cin / BK, tap = kt0 / cpt;
            tc = (kt0 - tap * cpt) * BK;
            tkw = tap % d.KW; tkh = (tap / d.KW) % d.KH; tkd = tap / (d.KW * d.KH);
          } else {
            tc = kt0 * BK;
          }
        }
      }
    };

    auto issue = [&](int stage) {
      if (ikt == 0) enter_tile();
      const unsigned sbase = lds0 + (unsigned)stage * (STAGE * 16);
      const unsigned sel = (1u << tkd) | (256u << tkh) | (65536u << tkw);
      const unsigned soff = (unsigned)(((long long)((tkd * d.dild * d.Hi + tkh * d.dilh) * d.Wi + tkw * d.dilw) * d.Cin + tc) * (long long)sizeof(T));
      const bool cok = tkd < d.KD && tc + js * E < d.Cin;
      if (ikt >= KTc) {
        // residual step r: X = residual rows, channels 64r .. 64r+63 of this channel tile; W = identity rows, the same 64 columns
        const unsigned ro = (unsigned)(ikt - KTc) * (unsigned)(BK * sizeof(T));
#pragma unroll
        for (int i = 0; i < XR; ++i) blds16(roff[i], rsrc_r, ro, sbase + (BCH * 8 + i * 256) * 16);
        // (256 x 256: the multiply waves hold the identity's diagonal blocks as a constant A fragment — no W rows for these steps)
        if (!BIG) {
#pragma unroll
          for (int i = 0; i < WL; ++i) blds16((unsigned)(((r0 + 32 * i) * 256 + js * E) * (int)sizeof(T)), rsrc_i, ro, sbase + (i * 256) * 16);      // (d.ident is 256 x 256)
        }
      } else {
#pragma unroll
        for (int i = 0; i < XR; ++i) {
          const bool ok = cok && (rmask[i] & sel) == sel;
          blds16(ok ? xoff[i] : 0xffffffffu, rsrc_x, soff, sbase + (BCH * 8 + i * 256) * 16);      // X rows 32*i + 8*pw .. +7
        }
#pragma unroll
        for (int i = 0; i < WL; ++i) blds16(woff[i], rsrc_w, wko, sbase + (i * 256) * 16);          // W rows 32*i + 8*pw .. +7
      }
      if (ikt >= KTc) {
      } else if (bm) {                       // channel block outer, the rectangle's taps inner; the weight K offset jumps with the tap
        if (++tkw == bkw1) { tkw = bkw0; if (++tkh == bkh1) { tkh = bkh0; tc += BK; } }
        wko = (unsigned)((tkh * d.KW + tkw) * d.Cin + tc) * (unsigned)sizeof(T);
      } else if (d.korder && d.lcin >= 0) {  // channel block outer, taps inner (see conv_igemm_ws_kernel)
        wko += (unsigned)d.Cin * (unsigned)sizeof(T);
        if (++tkw == d.KW) { tkw = 0; if (++tkh == d.KH) { tkh = 0; if (++tkd == d.KD) { tkd = 0; tc += BK; wko = (unsigned)tc * (unsigned)sizeof(T); } } }
      } else {
        wko += BK * (unsigned)sizeof(T);
        tc += BK;
        if (d.lcin >= 0 && tc >= d.Cin) {
          tc = 0;
          if (++tkw == d.KW) { tkw = 0; if (++tkh == d.KH) { tkh = 0; ++tkd; } }
        }
      }
      if (++ikt == KTTc) { ikt = 0; ++itile; if (itile < n_my) prepare_tile(itile); }
    };

    if (total > 0) prepare_tile(0);
    if (total > 0) issue(0);
    if (NST == 3 && total > 1) issue(1);
    int st = 0, gk = 0, gtile = 0;
    int gKTT = total > 0 ? bsteps(0) + KR : KTT;      // steps of the tile that step g belongs to (the requests run one step ahead of it)
    for (int g = 0; g < total; ++g) {
      // three stages: step g landed, step g+1 may still fly; two stages: the one request in flight is step g
      if (NST == 2 || g + 1 >= total) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(%0)" :: "n"(NP) : "memory");
      RGBM_BARRIER();              // step g is complete in LDS; every fragment read of step g-1 has returned: its stage is free
      if (NST == 3) { if (g + 2 < total) issue(st == 0 ? 2 : st - 1); }
      else { if (g + 1 < total) issue(st ^ 1); }
      st = st == NST - 1 ? 0 : st + 1;
      // 256 x 256: the multiply waves stage their output tile in the ring stage of the tile's last K step; the workgroup meets once more
      // behind that step (every multiply wave's fragment reads have returned) before the first staging write — see the epilogue
      if (STAGED) { if (++gk == gKTT) { gk = 0; RGBM_BARRIER(); if (++gtile < n_my) gKTT = bsteps(gtile) + KR; } }
    }
    return;
  }

  // -------------------------------------------------------------------- multiply waves
  const int wch = BIG ? (wave >> 2) * WCHW : (wave >> 1) * WCHW;
  const int wpix = BIG ? (wave & 3) * 64 : (wave & 1) * 64;
  const int li = lane & 31, lh = lane >> 5;
  // byte offsets (inside a stage) of this lane's chunk of step 0 in its first A / B fragment row; step s is at ^ (s << 5), fragment
  // f at + f * 4096 (32 rows of 128 bytes).  Rows of a fragment share bits 1..3 with the lane's first row, so one swizzle serves all.
  const int rowA = wch + m32_row_channel(li), rowB = wpix + li;
  const unsigned offA = (unsigned)(rowA * 8 + (lh ^ ((rowA >> 1) & 7))) * 16u;
  const unsigned offB = (unsigned)(BCH * 8 + rowB * 8 + (lh ^ ((rowB >> 1) & 7))) * 16u;
  const char* ldsc = reinterpret_cast<const char*>(lds3);
  f32x16 acc[FA][FB];
  // residual steps of the 256 x 256 tile: MFMA row li of a fragment carries channel 16 * id_s + id_c of the fragment's 32 (m32_row_channel),
  // a lane's eight K values of a 16-deep sub-step are channels 8 * lh .. + 7 of it: the identity block has its 1.0 in sub-step id_s, on the
  // lanes with lh == id_c >> 3, at K position id_c & 7 (16-bit slot of the operand; split pairs: of the hi operand, lo = 0)
  // (computed where it is used, from an opaque copy of the lane id: as loop invariants hipcc kept both fragments across the K loop — in scratch)
  auto ident_frag = [&](int sub) {
    int lq = lane;
    asm volatile("" : "+v"(lq));
    const int qi = lq & 31, qh = lq >> 5;
    const int id_s = (qi >> 2) & 1, id_c = (qi & 3) + 4 * (qi >> 3);
    const int lh = qh;
    const unsigned one = std::is_same<T, f16_t>::value ? 0x3c00u : 0x3f80u;
    const bool mine = sub == id_s && lh == (id_c >> 3);
    const unsigned w = mine ? one << (16 * (id_c & 1)) : 0u;
    const int q = (id_c & 7) >> 1;
    return make_uint4(q == 0 ? w : 0u, q == 1 ? w : 0u, q == 2 ? w : 0u, q == 3 ? w : 0u);
  };
  T* __restrict__ out = reinterpret_cast<T*>(d.out);
  const T* __restrict__ res = reinterpret_cast<const T*>(d.res);
  auto tile_interior = [&](int pix_tile, int ch_tile) {
    if (bm) return true;      // (the plan takes only layers whose every tile has the straight-line epilogue; dead rows are not stored)
    return (d.bias == nullptr || bias_lds) && d.m0 + (long long)(pix_tile + 1) * BPIX <= d.M && (ch_tile + 1) * BCH <= d.Cout && d.act != ACT_TANH;
  };
  int st = 0;
  for (int k = 0; k < n_my; ++k) {
    const int KTk = BIG ? bsteps(k) : KT;      // this tile's K steps (border-class tiles: from its table entry)
    {
      int pt, ct;
      tile_of(k, pt, ct);
      if (tile_interior(pt, ct) && d.bias && part == 0) {
        const float* bp = lbias + ct * BCH + wch + lh * 16;
#pragma unroll
        for (int a = 0; a < FA; ++a) {
          f32x16 b16;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const f32x4 b4 = *reinterpret_cast<const f32x4*>(bp + a * 32 + q * 4);
            b16[q * 4 + 0] = b4[0]; b16[q * 4 + 1] = b4[1]; b16[q * 4 + 2] = b4[2]; b16[q * 4 + 3] = b4[3];
          }
#pragma unroll
          for (int b = 0; b < FB; ++b) acc[a][b] = b16;
        }
      } else {
#pragma unroll
        for (int a = 0; a < FA; ++a)
#pragma unroll
          for (int b = 0; b < FB; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;
      }
    }
    if constexpr (X3) {
      // Split pairs: a K tile is 32 channels = two 16-deep steps.  A lane's K = 8 operand is the hi (first 8 bytes) or lo (last 8 bytes)
      // halves of two adjacent 16-byte chunks — chunks 4s + 2*lh and + 1, which sit at positions p and p ^ 1 of the swizzled row.  Every
      // row must list its eight k values in the SAME order (an A row meets every B row of the other operand), so the first half is read
      // from chunk 4s + 2*lh's own position (c ^ swz) and the second from that ^ 16 bytes: two 8-byte reads.  Per accumulator: lo*hi,
      // hi*lo, hi*hi (small terms first).
      const int zA = (rowA >> 1) & 7, zB = (rowB >> 1) & 7;
      unsigned oA3 = (unsigned)(rowA * 128) + (unsigned)(((2 * lh) ^ zA) << 4);
      unsigned oB3 = (unsigned)(BCH * 128 + rowB * 128) + (unsigned)(((2 * lh) ^ zB) << 4);
      const char* sb = ldsc;
      // whole 16-byte chunks (conflict-free ds_read_b128), hi / lo halves regrouped in registers: 8-byte reads of the halves are two-way
      // bank conflicted and twice as many
      auto rdp = [&](unsigned off, uint4& hi, uint4& lo) {
        const uint4 c0 = *reinterpret_cast<const uint4*>(sb + off), c1 = *reinterpret_cast<const uint4*>(sb + (off ^ 16u));
        hi = make_uint4(c0.x, c0.y, c1.x, c1.y);
        lo = make_uint4(c0.z, c0.w, c1.z, c1.w);
      };
      const int KTM = BIG ? KTk : KTT;         // 256 x 256: the residual steps follow in their block-diagonal form
      for (int kt = 0; kt < KTM; ++kt) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        RGBM_BARRIER();
        asm volatile("" : "+v"(oA3), "+v"(oB3));
        sb = ldsc + st * (STAGE * 16);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          uint4 Bh[FB], Bl[FB], Al, Ah, Aln, Ahn;
          const unsigned ob = oB3 ^ ((unsigned)s << 6), oa = oA3 ^ ((unsigned)s << 6);
#pragma unroll
          for (int b = 0; b < FB; ++b) rdp(ob + b * 4096, Bh[b], Bl[b]);
          rdp(oa, Ah, Al);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int a = 0; a < FA; ++a) {
            if (a + 1 < FA) rdp(oa + (a + 1) * 4096, Ahn, Aln);      // the next fragment's operands fly under these six MFMAs
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int b = 0; b < FB; ++b) Mma32<unsigned short>::run(Al, Bh[b], acc[a][b]);
#pragma unroll
            for (int b = 0; b < FB; ++b) Mma32<unsigned short>::run(Ah, Bl[b], acc[a][b]);
#pragma unroll
            for (int b = 0; b < FB; ++b) Mma32<unsigned short>::run(Ah, Bh[b], acc[a][b]);
            __builtin_amdgcn_sched_barrier(0);
            if (a + 1 < FA) { Al = Aln; Ah = Ahn; }
          }
        }
        st = st == NST - 1 ? 0 : st + 1;
      }
      if constexpr (BIG) {
        if (KR) {
          // residual step r: channels 32 r .. 32 r + 31 of the tile = one fragment of the waves that own them; the identity's
          // lo half is zero, so of the three products lo*hi vanishes: hi*lo (the residual's lo halves), then hi*hi
#pragma unroll
          for (int r = 0; r < BCH / BK; ++r) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            RGBM_BARRIER();
            if (wch == ((32 * r) / WCHW) * WCHW) {
              asm volatile("" : "+v"(oB3));
              sb = ldsc + st * (STAGE * 16);
#pragma unroll
              for (int s2 = 0; s2 < 2; ++s2) {
                uint4 Bh[FB], Bl[FB];
                const unsigned ob = oB3 ^ ((unsigned)s2 << 6);
#pragma unroll
                for (int b = 0; b < FB; ++b) rdp(ob + b * 4096, Bh[b], Bl[b]);
                const uint4 Aid = ident_frag(s2);
#pragma unroll
                for (int b = 0; b < FB; ++b) Mma32<unsigned short>::run(Aid, Bl[b], acc[((32 * r) % WCHW) / 32][b]);
#pragma unroll
                for (int b = 0; b < FB; ++b) Mma32<unsigned short>::run(Aid, Bh[b], acc[((32 * r) % WCHW) / 32][b]);
              }
            }
            st ^= 1;
          }
        }
      }
    } else if constexpr (BIG) {
      // Two multiply waves per SIMD cover each other's waits; within a wave the next step's fragments are requested as their registers
      // fall free: A[a] right behind the two MFMAs that read it, the B pair into a second set (8 registers) at the head of the step.
      // Only the first step of a K tile, behind the barrier, waits for all six reads.
      uint4 A[FA], B[FB], Bn[FB];
      unsigned oA = offA, oB = offB;
      auto ldB = [&](int s, uint4 (&bf)[FB]) {
#pragma unroll
        for (int b = 0; b < FB; ++b) bf[b] = *reinterpret_cast<const uint4*>(ldsc + st * (STAGE * 16) + (oB ^ ((unsigned)s << 5)) + b * 4096);
      };
      // Round 6, the K-tile barrier moved one sub-step EARLY (M32_SHIFT): behind a barrier both multiply waves of a SIMD wait for their first six
      // fragment reads at the same time - nothing covers that round trip, once per K tile.  A wave's reads of a K tile are all issued by the end
      // of its third sub-step (the fourth's fragments are requested as the third's MFMAs free their registers), so the barrier that says "the NEXT
      // K tile has landed and this one's stage may be refilled" can be passed in front of the fourth sub-step: its MFMAs then cover the first
      // reads of the next K tile, which start from registers.  The request waves see the same barrier sequence with the same meaning.  Not
      // across a tile's last K step: the epilogue stages the output in that step's ring stage, which must not be handed back before it.
      auto ldAs = [&](int stg, int s, int a) { A[a] = *reinterpret_cast<const uint4*>(ldsc + stg * (STAGE * 16) + (oA ^ ((unsigned)s << 5)) + a * 4096); };
      auto ldBs = [&](int stg, int s, uint4 (&bf)[FB]) {
#pragma unroll
        for (int b = 0; b < FB; ++b) bf[b] = *reinterpret_cast<const uint4*>(ldsc + stg * (STAGE * 16) + (oB ^ ((unsigned)s << 5)) + b * 4096);
      };
      auto first3 = [&]() {          // sub-steps 0 .. 2 of the K tile in stage st (their fragments, and sub-step 3's, are read from it)
#pragma unroll
        for (int s = 0; s < 3; ++s) {
          ldBs(st, s + 1, Bn);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int a = 0; a < FA; ++a) {
            Mma32<T>::run(A[a], B[0], acc[a][0]);
            Mma32<T>::run(A[a], B[1], acc[a][1]);
            __builtin_amdgcn_sched_barrier(0);
            ldAs(st, s + 1, a);
            __builtin_amdgcn_sched_barrier(0);
          }
          B[0] = Bn[0]; B[1] = Bn[1];
        }
      };
      // the tile's first K tile: barrier, then its first fragments (the one uncovered LDS round trip of the tile)
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      RGBM_BARRIER();
      // the step offsets (o ^ 32 s) are recomputed per K tile, two VALU each: kept across the loop as eight registers, one of them
      // lived in scratch and its reload (s_waitcnt vmcnt(0) behind the first MFMA) stalled every K tile
      asm volatile("" : "+v"(oA), "+v"(oB));
      ldBs(st, 0, B);
#pragma unroll
      for (int a = 0; a < FA; ++a) ldAs(st, 0, a);
      __builtin_amdgcn_sched_barrier(0);
      for (int kt = 0; kt + 1 < KTk; ++kt) {
        first3();
        if (M32_SHIFT) {
          // every read of this K tile's stage has been issued: wait for them, meet, and go on into the next K tile's stage
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          RGBM_BARRIER();
          asm volatile("" : "+v"(oA), "+v"(oB));
          ldBs(st ^ 1, 0, Bn);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int a = 0; a < FA; ++a) {
            Mma32<T>::run(A[a], B[0], acc[a][0]);
            Mma32<T>::run(A[a], B[1], acc[a][1]);
            __builtin_amdgcn_sched_barrier(0);
            ldAs(st ^ 1, 0, a);
            __builtin_amdgcn_sched_barrier(0);
          }
          B[0] = Bn[0]; B[1] = Bn[1];
        } else {
#pragma unroll
          for (int a = 0; a < FA; ++a) {
            Mma32<T>::run(A[a], B[0], acc[a][0]);
            Mma32<T>::run(A[a], B[1], acc[a][1]);
            __builtin_amdgcn_sched_barrier(0);
          }
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          RGBM_BARRIER();
          asm volatile("" : "+v"(oA), "+v"(oB));
          ldBs(st ^ 1, 0, B);
#pragma unroll
          for (int a = 0; a < FA; ++a) ldAs(st ^ 1, 0, a);
          __builtin_amdgcn_sched_barrier(0);
        }
        st ^= 1;
      }
      // the tile's last K tile: no early barrier (the epilogue, or the residual steps, follow in this stage)
      first3();
#if M32_RACE_PROBE
      if (wave == 5 && !KR) { for (int q = 0; q < 32; ++q) __builtin_amdgcn_s_sleep(2); }
#endif
#pragma unroll
      for (int a = 0; a < FA; ++a) {
        Mma32<T>::run(A[a], B[0], acc[a][0]);
        Mma32<T>::run(A[a], B[1], acc[a][1]);
        __builtin_amdgcn_sched_barrier(0);
      }
      st ^= 1;
      if (KR) {
        // residual step r: channels 64 r .. 64 r + 63 of the tile; sub-step s (16 channels from 64 r + 16 s) belongs to one fragment of the
        // waves that own those channels
#pragma unroll
        for (int r = 0; r < BCH / BK; ++r) {
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          RGBM_BARRIER();
#if M32_RACE_PROBE
          if (wave == 5 && r == BCH / BK - 1) { for (int q = 0; q < 32; ++q) __builtin_amdgcn_s_sleep(2); }
#endif
          asm volatile("" : "+v"(oB));
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            if (wch == ((64 * r + 16 * s) / WCHW) * WCHW) {      // wave-uniform
              ldB(s, B);
              const uint4 Aid = ident_frag(s & 1);
              Mma32<T>::run(Aid, B[0], acc[((64 * r + 16 * s) % WCHW) / 32][0]);
              Mma32<T>::run(Aid, B[1], acc[((64 * r + 16 * s) % WCHW) / 32][1]);
            }
          }
          st ^= 1;
        }
      }
    } else {
      // 16-bit types, 128-pixel tiles: fragment reads one 16-deep step ahead of the MFMAs, in two register sets
      auto load_step = [&](int st, int s, uint4 (&af)[FA], uint4 (&bf)[FB]) {
        const char* base = ldsc + st * (STAGE * 16);
        const unsigned oa = offA ^ ((unsigned)s << 5), ob = offB ^ ((unsigned)s << 5);
#pragma unroll
        for (int b = 0; b < FB; ++b) bf[b] = *reinterpret_cast<const uint4*>(base + ob + b * 4096);
#pragma unroll
        for (int a = 0; a < FA; ++a) af[a] = *reinterpret_cast<const uint4*>(base + oa + a * 4096);
      };
      auto mma_step = [&](const uint4 (&af)[FA], const uint4 (&bf)[FB]) {
#pragma unroll
        for (int a = 0; a < FA; ++a)
#pragma unroll
          for (int b = 0; b < FB; ++b) {
            Mma32<T>::run(af[a], bf[b], acc[a][b]);
          }
      };
      uint4 A0[FA], B0[FB], A1[FA], B1[FB];
      for (int kt = 0; kt < KTT; ++kt) {
        // every fragment read of the previous step has returned before the request waves may refill its stage
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        RGBM_BARRIER();
        load_step(st, 0, A0, B0);
        __builtin_amdgcn_sched_barrier(0);
        if (kt > 0) mma_step(A1, B1);                    // last step of K tile kt-1
        __builtin_amdgcn_sched_barrier(0);
        load_step(st, 1, A1, B1);
        __builtin_amdgcn_sched_barrier(0);
        mma_step(A0, B0);
        __builtin_amdgcn_sched_barrier(0);
        load_step(st, 2, A0, B0);
        __builtin_amdgcn_sched_barrier(0);
        mma_step(A1, B1);
        __builtin_amdgcn_sched_barrier(0);
        load_step(st, 3, A1, B1);
        __builtin_amdgcn_sched_barrier(0);
        mma_step(A0, B0);
        __builtin_amdgcn_sched_barrier(0);
        st = st == 2 ? 0 : st + 1;
      }
      mma_step(A1, B1);
    }

    // ---- epilogue of tile k (the request waves are already filling the ring for tile k+1) ----
    if constexpr (STAGED) {
      // The output tile is staged in the ring stage the LAST K step was read from (store_round): the eight 8 KB regions cover that whole
      // stage, so a wave's staging writes land on rows another multiply wave may still be reading for that step.  One workgroup barrier
      // per tile between the two (the request waves count it too): every wave's last fragment reads have returned before any staging write.
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      RGBM_BARRIER();
    }
    if constexpr (KSPLIT) {
      if (nsp > 1) {
        // K split: this wave's accumulators go to the scratch slot of (tile, part, wave) — lane-linear 16-byte pieces — and the wave counts
        // itself in.  The wave that finds the other nsp - 1 parts counted adds ALL parts in ascending order from the scratch (its own too:
        // one order whoever arrives last) and goes on into the epilogue; the others are done.  The counter is left at zero for the next
        // launch on this stream.  The parts of a tile run on any XCD, and the XCDs' L2s are not coherent with each other: the partial sums
        // are written and read with device-scope (sc1) accesses — written through to, and read at, the coherence point — between a
        // s_waitcnt vmcnt(0) behind the stores and the device-scope atomic.  (First form: plain stores between two __threadfence().  Right,
        // and 0.55 ms SLOWER per B = 1 forward: an agent-scope acquire invalidates the XCD's whole L2, 208 times per launch, under the
        // workgroups that are still streaming weights through it.)
        constexpr int WFL = FA * FB * 64 * 16;                // floats of one wave's accumulators
        float* sc = d.kscratch + (((long long)vtile * nsp + part) * NMW + wave) * WFL;
#pragma unroll
        for (int a = 0; a < FA; ++a)
#pragma unroll
          for (int b = 0; b < FB; ++b)
#pragma unroll
            for (int q = 0; q < 4; ++q)
            {
              const f32x4 v = f32x4{acc[a][b][4 * q], acc[a][b][4 * q + 1], acc[a][b][4 * q + 2], acc[a][b][4 * q + 3]};
              asm volatile("global_store_dwordx4 %0, %1, off sc1" :: "v"(sc + (((a * FB + b) * 4 + q) * 64 + lane) * 4), "v"(v) : "memory");
            }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        unsigned arrived = 0;
        if (lane == 0) arrived = __hip_atomic_fetch_add(d.kcount + (long long)vtile * NMW + wave, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        arrived = (unsigned)__builtin_amdgcn_readfirstlane((int)arrived);
        if (arrived != (unsigned)(nsp - 1)) continue;         // (n_my = 1: the wave is done)
#pragma unroll
        for (int a = 0; a < FA; ++a)
#pragma unroll
          for (int b = 0; b < FB; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;
        for (int p = 0; p < nsp; ++p) {
          const float* sp = d.kscratch + (((long long)vtile * nsp + p) * NMW + wave) * WFL;
          f32x4 t[FA * FB * 4];                            // a part's pieces all in flight, one wait
#pragma unroll
          for (int i = 0; i < FA * FB * 4; ++i)
            asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=v"(t[i]) : "v"(sp + (i * 64 + lane) * 4) : "memory");
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
          for (int i = 0; i < FA * FB * 4; ++i) asm volatile("" : "+v"(t[i]));      // (read behind the wait)
#pragma unroll
          for (int a = 0; a < FA; ++a)
#pragma unroll
            for (int b = 0; b < FB; ++b)
#pragma unroll
              for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[a][b][4 * q + e] += t[(a * FB + b) * 4 + q][e];
        }
        if (lane == 0) __hip_atomic_store(d.kcount + (long long)vtile * NMW + wave, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    int pix_tile, ch_tile;
    tile_of(k, pix_tile, ch_tile);
    const bool interior = tile_interior(pix_tile, ch_tile);
    long long obase[FB];
    int nn[FB];
    bool pok[FB];
    const bool dense_out = d.osd == 1 && d.osh == 1 && d.osw == 1 && d.opd == 0 && d.oph == 0 && d.opw == 0 && d.Dq == d.Do &&
                           d.Hq == d.Ho && d.Wq == d.Wo;
#pragma unroll
    for (int b = 0; b < FB; ++b) {
      const long long m = d.m0 + (long long)pix_tile * BPIX + wpix + b * 32 + li;
      pok[b] = m < d.M;
      if (dense_out && (interior || d.bias_stride == 0)) {
        nn[b] = 0;
        obase[b] = (pok[b] ? m : 0ll) * d.ldo;
        continue;
      }
      unsigned n, qd, qh, qw;
      decode_row(d, pok[b] ? (unsigned)m : 0u, n, qd, qh, qw);
      nn[b] = (int)n;
      obase[b] = ((((long long)n * d.Do + (qd * d.osd + d.opd)) * d.Ho + (qh * d.osh + d.oph)) * d.Wo + (qw * d.osw + d.opw)) * d.ldo;
    }
    constexpr int CHK = 16 / (int)sizeof(T);             // channels per 16-byte chunk
    constexpr int NQ = 16 / CHK;                         // chunks per lane, pixel and channel fragment
    if (interior) {
      const float nslope = d.act == ACT_RELU ? 0.f : d.act == ACT_PRELU ? d.slope : 1.f;
      // One sweep over the 8 fragments turns accumulators (+ residual) into packed 16-byte chunks — a fragment's 16 accumulators die
      // as its two chunks are made, and every residual read is issued before the first output store (a load behind a store in the
      // in-order vmcnt queue waits for the store's round trip) — then the chunks are stored.
      // Fragments in the order i = b*4 + a (pixel half outer).  Residual reads run two fragments ahead of their use, and the second
      // half's last reads are issued BEFORE the first half's stores: a load behind a store in the in-order vmcnt queue waits for the
      // store's round trip.  A fragment's 16 accumulators die as its two chunks are packed.  Every stage is fenced: hipcc otherwise
      // hoists all 16 reads to the front and spills what they deliver.
      auto fast = [&](auto resc) {
        constexpr int RES = decltype(resc)::value;
        constexpr int NF = FA * FB;
        constexpr int AR = FA < (X3 ? 2 : 4) ? FA : (X3 ? 2 : 4);      // channel fragments per store round: 64 channels of split pairs or 128 of 16-bit values = a 256-byte row
        static_assert(FA % AR == 0, "whole store rounds");
        uint4 pk[AR][NQ];          // one store round at a time
        uint4 rr[4][NQ];
        // interior tiles of a dense output: wave-uniform 64-bit bases (scalar registers) + ONE 32-bit lane offset per access pattern
        // (as per-lane 64-bit addresses hipcc hoisted sixteen of them out of the tile loop and spilled them around the K loop)
        const long long mrow = d.m0 + (long long)pix_tile * BPIX + wpix;                     // first pixel of this wave
        const int ch0 = ch_tile * BCH + wch;                                                  // first channel of this wave
        unsigned lofs_c = (unsigned)((li * d.ldo + lh * 16) * (int)sizeof(T));                // C layout: pixel li, 16 channels of half lh
        asm volatile("" : "+v"(lofs_c));                                                      // not loop-invariant for hipcc: nothing derived from it is hoisted
        auto rd = [&](int i) {
          const int b = i / FA, a = i % FA;
          const char* ub = reinterpret_cast<const char*>(res + (mrow + b * 32) * d.ldo + ch0 + a * 32);
#pragma unroll
          for (int q = 0; q < NQ; ++q) rr[i & 3][q] = *reinterpret_cast<const uint4*>(ub + lofs_c + q * 16);
        };
        auto make = [&](int i) {
          const int b = i / FA, a = i % FA;
#pragma unroll
          for (int q = 0; q < NQ; ++q) {
            float v[CHK], rv[CHK];
#pragma unroll
            for (int e = 0; e < CHK; ++e) v[e] = acc[a][b][q * CHK + e];
            if (RES != RES_NONE) unpack_chunk(rr[i & 3][q], rv, T());
            if (RES == RES_PRE_ACT) {
#pragma unroll
              for (int e = 0; e < CHK; ++e) v[e] += rv[e];
            }
#pragma unroll
            for (int e = 0; e < CHK; ++e) v[e] = v[e] < 0.f ? __builtin_fmaxf(v[e], -3.402823466e38f) * nslope : v[e];
            if (RES == RES_POST_ACT) {
#pragma unroll
              for (int e = 0; e < CHK; ++e) v[e] += rv[e];
            }
            pk[a % AR][q] = pack_chunk(v, T());
          }
        };
        auto store_round = [&](int b, int ar) {
          if constexpr (STAGED) {
            // Whole lines out: written from the C layout a store instruction touches 64 lines with 16 bytes each (measured: 315 of
            // 2890 cycles per K step of a 36-K-tile layer, 190 of them gone with whole lines).  The stage the last K tile was read
            // from is free until this wave passes the next barrier: 8 KB of it per wave hold 32 pixels x 128 channels as 256-byte
            // rows (chunk position ^ row: conflict-free both ways), read back as 16 lanes per pixel, 4 pixels = 1 KB per store
            // instruction.  LDS executes one wave's instructions in order: no wait between a half's writes, its reads and the next
            // half's writes.
            char* stg = const_cast<char*>(ldsc) + (st ^ 1) * (STAGE * 16) + wave * 8192;
            unsigned wofs = (unsigned)(li * 256 + (((lh * NQ) ^ (li & 15)) << 4));            // chunk (a*2*NQ + lh*NQ + q) ^ (li & 15) = this ^ (a*2*NQ + q)
            unsigned rofs = (unsigned)((lane >> 4) * 256 + (((lane & 15) ^ (lane >> 4)) << 4));   // row 4t + (lane>>4): its low 4 bits = (lane>>4) ^ 4t... see below
            unsigned gofs = (unsigned)(((lane >> 4) * d.ldo + (lane & 15) * CHK) * (int)sizeof(T));
            asm volatile("" : "+v"(wofs), "+v"(rofs), "+v"(gofs));
#pragma unroll
            for (int a = 0; a < AR; ++a)
#pragma unroll
              for (int q = 0; q < NQ; ++q)
                *reinterpret_cast<uint4*>(stg + (wofs ^ (unsigned)((a * 2 * NQ + q) << 4))) = pk[a][q];
            if (bm) {
              // border-class tiles: staging row 4t + (lane>>4) of this half is table row wpix + 32 b + 4t + (lane>>4) of the tile, whose
              // GEMM row the request waves left in LDS (enter_tile); a dead row is not stored
              const int* lrow = reinterpret_cast<const int*>(lbias + 2560) + (k & 1) * 256 + wpix + b * 32 + (lane >> 4);
              char* oc = reinterpret_cast<char*>(out + ch0 + ar * AR * 32) + (lane & 15) * 16;
#pragma unroll
              for (int t = 0; t < 8; ++t) {
                const int m = lrow[4 * t];
                const uint4 v = *reinterpret_cast<const uint4*>(stg + t * 1024 + (rofs ^ (unsigned)(((4 * t) & 15) << 4)));
                if (m >= 0) *reinterpret_cast<uint4*>(oc + (long long)m * d.ldo * (long long)sizeof(T)) = v;
              }
              return;
            }
            char* ob = reinterpret_cast<char*>(out + (mrow + b * 32) * d.ldo + ch0 + ar * AR * 32);
#pragma unroll
            for (int t = 0; t < 8; ++t) {
              // row p = 4t + (lane>>4); p & 15 = (4t & 15) | (lane>>4), so the chunk position is (lane&15) ^ (lane>>4) ^ (4t & 15)
              const uint4 v = *reinterpret_cast<const uint4*>(stg + t * 1024 + (rofs ^ (unsigned)(((4 * t) & 15) << 4)));
              *reinterpret_cast<uint4*>(ob + (long long)(4 * t) * d.ldo * (long long)sizeof(T) + gofs) = v;
            }
          } else {
#pragma unroll
            for (int a = 0; a < AR; ++a)
#pragma unroll
              for (int q = 0; q < NQ; ++q)
                *reinterpret_cast<uint4*>(reinterpret_cast<char*>(out + (mrow + b * 32) * d.ldo + ch0 + (ar * AR + a) * 32) + lofs_c + q * 16) = pk[a][q];
          }
        };
        if (RES != RES_NONE) { rd(0); rd(1); __builtin_amdgcn_sched_barrier(0); }
#pragma unroll
        for (int i = 0; i < NF; ++i) {
          make(i);
          __builtin_amdgcn_sched_barrier(0);
          if (RES != RES_NONE) {
            if (i < FA - 1) rd(i + 2);
            else if (i == FA - 1) {                               // the rest of the second half: all reads precede the first half's stores
#pragma unroll
              for (int k = FA + 1; k < NF; ++k) rd(k);
            }
            __builtin_amdgcn_sched_barrier(0);
          }
          if (i % AR == AR - 1) { store_round(i / FA, (i % FA) / AR); __builtin_amdgcn_sched_barrier(0); }
        }
      };
      if (BIG || res_in_acc) fast(IC<RES_NONE>{});      // a pre-activation residual has been added by KR extra K steps (identity weights): see the request waves
      else if (d.res_mode == RES_NONE) fast(IC<RES_NONE>{});
      else if (d.res_mode == RES_PRE_ACT) fast(IC<RES_PRE_ACT>{});
      else fast(IC<RES_POST_ACT>{});
      continue;
    }
    if constexpr (BIG) continue;      // launch_m32 gives this kernel whole interior tiles only (the generic epilogue's registers would spill accumulators)
#pragma unroll
    for (int a = 0; a < FA; ++a) {
      const int chL = ch_tile * BCH + wch + a * 32 + lh * 16;
#pragma unroll
      for (int b = 0; b < FB; ++b) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          const int c = chL + q * CHK;
          if (!pok[b] || c >= d.Cout) continue;
          const bool whole = c + CHK <= d.Cout;          // Cout is a multiple of 4: a 16-bit tail chunk holds 4 channels
          float v[CHK], rv[CHK];
#pragma unroll
          for (int e = 0; e < CHK; ++e) v[e] = acc[a][b][q * CHK + e];
          if (d.bias) {
            const float* bp = d.bias + (long long)nn[b] * d.bias_stride + c;
#pragma unroll
            for (int e = 0; e < CHK; ++e) if (e < 4 || whole) v[e] += bp[e];
          }
#pragma unroll
          for (int e = 0; e < CHK; ++e) rv[e] = 0.f;
          if (d.res_mode != RES_NONE && !res_in_acc) {
            if (whole) unpack_chunk(*reinterpret_cast<const uint4*>(res + obase[b] + c), rv, T());
            else load4(res + obase[b] + c, rv);
          }
          if (d.res_mode == RES_PRE_ACT && !res_in_acc) {
#pragma unroll
            for (int e = 0; e < CHK; ++e) v[e] += rv[e];
          }
#pragma unroll
          for (int e = 0; e < CHK; ++e) v[e] = apply_act_g(v[e], d.act, d.slope);
          if (d.res_mode == RES_POST_ACT) {
#pragma unroll
            for (int e = 0; e < CHK; ++e) v[e] += rv[e];
          }
          if (whole) *reinterpret_cast<uint4*>(out + obase[b] + c) = pack_chunk(v, T());
          else store4(out + obase[b] + c, v);
        }
      }
    }
  }
}

static std::atomic<long long> g_border_launches{0};
long long border_launch_count() { return g_border_launches.load(std::memory_order_relaxed); }

// GEMM rows [d.m0, d.M) on tiles of BCH channels x BPIX pixels
template <typename T, int BPIX, int BCH = 256>
static int launch_m32_range(ConvDesc d, hipStream_t s) {
  constexpr int NST = BPIX == 256 ? 2 : 3;
  // K-tile ring + bias table (up_1's stacked taps: 2304 channels) + 256 x 256: the GEMM rows of two border-class tiles
  constexpr size_t LDS = ((size_t)NST * (BCH + BPIX) * 8) * sizeof(uint4) + 2560 * sizeof(float) + (BPIX == 256 && BCH == 256 ? 2 * 256 * sizeof(int) : 0);
  d.n_pix_tiles = (int)((d.M - d.m0 + BPIX - 1) / BPIX);
  d.n_ch_tiles = (d.Cout + BCH - 1) / BCH;
  const long long ntiles = (long long)d.n_pix_tiles * d.n_ch_tiles;
  RGBM_REQUIRE(ntiles > 0 && ntiles < (1ll << 31) && d.M < (1ll << 31), "conv grid out of range");
  d.n_tiles = (int)ntiles;
  fill_fastdiv(d);
  if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(conv_igemm_m32_kernel<T, BPIX, BCH>), (int)LDS)) return rc;
  int n_cu = 0;
  if (int rc = persistent_grid_cus(&n_cu)) return rc;
  RGBM_REQUIRE(d.ksplit <= 1 || (BPIX == 128 && BCH <= 128 && ntiles * d.ksplit <= 4096 && d.kscratch && d.kcount), "K split: 64 / 128-channel x 128-pixel tiles, one workgroup per (tile, part)");
  const int grid = d.ksplit > 1 ? (int)(ntiles * d.ksplit) : ntiles < n_cu ? (int)ntiles : n_cu;
  RGBM_REQUIRE(d.btab == nullptr || (BPIX == 256 && BCH == 256 && d.m0 == 0 && grid == d.b_nwg), "border-class table: made for another grid");
  if (d.btab) g_border_launches.fetch_add(1, std::memory_order_relaxed);
  // profiler rows: 31 / 33 = the 256 x 256 launches (the roofline kernel), 40 / 41 = every other tile of this kernel
  prof_begin_launch(s, BPIX == 256 && BCH == 256 ? (std::is_same<T, bx3_t>::value ? 33 : 31) : (std::is_same<T, bx3_t>::value ? 41 : 40), d.algo_flops, d.algo_bytes);
  hipLaunchKernelGGL((conv_igemm_m32_kernel<T, BPIX, BCH>), dim3((unsigned)grid), dim3(BPIX == 256 ? 768 : 512), LDS, s, d);
  prof_end_launch(s);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

template <typename T>
static int launch_m32_tiles128(const ConvDesc& d, int bch, hipStream_t s) {
  return bch == 64 ? launch_m32_range<T, 128, 64>(d, s) : bch == 128 ? launch_m32_range<T, 128, 128>(d, s) : launch_m32_range<T, 128, 256>(d, s);
}

// CONV_M32_SMALL: every row on bch x 128 tiles (d.ksplit parts of each tile's K loop where the layer bound the stream's scratch)
template <typename T>
static int launch_m32_small(const ConvDesc& d, const ConvPlan& p, hipStream_t s) {
  return launch_m32_tiles128<T>(d, p.bch, s);
}

// CONV_M32: rows [0, main_rows) on 256 x 256 tiles (on border-class tiles where the layer bound their table, d.btab: conv_plan.h), the
// rest on tail_bch x 128 tiles in a second launch
template <typename T>
static int launch_m32(ConvDesc d, const ConvPlan& p, hipStream_t s) {
  if (p.main_rows > 0) {
    ConvDesc m = d;
    m.M = p.main_rows;
    const double frac = (double)m.M / (double)d.M;
    m.algo_flops = d.algo_flops * frac; m.algo_bytes = d.algo_bytes * frac;
    if (int rc = launch_m32_range<T, 256, 256>(m, s)) return rc;
    d.m0 = m.M;
    d.algo_flops *= 1.0 - frac; d.algo_bytes *= 1.0 - frac;
  }
  d.btab = nullptr;
  return p.tail_bch ? launch_m32_tiles128<T>(d, p.tail_bch, s) : 0;
}

// CONV_M32 / CONV_M32_SMALL (16-bit storage types and split pairs)
int launch_igemm_m32(const ConvDesc& d, int dtype, const ConvPlan& p, hipStream_t s) {
  const bool small = p.kernel == CONV_M32_SMALL;
  if (dtype == BF16) return small ? launch_m32_small<unsigned short>(d, p, s) : launch_m32<unsigned short>(d, p, s);
  if (dtype == F16) return small ? launch_m32_small<f16_t>(d, p, s) : launch_m32<f16_t>(d, p, s);
  if (dtype == BF16X3) return small ? launch_m32_small<bx3_t>(d, p, s) : launch_m32<bx3_t>(d, p, s);
  return conv_no_kernel();
}

}  // namespace rgbm
