// Implicit-GEMM convolution, 64-channel three-role tile (gfx950): conv_igemm_ws64_kernel, 16-bit storage types.
// Shared pieces: igemm_device.h.
#include "igemm_device.h"

namespace rgbm {

// ---------------------------------------------------------------------------------------------------------
// 256 pixel x 64 channel tile, bf16, three roles (layers with 33..64 output channels and no residual: up_2, up_3).
// These layers have short K (9..36 K tiles) and 6.6 GB of activations per launch: with the 2-stage kernel the epilogue
// (8-byte stores from the MFMA C layout) and the pipeline refill of every tile left them at 0.43 PFLOP/s / 1.5 TB/s.
//   waves 0-3  multiply: ds_read + MFMA only; at the end of a tile bias + activation + bf16 pack -> LDS staging tile
//   waves 4-7  request : tap walk, validity masks, 10 LDS-DMA pieces per K tile, counted vmcnt (loads only: stores
//                        share vmcnt on gfx9 and complete out of order, so they must not come from these waves)
//   waves 8-11 store   : move the staged tile of the PREVIOUS pixel tile to global memory as whole 128-byte rows, a slice
//                        per K step, while the multiply waves are already deep in the next tile
// Persistent over tiles with one continuous 3-stage K ring, one barrier per K step for all 12 waves plus one final
// barrier that publishes the last staged tile.
// ---------------------------------------------------------------------------------------------------------
//
// RH (row halo; 3x3, stride 1, pad = dilation <= 4, Cin a multiple of 64): a K step is one kernel ROW (kh) of one 64-channel
// input chunk.  The 3 kw taps of that row read the same pixels shifted by 0, dil, 2*dil GEMM rows, so ONE X stage of
// 256 + 2*dil rows serves all three (the multiply waves read their B fragments at row offsets kw*dil; lanes whose
// neighbour falls off the image row read a zero row instead), with the 3 x 64 weight rows of that kernel row beside it.
// Per tile the L2->LDS traffic drops 2.1x (3 x 57 KB instead of 9 x 40 KB for Cin = 64) and the barriers 3x; a step holds
// 96 MFMAs per wave.  Two 57 KB stages (plain double buffering) + the staging tile fit the 160 KB LDS.
template <bool RH, typename T>      // T: unsigned short (bf16) or f16_t
__global__ __launch_bounds__(768) void conv_igemm_ws64_kernel(const ConvDesc d) {
  constexpr int BCH = 64, BPIX = 256;
  constexpr int E = 8, BK = 64;
  constexpr int XR = BPIX / 32;              // 8 gathered rows per request thread
  constexpr int WL = BCH / 32;               // 2 weight rows per request thread
  constexpr int NP = XR + WL;                // 10 pieces per request wave and K tile
  constexpr int FM = 4, FN = 4;
  constexpr int HXROWS = 264;                // RH: X rows per stage (256 + 2*dil, padded to whole 8-row pieces)
  constexpr int HWROWS = 3 * BCH;            // RH: weight rows per stage (kw-major)
  constexpr int NST = RH ? 2 : 3;            // ring depth
  constexpr int STAGE = RH ? (HWROWS + HXROWS) * 8 : (BCH + BPIX) * 8;    // uint4 slots per stage (57 KB / 40 KB)
  constexpr int SROW = 144;                  // bytes per staged pixel row (128 + 16 pad)
  extern __shared__ __attribute__((aligned(16))) uint4 lds3[];
  const uint4* zrow = lds3 + NST * STAGE;    // RH: 8 slots (one row) of zeros
  unsigned char* stg = reinterpret_cast<unsigned char*>(lds3 + NST * STAGE + (RH ? 8 : 0));
  static_assert(NP == 10, "the counted waits below assume 10 pieces per tile");

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int NCC = d.Cin >> 6;                // RH: 64-channel input chunks
  const int KT = RH ? 3 * NCC : d.KT;        // K steps per tile
  if (RH && tid < 8) lds3[NST * STAGE + tid] = make_uint4(0u, 0u, 0u, 0u);      // visible after the first barrier
  // per-channel bias (zeros if there is none) as an LDS table behind the staging tile: the accumulators start from it, so the
  // multiply waves issue no global load — and wait on no vmcnt — anywhere (see conv_igemm_ws_kernel)
  float* lbias = reinterpret_cast<float*>(stg + BPIX * SROW);
  const bool bias_lds = d.bias == nullptr || d.bias_stride == 0;
  if (tid < BCH) lbias[tid] = (d.bias && bias_lds && tid < d.Cout) ? d.bias[tid] : 0.f;
  __syncthreads();
  const int n_my = ((int)d.n_tiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
  const int total = n_my * KT;               // every wave passes total + 1 barriers
  auto tile_of = [&](int k) {
    const int v = (int)blockIdx.x + k * (int)gridDim.x;
    const int nblk = d.n_tiles, bq = nblk >> 3, br = nblk & 7, xcd = v & 7, bidx = v >> 3;
    return (xcd < br ? xcd * (bq + 1) : br * (bq + 1) + (xcd - br) * bq) + bidx;      // pixel tile (one channel tile)
  };

  if (wave >= 8) {
    // ------------------------------------------------------------------ store waves
    const int ts = tid - 512;
    const int c = ts & 7;                     // 16-byte chunk = 8 channels
    const int r0 = ts >> 3;                   // rows r0 + 32*i
    T* __restrict__ out = reinterpret_cast<T*>(d.out);
    const int ch = c * 8;
    const int nch = d.Cout - ch;              // <= 0: nothing, 4: half chunk, >= 8: whole chunk
    const int per = (8 + (KT - 1) - 1) / (KT - 1);       // row groups per K step (KT >= 2)
    auto flush = [&](int k, int i0, int i1) {            // row groups [i0, i1) of tile k
      if (nch <= 0) return;
      const int pix_tile = tile_of(k);
      for (int i = i0; i < i1 && i < 8; ++i) {
        const int r = r0 + 32 * i;
        const long long m = (long long)pix_tile * BPIX + r;
        if (m >= d.M) continue;
        unsigned n, qd, qh, qw;
        decode_row(d, (unsigned)m, n, qd, qh, qw);
        const long long o = ((((long long)n * d.Do + (qd * d.osd + d.opd)) * d.Ho + (qh * d.osh + d.oph)) * d.Wo + (qw * d.osw + d.opw)) * d.ldo + ch;
        const uint4 v = *reinterpret_cast<const uint4*>(stg + r * SROW + c * 16);
        if (nch >= 8) *reinterpret_cast<uint4*>(out + o) = v;
        else *reinterpret_cast<uint2*>(out + o) = make_uint2(v.x, v.y);
      }
    };
    // Fused trailing 1x1 (y2 = act2(W2 . y + bias2), e.g. PSPNet's `final` after up_3): the staged tile already is the B
    // operand layout of an MFMA (pixel row = 64 contiguous channels), so the store waves multiply it by W2 (kept in
    // registers) and write only y2; the 64-channel tensor never reaches HBM.
    const int sw = wave - 8;
    const int lr = lane & 15, lg = lane >> 4;
    uint4 A2[2][2];
    float b2[2][4];
    if (d.w2) {
      const unsigned short* w2 = reinterpret_cast<const unsigned short*>(d.w2);
#pragma unroll
      for (int of = 0; of < 2; ++of)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          A2[of][ks] = make_uint4(0u, 0u, 0u, 0u);
          if (of * 16 < d.cout2) A2[of][ks] = *reinterpret_cast<const uint4*>(w2 + (long long)(of * 16 + lr) * d.kpad2 + ks * 32 + lg * 8);
        }
#pragma unroll
      for (int of = 0; of < 2; ++of)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c2 = of * 16 + lg * 4 + e;
          b2[of][e] = (d.bias2 && c2 < d.cout2) ? d.bias2[c2] : 0.f;
        }
    }
    const int perf = (4 + (KT - 1) - 1) / (KT - 1);       // fused: 16-pixel fragments per K step (4 per wave and tile)
    auto flush_fused = [&](int k, int j0, int j1) {
      const int pix_tile = tile_of(k);
      T* out2 = reinterpret_cast<T*>(d.out2);
      for (int j = j0; j < j1 && j < 4; ++j) {
        const int r = sw * 64 + j * 16 + lr;
        const long long m = (long long)pix_tile * BPIX + r;
        const uint4 B0 = *reinterpret_cast<const uint4*>(stg + r * SROW + lg * 16);
        const uint4 B1 = *reinterpret_cast<const uint4*>(stg + r * SROW + 64 + lg * 16);
        unsigned n, qd, qh, qw;
        decode_row(d, m < d.M ? (unsigned)m : 0u, n, qd, qh, qw);
        const long long o = ((((long long)n * d.Do + (qd * d.osd + d.opd)) * d.Ho + (qh * d.osh + d.oph)) * d.Wo + (qw * d.osw + d.opw)) * d.ldo2;
#pragma unroll
        for (int of = 0; of < 2; ++of) {
          if (of * 16 >= d.cout2) break;
          f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
          acc = MmaG<T>::run2(A2[of][0], B0, acc);
          acc = MmaG<T>::run2(A2[of][1], B1, acc);
          if (m < d.M) {
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = apply_act_g(acc[e] + b2[of][e], d.act2, d.slope2);
            store4(out2 + o + of * 16 + lg * 4, v);
          }
        }
      }
    };
    int g = 0;
    for (int k = 0; k < n_my; ++k)
      for (int kt = 0; kt < KT; ++kt, ++g) {
        RGBM_BARRIER();
        // the staged tile k-1 was published by barrier (k, 0); it must be drained before barrier (k, KT-1), after which
        // the multiply waves overwrite it
        if (k > 0 && kt < KT - 1) {
          if (d.w2) flush_fused(k - 1, kt * perf, (kt + 1) * perf);
          else flush(k - 1, kt * per, (kt + 1) * per);
        }
      }
    RGBM_BARRIER();             // publishes the last staged tile
    if (d.w2) flush_fused(n_my - 1, 0, 4);
    else flush(n_my - 1, 0, 8);
    return;
  }

  if (wave >= 4) {
    // ------------------------------------------------------------------ request waves
    if constexpr (RH) {
      const T* __restrict__ in = reinterpret_cast<const T*>(d.in);
      const T* __restrict__ wgt = reinterpret_cast<const T*>(d.wgt);
      const int pw = wave - 4;
      const int j = lane & 7, r8 = lane >> 3;
      const int dil = d.dilw;
      constexpr int NXP = HXROWS / 8;                      // 33 X pieces, 24 W pieces per step, dealt round-robin to 4 waves
      constexpr int NWP = HWROWS / 8;
      constexpr int MXP = (NXP + 3) / 4, MWP = NWP / 4;    // per wave: up to 9 X pieces, 6 W pieces
      const char* xrowp[MXP];
      unsigned xmask[MXP];
      const char* wrowp[MWP];
      const char* zero = reinterpret_cast<const char*>(g_zero_page);
      const unsigned ldsb = __builtin_amdgcn_readfirstlane(lds_addr(lds3));
#pragma unroll
      for (int i = 0; i < MWP; ++i) {                      // weight row wr = kw*64 + channel: K index of step (kh, cc) = (kh*3 + kw)*Cin + cc*64
        const int wr = (pw + 4 * i) * 8 + r8;
        const int kw = wr >> 6, ch = wr & 63;
        wrowp[i] = reinterpret_cast<const char*>(wgt + (long long)ch * d.Kpad + (long long)kw * d.Cin + (j ^ ((wr >> 1) & 7)) * E);
      }
      auto enter_tile = [&](int k) {
        const long long p0 = (long long)tile_of(k) * BPIX;
#pragma unroll
        for (int i = 0; i < MXP; ++i) {
          const int xr = (pw + 4 * i) * 8 + r8;            // LDS row xr holds GEMM row m = p0 - dil + xr
          const long long m = p0 - dil + xr;
          unsigned mk = 0;
          long long pix0 = 0;
          if ((pw + 4 * i) < NXP && xr < BPIX + 2 * dil && m >= 0 && m < d.M) {
            unsigned n, qd, qh, qw;
            decode_row(d, (unsigned)m, n, qd, qh, qw);
            for (int kh = 0; kh < 3; ++kh) mk |= (unsigned)((unsigned)((int)qh + (kh - 1) * dil) < (unsigned)d.Hi) << kh;
            pix0 = ((long long)n * d.Hi + ((int)qh - dil)) * d.Wi + (int)qw;      // input pixel of kernel row 0
          }
          xmask[i] = mk;
          xrowp[i] = reinterpret_cast<const char*>(in) + (pix0 * d.Cin + (j ^ ((xr >> 1) & 7)) * E) * 2ll;
        }
      };
      int ikh = 0, icc = 0, itile = 0;
      auto issue = [&](int stage) {
        if (ikh == 0 && icc == 0) enter_tile(itile);
        const unsigned sbase = ldsb + (unsigned)stage * (STAGE * 16);
        const long long xoff = ((long long)ikh * dil * d.Wi * d.Cin + icc * 64) * 2ll;
        const long long woff = ((long long)ikh * 3 * d.Cin + icc * 64) * 2ll;
#pragma unroll
        for (int i = 0; i < MXP; ++i) {
          if (pw + 4 * i < NXP) {                          // wave-uniform
            const char* src = ((xmask[i] >> ikh) & 1u) ? xrowp[i] + xoff : zero;
            glds16(src, sbase + (HWROWS * 8 + (pw + 4 * i) * 64) * 16);
          }
        }
#pragma unroll
        for (int i = 0; i < MWP; ++i) glds16(wrowp[i] + woff, sbase + ((pw + 4 * i) * 64) * 16);
        if (++icc == NCC) { icc = 0; if (++ikh == 3) { ikh = 0; ++itile; } }
      };
      if (total > 0) issue(0);
      for (int g = 0; g < total; ++g) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // step g landed (double buffering: nothing else is in flight)
        RGBM_BARRIER();                        // ... and every wave is done with the other stage
        if (g + 1 < total) issue((g + 1) & 1);
      }
      RGBM_BARRIER();
      return;
    }
    const T* __restrict__ in = reinterpret_cast<const T*>(d.in);
    const T* __restrict__ wgt = reinterpret_cast<const T*>(d.wgt);
    const int pw = wave - 4;
    const int tp = tid - 256;
    const int j = tp & 7;
    const int r0 = tp >> 3;                  // 0..31
    const int js = j ^ ((r0 >> 1) & 7);
    const char* rowp[XR];
    unsigned rmask[XR];
    const char* wrow[WL];
    const char* zero = reinterpret_cast<const char*>(g_zero_page);
    int tkd = 0, tkh = 0, tkw = 0, tc = 0;   // wave-uniform tap walker
    const unsigned lds0 = __builtin_amdgcn_readfirstlane(lds_addr(lds3 + pw * 64));

    // row descriptors: decoded once per 8-lane row group and exchanged, the next tile's behind the last request of the current
    // one (see conv_igemm_ws_kernel)
    long long mybase = 0;
    unsigned mymask = 0;
    auto prepare_tile = [&](int k) {
      const int pix_tile = tile_of(k);
      mybase = 0;
      mymask = 0;
      if (j < XR) {
        const long long m = (long long)pix_tile * BPIX + r0 + 32 * j;
        int xn = 0, xd0 = -(1 << 20), xh0 = 0, xw0 = 0;
        if (m < d.M) {
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
        const long long pix0 = ((long long)(xn + xd0) * d.Hi + xh0) * d.Wi + xw0;
        mybase = pix0 * d.Cin * (long long)sizeof(T);
      }
    };
    auto enter_tile = [&]() {
      const int grp = (tp & 63) & 56;
#pragma unroll
      for (int i = 0; i < XR; ++i) {
        const long long bb = __shfl(mybase, grp | i, 64);
        rmask[i] = (unsigned)__shfl((int)mymask, grp | i, 64);
        rowp[i] = reinterpret_cast<const char*>(in) + bb + (long long)(js * E) * (long long)sizeof(T);
      }
      tkd = tkh = tkw = tc = 0;
    };
#pragma unroll
    for (int i = 0; i < WL; ++i)              // one channel tile: the weight rows never change
      wrow[i] = reinterpret_cast<const char*>(wgt + (long long)(r0 + 32 * i) * d.Kpad + js * E);

    int ikt = 0, itile = 0;
    auto issue = [&](int stage) {
      if (ikt == 0) enter_tile();
      const unsigned sbase = lds0 + (unsigned)stage * (STAGE * 16);
      const unsigned sel = (1u << tkd) | (256u << tkh) | (65536u << tkw);
      const long long soff =
          ((long long)((tkd * d.dild * d.Hi + tkh * d.dilh) * d.Wi + tkw * d.dilw) * d.Cin + tc) * (long long)sizeof(T);
      const bool cok = tkd < d.KD && tc + js * E < d.Cin;
#pragma unroll
      for (int i = 0; i < XR; ++i) {
        const bool ok = cok && (rmask[i] & sel) == sel;
        const char* src = ok ? rowp[i] + soff : zero;
        glds16(src, sbase + (BCH * 8 + i * 256) * 16);
      }
      const long long wk = (long long)ikt * BK * (long long)sizeof(T);
#pragma unroll
      for (int i = 0; i < WL; ++i) glds16(wrow[i] + wk, sbase + (i * 256) * 16);
      tc += BK;
      if (d.lcin >= 0 && tc >= d.Cin) {
        tc = 0;
        if (++tkw == d.KW) { tkw = 0; if (++tkh == d.KH) { tkh = 0; ++tkd; } }
      }
      if (++ikt == KT) { ikt = 0; ++itile; if (itile < n_my) prepare_tile(itile); }
    };

    if (total > 0) prepare_tile(0);
    if (total > 0) issue(0);
    if (total > 1) issue(1);
    int st = 0;
    for (int g = 0; g < total; ++g) {
      if (g + 1 < total) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      RGBM_BARRIER();
      if (g + 2 < total) issue(st == 0 ? 2 : st - 1);
      st = st == 2 ? 0 : st + 1;
    }
    RGBM_BARRIER();
    return;
  }

  // -------------------------------------------------------------------- multiply waves
  const int wpix = wave * 64;
  const int lr = lane & 15, lg = lane >> 4;
  uint4 af0[FM], bf0[FN], af1[FM], bf1[FN];
  f32x4 acc[FM][FN];
  auto load_half = [&](int st, int s, uint4 (&af)[FM], uint4 (&bf)[FN]) {
    const uint4* W = lds3 + st * STAGE;
    const uint4* X = W + BCH * 8;
    const int cidx = s * 4 + lg;
#pragma unroll
    for (int a = 0; a < FM; ++a) {
      const int row = a * 16 + lr;
      af[a] = W[row * 8 + (cidx ^ ((row >> 1) & 7))];
    }
#pragma unroll
    for (int b = 0; b < FN; ++b) {
      const int row = wpix + b * 16 + lr;
      bf[b] = X[row * 8 + (cidx ^ ((row >> 1) & 7))];
    }
  };
  auto mma_half = [&](const uint4 (&af)[FM], const uint4 (&bf)[FN]) {
#pragma unroll
    for (int a = 0; a < FM; ++a)
#pragma unroll
      for (int b = 0; b < FN; ++b) MmaG<T>::run(af[a], bf[b], acc[a][b]);
  };
  int st = 0;
  for (int k = 0; k < n_my; ++k) {
#pragma unroll
    for (int a = 0; a < FM; ++a) {
      const f32x4 b4 = *reinterpret_cast<const f32x4*>(lbias + a * 16 + lg * 4);      // zeros unless bias_lds with a bias
#pragma unroll
      for (int b = 0; b < FN; ++b) acc[a][b] = b4;
    }
    if constexpr (RH) {
      // per tile: which lanes lose their left / right neighbour to the image edge (they read the zero row instead)
      const int dil = d.dilw;
      const long long p0 = (long long)tile_of(k) * BPIX;
      bool eL[FN], eR[FN];
#pragma unroll
      for (int b = 0; b < FN; ++b) {
        const long long m = p0 + wpix + b * 16 + lr;
        unsigned n, qd, qh, qw;
        decode_row(d, m < d.M ? (unsigned)m : 0u, n, qd, qh, qw);
        eL[b] = (int)qw - dil < 0;
        eR[b] = (int)qw + dil >= d.Wi;
      }
      for (int kt = 0; kt < KT; ++kt) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        RGBM_BARRIER();
        const uint4* W = lds3 + (st & 1) * STAGE;
        const uint4* X = W + HWROWS * 8;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
#pragma unroll
          for (int s2 = 0; s2 < 2; ++s2) {
            const int cidx = s2 * 4 + lg;
            uint4 af[FM], bf[FN];
#pragma unroll
            for (int a = 0; a < FM; ++a) {
              const int row = kw * 64 + a * 16 + lr;
              af[a] = W[row * 8 + (cidx ^ ((row >> 1) & 7))];
            }
#pragma unroll
            for (int b = 0; b < FN; ++b) {
              const int row = wpix + b * 16 + lr + kw * dil;
              const bool edge = kw == 0 ? eL[b] : (kw == 2 ? eR[b] : false);
              const uint4* src = edge ? zrow + cidx : X + row * 8 + (cidx ^ ((row >> 1) & 7));
              bf[b] = *src;
            }
#pragma unroll
            for (int a = 0; a < FM; ++a)
#pragma unroll
              for (int b = 0; b < FN; ++b) MmaG<T>::run(af[a], bf[b], acc[a][b]);
          }
        }
        ++st;
      }
    } else {
    for (int kt = 0; kt < KT; ++kt) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // fragment reads returned, staged tile written
      RGBM_BARRIER();
      load_half(st, 0, af0, bf0);
      __builtin_amdgcn_sched_barrier(0);
      if (kt > 0) mma_half(af1, bf1);
      __builtin_amdgcn_sched_barrier(0);
      load_half(st, 1, af1, bf1);
      __builtin_amdgcn_sched_barrier(0);
      mma_half(af0, bf0);
      __builtin_amdgcn_sched_barrier(0);
      st = st == 2 ? 0 : st + 1;
    }
    mma_half(af1, bf1);
    }
    // ---- bias + activation + bf16 pack into the staging tile (the store waves have drained the previous one) ----
    if (bias_lds && d.act != ACT_TANH) {
      // the bias is already in the accumulators; activation fixed at compile time per variant: straight-line code
      const float slope = d.slope;
      auto pack_tile = [&](auto actc) {
        constexpr int ACT = decltype(actc)::value;
#pragma unroll
        for (int b = 0; b < FN; ++b) {
          const int row = wpix + b * 16 + lr;
#pragma unroll
          for (int a = 0; a < FM; ++a) {
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float x = acc[a][b][e];
              v[e] = ACT == ACT_RELU ? (x < 0.f ? 0.f : x) : ACT == ACT_PRELU ? (x < 0.f ? x * slope : x) : x;
            }
            store4(reinterpret_cast<T*>(stg + row * SROW + (a * 16 + lg * 4) * 2), v);
          }
        }
      };
      if (d.act == ACT_RELU) pack_tile(IC<ACT_RELU>{});
      else if (d.act == ACT_PRELU) pack_tile(IC<ACT_PRELU>{});
      else pack_tile(IC<ACT_NONE>{});
      continue;
    }
    const int pix_tile = tile_of(k);
#pragma unroll
    for (int b = 0; b < FN; ++b) {
      const int row = wpix + b * 16 + lr;
      int n = 0;
      if (d.bias && d.bias_stride != 0) {
        const long long m = (long long)pix_tile * BPIX + row;
        unsigned nn, qd, qh, qw;
        decode_row(d, m < d.M ? (unsigned)m : 0u, nn, qd, qh, qw);
        n = (int)nn;
      }
#pragma unroll
      for (int a = 0; a < FM; ++a) {
        const int ch = a * 16 + lg * 4;
        float v[4] = {acc[a][b][0], acc[a][b][1], acc[a][b][2], acc[a][b][3]};
        if (d.bias && !bias_lds && ch < d.Cout) {
          const float* bp = d.bias + (long long)n * d.bias_stride + ch;
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] += bp[e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = apply_act_g(v[e], d.act, d.slope);
        store4(reinterpret_cast<T*>(stg + row * SROW + ch * 2), v);
      }
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  RGBM_BARRIER();
}

template <typename T>
static int launch_ws64(ConvDesc d, bool rh, hipStream_t s) {
  constexpr int BCH = 64, BPIX = 256;
  const size_t LDS = (rh ? 2 * (size_t)(3 * BCH + 264) * 8 * sizeof(uint4) + 128 + (size_t)BPIX * 144
                         : 3 * (size_t)(BCH + BPIX) * 8 * sizeof(uint4) + (size_t)BPIX * 144) + BCH * sizeof(float);   // + bias table
  d.n_pix_tiles = (int)((d.M + BPIX - 1) / BPIX);
  d.n_ch_tiles = 1;
  d.n_tiles = d.n_pix_tiles;
  fill_fastdiv(d);
  if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(conv_igemm_ws64_kernel<false, T>), 160 * 1024)) return rc;
  if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(conv_igemm_ws64_kernel<true, T>), 160 * 1024)) return rc;
  int n_cu = 0;
  if (int rc = persistent_grid_cus(&n_cu)) return rc;
  const int grid = d.n_tiles < n_cu ? d.n_tiles : n_cu;
  prof_begin_launch(s, 15, d.algo_flops, d.algo_bytes);
  if (rh) hipLaunchKernelGGL((conv_igemm_ws64_kernel<true, T>), dim3((unsigned)grid), dim3(768), LDS, s, d);
  else hipLaunchKernelGGL((conv_igemm_ws64_kernel<false, T>), dim3((unsigned)grid), dim3(768), LDS, s, d);
  prof_end_launch(s);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

// CONV_WS64 / CONV_WS64_ROWHALO (16-bit storage types only)
int launch_igemm_ws64(const ConvDesc& d, int dtype, const ConvPlan& p, hipStream_t s) {
  const bool rh = p.kernel == CONV_WS64_ROWHALO;
  if (dtype == BF16) return launch_ws64<unsigned short>(d, rh, s);
  if (dtype == F16) return launch_ws64<f16_t>(d, rh, s);
  return conv_no_kernel();
}

}  // namespace rgbm
