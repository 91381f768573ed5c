// Implicit-GEMM convolution, role-specialised persistent tiles on 16x16x32 MFMAs (gfx950): conv_igemm_ws_kernel, uniform-tap layers.
// Multiply waves that execute nothing but ds_read + MFMA, request waves that own the tap walk and the LDS-DMA; tiles of 128 x 256,
// 256 x 128 (WIDE) and 64 x 256 (SLIM) channels x pixels.  Shared pieces: igemm_device.h.
#include "igemm_device.h"

#ifndef WS_BUF
#define WS_BUF 1      // request waves: LDS-DMA through buffer descriptors (blds16) where the operands fit 32-bit offsets
#endif

namespace rgbm {

// ---------------------------------------------------------------------------------------------------------
// 128 x 256 tile, role-specialised: 8 multiply waves + 4 request waves, 3-stage LDS ring (uniform-tap layers only).
// Per K tile and wave conv_igemm_v3_kernel (igemm_generic.hip) issues 97 VALU + 71 SALU + 16 ds_read + 7 VMEM instructions next to its 32
// MFMAs (PMC, MFMA 34 % busy): the request bookkeeping, not bandwidth, sets the pace.  Here the 8 multiply waves execute
// nothing but ds_read + MFMA + one barrier per K tile, and the whole request side (tap walk, validity masks, 12 LDS-DMA
// pieces per wave and tile) lives in 4 extra waves, one per SIMD, whose scalar/vector work runs in the issue gaps of the
// MFMA streams.  Same operand layout and swizzle as the kernels there.
// ---------------------------------------------------------------------------------------------------------
// LDS chunk swizzle of the weight rows in conv_igemm_ws_kernel: conflict-free for its permuted fragment rows
__device__ __forceinline__ int swz_w(int row) { return ((row >> 1) & 1) | (((row >> 4) & 3) << 1); }

// 8-byte LDS read the compiler cannot merge with its neighbours (and does not count: the caller waits by hand)
template <int OFF>
__device__ __forceinline__ void lds_rd8(uint2& dst, unsigned addr) {
  asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF) : "memory");
}

// WIDE: the tile is 256 channels x 128 pixels instead of 128 x 256 (same LDS, same MFMA count, same 12 pieces per request wave):
// for Cout % 256 == 0 it halves the gathered-pixel bytes that cross L2 -> LDS at the price of twice the weight bytes, and the
// weight slice of a K tile is the same 32 KB for every workgroup of the chip while the pixel rows are a stream from HBM
// SLIM: a 64-channel x 256-pixel tile with FOUR multiply waves (8 waves, 512 threads; 10 pieces per request wave and K tile) for
// layers with at most 64 output channels in the storage types that have no ws64 kernel (split pairs, fp32) and for 16-bit
// layers that kernel does not take (residual adds): the role split of this kernel instead of the do-it-all generic tile.
template <typename T, bool WIDE, bool SLIM>
__global__ __launch_bounds__(SLIM ? 512 : 768) void conv_igemm_ws_kernel(const ConvDesc d) {
  static_assert(!SLIM || !WIDE, "slim tile: 64 x 256 only");
  constexpr int NMW = SLIM ? 4 : 8;          // multiply waves; four request waves follow
  constexpr int NTH = (NMW + 4) * 64;
  constexpr int BCH = SLIM ? 64 : WIDE ? 256 : 128, BPIX = (WIDE && !SLIM) ? 128 : 256;
  constexpr int E = 16 / sizeof(T);
  constexpr int BK = 8 * E;
  constexpr int XR = BPIX / 32;              // 8 gathered rows per request thread
  constexpr int WL = BCH / 32;               // 4 weight rows per request thread
  constexpr int NP = XR + WL;                // 12 LDS-DMA pieces per request wave and K tile
  constexpr int FM = 4, FN = 4;
  constexpr int STAGE = (BCH + BPIX) * 8;    // uint4 slots per stage (48 KB)
  extern __shared__ __attribute__((aligned(16))) uint4 lds3[];
  static_assert(NP == (SLIM ? 10 : 12), "the counted waits below assume 12 (slim: 10) pieces per tile");

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // 0..7 multiply, 8..11 request
  const int KT = d.KT;

  // Persistent: workgroup b owns tiles b, b + grid, b + 2*grid, ... (grid is a multiple of 8, so all of them map to the
  // same XCD) and the K-tile ring simply continues across tile boundaries: while the multiply waves write tile t's
  // outputs, the first two K tiles of tile t+1 are already landing.  Measured on the one-tile-per-workgroup version:
  // 15-19 us of prologue + pipeline fill + epilogue + relaunch per tile that nothing overlapped (a quarter of layer4).
  const int n_my = ((int)d.n_tiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
  const int total = n_my * KT;               // K-tile steps of this workgroup; every wave passes `total` barriers
  auto tile_of = [&](int k, int& pix_tile, int& ch_tile) {
    const int v = (int)blockIdx.x + k * (int)gridDim.x;          // virtual workgroup id -> XCD-aware tile order
    const int nblk = d.n_tiles, bq = nblk >> 3, br = nblk & 7, xcd = v & 7, bidx = v >> 3;
    const int lid = (xcd < br ? xcd * (bq + 1) : br * (bq + 1) + (xcd - br) * bq) + bidx;
    pix_tile = lid / d.n_ch_tiles;
    ch_tile = lid - pix_tile * d.n_ch_tiles;
  };

  // Per-channel bias table in LDS behind the ring (launch_ws reserves it): the multiply waves must not wait on vmcnt for
  // anything they do not need — on gfx9 the counter also covers their own output stores, in order, so a global bias read
  // after a tile's stores costs a full store round trip (measured: 5 us per tile).
  float* lbias = reinterpret_cast<float*>(lds3 + 3 * STAGE);
  const bool bias_lds = d.bias != nullptr && d.bias_stride == 0 && d.Cout <= 2048;
  if (bias_lds)
    for (int i = tid; i < d.Cout; i += NTH) lbias[i] = d.bias[i];
  __syncthreads();

  if (wave >= NMW) {
    // ------------------------------------------------------------------ request waves
    const T* __restrict__ in = reinterpret_cast<const T*>(d.in);
    const T* __restrict__ wgt = reinterpret_cast<const T*>(d.wgt);
    const int pw = wave - NMW;
    const int tp = tid - NMW * 64;
    const int j = tp & 7;
    const int r0 = tp >> 3;                  // 0..31
    const int js = j ^ ((r0 >> 1) & 7);
    const char* rowp[XR];
    unsigned rmask[XR];
    const char* wrow[WL];
    const char* zero = reinterpret_cast<const char*>(g_zero_page);
    int tkd = 0, tkh = 0, tkw = 0, tc = 0;   // wave-uniform tap walker
    long long wko = 0;                       // byte offset of the walker's K index in a weight row
    const unsigned lds0 = __builtin_amdgcn_readfirstlane(lds_addr(lds3 + pw * 64));      // this wave's first piece, stage 0
    // buffer form of the requests (d.buf_ok, set by the launcher when both operands fit 32-bit offsets): X offsets are taken from
    // (input base - xbias) so that a row whose tap (0,0,0) lies in the padding still has a non-negative offset
    const bool use_buf = WS_BUF && d.buf_ok;
    const long long xbias = ((long long)(d.pd * d.Hi + d.ph) * d.Wi + d.pw) * d.Cin * (long long)sizeof(T);
    const __amdgpu_buffer_rsrc_t rsrc_x = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(d.in)) - xbias, 0,
        (int)(unsigned)((long long)d.N * d.Di * d.Hi * d.Wi * d.Cin * (long long)sizeof(T) + xbias), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrc_w = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(d.wgt)), 0, (int)(unsigned)((long long)d.n_ch_tiles * BCH * d.Kpad * (long long)sizeof(T)), 0x00020000);
    unsigned xoff[XR], woff[WL];

    // The eight lanes (r0, j = 0..7) of a row group need the same XR row descriptors (GEMM rows r0 + 32*i): lane j decodes
    // row i = j once and the group exchanges them, instead of every lane decoding all XR rows (3 divisions, 7 bound tests and
    // two 64-bit products each: ~800 instructions per lane and tile, on the critical path of the first request of a tile —
    // with that work skipped a 4-K-tile launch ran 29 % faster, a 36-K-tile layer3 conv 7 %).  The decode of tile k+1 runs right
    // behind the LAST request of tile k (prepare_tile), i.e. while that request flies; the first request of tile k+1 only pays
    // the exchange (enter_tile).
    long long mybase = 0;
    unsigned mymask = 0;
    int my_ch_tile = 0;
    auto prepare_tile = [&](int k) {
      int pix_tile, ch_tile;
      tile_of(k, pix_tile, ch_tile);
      my_ch_tile = ch_tile;
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
        const long long b = __shfl(mybase, grp | i, 64);
        rmask[i] = (unsigned)__shfl((int)mymask, grp | i, 64);
        rowp[i] = reinterpret_cast<const char*>(in) + b + (long long)(js * E) * (long long)sizeof(T);
        xoff[i] = (unsigned)(b + xbias + (long long)(js * E) * (long long)sizeof(T));
      }
#pragma unroll
      for (int i = 0; i < WL; ++i) {
        const int row = r0 + 32 * i;
        wrow[i] = reinterpret_cast<const char*>(wgt + (long long)(my_ch_tile * BCH + row) * d.Kpad + (j ^ swz_w(row)) * E);
        woff[i] = (unsigned)(((long long)(my_ch_tile * BCH + row) * d.Kpad + (j ^ swz_w(row)) * E) * (long long)sizeof(T));
      }
      tkd = tkh = tkw = tc = 0;
      wko = 0;
    };

    int ikt = 0, itile = 0;                  // K tile / tile index of the next request
    auto issue = [&](int stage) {
      if (ikt == 0) enter_tile();
      const unsigned sbase = lds0 + (unsigned)stage * (STAGE * 16);
      const unsigned sel = (1u << tkd) | (256u << tkh) | (65536u << tkw);
      const long long soff =
          ((long long)((tkd * d.dild * d.Hi + tkh * d.dilh) * d.Wi + tkw * d.dilw) * d.Cin + tc) * (long long)sizeof(T);
      const bool cok = tkd < d.KD && tc + js * E < d.Cin;
      if (use_buf) {
#pragma unroll
        for (int i = 0; i < XR; ++i) {
          const bool ok = cok && (rmask[i] & sel) == sel;
          blds16(ok ? xoff[i] : 0xffffffffu, rsrc_x, (unsigned)soff, sbase + (BCH * 8 + i * 256) * 16);      // X rows 32*i + 8*pw .. +7
        }
#pragma unroll
        for (int i = 0; i < WL; ++i) blds16(woff[i], rsrc_w, (unsigned)wko, sbase + (i * 256) * 16);       // W rows 32*i + 8*pw .. +7
      } else {
#pragma unroll
      for (int i = 0; i < XR; ++i) {
        const bool ok = cok && (rmask[i] & sel) == sel;
        const char* src = ok ? rowp[i] + soff : zero;
        glds16(src, sbase + (BCH * 8 + i * 256) * 16);               // X rows 32*i + 8*pw .. +7
      }
#pragma unroll
      for (int i = 0; i < WL; ++i) glds16(wrow[i] + wko, sbase + (i * 256) * 16);   // W rows 32*i + 8*pw .. +7; wko = byte offset of K index tap * Cin + channel
      }
      if (d.korder && d.lcin >= 0) {
        // channel block outer, taps inner: the taps of one channel block read the same pixel rows shifted by a few rows / columns,
        // so between two uses of a cache line the XCD touches one channel block of its 32 tiles (~0.6 MB) instead of every channel
        // of them (2-4 MB, as much as its L2 holds): the pixels cross the fabric into L2 once per tile instead of once per kernel row
        wko += (long long)d.Cin * (long long)sizeof(T);
        if (++tkw == d.KW) { tkw = 0; if (++tkh == d.KH) { tkh = 0; if (++tkd == d.KD) { tkd = 0; tc += BK; wko = (long long)tc * (long long)sizeof(T); } } }
      } else {
        wko += BK * (long long)sizeof(T);
        tc += BK;
        if (d.lcin >= 0 && tc >= d.Cin) {
          tc = 0;
          if (++tkw == d.KW) { tkw = 0; if (++tkh == d.KH) { tkh = 0; ++tkd; } }
        }
      }
      if (++ikt == KT) { ikt = 0; ++itile; if (itile < n_my) prepare_tile(itile); }
    };

    if (total > 0) prepare_tile(0);
    if (total > 0) issue(0);
    if (total > 1) issue(1);
    int st = 0;
    for (int g = 0; g < total; ++g) {
      if (g + 1 >= total) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      else if (SLIM) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(12)" ::: "memory");   // step g landed; step g+1 may still fly
      RGBM_BARRIER();            // step g is complete in LDS; the stage of step g-1 is free
      if (g + 2 < total) issue(st == 0 ? 2 : st - 1);
      st = st == 2 ? 0 : st + 1;
    }
    return;
  }

  // -------------------------------------------------------------------- multiply waves
  const int wch = SLIM ? 0 : WIDE ? (wave >> 1) * 64 : (wave >> 2) * 64;
  const int wpix = (WIDE && !SLIM) ? (wave & 1) * 64 : (wave & 3) * 64;
  const int lr = lane & 15, lg = lane >> 4;
  // Fragment reads run half a K tile ahead of the MFMAs that consume them (two register sets): after the barrier of
  // step g the first-half fragments are requested, the second half of the previous step is multiplied out of registers
  // meanwhile, then the second-half fragments are requested under the first half's MFMAs.
  uint4 af0[FM], bf0[FN], af1[FM], bf1[FN];
  f32x4 acc[FM][FN];
  auto load_half = [&](int st, int s, uint4 (&af)[FM], uint4 (&bf)[FN]) {
    const uint4* W = lds3 + st * STAGE;
    const uint4* X = W + BCH * 8;
    const int cidx = s * 4 + lg;
#pragma unroll
    for (int a = 0; a < FM; ++a) {
      const int row = wch + (lr >> 2) * 16 + a * 4 + (lr & 3);       // MFMA row lr of fragment a = channel (lr>>2)*16 + a*4 + (lr&3)
      af[a] = W[row * 8 + (cidx ^ swz_w(row))];
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
  T* __restrict__ out = reinterpret_cast<T*>(d.out);
  const T* __restrict__ res = reinterpret_cast<const T*>(d.res);
  // split pairs: byte offsets (inside a stage) of this lane's two chunks of its first A / B fragment row
  unsigned x3a0 = 0, x3a1 = 0, x3b0 = 0, x3b1 = 0;
  if constexpr (std::is_same<T, bx3_t>::value) {
    const int ra = wch + (lr >> 2) * 16 + (lr & 3), rb = wpix + lr;
    x3a0 = (unsigned)(ra * 8 + (lg ^ swz_w(ra))) * 16u;
    x3a1 = (unsigned)(ra * 8 + ((4 + lg) ^ swz_w(ra))) * 16u;
    x3b0 = (unsigned)(BCH * 8 + rb * 8 + (lg ^ ((rb >> 1) & 7))) * 16u;
    x3b1 = (unsigned)(BCH * 8 + rb * 8 + ((4 + lg) ^ ((rb >> 1) & 7))) * 16u;
  }
  int st = 0;
  auto tile_interior = [&](int pix_tile, int ch_tile) {
    return (d.bias == nullptr || bias_lds) && (long long)(pix_tile + 1) * BPIX <= d.M && (ch_tile + 1) * BCH <= d.Cout &&
           d.act != ACT_TANH;
  };
  for (int k = 0; k < n_my; ++k) {
    {
      // interior tile with a per-channel bias (or none): the accumulators start at the bias, and the epilogue below is the
      // straight-line one.  (Tile coordinates are recomputed in the epilogue: nothing of this block lives across the K loop.)
      int pt, ct;
      tile_of(k, pt, ct);
      if (tile_interior(pt, ct) && d.bias) {
        const float* bp = lbias + ct * BCH + wch + lg * 16;
#pragma unroll
        for (int a = 0; a < FM; ++a) {
          const f32x4 b4 = *reinterpret_cast<const f32x4*>(bp + a * 4);
#pragma unroll
          for (int b = 0; b < FN; ++b) acc[a][b] = b4;
        }
      } else {
#pragma unroll
        for (int a = 0; a < FM; ++a)
#pragma unroll
          for (int b = 0; b < FN; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
    if constexpr (std::is_same<T, bx3_t>::value) {
      // split pairs: the two half-tile chunks of a lane (channels 4*lg.. and 16 + 4*lg..) together are the 8 k values of
      // one 16x16x32 operand — hi parts and lo parts separately — so a K tile (32 channels) is 16 x 3 full-rate MFMAs
      // (lo*hi, hi*lo, hi*hi; 16 independent accumulators between two uses of the same one)
      // The hi parts of a lane's two chunks are the first 8 bytes of each, the lo parts the last 8: read as 8-byte halves they land
      // in the operand registers directly.  (Read as two 16-byte chunks, every operand pair cost ~6 v_mov to regroup — 52 per wave
      // and K tile on the MFMA issue port, all behind the full read latency.  The 8-byte reads of a half wave hit each bank pair
      // twice, which costs the LDS array what the 16-byte reads cost.)  The reads are inline asm — hipcc merges plain 8-byte loads
      // back into 16-byte or paired ones and regroups with v_mov again — issued in the order the products need them and waited for
      // with counted waits (LDS reads return in order; at most 16 are outstanding).
      static_assert(!std::is_same<T, bx3_t>::value || (FM == 4 && FN == 4), "counted waits below: 4 x 4 fragments");
      for (int kt = 0; kt < KT; ++kt) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        RGBM_BARRIER();
        const unsigned sb = lds_addr(lds3 + st * STAGE);
        const unsigned pa0 = sb + x3a0, pa1 = sb + x3a1, pb0 = sb + x3b0, pb1 = sb + x3b1;
        uint2 ahp[FM][2], alp[FM][2], bhp[FN][2], blp[FN][2];
#define X3_RD_A(dst, a, half) { lds_rd8<(a) * 512 + (half) * 8>(dst[a][0], pa0); lds_rd8<(a) * 512 + (half) * 8>(dst[a][1], pa1); }
#define X3_RD_B(dst, b, half) { lds_rd8<(b) * 2048 + (half) * 8>(dst[b][0], pb0); lds_rd8<(b) * 2048 + (half) * 8>(dst[b][1], pb1); }
#define X3_T(p) "+v"(p[0]), "+v"(p[1])
#define X3_OP(p) make_uint4(p[0].x, p[0].y, p[1].x, p[1].y)
        X3_RD_A(alp, 0, 1) X3_RD_B(bhp, 0, 0) X3_RD_B(bhp, 1, 0) X3_RD_B(bhp, 2, 0) X3_RD_B(bhp, 3, 0)
        X3_RD_A(alp, 1, 1) X3_RD_A(alp, 2, 1) X3_RD_A(alp, 3, 1)
        asm volatile("s_waitcnt lgkmcnt(6)" : X3_T(alp[0]), X3_T(bhp[0]), X3_T(bhp[1]), X3_T(bhp[2]), X3_T(bhp[3]) :: "memory");
        const uint4 bh[FN] = {X3_OP(bhp[0]), X3_OP(bhp[1]), X3_OP(bhp[2]), X3_OP(bhp[3])};
        {
          const uint4 al = X3_OP(alp[0]);
#pragma unroll
          for (int b = 0; b < FN; ++b) MmaG<unsigned short>::run(al, bh[b], acc[0][b]);
        }
        __builtin_amdgcn_sched_barrier(0);
        X3_RD_A(ahp, 0, 0) X3_RD_A(ahp, 1, 0)
        asm volatile("s_waitcnt lgkmcnt(8)" : X3_T(alp[1]) :: "memory");
        {
          const uint4 al = X3_OP(alp[1]);
#pragma unroll
          for (int b = 0; b < FN; ++b) MmaG<unsigned short>::run(al, bh[b], acc[1][b]);
        }
        __builtin_amdgcn_sched_barrier(0);
        X3_RD_A(ahp, 2, 0) X3_RD_A(ahp, 3, 0)
        asm volatile("s_waitcnt lgkmcnt(10)" : X3_T(alp[2]) :: "memory");
        {
          const uint4 al = X3_OP(alp[2]);
#pragma unroll
          for (int b = 0; b < FN; ++b) MmaG<unsigned short>::run(al, bh[b], acc[2][b]);
        }
        __builtin_amdgcn_sched_barrier(0);
        X3_RD_B(blp, 0, 1) X3_RD_B(blp, 1, 1)
        asm volatile("s_waitcnt lgkmcnt(12)" : X3_T(alp[3]) :: "memory");
        {
          const uint4 al = X3_OP(alp[3]);
#pragma unroll
          for (int b = 0; b < FN; ++b) MmaG<unsigned short>::run(al, bh[b], acc[3][b]);
        }
        __builtin_amdgcn_sched_barrier(0);
        X3_RD_B(blp, 2, 1) X3_RD_B(blp, 3, 1)
        asm volatile("s_waitcnt lgkmcnt(0)"
                     : X3_T(ahp[0]), X3_T(ahp[1]), X3_T(ahp[2]), X3_T(ahp[3]), X3_T(blp[0]), X3_T(blp[1]), X3_T(blp[2]), X3_T(blp[3])
                     :: "memory");
        const uint4 ah[FM] = {X3_OP(ahp[0]), X3_OP(ahp[1]), X3_OP(ahp[2]), X3_OP(ahp[3])};
        const uint4 bl[FN] = {X3_OP(blp[0]), X3_OP(blp[1]), X3_OP(blp[2]), X3_OP(blp[3])};
#pragma unroll
        for (int a = 0; a < FM; ++a)
#pragma unroll
          for (int b = 0; b < FN; ++b) MmaG<unsigned short>::run(ah[a], bl[b], acc[a][b]);
#pragma unroll
        for (int a = 0; a < FM; ++a)
#pragma unroll
          for (int b = 0; b < FN; ++b) MmaG<unsigned short>::run(ah[a], bh[b], acc[a][b]);
#undef X3_RD_A
#undef X3_RD_B
#undef X3_T
#undef X3_OP
        st = st == 2 ? 0 : st + 1;
      }
    } else {
    for (int kt = 0; kt < KT; ++kt) {
      // every fragment read of the previous step has returned before the request waves may refill its stage
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      RGBM_BARRIER();
      load_half(st, 0, af0, bf0);
      __builtin_amdgcn_sched_barrier(0);
      if (kt > 0) mma_half(af1, bf1);                  // second half of K tile kt-1
      __builtin_amdgcn_sched_barrier(0);
      load_half(st, 1, af1, bf1);
      __builtin_amdgcn_sched_barrier(0);
      mma_half(af0, bf0);
      __builtin_amdgcn_sched_barrier(0);
      st = st == 2 ? 0 : st + 1;
    }
    mma_half(af1, bf1);
    }

    // ---- epilogue of tile k (the request waves are already filling the ring for tile k+1) ----
    // All 16 residual reads of a lane are requested before the first one is used: written as load-use-store per
    // fragment they were 16 dependent HBM round trips, 15-17 us per tile with the matrix pipe idle (measured as the
    // K-independent part of the launch time).
    int pix_tile, ch_tile;
    tile_of(k, pix_tile, ch_tile);
    const bool interior = tile_interior(pix_tile, ch_tile);
    long long obase[FN];
    int nn[FN];
    bool pok[FN];
    // every layer but the sub-pixel classes of the transposed convs enumerates its output tensor in storage order: GEMM row m IS
    // output pixel m, and the four coordinate divisions per lane and tile are only needed for a per-sample bias
    const bool dense_out = d.osd == 1 && d.osh == 1 && d.osw == 1 && d.opd == 0 && d.oph == 0 && d.opw == 0 && d.Dq == d.Do &&
                           d.Hq == d.Ho && d.Wq == d.Wo;
#pragma unroll
    for (int b = 0; b < FN; ++b) {
      const long long m = (long long)pix_tile * BPIX + wpix + b * 16 + lr;
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
    // channel map of this kernel: MFMA row r of fragment a is channel (r>>2)*16 + a*4 + (r&3) of the wave's 64, so the four
    // fragments give a lane 16 CONSECUTIVE channels (lg*16 ..) of its pixel: 16-byte residual reads and stores
    // (half as many memory instructions as the plain C layout's 8-byte pieces; the epilogue is issue-bound)
    const int chL = ch_tile * BCH + wch + lg * 16;
    constexpr int CHK = 16 / (int)sizeof(T);             // channels per 16-byte chunk
    constexpr int NQ = 16 / CHK;                         // chunks per lane and pixel
    // Interior tiles with a per-channel bias take a straight-line epilogue specialised on (activation, residual mode):
    // the generic loop below tests pixel / channel bounds, bias, residual mode and activation per 16-byte chunk and
    // reloads the bias in front of every chunk (behind the previous chunk's store, which may alias it) — ~1000
    // instructions, ~100 branches and 8 dependent bias round trips per wave and tile, measured as 9 us per tile with
    // the matrix pipe idle.
    if (interior) {
      // One activation expression for none / ReLU / PReLU: y = v < 0 ? max(v, -FLT_MAX) * nslope : v with nslope = 1 / 0 / slope
      // (the clamp keeps -inf * 0 from becoming NaN; a NaN fails the compare and passes through, like torch).  Specialised on
      // (activation, residual mode) as nine instantiations, hipcc hoisted the 64 compares of a lane in front of the dispatch
      // and kept their masks in 128 SGPRs (spilled to VGPR lanes with s_nop-padded v_writelane / v_readlane).
      const float nslope = d.act == ACT_RELU ? 0.f : d.act == ACT_PRELU ? d.slope : 1.f;
      auto fast = [&](auto resc) {
        constexpr int RES = decltype(resc)::value;
        // the residual reads of TWO pixel fragments are requested before their first store (see the vmcnt note above).  All four
        // at once (32 registers in the 16-bit types) pushed the kernel over its 168 registers: hipcc then spilled an ACCUMULATOR
        // out of the last MFMA block of every tile and reloaded it in the epilogue behind `s_waitcnt vmcnt(0)` — a scratch round
        // trip (~2 us) with the matrix pipe idle, per tile
        constexpr int GRP = 2;
#pragma unroll
        for (int bh = 0; bh < FN; bh += GRP) {
          uint4 rr[NQ][GRP];
          if (RES != RES_NONE) {
#pragma unroll
            for (int bb = 0; bb < GRP; ++bb)
#pragma unroll
              for (int q = 0; q < NQ; ++q)
                rr[q][bb] = *reinterpret_cast<const uint4*>(res + obase[bh + bb] + chL + q * CHK);
          }
#pragma unroll
          for (int bb = 0; bb < GRP; ++bb) {
            const int b = bh + bb;
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
              float v[CHK], rv[CHK];
#pragma unroll
              for (int e = 0; e < CHK; ++e) v[e] = acc[(q * CHK + e) >> 2][b][(q * CHK + e) & 3];
              if (RES != RES_NONE) unpack_chunk(rr[q][bb], rv, T());
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
              const uint4 pk = pack_chunk(v, T());
              *reinterpret_cast<uint4*>(out + obase[b] + chL + q * CHK) = pk;
            }
          }
        }
      };
      if (d.res_mode == RES_NONE) fast(IC<RES_NONE>{});
      else if (d.res_mode == RES_PRE_ACT) fast(IC<RES_PRE_ACT>{});
      else fast(IC<RES_POST_ACT>{});
      continue;
    }
#pragma unroll
    for (int bh = 0; bh < FN; bh += 2) {                 // two pixel fragments (2*NQ residual reads in flight) at a time
      uint4 rr[NQ][2];
#pragma unroll
      for (int bb = 0; bb < 2; ++bb)
#pragma unroll
        for (int q = 0; q < NQ; ++q) rr[q][bb] = make_uint4(0u, 0u, 0u, 0u);      // defined on every path: no value carried around the tile loop
      if (d.res_mode != RES_NONE) {
#pragma unroll
        for (int bb = 0; bb < 2; ++bb)
#pragma unroll
          for (int q = 0; q < NQ; ++q) {
            const int c = chL + q * CHK;
            const bool ok = pok[bh + bb] && c + CHK <= d.Cout;
            rr[q][bb] = *reinterpret_cast<const uint4*>(res + (ok ? obase[bh + bb] + c : 0ll));      // masked lanes read element 0
          }
      }
#pragma unroll
      for (int bb = 0; bb < 2; ++bb) {
        const int b = bh + bb;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          const int c = chL + q * CHK;
          if (!pok[b] || c >= d.Cout) continue;
          const bool whole = c + CHK <= d.Cout;          // Cout is a multiple of 4: a bf16 tail chunk holds 4 channels
          float v[CHK], rv[CHK];
#pragma unroll
          for (int e = 0; e < CHK; ++e) v[e] = acc[(q * CHK + e) >> 2][b][(q * CHK + e) & 3];
          if (d.bias) {
            const float* bp = d.bias + (long long)nn[b] * d.bias_stride + c;
#pragma unroll
            for (int e = 0; e < CHK; ++e) if (e < 4 || whole) v[e] += bp[e];
          }
#pragma unroll
          for (int e = 0; e < CHK; ++e) rv[e] = 0.f;
          if (d.res_mode != RES_NONE) {
            if (whole) unpack_chunk(rr[q][bb], rv, T());
            else load4(res + obase[b] + c, rv);
          }
          if (d.res_mode == RES_PRE_ACT) {
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

template <typename T, bool WIDE, bool SLIM = false>
static int launch_ws(ConvDesc d, hipStream_t s) {
  constexpr int BCH = SLIM ? 64 : WIDE ? 256 : 128, BPIX = (WIDE && !SLIM) ? 128 : 256;
  constexpr size_t LDS = 3 * (size_t)(BCH + BPIX) * 8 * sizeof(uint4) + 2048 * sizeof(float);      // K-tile ring + per-channel bias table
  d.n_pix_tiles = (int)((d.M + BPIX - 1) / BPIX);
  d.n_ch_tiles = (d.Cout + BCH - 1) / BCH;
  const long long ntiles = (long long)d.n_pix_tiles * d.n_ch_tiles;
  RGBM_REQUIRE(ntiles > 0 && ntiles < (1ll << 31) && d.M < (1ll << 31), "conv grid out of range");
  d.n_tiles = (int)ntiles;
  fill_fastdiv(d);
  if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(conv_igemm_ws_kernel<T, WIDE, SLIM>), (int)LDS)) return rc;
  int n_cu = 0;
  if (int rc = persistent_grid_cus(&n_cu)) return rc;
  const int grid = ntiles < n_cu ? (int)ntiles : n_cu;
  prof_begin_launch(s, SLIM ? (std::is_same<T, bx3_t>::value ? 34 : sizeof(T) == 2 ? 35 : 36) : WIDE && sizeof(T) == 2 ? 31 : WIDE && std::is_same<T, bx3_t>::value ? 33 : prof_row_ws<T>(), d.algo_flops, d.algo_bytes);
  hipLaunchKernelGGL((conv_igemm_ws_kernel<T, WIDE, SLIM>), dim3((unsigned)grid), dim3(SLIM ? 512 : 768), LDS, s, d);
  prof_end_launch(s);
  RGBM_CHECK_HIP(hipGetLastError());
  return 0;
}

template <typename T>
static int launch_ws_t(const ConvDesc& d, const ConvPlan& p, hipStream_t s) {
  return p.kernel == CONV_WS_SLIM ? launch_ws<T, false, true>(d, s) : p.kernel == CONV_WS_WIDE ? launch_ws<T, true>(d, s) : launch_ws<T, false>(d, s);
}

// CONV_WS / CONV_WS_WIDE / CONV_WS_SLIM
int launch_igemm_ws(const ConvDesc& d, int dtype, const ConvPlan& p, hipStream_t s) {
  return dtype == BF16 ? launch_ws_t<unsigned short>(d, p, s) : dtype == F16 ? launch_ws_t<f16_t>(d, p, s)
         : dtype == BF16X3 ? launch_ws_t<bx3_t>(d, p, s) : launch_ws_t<float>(d, p, s);
}

}  // namespace rgbm
