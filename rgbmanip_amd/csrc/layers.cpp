#include "layers.h"
#include "conv_plan.h"
#include "kernels.h"

#include <string.h>

#include <array>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

namespace rgbm {

static thread_local std::string g_err;
void set_error(const std::string& s) { g_err = s; }
const char* last_error_cstr() { return g_err.c_str(); }

static inline unsigned short host_f32_to_bf16(float f) {
  unsigned u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (unsigned short)(u >> 16);
}

int ensure_dynamic_lds(const void* fn, int bytes) {
  // (device, kernel) -> bytes granted.  Several host threads may launch (one per device, or several streams of one device): the
  // table is shared, so it is guarded
  static std::mutex mu;
  static std::map<std::pair<int, const void*>, int> set_for;
  int dev = 0;
  RGBM_CHECK_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu);
  int& have = set_for[std::make_pair(dev, fn)];
  if (bytes > have) {
    RGBM_CHECK_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    have = bytes;
  }
  return 0;
}

// compute units of the CURRENT device rounded down to a multiple of the 8 XCDs (>= 8): the grid of the persistent kernels (one
// resident workgroup per CU).  Cached per device.
int persistent_grid_cus(int* n_cu) {
  static std::mutex mu;
  static std::map<int, int> per_dev;
  int dev = 0;
  RGBM_CHECK_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu);
  int& n = per_dev[dev];
  if (n == 0) {
    RGBM_CHECK_HIP(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
    n = n / 8 * 8;
    if (n < 8) n = 8;
  }
  *n_cu = n;
  return 0;
}

static int upload_bytes(const void* host, size_t bytes, DevBuf& dev) {
  RGBM_CHECK_HIP(hipMalloc(dev.out(), bytes));
  RGBM_CHECK_HIP(hipMemcpy(dev.get(), host, bytes, hipMemcpyHostToDevice));
  return 0;
}

int upload_f32(const float* host, size_t n, DevBuf& dev) { return upload_bytes(host, n * sizeof(float), dev); }

int ConvScratch::ksplit(hipStream_t s, bool allocate, KSplit* out) {
  int dev = 0;
  RGBM_CHECK_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu_);
  auto it = per_stream_.find(std::make_pair(dev, s));
  if (it == per_stream_.end()) {
    *out = KSplit();
    if (!allocate) return 0;
    std::pair<DevBuf, DevBuf> e;
    RGBM_CHECK_HIP(hipMalloc(e.first.out(), kM32SplitFloats * sizeof(float)));
    RGBM_CHECK_HIP(hipMalloc(e.second.out(), kM32SplitCounters * sizeof(unsigned)));
    // zeroed on the stream that uses them: a plain hipMemset goes to the null stream, which a non-blocking stream (torch's side streams)
    // does not wait for — the first split launch there could read the counters before they were zero
    RGBM_CHECK_HIP(hipMemsetAsync(e.second.get(), 0, kM32SplitCounters * sizeof(unsigned), s));
    it = per_stream_.emplace(std::make_pair(dev, s), std::move(e)).first;
  }
  out->scratch = it->second.first.get<float>();
  out->count = it->second.second.get<unsigned>();
  return 0;
}

int ConvScratch::identity(int dtype, const void** out) {
  RGBM_REQUIRE(dtype == BF16 || dtype == F16 || dtype == BF16X3, "identity matrix: 16-bit or split-pair storage");
  int dev = 0;
  RGBM_CHECK_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu_);
  DevBuf& p = ident_[std::make_pair(dev, dtype)];
  if (!p) {
    // bf16 / fp16 ones on the diagonal.  Split pairs: element e of a 4-element chunk has its hi half in 16-bit slot e of the chunk's
    // first 8 bytes; lo = 0
    const bool x3 = dtype == BF16X3;
    std::vector<unsigned short> h(256 * 256 * (x3 ? 2 : 1), 0);
    for (int i = 0; i < 256; ++i) {
      if (x3) h[(i * 256 + (i & ~3)) * 2 + (i & 3)] = 0x3f80;
      else h[i * 256 + i] = dtype == F16 ? 0x3c00 : 0x3f80;
    }
    DevBuf m;
    if (int rc = upload_bytes(h.data(), h.size() * 2, m)) return rc;
    p = std::move(m);
  }
  *out = p.get();
  return 0;
}

static inline unsigned short host_f32_to_f16(float f) {
  const _Float16 h = (_Float16)(f > 65504.f ? 65504.f : (f < -65504.f ? -65504.f : f));      // round to nearest even, saturating
  unsigned short u;
  memcpy(&u, &h, 2);
  return u;
}

// Can these (BN-folded) weights be held as IEEE f16 without changing what the layer computes?  No value at or beyond the f16 range
// (+-65504 would saturate) and no appreciable share of the weight mass below the smallest normal f16 (2^-14: such values lose mantissa
// bits or flush to zero).  bf16's exponent range never asks this question; the f16 forms of a bf16 net (sweep_f16) are only used for
// checkpoints that pass (round-5 advice: the synthetic checkpoints of the tests do, a trained one need not).
bool weights_fit_f16(const std::vector<float>& w) {
  double total = 0.0, small = 0.0;
  for (float v : w) {
    const float a = v < 0.f ? -v : v;
    if (!(a < 65504.f)) return false;                  // also refuses NaN / inf
    total += a;
    if (a != 0.f && a < 6.103515625e-05f) small += a;
  }
  return small <= 1e-3 * total;
}

// host fp32 values -> device array in the storage type `dtype`
int upload_packed(const std::vector<float>& w, int dtype, DevBuf& dev) {
  if (dtype == BF16 || dtype == F16) {
    std::vector<unsigned short> h(w.size());
    for (size_t i = 0; i < w.size(); ++i) h[i] = dtype == BF16 ? host_f32_to_bf16(w[i]) : host_f32_to_f16(w[i]);
    return upload_bytes(h.data(), h.size() * 2, dev);
  }
  if (dtype == BF16X3) {
    // split-pair chunks (common.h, bx3_t): every 4 consecutive values become {hi01, hi23, lo01, lo23}
    RGBM_REQUIRE(w.size() % 4 == 0, "bf16x3 weights: element count must be a multiple of 4");
    std::vector<unsigned> h(w.size());
    for (size_t i = 0; i < w.size(); i += 4) {
      unsigned short hi[4], lo[4];
      for (int e = 0; e < 4; ++e) {
        hi[e] = host_f32_to_bf16(w[i + e]);
        unsigned u = (unsigned)hi[e] << 16;
        float hf;
        memcpy(&hf, &u, 4);
        lo[e] = host_f32_to_bf16(w[i + e] - hf);
      }
      h[i] = hi[0] | ((unsigned)hi[1] << 16); h[i + 1] = hi[2] | ((unsigned)hi[3] << 16);
      h[i + 2] = lo[0] | ((unsigned)lo[1] << 16); h[i + 3] = lo[2] | ((unsigned)lo[3] << 16);
    }
    return upload_bytes(h.data(), h.size() * 4, dev);
  }
  return upload_bytes(w.data(), w.size() * 4, dev);
}

int conv_pack_geom(const ConvGeom& g, int dtype, int Cin_pad, int Cout_pad, int cls, PackedConv* pc) {
  const int BK = conv_bk(dtype);
  RGBM_REQUIRE(Cin_pad % dtype_chunk(dtype) == 0 && Cin_pad >= g.Cin, "Cin_pad");
  RGBM_REQUIRE(Cout_pad % 4 == 0 && Cout_pad >= g.Cout, "Cout_pad");
  *pc = PackedConv();
  if (!g.transposed) {
    pc->KD = g.KD; pc->KH = g.KH; pc->KW = g.KW;
  } else {
    // ConvTranspose3d(k=3, s=2, p=1, op=1): out o = 2q+p.  p=0 -> single tap k=1 at input q;
    // p=1 -> taps (delta=0 -> k=2 at q), (delta=1 -> k=0 at q+1).
    RGBM_REQUIRE(g.KD == 3 && g.KH == 3 && g.KW == 3 && g.sd == 2 && g.sh == 2 && g.sw == 2, "transposed conv geometry");
    RGBM_REQUIRE(cls >= 0 && cls < 8, "sub-pixel class");
    pc->KD = 1 + ((cls >> 2) & 1); pc->KH = 1 + ((cls >> 1) & 1); pc->KW = 1 + (cls & 1);
  }
  pc->ntaps = pc->KD * pc->KH * pc->KW;
  if (pc->ntaps > 1 || g.transposed) RGBM_REQUIRE(is_pow2(Cin_pad), "multi-tap / transposed conv needs power-of-two Cin_pad");
  const int K = pc->ntaps * Cin_pad;
  pc->Kpad = (K + BK - 1) / BK * BK;
  pc->KT = pc->Kpad / BK;
  return 0;
}

// Device tables of a layer's border-class tiles (plan_border), keyed by what they depend on.  Uploaded at the first launch of a shape,
// never per call; the layer owns them.
struct BorderTables {
  struct Entry { DevBuf buf; int n_wg = 0, b_ent = 0, b_rows = 0; };
  std::mutex mu;
  std::map<std::array<long long, 7>, Entry> per_shape;      // (device, N, Hi, Wi, workgroups, residual steps, main_rows)
};

int ConvLayer::init(int dtype_, const ConvGeom& g_, const float* w, const float* bias_h, const float* bn_scale,
                    const float* bn_shift, int Cin_pad_, int Cout_pad_, std::shared_ptr<ConvScratch> scratch_) {
  g = g_;
  scratch = std::move(scratch_);
  dtype = dtype_;
  Cin_pad = Cin_pad_;
  Cout_pad = Cout_pad_;
  PackedConv pc;
  if (int rc = conv_pack_geom(g, dtype, Cin_pad, Cout_pad, 0, &pc)) return rc;
  const int bch = conv_ch_tile(Cout_pad);
  const int rows = (Cout_pad + bch - 1) / bch * bch;   // weight rows padded to the channel tile

  // bias (conv bias and/or folded BN shift)
  if (bias_h || bn_shift) {
    std::vector<float> b(Cout_pad, 0.f);
    for (int o = 0; o < g.Cout; ++o) {
      float v = bias_h ? bias_h[o] : 0.f;
      if (bn_scale) v *= bn_scale[o];
      if (bn_shift) v += bn_shift[o];
      b[o] = v;
    }
    if (upload_f32(b.data(), b.size(), bias)) return -2;
  }

  auto finish = [&](PackedConv& pc, std::vector<float>& packed) -> int {
    if (upload_packed(packed, dtype, pc.w)) return -2;
    packs.push_back(std::move(pc));
    return 0;
  };

  if (!g.transposed) {
    std::vector<float> packed((size_t)rows * pc.Kpad, 0.f);
    const long long kvol = (long long)g.KD * g.KH * g.KW;
    for (int o = 0; o < g.Cout; ++o) {
      const float sc = bn_scale ? bn_scale[o] : 1.f;
      for (int c = 0; c < g.Cin; ++c)
        for (int t = 0; t < pc.ntaps; ++t)
          packed[(size_t)o * pc.Kpad + (size_t)t * Cin_pad + c] = w[((long long)o * g.Cin + c) * kvol + t] * sc;
    }
    // finite in every storage type: within bf16's largest value (f16 saturates on upload; a NaN fails the comparison)
    w_finite = true;
    for (float v : packed)
      if (!((v < 0.f ? -v : v) <= 3.3895313892515355e38f)) { w_finite = false; break; }
    border = std::make_shared<BorderTables>();
    return finish(pc, packed);
  }

  // one weight set per sub-pixel class (conv_pack_geom); weight layout [Cin][Cout][3][3][3]
  for (int cls = 0; cls < 8; ++cls) {
    const int pd_ = (cls >> 2) & 1, ph_ = (cls >> 1) & 1, pw_ = cls & 1;
    if (int rc = conv_pack_geom(g, dtype, Cin_pad, Cout_pad, cls, &pc)) return rc;
    std::vector<float> packed((size_t)rows * pc.Kpad, 0.f);
    auto kidx = [](int p, int delta) { return p == 0 ? 1 : (delta == 0 ? 2 : 0); };
    for (int o = 0; o < g.Cout; ++o) {
      const float sc = bn_scale ? bn_scale[o] : 1.f;
      for (int c = 0; c < g.Cin; ++c)
        for (int dd = 0; dd < pc.KD; ++dd)
          for (int dh = 0; dh < pc.KH; ++dh)
            for (int dw = 0; dw < pc.KW; ++dw) {
              const int t = (dd * pc.KH + dh) * pc.KW + dw;
              const int kd = kidx(pd_, dd), kh = kidx(ph_, dh), kw = kidx(pw_, dw);
              packed[(size_t)o * pc.Kpad + (size_t)t * Cin_pad + c] =
                  w[(((long long)c * g.Cout + o) * 3 + kd) * 9 + kh * 3 + kw] * sc;
            }
    }
    if (finish(pc, packed)) return -2;
  }
  return 0;
}

void conv_out_dims(const ConvGeom& g, int Di, int Hi, int Wi, int& Do, int& Ho, int& Wo) {
  if (g.transposed) { Do = 2 * Di; Ho = 2 * Hi; Wo = 2 * Wi; return; }
  Do = (Di + 2 * g.pd - g.dild * (g.KD - 1) - 1) / g.sd + 1;
  Ho = (Hi + 2 * g.ph - g.dilh * (g.KH - 1) - 1) / g.sh + 1;
  Wo = (Wi + 2 * g.pw - g.dilw * (g.KW - 1) - 1) / g.sw + 1;
}

void ConvLayer::out_dims(int Di, int Hi, int Wi, int& Do, int& Ho, int& Wo) const { conv_out_dims(g, Di, Hi, Wi, Do, Ho, Wo); }

void conv_desc_geom(ConvDesc& d, const ConvGeom& g, const PackedConv& pc, int Cin_pad, int Cout_pad, int N, int Di, int Hi, int Wi,
                    int ldo, int cls) {
  memset(&d, 0, sizeof(d));
  conv_out_dims(g, Di, Hi, Wi, d.Do, d.Ho, d.Wo);
  d.N = N; d.Di = Di; d.Hi = Hi; d.Wi = Wi;
  d.Cin = Cin_pad;
  d.Cout = Cout_pad; d.ldo = ldo;
  d.act = g.act; d.slope = g.slope;
  d.KD = pc.KD; d.KH = pc.KH; d.KW = pc.KW;
  d.ntaps = pc.ntaps; d.KT = pc.KT; d.Kpad = pc.Kpad;
  d.lcin = (pc.ntaps > 1 || is_pow2(Cin_pad)) ? ilog2(Cin_pad) : -1;
  if (g.transposed) {
    d.Dq = Di; d.Hq = Hi; d.Wq = Wi;
    d.sd = d.sh = d.sw = 1; d.pd = d.ph = d.pw = 0;
    d.dild = d.dilh = d.dilw = 1;
    d.osd = d.osh = d.osw = 2;
    d.opd = (cls >> 2) & 1; d.oph = (cls >> 1) & 1; d.opw = cls & 1;
  } else {
    d.Dq = d.Do; d.Hq = d.Ho; d.Wq = d.Wo;
    d.sd = g.sd; d.sh = g.sh; d.sw = g.sw; d.pd = g.pd; d.ph = g.ph; d.pw = g.pw;
    d.dild = g.dild; d.dilh = g.dilh; d.dilw = g.dilw;
    d.osd = d.osh = d.osw = 1;
    d.opd = d.oph = d.opw = 0;
  }
  d.M = (long long)N * d.Dq * d.Hq * d.Wq;
}

int ConvLayer::build_desc(ConvDesc& d, const void* in, void* out, int N, int Di, int Hi, int Wi, int ldo, const void* res,
                          int res_mode, const float* bias_override, int bias_stride, int cls, bool out_plain_f32) const {
  RGBM_REQUIRE(!packs.empty(), "conv layer not initialised");
  const PackedConv& pc = packs[cls];
  conv_desc_geom(d, g, pc, Cin_pad, Cout_pad, N, Di, Hi, Wi, ldo, cls);
  d.in = in; d.out = out; d.res = res; d.wgt = pc.w.get();
  d.bias = bias_override ? bias_override : bias.get<float>();
  d.bias_stride = bias_override ? bias_stride : 0;
  d.res_mode = res ? res_mode : RES_NONE;
  d.out_f32 = (out_plain_f32 && dtype == BF16X3) ? 1 : 0;
  d.w_finite = w_finite ? 1 : 0;
  // algorithmic work: real (unpadded) channels, every tap counted (zero padding included, as usual)
  d.algo_flops = 2.0 * (double)d.M * g.Cout * (double)pc.ntaps * g.Cin;
  d.algo_bytes = ((double)d.M * g.Cout + (cls == 0 ? (double)N * Di * Hi * Wi * g.Cin : 0.0) +
                  (res ? (double)d.M * g.Cout : 0.0)) * (double)dtype_size(dtype) +
                 (double)g.Cout * pc.ntaps * g.Cin * (double)dtype_size(dtype);
  return 0;
}

static bool stream_is_capturing(hipStream_t s) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
}

int ConvLayer::attach_border(ConvDesc& d, const ConvPlan& p, int n_cu, int flags, bool upload) const {
  int dev = 0;
  RGBM_CHECK_HIP(hipGetDevice(&dev));
  const std::array<long long, 7> key = {dev, d.N, d.Hi, d.Wi, n_cu, p.identity_residual ? 1 : 0, p.main_rows};
  std::lock_guard<std::mutex> lock(border->mu);
  auto it = border->per_shape.find(key);
  if (it == border->per_shape.end()) {
    BorderPlan bp;
    if (!upload || !plan_border(d, dtype, flags, p.main_rows, n_cu, &bp)) return 0;
    std::vector<int> tab(bp.wg_off);
    BorderTables::Entry e;
    e.n_wg = bp.n_wg;
    e.b_ent = (int)tab.size();
    for (int i : bp.order) {
      const BorderTile& bt = bp.tiles[i];
      const BorderClass& bc = bp.classes[bt.cls];
      tab.push_back((int)bt.row0);
      tab.push_back(bt.steps - bp.kr);
      tab.push_back(bc.kh0 | bc.kh1 << 4 | bc.kw0 << 8 | bc.kw1 << 12 | bt.ch << 16);
      tab.push_back(0);
    }
    e.b_rows = (int)tab.size();
    tab.insert(tab.end(), bp.rows.begin(), bp.rows.end());
    if (int rc = upload_bytes(tab.data(), tab.size() * sizeof(int), e.buf)) return rc;
    it = border->per_shape.emplace(key, std::move(e)).first;
  }
  d.btab = it->second.buf.get<int>();
  d.b_nwg = it->second.n_wg; d.b_ent = it->second.b_ent; d.b_rows = it->second.b_rows;
  return 0;
}

int ConvLayer::launch(ConvDesc& d, const ConvPlan& p, const ConvTuning& t, hipStream_t s) const {
  d.m0 = 0;
  d.korder = p.korder; d.buf_ok = p.buf_ok;
  d.ksplit = 1; d.kscratch = nullptr; d.kcount = nullptr;
  d.ident = nullptr;
  d.btab = nullptr; d.b_nwg = d.b_ent = d.b_rows = 0;
  RGBM_REQUIRE(scratch != nullptr || (p.ksplit <= 1 && !p.identity_residual), "conv layer initialised without a ConvScratch");
  // Two facts of the launch, not of the plan: what a launch needs on the device is allocated and uploaded at its first use, which must
  // not happen on a stream that is being captured.  Both forms of either launch give the same bits.  (The capture is asked about only
  // where something is missing; rgbm_adapose_forward_graph runs an eager forward in front of its capture, so its graphs lack neither.)
  if (p.ksplit > 1) {
    ConvScratch::KSplit k;
    if (int rc = scratch->ksplit(s, false, &k)) return rc;
    if (!k.scratch && !stream_is_capturing(s))
      if (int rc = scratch->ksplit(s, true, &k)) return rc;
    // 1. no K-split scratch for this stream and the stream is being captured: unsplit
    if (k.scratch) { d.ksplit = p.ksplit; d.kscratch = k.scratch; d.kcount = k.count; }
  }
  if (p.border && border) {      // (no tables: a transposed layer, whose shapes border_shape_ok does not take)
    if (int rc = attach_border(d, p, t.n_cu, t.flags, false)) return rc;
    // 2. no border table for this shape and the stream is being captured: row-major tiles
    if (!d.btab && !stream_is_capturing(s))
      if (int rc = attach_border(d, p, t.n_cu, t.flags, true)) return rc;
  }
  if (p.identity_residual)
    if (int rc = scratch->identity(dtype, &d.ident)) return rc;
  return launch_conv(d, dtype, p, s);
}

int ConvLayer::run(const void* in, void* out, int N, int Di, int Hi, int Wi, int ldo, const void* res, int res_mode,
                   const float* bias_override, int bias_stride, hipStream_t s, bool out_plain_f32) const {
  const int nclass = g.transposed ? 8 : 1;
  for (int cls = 0; cls < nclass; ++cls) {
    ConvDesc d;
    ConvTuning t;
    ConvPlan p;
    if (int rc = build_desc(d, in, out, N, Di, Hi, Wi, ldo, res, res_mode, bias_override, bias_stride, cls, out_plain_f32)) return rc;
    if (int rc = conv_tuning(0, &t)) return rc;
    if (int rc = plan_conv(d, dtype, t, &p)) return rc;
    if (int rc = launch(d, p, t, s)) return rc;
  }
  return 0;
}

int ConvLayer::run_then_1x1(const ConvLayer& next, const void* in, void* mid, int ldmid, void* out2, int ldo2, int N, int Di, int Hi,
                            int Wi, bool allow_fuse, bool* fused, hipStream_t s, bool out2_plain_f32) const {
  if (fused) *fused = false;
  const ConvGeom& ng = next.g;
  const bool is1x1 = !ng.transposed && ng.KD == 1 && ng.KH == 1 && ng.KW == 1 && ng.sd == 1 && ng.sh == 1 && ng.sw == 1 &&
                     ng.pd == 0 && ng.ph == 0 && ng.pw == 0 && next.packs.size() == 1;
  if (allow_fuse && is1x1 && !g.transposed && dtype_size(dtype) == 2 && next.dtype == dtype && next.Cin_pad == Cout_pad) {
    ConvDesc d;
    ConvTuning t;
    ConvPlan p;
    if (int rc = build_desc(d, in, mid, N, Di, Hi, Wi, ldmid, nullptr, RES_NONE, nullptr, 0, 0)) return rc;
    d.w2 = next.packs[0].w.get(); d.bias2 = next.bias.get<float>(); d.out2 = out2; d.ldo2 = ldo2; d.cout2 = next.Cout_pad;
    d.kpad2 = next.packs[0].Kpad; d.act2 = ng.act; d.slope2 = ng.slope;
    // the fused form runs only on the three-role 64-channel kernel; a descriptor that no kernel takes with its 1x1 attached (plan_conv
    // refuses it) or that another kernel takes goes the two-layer way below
    if (!conv_tuning(0, &t) && !plan_conv(d, dtype, t, &p) && (p.kernel == CONV_WS64 || p.kernel == CONV_WS64_ROWHALO)) {
      d.algo_flops += 2.0 * (double)d.M * ng.Cout * ng.Cin;
      d.algo_bytes += ((double)d.M * ng.Cout - (double)d.M * g.Cout) * 2.0;      // writes y2 instead of y
      if (int rc = launch(d, p, t, s)) return rc;
      if (fused) *fused = true;
      return 0;
    }
  }
  if (int rc = run(in, mid, N, Di, Hi, Wi, ldmid, nullptr, RES_NONE, nullptr, 0, s)) return rc;
  int Do, Ho, Wo;
  out_dims(Di, Hi, Wi, Do, Ho, Wo);
  return next.run(mid, out2, N, Do, Ho, Wo, ldo2, nullptr, RES_NONE, nullptr, 0, s, out2_plain_f32);
}

int UpConvLayer::init(int dtype, int Cin, int Cout_, const float* w, const float* bias_h, int act_, float slope_,
                      std::shared_ptr<ConvScratch> scratch) {
  Cout = Cout_; act = act_; slope = slope_;
  RGBM_REQUIRE(Cout % dtype_chunk(dtype) == 0, "upconv Cout must be a multiple of the 16-byte chunk");
  std::vector<float> wz((size_t)9 * Cout * Cin);
  for (int t = 0; t < 9; ++t)
    for (int o = 0; o < Cout; ++o)
      for (int c = 0; c < Cin; ++c) wz[((size_t)t * Cout + o) * Cin + c] = w[((size_t)o * Cin + c) * 9 + t];
  ConvGeom g;
  g.Cin = Cin; g.Cout = 9 * Cout; g.act = ACT_NONE;
  // The 256-channel tiles (conv_igemm_m32_kernel) take output channel counts that are multiples of 256; up_2's 9 x 64 = 576 stacked rows
  // ran whole on the generic 128-channel tile at half that kernel's rate.  Rows [0, 512) now go to the 256-channel kernel and the last 64
  // to the 64-channel one, both writing their channel range of the same z (two launches, same values: a row's dot product does not
  // depend on which launch computes it up to the kernels' summation order).
  split = (dtype != F32 && 9 * Cout > 256 && (9 * Cout) % 256 != 0 && (9 * Cout) % 256 <= 64 && Cin % 64 == 0) ? (9 * Cout) / 256 * 256 : 0;
  if (split) {
    ConvGeom g1 = g, g2 = g;
    g1.Cout = split; g2.Cout = 9 * Cout - split;
    if (int rc = gemm.init(dtype, g1, wz.data(), nullptr, nullptr, nullptr, Cin, g1.Cout, scratch)) return rc;
    if (int rc = gemm2.init(dtype, g2, wz.data() + (size_t)split * Cin, nullptr, nullptr, nullptr, Cin, g2.Cout, scratch)) return rc;
  } else {
    if (int rc = gemm.init(dtype, g, wz.data(), nullptr, nullptr, nullptr, Cin, 9 * Cout, scratch)) return rc;
  }
  if (bias_h) { if (upload_f32(bias_h, Cout, bias)) return -2; }
  return 0;
}

int UpConvLayer::run_gemm(const void* in, void* z, int V, int h, int w, hipStream_t s) const {
  if (int rc = gemm.run(in, z, V, 1, h, w, 9 * Cout, nullptr, RES_NONE, nullptr, 0, s)) return rc;
  if (split)
    if (int rc = gemm2.run(in, reinterpret_cast<char*>(z) + (size_t)split * dtype_size(gemm.dtype), V, 1, h, w, 9 * Cout, nullptr, RES_NONE, nullptr, 0, s)) return rc;
  return 0;
}

int UpConvLayer::combine(const void* z, void* out, int V, int h, int w, int ldo, hipStream_t s, const float* drop) const {
  return launch_upconv_combine(gemm.dtype, z, bias.get<float>(), out, V, h, w, Cout, ldo, act, slope, s, drop);
}

int UpConvLayer::run(const void* in, void* z, void* out, int V, int h, int w, int ldo, hipStream_t s, const float* drop) const {
  if (int rc = run_gemm(in, z, V, h, w, s)) return rc;
  return combine(z, out, V, h, w, ldo, s, drop);
}

int UpConvFinal::init(int dtype_, const float* w3, const float* b3, float slope_, const float* wfin, const float* bfin) {
  RGBM_REQUIRE(dtype_ == BF16 || dtype_ == F16 || dtype_ == BF16X3, "upconv + final: 16-bit or split-pair storage");
  dtype = dtype_; slope = slope_;
  std::vector<float> z((size_t)9 * 64 * 64), f(wfin, wfin + 32 * 64);
  for (int t = 0; t < 9; ++t)
    for (int o = 0; o < 64; ++o)
      for (int c = 0; c < 64; ++c) z[((size_t)t * 64 + o) * 64 + c] = w3[((size_t)o * 64 + c) * 9 + t];
  if (int rc = upload_packed(z, dtype, wz)) return rc;
  if (int rc = upload_packed(f, dtype, wf)) return rc;
  if (dtype == BF16 && weights_fit_f16(f)) if (int rc = upload_packed(f, F16, wf_h)) return rc;      // else: no f16 tail (AdaPose::feat_f16)
  if (upload_f32(b3, 64, bias) || upload_f32(bfin, 32, biasf)) return -2;
  return 0;
}

int UpConvFinal::run(const void* in, void* out, int out_kind, int V, int h, int w, hipStream_t s) const {
  return launch_upconv_final(dtype, in, wz.get(), bias.get<float>(), slope, wf.get(), biasf.get<float>(), out, out_kind, V, h, w, s, wf_h.get());
}

}  // namespace rgbm
