// Host-side layer objects: weight packing (BN folding, NDHWC/K-major repack, bf16 conversion) and
// ConvDesc construction for the generic implicit-GEMM kernel.
#pragma once
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "common.h"

namespace rgbm {

struct HostTensor {
  const float* data = nullptr;   // fp32 host pointer (int64 tensors such as num_batches_tracked are skipped)
  std::vector<long long> shape;
  long long numel() const { long long n = 1; for (auto s : shape) n *= s; return n; }
};
typedef std::map<std::string, HostTensor> StateDict;

// One device allocation that frees itself.  Move-only: whatever holds one cannot be copied, and nothing is shared or counted.  The upload
// helpers below fill it; out() hands its slot to hipMalloc or to a launcher that returns an allocation through void**.
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; }
    return *this;
  }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { reset(); }
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
  }
  void** out() { reset(); return &p_; }
  template <class T = void> T* get() const { return static_cast<T*>(p_); }
  explicit operator bool() const { return p_ != nullptr; }

 private:
  void* p_ = nullptr;
};

// Device scratch of the conv_igemm_m32_kernel launches (igemm_m32.hip), freed with the object.  Per (device, stream) the K-split
// buffers: kM32SplitFloats fp32 partial accumulators and kM32SplitCounters arrival counters (conv_plan.h) — zero when allocated, and
// every launch leaves them zero; launches on one stream are ordered, so a stream's launches can share them.  Per (device, storage type)
// the 256 x 256 identity, the W operand of the residual steps.  A net owns one (AdaPose) and hands it to its layers, so the scratch
// dies with the net; two nets never share one, whatever streams they run on.
class ConvScratch {
 public:
  struct KSplit { float* scratch = nullptr; unsigned* count = nullptr; };
  // the buffers of (current device, s), nulls where there are none; allocate: make them first (the counters are zeroed on s)
  int ksplit(hipStream_t s, bool allocate, KSplit* out);
  // uploaded at the first call (a blocking copy: not inside a capture)
  int identity(int dtype, const void** out);

 private:
  std::mutex mu_;
  std::map<std::pair<int, hipStream_t>, std::pair<DevBuf, DevBuf>> per_stream_;
  std::map<std::pair<int, int>, DevBuf> ident_;
};

struct ConvGeom {
  int Cin = 0, Cout = 0;         // logical channels
  int KD = 1, KH = 1, KW = 1;
  int sd = 1, sh = 1, sw = 1;
  int pd = 0, ph = 0, pw = 0;
  int dild = 1, dilh = 1, dilw = 1;
  bool transposed = false;       // ConvTranspose3d k3 s2 p1 op1 (sub-pixel decomposition)
  int act = ACT_NONE;
  float slope = 0.f;
};

// One packed weight set (a transposed conv owns 8, one per output parity class).
struct PackedConv {
  DevBuf w;                      // [Cout_pad][Kpad] in the layer dtype
  int KD = 1, KH = 1, KW = 1, ntaps = 1, Kpad = 0, KT = 0;
};

// The geometry half of a layer and of its ConvDesc: what needs no device memory (ConvLayer fills in the pointers; rgbm_conv_plan asks
// plan_conv about a shape with these alone).  cls: sub-pixel class of a transposed conv (0 otherwise).
int conv_pack_geom(const ConvGeom& g, int dtype, int Cin_pad, int Cout_pad, int cls, PackedConv* pc);      // taps and K padding (pc->w stays null)
void conv_out_dims(const ConvGeom& g, int Di, int Hi, int Wi, int& Do, int& Ho, int& Wo);
void conv_desc_geom(ConvDesc& d, const ConvGeom& g, const PackedConv& pc, int Cin_pad, int Cout_pad, int N, int Di, int Hi, int Wi,
                    int ldo, int cls);      // zeroes d, then every field that is not a pointer

struct BorderTables;              // device tables of a layer's border-class tiles, one per launch shape (layers.cpp; conv_plan.h)
struct ConvPlan;
struct ConvTuning;

struct ConvLayer {
  ConvGeom g;
  int dtype = F32;
  int Cin_pad = 0;               // physical input channels (>= Cin, multiple of the 16-byte chunk)
  int Cout_pad = 0;              // physical output channels written (multiple of 4)
  DevBuf bias;                   // [Cout_pad] fp32 or null
  std::vector<PackedConv> packs; // 1, or 8 for transposed
  bool w_finite = false;         // no packed weight is NaN / inf in the storage type (ConvDesc::w_finite), checked once in init
  std::shared_ptr<BorderTables> border;      // filled by run(): uploaded once per (device, views, map size), freed with the layer
  std::shared_ptr<ConvScratch> scratch;      // the owner's (a net's, or capi.cpp's for the one-shot entry points), shared by its layers

  // weights: [Cout][Cin][KD][KH][KW] (or [Cin][Cout][3][3][3] when transposed), optional per-Cout scale/shift
  // (folded BN) and bias.  Cin_pad: physical channel count of the input tensor.
  int init(int dtype, const ConvGeom& g, const float* w, const float* bias, const float* bn_scale, const float* bn_shift,
           int Cin_pad, int Cout_pad, std::shared_ptr<ConvScratch> scratch);

  // Run on input [N][Di][Hi][Wi][Cin_pad] -> output [N][Do][Ho][Wo][ldo] (+ch offset via out pointer).
  // res: optional residual with the output's layout.  bias_override/bias_stride: per-sample bias.
  // out_plain_f32 (bf16x3 layers only): the output tensor is plain fp32 (for what gathers from it), see ConvDesc::out_f32
  int run(const void* in, void* out, int N, int Di, int Hi, int Wi, int ldo, const void* res, int res_mode,
          const float* bias_override, int bias_stride, hipStream_t s, bool out_plain_f32 = false) const;
  void out_dims(int Di, int Hi, int Wi, int& Do, int& Ho, int& Wo) const;
  // this conv followed by `next` (a 1x1, stride 1): one fused launch writing only out2 when the kernel selection allows it
  // (*fused = true; `mid` is then NOT written), otherwise the two layers one after the other through `mid`.  out2_plain_f32: `next`'s
  // out_plain_f32.
  int run_then_1x1(const ConvLayer& next, const void* in, void* mid, int ldmid, void* out2, int ldo2, int N, int Di, int Hi, int Wi,
                   bool allow_fuse, bool* fused, hipStream_t s, bool out2_plain_f32 = false) const;
  int build_desc(ConvDesc& d, const void* in, void* out, int N, int Di, int Hi, int Wi, int ldo, const void* res, int res_mode,
                 const float* bias_override, int bias_stride, int cls, bool out_plain_f32 = false) const;
  // The one place where a plan becomes a launch: every launch-time field of d (ksplit, kscratch, kcount, ident, korder, buf_ok, btab,
  // b_*, m0) from the plan p that run() / run_then_1x1() made of d under t, this layer's border tables and the scratch; then
  // launch_conv, whose launchers only compute grids and launch.
  int launch(ConvDesc& d, const ConvPlan& p, const ConvTuning& t, hipStream_t s) const;
  // this layer's border-class table for (d, p) on t.n_cu workgroups, nulls where there is none; upload: make it first
  int attach_border(ConvDesc& d, const ConvPlan& p, int n_cu, int flags, bool upload) const;
};

// PSPUpsample (x2 bilinear align_corners -> conv3x3 pad 1 + bias -> activation; pspnet.py:100-107) as a 1x1 GEMM at the low
// resolution with the nine taps stacked on the output channels, followed by the tap-combining kernel (upconv.hip)
struct UpConvLayer {
  ConvLayer gemm;                // 1x1: Cin -> 9*Cout rows in (tap, channel) order, no bias, no activation
  ConvLayer gemm2;               // round 6: the stacked rows behind the last multiple of 256 (up_2: 576 = 512 + 64), see init()
  int split = 0;                 // rows of `gemm` when the product runs as two launches (0: one launch)
  DevBuf bias;                   // [Cout] fp32 or null
  int Cout = 0, act = ACT_NONE;
  float slope = 0.f;
  // w: [Cout][Cin][3][3] (nn.Conv2d layout)
  int init(int dtype, int Cin, int Cout, const float* w, const float* bias_h, int act, float slope, std::shared_ptr<ConvScratch> scratch);
  size_t scratch_elems(int V, int h, int w) const { return (size_t)V * h * w * 9 * Cout; }
  // in [V][h][w][Cin] -> z scratch [V][h][w][9*Cout] -> out [V][2h][2w][ldo]
  // drop (optional): Dropout2d factors, drop[v * kDropoutPerView + channel] (kernels.h)
  int run(const void* in, void* z, void* out, int V, int h, int w, int ldo, hipStream_t s, const float* drop = nullptr) const;
  // run()'s two halves: the stacked GEMM in -> z, and the tap combination z -> out.  AdaPose::forward_samples runs the first once and
  // the second once per Dropout2d sample, on the same z with that sample's rows of `drop`.
  int run_gemm(const void* in, void* z, int V, int h, int w, hipStream_t s) const;
  int combine(const void* z, void* out, int V, int h, int w, int ldo, hipStream_t s, const float* drop = nullptr) const;
};

// PSPNet tail: up_3 (x2 bilinear -> conv3x3 64 -> 64 + bias -> PReLU) and `final` (conv1x1 64 -> 32 + bias) in ONE kernel
// (upconv_final.hip): neither the up-sampled tensor, nor the tap-stacked z, nor up_3's output reach memory.  16-bit / split pairs.
struct UpConvFinal {
  DevBuf wz;                     // [9 * 64][64] storage type, rows in (tap, channel) order
  DevBuf wf;                     // [32][64] storage type
  DevBuf wf_h;                   // bf16 nets: the same in f16 (out_kind 2: the f16 tail)
  DevBuf bias;                   // [64] up_3 bias
  DevBuf biasf;                  // [32] final bias
  float slope = 0.f;
  int dtype = 0;
  bool ready() const { return (bool)wz; }
  bool f16_ready() const { return (bool)wf_h; }      // `final`'s weights are representable in f16 (weights_fit_f16): the f16 tail exists
  // w3 [64][64][3][3], b3 [64], wfin [32][64], bfin [32] (nn.Conv2d layouts)
  int init(int dtype, const float* w3, const float* b3, float slope, const float* wfin, const float* bfin);
  // in [V][h][w][64] -> out [V][2h][2w][32] (storage type; plain fp32: split-pair path only; f16: bf16 path only)
  int run(const void* in, void* out, int out_kind, int V, int h, int w, hipStream_t s) const;      // out_kind: launch_upconv_final's out_f32 (0 storage type, 1 plain fp32, 2 f16)
};

// device upload helpers
bool weights_fit_f16(const std::vector<float>& w);      // no value saturates in IEEE f16, no appreciable weight mass below its smallest normal
int upload_packed(const std::vector<float>& w, int dtype, DevBuf& dev);      // host fp32 -> device array in storage type dtype
int upload_f32(const float* host, size_t n, DevBuf& dev);

}  // namespace rgbm
