// extern "C" boundary of librgbm_hip.so — see include/rgbm.h for the contract and the reference
// interfaces each entry point replaces.
#include "../../include/rgbm.h"

#include <string.h>

#include <algorithm>
#include <initializer_list>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "adapose.h"
#include "box_overlap.h"
#include "box_verify.h"
#include "control.h"
#include "cost3d.h"
#include "conv_plan.h"
#include "prof.h"
#include "sample_stats.h"
#include "view_fusion.h"

using namespace rgbm;

// One captured forward: the launch sequence of AdaPose::forward for a fixed batch size and fixed device pointers, replayed with a
// single hipGraphLaunch (small batches are launch-bound: ~150 launches of a few microseconds each per forward).  The capture stream is part
// of the key: the graph's split launches point at the net's scratch for that stream (ConvScratch, layers.h), so a replay on another stream
// would share the partial sums and arrival counters with whatever this net runs on the first.
struct ForwardGraph {
  int B = 0;
  hipStream_t stream = nullptr;
  const void* in[7] = {nullptr};
  void* ws = nullptr;
  size_t ws_bytes = 0;
  rgbm_adapose_out out;
  int opt_version = 0;
  int tuning_version = 0;
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  size_t nodes = 0;
  unsigned long long last_use = 0;
};

static void drop_graph(ForwardGraph& g) {
  if (g.exec) (void)hipGraphExecDestroy(g.exec);
  if (g.graph) (void)hipGraphDestroy(g.graph);
  g.exec = nullptr; g.graph = nullptr;
}

// Owns everything the handle holds on the device: the net's weights and buffers free themselves (layers.h: DevBuf), the captured graphs here.
struct rgbm_adapose {
  ~rgbm_adapose() { for (auto& g : graphs) drop_graph(g); }
  AdaPose net;
  int device;
  int opt_version = 0;                 // bumped by set_option / set_chunk: captured graphs of older settings are dropped
  unsigned long long tick = 0;
  std::vector<ForwardGraph> graphs;    // at most kMaxGraphs, least recently used evicted
  int drop_explicit = 0;               // B of the masks loaded by rgbm_adapose_set_dropout_masks: the next forward uses them instead of drawing
  int drop_last_B = 0;                 // batch of the last forward with Dropout2d (what rgbm_adapose_dropout_masks reads back)
};
static const size_t kMaxGraphs = 8;

// Dropout2d factor buffer for batches of up to B poses (grown, never shrunk; a new address invalidates captured graphs)
static int ensure_dropout_capacity(rgbm_adapose* h, int B) {
  AdaPose& n = h->net;
  if (2 * B <= n.drop_cap_views) return 0;
  const int views = std::max(2 * B, 2 * n.drop_cap_views);
  DevBuf m;
  RGBM_CHECK_HIP(hipMalloc(m.out(), (size_t)views * kDropoutPerView * sizeof(float)));
  if (n.drop_masks) (void)hipDeviceSynchronize();      // a forward in flight may still read the old buffer
  n.drop_masks = std::move(m);                         // frees the old one
  n.drop_cap_views = views;
  ++h->opt_version;
  return 0;
}

static AdaPose::Outputs to_out(const rgbm_adapose_out* o) {
  AdaPose::Outputs r;
  r.nocs1 = o->view1_nocs; r.nocs2 = o->view2_nocs; r.depth1 = o->view1_depth; r.depth2 = o->view2_depth;
  r.r1 = o->view1_r; r.r2 = o->view2_r; r.t1 = o->view1_t; r.t2 = o->view2_t; r.s1 = o->view1_s; r.s2 = o->view2_s;
  return r;
}

// What every forward entry point does before it runs the net: the null checks (`name` arguments), the Dropout2d buffer for this batch, and
// the call's stream and dropout instruction - masks loaded for one forward win over drawing.  finish_call() books what a forward that ran
// did to the handle's dropout state.
static int prepare_call(rgbm_adapose* h, const char* name, int B, std::initializer_list<const void*> pointers, void* stream, AdaPose::Call* call) {
  bool ok = h != nullptr;
  for (const void* p : pointers) ok = ok && p != nullptr;
  RGBM_REQUIRE(ok, std::string(name) + " arguments");
  if (h->net.drop_p > 0.f && B > 0)
    if (int rc = ensure_dropout_capacity(h, B)) return rc;
  call->stream = (hipStream_t)stream;
  call->dropout = h->drop_explicit ? AdaPose::Dropout::Loaded : h->net.drop_p > 0.f ? AdaPose::Dropout::Draw : AdaPose::Dropout::None;
  return 0;
}

static int finish_call(rgbm_adapose* h, int B, const AdaPose::Call& call, int rc) {
  if (rc == 0 && call.dropout != AdaPose::Dropout::None) {
    h->drop_last_B = B;
    if (call.dropout == AdaPose::Dropout::Loaded) h->drop_explicit = 0;      // masks set for one forward are used once
  }
  return rc;
}

static bool is_baseline(const rgbm_adapose* h) { return h != nullptr && h->net.arch == AdaPose::ARCH_BASELINE; }
static bool is_realworld(const rgbm_adapose* h) { return h != nullptr && h->net.arch == AdaPose::ARCH_REALWORLD; }
static bool is_v2(const rgbm_adapose* h) { return h != nullptr && h->net.arch == AdaPose::ARCH_V2; }
static bool is_v1(const rgbm_adapose* h) { return h != nullptr && h->net.arch == AdaPose::ARCH_V1; }

static int forward_call(rgbm_adapose* h, const char* name, int B, const float* img1, const float* img2, const int32_t* choose1,
                        const int32_t* choose2, const float* P1, const float* P2, const float* depths, void* workspace, size_t workspace_bytes,
                        const rgbm_adapose_out* out, void* stream, AdaPose::Call call) {
  if (is_baseline(h)) {      // the projections and the depth planes are not read and may be null
    RGBM_REQUIRE(!(call.dense || call.depth_map || call.conf_map || call.nocs_map), std::string(name) + ": not implemented for the baseline network "
                 "(the dense maps come from the cost volume, which this network does not have)");
    if (int rc = prepare_call(h, name, B, {img1, img2, choose1, choose2, workspace, out}, stream, &call)) return rc;
    return h->net.forward(B, img1, img2, choose1, choose2, P1, P2, depths, workspace, workspace_bytes, to_out(out), call);
  }
  RGBM_REQUIRE(!is_realworld(h) || (call.coor1 && call.coor2), std::string(name) + ": the real-world network reads the chosen points' normalised "
               "coordinates: call rgbm_adapose_forward_realworld (the dense / maps, graph, cached and samples forwards are not implemented for it)");
  RGBM_REQUIRE(is_realworld(h) || !(call.coor1 || call.coor2), std::string(name) + ": coor1 / coor2 belong to the real-world network (rgbm_adapose_create_realworld)");
  if (int rc = prepare_call(h, name, B, {img1, img2, choose1, choose2, P1, P2, depths, workspace, out}, stream, &call)) return rc;
  RGBM_REQUIRE(h->drop_explicit == 0 || h->drop_explicit == B, "dropout: the masks set for the next forward are for batch " + std::to_string(h->drop_explicit));
  return finish_call(h, B, call, h->net.forward(B, img1, img2, choose1, choose2, P1, P2, depths, workspace, workspace_bytes, to_out(out), call));
}

// The tail of the one-shot entry points (tests): wait for what was launched and report a device error in the library's way.  Their
// temporary weights are locals that free themselves behind this, whatever `rc` is.
static int finish_one_shot(int rc, void* stream) {
  if (rc) return rc;
  const hipError_t e = hipStreamSynchronize((hipStream_t)stream);
  if (e == hipSuccess) return 0;
  set_error(hipGetErrorString(e));
  return -2;
}

// Both create entry points: the state dict from the weight descriptors, then a handle around the net `arch` names.  mode: create()'s
// norm_mode or create_baseline()'s regress_pose.  A net that fails half built frees what it had uploaded when the handle goes.
static int create_handle(rgbm_adapose_t** h, const char* name, int device, const rgbm_weight_desc* w, int n_w, int dtype, int arch, int mode) {
  RGBM_REQUIRE(h != nullptr && w != nullptr && n_w > 0, std::string(name) + " arguments");
  RGBM_REQUIRE(dtype == RGBM_F32 || dtype == RGBM_BF16 || dtype == RGBM_F16 || dtype == RGBM_BF16X3, "dtype must be 0 (fp32), 1 (bf16), 2 (fp16) or 3 (bf16x3)");
  RGBM_CHECK_HIP(hipSetDevice(device));
  StateDict sd;
  for (int i = 0; i < n_w; ++i) {
    std::string key = w[i].name;
    if (key.rfind("module.", 0) == 0) key = key.substr(7);
    HostTensor t;
    t.data = w[i].data;
    for (int d = 0; d < w[i].ndim; ++d) t.shape.push_back(w[i].shape[d]);
    sd[key] = t;
  }
  std::unique_ptr<rgbm_adapose> obj(new rgbm_adapose());
  obj->device = device;
  if (int rc = arch == AdaPose::ARCH_BASELINE    ? obj->net.create_baseline(sd, dtype, mode)
               : arch == AdaPose::ARCH_REALWORLD ? obj->net.create_realworld(sd, dtype)
               : arch == AdaPose::ARCH_V2        ? obj->net.create_v2(sd, dtype)
               : arch == AdaPose::ARCH_V1        ? obj->net.create_v1(sd, dtype)
                                                 : obj->net.create(sd, dtype, mode)) return rc;
  *h = obj.release();
  return 0;
}

extern "C" {

int rgbm_version(void) { return RGBM_VERSION; }
const char* rgbm_last_error(void) { return last_error_cstr(); }

int rgbm_adapose_create(rgbm_adapose_t** h, int device, const rgbm_weight_desc* w, int n_w, int dtype, int norm_mode) {
  RGBM_REQUIRE(norm_mode == 0 || norm_mode == 1, "norm_mode: 0 = eval-mode (folded) BatchNorm3d, 1 = per-sample statistics");
  return create_handle(h, "create", device, w, n_w, dtype, AdaPose::ARCH_V5, norm_mode);
}

int rgbm_adapose_create_baseline(rgbm_adapose_t** h, int device, const rgbm_weight_desc* w, int n_w, int dtype, int regress_pose) {
  RGBM_REQUIRE(regress_pose == 0 || regress_pose == 1, "regress_pose: 0 or 1");
  return create_handle(h, "create_baseline", device, w, n_w, dtype, AdaPose::ARCH_BASELINE, regress_pose);
}

int rgbm_adapose_create_realworld(rgbm_adapose_t** h, int device, const rgbm_weight_desc* w, int n_w, int dtype) {
  return create_handle(h, "create_realworld", device, w, n_w, dtype, AdaPose::ARCH_REALWORLD, 0);
}

int rgbm_adapose_create_v2(rgbm_adapose_t** h, int device, const rgbm_weight_desc* w, int n_w, int dtype) {
  return create_handle(h, "create_v2", device, w, n_w, dtype, AdaPose::ARCH_V2, 0);
}

int rgbm_v2_point_rows(rgbm_adapose_t* h, const float* feat, const int32_t* choose, const float* P_views, const float* depths, float* homog_scratch,
                       float* rows, float* fuse64, float* planes, int B, int P, int S, int views, void* stream) {
  RGBM_REQUIRE(is_v2(h) && h->net.v2_w, "v2_point_rows: the handle does not hold the v2 network (rgbm_adapose_create_v2)");
  RGBM_REQUIRE(feat && choose && P_views && depths && homog_scratch && rows && B > 0, "v2_point_rows arguments");
  if (int rc = launch_homography(P_views, homog_scratch, 2 * B, B, (hipStream_t)stream)) return rc;
  return launch_v2_point_rows(F32, h->net.v2_w.get<float>(), feat, homog_scratch, depths, choose, rows, fuse64, planes, 2 * B, B, P, h->net.n_depth, S, S,
                              views, (hipStream_t)stream);
}

int rgbm_adapose_create_v1(rgbm_adapose_t** h, int device, const rgbm_weight_desc* w, int n_w, int dtype) {
  return create_handle(h, "create_v1", device, w, n_w, dtype, AdaPose::ARCH_V1, 0);
}

int rgbm_v1_point_rows(rgbm_adapose_t* h, const float* feat, const int32_t* choose, const float* P_views, const float* depths, float* homog_scratch,
                       float* fused32, float* nocs4, float* rows128, float* planes, float* layer_scratch, int B, int P, int S, int views,
                       void* stream) {
  RGBM_REQUIRE(is_v1(h) && h->net.v1_w, "v1_point_rows: the handle does not hold the v1 network (rgbm_adapose_create_v1)");
  RGBM_REQUIRE(feat && choose && P_views && depths && homog_scratch && fused32 && B > 0 && P > 0 && (views == B || views == 2 * B), "v1_point_rows arguments");
  RGBM_REQUIRE((nocs4 == nullptr) == (rows128 == nullptr), "v1_point_rows: nocs4 and rows128 come together (stage B writes both)");
  const long long N = (long long)views * P;
  const bool fused_mlp = N % 64 == 0 && !(g_debug_flags & DBG_POINT_MLP_R5);
  RGBM_REQUIRE(nocs4 == nullptr || fused_mlp || layer_scratch, "v1_point_rows: the per-layer stage B needs layer_scratch (views * P * 288 floats)");
  RGBM_REQUIRE((((uintptr_t)nocs4 | (uintptr_t)rows128 | (uintptr_t)layer_scratch) & 15) == 0, "v1_point_rows: nocs4, rows128 and layer_scratch must be 16-byte aligned");
  AdaPose::V1Scratch sc{};
  if (layer_scratch) sc = {layer_scratch, layer_scratch + N * 64, layer_scratch + N * 192, layer_scratch + N * 256};
  if (int rc = launch_homography(P_views, homog_scratch, 2 * B, B, (hipStream_t)stream)) return rc;
  return h->net.v1_stages(F32, feat, homog_scratch, depths, choose, fused32, planes, nocs4, rows128, sc, B, P, S, views, fused_mlp, (hipStream_t)stream);
}

int rgbm_adapose_forward_realworld(rgbm_adapose_t* h, int B, const float* img1, const float* img2, const int32_t* choose1, const int32_t* choose2,
                                   const float* coor1, const float* coor2, const float* P1, const float* P2, const float* depths, void* workspace,
                                   size_t workspace_bytes, const rgbm_adapose_out* out, int stop_after, void* stream) {
  RGBM_REQUIRE(is_realworld(h), "forward_realworld: the handle does not hold the real-world network (rgbm_adapose_create_realworld)");
  RGBM_REQUIRE(coor1 && coor2, "forward_realworld arguments");
  AdaPose::Call call;
  call.stop_after = stop_after;
  call.coor1 = coor1; call.coor2 = coor2;
  return forward_call(h, "forward_realworld", B, img1, img2, choose1, choose2, P1, P2, depths, workspace, workspace_bytes, out, stream, call);
}

int rgbm_pose_rows(rgbm_adapose_t* h, const float* nocs4, const float* coor1, const float* coor2, const float* depth, float* rows, int B, int P,
                   int views, void* stream) {
  RGBM_REQUIRE(is_realworld(h) && h->net.prow_w, "pose_rows: the handle does not hold the real-world network (rgbm_adapose_create_realworld)");
  return launch_pose_rows(h->net.prow_w.get<float>(), nocs4, coor1, coor2, depth, rows, B, P, views, (hipStream_t)stream);
}

int rgbm_pts2d_to_coor(const float* pts2d_dev, float* coor_dev, int64_t n_points, int W, int H, void* stream) {
  return launch_pts2d_to_coor(pts2d_dev, coor_dev, (long long)n_points, W, H, (hipStream_t)stream);
}

int rgbm_view_fusion_scratch_bytes(int B, int P, size_t* bytes) {
  RGBM_REQUIRE(bytes && B >= 1 && P >= kVfMinPoints && P <= kVfMaxPoints && P % 32 == 0, "view_fusion_scratch_bytes: B >= 1, P a multiple of 32 in [32, 4096]");
  *bytes = view_fusion_scratch_bytes(B, P);
  return 0;
}

int rgbm_view_fusion(rgbm_adapose_t* h, const float* x1, const float* x2, int B, int P, float* y1, float* y2, void* scratch,
                     size_t scratch_bytes, void* stream) {
  RGBM_REQUIRE(h && x1 && x2 && y1 && y2 && scratch, "view_fusion arguments");
  RGBM_REQUIRE(h->net.vf_w, "view_fusion: the handle holds no attention stack (rgbm_adapose_create_baseline builds one)");
  return launch_view_fusion(h->net.vf_w.get<float>(), x1, x2, B, P, y1, y2, scratch, scratch_bytes, 2, (hipStream_t)stream);
}

int rgbm_depth_head(rgbm_adapose_t* h, const float* x, int64_t n_rows, float* out, void* stream) {
  RGBM_REQUIRE(h && x && out && n_rows > 0, "depth_head arguments");
  RGBM_REQUIRE(h->net.dh_w, "depth_head: the handle holds no depth_head (rgbm_adapose_create_baseline builds one)");
  return launch_depth_head(h->net.dh_w.get<float>(), x, (long long)n_rows, out, nullptr, 0, (hipStream_t)stream);
}

int rgbm_adapose_destroy(rgbm_adapose_t* h) {
  delete h;
  return 0;
}

int rgbm_adapose_set_chunk(rgbm_adapose_t* h, int max_chunk_views) {
  RGBM_REQUIRE(h && max_chunk_views > 0, "set_chunk arguments");
  h->net.max_chunk = max_chunk_views;
  ++h->opt_version;
  return 0;
}

int rgbm_adapose_set_option(rgbm_adapose_t* h, const char* key, int value) {
  RGBM_REQUIRE(h && key, "set_option arguments");
  const std::string k = key;
  if (is_baseline(h) || is_v2(h) || is_v1(h))
    for (const char* cv : {"cost_impl", "sparse_tail", "sparse_dec", "sweep_f16", "igemm_conv6"})
      RGBM_REQUIRE(k != cv, "option " + k + " belongs to the cost volume, which the " + (is_v2(h) ? "v2" : is_v1(h) ? "v1" : "baseline") + " network does not have");
  if (is_realworld(h))
    RGBM_REQUIRE(!(k == "sweep_f16" && value != 0), "option sweep_f16 does not exist for the real-world network (its variance volume has no f16 form)");
  if (k == "max_chunk") { RGBM_REQUIRE(value > 0, "max_chunk"); h->net.max_chunk = value; }
  else if (k == "igemm_conv6") { RGBM_REQUIRE(value == 0 || value == 1, "igemm_conv6"); h->net.igemm_conv6 = value; }
  else if (k == "fuse_final") { RGBM_REQUIRE(value == 0 || value == 1, "fuse_final"); h->net.fuse_final = value; }
  else if (k == "sparse_tail") { RGBM_REQUIRE(value == 0 || value == 1, "sparse_tail"); h->net.sparse_tail = value; }
  else if (k == "upconv") { RGBM_REQUIRE(value >= 0 && value <= 7, "upconv"); h->net.upconv = value; }
  else if (k == "sparse_dec") { RGBM_REQUIRE(value >= 0 && value <= 2, "sparse_dec"); h->net.sparse_dec = value; }
  else if (k == "stem") { RGBM_REQUIRE(value == 0 || value == 1, "stem"); h->net.stem = value; }
  else if (k == "view2_heads") { RGBM_REQUIRE(value == 0 || value == 1, "view2_heads"); h->net.view2_heads = value; }
  else if (k == "sweep_f16") { RGBM_REQUIRE(value == 0 || value == 1, "sweep_f16"); h->net.sweep_f16 = value; }
  else if (k == "cost_impl") { RGBM_REQUIRE(value >= 0 && value <= 3, "cost_impl"); h->net.cost_impl = value; }
  else { set_error("unknown option " + k); return -1; }
  ++h->opt_version;
  return 0;
}

int rgbm_adapose_set_dropout(rgbm_adapose_t* h, float p, uint64_t seed) {
  RGBM_REQUIRE(h && (p == 0.f || (p > 0.f && p < 1.f)), "set_dropout: p must be 0 (off) or lie in (0, 1)");
  RGBM_REQUIRE(!(is_baseline(h) && p > 0.f), "set_dropout: Dropout2d is not implemented for the baseline network");
  RGBM_REQUIRE(!(is_realworld(h) && p > 0.f), "set_dropout: Dropout2d is not implemented for the real-world network");
  RGBM_REQUIRE(!(is_v2(h) && p > 0.f), "set_dropout: Dropout2d is not implemented for the v2 network");
  RGBM_REQUIRE(!(is_v1(h) && p > 0.f), "set_dropout: Dropout2d is not implemented for the v1 network");
  RGBM_CHECK_HIP(hipSetDevice(h->device));
  if (!h->net.drop_state) RGBM_CHECK_HIP(hipMalloc(h->net.drop_state.out(), 2 * sizeof(unsigned long long)));
  RGBM_CHECK_HIP(hipDeviceSynchronize());      // every forward issued before this call has drawn its masks
  RGBM_CHECK_HIP(hipMemset(h->net.drop_state.get(), 0, 2 * sizeof(unsigned long long)));
  RGBM_CHECK_HIP(hipDeviceSynchronize());
  h->net.drop_p = p;
  h->net.drop_seed = (unsigned long long)seed;
  ++h->opt_version;
  return 0;
}

int rgbm_adapose_dropout_masks(rgbm_adapose_t* h, int B, float* out_dev) {
  RGBM_REQUIRE(h && out_dev && B > 0, "dropout_masks arguments");
  RGBM_REQUIRE(h->drop_last_B == B && h->net.drop_masks, "dropout_masks: the last forward with dropout had batch " +
               std::to_string(h->drop_last_B) + ", not " + std::to_string(B));
  RGBM_CHECK_HIP(hipSetDevice(h->device));
  RGBM_CHECK_HIP(hipDeviceSynchronize());
  RGBM_CHECK_HIP(hipMemcpy(out_dev, h->net.drop_masks.get(), (size_t)2 * B * kDropoutPerView * sizeof(float), hipMemcpyDeviceToDevice));
  return 0;
}

int rgbm_adapose_set_dropout_masks(rgbm_adapose_t* h, int B, const float* masks_dev) {
  RGBM_REQUIRE(h && masks_dev && B > 0, "set_dropout_masks arguments");
  RGBM_REQUIRE(!is_baseline(h), "set_dropout_masks: Dropout2d is not implemented for the baseline network");
  RGBM_REQUIRE(!is_realworld(h), "set_dropout_masks: Dropout2d is not implemented for the real-world network");
  RGBM_REQUIRE(!is_v2(h), "set_dropout_masks: Dropout2d is not implemented for the v2 network");
  RGBM_REQUIRE(!is_v1(h), "set_dropout_masks: Dropout2d is not implemented for the v1 network");
  RGBM_CHECK_HIP(hipSetDevice(h->device));
  if (int rc = ensure_dropout_capacity(h, B)) return rc;
  RGBM_CHECK_HIP(hipDeviceSynchronize());      // no forward in flight reads the buffer any more
  RGBM_CHECK_HIP(hipMemcpy(h->net.drop_masks.get(), masks_dev, (size_t)2 * B * kDropoutPerView * sizeof(float), hipMemcpyDeviceToDevice));
  h->drop_explicit = B;
  return 0;
}

int rgbm_adapose_workspace_bytes(rgbm_adapose_t* h, int B, size_t* bytes) {
  RGBM_REQUIRE(h && bytes && B > 0, "workspace_bytes arguments");
  *bytes = h->net.workspace_bytes(B);
  return 0;
}

int rgbm_adapose_forward_ex(rgbm_adapose_t* h, int B, const float* img1, const float* img2, const int32_t* choose1,
                            const int32_t* choose2, const float* P1, const float* P2, const float* depths, void* workspace,
                            size_t workspace_bytes, const rgbm_adapose_out* out, int stop_after, void* stream) {
  AdaPose::Call call;
  call.stop_after = stop_after;
  return forward_call(h, "forward", B, img1, img2, choose1, choose2, P1, P2, depths, workspace, workspace_bytes, out, stream, call);
}

int rgbm_adapose_forward(rgbm_adapose_t* h, int B, const float* img1, const float* img2, const int32_t* choose1,
                         const int32_t* choose2, const float* P1, const float* P2, const float* depths, void* workspace,
                         size_t workspace_bytes, const rgbm_adapose_out* out, void* stream) {
  return rgbm_adapose_forward_ex(h, B, img1, img2, choose1, choose2, P1, P2, depths, workspace, workspace_bytes, out, 0, stream);
}

int rgbm_adapose_dense_workspace_bytes(rgbm_adapose_t* h, int B, size_t* bytes) {
  RGBM_REQUIRE(h && bytes && B > 0, "dense_workspace_bytes arguments");
  *bytes = h->net.dense_workspace_bytes(B);
  return 0;
}

int rgbm_adapose_forward_dense(rgbm_adapose_t* h, int B, const float* img1, const float* img2, const int32_t* choose1,
                               const int32_t* choose2, const float* P1, const float* P2, const float* depths, void* workspace,
                               size_t workspace_bytes, const rgbm_adapose_out* out, float* depth_map, float* conf_map, void* stream) {
  RGBM_REQUIRE(depth_map != nullptr, "forward_dense: depth_map is NULL (conf_map may be, depth_map may not)");
  AdaPose::Call call;
  call.dense = true; call.depth_map = depth_map; call.conf_map = conf_map;
  return forward_call(h, "forward_dense", B, img1, img2, choose1, choose2, P1, P2, depths, workspace, workspace_bytes, out, stream, call);
}

int rgbm_adapose_forward_maps(rgbm_adapose_t* h, int B, const float* img1, const float* img2, const int32_t* choose1,
                              const int32_t* choose2, const float* P1, const float* P2, const float* depths, void* workspace,
                              size_t workspace_bytes, const rgbm_adapose_out* out, float* depth_map, float* conf_map, float* nocs_map,
                              void* stream) {
  RGBM_REQUIRE(depth_map != nullptr || nocs_map != nullptr, "forward_maps: depth_map, conf_map and nocs_map are all NULL (or conf_map alone is given)");
  RGBM_REQUIRE(depth_map != nullptr || conf_map == nullptr, "forward_maps: conf_map needs depth_map");
  AdaPose::Call call;
  call.dense = depth_map != nullptr; call.depth_map = depth_map; call.conf_map = conf_map; call.nocs_map = nocs_map;
  return forward_call(h, "forward_maps", B, img1, img2, choose1, choose2, P1, P2, depths, workspace, workspace_bytes, out, stream, call);
}

int rgbm_nocs_map(rgbm_adapose_t* h, const float* feat_f32, int V, int HW, float* nocs_map, void* stream) {
  RGBM_REQUIRE(h && feat_f32 && nocs_map && V > 0 && HW > 0, "nocs_map arguments");
  RGBM_REQUIRE(((long long)V * HW) % 64 == 0, "nocs_map: V * HW must be a multiple of 64");
  return h->net.nocs_map_of(feat_f32, (long long)V * HW, nocs_map, (hipStream_t)stream);
}

int rgbm_cloud_gather(const float* map1, const float* map2, const int32_t* index, int n, int S2, int C, int cap, float* out, void* stream) {
  return rgbm::launch_cloud_gather(map1, map2, index, n, S2, C, cap, out, (hipStream_t)stream);
}

int rgbm_cloud_similarity_scratch_bytes(int n, int cap, size_t* bytes) {
  RGBM_REQUIRE(bytes && n >= 0 && cap >= 1, "cloud_similarity_scratch_bytes arguments");
  *bytes = rgbm::cloud_similarity_scratch_bytes(n, cap);
  return 0;
}

int rgbm_cloud_similarity(const float* nocs, const float* cloud, const int32_t* count, int n, int cap, uint32_t seed, double* bbox, double* srt,
                          int32_t* info, int32_t* valid, void* scratch, size_t scratch_bytes, void* stream) {
  return rgbm::launch_cloud_similarity(nocs, cloud, count, n, cap, seed, bbox, srt, info, valid, scratch, scratch_bytes, (hipStream_t)stream);
}

int rgbm_depth_to_points(const float* depth_map, const double* Kcrop, const double* E, int n, int S, float* points, void* stream) {
  return rgbm::launch_depth_to_points(depth_map, Kcrop, E, n, S, points, (hipStream_t)stream);
}

int rgbm_depth_consistency(const float* depth_a, const float* conf_a, const uint8_t* mask_a, const double* Kcrop_a, const double* E_a,
                           const float* depth_b, const double* Kcrop_b, const double* E_b, int n, int S, double px_max, double rel_max,
                           float conf_min, float* fused, float* reproj, float* rel, uint8_t* keep, void* stream) {
  return rgbm::launch_depth_consistency(depth_a, conf_a, mask_a, Kcrop_a, E_a, depth_b, Kcrop_b, E_b, n, S, px_max, rel_max, conf_min, fused,
                                        reproj, rel, keep, (hipStream_t)stream);
}

int rgbm_cloud_pack(const float* fused1, const uint8_t* keep1, const double* Kcrop1, const double* E1, const float* fused2,
                    const uint8_t* keep2, const double* Kcrop2, const double* E2, int n, int S, int cap, float* cloud, int32_t* index,
                    int32_t* count, void* stream) {
  return rgbm::launch_cloud_pack(fused1, keep1, Kcrop1, E1, fused2, keep2, Kcrop2, E2, n, S, cap, cloud, index, count, (hipStream_t)stream);
}

int rgbm_depth_fusion(const float* depth, const float* conf, const uint8_t* mask, const double* Kcrop, const double* E, int n, int V, int S,
                      double px_max, double rel_max, float conf_min, int n_min, float* fused, uint8_t* keep, uint8_t* nviews, uint16_t* agree,
                      void* stream) {
  return rgbm::launch_depth_fusion(depth, conf, mask, Kcrop, E, n, V, S, px_max, rel_max, conf_min, n_min, fused, keep, nviews, agree,
                                   (hipStream_t)stream);
}

int rgbm_cloud_pack_views(const float* fused, const uint8_t* keep, const double* Kcrop, const double* E, int n, int V, int S, int cap,
                          float* cloud, int32_t* index, int32_t* count, void* stream) {
  return rgbm::launch_cloud_pack_views(fused, keep, Kcrop, E, n, V, S, cap, cloud, index, count, (hipStream_t)stream);
}

int rgbm_cloud_gather_views(const float* maps, const int32_t* index, int n, int V, int S2, int C, int cap, float* out, void* stream) {
  return rgbm::launch_cloud_gather_views(maps, index, n, V, S2, C, cap, out, (hipStream_t)stream);
}

int rgbm_adapose_feature_bytes(rgbm_adapose_t* h, size_t* bytes) {
  RGBM_REQUIRE(h && bytes, "feature_bytes arguments");
  RGBM_REQUIRE(!is_baseline(h), "feature_bytes: the feature cache is not implemented for the baseline network");
  RGBM_REQUIRE(!is_v2(h), "feature_bytes: the feature cache is not implemented for the v2 network");
  RGBM_REQUIRE(!is_v1(h), "feature_bytes: the feature cache is not implemented for the v1 network");
  *bytes = h->net.feature_bytes();
  return 0;
}

int rgbm_adapose_features_workspace_bytes(rgbm_adapose_t* h, int V, size_t* bytes) {
  RGBM_REQUIRE(h && bytes && V > 0, "features_workspace_bytes arguments");
  RGBM_REQUIRE(!is_baseline(h), "features_workspace_bytes: the feature cache is not implemented for the baseline network");
  RGBM_REQUIRE(!is_v2(h), "features_workspace_bytes: the feature cache is not implemented for the v2 network");
  RGBM_REQUIRE(!is_v1(h), "features_workspace_bytes: the feature cache is not implemented for the v1 network");
  *bytes = h->net.features_workspace_bytes(V);
  return 0;
}

int rgbm_adapose_features(rgbm_adapose_t* h, int V, const float* img, const int32_t* slots_dev, void* pool, int pool_records,
                          void* workspace, size_t workspace_bytes, void* stream) {
  RGBM_REQUIRE(!is_baseline(h), "features: the feature cache is not implemented for the baseline network");
  RGBM_REQUIRE(!is_v2(h), "features: the feature cache is not implemented for the v2 network");
  RGBM_REQUIRE(!is_v1(h), "features: the feature cache is not implemented for the v1 network");
  AdaPose::Call call;      // a handle with Dropout2d on (or masks loaded) is refused by the net
  if (int rc = prepare_call(h, "features", 0, {img, slots_dev, pool, workspace}, stream, &call)) return rc;
  return h->net.features(V, img, slots_dev, pool, pool_records, workspace, workspace_bytes, call);
}

int rgbm_crop_fingerprint(const float* img, int V, int n_words, uint64_t* keys_out, void* stream) {
  return rgbm::launch_crop_fingerprint(img, V, n_words, reinterpret_cast<unsigned long long*>(keys_out), (hipStream_t)stream);
}

int rgbm_adapose_forward_cached(rgbm_adapose_t* h, int B, const void* pool, int pool_records, const int32_t* slot1_dev,
                                const int32_t* slot2_dev, const int32_t* choose1, const int32_t* choose2, const float* P1, const float* P2,
                                const float* depths, void* workspace, size_t workspace_bytes, const rgbm_adapose_out* out, void* stream) {
  RGBM_REQUIRE(!is_baseline(h), "forward_cached: the feature cache is not implemented for the baseline network");
  RGBM_REQUIRE(!is_v2(h), "forward_cached: the feature cache is not implemented for the v2 network");
  RGBM_REQUIRE(!is_v1(h), "forward_cached: the feature cache is not implemented for the v1 network");
  AdaPose::Call call;
  if (int rc = prepare_call(h, "forward_cached", B, {pool, slot1_dev, slot2_dev, choose1, choose2, P1, P2, depths, workspace, out}, stream, &call)) return rc;
  return h->net.forward_cached(B, pool, pool_records, slot1_dev, slot2_dev, choose1, choose2, P1, P2, depths, workspace, workspace_bytes,
                               to_out(out), call);      // refuses a call with Dropout2d
}

int rgbm_adapose_samples_workspace_bytes(rgbm_adapose_t* h, int B, int S, size_t* bytes) {
  RGBM_REQUIRE(h && bytes && B > 0, "samples_workspace_bytes arguments");
  RGBM_REQUIRE(S >= 1 && (long long)S * B <= (1 << 20), "samples_workspace_bytes: S >= 1 samples");
  RGBM_REQUIRE(!is_baseline(h), "samples_workspace_bytes: forward_samples is not implemented for the baseline network");
  RGBM_REQUIRE(!is_v2(h), "samples_workspace_bytes: forward_samples is not implemented for the v2 network");
  RGBM_REQUIRE(!is_v1(h), "samples_workspace_bytes: forward_samples is not implemented for the v1 network");
  *bytes = h->net.samples_workspace_bytes(B, S);
  return 0;
}

int rgbm_adapose_forward_samples(rgbm_adapose_t* h, int B, int S, const float* img1, const float* img2, const int32_t* choose1,
                                 const int32_t* choose2, const float* P1, const float* P2, const float* depths, void* workspace,
                                 size_t workspace_bytes, const rgbm_adapose_out* out, void* stream) {
  RGBM_REQUIRE(h != nullptr, "forward_samples arguments");
  RGBM_REQUIRE(!is_baseline(h), "forward_samples: not implemented for the baseline network (it has no Dropout2d)");
  RGBM_REQUIRE(!is_v2(h), "forward_samples: forward_samples is not implemented for the v2 network");
  RGBM_REQUIRE(!is_v1(h), "forward_samples: forward_samples is not implemented for the v1 network");
  RGBM_REQUIRE(B > 0 && S >= 1 && (long long)S * B <= (1 << 20), "forward_samples: B >= 1 poses and S >= 1 samples");
  RGBM_REQUIRE(h->net.drop_p > 0.f || h->drop_explicit, "forward_samples: Dropout2d is off and no masks are loaded (rgbm_adapose_set_dropout / "
               "rgbm_adapose_set_dropout_masks): the samples would be equal");
  RGBM_REQUIRE(h->drop_explicit == 0 || h->drop_explicit == S * B, "forward_samples: the masks set for the next forward are for batch " +
               std::to_string(h->drop_explicit) + ", not S x B = " + std::to_string(S * B));
  AdaPose::Call call;      // the net refuses the upconv A/B paths and a short workspace, also before anything is launched
  if (int rc = prepare_call(h, "forward_samples", S * B, {img1, img2, choose1, choose2, P1, P2, depths, workspace, out}, stream, &call)) return rc;
  return finish_call(h, S * B, call, h->net.forward_samples(B, S, img1, img2, choose1, choose2, P1, P2, depths, workspace, workspace_bytes,
                                                            to_out(out), call));
}

int rgbm_sample_box_stats(const double* boxes, const uint8_t* ok, int n, int S, int32_t* count, double* bbox_mean, double* bbox_std,
                          double* center_mean, double* center_cov, double* extent_mean, double* extent_std, double* axis_spread_deg,
                          void* stream) {
  return rgbm::launch_sample_box_stats(boxes, ok, n, S, count, bbox_mean, bbox_std, center_mean, center_cov, extent_mean, extent_std,
                                       axis_spread_deg, (hipStream_t)stream);
}

int rgbm_box_agreement(const double* a, const double* b, const uint8_t* ok_a, const uint8_t* ok_b, int n, int32_t* valid, double* iou,
                       double* inter_volume, double* volume_a, double* volume_b, double* center_dist, double* center_delta,
                       double* corner_dist, double* extent_a, double* extent_b, double* axis_angle_deg, double* axis_fold_deg,
                       double* rot_deg, void* stream) {
  const rgbm::BoxAgreementOut o{valid, iou, inter_volume, volume_a, volume_b, center_dist, center_delta, corner_dist,
                                extent_a, extent_b, axis_angle_deg, axis_fold_deg, rot_deg};
  return rgbm::launch_box_agreement(a, b, ok_a, ok_b, n, o, (hipStream_t)stream);
}

int rgbm_box_iou_matrix(const double* a, const double* b, const uint8_t* ok_a, const uint8_t* ok_b, int n, int P, int Q, double* iou,
                        void* stream) {
  return rgbm::launch_box_iou_matrix(a, b, ok_a, ok_b, n, P, Q, iou, (hipStream_t)stream);
}

int rgbm_box_silhouette_scratch_bytes(int n, int S, int V, size_t* bytes) {
  RGBM_REQUIRE(bytes, "box_silhouette_scratch_bytes arguments");
  RGBM_REQUIRE(S >= 1 && S <= rgbm::kVerifyBoxesMax && V >= 1 && V <= rgbm::kVerifyViewsMax && n >= 1 &&
               (long long)n * S * V <= (long long)rgbm::kVerifyRecordsMax, "box_silhouette: 1 <= S <= 64, 1 <= V <= 16, n >= 1 and n * S * V <= 2^24");
  *bytes = rgbm::box_silhouette_scratch_bytes(n, S, V);
  return 0;
}

int rgbm_box_silhouette(const double* boxes, const uint8_t* ok, const double* K, const double* E, const uint8_t* mask, int n, int S, int V,
                        int H, int W, int32_t* area_box, int32_t* inter, int32_t* area_mask, int32_t* rect, int32_t* flags, void* scratch,
                        size_t scratch_bytes, void* stream) {
  const rgbm::BoxSilhouetteOut o{area_box, inter, area_mask, rect, flags};
  return rgbm::launch_box_silhouette(boxes, ok, K, E, mask, n, S, V, H, W, o, scratch, scratch_bytes, (hipStream_t)stream);
}

int rgbm_cloud_in_box(const float* cloud, const int32_t* count, int count_cols, const double* boxes, const uint8_t* ok, int n, int S, int cap,
                      double inflate, int32_t* inside, int32_t* total, void* stream) {
  return rgbm::launch_cloud_in_box(cloud, count, count_cols, boxes, ok, n, S, cap, inflate, inside, total, (hipStream_t)stream);
}

int rgbm_sample_point_stats(const float* x, int n, int S, int64_t M, float* mean, float* std, void* stream) {
  return rgbm::launch_sample_point_stats(x, n, S, (long long)M, mean, std, (hipStream_t)stream);
}

int rgbm_adapose_graph_clear(rgbm_adapose_t* h) {
  RGBM_REQUIRE(h, "graph_clear arguments");
  for (auto& g : h->graphs) drop_graph(g);
  h->graphs.clear();
  return 0;
}

int rgbm_adapose_forward_graph(rgbm_adapose_t* h, int B, const float* img1, const float* img2, const int32_t* choose1,
                               const int32_t* choose2, const float* P1, const float* P2, const float* depths, void* workspace,
                               size_t workspace_bytes, const rgbm_adapose_out* out, void* stream, int32_t* n_nodes, int32_t* captured) {
  if (n_nodes) *n_nodes = 0;
  if (captured) *captured = 0;
  RGBM_REQUIRE(!is_baseline(h), "forward_graph: hipGraph replay is not implemented for the baseline network");
  RGBM_REQUIRE(!is_realworld(h), "forward_graph: hipGraph replay is not implemented for the real-world network");
  RGBM_REQUIRE(!is_v2(h), "forward_graph: hipGraph replay is not implemented for the v2 network");
  RGBM_REQUIRE(!is_v1(h), "forward_graph: hipGraph replay is not implemented for the v1 network");
  AdaPose::Call call;
  // the in-library profiler records events around launches: not capturable, and a timing run wants the launches themselves
  // masks loaded by rgbm_adapose_set_dropout_masks are for one forward: not captured
  if (prof_enabled() || (h && h->drop_explicit)) {
    if (captured) *captured = -1;
    return forward_call(h, "forward_graph", B, img1, img2, choose1, choose2, P1, P2, depths, workspace, workspace_bytes, out, stream, call);
  }
  if (int rc = prepare_call(h, "forward_graph", B, {img1, img2, choose1, choose2, P1, P2, depths, workspace, out}, stream, &call)) return rc;
  hipStream_t s = call.stream;
  RGBM_REQUIRE(s != nullptr, "forward_graph: stream capture is not allowed on the default (null) stream; pass a created stream");
  auto forward = [&](const AdaPose::Call& c) {
    return h->net.forward(B, img1, img2, choose1, choose2, P1, P2, depths, workspace, workspace_bytes, to_out(out), c);
  };
  const void* in[7] = {img1, img2, choose1, choose2, P1, P2, depths};
  ForwardGraph* hit = nullptr;
  for (size_t i = 0; i < h->graphs.size();) {
    ForwardGraph& g = h->graphs[i];
    if (g.opt_version != h->opt_version || g.tuning_version != g_tuning_version) {      // settings changed since the capture
      drop_graph(g);
      h->graphs.erase(h->graphs.begin() + i);
      continue;
    }
    if (g.B == B && g.stream == s && !memcmp(g.in, in, sizeof(in)) && g.ws == workspace && g.ws_bytes == workspace_bytes &&
        !memcmp(&g.out, out, sizeof(*out))) hit = &g;
    ++i;
  }
  if (!hit) {
    // an eager forward first: it sets the dynamic-LDS attributes of the kernels this shape uses and loads their code objects (neither
    // may happen inside a capture), and reports argument errors with their own messages
    AdaPose::Call warm = call;      // with dropout the warm-up draws the masks the replay draws again: the pose counter advances once
    if (call.dropout == AdaPose::Dropout::Draw) warm.dropout = AdaPose::Dropout::DrawNoAdvance;
    if (int rw = forward(warm)) return rw;
    ForwardGraph g;
    g.B = B; g.stream = s; memcpy(g.in, in, sizeof(in)); g.ws = workspace; g.ws_bytes = workspace_bytes; g.out = *out;
    g.opt_version = h->opt_version; g.tuning_version = g_tuning_version;
    RGBM_CHECK_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    const int rc = forward(call);
    const hipError_t ee = hipStreamEndCapture(s, &g.graph);
    if (rc) { if (g.graph) (void)hipGraphDestroy(g.graph); return rc; }
    if (ee != hipSuccess || !g.graph) { set_error(std::string("hipStreamEndCapture: ") + hipGetErrorString(ee)); return -2; }
    if (hipGraphGetNodes(g.graph, nullptr, &g.nodes) != hipSuccess) g.nodes = 0;
    const hipError_t ei = hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0);
    if (ei != hipSuccess) { (void)hipGraphDestroy(g.graph); set_error(std::string("hipGraphInstantiate: ") + hipGetErrorString(ei)); return -2; }
    if (h->graphs.size() >= kMaxGraphs) {
      size_t lru = 0;
      for (size_t i = 1; i < h->graphs.size(); ++i) if (h->graphs[i].last_use < h->graphs[lru].last_use) lru = i;
      drop_graph(h->graphs[lru]);
      h->graphs.erase(h->graphs.begin() + lru);
    }
    h->graphs.push_back(g);
    hit = &h->graphs.back();
    if (captured) *captured = 1;
  }
  hit->last_use = ++h->tick;
  if (n_nodes) *n_nodes = (int32_t)hit->nodes;
  RGBM_CHECK_HIP(hipGraphLaunch(hit->exec, s));
  return finish_call(h, B, call, 0);
}

static_assert(sizeof(PathFacts) == RGBM_PATH_FACT_INTS * sizeof(int32_t) && sizeof(ForwardPaths) == RGBM_PATH_INTS * sizeof(int32_t),
              "rgbm.h documents PathFacts and ForwardPaths int by int");

int rgbm_forward_paths(const int32_t* facts, int n_rows, int32_t* paths) {
  RGBM_REQUIRE(facts && paths && n_rows > 0, "forward_paths arguments");
  for (int r = 0; r < n_rows; ++r) {
    PathFacts f;
    memcpy(&f, facts + (size_t)r * RGBM_PATH_FACT_INTS, sizeof(f));
    if (f.flags < 0) f.flags = g_debug_flags;
    const ForwardPaths p = forward_paths(f);
    memcpy(paths + (size_t)r * RGBM_PATH_INTS, &p, sizeof(p));
  }
  return 0;
}

int rgbm_adapose_paths(rgbm_adapose_t* h, int B, int dense, int32_t* facts_out, int32_t* paths_out) {
  RGBM_REQUIRE(h && B > 0 && (dense == 0 || dense == 1) && facts_out && paths_out, "adapose_paths arguments");
  const PathFacts f = h->net.path_facts(B, dense != 0);
  const ForwardPaths p = forward_paths(f);
  memcpy(facts_out, &f, sizeof(f));
  memcpy(paths_out, &p, sizeof(p));
  return 0;
}

int rgbm_adapose_fetch(rgbm_adapose_t* h, int B, void* workspace, const char* name, float* out_dev, size_t capacity,
                       size_t* n_elems, void* stream) {
  RGBM_REQUIRE(h && workspace && name && out_dev && n_elems, "fetch arguments");
  const AdaPose& n = h->net;
  const ForwardPaths p = n.paths(B);      // of a plain forward issued now: what the forward whose workspace this is ran, unless options or flags changed since
  Arena A(workspace, 0);
  AdaPose::Buffers bf;
  n.plan(B, p, A, bf);
  const size_t V = 2 * (size_t)B, S = n.img, P = n.n_pts, D = n.n_depth;
  const size_t Vc = n.chunk_views((int)V);
  const std::string nm = name;
  const void* src = nullptr; size_t cnt = 0; int dt = n.dtype;
  if (nm == "imgpad") { src = bf.imgpad; cnt = V * S * S * n.img_cpad; }
  else if (nm == "conv1") { src = bf.c1; cnt = V * (S / 2) * (S / 2) * 64; }
  else if (nm == "layer4") { src = bf.lb[n.layer4_index()]; cnt = V * (S / 8) * (S / 8) * 512; }
  else if (nm == "cat") { src = bf.cat; cnt = V * (S / 8) * (S / 8) * 1024; }
  else if (nm == "u1") { src = bf.u1; cnt = V * (S / 4) * (S / 4) * 256; }
  else if (nm == "u2") { src = bf.u2; cnt = V * (S / 2) * (S / 2) * 64; }
  else if (nm == "u3") { src = bf.u3; cnt = V * S * S * 64; }
  else if (nm == "feat") { src = bf.feat; cnt = V * S * S * 32; if (p.feat_form == FEAT_F32_ONLY) { src = bf.featf; dt = F32; } else if (p.feat_form == FEAT_F16) dt = F16; }
  else if (nm == "vol") { src = bf.vol; cnt = Vc * D * S * S * 32; }
  else if (nm == "homog") { src = bf.homog; cnt = V * 12; dt = F32; }
  else if (nm == "prob") { src = bf.prob; cnt = V * P * D; dt = F32; }
  // pf96: after a forward of a split-pair net the buffer holds hi / lo pairs (adapose.cpp converts it in place for the pose MLP)
  else if (nm == "pf96") { src = bf.PF96; cnt = V * P * n.pose_in(); dt = n.pose_dtype() == BF16X3 ? BF16X3 : F32; }
  else if (nm == "pf2") { src = bf.pf2; cnt = V * 256; dt = F32; }
  else if (nm == "r6") { src = bf.r6; cnt = V * 6; dt = F32; }
  // the v2 network's per-point head (v2_head.hip): pose_mlp1's rows, fuse_conv's output and volume_conv's 24 plane values at the chosen pixels
  else if (nm == "v2_rows" && is_v2(h)) { src = bf.X1; cnt = V * P * 64; dt = F32; }
  else if (nm == "v2_fuse" && is_v2(h)) { src = bf.H64; cnt = V * P * 64; dt = F32; }
  else if (nm == "v2_planes" && is_v2(h)) { src = bf.prob; cnt = V * P * D; dt = F32; }
  // the v1 network's stages A and B (v1_head.hip, point_mlp_kernel's rows variant): the residual rows, volume_conv's plane values and the
  // 128-channel pose rows (split pairs behind a whole forward of a split-pair net, as pf96)
  else if (nm == "v1_fused" && is_v1(h)) { src = bf.X0; cnt = V * P * 32; dt = F32; }
  else if (nm == "v1_planes" && is_v1(h)) { src = bf.prob; cnt = V * P * D; dt = F32; }
  else if (nm == "v1_rows" && is_v1(h)) { src = bf.PF96; cnt = V * P * 128; dt = n.pose_dtype() == BF16X3 ? BF16X3 : F32; }
  else if (nm == "fused1" && bf.fused) { src = bf.fused; cnt = (size_t)B * P * 32; dt = F32; }
  else if (nm == "fused2" && bf.fused) { src = bf.fused + (size_t)B * P * 32; cnt = (size_t)B * P * 32; dt = F32; }
  // the taps of the cost regularisation: the outputs of these rows of kCost3d
  static const struct { const char* name; int row; } taps3d[] = {{"c0", 0}, {"c2", 2}, {"c4", 4}, {"c6", 6}, {"u7", 7}, {"u9", 8}, {"u11", 9}};
  int row3d = -1;
  for (const auto& t : taps3d)
    if (nm == t.name) { row3d = t.row; src = bf.c3[row3d]; cnt = cost3d_out_elems(row3d, (int)Vc, (int)D, (int)S); }
  if (is_baseline(h))      // the cost-volume buffers do not exist in this handle's workspace
    RGBM_REQUIRE(nm == "feat" || nm == "fused1" || nm == "fused2" || nm == "pf96" || nm == "pf2" || nm == "r6" || nm == "layer4" || nm == "cat" ||
                 nm == "u1" || nm == "u2", "tap '" + nm + "' does not exist in the baseline network");
  if (is_v2(h))      // neither the cost-volume buffers nor v5's pose buffers are written in this handle's workspace
    RGBM_REQUIRE(nm == "feat" || nm == "homog" || nm == "v2_rows" || nm == "v2_fuse" || nm == "v2_planes" || nm == "layer4" || nm == "cat" || nm == "u1" ||
                 nm == "u2", "tap '" + nm + "' does not exist in the v2 network");
  if (is_v1(h))      // no cost-volume buffers in this handle's workspace
    RGBM_REQUIRE(nm == "feat" || nm == "homog" || nm == "v1_fused" || nm == "v1_planes" || nm == "v1_rows" || nm == "pf2" || nm == "r6" || nm == "layer4" ||
                 nm == "cat" || nm == "u1" || nm == "u2", "tap '" + nm + "' does not exist in the v1 network");
  RGBM_REQUIRE(src != nullptr, "unknown intermediate name: " + nm);
  // with sparse cost regularisation c0..c5 / u7 / u9 are written only inside the chosen pixels' dependency cones (and c6 is computed
  // from them): the rest of these tensors is whatever the workspace held, so a tap of them is refused instead of returned partly stale
  const bool tap3d = row3d >= 0 && row3d < 9;      // u11 exists only with the dense tail, which computes all of it
  RGBM_REQUIRE(!(tap3d && p.mask_level > 0), "tap '" + nm + "' needs a dense cost regularisation: set option sparse_dec = 0 before the forward "
               "(the default computes it only inside the chosen pixels' dependency cones)");
  *n_elems = cnt;
  RGBM_REQUIRE(cnt <= capacity, "fetch capacity too small");
  return launch_to_f32(dt, src, out_dev, (long long)cnt, (hipStream_t)stream);
}

int rgbm_adapose_postprocess(int B, int P, int img_size, const float* nocs1, const float* depth1, const float* r1,
                             const int32_t* choose1, const double* Kcrop, const double* E1, double* bbox_world, double* ts,
                             int32_t* valid, void* stream) {
  RGBM_REQUIRE(B > 0 && nocs1 && depth1 && r1 && choose1 && Kcrop && E1 && bbox_world && ts && valid, "postprocess arguments");
  return launch_postprocess(nocs1, depth1, r1, choose1, Kcrop, E1, bbox_world, ts, valid, B, P, img_size, (hipStream_t)stream);
}

int rgbm_adapose_postprocess_scratch_bytes(int B, size_t* bytes) {
  RGBM_REQUIRE(B > 0 && bytes, "postprocess_scratch_bytes arguments");
  *bytes = postprocess_slices(B) > 1 ? postprocess_scratch_bytes(B) : 0;
  return 0;
}

int rgbm_adapose_postprocess_ws(int B, int P, int img_size, const float* nocs1, const float* depth1, const float* r1,
                                const int32_t* choose1, const double* Kcrop, const double* E1, double* bbox_world, double* ts,
                                int32_t* valid, void* scratch, size_t scratch_bytes, void* stream) {
  RGBM_REQUIRE(B > 0 && nocs1 && depth1 && r1 && choose1 && Kcrop && E1 && bbox_world && ts && valid, "postprocess arguments");
  return launch_postprocess(nocs1, depth1, r1, choose1, Kcrop, E1, bbox_world, ts, valid, B, P, img_size, (hipStream_t)stream,
                            scratch, scratch_bytes);
}

int rgbm_adapose_postprocess_ransac(int B, int P, int img_size, uint32_t seed, const float* nocs1, const float* depth1,
                                    const int32_t* choose1, const double* Kcrop, const double* E1, double* bbox_world, double* srt,
                                    int32_t* valid, void* stream) {
  return launch_umeyama_ransac(nocs1, depth1, choose1, Kcrop, E1, bbox_world, srt, valid, B, P, img_size, seed, (hipStream_t)stream);
}

int rgbm_gae(int T, int N, const float* rewards, const uint8_t* dones, const float* values, const float* last_values,
             float gamma, float lam, float* returns, float* adv, double* sums, void* stream) {
  RGBM_REQUIRE(rewards && dones && values && last_values && returns && adv && sums, "gae arguments");
  return launch_gae(T, N, rewards, dones, values, last_values, gamma, lam, returns, adv, sums, (hipStream_t)stream);
}

int rgbm_adv_normalise(int64_t n_local, float* adv, const double* sums, double count_total, void* stream) {
  RGBM_REQUIRE(adv && sums && n_local > 0 && count_total > 1.0, "adv_normalise arguments");
  return launch_adv_normalise(n_local, adv, sums, count_total, (hipStream_t)stream);
}

// The one-shot entry points below (tests) build a layer, run it and free it; their launches share ONE ConvScratch that lives as long as
// the process, so consecutive calls on a stream see the K-split counters the previous call left (zero), as a net's launches do.  Never
// destroyed: nothing is freed behind the runtime's own teardown at exit.
static const std::shared_ptr<ConvScratch>& one_shot_scratch() {
  static const auto* const scratch = new std::shared_ptr<ConvScratch>(std::make_shared<ConvScratch>());
  return *scratch;
}

static ConvGeom conv_nd_geom(int Cin, int Cout, int KD, int KH, int KW, int stride_d, int stride_hw, int pad_d, int pad_hw, int dil_hw,
                             int transposed, int act, float slope) {
  ConvGeom g;
  g.Cin = Cin; g.Cout = Cout; g.KD = KD; g.KH = KH; g.KW = KW;
  g.sd = stride_d; g.sh = g.sw = stride_hw; g.pd = pad_d; g.ph = g.pw = pad_hw;
  g.dild = 1; g.dilh = g.dilw = dil_hw; g.transposed = transposed != 0; g.act = act; g.slope = slope;
  return g;
}

int rgbm_conv_nd(int dtype, const void* in_dev, int N, int D, int H, int W, int Cin, int Cin_pad, const float* w_host,
                 int Cout, int Cout_pad, int KD, int KH, int KW, int stride_d, int stride_hw, int pad_d, int pad_hw,
                 int dil_hw, int transposed, const float* bias_host, const float* bn_scale_host, const float* bn_shift_host,
                 const void* res_dev, int res_mode, int act, float slope, void* out_dev, void* stream) {
  RGBM_REQUIRE(in_dev && w_host && out_dev, "conv arguments");
  const ConvGeom g = conv_nd_geom(Cin, Cout, KD, KH, KW, stride_d, stride_hw, pad_d, pad_hw, dil_hw, transposed, act, slope);
  ConvLayer L;
  if (int rc = L.init(dtype, g, w_host, bias_host, bn_scale_host, bn_shift_host, Cin_pad, Cout_pad, one_shot_scratch())) return rc;
  return finish_one_shot(L.run(in_dev, out_dev, N, D, H, W, Cout_pad, res_dev, res_mode, nullptr, 0, (hipStream_t)stream), stream);
}

int rgbm_conv_plan(int dtype, int N, int D, int H, int W, int Cin, int Cin_pad, int Cout, int Cout_pad, int KD, int KH, int KW,
                   int stride_d, int stride_hw, int pad_d, int pad_hw, int dil_hw, int transposed, int has_bias, int res_mode, int act,
                   int cls, int n_cu, int32_t* plan) {
  RGBM_REQUIRE(plan && n_cu >= 0 && dtype >= F32 && dtype <= BF16X3 && N > 0 && D > 0 && H > 0 && W > 0, "conv_plan arguments");
  const ConvGeom g = conv_nd_geom(Cin, Cout, KD, KH, KW, stride_d, stride_hw, pad_d, pad_hw, dil_hw, transposed, act, 0.f);
  PackedConv pc;
  if (int rc = conv_pack_geom(g, dtype, Cin_pad, Cout_pad, cls, &pc)) return rc;
  ConvDesc d;
  conv_desc_geom(d, g, pc, Cin_pad, Cout_pad, N, D, H, W, Cout_pad, cls);
  alignas(16) static const float buffer[4] = {};      // stands for every device buffer: never read, 16-byte aligned as rgbm_conv_nd's callers' are
  d.in = d.wgt = buffer; d.out = const_cast<float*>(buffer);
  d.bias = has_bias ? buffer : nullptr;
  d.res = res_mode != RES_NONE ? buffer : nullptr;
  d.res_mode = res_mode;
  ConvTuning t;
  ConvPlan p;
  if (int rc = conv_tuning(n_cu, &t)) return rc;
  if (int rc = plan_conv(d, dtype, t, &p)) return rc;
  const int32_t v[RGBM_CONV_PLAN_INTS] = {p.kernel, p.bch, p.bpix, p.ksplit, (int32_t)p.main_rows, p.tail_bch, p.identity_residual, (int32_t)d.M, d.KT};
  memcpy(plan, v, sizeof(v));
  return 0;
}

int rgbm_conv_border_plan(int dtype, int N, int H, int W, int Cin, int Cout, int K, int stride, int pad, int dil, int res_mode, int n_cu,
                          int32_t* head, int32_t* classes, int cap_classes, int32_t* tiles, int32_t* order, int cap_tiles, int32_t* wg_off,
                          int cap_wg, int32_t* rows, int64_t cap_rows) {
  RGBM_REQUIRE(head && n_cu >= 0 && dtype >= F32 && dtype <= BF16X3 && N > 0 && H > 0 && W > 0 && K > 0, "conv_border_plan arguments");
  const ConvGeom g = conv_nd_geom(Cin, Cout, 1, K, K, 1, stride, 0, pad, dil, 0, ACT_RELU, 0.f);
  PackedConv pc;
  const int E = dtype_chunk(dtype);
  const int Cin_pad = (Cin + E - 1) / E * E, Cout_pad = (Cout + 3) / 4 * 4;
  if (int rc = conv_pack_geom(g, dtype, Cin_pad, Cout_pad, 0, &pc)) return rc;
  ConvDesc d;
  conv_desc_geom(d, g, pc, Cin_pad, Cout_pad, N, 1, H, W, Cout_pad, 0);
  alignas(16) static const float buffer[4] = {};      // stands for every device buffer, as in rgbm_conv_plan
  d.in = d.wgt = buffer; d.out = const_cast<float*>(buffer);
  d.res = res_mode != RES_NONE ? buffer : nullptr;
  d.res_mode = res_mode;
  d.w_finite = 1;
  ConvTuning t;
  ConvPlan p;
  if (int rc = conv_tuning(n_cu, &t)) return rc;
  if (int rc = plan_conv(d, dtype, t, &p)) return rc;
  memset(head, 0, RGBM_BORDER_HEAD_INTS * sizeof(int32_t));
  BorderPlan bp;
  if (p.kernel != CONV_M32 || !p.border || !plan_border(d, dtype, t.flags, p.main_rows, t.n_cu, &bp)) return 0;
  const int32_t h[RGBM_BORDER_HEAD_INTS] = {1, (int32_t)bp.classes.size(), (int32_t)bp.tiles.size(), bp.n_wg, (int32_t)bp.rows.size(),
                                             (int32_t)bp.max_wg_steps, (int32_t)bp.total_steps, (int32_t)bp.parent_steps, bp.steps_per_tap, bp.kr};
  memcpy(head, h, sizeof(h));
  if (classes) {
    RGBM_REQUIRE((int)bp.classes.size() <= cap_classes, "conv_border_plan: cap_classes too small");
    for (size_t c = 0; c < bp.classes.size(); ++c) {
      classes[3 * c] = bp.classes[c].n_pix; classes[3 * c + 1] = bp.classes[c].mask; classes[3 * c + 2] = (int32_t)bp.classes[c].row0;
    }
  }
  if (tiles || order) RGBM_REQUIRE((int)bp.tiles.size() <= cap_tiles, "conv_border_plan: cap_tiles too small");
  if (tiles)
    for (size_t i = 0; i < bp.tiles.size(); ++i) {
      const BorderTile& bt = bp.tiles[i];
      const int32_t v[5] = {bt.cls, bt.ch, bt.mask, bt.steps, (int32_t)bt.row0};
      memcpy(tiles + 5 * i, v, sizeof(v));
    }
  if (order) memcpy(order, bp.order.data(), bp.order.size() * sizeof(int32_t));
  if (wg_off) {
    RGBM_REQUIRE(bp.n_wg + 1 <= cap_wg, "conv_border_plan: cap_wg too small");
    memcpy(wg_off, bp.wg_off.data(), bp.wg_off.size() * sizeof(int32_t));
  }
  if (rows) {
    RGBM_REQUIRE((int64_t)bp.rows.size() <= cap_rows, "conv_border_plan: cap_rows too small");
    memcpy(rows, bp.rows.data(), bp.rows.size() * sizeof(int32_t));
  }
  return 0;
}

int rgbm_conv_border_launches(int64_t* count) {
  RGBM_REQUIRE(count, "conv_border_launches arguments");
  *count = border_launch_count();
  return 0;
}

int rgbm_upsample_conv3x3(int dtype, const void* in_dev, int V, int h, int w, int Cin, const float* w_host, int Cout,
                          const float* bias_host, int act, float slope, void* z_scratch_dev, void* out_dev, void* stream) {
  RGBM_REQUIRE(in_dev && w_host && z_scratch_dev && out_dev, "upsample_conv3x3 arguments");
  UpConvLayer L;
  if (int rc = L.init(dtype, Cin, Cout, w_host, bias_host, act, slope, one_shot_scratch())) return rc;
  return finish_one_shot(L.run(in_dev, z_scratch_dev, out_dev, V, h, w, Cout, (hipStream_t)stream), stream);
}

int rgbm_upsample_conv3x3_final(int dtype, const void* in_dev, int V, int h, int w, const float* w3_host, const float* b3_host,
                                float slope, const float* wf_host, const float* bf_host, void* out_dev, int out_f32, void* stream) {
  RGBM_REQUIRE(in_dev && w3_host && b3_host && wf_host && bf_host && out_dev, "upsample_conv3x3_final arguments");
  UpConvFinal L;
  if (int rc = L.init(dtype, w3_host, b3_host, slope, wf_host, bf_host)) return rc;
  return finish_one_shot(L.run(in_dev, out_dev, out_f32, V, h, w, (hipStream_t)stream), stream);
}

int rgbm_stem(int dtype, const float* img1_dev, const float* img2_dev, const float* w_host, void* out_dev, int B, int S, void* stream) {
  RGBM_REQUIRE(img1_dev && img2_dev && w_host && out_dev && B > 0, "stem arguments");
  std::vector<float> pk;
  stem_pack(w_host, pk);
  DevBuf wd;
  if (int rc = upload_packed(pk, dtype, wd)) return rc;
  return finish_one_shot(launch_stem(dtype, img1_dev, img2_dev, wd.get(), out_dev, B, 2 * B, S, (hipStream_t)stream), stream);
}

int rgbm_bn_per_sample_scratch_bytes(int V, size_t* bytes) {
  RGBM_REQUIRE(V > 0 && bytes, "bn_per_sample_scratch_bytes arguments");
  *bytes = bn_scratch_bytes(V);
  return 0;
}
int rgbm_bn_per_sample(int dtype, void* y_dev, const void* res_dev, const float* gamma_dev, const float* beta_dev, void* scratch_dev,
                       int V, int64_t nvox, int C, int relu, void* stream) {
  RGBM_REQUIRE(y_dev && gamma_dev && beta_dev && scratch_dev, "bn_per_sample arguments");
  return launch_bn_per_sample(dtype, y_dev, res_dev, gamma_dev, beta_dev, scratch_dev, V, (long long)nvox, C, relu, (hipStream_t)stream);
}
int rgbm_maxpool3x3s2(int dtype, const void* in_dev, void* out_dev, int V, int H, int W, int C, void* stream) {
  return launch_maxpool3x3s2(dtype, in_dev, out_dev, V, H, W, C, (hipStream_t)stream);
}
int rgbm_resize_bilinear_ac(int dtype, const void* in_dev, void* out_dev, int V, int Hs, int Ws, int C, int Ho, int Wo,
                            void* stream) {
  return launch_resize_bilinear_ac(dtype, in_dev, out_dev, V, Hs, Ws, C, Ho, Wo, C, 0, (hipStream_t)stream);
}
int rgbm_adaptive_avgpool(int dtype, const void* in_dev, void* out_dev, int V, int H, int W, int C, int S, void* stream) {
  return launch_adaptive_avgpool(dtype, in_dev, out_dev, V, H, W, C, S, (hipStream_t)stream);
}
int rgbm_build_volume(int dtype, const void* feat_dev, const float* P_views_dev, const float* depths_dev, float* homog_scratch,
                      void* vol_dev, int V, int B, int D, int H, int W, void* stream) {
  if (int rc = launch_homography(P_views_dev, homog_scratch, V, B, (hipStream_t)stream)) return rc;
  return launch_build_volume(dtype, feat_dev, homog_scratch, depths_dev, vol_dev, 0, V, V, B, D, H, W, (hipStream_t)stream);
}
int rgbm_build_volume_fusion(int dtype, int fusion, const void* feat_dev, const float* P_views_dev, const float* depths_dev, float* homog_scratch,
                             void* vol_dev, int V, int B, int D, int H, int W, void* stream) {
  if (int rc = launch_homography(P_views_dev, homog_scratch, V, B, (hipStream_t)stream)) return rc;
  return launch_build_volume(dtype, feat_dev, homog_scratch, depths_dev, vol_dev, 0, V, V, B, D, H, W, (hipStream_t)stream, fusion);
}

}  // extern "C"

#include "prof.h"
extern "C" {
int rgbm_prof_rows(void) { return rgbm::kProfVariants; }
int rgbm_microbench_mfma_scratch_floats(int* n) {
  RGBM_REQUIRE(n, "microbench_mfma_scratch_floats arguments");
  return rgbm::microbench_mfma_scratch_floats(n);
}
int rgbm_microbench_mfma(float* scratch, int iters, int random_operands, double* flops, void* stream) {
  return rgbm::launch_microbench_mfma(scratch, iters, random_operands, flops, (hipStream_t)stream);
}
int rgbm_microbench_copy(const void* src, void* dst, size_t bytes, void* stream) {
  return rgbm::launch_microbench_copy(src, dst, bytes, (hipStream_t)stream);
}
int rgbm_prof_start(void) { return rgbm::prof_start(); }
int rgbm_prof_select(int row) {
  RGBM_REQUIRE(row >= -1 && row < rgbm::kProfVariants, "prof_select: row out of range");
  return rgbm::prof_select(row);
}
int rgbm_prof_stop(double* stats) {
  RGBM_REQUIRE(stats != nullptr, "prof_stop arguments");
  return rgbm::prof_stop(stats, rgbm::kProfVariants);
}
}

// Layer-level entry for the halo-tiled 3-D conv (tests): layer 0..6 = conv0..conv6, 7..9 = conv7/9/11 (transposed).
extern "C" int rgbm_conv3d_tile(int layer, int dtype, const void* in_dev, int N, int D, int H, int W, const float* w_host,
                                const float* bn_scale_host, const float* bn_shift_host, const void* res_dev, void* out_dev,
                                void* stream) {
  RGBM_REQUIRE(layer >= 0 && layer < kCost3dLayers && in_dev && w_host && bn_scale_host && bn_shift_host && out_dev, "conv3d_tile arguments");
  const Cost3dLayer& L = kCost3d[layer];
  const int coutp = cost3d_coutp(layer);
  std::vector<float> packed;
  conv3d_tile_pack(w_host, bn_scale_host, L.cin, L.cout, coutp, L.transposed, dtype, packed);
  DevBuf wdev, bdev;
  if (upload_packed(packed, dtype, wdev)) return -2;
  std::vector<float> bpad(coutp, 0.f);
  for (int o = 0; o < L.cout; ++o) bpad[o] = bn_shift_host[o];
  if (upload_f32(bpad.data(), bpad.size(), bdev)) return -2;
  Conv3dTileDesc d;
  memset(&d, 0, sizeof(d));
  d.in = in_dev; d.wgt = wdev.get(); d.out = out_dev; d.bias = bdev.get<float>(); d.res = res_dev;
  d.N = N; d.Di = D; d.Hi = H; d.Wi = W;
  if (L.transposed) { d.Do = 2 * D; d.Ho = 2 * H; d.Wo = 2 * W; d.Dq = D; d.Hq = H; d.Wq = W; }
  else {
    const int s = L.stride;
    d.Do = (D + 2 - 3) / s + 1; d.Ho = (H + 2 - 3) / s + 1; d.Wo = (W + 2 - 3) / s + 1;
    d.Dq = d.Do; d.Hq = d.Ho; d.Wq = d.Wo;
  }
  d.Cout = L.cout; d.relu = 1; d.prof_variant = -1;
  return finish_one_shot(launch_conv3d_tile(layer, dtype, d, (hipStream_t)stream), stream);
}

// Kernel-level entry for the depth-sweeping conv0 + fused plane sweep (tests): bf16 features [V][H][W][32] -> [V][D][H][W][8].
static int conv0_sweep_entry(int dtype, int feat_f16, const void* feat_dev, const float* P_views_dev, const float* depths_dev,
                             float* homog_scratch, const float* w_host, const float* bn_scale_host, const float* bn_shift_host,
                             void* out_dev, int V, int B, int D, int H, int W, void* stream) {
  RGBM_REQUIRE(feat_dev && P_views_dev && depths_dev && homog_scratch && w_host && bn_scale_host && bn_shift_host && out_dev,
               "conv0_sweep arguments");
  RGBM_REQUIRE(dtype == BF16 || dtype == F16 || dtype == BF16X3, "conv0_sweep: 16-bit storage types or bf16x3 (fp32 features in, split-pair c0 out)");
  if (int rc = launch_homography(P_views_dev, homog_scratch, V, B, (hipStream_t)stream)) return rc;
  std::vector<float> packed;
  conv0_sweep_pack(w_host, bn_scale_host, packed);
  DevBuf wdev, bdev;
  if (dtype == BF16X3) { if (conv0_sweep_x3_upload(packed, wdev.out())) return -2; }
  else if (upload_packed(packed, feat_f16 ? (int)F16 : dtype, wdev)) return -2;
  std::vector<float> bpad(cost3d_coutp(0), 0.f);
  for (int o = 0; o < kCost3d[0].cout; ++o) bpad[o] = bn_shift_host[o];
  if (upload_f32(bpad.data(), bpad.size(), bdev)) return -2;
  Conv3dTileDesc d;
  memset(&d, 0, sizeof(d));
  d.wgt = wdev.get(); d.out = out_dev; d.bias = bdev.get<float>();
  d.N = V; d.Di = D; d.Hi = H; d.Wi = W; d.Do = D; d.Ho = H; d.Wo = W; d.Dq = D; d.Hq = H; d.Wq = W;
  d.Cout = kCost3d[0].cout; d.relu = 1; d.prof_variant = -1;
  d.feat = feat_dev; d.homog = homog_scratch; d.depths = depths_dev; d.v0 = 0; d.V = V; d.B = B;
  d.feat_f16 = feat_f16;
  return finish_one_shot(dtype == BF16X3 ? launch_conv0_sweep_x3(d, (hipStream_t)stream) : launch_conv0_sweep(d, dtype, (hipStream_t)stream), stream);
}

extern "C" int rgbm_conv0_sweep_dt(int dtype, const void* feat_dev, const float* P_views_dev, const float* depths_dev,
                                   float* homog_scratch, const float* w_host, const float* bn_scale_host, const float* bn_shift_host,
                                   void* out_dev, int V, int B, int D, int H, int W, void* stream) {
  return conv0_sweep_entry(dtype, 0, feat_dev, P_views_dev, depths_dev, homog_scratch, w_host, bn_scale_host, bn_shift_host, out_dev, V, B, D,
                           H, W, stream);
}

extern "C" int rgbm_conv0_sweep_f16feat(const void* feat_f16_dev, const float* P_views_dev, const float* depths_dev,
                                        float* homog_scratch, const float* w_host, const float* bn_scale_host,
                                        const float* bn_shift_host, void* out_bf16_dev, int V, int B, int D, int H, int W, void* stream) {
  return conv0_sweep_entry(BF16, 1, feat_f16_dev, P_views_dev, depths_dev, homog_scratch, w_host, bn_scale_host, bn_shift_host, out_bf16_dev,
                           V, B, D, H, W, stream);
}

extern "C" int rgbm_conv0_sweep(const void* feat_dev, const float* P_views_dev, const float* depths_dev, float* homog_scratch,
                                const float* w_host, const float* bn_scale_host, const float* bn_shift_host, void* out_dev,
                                int V, int B, int D, int H, int W, void* stream) {
  return rgbm_conv0_sweep_dt(BF16, feat_dev, P_views_dev, depths_dev, homog_scratch, w_host, bn_scale_host, bn_shift_host, out_dev,
                             V, B, D, H, W, stream);
}

// Batched device-side prepare_model_input (interface_v5.py:58-170); see include/rgbm.h.
extern "C" int rgbm_prepare_inputs(const float* rgb_dev, const uint8_t* mask_dev, const double* K_dev, int N, int H, int W, int S,
                                   int P, uint32_t seed, float* img_out, int32_t* choose_out, float* pts2d_out, double* Kcrop_out,
                                   int32_t* window_out, int32_t* valid_out, uint8_t* scratch, void* stream) {
  return launch_prepare_inputs(rgb_dev, mask_dev, K_dev, nullptr, N, H, W, S, P, seed, img_out, choose_out, pts2d_out, Kcrop_out,
                               window_out, valid_out, scratch, (hipStream_t)stream);
}

extern "C" int rgbm_prepare_inputs_indexed(const float* rgb_dev, const uint8_t* mask_dev, const double* K_dev,
                                           const int32_t* frame_map_dev, int N, int H, int W, int S, int P, uint32_t seed,
                                           float* img_out, int32_t* choose_out, float* pts2d_out, double* Kcrop_out,
                                           int32_t* window_out, int32_t* valid_out, uint8_t* scratch, void* stream) {
  RGBM_REQUIRE(frame_map_dev, "prepare_inputs_indexed frame_map");
  return launch_prepare_inputs(rgb_dev, mask_dev, K_dev, frame_map_dev, N, H, W, S, P, seed, img_out, choose_out, pts2d_out,
                               Kcrop_out, window_out, valid_out, scratch, (hipStream_t)stream);
}

extern "C" int rgbm_prepare_inputs_ex(const float* rgb_dev, const uint8_t* mask_dev, const double* K_dev, const int32_t* frame_map_dev,
                                      int frame0, int N, int H, int W, int S, int P, uint32_t seed, float* img_out, int32_t* choose_out,
                                      float* pts2d_out, double* Kcrop_out, int32_t* window_out, int32_t* valid_out, uint8_t* scratch,
                                      void* stream) {
  RGBM_REQUIRE(frame0 >= 0, "prepare_inputs_ex frame0");
  return launch_prepare_inputs(rgb_dev, mask_dev, K_dev, frame_map_dev, N, H, W, S, P, seed, img_out, choose_out, pts2d_out,
                               Kcrop_out, window_out, valid_out, scratch, (hipStream_t)stream, frame0);
}

extern "C" int rgbm_prepare_inputs_u8(const uint8_t* rgb_dev, const uint8_t* mask_dev, const double* K_dev, const int32_t* frame_map_dev,
                                      int frame0, int N, int H, int W, int S, int P, uint32_t seed, float* img_out, int32_t* choose_out,
                                      float* pts2d_out, double* Kcrop_out, int32_t* window_out, int32_t* valid_out, uint8_t* scratch,
                                      void* stream) {
  RGBM_REQUIRE(frame0 >= 0, "prepare_inputs_u8 frame0");
  return launch_prepare_inputs_u8(rgb_dev, mask_dev, K_dev, frame_map_dev, N, H, W, S, P, seed, img_out, choose_out, pts2d_out,
                                  Kcrop_out, window_out, valid_out, scratch, (hipStream_t)stream, frame0);
}

extern "C" int rgbm_prepare_inputs_opt(const void* rgb_dev, int pixel_type, int normalize, const uint8_t* mask_dev, const double* K_dev,
                                       const int32_t* frame_map_dev, int frame0, int N, int H, int W, int S, int P, uint32_t seed,
                                       float* img_out, int32_t* choose_out, float* pts2d_out, double* Kcrop_out, int32_t* window_out,
                                       int32_t* valid_out, uint8_t* scratch, void* stream) {
  RGBM_REQUIRE(frame0 >= 0, "prepare_inputs_opt frame0");
  return launch_prepare_inputs_opt(rgb_dev, pixel_type, normalize, mask_dev, K_dev, frame_map_dev, N, H, W, S, P, seed, img_out, choose_out,
                                   pts2d_out, Kcrop_out, window_out, valid_out, scratch, (hipStream_t)stream, frame0);
}

extern "C" int rgbm_prepare_inputs_native(const void* rgb_dev, int pixel_type, int normalize, const uint8_t* mask_dev, const double* K_dev,
                                          const int32_t* frame_map_dev, int frame0, int N, int H, int W, int S, int P, uint32_t seed,
                                          float* img_out, int32_t* choose_out, float* pts2d_out, double* Kcrop_out, int32_t* window_out,
                                          int32_t* valid_out, uint8_t* scratch, void* stream) {
  RGBM_REQUIRE(frame0 >= 0, "prepare_inputs_native frame0");
  return launch_prepare_inputs_native(rgb_dev, pixel_type, normalize, mask_dev, K_dev, frame_map_dev, N, H, W, S, P, seed, img_out, choose_out,
                                      pts2d_out, Kcrop_out, window_out, valid_out, scratch, (hipStream_t)stream, frame0);
}

extern "C" int rgbm_prepare_inputs_windows(const void* pix_dev, int pixel_type, int normalize, const uint8_t* mask_pix_dev,
                                           const int64_t* offset_dev, const int32_t* window_dev, const int32_t* valid_in_dev, const double* K_dev,
                                           int frame0, int N, int H, int W, int S, int P, uint32_t seed, float* img_out, int32_t* choose_out,
                                           float* pts2d_out, double* Kcrop_out, int32_t* valid_out, uint8_t* scratch, void* stream) {
  static_assert(sizeof(int64_t) == sizeof(long long), "offset table");
  return launch_prepare_inputs_windows(pix_dev, pixel_type, normalize, mask_pix_dev, reinterpret_cast<const long long*>(offset_dev), window_dev,
                                       valid_in_dev, K_dev, frame0, N, H, W, S, P, seed, img_out, choose_out, pts2d_out, Kcrop_out, valid_out,
                                       scratch, (hipStream_t)stream);
}

extern "C" int rgbm_adapose_postprocess_regressed(int B, int P, const float* nocs1, const float* r1, const float* t1, const float* s1,
                                                  const double* E1, double* bbox_out, double* ts_out, int32_t* valid_out, void* stream) {
  return launch_postprocess_regressed(nocs1, r1, t1, s1, E1, bbox_out, ts_out, valid_out, B, P, (hipStream_t)stream);
}

extern "C" int rgbm_quantize_frames(const float* src_dev, uint8_t* dst_dev, size_t n, void* stream) {
  return launch_quantize_frames(src_dev, dst_dev, n, (hipStream_t)stream);
}

extern "C" int rgbm_adapose_postprocess_pnp(int B, int P, uint32_t seed, const float* nocs1, const float* pts2d1, const float* nocs2,
                                            const float* pts2d2, const double* K, const double* E1, const double* E2, double* bbox_out,
                                            double* srt_out, int32_t* info_out, int32_t* valid_out, void* stream) {
  return launch_pnp_ransac(nocs1, pts2d1, nocs2, pts2d2, K, E1, E2, bbox_out, srt_out, info_out, valid_out, B, P, seed, (hipStream_t)stream);
}

extern "C" int rgbm_adapose_postprocess_pnp_scaled(int B, int P, uint32_t seed, const float* nocs1, const float* pts2d1, const float* s1,
                                                   const double* K, const double* E1, double* bbox_out, double* srt_out, int32_t* info_out,
                                                   int32_t* valid_out, void* stream) {
  return launch_pnp_scaled(nocs1, pts2d1, s1, K, E1, bbox_out, srt_out, info_out, valid_out, B, P, seed, (hipStream_t)stream);
}

extern "C" int rgbm_projection(const double* Kcrop_dev, const double* E_dev, float* P_dev, int N, void* stream) {
  return launch_projection(Kcrop_dev, E_dev, P_dev, N, (hipStream_t)stream);
}

extern "C" int rgbm_mask_extent(const uint8_t* mask_dev, int N, int H, int W, int32_t* ext_out, int32_t* count_out, void* stream) {
  return launch_mask_extent(mask_dev, N, H, W, ext_out, count_out, (hipStream_t)stream);
}

// ---- controller step (control.hip) and synthetic camera (synth_env.hip) ---------------------------------------------
static_assert(sizeof(rgbm_control_reward_args) == sizeof(rgbm::ControlRewardArgs), "control reward args ABI mismatch");
static_assert(sizeof(rgbm_synth_scene) == sizeof(rgbm::SynthScene), "synth scene ABI mismatch");
extern "C" int rgbm_lookat_quat(const double* dir_dev, int N, int batch_zero, double* quat_dev, void* stream) {
  return rgbm::launch_lookat_quat(dir_dev, quat_dev, N, batch_zero, (hipStream_t)stream);
}
extern "C" int rgbm_control_action_to_pose(const float* action_dev, int lda, const double* pose_mid, const double* pose_min,
                                           const double* pose_max, int N, double* pose_dev, void* stream) {
  return rgbm::launch_control_action(action_dev, lda, pose_mid, pose_min, pose_max, pose_dev, N, (hipStream_t)stream);
}
extern "C" int rgbm_control_reward(const rgbm_control_reward_args* args, void* stream) {
  RGBM_REQUIRE(args, "control_reward args");
  return rgbm::launch_control_reward(*reinterpret_cast<const rgbm::ControlRewardArgs*>(args), (hipStream_t)stream);
}
extern "C" int rgbm_control_grasp_frame(const double* est_dev, int N, double* center_dev, double* direction_dev, void* stream) {
  return rgbm::launch_control_grasp_frame(est_dev, center_dev, direction_dev, N, (hipStream_t)stream);
}
extern "C" int rgbm_synth_camera(const rgbm_synth_scene* scene, double* K_dev, double* E_dev, double* rays_dev, void* stream) {
  RGBM_REQUIRE(scene, "synth_camera scene");
  return rgbm::launch_synth_camera(*reinterpret_cast<const rgbm::SynthScene*>(scene), K_dev, E_dev, rays_dev, (hipStream_t)stream);
}
extern "C" int rgbm_synth_render(const rgbm_synth_scene* scene, const double* rays_dev, float* color_dev, uint8_t* mask_dev,
                                 void* stream) {
  RGBM_REQUIRE(scene, "synth_render scene");
  return rgbm::launch_synth_render(*reinterpret_cast<const rgbm::SynthScene*>(scene), rays_dev, color_dev, mask_dev,
                                   (hipStream_t)stream);
}
extern "C" int rgbm_synth_render_u8(const rgbm_synth_scene* scene, const double* rays_dev, uint8_t* color_dev, uint8_t* mask_dev,
                                    int32_t* extent_dev, int32_t* count_dev, void* stream) {
  RGBM_REQUIRE(scene, "synth_render_u8 scene");
  return rgbm::launch_synth_render_u8(*reinterpret_cast<const rgbm::SynthScene*>(scene), rays_dev, color_dev, mask_dev, extent_dev,
                                      count_dev, (hipStream_t)stream);
}

extern "C" int rgbm_debug_flags(int flags) { rgbm::g_debug_flags = flags; ++rgbm::g_tuning_version; return 0; }

extern "C" int rgbm_set_tuning(const char* key, long long value) {
  RGBM_REQUIRE(key != nullptr, "set_tuning arguments");
  const std::string k = key;
  if (k == "ws_min_rows") { RGBM_REQUIRE(value >= 0, "ws_min_rows"); rgbm::g_ws_min_rows = value; }
  else if (k == "gemm_kernel") { RGBM_REQUIRE(value >= 0 && value <= 2, "gemm_kernel"); rgbm::g_gemm_kernel = (int)value; }
  else { set_error("unknown tuning key " + k); return -1; }
  ++rgbm::g_tuning_version;
  return 0;
}

// ---- PPO policy -------------------------------------------------------------------------------------------------
static_assert(sizeof(rgbm_policy_layout) == sizeof(rgbm::PolicyLayout), "policy layout ABI mismatch");
static_assert(sizeof(rgbm::PolicyOptState) == 40 || sizeof(rgbm::PolicyOptState) == 48, "opt state size");
extern "C" {
int rgbm_policy_forward(const float* params, const rgbm_policy_layout* L, int n, int mode, const float* obs, const float* noise,
                        float* actions, float* logp, float* value, float* mu, void* stream) {
  RGBM_REQUIRE(params && L && obs && mu, "policy_forward arguments");
  RGBM_REQUIRE(mode == 1 || (logp && value && actions), "policy_forward outputs");
  RGBM_REQUIRE(mode != 0 || noise, "policy_forward: act needs noise");
  return launch_policy_forward(params, *reinterpret_cast<const PolicyLayout*>(L), n, mode, obs, noise, actions, logp, value, mu,
                               (hipStream_t)stream);
}
int rgbm_ppo_partial_floats(const rgbm_policy_layout* L, int n, size_t* count) {
  RGBM_REQUIRE(L && count && n > 0, "ppo_partial_floats arguments");
  *count = (size_t)policy_partial_floats(*reinterpret_cast<const PolicyLayout*>(L), n);
  return 0;
}
int rgbm_ppo_minibatch_fwd_bwd(const float* params, const rgbm_policy_layout* L, int n, const float* obs, const float* actions,
                               const float* old_logp, const float* adv, const float* returns, const float* old_values,
                               const float* old_mu, const float* old_log_std, float clip, float vcoef, float ecoef,
                               float* partial_scratch, float* grads_flat, void* stream) {
  RGBM_REQUIRE(params && L && obs && actions && old_logp && adv && returns && old_values && old_mu && old_log_std &&
               partial_scratch && grads_flat, "ppo_minibatch arguments");
  return launch_ppo_minibatch(params, *reinterpret_cast<const PolicyLayout*>(L), n, obs, actions, old_logp, adv, returns,
                              old_values, old_mu, old_log_std, clip, vcoef, ecoef, partial_scratch, grads_flat, (hipStream_t)stream);
}
static_assert(sizeof(rgbm_policy_desc) == sizeof(rgbm::PolicyDesc), "policy desc ABI mismatch");
static_assert(RGBM_POLICY_MAX_HIDDEN == rgbm::POLICY_MAX_HIDDEN && RGBM_POLICY_MAX_WIDTH == rgbm::POLICY_MAX_WIDTH &&
                  RGBM_POLICY_MAX_ACT == rgbm::POLICY_MAX_ACT && RGBM_ACT_ELU == rgbm::PACT_ELU && RGBM_ACT_SIGMOID == rgbm::PACT_SIGMOID,
              "policy desc constants");

int rgbm_policy_forward_ex(const float* params, const rgbm_policy_desc* D, int n, int mode, const float* obs, const float* states,
                           const float* noise, float* actions, float* logp, float* value, float* mu, void* stream) {
  RGBM_REQUIRE(params && D && obs && mu, "policy_forward_ex arguments");
  RGBM_REQUIRE(mode == 1 || (logp && value && actions), "policy_forward_ex outputs");
  RGBM_REQUIRE(mode != 0 || noise, "policy_forward_ex: act needs noise");
  return launch_policy_forward_ex(params, *reinterpret_cast<const PolicyDesc*>(D), n, mode, obs, states, noise, actions, logp, value,
                                  mu, (hipStream_t)stream);
}
int rgbm_ppo_scratch_floats_ex(const rgbm_policy_desc* D, int n, int clipped_value_loss, size_t* count) {
  RGBM_REQUIRE(D && count && n > 0, "ppo_scratch_floats_ex arguments");
  return ppo_scratch_floats_ex(*reinterpret_cast<const PolicyDesc*>(D), n, clipped_value_loss, count);
}
int rgbm_ppo_minibatch_fwd_bwd_ex(const float* params, const rgbm_policy_desc* D, int n, const float* obs, const float* states,
                                  const float* actions, const float* old_logp, const float* adv, const float* returns,
                                  const float* old_values, const float* old_mu, const float* old_sigma, float clip, float vcoef,
                                  float ecoef, int clipped_value_loss, float* scratch, float* grads_flat, void* stream) {
  RGBM_REQUIRE(params && D && obs && actions && old_logp && adv && returns && old_mu && old_sigma && scratch && grads_flat,
               "ppo_minibatch_ex arguments");
  return launch_ppo_minibatch_ex(params, *reinterpret_cast<const PolicyDesc*>(D), n, obs, states, actions, old_logp, adv, returns,
                                 old_values, old_mu, old_sigma, clip, vcoef, ecoef, clipped_value_loss, scratch, grads_flat,
                                 (hipStream_t)stream);
}
int rgbm_ppo_clip_adam_ex(float* params, const float* grads_flat, float* exp_avg, float* exp_avg_sq, void* opt_state, int total,
                          float inv_world, float max_norm, float desired_kl, float lr_min, float lr_max, int adaptive, void* stream) {
  RGBM_REQUIRE(params && grads_flat && exp_avg && exp_avg_sq && opt_state && total > 0, "ppo_clip_adam_ex arguments");
  return launch_ppo_adam(params, grads_flat, exp_avg, exp_avg_sq, reinterpret_cast<PolicyOptState*>(opt_state), total, inv_world,
                         max_norm, desired_kl, lr_min, lr_max, adaptive, (hipStream_t)stream);
}
int rgbm_ppo_clip_adam(float* params, const float* grads_flat, float* exp_avg, float* exp_avg_sq, void* opt_state,
                       const rgbm_policy_layout* L, float inv_world, float max_norm, float desired_kl, float lr_min,
                       float lr_max, int adaptive, void* stream) {
  RGBM_REQUIRE(params && grads_flat && exp_avg && exp_avg_sq && opt_state && L, "ppo_clip_adam arguments");
  return launch_ppo_adam(params, grads_flat, exp_avg, exp_avg_sq, reinterpret_cast<PolicyOptState*>(opt_state), L->total,
                         inv_world, max_norm, desired_kl, lr_min, lr_max, adaptive, (hipStream_t)stream);
}
}
