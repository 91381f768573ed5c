// AdaPose stereo pose network forward, orchestrated on one HIP stream.
// Follows /root/reference/models/pose_estimator/AdaPose/lib/network_v5.py:418-519 (eval mode) with an
// MI355X-first dataflow: channels-last tensors, BN folded into the 3-D convs, the probability conv and the
// depth-guided fusion evaluated only at the 1024 sampled pixels, the cost volume processed in view chunks
// so its footprint is bounded, the second half of pose_mlp2's first layer (global feature) turned into a
// per-view bias.  Views are ordered v = side*B + b (all view-1 images, then all view-2 images).
#include "adapose.h"
#include "../../include/rgbm.h"
#include "cost3d.h"
#include "sample_stats.h"
#include "view_fusion.h"

#include <math.h>
#include <string.h>

namespace rgbm {

static const int kLayerPlanes[4] = {64, 128, 256, 512};
static const int kLayerBlocks[4] = {3, 4, 6, 3};
static const int kLayerStride[4] = {1, 2, 1, 1};
static const int kLayerDil[4] = {1, 1, 2, 4};
static const int kPspBins[4] = {1, 2, 3, 6};

static const HostTensor* find(const StateDict& sd, const std::string& name) {
  auto it = sd.find(name);
  return it == sd.end() ? nullptr : &it->second;
}

#define GET(var, name)                                               \
  const HostTensor* var = find(sd, name);                            \
  RGBM_REQUIRE(var != nullptr, std::string("missing weight ") + (name))

static int init_conv2d(ConvLayer& L, const std::shared_ptr<ConvScratch>& scratch, int dtype, const StateDict& sd, const std::string& wname, const char* bname, int Cin,
                       int Cout, int k, int stride, int pad, int dil, int act, float slope, int Cin_pad) {
  GET(w, wname);
  RGBM_REQUIRE(w->numel() == (long long)Cout * Cin * k * k, "weight shape " + wname);
  const float* b = nullptr;
  if (bname) { GET(bt, std::string(bname)); b = bt->data; }
  ConvGeom g;
  g.Cin = Cin; g.Cout = Cout; g.KH = g.KW = k; g.sh = g.sw = stride; g.ph = g.pw = pad; g.dilh = g.dilw = dil;
  g.act = act; g.slope = slope;
  return L.init(dtype, g, w->data, b, nullptr, nullptr, Cin_pad, Cout, scratch);
}

static int bn_fold(const StateDict& sd, const std::string& p, int C, std::vector<float>& scale, std::vector<float>& shift) {
  GET(gm, p + "weight"); GET(bt, p + "bias"); GET(mu, p + "running_mean"); GET(var, p + "running_var");
  RGBM_REQUIRE(gm->numel() == C && bt->numel() == C && mu->numel() == C && var->numel() == C, "bn shape " + p);
  scale.resize(C); shift.resize(C);
  for (int i = 0; i < C; ++i) {
    const float inv = 1.0f / sqrtf(var->data[i] + 1e-5f);
    scale[i] = gm->data[i] * inv;
    shift[i] = bt->data[i] - mu->data[i] * scale[i];
  }
  return 0;
}

// a row of kCost3d as the generic implicit-GEMM layer sees it (k3 p1)
static ConvGeom cost3d_geom(const Cost3dLayer& L, int act) {
  ConvGeom g;
  g.Cin = L.cin; g.Cout = L.cout; g.KD = g.KH = g.KW = 3; g.sd = g.sh = g.sw = L.stride; g.pd = g.ph = g.pw = 1;
  g.transposed = L.transposed; g.act = act;
  return g;
}

static int init_linear(ConvLayer& L, const std::shared_ptr<ConvScratch>& scratch, const StateDict& sd, const std::string& p, int Cin, int Cout, int act, int Cin_pad,
                       int Cout_pad, const float* w_override = nullptr, int ldtype = F32) {
  GET(w, p + ".weight"); GET(b, p + ".bias");
  ConvGeom g;
  g.Cin = Cin; g.Cout = Cout; g.act = act;
  return L.init(ldtype, g, w_override ? w_override : w->data, b->data, nullptr, nullptr, Cin_pad, Cout_pad, scratch);
}

int AdaPose::create(const StateDict& sd, int dtype_, int norm_mode_) {
  dtype = dtype_;
  norm_mode = norm_mode_;
  if (int rc = create_backbone(sd)) return rc;
  if (int rc = create_cost(sd)) return rc;
  if (int rc = create_point_heads(sd, true)) return rc;
  return create_pose(sd);
}

// The baseline network (lib/network_baseline.py:523-669): the same PSPNet and point heads, the cost volume and the depth-guided fusion
// replaced by the cross-view attention stack and depth_head (view_fusion.hip); the pose branch only with regress_pose.
int AdaPose::create_baseline(const StateDict& sd, int dtype_, int regress_pose_) {
  dtype = dtype_;
  norm_mode = 0;
  arch = ARCH_BASELINE;
  regress_pose = regress_pose_;
  if (int rc = create_backbone(sd)) return rc;
  if (int rc = create_point_heads(sd, regress_pose != 0)) return rc;
  {
    std::vector<float> wv((size_t)kVfWeightFloats);
    for (int blk = 0; blk < kVfBlocks; ++blk)
      for (int dir = 0; dir < 2; ++dir)
        for (int l = 0; l < 4; ++l) {
          const std::string p = "view_fusion.blocks." + std::to_string(blk) + ".fusion" + std::to_string(dir + 1) + ".linears." + std::to_string(l);
          GET(w, p + ".weight"); GET(b, p + ".bias");
          RGBM_REQUIRE(w->numel() == kVfDim * kVfDim && b->numel() == kVfDim, "view_fusion weight shape " + p);
          float* dst = wv.data() + (size_t)((blk * 2 + dir) * 4 + l) * kVfLinearFloats;
          memcpy(dst, w->data, sizeof(float) * kVfDim * kVfDim);
          memcpy(dst + kVfDim * kVfDim, b->data, sizeof(float) * kVfDim);
        }
    if (upload_f32(wv.data(), wv.size(), vf_w)) return -2;
  }
  {
    std::vector<float> wd((size_t)kDepthHeadFloats);
    static const char* const names[3] = {"depth_head.0", "depth_head.2", "depth_head.4"};
    static const int cin[3] = {32, 64, 32}, cout[3] = {64, 32, 1}, woff[3] = {kDhW0, kDhW1, kDhW2}, boff[3] = {kDhB0, kDhB1, kDhB2};
    for (int l = 0; l < 3; ++l) {
      GET(w, std::string(names[l]) + ".weight"); GET(b, std::string(names[l]) + ".bias");
      RGBM_REQUIRE(w->numel() == (long long)cin[l] * cout[l] && b->numel() == cout[l], std::string("depth_head weight shape ") + names[l]);
      memcpy(wd.data() + woff[l], w->data, sizeof(float) * cin[l] * cout[l]);
      memcpy(wd.data() + boff[l], b->data, sizeof(float) * cout[l]);
    }
    if (upload_f32(wd.data(), wd.size(), dh_w)) return -2;
  }
  return regress_pose ? create_pose(sd) : 0;
}

// The real-world network (lib/network_realworld.py:133-232): v5's state dict plus camera_pts_mlp, pose_mlp1.0 128 wide.  Its per-point
// branch stops at the NOCS (layers 4 / 5 of the point kernel's table are zero); pose_rows_kernel runs both 3 -> 32 -> 64 MLPs.
int AdaPose::create_realworld(const StateDict& sd, int dtype_) {
  RGBM_REQUIRE(dtype_ != F16, "create_realworld: dtype fp16 is not implemented for the real-world network (a voxel of its cost volume is a product of "
               "two feature values, which squares their range, and f16 saturates at 65504): use fp32, bf16 or bf16x3");
  dtype = dtype_;
  norm_mode = 0;
  arch = ARCH_REALWORLD;
  if (int rc = create_backbone(sd)) return rc;
  if (int rc = create_cost(sd)) return rc;
  if (int rc = create_point_heads(sd, false)) return rc;
  {
    static const char* const names[4] = {"camera_pts_mlp.0", "camera_pts_mlp.2", "nocs_pts_mlp.0", "nocs_pts_mlp.2"};
    const float* w[4]; const float* b[4];
    for (int l = 0; l < 4; ++l) {
      GET(wt, std::string(names[l]) + ".weight"); GET(bt, std::string(names[l]) + ".bias");
      const int cin = l % 2 ? 32 : 3, cout = l % 2 ? 64 : 32;
      RGBM_REQUIRE(wt->numel() == (long long)cin * cout && bt->numel() == cout, std::string("pose rows MLP shape ") + names[l]);
      w[l] = wt->data; b[l] = bt->data;
    }
    std::vector<float> table((size_t)kPoseRowsFloats);
    pose_rows_pack(w, b, table.data());
    if (upload_f32(table.data(), table.size(), prow_w)) return -2;
  }
  return create_pose(sd);
}

// The v2 network (lib/network_v2.py:40-197): PSPNet, instance_color and nocs_head as v5's; volume_conv, fuse_conv and pose_mlp1 become the
// LDS image of v2_point_rows_kernel; pose_mlp2 (128 -> 128 -> 128) keeps its global half as a per-view bias, as create_pose does at 256;
// size_estimator 128 -> 128 -> 64 -> 3 sits in row 2 of head_w / head_b.  Every layer behind the feature map is fp32.
int AdaPose::create_v2(const StateDict& sd, int dtype_) {
  dtype = dtype_;
  norm_mode = 0;
  arch = ARCH_V2;
  if (int rc = create_backbone(sd)) return rc;
  if (int rc = create_point_heads(sd, false)) return rc;
  {
    V2HeadWeights m{};
    std::vector<float> scale[3], shift[3];
    static const int vc_in[3] = {32, 16, 8}, vc_out[3] = {16, 8, 1};
    for (int l = 0; l < 3; ++l) {
      const std::string p = "volume_conv." + std::to_string(l) + ".";
      GET(w, p + "conv.weight");
      RGBM_REQUIRE(w->numel() == (long long)vc_in[l] * vc_out[l], "weight shape " + p + "conv.weight");
      if (int rc = bn_fold(sd, p + "bn.", vc_out[l], scale[l], shift[l])) return rc;
      m.vc_w[l] = w->data; m.vc_scale[l] = scale[l].data(); m.vc_shift[l] = shift[l].data();
    }
    static const char* const fc[2] = {"fuse_conv.0", "fuse_conv.2"};
    static const char* const pm[2] = {"pose_mlp1.0", "pose_mlp1.2"};
    static const int fc_in[2] = {24, 32}, fc_out[2] = {32, 64};
    for (int l = 0; l < 2; ++l) {
      GET(fw, std::string(fc[l]) + ".weight"); GET(fb, std::string(fc[l]) + ".bias");
      RGBM_REQUIRE(fw->numel() == (long long)fc_in[l] * fc_out[l] && fb->numel() == fc_out[l], std::string("weight shape ") + fc[l]);
      GET(pw, std::string(pm[l]) + ".weight"); GET(pb, std::string(pm[l]) + ".bias");
      RGBM_REQUIRE(pw->numel() == 64 * 64 && pb->numel() == 64, std::string("weight shape ") + pm[l] + ": 64 x 64 expected");
      m.fc_w[l] = fw->data; m.fc_b[l] = fb->data; m.pm_w[l] = pw->data; m.pm_b[l] = pb->data;
    }
    std::vector<float> table((size_t)kV2HeadFloats);
    v2_head_pack(m, table.data());
    if (upload_f32(table.data(), table.size(), v2_w)) return -2;
  }
  {
    // pose_mlp2.0 sees cat(point row[64], global mean[64]); the global half becomes a per-view bias
    GET(w, "pose_mlp2.0.weight"); GET(b, "pose_mlp2.0.bias");
    RGBM_REQUIRE(w->numel() == 128 * 128 && b->numel() == 128, "pose_mlp2.0 shape: 128 x 128 expected");
    std::vector<float> wl(128 * 64);
    for (int o = 0; o < 128; ++o) for (int i = 0; i < 64; ++i) wl[o * 64 + i] = w->data[o * 128 + i];
    if (int rc = init_linear(pm2[0], scratch, sd, "pose_mlp2.0", 64, 128, ACT_RELU, 64, 128, wl.data(), F32)) return rc;
    if (upload_f32(w->data, 128 * 128, pm2_0_wfull)) return -2;
    if (upload_f32(b->data, 128, pm2_0_bias)) return -2;
    GET(w2, "pose_mlp2.2.weight");
    RGBM_REQUIRE(w2->numel() == 128 * 128, "pose_mlp2.2 shape: 128 x 128 expected");
    if (int rc = init_linear(pm2[1], scratch, sd, "pose_mlp2.2", 128, 128, ACT_RELU, 128, 128, nullptr, F32)) return rc;
  }
  const int dims[4] = {128, 128, 64, 3};
  for (int l = 0; l < 3; ++l) {
    GET(w, "size_estimator." + std::to_string(2 * l) + ".weight");
    GET(b, "size_estimator." + std::to_string(2 * l) + ".bias");
    RGBM_REQUIRE(w->numel() == (long long)dims[l] * dims[l + 1] && b->numel() == dims[l + 1], "size_estimator weight shape");
    if (upload_f32(w->data, w->numel(), head_w[2][l])) return -2;
    if (upload_f32(b->data, b->numel(), head_b[2][l])) return -2;
  }
  return 0;
}

// The v1 network (lib/network.py:39-218): PSPNet, instance_color, nocs_head and nocs_pts_mlp as v5's; volume_conv and fuse_conv (24 -> 32
// -> 32) become the LDS image of v1_fused_points_kernel; the pose branch is v5's on 128-channel rows (create_pose at pose_in() == 128).
int AdaPose::create_v1(const StateDict& sd, int dtype_) {
  dtype = dtype_;
  norm_mode = 0;
  arch = ARCH_V1;
  if (int rc = create_backbone(sd)) return rc;
  if (int rc = create_point_heads(sd, true)) return rc;
  {
    V1HeadWeights m{};
    std::vector<float> scale[3], shift[3];
    static const int vc_in[3] = {32, 16, 8}, vc_out[3] = {16, 8, 1};
    for (int l = 0; l < 3; ++l) {
      const std::string p = "volume_conv." + std::to_string(l) + ".";
      GET(w, p + "conv.weight");
      RGBM_REQUIRE(w->numel() == (long long)vc_in[l] * vc_out[l], "weight shape " + p + "conv.weight");
      if (int rc = bn_fold(sd, p + "bn.", vc_out[l], scale[l], shift[l])) return rc;
      m.vc_w[l] = w->data; m.vc_scale[l] = scale[l].data(); m.vc_shift[l] = shift[l].data();
    }
    static const char* const fc[2] = {"fuse_conv.0", "fuse_conv.2"};
    static const int fc_in[2] = {24, 32}, fc_out[2] = {32, 32};
    for (int l = 0; l < 2; ++l) {
      GET(fw, std::string(fc[l]) + ".weight"); GET(fb, std::string(fc[l]) + ".bias");
      RGBM_REQUIRE(fw->numel() == (long long)fc_in[l] * fc_out[l] && fb->numel() == fc_out[l], std::string("weight shape ") + fc[l]);
      m.fc_w[l] = fw->data; m.fc_b[l] = fb->data;
    }
    std::vector<float> table((size_t)kV1HeadFloats);
    v1_head_pack(m, table.data());
    if (upload_f32(table.data(), table.size(), v1_w)) return -2;
  }
  return create_pose(sd);
}

int AdaPose::create_backbone(const StateDict& sd) {
  const int E = dtype_chunk(dtype);
  img_cpad = E;                              // RGB padded to one 16-byte chunk
  const std::string fe = "img_extractor.feats.";
  if (int rc = init_conv2d(conv1, scratch, dtype, sd, fe + "conv1.weight", nullptr, 3, 64, 7, 2, 3, 1, ACT_RELU, 0.f, img_cpad)) return rc;
  if (dtype != F32) {
    GET(w1, fe + "conv1.weight");
    RGBM_REQUIRE(w1->numel() == 64 * 3 * 7 * 7, "conv1 shape");
    std::vector<float> pk;
    stem_pack(w1->data, pk);
    if (int rc = upload_packed(pk, dtype, stem_w)) return rc;
    // same-box A/B at batch 256 (tools/ab_option.py <dtype> stem 0 1): bf16 forward 56.58 -> 55.62 ms; split pairs 125.06 -> 124.68 ms
    // with 4-row tiles (8-row tiles: 79 KB of staging, 122.63 -> 122.91 ms)
    stem = 1;
  }
  int inpl = 64, nb = 0;
  for (int li = 0; li < 4; ++li) {
    for (int b = 0; b < kLayerBlocks[li]; ++b) {
      Block& blk = blocks[nb++];
      const int planes = kLayerPlanes[li];
      const int cin = b == 0 ? inpl : planes;
      const int stride = b == 0 ? kLayerStride[li] : 1;
      const int dil = b == 0 ? 1 : kLayerDil[li];      // block 0 never dilated (pspnet.py:59-62)
      const std::string p = fe + "layer" + std::to_string(li + 1) + "." + std::to_string(b) + ".";
      if (int rc = init_conv2d(blk.c1, scratch, dtype, sd, p + "conv1.weight", nullptr, cin, planes, 3, stride, dil, dil, ACT_RELU, 0.f, cin)) return rc;
      if (int rc = init_conv2d(blk.c2, scratch, dtype, sd, p + "conv2.weight", nullptr, planes, planes, 3, 1, dil, dil, ACT_RELU, 0.f, planes)) return rc;
      blk.has_ds = find(sd, p + "downsample.0.weight") != nullptr;
      if (blk.has_ds)
        if (int rc = init_conv2d(blk.ds, scratch, dtype, sd, p + "downsample.0.weight", nullptr, cin, planes, 1, stride, 0, 1, ACT_NONE, 0.f, cin)) return rc;
      blk.stride = stride; blk.planes = planes;
    }
    inpl = kLayerPlanes[li];
  }
  n_blocks = nb;
  for (int i = 0; i < 4; ++i)
    if (int rc = init_conv2d(psp[i], scratch, dtype, sd, "img_extractor.psp.stages." + std::to_string(i) + ".1.weight", nullptr, 512, 128, 1, 1, 0, 1, ACT_RELU, 0.f, 512)) return rc;
  struct { ConvLayer* L; const char* nm; int cin, cout; } ups[3] = {{&up1, "up_1", 1024, 256}, {&up2, "up_2", 256, 64}, {&up3, "up_3", 64, 64}};
  for (auto& u : ups) {
    const std::string p = std::string("img_extractor.") + u.nm + ".conv.";
    GET(sl, p + "1.weight");
    const std::string bn = p + "0.bias";
    if (int rc = init_conv2d(*u.L, scratch, dtype, sd, p + "0.weight", bn.c_str(), u.cin, u.cout, 3, 1, 1, 1, ACT_PRELU, sl->data[0], u.cin)) return rc;
    UpConvLayer* uc = u.L == &up1 ? &up1c : u.L == &up2 ? &up2c : nullptr;
    if (uc) {
      GET(w, p + "0.weight"); GET(b, bn);
      if (int rc = uc->init(dtype, u.cin, u.cout, w->data, b->data, ACT_PRELU, sl->data[0], scratch)) return rc;
    }
  }
  if (int rc = init_conv2d(fin, scratch, dtype, sd, "img_extractor.final.weight", "img_extractor.final.bias", 64, 32, 1, 1, 0, 1, ACT_NONE, 0.f, 64)) return rc;
  if (dtype != F32) {
    GET(w3, "img_extractor.up_3.conv.0.weight"); GET(b3, "img_extractor.up_3.conv.0.bias"); GET(s3, "img_extractor.up_3.conv.1.weight");
    GET(wf, "img_extractor.final.weight"); GET(bfin, "img_extractor.final.bias");
    if (int rc = tail.init(dtype, w3->data, b3->data, s3->data[0], wf->data, bfin->data)) return rc;
  }
  return 0;
}

int AdaPose::create_cost(const StateDict& sd) {
  const std::string cr = "cost_regularization.";
  // every row of kCost3d in its three forms: the generic layer with BatchNorm folded in, with norm_mode 1 the raw layer and its gamma /
  // beta, and the halo-tile pack (conv3d_tile.hip); conv0 and conv11 have further packs of their own
  for (int i = 0; i < kCost3dLayers; ++i) {
    const Cost3dLayer& L = kCost3d[i];
    const std::string p = cr + L.name + ".";
    GET(w, p + "conv.weight");
    RGBM_REQUIRE(w->numel() == (long long)L.cout * L.cin * 27, "weight shape " + p);
    std::vector<float> scale, shift, packed;
    if (int rc = bn_fold(sd, p + "bn.", L.cout, scale, shift)) return rc;
    if (int rc = c3d[i].init(dtype, cost3d_geom(L, ACT_RELU), w->data, nullptr, scale.data(), shift.data(), L.cin, L.cout, scratch)) return rc;
    if (norm_mode == 1) {
      GET(gm, p + "bn.weight"); GET(bt, p + "bn.bias");
      if (int rc = c3d_raw[i].init(dtype, cost3d_geom(L, ACT_NONE), w->data, nullptr, nullptr, nullptr, L.cin, L.cout, scratch)) return rc;
      if (upload_f32(gm->data, L.cout, bn_gamma[i])) return -2;
      if (upload_f32(bt->data, L.cout, bn_beta[i])) return -2;
    }
    const int coutp = cost3d_coutp(i);
    conv3d_tile_pack(w->data, scale.data(), L.cin, L.cout, coutp, L.transposed, dtype, packed);
    if (upload_packed(packed, dtype, t3d[i].w)) return -2;
    std::vector<float> bpad(coutp, 0.f);
    for (int o = 0; o < L.cout; ++o) bpad[o] = shift[o];
    if (upload_f32(bpad.data(), bpad.size(), t3d[i].bias)) return -2;
    if (i == 9 && dtype != F32) {
      // conv11 for the sparse tail (prob_sparse2_kernel): one operand per in-plane tap, both depth parities on the 16 MFMA rows
      std::vector<float> pt;
      prob_sparse_pack(w->data, scale.data(), pt);
      if (dtype == BF16X3) { if (conv0_sweep_x3_upload(pt, w11_taps.out())) return -2; }
      else if (upload_packed(pt, dtype, w11_taps)) return -2;
    }
    if (i == 9 && dtype == BF16X3) {
      // conv11 for the sparse tail (prob_sparse.hip): its step structure is the 16-bit kernels' (two taps x 16 channels per
      // MFMA), so the weights are packed in that geometry and split into hi / lo operand arrays
      std::vector<float> p16;
      conv3d_tile_pack(w->data, scale.data(), L.cin, L.cout, coutp, true, BF16, p16);
      if (conv0_sweep_x3_upload(p16, w11_x3.out())) return -2;
    }
    if (i == 0 && dtype != F32) {
      // the same conv0 weights in the depth-sweeping kernel's paired-tap fragment order (conv0_sweep.hip / conv0_sweep_x3.hip)
      conv0_sweep_pack(w->data, scale.data(), packed);
      if (dtype == BF16X3) { if (conv0_sweep_x3_upload(packed, sweep_w.out())) return -2; }
      else if (upload_packed(packed, dtype, sweep_w)) return -2;
      // the f16 form of the sweep (sweep_f16) only for weights that f16 can hold: otherwise sweep_w_f16 stays null and feat_f16() is false
      // (never for the real-world network: its variance volume has no f16 form)
      if (dtype == BF16 && arch != ARCH_REALWORLD && weights_fit_f16(packed) && upload_packed(packed, F16, sweep_w_f16)) return -2;
    }
  }
  {
    GET(w, cr + "prob.weight");
    RGBM_REQUIRE(w->numel() == 8 * 27, "prob weight shape");
    std::vector<float> wp(27 * 8);
    for (int c = 0; c < 8; ++c) for (int t = 0; t < 27; ++t) wp[t * 8 + c] = w->data[c * 27 + t];
    if (upload_f32(wp.data(), wp.size(), wprob)) return -2;
  }
  return 0;
}

// pts_mlp = false (the baseline network without its pose branch has no nocs_pts_mlp): layers 4 / 5 of the point kernel's table are zero
int AdaPose::create_point_heads(const StateDict& sd, bool pts_mlp) {
  // fp32 point heads as 1x1 convs
  if (int rc = init_linear(inst, scratch, sd, "instance_color.0", 32, 64, ACT_RELU, 32, 64)) return rc;
  if (int rc = init_linear(nh[0], scratch, sd, "nocs_head.0", 64, 128, ACT_RELU, 64, 128)) return rc;
  if (int rc = init_linear(nh[1], scratch, sd, "nocs_head.2", 128, 64, ACT_RELU, 128, 64)) return rc;
  if (int rc = init_linear(nh[2], scratch, sd, "nocs_head.4", 64, 3, ACT_TANH, 64, 4)) return rc;
  if (pts_mlp) {
    if (int rc = init_linear(npm[0], scratch, sd, "nocs_pts_mlp.0", 3, 32, ACT_RELU, 4, 32)) return rc;
    if (int rc = init_linear(npm[1], scratch, sd, "nocs_pts_mlp.2", 32, 64, ACT_RELU, 32, 64)) return rc;
  }
  {
    // the same six layers as one LDS image for point_mlp_kernel (head_kernels.hip)
    static const char* const names[6] = {"instance_color.0", "nocs_head.0", "nocs_head.2", "nocs_head.4", "nocs_pts_mlp.0", "nocs_pts_mlp.2"};
    static const int cin[6] = {32, 64, 128, 64, 3, 32}, cout[6] = {64, 128, 64, 3, 32, 64};
    const float* w[6]; const float* b[6];
    const std::vector<float> zeros(32 * 64, 0.f);
    for (int l = 0; l < 6; ++l) {
      if (l >= 4 && !pts_mlp) { w[l] = b[l] = zeros.data(); continue; }
      GET(wt, std::string(names[l]) + ".weight"); GET(bt, std::string(names[l]) + ".bias");
      RGBM_REQUIRE(wt->numel() == (long long)cin[l] * cout[l] && bt->numel() == cout[l], std::string("point MLP shape ") + names[l]);
      w[l] = wt->data; b[l] = bt->data;
    }
    std::vector<float> table((size_t)point_mlp_table_floats());
    point_mlp_pack(w, b, table.data());
    if (upload_f32(table.data(), table.size(), pmlp_table)) return -2;
  }
  return 0;
}

int AdaPose::create_pose(const StateDict& sd) {
  {
    GET(w, "pose_mlp1.0.weight");
    RGBM_REQUIRE(w->numel() == 128ll * pose_in(), "pose_mlp1.0 shape: " + std::to_string(pose_in()) + " input channels expected");
  }
  if (int rc = init_linear(pm1[0], scratch, sd, "pose_mlp1.0", pose_in(), 128, ACT_RELU, pose_in(), 128, nullptr, pose_dtype())) return rc;
  if (int rc = init_linear(pm1[1], scratch, sd, "pose_mlp1.2", 128, 128, ACT_RELU, 128, 128, nullptr, pose_dtype())) return rc;
  {
    // pose_mlp2.0 sees cat(point feature[128], global mean[128]); the global half becomes a per-view bias
    GET(w, "pose_mlp2.0.weight"); GET(b, "pose_mlp2.0.bias");
    RGBM_REQUIRE(w->numel() == 256 * 256, "pose_mlp2.0 shape");
    std::vector<float> wl(256 * 128);
    for (int o = 0; o < 256; ++o) for (int i = 0; i < 128; ++i) wl[o * 128 + i] = w->data[o * 256 + i];
    if (int rc = init_linear(pm2[0], scratch, sd, "pose_mlp2.0", 128, 256, ACT_RELU, 128, 256, wl.data(), pose_dtype())) return rc;
    if (upload_f32(w->data, 256 * 256, pm2_0_wfull)) return -2;
    if (upload_f32(b->data, 256, pm2_0_bias)) return -2;
  }
  if (int rc = init_linear(pm2[1], scratch, sd, "pose_mlp2.2", 256, 256, ACT_RELU, 256, 256, nullptr, pose_dtype())) return rc;
  const char* hn[3] = {"rotation_estimator", "translation_estimator", "size_estimator"};
  const int hout[3] = {6, 3, 3};
  for (int h = 0; h < 3; ++h) {
    const int dims[4] = {256, 256, 128, hout[h]};
    for (int l = 0; l < 3; ++l) {
      GET(w, std::string(hn[h]) + "." + std::to_string(2 * l) + ".weight");
      GET(b, std::string(hn[h]) + "." + std::to_string(2 * l) + ".bias");
      RGBM_REQUIRE(w->numel() == (long long)dims[l] * dims[l + 1], "head weight shape");
      if (upload_f32(w->data, w->numel(), head_w[h][l])) return -2;
      if (upload_f32(b->data, b->numel(), head_b[h][l])) return -2;
    }
  }
  return 0;
}

static_assert(F32 == RGBM_F32 && BF16 == RGBM_BF16 && F16 == RGBM_F16 && BF16X3 == RGBM_BF16X3, "forward_paths.cpp reads DType by its C-ABI values");
static_assert(PATH_FLAG_PSP_STAGE_R5 == DBG_PSP_STAGE_R5 && PATH_FLAG_POINT_MLP_R5 == DBG_POINT_MLP_R5 && PATH_FLAG_TILE_CONV0 == DBG_TILE_CONV0 &&
              PATH_FLAG_POSE_MLP_R6 == DBG_POSE_MLP_R6, "forward_paths.h names the DebugFlag bits it reads");

// the only reader of the options and the debug flags behind set_option: everything below an entry point reads the ForwardPaths made of these
PathFacts AdaPose::path_facts(int B, bool dense) const {
  PathFacts f = {};
  f.arch = arch; f.dtype = dtype; f.norm_mode = norm_mode;
  f.cost_impl = cost_impl; f.sparse_tail = sparse_tail; f.sparse_dec = sparse_dec; f.sweep_f16 = sweep_f16; f.igemm_conv6 = igemm_conv6;
  f.fuse_final = fuse_final; f.upconv = upconv; f.stem = stem; f.view2_heads = view2_heads; f.pose_x3 = pose_x3;
  f.flags = g_debug_flags;
  f.stem_w = (bool)stem_w; f.sweep_w = (bool)sweep_w; f.sweep_w_f16 = (bool)sweep_w_f16; f.w11_x3 = (bool)w11_x3; f.w11_taps = (bool)w11_taps;
  f.tail_ready = tail.ready(); f.tail_f16_ready = tail.f16_ready(); f.pmlp_table = (bool)pmlp_table;
  f.psp_shape_ok = 1;
  for (const ConvLayer& L : psp)
    f.psp_shape_ok &= L.packs.size() == 1 && L.packs[0].Kpad == 512 && L.Cout_pad == 128 && !L.bias;
  auto pose_layer_ok = [](const ConvLayer& L, int cin, int cout) {
    return L.dtype == F16 && L.packs.size() == 1 && L.packs[0].ntaps == 1 && L.Cin_pad == cin && L.Cout_pad == cout && L.g.act == ACT_RELU &&
           L.packs[0].Kpad >= cin && L.bias;
  };
  f.pose_shape_ok = pose_mlp_fits(n_pts) && pose_layer_ok(pm1[0], 96, 128) && pose_layer_ok(pm1[1], 128, 128) && pose_layer_ok(pm2[0], 128, 256) &&
                    pose_layer_ok(pm2[1], 256, 256);
  f.dense = dense; f.V = 2 * B; f.Vh = view2_heads ? 2 * B : B; f.n_pts = n_pts;
  return f;
}

int AdaPose::chunk_poses(int B) const {
  const int cap = max_chunk / 2 > 0 ? max_chunk / 2 : 1;
  return B < cap ? B : cap;
}

int AdaPose::chunk_views(int V) const {
  const int cap = norm_mode == 1 && max_chunk > 32 ? 32 : max_chunk;      // per-sample BN materialises the 32-channel volume (154 MB per view in fp32)
  return V < cap ? V : cap;
}

// Shared by workspace_bytes() (base == nullptr) and forward(): identical allocation order => identical offsets.
int AdaPose::plan(int B, const ForwardPaths& p, Arena& A, Buffers& bf) const {
  const int V = 2 * B, P = n_pts, S = img;
  const size_t es = dtype_size(dtype);
  const size_t VP = (size_t)V * P;
  bf.Pviews = (float*)A.alloc((size_t)V * 16 * 4);
  bf.homog = (float*)A.alloc((size_t)V * 12 * 4);
  bf.choose = (int*)A.alloc(VP * 4);
  bf.masks = (unsigned char*)A.alloc((size_t)V * sparse_mask_bytes_per_view(img));
  bf.sweep_list = (int*)A.alloc((size_t)V * ((img + 11) / 12) * ((img + 15) / 16) * 4);
  bf.sweep_count = (int*)A.alloc((size_t)(V + 64) * 4);      // total, then one count per view
  bf.feat = A.alloc((size_t)V * S * S * 32 * es);
  bf.featf = dtype == BF16X3 ? (float*)A.alloc((size_t)V * S * S * 32 * 4) : nullptr;
  bf.X0 = (float*)A.alloc(VP * 32 * 4);
  bf.X1 = (float*)A.alloc(VP * 64 * 4);
  bf.H128 = (float*)A.alloc(VP * 128 * 4);
  bf.H64 = (float*)A.alloc(VP * 64 * 4);
  bf.nocs4 = (float*)A.alloc(VP * 4 * 4);
  bf.N32 = (float*)A.alloc(VP * 32 * 4);
  bf.PF96 = (float*)A.alloc(VP * pose_in() * 4);      // the pose rows: 96 channels, 128 for the real-world and the v1 network
  bf.PF96h = pose_dtype() == F16 ? A.alloc(VP * pose_in() * 2) : nullptr;
  bf.prob = (float*)A.alloc(VP * n_depth * 4);
  bf.depth = (float*)A.alloc(VP * 4);
  bf.Q128a = (float*)A.alloc(VP * 128 * 4);
  bf.Q128b = (float*)A.alloc(VP * 128 * 4);
  bf.G256a = (float*)A.alloc(VP * 256 * 4);
  bf.G256b = (float*)A.alloc(VP * 256 * 4);
  bf.glob = (float*)A.alloc((size_t)V * 128 * 4);
  bf.vbias = (float*)A.alloc((size_t)V * 256 * 4);
  bf.pf2 = (float*)A.alloc((size_t)V * 256 * 4);
  bf.h1 = (float*)A.alloc((size_t)V * 256 * 4);
  bf.h2 = (float*)A.alloc((size_t)V * 128 * 4);
  bf.r6 = (float*)A.alloc((size_t)V * 8 * 4);
  bf.R = (float*)A.alloc((size_t)V * 9 * 4);
  bf.tv = (float*)A.alloc((size_t)V * 4 * 4);
  bf.sv = (float*)A.alloc((size_t)V * 4 * 4);
  const size_t m0 = A.mark();
  // ---- phase A: PSPNet ----
  bf.imgpad = A.alloc((size_t)V * S * S * img_cpad * es);
  bf.c1 = A.alloc((size_t)V * (S / 2) * (S / 2) * 64 * es);
  const size_t lbuf = (size_t)V * ((size_t)(S / 4) * (S / 4) * 64 > (size_t)(S / 8) * (S / 8) * 512 ? (size_t)(S / 4) * (S / 4) * 64 : (size_t)(S / 8) * (S / 8) * 512) * es;
  for (int i = 0; i < 4; ++i) bf.lb[i] = A.alloc(lbuf);
  for (int i = 0; i < 4; ++i) {
    bf.pooled[i] = A.alloc((size_t)V * kPspBins[i] * kPspBins[i] * 512 * es);
    bf.stage[i] = A.alloc((size_t)V * kPspBins[i] * kPspBins[i] * 128 * es);
  }
  const size_t f8 = (size_t)(S / 8) * (S / 8), f4 = (size_t)(S / 4) * (S / 4), f2 = (size_t)(S / 2) * (S / 2), f1 = (size_t)S * S;
  bf.cat = A.alloc((size_t)V * f8 * 1024 * es);
  bf.ups = A.alloc((size_t)V * f4 * 1024 * es);      // == f2*256 == f1*64
  bf.u1 = A.alloc((size_t)V * f4 * 256 * es);
  bf.u2 = A.alloc((size_t)V * f2 * 64 * es);
  bf.u3 = A.alloc((size_t)V * f1 * 64 * es);
  A.release(m0);
  bf.fused = nullptr; bf.vf_scratch = nullptr;
  if (arch == ARCH_BASELINE) {
    // ---- phase B of the baseline network: the fused rows of both views and the attention stack's scratch for one chunk of poses ----
    bf.fused = (float*)A.alloc(VP * 32 * 4);
    bf.vf_scratch = A.alloc(view_fusion_scratch_bytes(chunk_poses(B), P));
    bf.vol = bf.bn_scratch = nullptr;
    for (auto& c : bf.c3) c = nullptr;
    A.release(m0);
    return 0;
  }
  if (arch == ARCH_V2 || arch == ARCH_V1) {      // no cost volume: the per-point buffers above are all its heads need
    bf.vol = bf.bn_scratch = nullptr;
    for (auto& c : bf.c3) c = nullptr;
    return 0;
  }
  // ---- phase B: cost volume, per chunk of views ----
  const int Vc = chunk_views(V);
  const int D = n_depth;
  const size_t vox = (size_t)D * S * S;
  bf.vol = p.vol ? A.alloc((size_t)Vc * vox * 32 * es) : nullptr;
  bf.bn_scratch = p.bn_scratch ? A.alloc(bn_scratch_bytes(Vc)) : nullptr;
  for (int l = 0; l < kCost3dLayers; ++l) bf.c3[l] = A.alloc(cost3d_out_elems(l, Vc, D, S) * es);
  A.release(m0);
  return 0;
}

static size_t plan_bytes(const AdaPose& n, int B, const ForwardPaths& p) {
  Arena A(nullptr, 0);
  AdaPose::Buffers bf;
  n.plan(B, p, A, bf);
  return A.peak + 256;
}

size_t AdaPose::workspace_bytes(int B) const { return plan_bytes(*this, B, paths(B)); }

int AdaPose::open_workspace(int B, const ForwardPaths& p, void* workspace, size_t workspace_size, size_t head, const char* pre, const char* post,
                            Buffers& bf) const {
  RGBM_REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace must be 256-byte aligned");
  RGBM_REQUIRE(n_depth % 8 == 0 && img % 8 == 0, "depth/img must be multiples of 8");
  const size_t need = head + plan_bytes(*this, B, p);
  RGBM_REQUIRE(workspace_size >= need, std::string(pre) + "workspace too small: need " + std::to_string(need) + post);
  Arena A((char*)workspace + head, workspace_size - head);
  return plan(B, p, A, bf);
}

// samples > 1 (forward_samples): Vout = samples x 2B views leave the PSPNet, and in front of the first Dropout2d site only the 2B input views
// differ.  Everything up to up_1's stacked GEMM runs on those 2B views; up_1's tap combination then runs once per sample and view half,
// writing the B views of that block where the tiled batch has them (view rows half * samples * B + k * B) with that block's mask rows.
int AdaPose::pspnet(const Buffers& bf, int Vout, const float* img1, const float* img2, const Call& call, const ForwardPaths& p, int samples) const {
  const int S = img;
  int V = Vout / samples;            // views of the shared prefix; all Vout behind up_1's tap combination
  hipStream_t s = call.stream;
  const float* drop = call.dropout != Dropout::None ? drop_masks.get<float>() : nullptr;      // factors [V][kDropoutPerView]
  int H = S / 2, W = S / 2;
  if (p.stem == STEM_FUSED) {
    // NCHW fp32 images -> conv1 + ReLU + max-pool in one kernel (no padded copy, no 112 x 112 x 64 tensor)
    // img2 == nullptr (features()): all V views, any V >= 1, lie in img1
    if (img2 == nullptr) { if (int rc = launch_stem_views(dtype, img1, stem_w.get(), bf.lb[0], V, S, s)) return rc; }
    else if (int rc = launch_stem(dtype, img1, img2, stem_w.get(), bf.lb[0], V / 2, V, S, s)) return rc;
  } else {
    const size_t es = dtype_size(dtype);
    const int B = img2 == nullptr ? V : V / 2;
    if (int rc = launch_nchw_to_nhwc_pad(dtype, img1, bf.imgpad, B, 3, S, S, img_cpad, s)) return rc;
    if (img2 != nullptr)
      if (int rc = launch_nchw_to_nhwc_pad(dtype, img2, (char*)bf.imgpad + (size_t)B * S * S * img_cpad * es, B, 3, S, S, img_cpad, s)) return rc;
    if (int rc = conv1.run(bf.imgpad, bf.c1, V, 1, S, S, 64, nullptr, 0, nullptr, 0, s)) return rc;
    if (int rc = launch_maxpool3x3s2(dtype, bf.c1, bf.lb[0], V, H, W, 64, s)) return rc;
  }
  H = S / 4; W = S / 4;
  int xi = 0;                                   // index of the buffer holding x
  for (int i = 0; i < n_blocks; ++i) {
    const Block& blk = blocks[i];
    void* x = bf.lb[xi];
    void* t = bf.lb[(xi + 1) & 3];
    void* r = bf.lb[(xi + 2) & 3];
    void* y = bf.lb[(xi + 3) & 3];
    int Do, Ho, Wo;
    blk.c1.out_dims(1, H, W, Do, Ho, Wo);
    if (int rc = blk.c1.run(x, t, V, 1, H, W, blk.planes, nullptr, 0, nullptr, 0, s)) return rc;
    const void* res = x;
    if (blk.has_ds) {
      if (int rc = blk.ds.run(x, r, V, 1, H, W, blk.planes, nullptr, 0, nullptr, 0, s)) return rc;
      res = r;
    }
    if (int rc = blk.c2.run(t, y, V, 1, Ho, Wo, blk.planes, res, RES_PRE_ACT, nullptr, 0, s)) return rc;
    H = Ho; W = Wo;
    xi = (xi + 3) & 3;
  }
  const void* f = bf.lb[xi];                    // [V][H][W][512], H = W = S/8; xi == layer4_index()
  RGBM_REQUIRE(H == S / 8 && W == S / 8, "feature stride");
  if (p.psp_stage == PSP_ROUND5) {      // the PSP stage as rounds 1-5 ran it: copy, pooling, four GEMM launches, four resizes
    if (int rc = launch_copy_channels(dtype, f, bf.cat, (long long)V * H * W, 512, 1024, 0, s)) return rc;
    {
      void* outs[4] = {bf.pooled[0], bf.pooled[1], bf.pooled[2], bf.pooled[3]};
      if (int rc = launch_adaptive_avgpool_multi(dtype, f, outs, kPspBins, 4, V, H, W, 512, s)) return rc;     // all four bin sizes, one launch
    }
    for (int i = 0; i < 4; ++i) {
      const int Sb = kPspBins[i];
      if (int rc = psp[i].run(bf.pooled[i], bf.stage[i], V, 1, Sb, Sb, 128, nullptr, 0, nullptr, 0, s)) return rc;
      if (int rc = launch_resize_bilinear_ac(dtype, bf.stage[i], bf.cat, V, Sb, Sb, 128, H, W, 1024, 512 + 128 * i, s)) return rc;
    }
  } else {
    // Small batches (the deployment shape, B = 1 .. 8): pooling and the four 512 -> 128 convs of the 50 cells per view in one launch on the
    // vector pipe (misc_kernels.hip; the GEMM launches it replaces had 2 .. 576 rows); larger ones keep the pooling launch and the
    // implicit GEMMs.  The concat (backbone channels + the four resized stages) is one launch at any size.
    if (p.psp_stage == PSP_ONE_LAUNCH) {
      const void* w[4] = {psp[0].packs[0].w.get(), psp[1].packs[0].w.get(), psp[2].packs[0].w.get(), psp[3].packs[0].w.get()};
      void* outs[4] = {bf.stage[0], bf.stage[1], bf.stage[2], bf.stage[3]};
      if (int rc = launch_psp_pool_conv(dtype, f, 512, w, outs, kPspBins, V, H, W, psp[0].g.act, psp[0].g.slope, s)) return rc;
    } else {
      void* outs[4] = {bf.pooled[0], bf.pooled[1], bf.pooled[2], bf.pooled[3]};
      if (int rc = launch_adaptive_avgpool_multi(dtype, f, outs, kPspBins, 4, V, H, W, 512, s)) return rc;     // all four bin sizes, one launch
      for (int i = 0; i < 4; ++i)
        if (int rc = psp[i].run(bf.pooled[i], bf.stage[i], V, 1, kPspBins[i], kPspBins[i], 128, nullptr, 0, nullptr, 0, s)) return rc;
    }
    const void* stages[4] = {bf.stage[0], bf.stage[1], bf.stage[2], bf.stage[3]};
    if (int rc = launch_psp_resize_cat(dtype, f, stages, kPspBins, bf.cat, V, H, W, s)) return rc;
  }
  // up_1 / up_2: 1x1 GEMM at the low resolution (nine taps stacked on the output channels, z in `ups`: 9/16 of the up-sampled
  // tensor it replaces) + tap combination; or, for A/B, the x2 resize followed by the 3x3 conv on the up-sampled grid
  // Dropout2d is applied in the tap combination's epilogue only: the A/B paths refuse it
  RGBM_REQUIRE(drop == nullptr || (p.up1 && p.up2), "dropout needs option upconv bits 0 and 1 (up_1 / up_2 through the tap combination)");
  if (samples > 1) {
    RGBM_REQUIRE(drop != nullptr && p.up1 && p.up2 && img2 != nullptr && V % 2 == 0, "pspnet: samples need Dropout2d masks and both views");
    const int B = V / 2;
    const size_t zview = up1c.scratch_elems(1, H, W) * dtype_size(dtype), oview = (size_t)4 * H * W * 256 * dtype_size(dtype);
    if (int rc = up1c.run_gemm(bf.cat, bf.ups, V, H, W, s)) return rc;
    for (int half = 0; half < 2; ++half)
      for (int k = 0; k < samples; ++k) {
        const size_t row = (size_t)half * samples * B + (size_t)k * B;
        if (int rc = up1c.combine((const char*)bf.ups + (size_t)half * B * zview, (char*)bf.u1 + row * oview, B, H, W, 256, s,
                                  drop + row * kDropoutPerView)) return rc;
      }
    V = Vout;
  } else if (p.up1) {
    if (int rc = up1c.run(bf.cat, bf.ups, bf.u1, V, H, W, 256, s, drop)) return rc;
  } else {
    if (int rc = launch_resize_bilinear_ac(dtype, bf.cat, bf.ups, V, H, W, 1024, 2 * H, 2 * W, 1024, 0, s)) return rc;
    if (int rc = up1.run(bf.ups, bf.u1, V, 1, 2 * H, 2 * W, 256, nullptr, 0, nullptr, 0, s)) return rc;
  }
  if (p.up2) {
    if (int rc = up2c.run(bf.u1, bf.ups, bf.u2, V, 2 * H, 2 * W, 64, s, drop ? drop + 256 : nullptr)) return rc;
  } else {
    if (int rc = launch_resize_bilinear_ac(dtype, bf.u1, bf.ups, V, 2 * H, 2 * W, 256, 4 * H, 4 * W, 256, 0, s)) return rc;
    if (int rc = up2.run(bf.ups, bf.u2, V, 1, 4 * H, 4 * W, 64, nullptr, 0, nullptr, 0, s)) return rc;
  }
  const bool plain_f32 = p.feat_form == FEAT_F32_ONLY;
  void* const feat = plain_f32 ? (void*)bf.featf : bf.feat;
  if (p.up3 == UP3_TAIL_KERNEL)       // up_3 + final from the half-resolution tensor in one kernel: no up-sampled tensor, no z, no u3
    return tail.run(bf.u2, feat, p.feat_form, V, 4 * H, 4 * W, s);
  if (int rc = launch_resize_bilinear_ac(dtype, bf.u2, bf.ups, V, 4 * H, 4 * W, 64, 8 * H, 8 * W, 64, 0, s)) return rc;
  // up_3 + final: one launch on the bf16 path (the 64-channel up_3 output then never reaches HBM: `u3` is not written)
  // bf16x3, default path: `final` writes the plain-fp32 feature map directly (no split-pair copy, no 6.6 GB conversion pass)
  return up3.run_then_1x1(fin, bf.ups, bf.u3, 64, feat, 32, V, 1, 8 * H, 8 * W, p.up3 == UP3_FUSED_FINAL, nullptr, s, plain_f32);
}

int AdaPose::feat_copy(const Buffers& bf, int V, const Call& call, const ForwardPaths& p) const {
  return p.feat_copy ? launch_bx3_to_f32(bf.feat, bf.featf, (long long)V * img * img * 32, call.stream) : 0;
}

int AdaPose::cost_volume(const Buffers& bf, int V, int B, const float* depths, const Call& call, const ForwardPaths& p) const {
  const int S = img, D = n_depth, P = n_pts;
  hipStream_t s = call.stream;
  const int Vh = view2_heads ? V : B;      // views whose probability volume is computed (partners are looked up among all V)
  const int Vc0 = chunk_views(V);
  // the rows of kCost3d on this forward's buffers, as the three chunk bodies walk them: input, output, skip tensor, down-sampling of the
  // input grid, output channels
  struct Layer3d { const void* in; void* out; const void* res; int div, C; };
  Layer3d l3d[kCost3dLayers];
  for (int i = 0; i < kCost3dLayers; ++i)
    l3d[i] = {i == 0 ? bf.vol : bf.c3[i - 1], bf.c3[i], kCost3d[i].skip >= 0 ? bf.c3[kCost3d[i].skip] : nullptr, kCost3d[i].in_div, kCost3d[i].cout};
  void* const u11 = bf.c3[kCost3dLayers - 1];
  // halo-tiled path (COST_TILES): one launch per layer; conv0 optionally builds its input on the fly
  // layer: the kernel's id, a row of kCost3d or 10 = row 0 with the plane sweep fused in (no input tensor); grids and channels come from the row
  auto tile = [&](int layer, const Layer3d& l, int Vc, int v0, const unsigned char* tmask) -> int {
    const int li = layer == 10 ? 0 : layer;
    const int Cin = kCost3d[li].cin, Cout = kCost3d[li].cout, qi = l.div, qo = cost3d_out_div(li);
    const bool transposed = kCost3d[li].transposed;
    const int Di = D / qi, Hi = S / qi, Wi = S / qi, Do = D / qo, Ho = S / qo, Wo = S / qo;
    const void* res = l.res;
    Conv3dTileDesc d;
    memset(&d, 0, sizeof(d));
    d.in = layer == 10 ? nullptr : l.in; d.wgt = t3d[li].w.get(); d.out = l.out; d.bias = t3d[li].bias.get<float>(); d.res = res;
    d.N = Vc; d.Di = Di; d.Hi = Hi; d.Wi = Wi; d.Do = Do; d.Ho = Ho; d.Wo = Wo;
    d.Dq = transposed ? Di : Do; d.Hq = transposed ? Hi : Ho; d.Wq = transposed ? Wi : Wo;
    d.Cout = Cout; d.relu = 1;
    d.feat = bf.feat; d.homog = bf.homog; d.depths = depths; d.v0 = v0; d.V = V; d.B = B;
    d.out_classmajor = layer == 9 ? 1 : 0;      // u11 is only gathered sparsely by the prob kernel
    d.tile_mask = tmask;
    d.fusion = layer == 10 ? fusion() : FUSION_SUM;      // only the kernels that build voxels have a fusion
    d.tile_mask_stride = sparse_mask_bytes_per_view(S);
    if (layer == 10 && p.sweep_list) { d.tile_list = bf.sweep_list; d.tile_count = bf.sweep_count; }
    // profiler rows (prof.h): conv0 + fused warp on its own; bf16 layers one row each, f32 layers aggregated
    d.prof_variant = dtype == BF16X3 ? (layer == 10 ? 28 : 27) : layer == 10 ? 10 + (dtype != F32 ? 1 : 0) : (dtype != F32 ? 16 + layer : 8);
    d.algo_flops = 2.0 * Vc * (double)(transposed ? Di * Hi * Wi : Do * Ho * Wo) * Cout * 27.0 * Cin;
    // layer 10 (conv0 with the plane sweep fused in) reads the two feature maps of a pair, not the 32 x D x H x W volume it
    // never materialises: algorithmic bytes = features in + c0 out
    d.algo_bytes = ((layer == 10 ? (double)Vc * Hi * Wi * Cin : (double)Vc * Di * Hi * Wi * Cin) +
                    (double)Vc * Do * Ho * Wo * Cout * (res ? 2 : 1)) * (double)dtype_size(dtype);
    if (layer == 10 && (p.conv0 == CONV0_SWEEP16 || p.conv0 == CONV0_SWEEP16_F16)) {
      d.wgt = sweep_w.get();
      if (p.conv0 == CONV0_SWEEP16_F16) { d.wgt = sweep_w_f16.get(); d.feat_f16 = 1; }
      return launch_conv0_sweep(d, dtype, s);
    }
    if (layer == 10 && p.conv0 == CONV0_SWEEP_X3) {
      d.wgt = sweep_w.get();
      d.feat = bf.featf;
      return launch_conv0_sweep_x3(d, s);
    }
    return launch_conv3d_tile(layer, dtype, d, s);
  };
  // Sparse cost regularisation (sparse_dec, with the sparse tail only): the tail reads the probability volume at the chosen pixels, so every
  // layer is needed only inside their dependency cones (prob_sparse.hip: sparse_mask_kernel) — conv1 .. conv5, conv7 / conv9 skip the
  // other tiles, the depth-sweeping conv0 walks the list of needed ones.  conv6 stays dense (a 0.3 ms GEMM): what it computes from
  // unwritten input tiles is never read by anything that is read.
  for (int v0 = 0; v0 < Vh; v0 += Vc0) {
    const int Vc = Vh - v0 < Vc0 ? Vh - v0 : Vc0;
    int classmajor = 0;      // layout of the u11 the chunk body leaves behind
    if (p.cost_body == COST_BN_PER_SAMPLE) {
      // per-sample BatchNorm3d: every layer = un-normalised conv (generic implicit GEMM) -> per-view batch statistics -> normalise + ReLU (+ skip)
      if (int rc = launch_build_volume(dtype, bf.feat, bf.homog, depths, bf.vol, v0, Vc, V, B, D, S, S, s, fusion())) return rc;
      for (int i = 0; i < 10; ++i) {
        const Layer3d& l = l3d[i];
        const ConvLayer& L = c3d_raw[i];
        int Do, Ho, Wo;
        L.out_dims(D / l.div, S / l.div, S / l.div, Do, Ho, Wo);
        if (int rc = L.run(l.in, l.out, Vc, D / l.div, S / l.div, S / l.div, l.C, nullptr, RES_NONE, nullptr, 0, s)) return rc;
        if (int rc = launch_bn_per_sample(dtype, l.out, l.res, bn_gamma[i].get<float>(), bn_beta[i].get<float>(), bf.bn_scratch, Vc,
                                          (long long)Do * Ho * Wo, l.C, 1, s)) return rc;
      }
    } else if (p.cost_body == COST_GENERIC) {
      // generic implicit GEMM on the materialised volume; the skip adds of conv7 / 9 / 11 are post-ReLU (network_v5.py:287-289)
      if (int rc = launch_build_volume(dtype, bf.feat, bf.homog, depths, bf.vol, v0, Vc, V, B, D, S, S, s, fusion())) return rc;
      for (int i = 0; i < 10; ++i) {
        const Layer3d& l = l3d[i];
        if (int rc = c3d[i].run(l.in, l.out, Vc, D / l.div, S / l.div, S / l.div, l.C, l.res, RES_POST_ACT, nullptr, 0, s)) return rc;
      }
    } else {
      // halo-tiled layers; conv0 on the materialised volume (cost_impl 1) or with the plane sweep fused in
      const unsigned char* mk[10] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
      if (p.mask_level > 0) {
        int td, th, tw;
        for (int L : {1, 2, 3, 4, 5, 7, 8}) RGBM_REQUIRE(!conv3d_tile_dims(L, dtype, &td, &th, &tw) && th == 8 && tw == 8, "sparse cost regularisation: 8 x 8 tiles expected");
        if (int rc = launch_sparse_masks(bf.choose, v0, Vc, P, S, bf.masks, bf.sweep_list, bf.sweep_count, s)) return rc;
        for (int L : {7, 8}) mk[L] = bf.masks + sparse_mask_offset(S, L);
        if (p.mask_level >= 2)
          for (int L : {1, 2, 3, 4, 5}) mk[L] = bf.masks + sparse_mask_offset(S, L);
      }
      // one launch per row; the rows that are not simply their halo-tile kernel say so
      for (int i = 0; i < (p.tail_sparse ? 9 : kCost3dLayers); ++i) {
        const Layer3d& l = l3d[i];
        if (i == 0 && p.conv0 == CONV0_TILE_VOLUME) {
          if (int rc = launch_build_volume(dtype, bf.feat, bf.homog, depths, bf.vol, v0, Vc, V, B, D, S, S, s, fusion())) return rc;
          if (int rc = tile(0, l, Vc, v0, nullptr)) return rc;
        } else if (i == 0) {
          if (int rc = tile(10, l, Vc, v0, nullptr)) return rc;
        } else if (i == 6 && p.conv6_igemm) {
          if (int rc = c3d[6].run(l.in, l.out, Vc, D / l.div, S / l.div, S / l.div, l.C, nullptr, RES_NONE, nullptr, 0, s)) return rc;
        } else {
          if (int rc = tile(i, l, Vc, v0, mk[i])) return rc;      // masks: rows 1-5, 7 and 8 (above)
        }
      }
      if (p.tail_sparse) {
        // conv11 + skip + prob conv + softmax + depth only on the 3x3 neighbourhoods of the chosen pixels (prob_sparse.hip)
        if (int rc = launch_prob_sparse(l3d[9].in, l3d[9].res, dtype == BF16X3 ? w11_x3.get() : t3d[9].w.get(), t3d[9].bias.get<float>(),
                                        wprob.get<float>(), bf.choose, depths, bf.prob, bf.depth, v0, Vc, B, P, D, S, S, dtype, s, w11_taps.get())) return rc;
        continue;
      }
      classmajor = 1;      // u11 is only gathered: conv11's halo-tile kernel writes it class-major
    }
    if (int rc = launch_prob_softmax_depth(dtype, u11, wprob.get<float>(), bf.choose, depths, bf.prob, bf.depth, v0, Vc, B, P, D, S, S, classmajor, s)) return rc;
    // the dense head on the u11 of every chunk, beside the point kernel (rows v0 .. v0 + Vc - 1 of the maps)
    if (call.depth_map != nullptr)
      if (int rc = launch_dense_depth(dtype, u11, wprob.get<float>(), depths, call.depth_map, call.conf_map, v0, Vc, B, D, S, S, classmajor, s)) return rc;
  }
  return 0;
}

int AdaPose::forward(int B, const float* img1, const float* img2, const int* choose1, const int* choose2, const float* P1,
                     const float* P2, const float* depths, void* workspace, size_t workspace_size, const Outputs& out,
                     const Call& call) const {
  RGBM_REQUIRE(call.depth_map == nullptr || call.dense, "forward: depth_map needs a dense call");
  RGBM_REQUIRE(call.depth_map != nullptr || call.conf_map == nullptr, "forward_maps: conf_map without depth_map");
  RGBM_REQUIRE(call.nocs_map == nullptr || pmlp_table, "forward_maps: no point MLP table");
  RGBM_REQUIRE(B > 0, "batch");
  RGBM_REQUIRE(arch != ARCH_BASELINE || !(call.dense || call.depth_map || call.conf_map || call.nocs_map),
               "baseline network: the dense / maps forwards are not implemented (they read the cost volume this network does not have)");
  RGBM_REQUIRE(arch != ARCH_BASELINE || call.dropout == Dropout::None, "baseline network: Dropout2d is not implemented");
  RGBM_REQUIRE(arch != ARCH_REALWORLD || !(call.dense || call.depth_map || call.conf_map || call.nocs_map),
               "real-world network: the dense / maps forwards are not implemented");
  RGBM_REQUIRE(arch != ARCH_REALWORLD || call.dropout == Dropout::None, "real-world network: Dropout2d is not implemented");
  RGBM_REQUIRE(arch != ARCH_REALWORLD || (call.coor1 != nullptr && call.coor2 != nullptr),
               "real-world network: the forward needs coor1 / coor2 (rgbm_adapose_forward_realworld)");
  RGBM_REQUIRE(arch != ARCH_V2 || !(call.dense || call.depth_map || call.conf_map || call.nocs_map),
               "v2 network: the dense / maps forwards are not implemented (it has no probability volume, and its stereo part runs at the chosen pixels only)");
  RGBM_REQUIRE(arch != ARCH_V2 || call.dropout == Dropout::None, "v2 network: Dropout2d is not implemented");
  RGBM_REQUIRE(arch != ARCH_V2 || (call.coor1 == nullptr && call.coor2 == nullptr), "v2 network: coor1 / coor2 belong to the real-world network");
  RGBM_REQUIRE(arch != ARCH_V1 || !(call.dense || call.depth_map || call.conf_map || call.nocs_map),
               "v1 network: the dense / maps forwards are not implemented (it has no probability volume, and its stereo part runs at the chosen pixels only)");
  RGBM_REQUIRE(arch != ARCH_V1 || call.dropout == Dropout::None, "v1 network: Dropout2d is not implemented");
  RGBM_REQUIRE(arch != ARCH_V1 || (call.coor1 == nullptr && call.coor2 == nullptr), "v1 network: coor1 / coor2 belong to the real-world network");
  const ForwardPaths p = paths(B, call.dense);
  Buffers bf;
  if (int rc = open_workspace(B, p, workspace, workspace_size, 0, call.dense ? "forward_dense: " : "", call.dense ? " (rgbm_adapose_dense_workspace_bytes)" : "", bf)) return rc;
  const int V = 2 * B;
  hipStream_t s = call.stream;

  // ---- stage inputs: views = [view1 batch ; view2 batch] ----
  // the baseline network ignores the projections and the depth planes (network_baseline.py:609-669 never reads them): they may be null
  if (arch == ARCH_BASELINE) {
    RGBM_CHECK_HIP(hipMemcpyAsync(bf.choose, choose1, (size_t)B * n_pts * sizeof(int), hipMemcpyDeviceToDevice, s));
    RGBM_CHECK_HIP(hipMemcpyAsync(bf.choose + (size_t)B * n_pts, choose2, (size_t)B * n_pts * sizeof(int), hipMemcpyDeviceToDevice, s));
  } else if (int rc = launch_stage_in(P1, P2, choose1, choose2, bf.Pviews, bf.choose, B, n_pts, s)) return rc;
  // Dropout2d: masks loaded for this forward (rgbm_adapose_set_dropout_masks), or drawn for poses counter .. counter + B - 1
  if (call.dropout != Dropout::None) {
    const bool loaded = call.dropout == Dropout::Loaded;
    RGBM_REQUIRE(V <= drop_cap_views && drop_masks && (loaded || drop_state), "dropout: mask buffer smaller than the batch");
    RGBM_REQUIRE((upconv & 3) == 3, "dropout needs option upconv bits 0 and 1 (up_1 / up_2 through the tap combination)");
    if (!loaded)
      if (int rc = launch_dropout_masks(drop_masks.get<float>(), drop_state.get<unsigned long long>(), B, drop_p, drop_seed, call.dropout == Dropout::Draw ? 1 : 0, s)) return rc;
  }
  if (int rc = pspnet(bf, V, img1, img2, call, p)) return rc;
  if (arch != ARCH_BASELINE)
    if (int rc = launch_homography(bf.Pviews, bf.homog, V, B, s)) return rc;
  if (int rc = feat_copy(bf, V, call, p)) return rc;
  if (call.stop_after == 1) return 0;
  if (arch == ARCH_BASELINE) return heads_baseline(bf, B, out, call, p);
  if (arch == ARCH_V2) return heads_v2(bf, B, depths, out, call, p);
  if (arch == ARCH_V1) return heads_v1(bf, B, depths, out, call, p);
  return heads(bf, B, depths, out, call, p);
}

// S Dropout2d samples of B poses: forward() of the S x B poses that are the B poses tiled S times (pose k * B + b = sample k of pose b),
// with the part of the PSPNet in front of the first Dropout2d site run once (pspnet(): samples).  The per-pose inputs are tiled into a
// staging block at the head of the workspace; the plan for S x B poses follows it.
static size_t samples_staging_bytes(const AdaPose& n, int SB) {
  return align_up((size_t)SB * (2 * 16 * sizeof(float) + 2 * n.n_pts * sizeof(int) + n.n_depth * sizeof(float)), 256);
}

size_t AdaPose::samples_workspace_bytes(int B, int S) const { return samples_staging_bytes(*this, S * B) + workspace_bytes(S * B); }

int AdaPose::forward_samples(int B, int S, const float* img1, const float* img2, const int* choose1, const int* choose2, const float* P1,
                             const float* P2, const float* depths, void* workspace, size_t workspace_size, const Outputs& out,
                             const Call& call) const {
  RGBM_REQUIRE(B > 0 && S >= 1 && (long long)S * B <= (1 << 20), "forward_samples: B >= 1 poses and S >= 1 samples");
  RGBM_REQUIRE(arch != ARCH_BASELINE, "forward_samples: not implemented for the baseline network (it has no Dropout2d)");
  RGBM_REQUIRE(arch != ARCH_REALWORLD, "forward_samples: not implemented for the real-world network");
  RGBM_REQUIRE(arch != ARCH_V2, "forward_samples: not implemented for the v2 network (it has no Dropout2d)");
  RGBM_REQUIRE(arch != ARCH_V1, "forward_samples: not implemented for the v1 network (it has no Dropout2d)");
  RGBM_REQUIRE(!(call.dense || call.depth_map || call.conf_map || call.nocs_map) && call.stop_after == 0, "forward_samples: no dense / maps form");
  RGBM_REQUIRE(call.dropout == Dropout::Draw || call.dropout == Dropout::Loaded,
               "forward_samples: Dropout2d is off and no masks are loaded (rgbm_adapose_set_dropout / rgbm_adapose_set_dropout_masks): the samples would be equal");
  RGBM_REQUIRE((upconv & 3) == 3, "forward_samples needs option upconv bits 0 and 1 (the masks are applied in the tap combination of up_1 / up_2)");
  const int SB = S * B, V = 2 * SB;
  RGBM_REQUIRE(V <= drop_cap_views && drop_masks && (call.dropout == Dropout::Loaded || drop_state), "forward_samples: mask buffer smaller than S x B poses");
  PathFacts facts = path_facts(SB, false);
  facts.V = 2 * B;      // the PSPNet's shared prefix runs on the 2B input views
  const ForwardPaths p = forward_paths(facts);
  // staging block: P1, P2 [SB][16], choose1, choose2 [SB][P], depths [SB][D]
  const size_t stage = samples_staging_bytes(*this, SB);
  Buffers bf;
  if (int rc = open_workspace(SB, p, workspace, workspace_size, stage, "forward_samples: ", " (rgbm_adapose_samples_workspace_bytes)", bf)) return rc;
  hipStream_t s = call.stream;
  float* tP1 = (float*)workspace;
  float* tP2 = tP1 + (size_t)SB * 16;
  int* tc1 = (int*)(tP2 + (size_t)SB * 16);
  int* tc2 = tc1 + (size_t)SB * n_pts;
  float* tdep = (float*)(tc2 + (size_t)SB * n_pts);
  if (int rc = launch_tile_words(P1, tP1, (long long)B * 16, S, s)) return rc;
  if (int rc = launch_tile_words(P2, tP2, (long long)B * 16, S, s)) return rc;
  if (int rc = launch_tile_words(choose1, tc1, (long long)B * n_pts, S, s)) return rc;
  if (int rc = launch_tile_words(choose2, tc2, (long long)B * n_pts, S, s)) return rc;
  if (int rc = launch_tile_words(depths, tdep, (long long)B * n_depth, S, s)) return rc;
  if (int rc = launch_stage_in(tP1, tP2, tc1, tc2, bf.Pviews, bf.choose, SB, n_pts, s)) return rc;
  if (call.dropout == Dropout::Draw)      // poses counter .. counter + SB - 1, as the plain forward of the tiled batch draws them
    if (int rc = launch_dropout_masks(drop_masks.get<float>(), drop_state.get<unsigned long long>(), SB, drop_p, drop_seed, 1, s)) return rc;
  if (int rc = pspnet(bf, V, img1, img2, call, p, S)) return rc;
  if (int rc = launch_homography(bf.Pviews, bf.homog, V, SB, s)) return rc;
  if (int rc = feat_copy(bf, V, call, p)) return rc;
  return heads(bf, SB, tdep, out, call, p);
}

// Everything behind the PSPNet of the baseline network (network_baseline.py:617-669): the gathered rows feed the NOCS branch as in v5 and,
// untouched, the attention stack; depth_head and the pose branch read the fused rows.
AdaPose::FeatSource AdaPose::gather_source(const Buffers& bf, const ForwardPaths& p) const {
  if (dtype == BF16X3) return {bf.featf, F32};
  return {bf.feat, p.feat_form == FEAT_F16 ? (int)F16 : dtype};
}

PointMlpDesc AdaPose::point_mlp_desc(const Buffers& bf, const FeatSource& src, int Vh) const {
  PointMlpDesc pd{};
  pd.table = pmlp_table.get<float>(); pd.feat = src.feat; pd.choose = bf.choose; pd.nocs4 = bf.nocs4; pd.pf = bf.PF96 + 32; pd.ldpf = 96; pd.P = n_pts; pd.HW = img * img;
  if (arch == ARCH_REALWORLD) { pd.pf = bf.X1; pd.ldpf = 64; }      // layers 4 / 5 of its table are zero: the 64 channels go to a buffer nothing reads
  pd.N = (long long)Vh * n_pts;
  return pd;
}

// view2_heads = 0: the view-2 outputs are filled with NaN, so that a consumer of one fails loudly instead of reading stale numbers
int AdaPose::stage_out(const Buffers& bf, int B, const Outputs& out, hipStream_t s) const {
  float* const on[2] = {out.nocs1, out.nocs2};
  float* const od[2] = {out.depth1, out.depth2};
  float* const orr[2] = {out.r1, out.r2};
  float* const ot[2] = {out.t1, out.t2};
  float* const os[2] = {out.s1, out.s2};
  return launch_stage_out(bf.nocs4, bf.depth, bf.R, bf.tv, bf.sv, on, od, orr, ot, os, B, n_pts, view2_heads, s);
}

int AdaPose::heads_baseline(const Buffers& bf, int B, const Outputs& out, const Call& call, const ForwardPaths& p) const {
  const int V = 2 * B, P = n_pts, S = img;
  hipStream_t s = call.stream;
  const FeatSource src = gather_source(bf, p);
  const int Vh = view2_heads ? V : B;
  RGBM_REQUIRE(pmlp_table && ((long long)Vh * P) % 64 == 0, "baseline network: the point MLP kernel needs a multiple of 64 points");
  // both views' rows: view 2's are every block's keys even without its heads
  if (int rc = launch_gather_points(src.dtype, src.feat, bf.choose, bf.X0, V, P, S * S, 32, s)) return rc;
  if (int rc = launch_point_mlp(src.dtype, point_mlp_desc(bf, src, Vh), s)) return rc;
  // the attention stack, a chunk of poses at a time (max_chunk views = max_chunk / 2 poses): a pose's rows do not depend on its chunk
  const size_t view2 = (size_t)B * P * 32;
  const int Bc0 = chunk_poses(B);
  for (int b0 = 0; b0 < B; b0 += Bc0) {
    const int Bc = B - b0 < Bc0 ? B - b0 : Bc0;
    const size_t o = (size_t)b0 * P * 32;
    if (int rc = launch_view_fusion(vf_w.get<float>(), bf.X0 + o, bf.X0 + view2 + o, Bc, P, bf.fused + o, bf.fused + view2 + o, bf.vf_scratch,
                                    view_fusion_scratch_bytes(Bc0, P), view2_heads ? 2 : 1, s)) return rc;
  }
  if (call.stop_after == 2) return 0;
  // depth_head on the fused rows; the same rows are channels 0..31 of the pose feature (network_baseline.py:633-641)
  if (int rc = launch_depth_head(dh_w.get<float>(), bf.fused, (long long)Vh * P, bf.depth, regress_pose ? bf.PF96 : nullptr, 96, s)) return rc;
  if (regress_pose)
    if (int rc = pose_branch(bf, Vh, call, p)) return rc;
  if (int rc = stage_out(bf, B, out, s)) return rc;
  if (!regress_pose) {      // no pose branch: the six r / t / s outputs are NaN
    float* const rts[6] = {out.r1, out.t1, out.s1, out.r2, out.t2, out.s2};
    for (int i = 0; i < 6; ++i)
      if (int rc = launch_fill_nan(rts[i], (long long)B * (i % 3 == 0 ? 9 : 3), s)) return rc;
  }
  return 0;
}

// Everything behind the PSPNet of the v2 network (network_v2.py:152-197): the NOCS branch as in v5; the stereo part and pose_mlp1 at the
// chosen pixels in one kernel (v2_head.hip); the size branch pose_mlp2 -> mean -> size_estimator on 64 / 128 channels, every mean over a
// view's points finished in the fixed order of launch_mean_points_partial's slices.  No depth, rotation or translation: those outputs are NaN.
int AdaPose::heads_v2(const Buffers& bf, int B, const float* depths, const Outputs& out, const Call& call, const ForwardPaths& p) const {
  const int V = 2 * B, P = n_pts, S = img, D = n_depth;
  hipStream_t s = call.stream;
  const FeatSource src = gather_source(bf, p);
  const int Vh = view2_heads ? V : B;
  RGBM_REQUIRE(v2_w, "v2 network: no packed head table");
  if (p.point_mlp) {
    if (int rc = launch_point_mlp(src.dtype, point_mlp_desc(bf, src, Vh), s)) return rc;
  } else {
    if (int rc = launch_gather_points(src.dtype, src.feat, bf.choose, bf.X0, Vh, P, S * S, 32, s)) return rc;
    if (int rc = inst.run(bf.X0, bf.X1, Vh, 1, 1, P, 64, nullptr, 0, nullptr, 0, s)) return rc;
    if (int rc = nh[0].run(bf.X1, bf.H128, Vh, 1, 1, P, 128, nullptr, 0, nullptr, 0, s)) return rc;
    if (int rc = nh[1].run(bf.H128, bf.H64, Vh, 1, 1, P, 64, nullptr, 0, nullptr, 0, s)) return rc;
    if (int rc = nh[2].run(bf.H64, bf.nocs4, Vh, 1, 1, P, 4, nullptr, 0, nullptr, 0, s)) return rc;
  }
  // rows (pose_mlp1's output) in X1; fuse_conv's output in H64 and volume_conv's 24 values in prob, for rgbm_adapose_fetch
  if (int rc = launch_v2_point_rows(src.dtype, v2_w.get<float>(), src.feat, bf.homog, depths, bf.choose, bf.X1, bf.H64, bf.prob, V, B, P, D, S, S, Vh, s)) return rc;
  if (call.stop_after == 2) return 0;
  if (int rc = launch_mean_points_partial(F32, bf.X1, bf.Q128a, Vh, P, 64, s)) return rc;
  if (int rc = launch_view_linear_mean(bf.Q128a, P, bf.glob, pm2_0_wfull.get<float>(), pm2_0_bias.get<float>(), bf.vbias, Vh, 64, 128, 128, 64, 0, s)) return rc;
  if (int rc = pm2[0].run(bf.X1, bf.Q128b, Vh, 1, 1, P, 128, nullptr, 0, bf.vbias, 128, s)) return rc;
  if (int rc = pm2[1].run(bf.Q128b, bf.G256b, Vh, 1, 1, P, 128, nullptr, 0, nullptr, 0, s)) return rc;
  if (int rc = launch_mean_points_partial(F32, bf.G256b, bf.G256a, Vh, P, 128, s)) return rc;
  if (int rc = launch_view_linear_mean(bf.G256a, P, bf.pf2, head_w[2][0].get<float>(), head_b[2][0].get<float>(), bf.h1, Vh, 128, 128, 128, 0, 1, s)) return rc;
  if (int rc = launch_view_linear(bf.h1, head_w[2][1].get<float>(), head_b[2][1].get<float>(), bf.h2, Vh, 128, 64, 128, 0, 1, s)) return rc;
  if (int rc = launch_view_linear(bf.h2, head_w[2][2].get<float>(), head_b[2][2].get<float>(), bf.sv, Vh, 64, 3, 64, 0, 0, s)) return rc;
  // nocs and s through the staging kernel (view 2's are NaN without its heads); what this network does not compute is NaN
  if (int rc = stage_out(bf, B, out, s)) return rc;
  float* const nan_out[6] = {out.depth1, out.depth2, out.r1, out.r2, out.t1, out.t2};
  const long long nan_n[6] = {(long long)B * P, (long long)B * P, (long long)B * 9, (long long)B * 9, (long long)B * 3, (long long)B * 3};
  for (int i = 0; i < 6; ++i)
    if (int rc = launch_fill_nan(nan_out[i], nan_n[i], s)) return rc;
  return 0;
}

// Stages A and B of the v1 heads (network.py:167-197), two launches: A waits on gathers and wants many waves per CU, B keeps 88 KB of
// weights resident with one wave per SIMD.  Without the one-launch B (a point count that is no multiple of 64, or the point-MLP debug
// flag) the same six layers run as the GEMM launches of v5's per-layer branch, and a column copy puts instance_color's output into the rows.
int AdaPose::v1_stages(int feat_dtype, const void* feat, const float* homog, const float* depths, const int* choose, float* fused32, float* planes,
                       float* nocs4, float* rows128, const V1Scratch& sc, int B, int P, int S, int Vh, bool fused_mlp, hipStream_t s) const {
  RGBM_REQUIRE(v1_w && pmlp_table, "v1 network: no packed head tables");
  if (int rc = launch_v1_fused_points(feat_dtype, v1_w.get<float>(), feat, homog, depths, choose, fused32, planes, 2 * B, B, P, n_depth, S, S, Vh, s)) return rc;
  if (nocs4 == nullptr || rows128 == nullptr) return 0;      // stage A alone
  const long long N = (long long)Vh * P;
  if (fused_mlp) return launch_point_mlp_rows(pmlp_table.get<float>(), fused32, nocs4, rows128, N, s);
  RGBM_REQUIRE(sc.h64a && sc.h128 && sc.h64b && sc.n32, "v1 network: the per-layer point branch needs its scratch");
  // One view per launch: which GEMM kernel and K split a launch takes depends on its row count (conv_plan.cpp), and with it the rounding
  // of its sums; launches of P rows each make a view's rows the same bits whether B or 2B views get heads.  6 Vh small launches: this is
  // the stand-in path, the forward at 1024 points runs the one-launch kernel above.
  for (long long v = 0; v < Vh; ++v) {
    const long long r = v * P;
    if (int rc = inst.run(fused32 + r * 32, sc.h64a + r * 64, 1, 1, 1, P, 64, nullptr, 0, nullptr, 0, s)) return rc;
    if (int rc = nh[0].run(sc.h64a + r * 64, sc.h128 + r * 128, 1, 1, 1, P, 128, nullptr, 0, nullptr, 0, s)) return rc;
    if (int rc = nh[1].run(sc.h128 + r * 128, sc.h64b + r * 64, 1, 1, 1, P, 64, nullptr, 0, nullptr, 0, s)) return rc;
    if (int rc = nh[2].run(sc.h64b + r * 64, nocs4 + r * 4, 1, 1, 1, P, 4, nullptr, 0, nullptr, 0, s)) return rc;
    if (int rc = npm[0].run(nocs4 + r * 4, sc.n32 + r * 32, 1, 1, 1, P, 32, nullptr, 0, nullptr, 0, s)) return rc;
    if (int rc = npm[1].run(sc.n32 + r * 32, rows128 + r * 128 + 64, 1, 1, 1, P, 128, nullptr, 0, nullptr, 0, s)) return rc;
  }
  return launch_copy_cols(sc.h64a, rows128, N, 64, 128, 64, s);
}

// Everything behind the PSPNet of the v1 network: stage A (fused32 in X0, volume_conv's 24 values in prob, for rgbm_adapose_fetch), stage
// B (nocs4, the 128-channel pose rows in PF96), then v5's pose branch and staging unchanged.  This network has no depth: those outputs are NaN.
int AdaPose::heads_v1(const Buffers& bf, int B, const float* depths, const Outputs& out, const Call& call, const ForwardPaths& p) const {
  const int V = 2 * B, P = n_pts, S = img;
  hipStream_t s = call.stream;
  const FeatSource src = gather_source(bf, p);
  const int Vh = view2_heads ? V : B;
  const V1Scratch sc = {bf.X1, bf.H128, bf.H64, bf.N32};
  if (int rc = v1_stages(src.dtype, src.feat, bf.homog, depths, bf.choose, bf.X0, bf.prob, bf.nocs4, bf.PF96, sc, B, P, S, Vh, p.point_mlp != 0, s)) return rc;
  if (call.stop_after == 2) return 0;
  if (int rc = pose_branch(bf, Vh, call, p)) return rc;
  if (int rc = stage_out(bf, B, out, s)) return rc;
  if (int rc = launch_fill_nan(out.depth1, (long long)B * P, s)) return rc;
  return launch_fill_nan(out.depth2, (long long)B * P, s);
}

int AdaPose::nocs_map_of(const float* feat_f32, long long pixels, float* nocs_map, hipStream_t s) const {
  RGBM_REQUIRE(pmlp_table, "nocs_map: no point MLP table");
  return launch_dense_nocs(F32, pmlp_table.get<float>(), feat_f32, nocs_map, pixels, s);
}

// Everything behind the PSPNet: reads the feature map(s) in bf.feat / bf.featf, bf.homog, bf.choose (forward() and forward_cached() fill them)
int AdaPose::heads(const Buffers& bf, int B, const float* depths, const Outputs& out, const Call& call, const ForwardPaths& p) const {
  const int V = 2 * B, P = n_pts, S = img, D = n_depth;
  hipStream_t s = call.stream;
  const FeatSource src = gather_source(bf, p);

  const int Vh = view2_heads ? V : B;      // views that get heads: both crops of every pose, or the view-1 crops only (option view2_heads)
  // ---- per-point NOCS branch (network_v5.py:432-444) ----
  if (p.point_mlp) {
    // gather + the six layers in one launch (head_kernels.hip): a wave carries 16 points through the whole branch, weights and activations in LDS
    if (int rc = launch_point_mlp(src.dtype, point_mlp_desc(bf, src, Vh), s)) return rc;
  } else {
    if (int rc = launch_gather_points(src.dtype, src.feat, bf.choose, bf.X0, Vh, P, S * S, 32, s)) return rc;
    if (int rc = inst.run(bf.X0, bf.X1, Vh, 1, 1, P, 64, nullptr, 0, nullptr, 0, s)) return rc;
    if (int rc = nh[0].run(bf.X1, bf.H128, Vh, 1, 1, P, 128, nullptr, 0, nullptr, 0, s)) return rc;
    if (int rc = nh[1].run(bf.H128, bf.H64, Vh, 1, 1, P, 64, nullptr, 0, nullptr, 0, s)) return rc;
    if (int rc = nh[2].run(bf.H64, bf.nocs4, Vh, 1, 1, P, 4, nullptr, 0, nullptr, 0, s)) return rc;
    if (arch != ARCH_REALWORLD) {      // (the real-world network's nocs_pts_mlp runs in pose_rows_kernel, below)
      if (int rc = npm[0].run(bf.nocs4, bf.N32, Vh, 1, 1, P, 32, nullptr, 0, nullptr, 0, s)) return rc;
      if (int rc = npm[1].run(bf.N32, bf.PF96 + 32, Vh, 1, 1, P, 96, nullptr, 0, nullptr, 0, s)) return rc;
    }
  }

  // the same branch's layers 0..3 on every pixel of the Vh feature maps (the dense NOCS map)
  if (call.nocs_map != nullptr)
    if (int rc = launch_dense_nocs(src.dtype, pmlp_table.get<float>(), src.feat, call.nocs_map, (long long)Vh * S * S, s)) return rc;

  // ---- plane-sweep cost volume -> probability at the sampled pixels -> depth ----
  if (int rc = cost_volume(bf, V, B, depths, call, p)) return rc;
  if (call.stop_after == 2) return 0;

  // ---- depth-guided fusion + pose regression (network_v5.py:457-508) ----
  // the real-world network (network_realworld.py:201-217): the pose rows are camera_pts_mlp(x / W, y / H, depth) | nocs_pts_mlp(nocs)
  if (arch == ARCH_REALWORLD) {
    if (int rc = launch_pose_rows(prow_w.get<float>(), bf.nocs4, call.coor1, call.coor2, bf.depth, bf.PF96, B, P, Vh, s)) return rc;
  } else if (int rc = launch_fuse_points(src.dtype, src.feat, bf.homog, depths, bf.choose, bf.prob, bf.PF96, V, B, P, D, S, S, 96, 0, s, Vh)) return rc;
  if (int rc = pose_branch(bf, Vh, call, p)) return rc;

  // ---- outputs (fp32, reference shapes) ----
  return stage_out(bf, B, out, s);
}

// pose_mlp1 -> mean -> pose_mlp2 -> mean -> the three heads + Ortho6d on the pose features PF96 of views 0 .. Vh - 1 (network_v5.py:470-508;
// network_baseline.py:643-659 is the same code)
int AdaPose::pose_branch(const Buffers& bf, int Vh, const Call& call, const ForwardPaths& p) const {
  const int P = n_pts;
  hipStream_t s = call.stream;
  // bf16 nets: the four big per-point layers of the pose MLP run in fp16 storage (fp32 they took 1.8 ms per 512 views at
  // 78 TFLOP/s on the fp32 matrix path); PF96 is produced in fp32 by its two writers and converted once
  const int pdt = pose_dtype();
  // ... and since round 7 as two launches (pose_mlp.hip): neither PF96h, Q128a nor the two 256-channel per-point tensors reach memory;
  // the slices' sums land where launch_mean_points_partial put them.  Debug flag 524288: the per-layer launches (also taken for a point
  // count that is not a whole number of slabs per slice, and for layers of another shape)
  if (p.pose_mlp) {
    PoseMlpDesc pd{};
    const ConvLayer* L[4] = {&pm1[0], &pm1[1], &pm2[0], &pm2[1]};
    for (int l = 0; l < 4; ++l) { pd.w[l] = L[l]->packs[0].w.get(); pd.ldw[l] = L[l]->packs[0].Kpad; pd.bias[l] = L[l]->bias.get<float>(); }
    pd.pf96 = bf.PF96; pd.vbias = bf.vbias; pd.q128 = bf.Q128b; pd.part128 = (float*)bf.Q128a; pd.part256 = (float*)bf.G256a; pd.V = Vh; pd.P = P;
    if (int rc = launch_pose_mlp1(pd, s)) return rc;
    if (int rc = launch_view_linear_mean((const float*)bf.Q128a, P, bf.glob, pm2_0_wfull.get<float>(), pm2_0_bias.get<float>(), bf.vbias, Vh, 128, 256, 256, 128, 0, s)) return rc;
    if (int rc = launch_pose_mlp2(pd, s)) return rc;
  } else {
    const void* pf_in = bf.PF96;
    if (pdt == F16) {
      if (int rc = launch_f32_to_f16(bf.PF96, bf.PF96h, (long long)Vh * P * pose_in(), s)) return rc;
      pf_in = bf.PF96h;
    } else if (pdt == BF16X3) {
      if (int rc = launch_f32_to_bx3(bf.PF96, bf.PF96, (long long)Vh * P * pose_in(), s)) return rc;      // in place: same 4-byte slots
    }
    if (int rc = pm1[0].run(pf_in, bf.Q128a, Vh, 1, 1, P, 128, nullptr, 0, nullptr, 0, s)) return rc;
    if (int rc = pm1[1].run(bf.Q128a, bf.Q128b, Vh, 1, 1, P, 128, nullptr, 0, nullptr, 0, s)) return rc;
    // the two means over a view's points are finished by their consumers (the slices' partial sums in Q128a / G256a: free at that point)
    if (int rc = launch_mean_points_partial(pdt, bf.Q128b, (float*)bf.Q128a, Vh, P, 128, s)) return rc;
    if (int rc = launch_view_linear_mean((const float*)bf.Q128a, P, bf.glob, pm2_0_wfull.get<float>(), pm2_0_bias.get<float>(), bf.vbias, Vh, 128, 256, 256, 128, 0, s)) return rc;
    if (int rc = pm2[0].run(bf.Q128b, bf.G256a, Vh, 1, 1, P, 256, nullptr, 0, bf.vbias, 256, s)) return rc;
    if (int rc = pm2[1].run(bf.G256a, bf.G256b, Vh, 1, 1, P, 256, nullptr, 0, nullptr, 0, s)) return rc;
    if (int rc = launch_mean_points_partial(pdt, bf.G256b, (float*)bf.G256a, Vh, P, 256, s)) return rc;
  }
  float* hout[3] = {bf.r6, bf.tv, bf.sv};
  const int hdim[3] = {6, 3, 3};
  float *hw[3][3], *hb[3][3];
  for (int h = 0; h < 3; ++h)
    for (int l = 0; l < 3; ++l) { hw[h][l] = head_w[h][l].get<float>(); hb[h][l] = head_b[h][l].get<float>(); }
  return launch_pose_heads_mean((const float*)bf.G256a, P, bf.pf2, bf.R, hw, hb, hout, hdim, Vh, s);      // + Ortho6d -> R
}

// ---- feature cache (feature_cache.hip, DESIGN.md "Feature cache") ----
// A record is what heads() reads of one view's feature map: bf.feat for 16-bit and fp32 storage, bf.featf for split pairs - preceded by
// the split-pair map where something still reads it (per-sample BN, the halo-tile conv0 and the materialised volume do).
int AdaPose::feature_parts(const Buffers& bf, const ForwardPaths& p, FeaturePart parts[2]) const {
  const size_t one = (size_t)img * img * 32;
  if (dtype != BF16X3) { parts[0] = {bf.feat, 0, one * dtype_size(dtype)}; return 1; }
  if (p.feat_form == FEAT_F32_ONLY) { parts[0] = {bf.featf, 0, one * 4}; return 1; }
  parts[0] = {bf.feat, 0, one * 4};
  parts[1] = {bf.featf, one * 4, one * 4};
  return 2;
}

size_t AdaPose::feature_bytes() const {
  Buffers bf{};
  FeaturePart parts[2];
  const int n = feature_parts(bf, paths(1), parts);
  return parts[n - 1].off + parts[n - 1].bytes;
}

size_t AdaPose::features_workspace_bytes(int V) const { return workspace_bytes((V + 1) / 2); }

int AdaPose::features(int V, const float* images, const int* slots, void* pool, int pool_records, void* workspace, size_t workspace_size,
                      const Call& call) const {
  hipStream_t s = call.stream;
  RGBM_REQUIRE(V > 0 && pool_records > 0, "features: views and pool records");
  RGBM_REQUIRE(arch != ARCH_BASELINE, "baseline network: the feature cache is not implemented");
  RGBM_REQUIRE(arch != ARCH_REALWORLD, "real-world network: the feature cache is not implemented");
  RGBM_REQUIRE(arch != ARCH_V2, "v2 network: the feature cache is not implemented");
  RGBM_REQUIRE(arch != ARCH_V1, "v1 network: the feature cache is not implemented");
  RGBM_REQUIRE(call.dropout == Dropout::None, "features: Dropout2d is on (its masks are drawn per pose and per forward, so a kept feature map would change "
               "what the net computes); the feature cache needs set_dropout(0)");
  RGBM_REQUIRE(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)pool & 15) == 0, "features: workspace must be 256-byte, pool 16-byte aligned");
  PathFacts facts = path_facts((V + 1) / 2, false);
  facts.V = V;      // any V >= 1 views enter the PSPNet
  const ForwardPaths p = forward_paths(facts);
  Buffers bf;
  if (int rc = open_workspace((V + 1) / 2, p, workspace, workspace_size, 0, "features ", "", bf)) return rc;
  if (int rc = pspnet(bf, V, images, nullptr, call, p)) return rc;
  if (int rc = feat_copy(bf, V, call, p)) return rc;
  FeaturePart parts[2];
  const int np = feature_parts(bf, p, parts);
  const size_t rec = parts[np - 1].off + parts[np - 1].bytes;
  for (int i = 0; i < np; ++i)
    if (int rc = launch_feature_store(parts[i].buf, pool, slots, V, pool_records, parts[i].off, parts[i].bytes, rec, s)) return rc;
  return 0;
}

int AdaPose::forward_cached(int B, const void* pool, int pool_records, const int* slot1, const int* slot2, const int* choose1,
                            const int* choose2, const float* P1, const float* P2, const float* depths, void* workspace,
                            size_t workspace_size, const Outputs& out, const Call& call) const {
  hipStream_t s = call.stream;
  RGBM_REQUIRE(B > 0 && pool_records > 0, "forward_cached: batch and pool records");
  RGBM_REQUIRE(arch != ARCH_BASELINE, "baseline network: the feature cache is not implemented");
  RGBM_REQUIRE(arch != ARCH_REALWORLD, "real-world network: the feature cache is not implemented");
  RGBM_REQUIRE(arch != ARCH_V2, "v2 network: the feature cache is not implemented");
  RGBM_REQUIRE(arch != ARCH_V1, "v1 network: the feature cache is not implemented");
  RGBM_REQUIRE(call.dropout == Dropout::None, "forward_cached: Dropout2d is on (its masks are drawn per pose and per forward, so a kept feature map would "
               "change what the net computes); the feature cache needs set_dropout(0)");
  RGBM_REQUIRE(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)pool & 15) == 0, "forward_cached: workspace must be 256-byte, pool 16-byte aligned");
  const ForwardPaths p = paths(B, call.dense);
  Buffers bf;
  if (int rc = open_workspace(B, p, workspace, workspace_size, 0, "", "", bf)) return rc;
  const int V = 2 * B, P = n_pts;
  if (int rc = launch_stage_in(P1, P2, choose1, choose2, bf.Pviews, bf.choose, B, P, s)) return rc;
  FeaturePart parts[2];
  const int np = feature_parts(bf, p, parts);
  const size_t rec = parts[np - 1].off + parts[np - 1].bytes;
  for (int i = 0; i < np; ++i)
    if (int rc = launch_feature_gather(pool, parts[i].buf, slot1, slot2, B, pool_records, parts[i].off, parts[i].bytes, rec, s)) return rc;
  if (int rc = launch_homography(bf.Pviews, bf.homog, V, B, s)) return rc;
  if (int rc = heads(bf, B, depths, out, call, p)) return rc;
  // a slot outside the pool: that pose's ten outputs are NaN (nothing was read for it; every other pose is what a clean call gives)
  float* const o[10] = {out.nocs1, out.nocs2, out.depth1, out.depth2, out.r1, out.r2, out.t1, out.t2, out.s1, out.s2};
  const int per[10] = {3 * P, 3 * P, P, P, 9, 9, 3, 3, 3, 3};
  return launch_feature_bad_slot_nan(slot1, slot2, B, pool_records, o, per, s);
}

}  // namespace rgbm
