#pragma once
#include "forward_paths.h"
#include "kernels.h"
#include "layers.h"

namespace rgbm {

struct Arena {
  char* base; size_t off; size_t cap; size_t peak;
  explicit Arena(void* b, size_t c) : base((char*)b), off(0), cap(c), peak(0) {}
  void* alloc(size_t bytes) {
    off = align_up(off, 256);
    void* p = base ? base + off : nullptr;
    off += bytes;
    if (off > peak) peak = off;
    return p;
  }
  size_t mark() const { return off; }
  void release(size_t m) { off = m; }
};

struct AdaPose {
  // which network the handle holds: network_v5.py's StereoPoseNet_with_depth, or network_baseline.py's StereoPoseNet_with_depth_baseline
  // (the cost volume and the depth-guided fusion replaced by the cross-view attention stack and depth_head: view_fusion.hip)
  // ARCH_REALWORLD, network_realworld.py's StereoPoseNet_with_depth_for_realdemo: v5 with the fused volume a variance (-2 ref warped
  // instead of ref + warped: `fusion` of the conv0 kernels) and the pose rows built from camera points (camera_pts_mlp on x / W, y / H,
  // depth in front of nocs_pts_mlp's 64 channels, pose_mlp1.0 128 wide: head_kernels.hip pose_rows_kernel) instead of depth-guided features
  // ARCH_V2, network_v2.py's StereoPoseNet: no cost regularisation and no depth; the stereo part is pointwise (ref + warped over the planes
  // -> volume_conv -> fuse_conv, all 1x1), so it is evaluated at the chosen pixels only, together with pose_mlp1 (v2_head.hip); a 64 / 128
  // wide size branch behind it, no rotation or translation head (the depth / r / t outputs are NaN)
  // ARCH_V1, network.py's StereoPoseNet: v2's pointwise stereo part with a 32-channel fuse_conv whose result is a residual on the feature
  // row (v1_head.hip, stage A), then v5's NOCS branch on those rows with instance_color's output kept as the first half of a 128-channel
  // pose row (point_mlp_kernel's rows variant, stage B) and v5's pose branch at that width; no depth (the depth outputs are NaN)
  enum { ARCH_V5 = PATH_ARCH_V5, ARCH_BASELINE = PATH_ARCH_BASELINE, ARCH_REALWORLD = PATH_ARCH_REALWORLD, ARCH_V2 = PATH_ARCH_V2, ARCH_V1 = PATH_ARCH_V1 };
  int arch = ARCH_V5;
  DevBuf v2_w;                    // v2: volume_conv (BatchNorm folded), fuse_conv and pose_mlp1 as v2_point_rows_kernel's LDS image (kernels.h: kV2HeadFloats)
  DevBuf v1_w;                    // v1: volume_conv (BatchNorm folded) and fuse_conv as v1_fused_points_kernel's LDS image (kernels.h: kV1HeadFloats)
  int fusion() const { return arch == ARCH_REALWORLD ? FUSION_VARIANCE : FUSION_SUM; }      // how the plane sweep fuses a view with its warped partner
  int pose_in() const { return arch == ARCH_REALWORLD || arch == ARCH_V1 ? 128 : 96; }      // channels of a pose row (input of pose_mlp1.0)
  DevBuf prow_w;                  // real-world: camera_pts_mlp and nocs_pts_mlp as pose_rows_kernel's LDS image (kernels.h: kPoseRowsFloats)
  int regress_pose = 1;           // baseline only: 0 = no pose branch (the six r / t / s outputs are NaN)
  DevBuf vf_w;                    // baseline: the attention stack's 32 linears (view_fusion.h: kVfWeightFloats)
  DevBuf dh_w;                    // baseline: depth_head (kDepthHeadFloats)
  int dtype = F32;
  // storage type of the pose MLP (pose_mlp1 / pose_mlp2, network_v5.py:470-494): fp16 for the bf16 throughput mode (its
  // activations are O(1); fp16 per-point features keep 11 mantissa bits, the means over points stay fp32, and the rotation
  // error stays at the 2e-3 the bf16 backbone sets), fp32 for fp32 nets and for the fp16 accuracy mode (where fp16 here would
  // raise the rotation error from 4e-5 to 3e-4)
  // storage type of the four per-point layers of the pose MLP: fp16 for bf16 nets, split pairs for split-pair nets (the exact-fp32
  // matrix path runs at a sixteenth of the bf16 rate: 1.5 ms per step for these layers), fp32 otherwise
  int pose_dtype() const { return pose_storage(dtype, pose_x3); }
  int pose_x3 = 1;
  int img = 224, n_pts = 1024, n_depth = 24;
  int img_cpad = 4;
  int max_chunk = 512;           // views per cost-volume chunk (bounds the workspace: ~80 MB per view in bf16; 512 = batch 256 in one chunk)

  // the K-split buffers (per stream) and identity matrices of this net's implicit-GEMM launches: handed to every ConvLayer below, freed with the net
  std::shared_ptr<ConvScratch> scratch = std::make_shared<ConvScratch>();
  struct Block { ConvLayer c1, c2, ds; bool has_ds = false; int stride = 1, planes = 0; };
  ConvLayer conv1;
  Block blocks[16];
  int n_blocks = 0;
  ConvLayer psp[4], up1, up2, up3, fin;
  UpConvLayer up1c, up2c;       // up_1 / up_2 as a low-resolution 1x1 GEMM + tap combination (upconv.hip)
  int sparse_dec = 2;           // with the sparse tail: 2 = every 3-D layer (and the plane sweep) only on the tiles inside the chosen pixels' dependency cones, 1 = conv7 / conv9 only, 0 = dense (A/B, and the c0 .. u9 taps)
  DevBuf stem_w;                // conv1 packed for the one-kernel stem (stem.hip; 16-bit and split-pair storage)
  int stem = 0;                 // 1: NCHW images -> conv1 7x7 + ReLU + max-pool in one kernel (default for 16-bit and split-pair storage, set in create()); 0: copy, implicit-GEMM conv, pool (materialises `conv1`)
  UpConvFinal tail;             // up_3 + final in one kernel (upconv_final.hip; 16-bit and split-pair storage)
  int upconv = 7;               // bit 0: up_1, bit 1: up_2 through UpConvLayer, bit 2: up_3 + final through UpConvFinal (16-bit / split pairs); 0 = x2 resize + 3x3 conv on the up-sampled grid, for A/B and tests
  // The ten layers of the cost regularisation, indexed as the rows of kCost3d (cost3d.h: 0..6 conv0..6, 7..9 conv7/9/11), in three forms:
  ConvLayer c3d[10];            // generic implicit-GEMM versions (kept for A/B: cost_impl = 0; conv6 of the default path)
  // norm_mode 1 (per-sample BatchNorm3d: the as-shipped train-mode behaviour at batch 1): the same ten layers without
  // BN / activation, their gamma / beta, and the in-place normalisation of bn_kernels.hip behind each of them
  int norm_mode = 0;
  ConvLayer c3d_raw[10];
  DevBuf bn_gamma[10], bn_beta[10];
  struct Tile3d { DevBuf w, bias; };
  Tile3d t3d[10];               // halo-tiled versions
  int igemm_conv6 = 1;          // bf16 + cost_impl 3: conv6 through the implicit-GEMM path instead of the halo-tile kernel
  int fuse_final = 1;           // bf16: PSPNet `final` 1x1 fused into up_3's kernel (0 = two launches; `u3` is then materialised)
  int view2_heads = 1;          // 0: the cost volume, the point heads and the pose regression run for the view-1 crops only (the view-2 outputs are
                                // filled with NaN): what `AdaPoseEstimator_v5.estimate` consumes — interface_v5.py:318-374 builds the box from
                                // view1_nocs / view1_depth / view1_r and drops the rest — at ~3/4 of the time; the backbone still runs on both views
  int sparse_tail = 1;          // cost_impl 3: evaluate conv11 + prob only where prob is gathered (0 = dense conv11, for A/B and tests)
  int sweep_f16 = 1;            // bf16 nets: `final` writes the feature map as f16 and the plane sweep blends it with packed f16 FMAs (conv0_sweep.hip; 0 = bf16 feature map, fp32 blend)
  DevBuf w11_taps;              // conv11 for the sparse tail's round-6 kernel: prob_sparse_pack's nine in-plane-tap operands (bf16x3: hi operands, then lo)
  DevBuf sweep_w_f16;           // bf16 nets: the same conv0 weights as f16 (sweep_f16)
  DevBuf sweep_w;               // conv0 weights in conv0_sweep.hip fragment order (16-bit nets; bf16x3 nets: hi + lo operand arrays of conv0_sweep_x3.hip)
  int cost_impl = 3;            // 0 generic igemm + materialised volume, 1 tiled + materialised volume, 2 tiled + fused warp,
                                // 3 = 2 with the depth-sweeping conv0 kernel (bf16; fp32 nets run 2)
  DevBuf w11_x3;                // bf16x3 nets: conv11 weights for prob_sparse (16-bit step geometry, hi operands then lo operands)
  DevBuf wprob;
  ConvLayer inst, nh[3], npm[2], pm1[2], pm2[2];
  DevBuf pm2_0_wfull;
  DevBuf pmlp_table;            // the per-point NOCS branch's six layers as point_mlp_kernel's LDS image (kernels.h: point_mlp_pack)
  DevBuf pm2_0_bias;
  DevBuf head_w[3][3], head_b[3][3];

  // Seeded Dropout2d of PSPNet (dropout.hip; set through rgbm_adapose_set_dropout): p = 0 is off.  drop_masks [drop_cap_views][kDropoutPerView]
  // holds the factors of the last forward, drop_state the device pose counter (+ the mask kernel's ticket).  Which masks a forward uses
  // is the call's business (Call::dropout); which call comes next and what the last one drew is the handle's (capi.cpp).
  float drop_p = 0.f;
  unsigned long long drop_seed = 0;
  DevBuf drop_masks;
  DevBuf drop_state;
  int drop_cap_views = 0;

  // What one call wants beyond the network's inputs and outputs.  The entry point (capi.cpp) fills it; forward() / forward_cached() pass
  // it down pspnet() / heads() / cost_volume(), none of which writes the net.  Beside it travel the call's ForwardPaths: every entry
  // point asks paths() once, and nothing below it reads an option or the debug flags again.
  enum class Dropout {
    None,            // no Dropout2d
    Loaded,          // the factors rgbm_adapose_set_dropout_masks put into drop_masks
    Draw,            // draw for poses counter .. counter + B - 1 and advance the counter
    DrawNoAdvance    // draw without advancing (the eager warm-up in front of a graph capture, which the replay draws again)
  };
  struct Call {
    hipStream_t stream = nullptr;
    int stop_after = 0;
    // a dense cost regularisation and the dense tail for this call: what options sparse_dec = 0, sparse_tail = 0 give.  The ten point
    // outputs are those of a handle built with the two options.
    bool dense = false;
    // depth_map / conf_map [Vh][img][img] fp32, Vh = 2B or, with view2_heads = 0, B: the dense head (dense_depth.hip) on every chunk's
    // u11 (needs `dense`; conf_map may be null alone).  nocs_map [Vh][img][img][3] fp32: layers 0..3 of the point MLP table on every pixel
    // (head_kernels.hip: dense_nocs_kernel), launched behind the per-point branch in heads(), so that nocs_map read at choose is the
    // point NOCS bit for bit; it needs nothing dense, and the ten outputs are the plain forward's bit for bit.
    float *depth_map = nullptr, *conf_map = nullptr, *nocs_map = nullptr;
    Dropout dropout = Dropout::None;
    // real-world network only (required there): the chosen points' normalised image coordinates (x / W, y / H) [B][P][2] fp32 of both views
    const float *coor1 = nullptr, *coor2 = nullptr;
  };

  struct Buffers {
    float *Pviews, *homog; int* choose; void* feat;
    unsigned char* masks;           // sparse cost regularisation: tile masks of the 3-D layers per view of a cost-volume chunk (prob_sparse.hip)
    int *sweep_list, *sweep_count;  // ... and the needed tiles of the depth-sweeping conv0
    float* featf;                      // bf16x3 nets: plain fp32 copy of feat (what the plane sweep and the point heads gather from)
    float *X0, *X1, *H128, *H64, *nocs4, *N32, *PF96, *prob, *depth, *Q128a, *Q128b, *G256a, *G256b;
    void* PF96h;                       // fp16 copy of PF96 (pose MLP input of 16-bit nets)
    float *glob, *vbias, *pf2, *h1, *h2, *r6, *R, *tv, *sv;
    void *imgpad, *c1, *lb[4], *pooled[4], *stage[4], *cat, *ups, *u1, *u2, *u3;
    void *vol, *c3[10];                // the plane-sweep volume (where it is materialised) and the outputs of the ten rows of kCost3d
    void* bn_scratch;
    float* fused;                      // baseline: the attention stack's output rows [V][P][32]
    void* vf_scratch;                  // ... and its scratch for one chunk of poses
  };
  struct Outputs {   // device fp32, reference shapes (network_v5.py:510-515)
    float *nocs1, *nocs2;   // [B,P,3]
    float *depth1, *depth2; // [B,P]
    float *r1, *r2;         // [B,3,3]
    float *t1, *t2, *s1, *s2;  // [B,3]
  };

  int create(const StateDict& sd, int dtype, int norm_mode = 0);
  int create_baseline(const StateDict& sd, int dtype, int regress_pose);
  int create_realworld(const StateDict& sd, int dtype);
  int create_v2(const StateDict& sd, int dtype);
  int create_v1(const StateDict& sd, int dtype);
  // the parts of a network create() / create_baseline() put together (dtype is set before)
  int create_backbone(const StateDict& sd);
  int create_cost(const StateDict& sd);
  int create_point_heads(const StateDict& sd, bool pts_mlp);
  int create_pose(const StateDict& sd);
  // Path selection (forward_paths.h): the facts of a call of B poses as this handle and the process's debug flags stand now, and what
  // forward_paths makes of them.  forward_samples() and features() set the views entering the PSPNet (PathFacts::V) themselves.
  PathFacts path_facts(int B, bool dense) const;
  ForwardPaths paths(int B, bool dense = false) const { return forward_paths(path_facts(B, dense)); }
  size_t workspace_bytes(int B) const;
  // the map rules of a call (depth_map needs dense, conf_map needs depth_map, nocs_map needs the point MLP table) are checked here
  int forward(int B, const float* img1, const float* img2, const int* choose1, const int* choose2, const float* P1,
              const float* P2, const float* depths, void* workspace, size_t workspace_size, const Outputs& out, const Call& call) const;
  // S Dropout2d samples of each of B poses from one pass over the part of the PSPNet in front of up_1's tap combination: the ten
  // outputs [S * B] (row k * B + b) of forward() on the B poses tiled S times, masks and pose counter included.  Refuses, before anything
  // is launched, a call without Dropout2d masks (call.dropout Draw or Loaded), the upconv A/B paths and the baseline network.  Eager, one
  // stream; no dense / maps, feature-cache or graph form.
  size_t samples_workspace_bytes(int B, int S) const;
  int forward_samples(int B, int S, const float* img1, const float* img2, const int* choose1, const int* choose2, const float* P1,
                      const float* P2, const float* depths, void* workspace, size_t workspace_size, const Outputs& out, const Call& call) const;
  // the workspace of a dense call: the plan holds u11 whatever the options and the call say
  size_t dense_workspace_bytes(int B) const { return workspace_bytes(B); }
  int nocs_map_of(const float* feat_f32, long long pixels, float* nocs_map, hipStream_t s) const;      // the kernel alone on an fp32 feature array
  // Feature cache: the forward split at the PSPNet's output.  features() runs the PSPNet on V >= 1 views of one image array
  // [V][3][img][img] and writes view v's record (feature_bytes() long) to pool + slots[v] * feature_bytes(); forward_cached() is
  // forward() with the PSPNet replaced by reading records slot1[b] / slot2[b].  Both refuse a call with Dropout2d (call.dropout != None).
  // A slot outside [0, pool_records) is neither written nor read; forward_cached() returns NaN outputs for such a pose.
  size_t feature_bytes() const;
  size_t features_workspace_bytes(int V) const;
  int features(int V, const float* images, const int* slots, void* pool, int pool_records, void* workspace, size_t workspace_size,
               const Call& call) const;
  int forward_cached(int B, const void* pool, int pool_records, const int* slot1, const int* slot2, const int* choose1, const int* choose2,
                     const float* P1, const float* P2, const float* depths, void* workspace, size_t workspace_size, const Outputs& out,
                     const Call& call) const;
  struct FeaturePart { void* buf; size_t off, bytes; };      // a feature buffer of the workspace and its place inside a record
  int feature_parts(const Buffers& bf, const ForwardPaths& p, FeaturePart parts[2]) const;
  int heads(const Buffers& bf, int B, const float* depths, const Outputs& out, const Call& call, const ForwardPaths& p) const;
  int heads_baseline(const Buffers& bf, int B, const Outputs& out, const Call& call, const ForwardPaths& p) const;
  int heads_v2(const Buffers& bf, int B, const float* depths, const Outputs& out, const Call& call, const ForwardPaths& p) const;
  int heads_v1(const Buffers& bf, int B, const float* depths, const Outputs& out, const Call& call, const ForwardPaths& p) const;
  // stages A and B of the v1 heads on N = Vh * P points: feat (dtype) -> fused32 [N][32], nocs4 [N][4], rows128 [N][128]; `fused_mlp` picks
  // B's one-launch kernel (N % 64 == 0) or the per-layer composition, which needs the scratch h64a [N][64], h128 [N][128], h64b [N][64], n32 [N][32]
  struct V1Scratch { float *h64a, *h128, *h64b, *n32; };
  int v1_stages(int feat_dtype, const void* feat, const float* homog, const float* depths, const int* choose, float* fused32, float* planes,
                float* nocs4, float* rows128, const V1Scratch& sc, int B, int P, int S, int Vh, bool fused_mlp, hipStream_t s) const;
  // what the point heads gather from: the feature map of this forward and its element type (fp32 copy for split pairs, f16 with FEAT_F16)
  struct FeatSource { const void* feat; int dtype; };
  FeatSource gather_source(const Buffers& bf, const ForwardPaths& p) const;
  PointMlpDesc point_mlp_desc(const Buffers& bf, const FeatSource& src, int Vh) const;      // the one-launch per-point branch on views 0 .. Vh - 1
  int stage_out(const Buffers& bf, int B, const Outputs& out, hipStream_t s) const;      // the staged point / pose results -> the ten outputs
  int pose_branch(const Buffers& bf, int Vh, const Call& call, const ForwardPaths& p) const;
  int chunk_poses(int B) const;      // baseline: poses per launch of the attention stack (max_chunk views)
  int layer4_index() const { return (3 * n_blocks) & 3; }      // which of the rotating buffers bf.lb holds the layer4 output (debug fetch)

  // exposed for layer-level tests
  int plan(int B, const ForwardPaths& p, Arena& A, Buffers& bf) const;
  // What every forward does in front of its first launch: the workspace is aligned and holds the plan of B poses behind `head` bytes
  // (forward_samples' staging block), which is laid out into bf.  The size error reads pre + "workspace too small: need N" + post.
  int open_workspace(int B, const ForwardPaths& p, void* workspace, size_t workspace_size, size_t head, const char* pre, const char* post,
                     Buffers& bf) const;
  // img2 == nullptr: all V views (any V >= 1) lie in img1
  // samples > 1: V = samples x 2B views, the 2B input views shared up to up_1's stacked GEMM (forward_samples)
  int pspnet(const Buffers& bf, int V, const float* img1, const float* img2, const Call& call, const ForwardPaths& p, int samples = 1) const;
  // behind the PSPNet, split pairs: the plain-fp32 copy of the feature map where the paths ask for it
  int feat_copy(const Buffers& bf, int V, const Call& call, const ForwardPaths& p) const;
  int cost_volume(const Buffers& bf, int V, int B, const float* depths, const Call& call, const ForwardPaths& p) const;
  int chunk_views(int V) const;
};

const char* last_error_cstr();

}  // namespace rgbm
