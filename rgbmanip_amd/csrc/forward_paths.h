// Which of its alternative kernel paths an AdaPose forward runs: the decision, and nothing else.  forward_paths is a pure function of
// plain ints (no HIP header, no device buffer, no global read), so it can be asked without a GPU (rgbm_forward_paths) and tested directly.
// AdaPose::path_facts gathers the facts once per call; plan() / pspnet() / cost_volume() / heads() / pose_branch() launch what the paths
// say.  It is the only place where an option, a debug flag, a storage type and a weight pack's existence meet.  Both structs are the int
// arrays include/rgbm.h documents entry by entry (RGBM_PATH_FACT_INTS / RGBM_PATH_INTS), in that order.
#pragma once

namespace rgbm {

struct PathFacts {
  int arch, dtype, norm_mode;      // PATH_ARCH_*, DType, 0 folded / 1 per-sample BatchNorm3d
  int cost_impl, sparse_tail, sparse_dec, sweep_f16, igemm_conv6, fuse_final, upconv, stem, view2_heads, pose_x3;      // the options
  int flags;                       // the rgbm_debug_flags word at the time of the call
  int stem_w, sweep_w, sweep_w_f16, w11_x3, w11_taps, tail_ready, tail_f16_ready, pmlp_table;      // 0 / 1: the packs create() built
  int psp_shape_ok, pose_shape_ok; // the four PSP 1x1 layers / the four per-point pose layers and the point count fit the fused kernels
  int dense, V, Vh, n_pts;         // the call: dense cost regularisation and tail, views entering the PSPNet, views that get heads, points per view
};

// PATH_ARCH_REALWORLD: v5's network on a variance cost volume (-2 ref warped); a product of two features squares their range, so no f16
// feature map and no packed-f16 sweep for it (forward_paths never answers FEAT_F16 / CONV0_SWEEP16_F16)
// PATH_ARCH_V2: network_v2.py's StereoPoseNet - PSPNet and point heads as v5, no 3-D paths (as for the baseline); its pose branch is a
// kernel of its own (v2_head.hip), so pose_mlp is never answered 1
// PATH_ARCH_V1: network.py's StereoPoseNet - as PATH_ARCH_V2 in front of the heads (no 3-D paths, split pairs write the plain fp32 map
// only); point_mlp follows v5's rule (it picks stage B's one-launch kernel); its pose rows are 128 wide, so pose_mlp is never answered 1
enum { PATH_ARCH_V5 = 0, PATH_ARCH_BASELINE = 1, PATH_ARCH_REALWORLD = 2, PATH_ARCH_V2 = 3, PATH_ARCH_V1 = 4 };
enum { STEM_GENERIC = 0, STEM_FUSED = 1 };
enum { PSP_POOLED_GEMMS = 0, PSP_ONE_LAUNCH = 1, PSP_ROUND5 = 2 };
enum { UP3_TWO_LAUNCHES = 0, UP3_FUSED_FINAL = 1, UP3_TAIL_KERNEL = 2 };
// What `final` writes and the plane sweep, the point heads and the feature cache read (the values of UpConvFinal::run's out_mode).
// FEAT_F32_ONLY, split pairs on the depth-sweeping conv0: nothing reads the split-pair map, `final` writes plain fp32 into featf.
// FEAT_F16, bf16 nets with option sweep_f16: the same bytes as f16 - three more mantissa bits, the sweep's blend in packed f16; needs the
// one-kernel up_3 + final (its epilogue knows the form) and the 16-bit sweep (the halo-tile / volume paths read the storage type).
enum { FEAT_STORAGE = 0, FEAT_F32_ONLY = 1, FEAT_F16 = 2 };
enum { COST_NONE = 0, COST_BN_PER_SAMPLE = 1, COST_GENERIC = 2, COST_TILES = 3 };      // COST_NONE: the baseline network
// row 0 of kCost3d: the body's own layer on the volume, or inside COST_TILES one of five kernels
enum { CONV0_BODY = 0, CONV0_TILE_VOLUME = 1, CONV0_TILE_WARP = 2, CONV0_SWEEP16 = 3, CONV0_SWEEP16_F16 = 4, CONV0_SWEEP_X3 = 5 };

struct ForwardPaths {
  int stem, psp_stage;             // STEM_*, PSP_*
  int up1, up2, up3;               // up_1 / up_2: 1 = low-resolution 1x1 GEMM + tap combination, 0 = x2 resize + 3x3 conv; UP3_*
  int feat_form, feat_copy;        // FEAT_*; 1 = the plain-fp32 copy of a split-pair map is a launch of its own behind the PSPNet
  int cost_body, conv0, conv6_igemm;      // COST_*, CONV0_*, 1 = conv6 on the implicit-GEMM kernel
  int mask_level, sweep_list;      // tile masks: 0 none, 1 conv7 / conv9, 2 conv1 .. conv5 too and the depth-sweeping conv0 walks the tile list
  int tail_sparse;                 // 1 = conv11 + prob only where prob is gathered (u11 is never written)
  int vol, bn_scratch;             // 1 = the workspace holds the plane-sweep volume / the per-sample BatchNorm scratch
  int point_mlp, pose_mlp;         // 1 = the one-launch point MLP / the two-launch pose MLP, 0 = per layer
};

// the debug flags the decision reads (DebugFlag, kernels.h; the others switch variants inside one launcher and stay there)
enum { PATH_FLAG_PSP_STAGE_R5 = 1024, PATH_FLAG_POINT_MLP_R5 = 2048, PATH_FLAG_TILE_CONV0 = 4096, PATH_FLAG_POSE_MLP_R6 = 1 << 19 };

int pose_storage(int dtype, int pose_x3);      // DType of the four per-point layers of the pose MLP
ForwardPaths forward_paths(const PathFacts& f);

}  // namespace rgbm
