#include "forward_paths.h"

#include "../../include/rgbm.h"

namespace rgbm {

int pose_storage(int dtype, int pose_x3) { return dtype == RGBM_BF16 ? RGBM_F16 : (dtype == RGBM_BF16X3 && pose_x3) ? RGBM_BF16X3 : RGBM_F32; }

ForwardPaths forward_paths(const PathFacts& f) {
  ForwardPaths p = {};
  const bool b16 = f.dtype == RGBM_BF16 || f.dtype == RGBM_F16;      // 16-bit storage: the depth-sweeping conv0, implicit-GEMM conv6 and the sparse tail exist for these
  const bool x3 = f.dtype == RGBM_BF16X3;
  const bool eval_bn = f.norm_mode == 0;
  // debug flag 4096: the halo-tile conv0 instead of either depth-sweeping kernel, in every storage type (the runtime way out should a
  // compiler update bring the sweep kernels' hand-counted asm gathers out of step)
  const bool v2 = f.arch == PATH_ARCH_V2 || f.arch == PATH_ARCH_V1;      // no cost regularisation: nothing below may depend on its options
  const bool sweep = !v2 && f.cost_impl == 3 && !(f.flags & PATH_FLAG_TILE_CONV0);

  // ---- PSPNet ----
  p.stem = f.stem && f.stem_w ? STEM_FUSED : STEM_GENERIC;
  // small batches (the deployment shape, B = 1 .. 8): pooling and the four 512 -> 128 convs of the 50 cells per view in one launch
  const int kPspSmallViews = 32;
  p.psp_stage = (f.flags & PATH_FLAG_PSP_STAGE_R5) ? PSP_ROUND5 : (f.V <= kPspSmallViews && f.psp_shape_ok) ? PSP_ONE_LAUNCH : PSP_POOLED_GEMMS;
  p.up1 = f.upconv & 1;
  p.up2 = (f.upconv >> 1) & 1;
  p.up3 = (f.upconv & 4) && f.tail_ready ? UP3_TAIL_KERNEL : f.fuse_final ? UP3_FUSED_FINAL : UP3_TWO_LAUNCHES;
  // sweep_w_f16 exists only for conv0 weights that f16 can hold, tail_f16_ready only for such `final` weights: otherwise all bf16
  // (the v2 and v1 networks only gather from the map: nothing of them reads split pairs)
  if (x3 && (v2 || (sweep && f.sweep_w && eval_bn))) p.feat_form = FEAT_F32_ONLY;
  else if (f.arch != PATH_ARCH_REALWORLD && f.dtype == RGBM_BF16 && f.sweep_f16 && sweep && f.sweep_w_f16 && eval_bn && p.up3 == UP3_TAIL_KERNEL && f.tail_f16_ready) p.feat_form = FEAT_F16;
  else p.feat_form = FEAT_STORAGE;
  // split pairs: everything that GATHERS from the feature map (plane sweep, point heads) reads a plain fp32 copy of it
  p.feat_copy = x3 && p.feat_form != FEAT_F32_ONLY;

  // ---- cost regularisation (the baseline, the v2 and the v1 network have none) ----
  if (f.arch != PATH_ARCH_BASELINE && !v2) {
    p.cost_body = !eval_bn ? COST_BN_PER_SAMPLE : f.cost_impl == 0 ? COST_GENERIC : COST_TILES;
    p.vol = !(f.cost_impl >= 2 && eval_bn);      // the fused-warp and depth-sweeping conv0 never materialise it
    p.bn_scratch = !eval_bn;
    if (p.cost_body == COST_TILES) {
      p.conv0 = f.cost_impl == 1 ? CONV0_TILE_VOLUME
              : sweep && b16 && f.sweep_w ? (p.feat_form == FEAT_F16 ? CONV0_SWEEP16_F16 : CONV0_SWEEP16)
              : sweep && x3 && f.sweep_w ? CONV0_SWEEP_X3 : CONV0_TILE_WARP;
      // conv6 (64 -> 64, K = 27 x 64): a plain GEMM shape, 2.7x faster on the role-specialised implicit-GEMM kernel
      p.conv6_igemm = f.cost_impl == 3 && (b16 || x3) && f.igemm_conv6;
      // the sparse tail runs in a call that is not dense; with it the layers skip tiles outside the chosen pixels' dependency cones
      p.tail_sparse = !f.dense && f.sparse_tail && f.cost_impl == 3 && (b16 || (x3 && f.w11_x3));
      p.mask_level = f.sparse_dec != 0 && p.tail_sparse && sweep && f.sweep_w ? (f.sparse_dec >= 2 ? 2 : 1) : 0;
      p.sweep_list = p.mask_level == 2;
    }
  }

  // ---- heads ----
  // the baseline network has the one-launch point MLP only (heads_baseline refuses what it cannot run)
  p.point_mlp = f.arch == PATH_ARCH_BASELINE || (f.pmlp_table && !(f.flags & PATH_FLAG_POINT_MLP_R5) && ((long long)f.Vh * f.n_pts) % 64 == 0);
  // (the real-world network's pose_mlp1.0 is 128 wide: pose_shape_ok asks for 96, so its pose MLP runs per layer)
  p.pose_mlp = !v2 && pose_storage(f.dtype, f.pose_x3) == RGBM_F16 && !(f.flags & PATH_FLAG_POSE_MLP_R6) && f.pose_shape_ok;
  return p;
}

}  // namespace rgbm
