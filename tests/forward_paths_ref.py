"""Path selection of the AdaPose forward as commit 4fa0cbe spells it, restated in numpy from that commit's rgbmanip_amd/csrc/adapose.cpp
(the line numbers below are that file's), where every decision was an inline condition at its point of use.  It is the reference
tests/test_forward_paths.py holds rgbm_forward_paths (csrc/forward_paths.cpp) to; it is not derived from that function.

`paths(facts)` takes an int array [n, N_FACTS] (columns: FACTS, include/rgbm.h's facts[]) and returns [n, N_PATHS] (columns: PATHS)."""
import numpy as np

F32, BF16, F16, BF16X3 = 0, 1, 2, 3
FACTS = ("arch", "dtype", "norm_mode", "cost_impl", "sparse_tail", "sparse_dec", "sweep_f16", "igemm_conv6", "fuse_final", "upconv", "stem",
         "view2_heads", "pose_x3", "flags", "stem_w", "sweep_w", "sweep_w_f16", "w11_x3", "w11_taps", "tail_ready", "tail_f16_ready", "pmlp_table",
         "psp_shape_ok", "pose_shape_ok", "dense", "V", "Vh", "n_pts")
PATHS = ("stem", "psp_stage", "up1", "up2", "up3", "feat_form", "feat_copy", "cost_body", "conv0", "conv6_igemm", "mask_level", "sweep_list",
         "tail_sparse", "vol", "bn_scratch", "point_mlp", "pose_mlp")
N_FACTS, N_PATHS = len(FACTS), len(PATHS)
DBG_PSP_STAGE_R5, DBG_POINT_MLP_R5, DBG_TILE_CONV0, DBG_POSE_MLP_R6 = 1024, 2048, 4096, 524288      # kernels.h:173-177


def paths(facts):
    facts = np.asarray(facts, np.int64)
    f = {k: facts[:, i] for i, k in enumerate(FACTS)}
    on = lambda k: f[k] != 0                                                                # noqa: E731
    flag = lambda bit: (f["flags"] & bit) != 0                                              # noqa: E731
    v5 = f["arch"] == 0
    dtype, norm_mode, cost_impl = f["dtype"], f["norm_mode"], f["cost_impl"]
    b16 = (dtype == BF16) | (dtype == F16)                                                  # :524 dtype_size(dtype) == 2
    # :294-296 feat_f32_only()
    f32_only = (dtype == BF16X3) & (cost_impl == 3) & on("sweep_w") & (norm_mode == 0) & ~flag(DBG_TILE_CONV0)
    # :301-304 feat_f16()
    f16 = ((dtype == BF16) & on("sweep_f16") & (cost_impl == 3) & on("sweep_w_f16") & (norm_mode == 0) & ~flag(DBG_TILE_CONV0) & ((f["upconv"] & 4) != 0)
           & on("tail_ready") & on("tail_f16_ready"))
    # :306-309 sparse_tail_active(dense)
    tail_active = ~on("dense") & on("sparse_tail") & (norm_mode == 0) & (cost_impl == 3) & (b16 | ((dtype == BF16X3) & on("w11_x3")))
    # :311-313 sparse_active(dense)
    sparse_ok = on("sparse_dec") & tail_active & on("sweep_w") & ~flag(DBG_TILE_CONV0)

    p = {}
    p["stem"] = on("stem") & on("stem_w")                                                   # :415
    # :451 the round-5 stage; :466-469 the one-launch stage up to kPspSmallViews = 32 views (:22); :473-478 pooling + GEMMs
    p["psp_stage"] = np.where(flag(DBG_PSP_STAGE_R5), 2, np.where((f["V"] <= 32) & on("psp_shape_ok"), 1, 0))
    p["up1"] = (f["upconv"] & 1) != 0                                                       # :498 (:486-497 samples: both bits are required)
    p["up2"] = (f["upconv"] & 2) != 0                                                       # :504
    tail_kernel = ((f["upconv"] & 4) != 0) & on("tail_ready")                               # :511
    p["up3"] = np.where(tail_kernel, 2, np.where(on("fuse_final"), 1, 0))                   # :511-516 (run_then_1x1's fuse_final != 0)
    p["feat_form"] = np.where(f32_only, 1, np.where(f16, 2, 0))                             # :510-516: plain_f32 ? 1 : feat_f16() ? 2 : 0
    p["feat_copy"] = (dtype == BF16X3) & ~f32_only                                          # :685 (and :737, :924)
    # :577-637 the three chunk bodies; the baseline network never reaches cost_volume() (:688) and plans neither buffer (:379-387)
    bn, generic = v5 & (norm_mode == 1), v5 & (norm_mode != 1) & (cost_impl == 0)           # :581, :593
    tiles = v5 & ~bn & ~generic                                                             # :600
    p["cost_body"] = np.where(bn, 1, np.where(generic, 2, np.where(tiles, 3, 0)))
    # :618 build_volume + tile(0); :621 tile(10), which is (:561-571) the 16-bit sweep (on f16 features :563), the split-pair sweep or the halo tile
    sweep16 = (cost_impl == 3) & b16 & on("sweep_w") & ~flag(DBG_TILE_CONV0)                 # :561
    sweep_x3 = (cost_impl == 3) & (dtype == BF16X3) & on("sweep_w") & ~flag(DBG_TILE_CONV0)  # :566
    conv0 = np.where(cost_impl == 1, 1, np.where(sweep16, np.where(f16, 4, 3), np.where(sweep_x3, 5, 2)))
    p["conv0"] = np.where(tiles, conv0, 0)
    p["conv6_igemm"] = tiles & (cost_impl == 3) & (b16 | (dtype == BF16X3)) & on("igemm_conv6")      # :623
    p["mask_level"] = np.where(tiles & sparse_ok, np.where(f["sparse_dec"] >= 2, 2, 1), 0)  # :604-612
    p["sweep_list"] = tiles & sparse_ok & (f["sparse_dec"] >= 2)                            # :611 with :551
    p["tail_sparse"] = tiles & tail_active                                                  # :615
    p["vol"] = v5 & ~((cost_impl >= 2) & (norm_mode == 0))                                  # :392 (:383 baseline: null)
    p["bn_scratch"] = v5 & (norm_mode == 1)                                                 # :393
    # :807; heads_baseline (:764-770) has the one-launch kernel only
    p["point_mlp"] = ~v5 | (on("pmlp_table") & ~flag(DBG_POINT_MLP_R5) & ((f["Vh"] * f["n_pts"]) % 64 == 0))
    pdt_f16 = dtype == BF16                                                                 # adapose.h:36 pose_dtype() == F16
    p["pose_mlp"] = pdt_f16 & ~flag(DBG_POSE_MLP_R6) & on("pose_shape_ok")                  # :850-856
    return np.stack([np.asarray(p[k]).astype(np.int32) for k in PATHS], axis=1)
