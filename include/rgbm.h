/* rgbm.h — C ABI of librgbm_hip.so (MI355X / gfx950).
 *
 * The reference (hyperplane-lab/RGBManip) is pure Python and has no FFI: its "plugin ABI" for this path is the
 * set of Python classes selected by Hydra name strings.  Each entry point below states which reference
 * interface it stands in for (paths relative to /root/reference).  The Python classes in rgbmanip_amd/ mirror
 * those interfaces and bind these functions through ctypes.
 *
 * Conventions: every function returns 0 on success, a negative code on error (rgbm_last_error() has the text);
 * all `*_dev` / device pointers are HIP device memory owned by the caller (e.g. the PyTorch caching allocator);
 * all work is enqueued on `stream` (a hipStream_t passed as void*; NULL = default stream) with no hidden
 * synchronisation; handles own only their packed weights; a handle is not thread-safe, distinct handles are.
 * Forwards on different streams may overlap on the device (round 4: they differed intermittently from the one-stream result until the library was
 * built without packed fp32 instructions; tools/check_two_stream_forwards.py is the regression check, DESIGN.md section 5d has the finding).
 * dtype: 0 = fp32 (exact-fp32 MFMA, the parity gate), 1 = bf16 storage + fp32 accumulate (throughput mode).
 */
#ifndef RGBM_H_
#define RGBM_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RGBM_VERSION 100
#define RGBM_F32 0
#define RGBM_BF16 1
#define RGBM_F16 2       /* IEEE half storage (saturating stores), fp32 accumulation; same kernels as RGBM_BF16 */
#define RGBM_BF16X3 3    /* split pairs: every value kept as bf16 hi + bf16 lo (16 significand bits, 4 bytes, fp32 tensor layout with
                            each 16-byte chunk of 4 channels holding {hi01, hi23, lo01, lo23}); products hi*hi + lo*hi + hi*lo on
                            the bf16 matrix pipe, fp32 accumulation: fp32-level results (1e-4 gate) at 3 MFMAs per product */

int rgbm_version(void);
const char* rgbm_last_error(void);

/* ------------------------------------------------------------------------------------------------------------
 * AdaPose estimator network.
 * Replaces: StereoPoseNet_with_depth.__init__/load_state_dict and .forward
 *   models/pose_estimator/AdaPose/lib/network_v5.py:301-376, 418-519   (called from interface_v5.py:43-56, 279-280)
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct rgbm_weight_desc {
  const char* name;        /* state_dict key, with or without the DataParallel "module." prefix */
  const float* data;       /* host fp32, contiguous, PyTorch layout */
  int ndim;
  const int64_t* shape;
} rgbm_weight_desc;

typedef struct rgbm_adapose rgbm_adapose_t;

typedef struct rgbm_adapose_out {   /* device fp32, shapes of the reference's output dict (network_v5.py:510-515) */
  float *view1_nocs, *view2_nocs;   /* [B,1024,3] */
  float *view1_depth, *view2_depth; /* [B,1024]   */
  float *view1_r, *view2_r;         /* [B,3,3]    */
  float *view1_t, *view2_t;         /* [B,3]      */
  float *view1_s, *view2_s;         /* [B,3]      */
} rgbm_adapose_out;

/* dtype: RGBM_F32 (parity mode), RGBM_BF16 (throughput mode) or RGBM_F16.
 * norm_mode: 0 = eval-mode BatchNorm3d folded into the convs (the default and the benchmarked path);
 *            1 = per-sample statistics: every BatchNorm3d of the cost-regularisation net normalises a view's volume with that
 *                volume's own biased mean / variance — what the reference as shipped computes (interface_v5.py:39-56 never calls
 *                .eval() and runs one pose per call), with Dropout2d as identity unless rgbm_adapose_set_dropout turns it on.  Generic
 *                kernels, materialised volume. */
int rgbm_adapose_create(rgbm_adapose_t** h, int device, const rgbm_weight_desc* w, int n_w, int dtype, int norm_mode);
int rgbm_adapose_destroy(rgbm_adapose_t* h);

/* The baseline network, StereoPoseNet_with_depth_baseline (lib/network_baseline.py:523-669; interface_baseline.py builds it): v5's PSPNet
 * and point heads, with the plane-sweep cost volume and the depth-guided fusion replaced by ViewFusion(32, 4 heads, depth 4)
 * (lib/fusion.py) between the two views' gathered rows and a per-point depth_head (32 -> 64 -> 32 -> 1, ReLUs).  DESIGN.md section 5m.
 * rgbm_adapose_create_baseline: the same handle type from a baseline state dict (img_extractor.*, instance_color, nocs_head,
 *   view_fusion.blocks.{0..3}.fusion{1,2}.linears.{0..3}.{weight,bias}, depth_head.{0,2,4} and, with regress_pose = 1, nocs_pts_mlp,
 *   pose_mlp1 / pose_mlp2 and the three estimators); a missing weight is reported by name.  dtype is the PSPNet's storage type; the
 *   attention stack, depth_head and the point heads are fp32 whatever it is.
 *   On such a handle rgbm_adapose_workspace_bytes, rgbm_adapose_forward(_ex) and rgbm_adapose_fetch work: the arguments are unchanged,
 *   P1 / P2 / depths are not read (the reference ignores them) and may be NULL; with regress_pose = 0 the six r / t / s outputs are NaN.
 *   Options view2_heads (0: view 2's nocs_head, depth_head, pose branch and the last block's fusion2 are skipped and its five outputs
 *   are NaN; its rows still feed every block's keys), max_chunk (the attention stack runs max_chunk / 2 poses at a time), stem, upconv
 *   and fuse_final are honoured; the cost-volume options (cost_impl, sparse_tail, sparse_dec, sweep_f16, igemm_conv6) are errors.
 *   rgbm_adapose_fetch also serves "fused1" / "fused2" [B][P][32].  Refused, with nothing launched: rgbm_adapose_forward_dense /
 *   _forward_maps, rgbm_adapose_set_dropout with p > 0 and _set_dropout_masks, the feature-cache calls, rgbm_adapose_forward_graph.
 * rgbm_view_fusion: the attention stack alone with the handle's weights.  x1 / x2 [B][P][32] fp32 (the two views' rows, point-major) ->
 *   y1 / y2 [B][P][32]; P a multiple of 32 in [32, 4096], 1 <= B <= 65535, 16-byte aligned buffers, outputs distinct from inputs.  All
 *   arithmetic is fp32 (q k^T on the fp32 matrix pipe, the rest FMAs); keys are walked in tiles with a running maximum and sum, so no score
 *   reaches memory and scores of +-200 are exact to fp32.  A pose's result does not depend on B and is the same bytes on every call.
 *   scratch: rgbm_view_fusion_scratch_bytes(B, P) bytes (ten [B][P][32] fp32 buffers), 16-byte aligned, contents irrelevant.
 * rgbm_depth_head: x [n_rows][32] fp32 -> out [n_rows] fp32 with the handle's depth_head. */
int rgbm_adapose_create_baseline(rgbm_adapose_t** h, int device, const rgbm_weight_desc* w, int n_w, int dtype, int regress_pose);
int rgbm_view_fusion(rgbm_adapose_t* h, const float* x1, const float* x2, int B, int P, float* y1, float* y2, void* scratch,
                     size_t scratch_bytes, void* stream);
int rgbm_view_fusion_scratch_bytes(int B, int P, size_t* bytes);
int rgbm_depth_head(rgbm_adapose_t* h, const float* x, int64_t n_rows, float* out, void* stream);
/* The real-world network, StereoPoseNet_with_depth_for_realdemo (lib/network_realworld.py; interface_realworld.py builds it): v5 with two
 * pieces exchanged.  DESIGN.md section 5r.
 *   - The fused plane-sweep volume is a variance: per view ref^2 + warped^2 - (ref + warped)^2 = -2 ref warped channel by channel
 *     (network_realworld.py:145-166) where v5 has ref + warped; 0 where the partner view projects outside the image.  Every conv0 form this
 *     network reaches takes the fusion as a compile-time parameter: the voxel is one fp32 product of the existing bilinear sum, rounded
 *     once to the voxel's storage.  The packed-f16 forms do not (a product of two features squares their range, f16 saturates at 65504):
 *     rgbm_forward_paths never answers paths[5] = 2 or paths[8] = 4 for arch 2, option sweep_f16 = 1 is an error, and dtype RGBM_F16 is
 *     refused at create.  Everything behind conv0 is v5's code.
 *   - The pose rows are camera_pts_mlp(x / W, y / H, depth) [64] in front of nocs_pts_mlp(nocs) [64] (one kernel, fp32, weights in LDS);
 *     pose_mlp1.0 is 128 -> 128 and the pose MLP runs per layer.  There is no depth-guided fusion.
 * rgbm_adapose_create_realworld: the same handle type from v5's keys plus camera_pts_mlp.{0,2}.{weight,bias}, pose_mlp1.0.weight
 *   [128][128][1]; a missing weight is reported by name ("missing weight <key>") and what was uploaded is freed.
 * rgbm_adapose_forward_realworld: rgbm_adapose_forward_ex with two more inputs, coor1 / coor2 [B][P][2] fp32 device: the chosen points'
 *   pixel coordinates in the uncropped frame divided by its width and height (interface_realworld.py:264-269; rgbm_pts2d_to_coor).  The
 *   other forwards refuse such a handle, as do Dropout2d, the feature cache, forward_samples and hipGraph replay.  Options view2_heads,
 *   cost_impl, sparse_tail, sparse_dec, igemm_conv6, max_chunk, stem, upconv and fuse_final work as for v5; rgbm_adapose_fetch's "pf96"
 *   holds the [2B][P][128] pose rows.
 * rgbm_pts2d_to_coor: coor[i] = (pts2d[i][0] / W, pts2d[i][1] / H), n_points pairs, true IEEE float32 divisions (640 and 480 are no
 *   powers of two: a reciprocal multiply rounds differently).
 * rgbm_pose_rows: the pose-rows kernel alone with the handle's weights (tests, timing).  Views are ordered [view-1 poses ; view-2 poses];
 *   nocs4 [views * P][4] fp32 (x, y, z, unused), depth [views * P] fp32, coor1 / coor2 [B][P][2] (coor2 may be NULL with views = B) ->
 *   rows [views * P][128] fp32, 16-byte aligned; views = B or 2 B. */
int rgbm_adapose_create_realworld(rgbm_adapose_t** h, int device, const rgbm_weight_desc* w, int n_w, int dtype);
int rgbm_adapose_forward_realworld(rgbm_adapose_t* h, int B, const float* img1, const float* img2, const int32_t* choose1, const int32_t* choose2,
                                   const float* coor1, const float* coor2, const float* P1, const float* P2, const float* depths, void* workspace,
                                   size_t workspace_bytes, const rgbm_adapose_out* out, int stop_after, void* stream);
int rgbm_pts2d_to_coor(const float* pts2d_dev, float* coor_dev, int64_t n_points, int W, int H, void* stream);
int rgbm_pose_rows(rgbm_adapose_t* h, const float* nocs4, const float* coor1, const float* coor2, const float* depth, float* rows, int B, int P,
                   int views, void* stream);
/* The v2 network, StereoPoseNet (lib/network_v2.py; interface_v2.py builds it): v5's PSPNet and NOCS branch, no cost regularisation and no
 * depth.  Its stereo part is pointwise - ref + warped over the 24 planes, volume_conv (three 1x1x1 Conv3d + BatchNorm + ReLU, 32 -> 16 ->
 * 8 -> 1), fuse_conv (1x1 Conv2d 24 -> 32, ReLU, 32 -> 64), a gather at `choose` - so one kernel evaluates it at the chosen pixels only,
 * with pose_mlp1 (64 -> 64 -> 64) behind it, in fp32 whatever the storage type: no volume exists in memory.  pose_mlp2 (128 -> 128 -> 128)
 * and size_estimator (128 -> 128 -> 64 -> 3) follow; every mean over a view's points is finished in a fixed order.  DESIGN.md section 5s.
 * rgbm_adapose_create_v2: the same handle type from a StereoPoseNet state dict (eval BatchNorm folded at create); all four storage types;
 *   a missing weight is reported by name.  rgbm_adapose_forward / _forward_ex serve the handle: view*_nocs and view*_s are written,
 *   view*_depth / _r / _t are NaN (this network has none), and with option view2_heads = 0 the view-2 outputs are NaN too.  The dense /
 *   maps forwards, forward_realworld, forward_samples, the feature cache, Dropout2d and hipGraph replay refuse the handle by name; the
 *   cost-volume options are errors.  rgbm_adapose_fetch knows "v2_rows" [2B][P][64] (pose_mlp1's output), "v2_fuse" [2B][P][64]
 *   (fuse_conv's output at the chosen pixels) and "v2_planes" [2B][P][24] (volume_conv's) besides the PSPNet taps.
 * rgbm_v2_point_rows: the kernel alone with the handle's weights (tests, timing).  feat [2B][S][S][32] fp32 maps, views ordered
 *   [view-1 poses ; view-2 poses]; choose [views * P] pixel indices into the S x S crop; P_views [2B][16] the views' projections,
 *   depths [B][24]; homog_scratch 2B x 12 floats -> rows [views * P][64], and, where not NULL, fuse64 [views * P][64] and planes
 *   [views * P][24]; views = B or 2 B; feat, rows and fuse64 16-byte aligned.  A view whose projection cannot be inverted gets NaN rows, no other view does. */
int rgbm_adapose_create_v2(rgbm_adapose_t** h, int device, const rgbm_weight_desc* w, int n_w, int dtype);
int rgbm_v2_point_rows(rgbm_adapose_t* h, const float* feat, const int32_t* choose, const float* P_views, const float* depths, float* homog_scratch,
                       float* rows, float* fuse64, float* planes, int B, int P, int S, int views, void* stream);
/* The v1 network, StereoPoseNet (lib/network.py; interface.py builds it): v2's pointwise stereo part with a 32-channel fuse_conv whose
 * result is a residual on the feature row, fused = relu(feat + fuse_conv(volume_conv(ref + warped))), then v5's heads on the new rows:
 * instance_color 32 -> 64, nocs_head, nocs_pts_mlp, pose rows cat(instance_color 64, nocs_pts_mlp 64) = 128 channels, pose_mlp1 / pose_mlp2
 * at v5's widths and the three regression heads with Ortho6d.  No depth.  Two launches at the chosen pixels, fp32 whatever the storage
 * type: stage A (v1_fused_points_kernel) writes the residual rows, stage B (point_mlp_kernel on rows) the NOCS and the pose rows.
 * DESIGN.md section 5t.
 * rgbm_adapose_create_v1: the same handle type from that class's state dict (eval BatchNorm folded at create); all four storage types; a
 *   missing weight is reported by name.  rgbm_adapose_forward / _forward_ex serve the handle: view*_nocs, _r, _t and _s are written,
 *   view*_depth is NaN, and with option view2_heads = 0 the view-2 outputs are NaN too.  The dense / maps forwards, forward_realworld,
 *   forward_samples, the feature cache (rgbm_adapose_feature_bytes included), Dropout2d and hipGraph replay refuse the handle by name;
 *   the cost-volume options are errors.  rgbm_adapose_fetch knows "v1_fused" [2B][P][32] (stage A's rows), "v1_planes" [2B][P][24]
 *   (volume_conv's) and "v1_rows" [2B][P][128] (the pose rows) besides the PSPNet taps.
 * rgbm_v1_point_rows: stages A and B alone with the handle's weights (tests, timing).  feat, choose, P_views, depths, homog_scratch, B, P,
 *   S and views as for rgbm_v2_point_rows -> fused32 [views * P][32]; where not NULL, planes [views * P][24]; nocs4 [views * P][4] and
 *   rows128 [views * P][128] are NULL together (stage A alone) or given together.  Stage B is one launch when views * P is a multiple of
 *   64 and debug flag 2048 is off; otherwise it runs per layer and needs layer_scratch (views * P * 288 floats; may be NULL else).  feat
 *   and every output 16-byte aligned: a misaligned buffer is refused before any launch.  A view whose projection cannot be inverted
 *   gets NaN rows, no other view does. */
int rgbm_adapose_create_v1(rgbm_adapose_t** h, int device, const rgbm_weight_desc* w, int n_w, int dtype);
int rgbm_v1_point_rows(rgbm_adapose_t* h, const float* feat, const int32_t* choose, const float* P_views, const float* depths, float* homog_scratch,
                       float* fused32, float* nocs4, float* rows128, float* planes, float* layer_scratch, int B, int P, int S, int views,
                       void* stream);
/* views per cost-volume chunk (default 512 = batch 256 in one chunk); bounds the workspace */
int rgbm_adapose_set_chunk(rgbm_adapose_t* h, int max_chunk_views);
/* options: "max_chunk" (views per cost-volume chunk), "fuse_final" (bf16 only; 1 [default] = PSPNet's final 1x1 runs inside
 * up_3's kernel and the 64-channel up_3 output is never written; 0 = two launches), "sparse_tail" (bf16 + cost_impl 3 only; 1 [default] = conv11, the
 * skip add, the prob conv, softmax and depth are evaluated only on the 3x3 neighbourhoods of the chosen pixels and u11
 * is never written; 0 = dense conv11 + gathering prob kernel), "cost_impl" (3 = 2 with the depth-sweeping conv0 kernel [default for bf16;
 * fp32 nets run 2]; 2 = halo-tiled 3-D convs with the plane-sweep volume fused into conv0's loader; 1 = halo-tiled convs on a materialised volume; 0 = generic implicit
 * GEMM on a materialised volume), "igemm_conv6" (1 [default] = conv6 of the cost regularisation on the implicit-GEMM kernel), "upconv" (bit 0 / 1:
 * PSPUpsample up_1 / up_2 as a 1x1 GEMM at the low resolution + tap combination, bit 2: up_3 + `final` in one kernel from the
 * half-resolution tensor [16-bit and split-pair nets]; default 7; 0 = x2 resize followed by the 3x3 conv, the reference's operator
 * order), "stem" (1 [default for 16-bit and split-pair nets] = conv1 7x7 + ReLU + max-pool in one kernel from the NCHW images; 0 = padded
 * NHWC copy, implicit-GEMM conv, pool kernel — the only path that materialises the `conv1` tap of rgbm_adapose_fetch).
 * "sparse_dec" (sparse cost regularisation with the sparse tail: the probability volume is read only at the chosen pixels, so every 3-D
 * layer has a dependency cone per axis; 2 [default] = the plane sweep, conv1..conv5, conv7 and conv9 run only on the tiles inside those
 * cones — c0..c5 / u7 / u9 are undefined elsewhere, every network output is bit-identical; 1 = conv7 / conv9 only; 0 = dense).
 * "view2_heads" (1 [default] = all ten outputs; 0 = the probability volume, the point heads and the pose regression run for the
 * view-1 crops only and the five view-2 outputs are filled with NaN: what AdaPoseEstimator_v5.estimate consumes,
 * interface_v5.py:318-374, at about three quarters of the time; the backbone still runs on both views).
 * "sweep_f16" (bf16 nets with cost_impl 3 and upconv bit 2; 1 [default since round 5] = `final` writes the 32-channel feature map as f16
 * instead of bf16 - same bytes, three more mantissa bits - and the plane sweep (persistent conv0_sweep kernel) blends it with packed f16
 * FMAs and multiplies with f16 MFMAs; c0 and everything behind it stay bf16.  Features beyond +-65504 saturate, as in an fp16 net; 0 =
 * bf16 feature map and the fp32 blend of rounds 1-4.  The "feat" tap of rgbm_adapose_fetch converts from whichever form was written.
 * With 1 the one-kernel up_3 + `final` also runs its tap combination, PReLU and `final` in packed f16: faster, and closer to fp32).
 * Set before querying the workspace size.
 * Where an option applies only to some storage types, cost_impl values or weight packs, the rule is stated once, in code: the paths[]
 * entry of rgbm_forward_paths (below) named here.  fuse_final: [4].  sparse_tail: [12].  cost_impl: [7] [8] [13].  igemm_conv6: [9].
 * upconv: [2] [3] [4].  stem: [0].  sparse_dec: [10] [11].  sweep_f16: [5] and [8].  view2_heads: facts [26]. */
int rgbm_adapose_set_option(rgbm_adapose_t* h, const char* key, int value);
/* Path selection: which of its alternative kernel paths a forward runs, decided in one pure function (csrc/forward_paths.cpp) of plain
 * ints.  rgbm_forward_paths never touches the HIP runtime (works without a GPU): facts [n_rows][RGBM_PATH_FACT_INTS] ->
 * paths [n_rows][RGBM_PATH_INTS], row by row.
 *   facts: [0] arch 0 v5 / 1 baseline / 2 real-world (v5's paths, never paths[5] = 2 or paths[8] = 4) / 3 v2 (no 3-D paths: [7] .. [14] and [16] are 0; split pairs: [5] = 1) / 4 v1 (as 3: paths [7] .. [14] are 0, [15] by v5's rule, [16] = 0)  [1] dtype (RGBM_F32 ..)  [2] norm_mode
 *     [3] cost_impl [4] sparse_tail [5] sparse_dec [6] sweep_f16 [7] igemm_conv6 [8] fuse_final [9] upconv [10] stem [11] view2_heads: the
 *     options of rgbm_adapose_set_option  [12] pose_x3 (1: split-pair nets run the per-point pose layers on split pairs)
 *     [13] the rgbm_debug_flags word (negative: the process's current one, as rgbm_conv_plan takes it); read here: 1024 (PSP stage of rounds 1-5), 2048 (per-layer point MLP), 4096 (halo-tile conv0
 *     instead of the depth-sweeping kernels), 524288 (per-layer pose MLP)
 *     0 / 1, what the handle's create built:  [14] one-kernel stem pack  [15] depth-sweeping conv0 pack  [16] its f16 form (bf16 nets whose
 *     conv0 weights f16 can hold)  [17] conv11 split-pair pack of the sparse tail  [18] conv11 in-plane-tap pack  [19] one-kernel up_3 + final
 *     [20] its f16 form  [21] point MLP table  [22] the four PSP 1x1 layers fit the one-launch stage  [23] the four per-point pose layers
 *     and the point count fit the fused pose MLP
 *     the call:  [24] dense  [25] views entering the PSPNet  [26] views that get heads  [27] points per view
 *   paths: [0] stem: 0 copy + implicit-GEMM conv + pool, 1 one kernel (option stem and [14])
 *     [1] PSP stage: 0 pooling + four implicit GEMMs, 1 pooling and the 50 cells per view in one launch (at most 32 views and [22]),
 *         2 rounds 1-5 (flag 1024)
 *     [2] up_1  [3] up_2: 1 = 1x1 GEMM at the low resolution + tap combination (upconv bit 0 / 1), 0 = x2 resize + 3x3 conv
 *     [4] up_3 + final: 2 one kernel from the half-resolution tensor (upconv bit 2 and [19]), else 1 `final` inside up_3's kernel
 *         (fuse_final) or 0 two launches
 *     [5] feature map: 0 the storage type; 1 plain fp32 only (split pairs, cost_impl 3, [15], norm_mode 0, not flag 4096: nothing reads
 *         the split-pair map); 2 f16 (bf16, sweep_f16, cost_impl 3, [16], norm_mode 0, not flag 4096, paths [4] = 2 and [20])
 *     [6] 1 = the split-pair map is copied to plain fp32 by a launch of its own (split pairs without [5] = 1)
 *     [7] cost regularisation: 0 none (baseline, v2), 1 per-sample BatchNorm3d on generic layers (norm_mode 1), 2 generic implicit GEMM
 *         (cost_impl 0), 3 halo tiles
 *     [8] conv0: 0 the layer of body 1 / 2 on the materialised volume; in body 3: 1 halo tile on the volume (cost_impl 1), 2 halo tile with
 *         the plane sweep fused in, 3 depth-sweeping kernel (16-bit storage, cost_impl 3, [15], not flag 4096), 4 the same on f16 features
 *         ([5] = 2), 5 split-pair depth-sweeping kernel (same conditions)
 *     [9] 1 = conv6 on the implicit-GEMM kernel (body 3, cost_impl 3, 16-bit or split-pair storage, igemm_conv6)
 *     [10] tile masks: 0 none, 1 conv7 / conv9, 2 conv1 .. conv5 too (sparse_dec, [12], cost_impl 3, [15], not flag 4096)
 *     [11] 1 = the depth-sweeping conv0 walks the list of needed tiles ([10] = 2)
 *     [12] 1 = sparse tail (sparse_tail, not a dense call, body 3, cost_impl 3, 16-bit storage or split pairs with [17])
 *     [13] 1 = the workspace holds the plane-sweep volume (v5 and not (cost_impl >= 2 and norm_mode 0))  [14] ... the BatchNorm scratch (body 1)
 *     [15] point MLP: 1 one launch ([21], not flag 2048, [26] x [27] a multiple of 64; the baseline network: always), 0 per layer
 *     [16] pose MLP: 1 two fused launches (bf16 nets, [23], not flag 524288), 0 per layer
 * rgbm_adapose_paths: the handle's own facts for a call of B poses (dense = 1: a rgbm_adapose_forward_dense call) under the process's
 * current debug flags, and the paths a forward issued now would run.  Launches nothing. */
#define RGBM_PATH_FACT_INTS 28
#define RGBM_PATH_INTS 17
int rgbm_forward_paths(const int32_t* facts, int n_rows, int32_t* paths);
int rgbm_adapose_paths(rgbm_adapose_t* h, int B, int dense, int32_t* facts_out, int32_t* paths_out);
int rgbm_adapose_workspace_bytes(rgbm_adapose_t* h, int B, size_t* bytes);
/* Seeded Dropout2d of PSPNet (pspnet.py:122,150,154: p = 0.15 after up_1 and after up_2), active in the reference as shipped
 * (interface_v5.py:39-56 never calls .eval()).  p = 0 is off (the default: no kernel changes); otherwise 0 < p < 1.  Every
 * (pose, view, site, channel) gets one keep decision, a pure function of (seed, global pose index, view, site, channel)
 * (DESIGN.md "Seeded Dropout2d"): kept channels are scaled by fp32(1 / (1 - p)), dropped ones zeroed, in the epilogue of the
 * tap combination that writes up_1 / up_2 (option upconv bits 0 and 1 are required).  The global pose index of pose b of a forward is
 * a device counter + b; the forward advances the counter by B, so masks do not depend on how poses are batched, chunked or replayed
 * from a graph (a replay draws fresh masks).  set_dropout resets the counter to 0 after synchronising the device and invalidates
 * captured graphs.  Forwards with dropout on, issued to one handle from two streams at the same time, share the counter and the
 * factor buffer: unsupported (the same rule as the per-stream K-split scratch of rgbm_adapose_forward_graph). */
int rgbm_adapose_set_dropout(rgbm_adapose_t* h, float p, uint64_t seed);
/* The factors the last forward used (drawn or set), batch B: out_dev [2B][320] fp32, views = the view-1 crops of the batch, then the
 * view-2 crops; per view up_1's 256 channels, then up_2's 64.  Synchronises the device. */
int rgbm_adapose_dropout_masks(rgbm_adapose_t* h, int B, float* out_dev);
/* Explicit factors (same layout) for the next forward of batch B, which uses them instead of drawing and does not advance the counter
 * (whether or not set_dropout is on); a forward_graph call runs that forward eagerly.  Synchronises the device. */
int rgbm_adapose_set_dropout_masks(rgbm_adapose_t* h, int B, const float* masks_dev);
/* img1/img2 [B,3,224,224] fp32 NCHW normalised; choose1/2 [B,1024] int32; P1/P2 [B,4,4] fp32; depths [B,24] fp32.
 * Same argument meaning as network_v5.py:418 (view1_img, view1_choose, view2_img, view2_choose, view1_proj,
 * view2_proj, depth_values).  workspace must be 256-byte aligned. */
int rgbm_adapose_forward(rgbm_adapose_t* h, int B, const float* img1, const float* img2, const int32_t* choose1,
                         const int32_t* choose2, const float* P1, const float* P2, const float* depths, void* workspace,
                         size_t workspace_bytes, const rgbm_adapose_out* out, void* stream);

/* S Dropout2d samples of each of B poses from one pass over the shared part of the backbone.
 * rgbm_adapose_forward_samples: the inputs of rgbm_adapose_forward for B poses; the ten outputs in `out` have leading dimension S * B,
 *   row s * B + b = sample s of pose b.  The result is DEFINED as what rgbm_adapose_forward returns for the batch of S * B poses that is
 *   the B poses tiled S times, with the masks that forward would draw: pose s * B + b has global pose index counter + s * B + b, the counter
 *   advances by S * B, rgbm_adapose_dropout_masks(h, S * B, ..) afterwards returns those [2 S B][320] factors in the usual order (the view-1
 *   rows, then the view-2 rows), and masks loaded with rgbm_adapose_set_dropout_masks for S * B poses are used once, as by a plain forward.
 *   Both Dropout2d sites lie behind up_1's stacked GEMM, so the stem, ResNet-34, the PSP stage, the concat and that GEMM run once on
 *   the 2B input views; up_1's tap combination then runs once per (sample, view half) on the same stacked rows with that block's mask
 *   rows, and up_2, the tail, the homographies, the cost volume and the heads run as they are on 2 S B views (choose, P and depths tiled
 *   on the device).  Same kernels as the plain forward: where the kernel selection of the shared part does not depend on the number of
 *   views (small batches choose other GEMM tiles than large ones; tuning key ws_min_rows pins them) the outputs equal the tiled forward's
 *   bit for bit, elsewhere to the rounding between those tiles.  S = 1 is the plain forward.
 *   Works with norm_mode 0 and 1, every storage type, option view2_heads 0 / 1 and the cost-volume chunking.  Refused with a message,
 *   before anything is launched: Dropout2d off with no masks loaded (the samples would be equal), masks loaded for another batch than
 *   S * B, option upconv without bits 0 and 1, the baseline network, S < 1, a workspace that is too small.  Eager on one stream (the
 *   one-stream rule of rgbm_adapose_set_dropout applies).  There is no hipGraph form, no feature-cache form and no dense / maps form.
 * rgbm_adapose_samples_workspace_bytes: the workspace of such a call (256-byte aligned): the plan for S * B poses behind a staging block
 *   for the tiled inputs. */
int rgbm_adapose_samples_workspace_bytes(rgbm_adapose_t* h, int B, int S, size_t* bytes);
int rgbm_adapose_forward_samples(rgbm_adapose_t* h, int B, int S, const float* img1, const float* img2, const int32_t* choose1,
                                 const int32_t* choose2, const float* P1, const float* P2, const float* depths, void* workspace,
                                 size_t workspace_bytes, const rgbm_adapose_out* out, void* stream);
/* Statistics over S samples per pose (sample_stats.hip; float64 numpy twins in rgbmanip_amd/samples.py).  Device pointers.
 * rgbm_sample_box_stats: boxes [S][n][8][3] fp64 (world-frame corners in get_3d_bbox's order, lib/utils.py:49-56), ok [S][n] uint8.
 *   A sample counts if its ok is set and all 24 of its coordinates are finite.  Per pose, over the counted samples in ascending s, in
 *   fp64 with two passes (mean, then deviations): count [n] int32; bbox_mean / bbox_std [n][8][3] (population std); center_mean [n][3]
 *   and center_cov [n][3][3] (centre = mean of the 8 corners); extent_mean / extent_std [n][3], the lengths of the three edges that
 *   leave corner 0, in the order x, y, z of the box frame (to corners 2, 4, 1); axis_spread_deg [n][3], per edge direction the RMS
 *   angle in degrees between each sample's unit edge vector and the normalised sum of the samples' unit vectors (acos of the dot
 *   product clamped to [-1, 1]).  count = 0: every statistic is NaN.  count = 1: the spreads are 0.  One workgroup per pose, no atomics.
 *   1 <= S <= 64 and 1 <= n <= 65535, refused otherwise.
 * rgbm_sample_point_stats: x [S][n][M] fp32 -> mean / std [n][M] fp32, per element over s ascending: accumulated in fp64, two passes,
 *   population std, rounded once to fp32; NaN propagates.  S, n, M >= 1. */
int rgbm_sample_box_stats(const double* boxes, const uint8_t* ok, int n, int S, int32_t* count, double* bbox_mean, double* bbox_std,
                          double* center_mean, double* center_cov, double* extent_mean, double* extent_std, double* axis_spread_deg,
                          void* stream);
int rgbm_sample_point_stats(const float* x, int n, int S, int64_t M, float* mean, float* std, void* stream);

/* Agreement of two oriented boxes (box_overlap.hip; float64 numpy twins in rgbmanip_amd/boxes.py).  Device pointers, fp64.
 * A box is [8][3] corners in get_3d_bbox's order (lib/utils.py:49-56), read as the parallelepiped o + a ex + b ey + c ez,
 *   0 <= a, b, c <= 1, o = corner 0, ex / ey / ez = corner 2 / 4 / 1 - corner 0 (the edges of rgbm_sample_box_stats); the other four
 *   corners enter the finiteness check, the centre (mean of the 8) and corner_dist only.  volume = |det[ex ey ez]|.  A box is unusable
 *   when one of its 24 coordinates is not finite, its volume is not > 0 or its ok byte is 0; ok_a / ok_b may be NULL (every box may
 *   count).  Every metric of a pair with an unusable box is NaN, its valid 0.  Coordinate range: edge lengths within 1e-60 .. 1e60
 *   (boxes are metres); the face normals go through products of four edge lengths, and where those overflow or vanish the results
 *   are not defined.
 * Intersection volume: exact for two parallelepipeds, 1/3 sum_f d_f area(P_f) over the 12 faces with P_f the face clipped by the other
 *   box's half-spaces, in coordinates relative to the centre of box A, summed in face order (A's, then B's; no atomics: two calls give
 *   the same bytes).  Coincident planes, tau = 1e-12, L the longer of |ex + ey + ez|: a plane of B with n_A . n_B >= 1 - tau and
 *   |d_A - d_B| <= tau L against a plane of A is dropped, one with n_A . n_B <= -(1 - tau) and |d_A + d_B| <= tau L makes the volume 0.
 *   inter = clamp(sum, 0, min(volume_a, volume_b)), iou = inter / (volume_a + volume_b - inter).
 * rgbm_box_agreement: a, b [n][8][3], ok_a, ok_b [n] uint8 -> for pair i = (a[i], b[i]): valid [n] int32, iou, inter_volume, volume_a,
 *   volume_b [n]; center_dist [n] and center_delta [n][3] (b - a); corner_dist [n], the mean over the 8 corners of |a_k - b_k|;
 *   extent_a, extent_b [n][3], the edge lengths x, y, z; axis_angle_deg [n][3] = acos(clamp(u_a . u_b)) of the unit edges, 0..180;
 *   axis_fold_deg [n][3] = min(angle, 180 - angle); rot_deg [n] = acos(clamp((sum_e u_a[e] . u_b[e] - 1) / 2)).
 *   1 <= n <= 2^24, refused otherwise; every output pointer is required.
 * rgbm_box_iou_matrix: a [n][P][8][3], b [n][Q][8][3], ok_a [n][P], ok_b [n][Q] -> iou [n][P][Q], NaN where either box is unusable.
 *   1 <= P, Q <= 64 and n >= 1, n P Q <= 2^31 - 1, refused otherwise.  A refused call launches nothing and writes nothing. */
int rgbm_box_agreement(const double* a, const double* b, const uint8_t* ok_a, const uint8_t* ok_b, int n, int32_t* valid, double* iou,
                       double* inter_volume, double* volume_a, double* volume_b, double* center_dist, double* center_delta,
                       double* corner_dist, double* extent_a, double* extent_b, double* axis_angle_deg, double* axis_fold_deg,
                       double* rot_deg, void* stream);
int rgbm_box_iou_matrix(const double* a, const double* b, const uint8_t* ok_a, const uint8_t* ok_b, int n, int P, int Q, double* iou,
                        void* stream);

/* Box verification without ground truth (box_verify.hip; float64 numpy twins in rgbmanip_amd/verify.py, which evaluate the same
 * expressions in the same order: every output is an integer and kernel and twin are equal).  Device pointers; the box model is the one
 * above (o = corner 0, e_0 / e_1 / e_2 = corner 2 / 4 / 1 - o).
 * rgbm_box_silhouette: boxes [n][S][8][3] fp64 world frame, ok [n][S] uint8 or NULL, K [n][V][3][3] fp64 (the original intrinsics;
 *   only K00, K11, K02, K12 are read), E [n][V][4][4] fp64 world -> camera (X_cam = E X_world), mask [n][V][H][W] uint8 (any non-zero
 *   byte is foreground).  For box s of pose i in view v: camera-frame corners c_k = ((E_r0 x + E_r1 y) + E_r2 z) + E_r3; o = c_0,
 *   e_0, e_1, e_2 = c_2 - o, c_4 - o, c_1 - o; n_k = e_{k+1} x e_{k+2}; det = e_0 . n_0; lo = min(0, det), hi = max(0, det).  Pixel
 *   (v, u) has xn = (u - K02) / K00, yn = (v - K12) / K11 (the integer pixel coordinate, no half-pixel offset).  Slab k: q0 = -(n_k . o),
 *   dq = (n_k.x xn + n_k.y yn) + n_k.z; dq != 0: t1 = (lo - q0) / dq, t2 = (hi - q0) / dq, tn = min, tf = max; otherwise tn = -inf if
 *   lo <= q0 <= hi, else +inf, and tf = +inf.  tmin = max_k tn, tmax = min_k tf; the pixel is inside the silhouette iff tmax >= tmin
 *   and tmin > 0 (the hit rule of rgbm_synth_render: a box that contains the camera has an empty silhouette and is flagged).  A box is
 *   usable when its 24 coordinates, the first three rows of E and K00, K11, K02, K12 are finite, K00 and K11 are not 0, |det| > 0 and
 *   its ok byte is not 0.  Outputs, all int32: area_box [n][S][V] silhouette pixels inside the frame; inter [n][S][V] those with a
 *   non-zero mask byte; area_mask [n][V] non-zero mask bytes; rect [n][S][V][4] row min, col min, row max, col max of the silhouette,
 *   (H, W, -1, -1) when it is empty; flags [n][S][V]: bit 1 usable, bit 2 the camera is inside the box (lo <= q0_k <= hi for all k),
 *   bit 4 the silhouette touches the frame border, bit 8 some c_k has z <= 0.  An unusable box has zero counts, the empty rect and
 *   flags 0.  The mask of a (pose, view) is read once whatever S is; integer atomics only, so two calls give the same bytes.
 *   1 <= S <= 64, 1 <= V <= 16, n >= 1, n S V <= 2^24, H W < 2^31, refused otherwise; scratch: rgbm_box_silhouette_scratch_bytes
 *   bytes, 8-byte aligned (one record and one pixel bound per pose, view and box).
 * rgbm_cloud_in_box: cloud [n][cap][3] fp32 and count [n][count_cols] int32 as rgbm_cloud_pack (count_cols = 2) or
 *   rgbm_cloud_pack_views (count_cols = V, or a folded count with 1) write them: the first total = min(sum_c max(count_c, 0), cap) rows
 *   of a pose hold its points.  boxes [n][S][8][3] fp64 world frame, ok [n][S] or NULL, inflate >= 0.  With the world-frame o, n_k, det,
 *   lo, hi of a box and p a row converted to fp64: a_k = n_k . (p - o) = (n_k.x d_x + n_k.y d_y) + n_k.z d_z; p is inside iff
 *   lo - inflate |det| <= a_k <= hi + inflate |det| for k = 0, 1, 2 (the box grown by inflate edge lengths on every side); a row that
 *   is not finite is never inside.  inside [n][S] int32 (0 for an unusable box: a non-finite coordinate, |det| not > 0, ok 0),
 *   total [n] int32.  The cloud is read once per pose for all S boxes.  1 <= S <= 64, n >= 1, n S <= 2^24, 1 <= count_cols <= 16,
 *   0 <= cap <= 2^30, refused otherwise.  A refused call launches nothing and writes nothing. */
int rgbm_box_silhouette_scratch_bytes(int n, int S, int V, size_t* bytes);
int rgbm_box_silhouette(const double* boxes, const uint8_t* ok, const double* K, const double* E, const uint8_t* mask, int n, int S, int V,
                        int H, int W, int32_t* area_box, int32_t* inter, int32_t* area_mask, int32_t* rect, int32_t* flags, void* scratch,
                        size_t scratch_bytes, void* stream);
int rgbm_cloud_in_box(const float* cloud, const int32_t* count, int count_cols, const double* boxes, const uint8_t* ok, int n, int S, int cap,
                      double inflate, int32_t* inside, int32_t* total, void* stream);

/* Dense depth and confidence maps of the crops (what lib/network_v3.py:406-408 returns as view1_depth: softmax over the D planes of the
 * regularised cost volume, then the expectation with the depth values), beside the ten point outputs.
 * rgbm_adapose_forward_dense: the arguments of rgbm_adapose_forward plus two caller-owned fp32 device buffers [V'][224][224],
 *   V' = 2B (rows: the view-1 crops, then the view-2 crops) or, with option view2_heads = 0, B (view-1 maps only; the cost volume of the
 *   view-2 crops is not built, as in rgbm_adapose_forward).  depth_map[v][y][x] = sum_d p[d] depths[v % B][d], conf_map[v][y][x] =
 *   max_d p[d], p = softmax_d of the prob conv (Conv3d 8 -> 1, 3^3, zero padding, network_v5.py:280,290) evaluated at every pixel; fp32
 *   sums in the order of the point head, so depth_map read at choose1[b][p] is view1_depth[b][p].  conf_map may be NULL, depth_map not.
 *   For this one call the network runs with a dense cost regularisation and the dense tail — the effect of options sparse_dec = 0 and
 *   sparse_tail = 0 — without changing the handle's options: the ten outputs in `out` are bit for bit those of a handle built with
 *   these two options, and can differ from the default sparse-tail outputs by the rounding between the two tails (16-bit and split-pair
 *   storage; the bound of tests/test_gpu_adapose.py::test_prob_sparse_kernels_agree).  Works with Dropout2d on (the masks are drawn
 *   upstream of the cost volume).  There is no hipGraph and no feature-cache form of this call.
 * rgbm_adapose_dense_workspace_bytes: the workspace of such a call (256-byte aligned, as for rgbm_adapose_forward).  The workspace plan
 *   holds conv11's output whatever the options and the call say, so this is rgbm_adapose_workspace_bytes(B); the query reads the handle only.
 * rgbm_depth_to_points: depth_map [n][S][S] fp32, Kcrop [n][3][3] fp64 (cropped intrinsics), E [n][4][4] fp64 (world -> camera) ->
 *   points [n][S][S][3] fp32 in the world frame: inv(E) (depth Kcrop^-1 (x, y, 1)^T), the per-pixel form of the back-projection of
 *   interface_v5.py:329-336 followed by ex_inv of :369-372 (fp64 arithmetic, rounded once).  A pixel whose depth is not finite yields
 *   NaN; nothing is clamped.  n <= 65535. */
int rgbm_adapose_dense_workspace_bytes(rgbm_adapose_t* h, int B, size_t* bytes);
int rgbm_adapose_forward_dense(rgbm_adapose_t* h, int B, const float* img1, const float* img2, const int32_t* choose1,
                               const int32_t* choose2, const float* P1, const float* P2, const float* depths, void* workspace,
                               size_t workspace_bytes, const rgbm_adapose_out* out, float* depth_map, float* conf_map, void* stream);
int rgbm_depth_to_points(const float* depth_map, const double* Kcrop, const double* E, int n, int S, float* points, void* stream);

/* Two-view geometric consistency of dense depth maps, and the packed point cloud of the pixels that pass it.
 * rgbm_depth_consistency: depth_a / depth_b [n][S][S] fp32 (camera z of the crops of views a and b), Kcrop_* [n][3][3] fp64 (fx, fy, cx,
 *   cy are read), E_* [n][4][4] fp64 (world -> camera); conf_a [n][S][S] fp32 and mask_a [n][S][S] uint8 may be NULL.  Per pixel (x, y)
 *   of view a with depth d, in fp64, rounded once into the fp32 results:
 *     1. d not finite or <= 0, or an E without a finite inverse: keep 0, fused / reproj / rel NaN;
 *     2. X = inv(E_a) (d Kcrop_a^-1 (x, y, 1)^T), (u, v, z) its projection through Kcrop_b E_b[:3]; z <= 0 or u, v outside
 *        [0, S - 1]: as 1;
 *     3. depth_b sampled bilinearly at (u, v) (taps floor(u) and min(floor(u) + 1, S - 1), v alike); a tap that is not finite or <= 0:
 *        as 1;
 *     4. (u, v) at the sampled depth back-projected through view b and projected into view a: (x', y', d'); reproj = hypot(x' - x,
 *        y' - y) in pixels, rel = |d' - d| / d — written whatever step 5 decides (diagnostic maps; reproj and rel may be NULL);
 *     5. keep = reproj < px_max && rel < rel_max && (conf_a == NULL || conf >= conf_min) && (mask_a == NULL || mask != 0);
 *        fused = keep ? (d + d') / 2 : NaN.
 *   px_max, rel_max, conf_min: finite and >= 0.  n <= 65535, S <= 4096.
 * rgbm_cloud_pack: ordered compaction.  For pose i the pixels of view 1 with keep1 != 0 in row-major order, then those of view 2, each
 *   back-projected to the world frame with the arithmetic of rgbm_depth_to_points (same bits): cloud [n][cap][3] fp32, index [n][cap]
 *   int32 = view * S * S + pixel (view 0 or 1), count [n][2] int32 = the pixels kept per view — the full counts even when their sum
 *   exceeds cap.  Only the first cap rows are written; rows min(cap, total) .. cap - 1 hold NaN / -1.  fused2, keep2, Kcrop2 and E2 may
 *   be NULL together (a one-view cloud).  The order does not depend on scheduling (no atomics); cap >= 0. */
int rgbm_depth_consistency(const float* depth_a, const float* conf_a, const uint8_t* mask_a, const double* Kcrop_a, const double* E_a,
                           const float* depth_b, const double* Kcrop_b, const double* E_b, int n, int S, double px_max, double rel_max,
                           float conf_min, float* fused, float* reproj, float* rel, uint8_t* keep, void* stream);
int rgbm_cloud_pack(const float* fused1, const uint8_t* keep1, const double* Kcrop1, const double* E1, const float* fused2,
                    const uint8_t* keep2, const double* Kcrop2, const double* E2, int n, int S, int cap, float* cloud, int32_t* index,
                    int32_t* count, void* stream);

/* Dense NOCS maps, and a box fitted to the two-view cloud.
 * rgbm_adapose_forward_maps: the arguments of rgbm_adapose_forward_dense plus nocs_map [V'][224][224][3] fp32 (V' as for depth_map): the
 *   network's per-pixel NOCS branch (gather -> instance_color -> nocs_head -> tanh, network_v5.py:432-438) evaluated at every pixel of
 *   the feature map with the arithmetic of the point branch, so nocs_map read at choose1[b][p] is view1_nocs[b][p] bit for bit.
 *   depth_map != NULL: rgbm_adapose_forward_dense plus the NOCS map (nocs_map may then be NULL).  depth_map == NULL (conf_map must be NULL
 *   too): the plain rgbm_adapose_forward plus the NOCS map — the handle's sparse_dec / sparse_tail stay in force, the workspace is that of
 *   rgbm_adapose_workspace_bytes, the ten outputs are bit for bit those of rgbm_adapose_forward.  All three NULL: an argument error.
 *   There is no hipGraph and no feature-cache form of this call.
 * rgbm_nocs_map: the kernel alone, with the handle's weights, on a plain fp32 feature array feat_f32 [V][HW][32] -> nocs_map [V][HW][3];
 *   V * HW must be a multiple of 64.  A NaN feature gives NaN in its own pixel and nowhere else.
 * rgbm_cloud_gather: rows of per-pixel maps at a packed cloud's indices.  map1 / map2 [n][S2][C] fp32 (map2 may be NULL), index [n][cap]
 *   int32 as rgbm_cloud_pack writes it -> out [n][cap][C] fp32, out[i][r] = map{1 + index / S2}[i][index % S2].  Rows with index < 0,
 *   index >= 2 S2, or index >= S2 while map2 == NULL hold NaN.  1 <= C <= 4, cap >= 0.
 * rgbm_cloud_similarity: the reference's similarity RANSAC (lib/align.py:10-104) between the cloud's object-space rows nocs [n][cap][3]
 *   and its world-frame rows cloud [n][cap][3] (both fp32, arithmetic in fp64), count [n][2] as rgbm_cloud_pack writes it.  For pose b
 *   with m = min(cap, count[b][0] + count[b][1]), over rows 0 .. m - 1:
 *     1. m < 5, or a NaN among the m rows of either array: invalid;
 *     2. threshold 2 max ||s - mean s|| / 10; 128 five-point Umeyama hypotheses, sample k of hypothesis i = mix32(seed, 128 b + i, k) mod m
 *        (the hash of rgbm_adapose_postprocess_ransac); inlier counts of every hypothesis over all m rows against scale * threshold; the
 *        reference's sequential scan over the counts (a strictly better ratio wins, confidence break, best ratio < 0.1: no consensus);
 *        Umeyama over the kept hypothesis's inliers;
 *     3. the box: half = max |nocs| over the m rows per axis, size = 2 half scale, get_3d_bbox corners through [R | t] rounded to float32
 *        (interface_v5.py:348-367); no world transform, the cloud is in the world frame already.
 *   bbox [n][8][3] fp64, srt [n][13] fp64 (scale, R row-major, t), valid [n] int32, info [n][4] int32 = (m, the kept hypothesis or -1,
 *   its inlier count, the hypotheses the scan examined; -1, 0, 0 behind m for an invalid pose).  Invalid, no-consensus and non-finite
 *   poses: valid 0, the +10 default_bbox, srt[0] NaN.  A pose's rows are cut into slices of whole workgroups whose integer counts and fp64
 *   partial sums are combined in slice order (no floating-point atomics): results are bit-identical from run to run.
 *   scratch: rgbm_cloud_similarity_scratch_bytes(n, cap) bytes of device memory, 8-byte aligned, contents irrelevant.  cap >= 1,
 *   n <= 65535. */
int rgbm_adapose_forward_maps(rgbm_adapose_t* h, int B, const float* img1, const float* img2, const int32_t* choose1,
                              const int32_t* choose2, const float* P1, const float* P2, const float* depths, void* workspace,
                              size_t workspace_bytes, const rgbm_adapose_out* out, float* depth_map, float* conf_map, float* nocs_map,
                              void* stream);
int rgbm_nocs_map(rgbm_adapose_t* h, const float* feat_f32, int V, int HW, float* nocs_map, void* stream);
int rgbm_cloud_gather(const float* map1, const float* map2, const int32_t* index, int n, int S2, int C, int cap, float* out, void* stream);
int rgbm_cloud_similarity_scratch_bytes(int n, int cap, size_t* bytes);
int rgbm_cloud_similarity(const float* nocs, const float* cloud, const int32_t* count, int n, int cap, uint32_t seed, double* bbox, double* srt,
                          int32_t* info, int32_t* valid, void* scratch, size_t scratch_bytes, void* stream);

/* Multi-view depth fusion: the consistency check over V views of a pose, and the cloud of all of them.
 * rgbm_depth_fusion: depth [n][V][S][S] fp32 (camera z of the V crops of pose i), conf [n][V][S][S] fp32 and mask [n][V][S][S] uint8 (may
 *   be NULL), Kcrop [n][V][3][3] fp64, E [n][V][4][4] fp64 (world -> camera).  Per pixel (x, y) of view a with depth d, in fp64, rounded
 *   once:
 *     0. d not finite or <= 0, or E_a without a finite inverse: keep 0, fused NaN, nviews 0, agree 0;
 *     1. the sources b = 0 .. V - 1, b != a, in increasing order: a source whose E_b has no finite inverse does not agree; otherwise rules
 *        2-4 of rgbm_depth_consistency (same taps, same clamp of the second tap, same NaN / <= 0 tap rule) give (x', y', d'_b), and b
 *        agrees iff hypot(x' - x, y' - y) < px_max && |d'_b - d| / d < rel_max;
 *     2. c = the number of agreeing sources: nviews = c, agree = the bit set of the agreeing b — written whatever 3 decides (agree may
 *        be NULL);
 *     3. keep = c >= n_min && (conf == NULL || conf >= conf_min) && (mask == NULL || mask != 0);
 *        fused = keep ? (d + sum of d'_b over the agreeing b, added in increasing b) / (1 + c) : NaN.
 *   2 <= V <= 16, 1 <= n_min <= V - 1, n >= 1, n V <= 65535, S <= 4096; px_max, rel_max, conf_min finite and >= 0.  No atomics: results
 *   are bit-identical from run to run.  At V = 2, n_min = 1, fused and keep of view 0 are the bits rgbm_depth_consistency(a = view 0, b =
 *   view 1) writes, and those of view 1 the bits of the opposite direction.
 * rgbm_cloud_pack_views: rgbm_cloud_pack's ordered compaction over V views.  fused [n][V][S][S] fp32, keep [n][V][S][S] uint8, Kcrop
 *   [n][V][3][3], E [n][V][4][4] -> for pose i the kept pixels of view 0 in row-major order, then view 1's, ...: cloud [n][cap][3] fp32
 *   (the back-projection of rgbm_depth_to_points, same bits), index [n][cap] int32 = view * S * S + pixel, count [n][V] int32 = the
 *   pixels kept per view, whatever cap is.  Rows min(cap, total) .. cap - 1 hold NaN / -1.  1 <= V <= 16, n <= 65535, S <= 4096, cap >=
 *   0; no atomics.  At V = 2 the three outputs are byte for byte those of rgbm_cloud_pack, at V = 1 those of its one-view form.
 * rgbm_cloud_gather_views: maps [n][V][S2][C] fp32, index [n][cap] int32 as rgbm_cloud_pack_views writes it -> out [n][cap][C] fp32,
 *   out[i][r] = maps[i][index / S2][index % S2].  Rows with an index outside [0, V S2) hold NaN.  1 <= V <= 16, 1 <= C <= 4, cap >= 0. */
int rgbm_depth_fusion(const float* depth, const float* conf, const uint8_t* mask, const double* Kcrop, const double* E, int n, int V, int S,
                      double px_max, double rel_max, float conf_min, int n_min, float* fused, uint8_t* keep, uint8_t* nviews, uint16_t* agree,
                      void* stream);
int rgbm_cloud_pack_views(const float* fused, const uint8_t* keep, const double* Kcrop, const double* E, int n, int V, int S, int cap,
                          float* cloud, int32_t* index, int32_t* count, void* stream);
int rgbm_cloud_gather_views(const float* maps, const int32_t* index, int n, int V, int S2, int C, int cap, float* out, void* stream);

/* Post-processing of one batch of network outputs into world-frame handle boxes.
 * Replaces: compute_scale_and_translation / get_3d_bbox / transform_coordinates_3d and the tail of predict()
 *   models/pose_estimator/AdaPose/lib/utils.py:40-119, models/pose_estimator/AdaPose/interface_v5.py:318-321,354-374
 * nocs1 [B,P,3] f32, depth1 [B,P] f32, r1 [B,3,3] f32, choose1 [B,P] i32, Kcrop [B,3,3] f64 (cropped intrinsics),
 * E1 [B,4,4] f64 (world->camera of view 1)  ->  bbox_world [B,8,3] f64, ts [B,4] f64 (t xyz, scale), valid [B] i32
 * (0 where the reference would return default_bbox (+10 cube), which is what bbox_world then holds). */
int rgbm_adapose_postprocess(int B, int P, int img_size, const float* nocs1, const float* depth1, const float* r1,
                             const int32_t* choose1, const double* Kcrop, const double* E1, double* bbox_world, double* ts,
                             int32_t* valid, void* stream);
/* The same post-processing with caller-provided device scratch (rgbm_adapose_postprocess_scratch_bytes(B) bytes, 8-byte aligned,
 * contents irrelevant; 0 bytes = not needed at this batch size): small batches cut the three passes over the 523 776 point pairs of
 * the exact-median search into up to 32 slices per pose (one workgroup each) instead of running one workgroup per pose — 1.1 ms of
 * a 2.9 ms B = 1 call otherwise.  Results are bit-identical to rgbm_adapose_postprocess. */
int rgbm_adapose_postprocess_scratch_bytes(int B, size_t* bytes);
int rgbm_adapose_postprocess_ws(int B, int P, int img_size, const float* nocs1, const float* depth1, const float* r1,
                                const int32_t* choose1, const double* Kcrop, const double* E1, double* bbox_world, double* ts,
                                int32_t* valid, void* scratch, size_t scratch_bytes, void* stream);

/* The `direct_regression: True` tail of AdaPoseEstimator_v4.predict (interface_v4.py:322-325, 358-378): translation t1 and scale
 * ||s1|| come from the network's own heads, so no pair median is searched.  half = max |nocs1| over the P points per axis, size = 2 half
 * scale, get_3d_bbox corners, sRT = [r1 | t1] (r1 is not multiplied by the scale), world frame through inv(E1); the reference's dtypes:
 * scale, size and the camera-frame box in float32, the world transform in float64.
 * nocs1 [B,P,3] f32, r1 [B,3,3] f32, t1 [B,3] f32, s1 [B,3] f32, E1 [B,4,4] f64 (device) -> bbox_world [B,8,3] f64, ts [B,4] f64
 * (t xyz, scale), valid [B] i32 (0 and the +10 default_bbox wherever the box or inv(E1) is non-finite; a NaN stays in its pose).
 * Any B >= 1 and 1 <= P <= 1024; one launch of one workgroup per pose, no scratch. */
int rgbm_adapose_postprocess_regressed(int B, int P, const float* nocs1, const float* r1, const float* t1, const float* s1,
                                       const double* E1, double* bbox_world, double* ts, int32_t* valid, void* stream);

/* The `direct_regression: False`, `use_depth: True` tail of predict: back-projected predicted depth vs
 * predicted NOCS, 128-hypothesis Umeyama RANSAC, final fit over the inliers, bbox to the world frame.
 * Replaces: interface_v5.py:322-339, 348-374; lib/align.py:10-104 (estimateSimilarityUmeyama / estimateSimilarityTransform)
 * nocs1 [B,P,3] f32, depth1 [B,P] f32, choose1 [B,P] i32, Kcrop [B,3,3] f64, E1 [B,4,4] f64 (device) ->
 * bbox_world [B,8,3] f64, srt [B,13] f64 (scale, R row-major, t; scale NaN where the reference returns None), valid [B].
 * 5 <= P <= 1024.  The 5-point samples are a seeded hash (mix32(seed, 128 b + i, k) mod P) instead of np.random.randint.
 * The third branch (`use_depth: False`, cv2.solvePnPRansac) is not provided. */
int rgbm_adapose_postprocess_ransac(int B, int P, int img_size, uint32_t seed, const float* nocs1, const float* depth1,
                                    const int32_t* choose1, const double* Kcrop, const double* E1, double* bbox_world, double* srt,
                                    int32_t* valid, void* stream);
/* Tail of AdaPoseEstimator_v5.predict for `direct_regression: False`, `use_depth: False` (interface_v5.py:340-346, lib/utils.py:121-195,
 * lib/align.py:104-115): mutual NOCS matches of the two views -> epipolar gate -> DLT triangulation -> scale (median of pair ratios)
 * -> EPnP-RANSAC (100 five-point hypotheses, reprojection error 3 px) on (nocs1 * scale, pixels of view 1) -> EPnP over the inliers
 * -> VVS refinement over all points -> bbox in the world frame.  The OpenCV routines the reference calls are restated from their
 * published algorithms; RANSAC subsets come from a seeded hash (pose b, iteration i, draw k: mix32(seed, 128 b + i, k) mod P, first
 * five distinct).  nocs [B,P,3] f32; pts2d [B,P,2] f32 pixel coordinates in the ORIGINAL frame (prepare_model_input's view_pts2d);
 * K [B,3,3] f64 original intrinsics; E1 / E2 [B,4,4] f64 world -> camera.  bbox_out [B,8,3] f64 (default bbox when no match / no
 * consensus / non-finite); srt_out [B,13] f64 = scale, R (9), t (3); info_out [B,4] i32 = matches, RANSAC ok, inliers, hypotheses
 * examined; valid_out [B] i32. */
int rgbm_adapose_postprocess_pnp(int B, int P, uint32_t seed, const float* nocs1, const float* pts2d1, const float* nocs2,
                                 const float* pts2d2, const double* K, const double* E1, const double* E2, double* bbox_out,
                                 double* srt_out, int32_t* info_out, int32_t* valid_out, void* stream);
/* Tail of AdaPoseEstimator_realworld.predict (interface_realworld.py:295-320): scale = ||s1|| in float32, as np.linalg.norm of the float32
 * size vector the network regressed (s1 [B,3] f32), then the steps of rgbm_adapose_postprocess_pnp from EPnP-RANSAC on - the same device
 * functions, the same hash stream, 5 <= P <= 1024 - on (nocs1 * scale, pixels of view 1): no NOCS matching, no triangulation.  The box is
 * get_3d_bbox(2 max|nocs1| scale), a float32 product as in the reference, under [R | t], taken to the world frame through inv(E1).
 * srt_out as above (scale as a double); info_out [B,4] i32 = P, RANSAC ok, inliers, hypotheses examined.  No consensus or a non-finite
 * result gives the default box and valid = 0: the reference has no `success` check on this path and would use whatever cv2 left in r, t.
 * Parity of the restated OpenCV routines with cv2 is unpinned, as for the tail above. */
int rgbm_adapose_postprocess_pnp_scaled(int B, int P, uint32_t seed, const float* nocs1, const float* pts2d1, const float* s1,
                                        const double* K, const double* E1, double* bbox_out, double* srt_out, int32_t* info_out,
                                        int32_t* valid_out, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Batched device-side input preparation.
 * Replaces: AdaPoseEstimator_v5.prepare_model_input   models/pose_estimator/AdaPose/interface_v5.py:58-170
 *           get_bbox                                  models/pose_estimator/AdaPose/lib/utils.py:10-38
 * rgb [N,H,W,3] f32 in [0,1] (the env's camera frames), mask [N,H,W] u8 (0/1), K [N,3,3] f64 camera intrinsics  ->
 * img [N,3,S,S] f32 (cropped, INTER_LINEAR-resized, ImageNet-normalised), choose [N,P] i32 (pixel indices of the
 * INTER_NEAREST-resized mask: every nonzero pixel in order, wrap-padded to P, or an ordered random P-subset),
 * pts2d [N,P,2] f32 (optional, may be NULL), Kcrop [N,3,3] f64 (crop-adjusted intrinsics), window [N,4] i32
 * (rmin,rmax,cmin,cmax), valid [N] i32 (0 where the reference returns None: empty mask / empty resized mask; such
 * frames get finite dummy outputs).  scratch: N*S*S bytes.  The P-subset is drawn by a seeded hash instead of the
 * reference's global np.random.shuffle (same distribution, reproducible).  H, W >= 440 (the reference's crop window is up to 440 pixels wide, interface_v5.py:63-88); S*S <= 65536.
 * ---------------------------------------------------------------------------------------------------------- */
int rgbm_prepare_inputs(const float* rgb_dev, const uint8_t* mask_dev, const double* K_dev, int N, int H, int W, int S, int P,
                        uint32_t seed, float* img_out, int32_t* choose_out, float* pts2d_out, double* Kcrop_out,
                        int32_t* window_out, int32_t* valid_out, uint8_t* scratch, void* stream);

/* The same, reading frame f's image and mask from entry frame_map[f] of rgb_dev / mask_dev (e.g. the controller's view
 * queue [T*N,H,W,...]) instead of gathering the selected views first; frame_map[f] < 0 = no such view
 * (treated as an empty mask: valid 0).  K_dev, every output and the subset hash stay indexed by f. */
int rgbm_prepare_inputs_indexed(const float* rgb_dev, const uint8_t* mask_dev, const double* K_dev, const int32_t* frame_map_dev,
                                int N, int H, int W, int S, int P, uint32_t seed, float* img_out, int32_t* choose_out,
                                float* pts2d_out, double* Kcrop_out, int32_t* window_out, int32_t* valid_out, uint8_t* scratch,
                                void* stream);
/* Both of the above with a hash offset: frame f of this call draws its 1024-subset as frame frame0 + f would in one call over the
 * whole batch, so a batch prepared in pieces (estimate() uploads and prepares host frames chunk by chunk while the previous chunk
 * computes) chooses the same pixels as the unchunked call.  frame_map_dev may be null (frames in order). */
int rgbm_prepare_inputs_ex(const float* rgb_dev, const uint8_t* mask_dev, const double* K_dev, const int32_t* frame_map_dev,
                           int frame0, int N, int H, int W, int S, int P, uint32_t seed, float* img_out, int32_t* choose_out,
                           float* pts2d_out, double* Kcrop_out, int32_t* window_out, int32_t* valid_out, uint8_t* scratch,
                           void* stream);
/* rgbm_prepare_inputs_ex on 8-bit frames: rgb_dev [M,H,W,3] u8, a camera's bytes as they are (no float32 copy of the frames).
 * Byte b means the float32 value fl32(b / 255), correctly rounded — numpy's float32(b) / float32(255); each tap is converted as
 * (float)((double)b / 255.0), which equals it for all 256 values (b * (1 / 255.f) is one ulp off for 126 of them), and everything
 * after the tap load is the float path's arithmetic.  Every output is therefore bit-identical to rgbm_prepare_inputs_ex on float32
 * frames holding fl32(b / 255).  Same arguments, shape limits and error codes; frame_map_dev may be null, frame0 >= 0. */
int rgbm_prepare_inputs_u8(const uint8_t* rgb_dev, const uint8_t* mask_dev, const double* K_dev, const int32_t* frame_map_dev,
                           int frame0, int N, int H, int W, int S, int P, uint32_t seed, float* img_out, int32_t* choose_out,
                           float* pts2d_out, double* Kcrop_out, int32_t* window_out, int32_t* valid_out, uint8_t* scratch,
                           void* stream);
/* rgbm_prepare_inputs_ex / rgbm_prepare_inputs_u8 behind one entry point, with the image transform as a switch.
 * pixel_type 0: rgb_dev is [M,H,W,3] f32, 1: [M,H,W,3] u8 (byte b = fl32(b / 255), as above).
 * normalize 1: ToTensor + ImageNet Normalize - exactly rgbm_prepare_inputs_ex (pixel_type 0) / rgbm_prepare_inputs_u8 (pixel_type 1), bit
 *   for bit.  normalize 0: plain ToTensor, img_out holds the bilinear-resized crop itself - what AdaPoseEstimator_v4 feeds its network
 *   for every task but "pots" (interface_v4.py:52-58).  The switch is a compile-time parameter of the crop kernel; window, mask resize,
 *   choose, pts2d, Kcrop, valid, the subset hash, shape limits and error codes do not depend on it.
 * A pixel_type or normalize outside {0, 1} is an argument error: nothing is launched. */
int rgbm_prepare_inputs_opt(const void* rgb_dev, int pixel_type, int normalize, const uint8_t* mask_dev, const double* K_dev,
                            const int32_t* frame_map_dev, int frame0, int N, int H, int W, int S, int P, uint32_t seed, float* img_out,
                            int32_t* choose_out, float* pts2d_out, double* Kcrop_out, int32_t* window_out, int32_t* valid_out,
                            uint8_t* scratch, void* stream);
/* rgbm_prepare_inputs_opt with the points drawn as AdaPoseEstimator_v2.prepare_model_input draws them (interface_v2.py:74-98, "sample, then
 * resize"): the candidates are the non-zero pixels of mask[rmin:rmax, cmin:cmax] at the frame's own resolution, in row-major order, index
 * i = row * crop_w + col with crop_w = rmax - rmin (up to 440 x 440 = 193 600 of them).  The subset rule is unchanged on that index: more
 * than P candidates -> the P smallest (mix32(seed, frame0 + f, i), i) in index order; 1 .. P -> wrap padding; none, or an invalid frame ->
 * zeros and valid = 0.  pts2d_out (may be NULL) = (cmin + col, rmin + row), whole pixels of the frame as float32; choose_out =
 * floor(row * ratio) * S + floor(col * ratio), ratio = S / crop_w in fp64, so indices repeat when crop_w > S.  img_out, Kcrop_out and
 * window_out are rgbm_prepare_inputs_opt's, same arguments, same scratch.  One workgroup per frame; the window's mask is staged as a bit
 * mask in LDS.  P <= 8192. */
int rgbm_prepare_inputs_native(const void* rgb_dev, int pixel_type, int normalize, const uint8_t* mask_dev, const double* K_dev,
                               const int32_t* frame_map_dev, int frame0, int N, int H, int W, int S, int P, uint32_t seed, float* img_out,
                               int32_t* choose_out, float* pts2d_out, double* Kcrop_out, int32_t* window_out, int32_t* valid_out,
                               uint8_t* scratch, void* stream);
/* rgbm_prepare_inputs_opt from crop windows the HOST has cut out of the frames (estimate() with cfg hip_upload: "windows"): only the
 * pixels the crop kernel reads cross PCIe.  The caller derives frame f's window (rmin, rmax, cmin, cmax) = window_dev[f] from the mask
 * with get_bbox's integer arithmetic (lib/utils.py:10-38 with H x W for 480 x 640; an empty mask: (0, 40, 0, 40) and valid_in_dev[f] = 0)
 * and packs, with h = rmax - rmin and w = cmax - cmin:
 *   pix_dev       the h*w*3 pixels of rows rmin..rmax-1 x columns cmin..cmax-1, row-major, at ELEMENT offset 3 * offset_dev[f];
 *                 pixel_type 0: f32 elements, 1: u8 elements (byte b = fl32(b / 255), exactly as in rgbm_prepare_inputs_u8)
 *   mask_pix_dev  the h*w mask bytes of the same window (non-zero = object) at mask_pix_dev + offset_dev[f]
 *   offset_dev    [N] i64, the exclusive prefix sum of h*w over the frames of the call;  window_dev [N][4] i32;  valid_in_dev [N] i32
 * H, W: the size of the frames the windows were cut from (Kcrop and pts2d are in frame coordinates; H, W >= 440 as above).
 * img_out, choose_out, pts2d_out (may be NULL), Kcrop_out and valid_out are bit-identical to what rgbm_prepare_inputs_opt writes from the
 * whole frames with the same pixel_type, normalize, frame0, seed, S and P (frame_map_dev NULL), whose window_out equals window_dev: the
 * crop kernel runs the same interpolation body on the packed pixels, Kcrop comes from the same fp64 expressions, the choose stage is
 * the same kernel.  That includes an empty mask (valid_in 0): pack the frame's 40 x 40 corner; Kcrop is the identity, valid_out 0.
 * The windows are trusted: every tap is read at offset_dev[f] + y * w + x with y < h, x < w, so the packed buffers must hold
 * offset_dev[N-1] + h*w pixels.  scratch: N*S*S bytes.  Argument errors (nothing is launched): pixel_type or normalize outside {0, 1},
 * a null pointer other than pts2d_out, frame0 < 0 and the shape limits of rgbm_prepare_inputs. */
int rgbm_prepare_inputs_windows(const void* pix_dev, int pixel_type, int normalize, const uint8_t* mask_pix_dev, const int64_t* offset_dev,
                                const int32_t* window_dev, const int32_t* valid_in_dev, const double* K_dev, int frame0, int N, int H, int W,
                                int S, int P, uint32_t seed, float* img_out, int32_t* choose_out, float* pts2d_out, double* Kcrop_out,
                                int32_t* valid_out, uint8_t* scratch, void* stream);
/* Float frames -> 8-bit frames, the write side of a byte view queue whose environment hands over float frames:
 * dst[i] = (uint8) min(max(rintf(src[i] * 255.f), 0), 255), rint = round half to even, NaN -> 0 (+inf -> 255, -inf -> 0).
 * rintf(fl32(b / 255) * 255.f) == b for every byte b, so quantise -> rgbm_prepare_inputs_u8 is the identity on byte-valued frames.
 * Any n > 0; src_dev 4-byte aligned, dst_dev any address (wide loads and stores between a scalar head and tail). */
int rgbm_quantize_frames(const float* src_dev, uint8_t* dst_dev, size_t n, void* stream);

/* Per-env mask extent for the controller's view queue.
 * Replaces: the np.nonzero / np.where loop of ControlInterface.add_view   models/controller/rl_pose.py:130-149
 * mask [N,H,W] u8 -> ext [N,4] i32 = (row min, col min, row max, col max), (2H, 2W, 0, 0) for an empty mask; count [N]. */
/* Projection matrices the network takes (interface_v5.py:264-270): P = eye(4), P[:3, :] = Kcrop @ E[:3, :] in fp64, stored as
 * float32.  Kcrop_dev [N][3][3] f64 (rgbm_prepare_inputs' Kcrop_out), E_dev [N][4][4] f64, P_dev [N][4][4] f32. */
int rgbm_projection(const double* Kcrop_dev, const double* E_dev, float* P_dev, int N, void* stream);
int rgbm_mask_extent(const uint8_t* mask_dev, int N, int H, int W, int32_t* ext_out, int32_t* count_out, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Controller step on the device: everything ControlInterface.step does between the simulator and the
 * estimator, one thread per environment, float64 in numpy's evaluation order.
 * ---------------------------------------------------------------------------------------------------------- */
/* Replaces: utils.transform.lookat_quat   utils/transform.py:50-99 (per-row branches; batch_zero = its whole-batch norm test)
 * dir [N,3] f64 -> quat [N,4] f64 (w,x,y,z).  The reference takes an eigenvector of Horn's matrix whose SIGN is LAPACK's
 * choice; here the first non-negligible component is positive (same rotation). */
int rgbm_lookat_quat(const double* dir_dev, int N, int batch_zero, double* quat_dev, void* stream);
/* Replaces: the action decode of ControlInterface.step   models/controller/rl_pose.py:390-408 (action_type "pose")
 * action [N,lda] f32 (device) -> pose [N,7] f64: clip(a[:3] + pose_mid, pose_min, pose_max), lookat_quat((1, dy, dz)).
 * pose_mid / pose_min / pose_max: 3 host doubles each. */
int rgbm_control_action_to_pose(const float* action_dev, int lda, const double* pose_mid, const double* pose_min,
                                const double* pose_max, int N, double* pose_dev, void* stream);
/* Replaces: ControlInterface.get_reward   models/controller/rl_pose.py:225-358, including quat_to_axis' batch scramble
 * (utils/transform.py:234) and LOSS:far aliasing the scaled far term (:247, :322).  All pointers are device pointers. */
typedef struct rgbm_control_reward_args {
  const float* action;        /* [N,lda] f32 policy action: xyz, dy, dz, -, view weights (T) */
  const double* cam_pose;     /* [N,7]   env.camera_pose(robot_frame=True) */
  const double* target;       /* [N,7]   last_pose_target */
  const float* move_success;  /* [N]     cam_move_to()[0] as float32 */
  const double* bbox;         /* [N,4]   bbox_queue[s % T] */
  const double* avail;        /* [N]     available[s % T] */
  const double* gt_bbox;      /* [N,8,3] gt_bbox[s] */
  const double* pred_bbox;    /* [N,8,3] pred_bbox[s] */
  const double* pose_cur;     /* [N,7]   pose_queue[s] */
  const double* pose_prev;    /* [N,7]   pose_queue[s-1] */
  const double* robot_pose;   /* [N,7]   env.robot_pose() */
  const double* success;      /* [N] */
  double* reward;             /* [N] out */
  double* terms;              /* [17][N] out or NULL: the 14 REW:* terms in sum order, LOSS:center_diff, LOSS:open_diff, LOSS:far */
  double coef[14];            /* diff, move_success, move_period, far, ori, xyz_lookat, bbox, bbox_boundary, have_bbox, center,
                                 open, view, view_norm, success */
  double proper_pos[3];
  double precision2;          /* precision^2: 0.01 for mugs, 0.04 otherwise */
  int N, T, lda, pots, first; /* T = max_steps (view weights per action); first = (accumulate_steps == 0) */
  int pad_;
} rgbm_control_reward_args;
int rgbm_control_reward(const rgbm_control_reward_args* args, void* stream);
/* Replaces: the centre / axis math of ControlInterface.call_manipulation   models/controller/rl_pose.py:364-377
 * est [N,8,3] f64 -> center [N,3], direction [N,3,3]. */
int rgbm_control_grasp_frame(const double* est_dev, int N, double* center_dev, double* direction_dev, void* stream);

/* Synthetic camera of the MultiVecEnv stand-in (no reference code: the reference renders with SAPIEN).
 * Produces what MultiVecEnv.get_image() returns (env/my_vec_env.py:266, base_manipulation.py:653-687) for a scene of one
 * oriented box per env.  rays [N,12] is scratch written by rgbm_synth_camera and read by rgbm_synth_render.
 * Bit-identical to oracle/synth_env_ref.py. */
typedef struct rgbm_synth_scene {
  const double* cam_pose;     /* [N,7] camera pose in the robot frame (x forward, y left, z up) */
  const double* robot_pose;   /* [N,7] robot root (position used) */
  const double* box;          /* [N,15] centre (3), axis rows X,Y,Z (9), half extents (3) */
  double fx, fy, cx, cy;
  int N, H, W, env0;
} rgbm_synth_scene;
int rgbm_synth_camera(const rgbm_synth_scene* scene, double* K_dev, double* E_dev, double* rays_dev, void* stream);
int rgbm_synth_render(const rgbm_synth_scene* scene, const double* rays_dev, float* color_dev, uint8_t* mask_dev, void* stream);
/* The same camera delivering bytes, e.g. straight into a slot of an 8-bit view queue: one kernel instead of render -> quantise ->
 * mask extent.  color_dev [N,H,W,3] u8 is bit for bit rgbm_quantize_frames of the frame rgbm_synth_render writes for this scene
 * (per channel the same float64 expression, rounded to float32, then min(max(rintf(x * 255.f), 0), 255)); mask_dev [N,H,W] u8 is
 * rgbm_synth_render's 0 / 1 mask.  extent_dev [N,4] i32 = (row min, col min, row max, col max) and count_dev [N] i32 are what
 * rgbm_mask_extent returns on that mask ((2H, 2W, 0, 0) and 0 for an env without a hit); the entry point initialises them itself
 * on `stream`.  Both may be NULL (colour and mask only); exactly one NULL is an argument error.  Any H, W and any output
 * addresses: 32-bit stores when H*W % 4 == 0 and color_dev, mask_dev are 4-byte aligned, byte stores otherwise. */
int rgbm_synth_render_u8(const rgbm_synth_scene* scene, const double* rays_dev, uint8_t* color_dev, uint8_t* mask_dev,
                         int32_t* extent_dev, int32_t* count_dev, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * PPO rollout storage.
 * Replaces: RolloutStorage.compute_returns   algo/ppo/ppo/storage.py:50-64
 * rewards/values/returns/adv [T,N] f32, dones [T,N] u8, last_values [N] f32.
 * sums: device f64 buffer with room for 2 + 2*ceil(N/256) doubles; on return sums[0..1] = {sum(adv), sum(adv^2)}
 * of the un-normalised advantages (all-reduce these two over ranks for the global normalisation), then
 * rgbm_adv_normalise applies (adv - mean) / (unbiased_std + 1e-8) with count_total = T*N summed over ranks.
 * ---------------------------------------------------------------------------------------------------------- */
int rgbm_gae(int T, int N, const float* rewards, const uint8_t* dones, const float* values, const float* last_values,
             float gamma, float lam, float* returns, float* adv, double* sums, void* stream);
int rgbm_adv_normalise(int64_t n_local, float* adv, const double* sums, double count_total, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * PPO policy (actor-critic MLPs) on a flat fp32 parameter vector laid out in the reference's state_dict order
 * (log_std, actor.{0,2,..}.{weight,bias}, critic.{0,2,..}.{weight,bias}).  Two descriptors: rgbm_policy_layout is the
 * shipped shape (obs -> h0 -> h1 -> h2 -> {act, 1}, ELU, both nets alike, widths <= 128, action dim <= 16);
 * rgbm_policy_desc and the *_ex entry points cover every ActorCritic the reference builds (module.py:10-54): per net 1..6
 * hidden layers of width 1..512, observation / state dim 1..512, action dim 1..32, one of six activations, an optional
 * second input for the critic, clipped or plain-MSE value loss.  A descriptor of the shipped shape runs the same kernels
 * through either set of entry points.  fp32 throughout; a descriptor outside the bounds is an error, nothing is launched.
 * Replaces: ActorCritic.act / act_inference / evaluate   algo/ppo/ppo/module.py:73-107
 *           one minibatch of PPO.update                   algo/ppo/ppo/ppo.py:472-528
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct rgbm_policy_layout {
  int dims[5];        /* obs, h0, h1, h2, act */
  int log_std;        /* offsets (in floats) into the flat parameter vector */
  int w[2][4];        /* [net: 0 actor, 1 critic][layer] weight offsets, row-major [out][in] */
  int b[2][4];
  int total;          /* number of parameters */
} rgbm_policy_layout;
/* mode 0: act (actions = mu + exp(2*log_std)*noise, log-prob, value, mu); 1: act_inference (mu only);
 * 2: evaluate (log-prob of the given actions, value, mu).  obs [n,dims[0]], noise/actions/mu [n,dims[4]], logp/value [n]. */
int rgbm_policy_forward(const float* params, const rgbm_policy_layout* L, int n, int mode, const float* obs, const float* noise,
                        float* actions, float* logp, float* value, float* mu, void* stream);
/* scratch floats needed by rgbm_ppo_minibatch_fwd_bwd for n rows */
int rgbm_ppo_partial_floats(const rgbm_policy_layout* L, int n, size_t* count);
/* forward + clipped-surrogate / clipped-value / entropy loss + backward for one minibatch of n rows.
 * grads_flat [total+4]: d loss / d params (mean over the n rows), then {sum surrogate, sum value loss, sum KL, rows}.
 * With several ranks: all-reduce(sum) grads_flat, then call rgbm_ppo_clip_adam with inv_world = 1/world. */
int rgbm_ppo_minibatch_fwd_bwd(const float* params, const rgbm_policy_layout* L, int n, const float* obs, const float* actions,
                               const float* old_logp, const float* adv, const float* returns, const float* old_values,
                               const float* old_mu, const float* old_log_std, float clip, float vcoef, float ecoef,
                               float* partial_scratch, float* grads_flat, void* stream);
/* clip_grad_norm_(max_norm) + KL-adaptive learning rate (ppo.py:486-495) + Adam(0.9,0.999,1e-8) in one launch.
 * opt_state: 48-byte device record {int t, n_updates; float lr, last_kl, last_norm, pad; double sum_surr, sum_vloss}. */
int rgbm_ppo_clip_adam(float* params, const float* grads_flat, float* exp_avg, float* exp_avg_sq, void* opt_state,
                       const rgbm_policy_layout* L, float inv_world, float max_norm, float desired_kl, float lr_min,
                       float lr_max, int adaptive, void* stream);

#define RGBM_POLICY_MAX_HIDDEN 6      /* hidden layers per net */
#define RGBM_POLICY_MAX_WIDTH 512     /* hidden width, observation dim, state dim */
#define RGBM_POLICY_MAX_ACT 32        /* action dim */
#define RGBM_ACT_ELU 0
#define RGBM_ACT_SELU 1               /* torch's scale / alpha */
#define RGBM_ACT_RELU 2               /* the reference's "relu" and "crelu" */
#define RGBM_ACT_LRELU 3              /* LeakyReLU(0.01) */
#define RGBM_ACT_TANH 4
#define RGBM_ACT_SIGMOID 5
typedef struct rgbm_policy_desc {
  int obs_dim, state_dim, act_dim;
  int activation;                     /* RGBM_ACT_*, both nets */
  int asymmetric;                     /* 1: the critic's first layer reads states [n,state_dim] instead of obs */
  int n_hidden[2];                    /* [net: 0 actor, 1 critic] */
  int hidden[2][RGBM_POLICY_MAX_HIDDEN];
  int w[2][RGBM_POLICY_MAX_HIDDEN + 1];   /* n_hidden+1 linear layers per net: weight offsets (floats), row-major [out][in] */
  int b[2][RGBM_POLICY_MAX_HIDDEN + 1];
  int log_std;
  int total;                          /* number of parameters */
} rgbm_policy_desc;
/* rgbm_policy_forward for any descriptor; states may be NULL unless asymmetric and mode != 1. */
int rgbm_policy_forward_ex(const float* params, const rgbm_policy_desc* D, int n, int mode, const float* obs, const float* states,
                           const float* noise, float* actions, float* logp, float* value, float* mu, void* stream);
/* floats of device scratch rgbm_ppo_minibatch_fwd_bwd_ex needs for n rows: per 64-row tile the partial gradient and, for the
 * general kernels, the activations and deltas of both nets (the backward pass keeps them in global memory, not in LDS). */
int rgbm_ppo_scratch_floats_ex(const rgbm_policy_desc* D, int n, int clipped_value_loss, size_t* count);
/* rgbm_ppo_minibatch_fwd_bwd for any descriptor.  clipped_value_loss 1: max((v-ret)^2, (v_clipped-ret)^2) (ppo.py:505-510);
 * 0: mean((ret-v)^2) (ppo.py:512), old_values may then be NULL.  Same grads_flat layout; the reduction over tiles is
 * fixed-order, so the same inputs give the same bits. */
int rgbm_ppo_minibatch_fwd_bwd_ex(const float* params, const rgbm_policy_desc* D, int n, const float* obs, const float* states,
                                  const float* actions, const float* old_logp, const float* adv, const float* returns,
                                  const float* old_values, const float* old_mu, const float* old_log_std, float clip, float vcoef,
                                  float ecoef, int clipped_value_loss, float* scratch, float* grads_flat, void* stream);
/* rgbm_ppo_clip_adam by parameter count. */
int rgbm_ppo_clip_adam_ex(float* params, const float* grads_flat, float* exp_avg, float* exp_avg_sq, void* opt_state, int total,
                          float inv_world, float max_norm, float desired_kl, float lr_min, float lr_max, int adaptive, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Layer-level entry points (used by the parity tests and by the Python host for pieces it drives itself).
 * ---------------------------------------------------------------------------------------------------------- */
/* Generic N-D convolution on channels-last tensors, weights given in PyTorch layout on the host
 * (nn.Conv2d/Conv3d: [Cout][Cin][KD][KH][KW]; nn.ConvTranspose3d(k3,s2,p1,op1) when transposed=1: [Cin][Cout][3][3][3]).
 * in_dev [N][D][H][W][Cin_pad], out_dev [N][Do][Ho][Wo][Cout_pad] in `dtype`; act 0 none 1 relu 2 prelu 3 tanh;
 * res_mode 0 none 1 add before activation 2 add after activation. */
int rgbm_conv_nd(int dtype, const void* in_dev, int N, int D, int H, int W, int Cin, int Cin_pad, const float* w_host,
                 int Cout, int Cout_pad, int KD, int KH, int KW, int stride_d, int stride_hw, int pad_d, int pad_hw,
                 int dil_hw, int transposed, const float* bias_host, const float* bn_scale_host, const float* bn_shift_host,
                 const void* res_dev, int res_mode, int act, float slope, void* out_dev, void* stream);
/* What rgbm_conv_nd would launch for this geometry (same arguments; has_bias / res_mode say whether there is a bias / residual buffer),
 * without launching anything: buffers are taken as 16-byte aligned, debug flags and tuning are the process's current ones.  cls: sub-pixel
 * class 0..7 of a transposed conv (one launch each), else 0.  n_cu: compute units to plan for; 0 = the current device's, any positive value
 * is taken as given and the HIP runtime is not touched (works without a GPU).  plan[RGBM_CONV_PLAN_INTS]:
 *   [0] kernel: 0 generic tile, 1 v3, 2 ws 128 x 256, 3 ws wide 256 x 128, 4 ws slim 64 x 256, 5 ws64, 6 ws64 row halo,
 *       7 m32 main + tail launch (256-multiple channels), 8 m32 small launch (one launch of 128-pixel tiles that does not fill the grid)
 *   [1] [2] tile channels x pixels (kernel 7: of the main launch)      [3] K parts the launch asks for (1 = no split)
 *   [4] kernel 7: GEMM rows on 256 x 256 tiles      [5] kernel 7: channel tile of the 128-pixel tail launch (0 = none)
 *   [6] 1 = residual added through identity K steps, 0 = in the epilogue (or none)      [7] GEMM rows M      [8] K tiles KT */
#define RGBM_CONV_PLAN_INTS 9
int rgbm_conv_plan(int dtype, int N, int D, int H, int W, int Cin, int Cin_pad, int Cout, int Cout_pad, int KD, int KH, int KW,
                   int stride_d, int stride_hw, int pad_d, int pad_hw, int dil_hw, int transposed, int has_bias, int res_mode, int act,
                   int cls, int n_cu, int32_t* plan);
/* Border-class tiles of a dilated 2-D conv (K x K, stride, pad, dil; one pre-activation residual when res_mode = 1) on the 256 x 256
 * tiles of kernel 7: output pixels whose set of in-range taps is the same form a class, a tile is 256 rows of one class taken across
 * views (row r of a class: view r / n, class pixel r % n, row-major inside the class, up to the last GEMM row of the 256 x 256 launch; the class
 * is padded to whole tiles with dead rows)
 * and walks only the class's taps, and the tiles are dealt in the order of the views they cover (the last round longest first) to the
 * workgroup with the fewest K steps so far.  Every row then
 * of the 256 x 256 launch (rgbm_conv_plan's [4]) then runs on these tiles; the rows behind them keep their tail launch.  Works without a GPU when n_cu > 0 (as rgbm_conv_plan).  The plan declines (head[0] = 0,
 * nothing else filled) for 1 x 1 convs, stride != 1, launches that do not reach the 256 x 256 tiles, shapes where no K step is saved,
 * and under debug flag 32 / 1048576; a layer whose weights hold a NaN / inf declines at its launches.
 *   head[RGBM_BORDER_HEAD_INTS]: [0] 1 = taken  [1] classes  [2] tiles  [3] workgroups  [4] table rows (dead ones included)
 *     [5] K steps of the busiest workgroup  [6] K steps of all tiles (mean per workgroup = [6] / [3])
 *     [7] K steps of the row-major tiles (every tile walks every tap)  [8] K steps per tap (Cin / 64; split pairs: Cin / 32)
 *     [9] residual steps per tile
 *   classes[3 * cap_classes]: {pixels of a view, tap mask (bit kh * K + kw), first table row} per class
 *   tiles[5 * cap_tiles]: {class, channel tile, tap mask, K steps (residual steps included), first table row} per tile
 *   order[cap_tiles] + wg_off[cap_wg]: workgroup b runs tiles order[wg_off[b] .. wg_off[b + 1]) in this order
 *   rows[cap_rows]: GEMM row (view * H + h) * W + w (below rgbm_conv_plan's [4]) of every table row, -1 = dead
 * Every array may be null (not wanted); a capacity that is too small is an error. */
#define RGBM_BORDER_HEAD_INTS 10
int rgbm_conv_border_plan(int dtype, int N, int H, int W, int Cin, int Cout, int K, int stride, int pad, int dil, int res_mode, int n_cu,
                          int32_t* head, int32_t* classes, int cap_classes, int32_t* tiles, int32_t* order, int cap_tiles, int32_t* wg_off,
                          int cap_wg, int32_t* rows, int64_t cap_rows);
/* Launches that ran on border-class tiles since the library was loaded (process-wide; what a test reads to see that a launch took them). */
int rgbm_conv_border_launches(int64_t* count);
/* Per-sample BatchNorm3d of the as-shipped mode (norm_mode = 1), in place: y_dev [V][nvox][C] (C % 4 == 0, C <= 64) in `dtype`
 * -> relu(gamma * (y - mean_v) / sqrt(var_v + 1e-5) + beta) + res, with the biased mean / variance of each view v's own volume;
 * relu 0 skips the ReLU, res_dev may be null (post-activation skip add otherwise, same layout).  gamma_dev / beta_dev [C] fp32;
 * scratch_dev holds rgbm_bn_per_sample_scratch_bytes(V) bytes. */
int rgbm_bn_per_sample_scratch_bytes(int V, size_t* bytes);
int rgbm_bn_per_sample(int dtype, void* y_dev, const void* res_dev, const float* gamma_dev, const float* beta_dev, void* scratch_dev,
                       int V, int64_t nvox, int C, int relu, void* stream);
/* Halo-tiled 3-D conv of the cost-regularisation stack, one layer: layer 0..6 = conv0..conv6 (k3, pad 1, stride 1/2),
 * 7..9 = conv7/conv9/conv11 (ConvTranspose3d k3 s2 p1 op1).  Channels are fixed by the layer (network_v5.py:263-278);
 * in_dev [N][D][H][W][Cin], out_dev [N][Do][Ho][Wo][Cout], folded BN scale/shift on the host, ReLU, optional
 * post-activation residual res_dev (same layout as out). */
int rgbm_conv3d_tile(int layer, int dtype, const void* in_dev, int N, int D, int H, int W, const float* w_host,
                     const float* bn_scale_host, const float* bn_shift_host, const void* res_dev, void* out_dev, void* stream);
/* PSPUpsample (pspnet.py:100-107: x2 bilinear align_corners=True -> Conv2d 3x3 pad 1 + bias -> activation) as the network runs
 * it: a 1x1 GEMM at the low resolution with the nine taps stacked on the output channels (z_scratch_dev: V*h*w*9*Cout elements
 * of `dtype`), then the tap-combining kernel.  in_dev [V][h][w][Cin], w_host [Cout][Cin][3][3], out_dev [V][2h][2w][Cout]. */
int rgbm_upsample_conv3x3(int dtype, const void* in_dev, int V, int h, int w, int Cin, const float* w_host, int Cout,
                          const float* bias_host, int act, float slope, void* z_scratch_dev, void* out_dev, void* stream);
/* The PSPNet tail as the 16-bit / split-pair network runs it: up_3 (PSPUpsample 64 -> 64, PReLU `slope`) and `final`
 * (pspnet.py:136, Conv2d 1x1 64 -> 32 + bias) in one kernel (upconv_final.hip).  in_dev [V][h][w][64] (h, w multiples of 8),
 * w3_host [64][64][3][3], b3_host [64], wf_host [32][64], bf_host [32]; dtype RGBM_BF16 / RGBM_F16 / RGBM_BF16X3.
 * out_f32 is an ENUM since round 5 (it was a boolean before; any other value is refused with RGBM_ERR_ARG):
 *   0 = out_dev [V][2h][2w][32] in `dtype`;
 *   1 = plain fp32 output (RGBM_BF16X3 only: the feature map the split-pair plane sweep gathers from);
 *   2 = IEEE f16 output through the packed-f16 tail (RGBM_BF16 only: the bf16 network's `sweep_f16` feature map; refused when
 *       `final`'s weights do not fit f16 — a value >= 65504 or more than 0.1 % of the weight mass below 2^-14). */
int rgbm_upsample_conv3x3_final(int dtype, const void* in_dev, int V, int h, int w, const float* w3_host, const float* b3_host,
                                float slope, const float* wf_host, const float* bf_host, void* out_dev, int out_f32, void* stream);
/* The ResNet stem as the 16-bit / split-pair network runs it (stem.hip): Conv2d 7x7 stride 2 pad 3 (3 -> 64, no bias, pspnet.py:37)
 * -> ReLU -> MaxPool2d 3x3 stride 2 pad 1 (pspnet.py:39) in one kernel.  img1_dev / img2_dev [B][3][S][S] fp32 NCHW (views
 * 0..B-1 / B..2B-1), w_host [64][3][7][7]; out_dev [2B][S/4][S/4][64] in `dtype` (RGBM_BF16 / RGBM_F16 / RGBM_BF16X3); S % 32 == 0. */
int rgbm_stem(int dtype, const float* img1_dev, const float* img2_dev, const float* w_host, void* out_dev, int B, int S, void* stream);
int rgbm_maxpool3x3s2(int dtype, const void* in_dev, void* out_dev, int V, int H, int W, int C, void* stream);
int rgbm_resize_bilinear_ac(int dtype, const void* in_dev, void* out_dev, int V, int Hs, int Ws, int C, int Ho, int Wo,
                            void* stream);
int rgbm_adaptive_avgpool(int dtype, const void* in_dev, void* out_dev, int V, int H, int W, int C, int S, void* stream);
/* fused plane-sweep volume for views [0,V): feat [V][H][W][32] (dtype), P [V][4][4] f32 (views ordered side*B+b),
 * depths [B][D] f32 -> vol [V][D][H][W][32]; homog_scratch: V*12 floats */
int rgbm_build_volume(int dtype, const void* feat_dev, const float* P_views_dev, const float* depths_dev, float* homog_scratch,
                      void* vol_dev, int V, int B, int D, int H, int W, void* stream);
/* the same with the fusion named: 0 = feat[v] + warped (rgbm_build_volume), 1 = the real-world network's variance -2 feat[v] warped
 * (one fp32 product, rounded once to the storage type; not for RGBM_F16) */
int rgbm_build_volume_fusion(int dtype, int fusion, const void* feat_dev, const float* P_views_dev, const float* depths_dev, float* homog_scratch,
                             void* vol_dev, int V, int B, int D, int H, int W, void* stream);
/* conv0 of the cost-regularisation net with the plane sweep fused in, depth-sweeping kernel (bf16 only; what
 * cost_impl = 3 runs): feat [V][H][W][32] bf16 (views 0..B-1 = view 1, B..2B-1 = view 2), P_views [V][4][4], depths [B][D],
 * homog_scratch [V*12] floats, w_host [8][32][3][3][3] + folded BatchNorm scale/shift [8] on the host ->
 * out [V][D][H][W][8] bf16 = ReLU(BN(conv3d(feat[v] + homo_warping(feat[partner(v)])))) (network_v5.py:262,378-430). */
int rgbm_conv0_sweep(const void* feat_dev, const float* P_views_dev, const float* depths_dev, float* homog_scratch,
                     const float* w_host, const float* bn_scale_host, const float* bn_shift_host, void* out_dev,
                     int V, int B, int D, int H, int W, void* stream);
/* the same kernel for either 16-bit storage type (dtype = RGBM_BF16 or RGBM_F16; feat / out in that type); dtype = RGBM_BF16X3
 * runs conv0_sweep_x3_kernel: feat is PLAIN fp32 [V][H][W][32], out is the split-pair tensor [V][D][H][W][8] */
int rgbm_conv0_sweep_dt(int dtype, const void* feat_dev, const float* P_views_dev, const float* depths_dev, float* homog_scratch,
                        const float* w_host, const float* bn_scale_host, const float* bn_shift_host, void* out_dev,
                        int V, int B, int D, int H, int W, void* stream);
/* what a bf16 net runs by default since round 5 (option "sweep_f16" = 1): feat is f16 [V][H][W][32] (written so by the net's `final`
 * layer), the conv0 weights are rounded to f16, the blend is packed-f16 arithmetic, out is bf16 [V][D][H][W][8].  Features beyond
 * +-65504 saturate (as in an fp16 net); set the option to 0 for the all-bf16 form (rgbm_conv0_sweep). */
int rgbm_conv0_sweep_f16feat(const void* feat_f16_dev, const float* P_views_dev, const float* depths_dev, float* homog_scratch,
                             const float* w_host, const float* bn_scale_host, const float* bn_shift_host, void* out_bf16_dev,
                             int V, int B, int D, int H, int W, void* stream);
/* debugging access to a named intermediate of the last rgbm_adapose_forward on (h, B, workspace):
 * converts it to fp32 into out_dev (elems = capacity in floats); *n_elems returns its size.  Intermediates of the
 * PSPNet phase are overwritten by the cost-volume phase, so pass stop_after = 1 to rgbm_adapose_forward_ex first.
 * The 3-D taps "c0" "c2" "c4" "c6" "u7" "u9" exist as whole tensors only with option sparse_dec = 0: with the default (sparse cost
 * regularisation) the call fails with an error instead of returning tensors that are stale outside the dependency cones.
 * "pf96" of a split-pair net is converted back from the hi / lo pairs the pose MLP consumed. */
int rgbm_adapose_forward_ex(rgbm_adapose_t* h, int B, const float* img1, const float* img2, const int32_t* choose1,
                            const int32_t* choose2, const float* P1, const float* P2, const float* depths, void* workspace,
                            size_t workspace_bytes, const rgbm_adapose_out* out, int stop_after, void* stream);
/* rgbm_adapose_forward replayed from a hipGraph (small batches — the reference calls the network at batch 1 per env,
 * interface_v5.py:213-227,259-280, and ships num_envs: 8 — are launch-bound: ~150 launches per forward).  The first call with a
 * given (B, every device pointer, workspace, outputs, stream) runs the forward once eagerly, captures its launch sequence on `stream` and
 * keeps the instantiated graph (up to 8 per handle, least recently used evicted; dropped when an option changes); later calls with the
 * same arguments replay it with one hipGraphLaunch.  The caller keeps every buffer alive and at the same address.  `stream` must be
 * a created (non-null) stream.  *n_nodes (optional) = graph nodes (kernel launches + copies) of this batch size; *captured
 * (optional) = 1 when this call did the capture, 0 on a replay, -1 when it ran eagerly because rgbm_prof_start is active.
 * The capture stream is part of the key: the captured launches of a small batch use the K-split scratch of the stream they were captured on
 * (rgbm_debug_flags 16384), which other streams' forwards do not share, so a call with the same buffers on another stream warms up and
 * captures a graph of its own (*captured = 1, the same limit of 8) instead of replaying the first stream's. */
int rgbm_adapose_forward_graph(rgbm_adapose_t* h, int B, const float* img1, const float* img2, const int32_t* choose1,
                               const int32_t* choose2, const float* P1, const float* P2, const float* depths, void* workspace,
                               size_t workspace_bytes, const rgbm_adapose_out* out, void* stream, int32_t* n_nodes, int32_t* captured);
int rgbm_adapose_graph_clear(rgbm_adapose_t* h);
/* Feature cache: the forward split where the PSPNet ends.  A view's 32-channel feature map depends on its image alone (shared weights,
 * no Dropout2d in eval mode), so a caller that meets a frame in two forwards - the controller loop pairs frame t with frame t - 1 in
 * every step - computes the map once, keeps it in a pool of records it owns, and runs the rest of the forward from slot tables.
 * rgbm_adapose_feature_bytes: size of one view's record = exactly what the stages behind the PSPNet read with the handle's current
 *   options: the f16 (option sweep_f16 = 0: bf16) map for bf16 nets, the fp16 map for fp16 nets, the fp32 map for fp32 and bf16x3
 *   nets; bf16x3 nets on the paths that still read the split-pair map (norm_mode 1, cost_impl < 3) keep that map in front of the
 *   fp32 one (twice the size).  Query it after the options are set; records written under other options are not interchangeable.
 * rgbm_adapose_features: the PSPNet - the launches and arithmetic of rgbm_adapose_forward - on V >= 1 views (odd V included) of one
 *   array img [V,3,224,224] fp32; view v's record goes to pool + slots_dev[v] * feature_bytes.  pool: pool_records records, 16-byte
 *   aligned.  workspace: rgbm_adapose_features_workspace_bytes(V) bytes, 256-byte aligned (the one of rgbm_adapose_workspace_bytes(B)
 *   serves V <= 2 B views).
 * rgbm_adapose_forward_cached: rgbm_adapose_forward with the PSPNet replaced by reading records slot1_dev[b] / slot2_dev[b] ([B] int32
 *   each) for the view-1 / view-2 crop of pose b; every option (view2_heads, sparse_dec, chunking, norm_mode ...) holds as in the plain
 *   forward, and the workspace is that of rgbm_adapose_workspace_bytes(B).  With records written by one rgbm_adapose_features call on
 *   the 2 B views in [view1 batch ; view2 batch] order the outputs are bit-identical to rgbm_adapose_forward's.
 * Refused (error through rgbm_last_error, nothing launched): a handle with Dropout2d on (set_dropout p > 0 or explicit masks pending) -
 *   the masks are per pose and per forward, a kept map would change the as-shipped semantics.  A slot outside [0, pool_records) is
 *   checked on the device: features writes nothing for it; forward_cached reads nothing, and that pose's ten outputs are NaN (the
 *   other poses are unaffected).  Not provided: a graph-replayed or split-stream cached forward. */
int rgbm_adapose_feature_bytes(rgbm_adapose_t* h, size_t* bytes);
int rgbm_adapose_features_workspace_bytes(rgbm_adapose_t* h, int V, size_t* bytes);
int rgbm_adapose_features(rgbm_adapose_t* h, int V, const float* img, const int32_t* slots_dev, void* pool, int pool_records,
                          void* workspace, size_t workspace_bytes, void* stream);
int rgbm_adapose_forward_cached(rgbm_adapose_t* h, int B, const void* pool, int pool_records, const int32_t* slot1_dev,
                                const int32_t* slot2_dev, const int32_t* choose1, const int32_t* choose2, const float* P1, const float* P2,
                                const float* depths, void* workspace, size_t workspace_bytes, const rgbm_adapose_out* out, void* stream);
int rgbm_adapose_fetch(rgbm_adapose_t* h, int B, void* workspace, const char* name, float* out_dev, size_t capacity,
                       size_t* n_elems, void* stream);
/* Content key of prepared crops: a caller that gets its frames as fresh arrays on every call (the numpy `estimate` boundary) has no
 * slot to name a frame by; it recognises the PSPNet's input, img[v] ([3,S,S] fp32 = n_words 32-bit words), by two 64-bit words
 *   keys_out[v][k] = sum over i < n_words of mix((bits(w_i) | (uint64)i << 32) ^ SEED_k)   (mod 2^64),   k = 0, 1,
 *   mix(x): x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31      (splitmix64's finaliser),
 *   SEED_0 = 0x9E3779B97F4A7C15, SEED_1 = 0xD1B54A32D192ED03.
 * Integer arithmetic throughout, and the sum commutes: the keys do not depend on the grid or on the order of the partial sums.  The
 * bit pattern is hashed, not the value: +0.0 and -0.0 differ, every NaN pattern is its own.  img: V rows of n_words words, dense, 4-byte
 * aligned (rows that are not 16-byte aligned are read through a scalar head and tail); V in [1, 65535], n_words >= 1; keys_out: [V,2]
 * uint64 on the device, written by this call (zeroed, then summed into).  One launch for any V.  (rgbmanip_amd/feature_keys.py holds
 * the numpy restatement and the host table that turns keys into record slots.) */
int rgbm_crop_fingerprint(const float* img, int V, int n_words, uint64_t* keys_out, void* stream);

/* Live per-kernel timing for bench.py's roofline figure: between start and stop every convolution launch is
 * bracketed by HIP events recorded on its own stream.  stats: host double[RGBM_PROF_ROWS * 4], one row per kernel family,
 * columns {launches, total ms, algorithmic FLOPs, algorithmic bytes}; rgbm_prof_rows() returns RGBM_PROF_ROWS of the
 * library that is loaded (size the buffer from it when binding dynamically).  Rows:
 *  0..7   conv_igemm_glds_kernel<dtype, BCH> (row = dtype*4 + {0:16,1:32,2:64,3:128}-channel tile; dtype 0 f32, 1 16-bit)
 *  8 / 9  conv3d_tile_kernel f32 / (unused)          10 / 11  conv3d_tile_kernel conv0 + fused plane sweep f32 / 16-bit
 *  12 / 13 conv_igemm_ws_kernel 128 x 256 tile (and conv_igemm_v3_kernel) f32 / 16-bit
 *  14     conv0_sweep[_persistent]_kernel (16-bit)            15  conv_igemm_ws64_kernel (16-bit)
 *  16..25 conv3d_tile_kernel 16-bit per layer (conv0..conv6, conv7, conv9, conv11)
 *  26..29 bf16x3: generic implicit GEMM, 3-D layers, conv0 + plane sweep, ws 128 x 256 tile
 *  30 / 32 pose_mlp1_kernel / pose_mlp2_kernel: the per-point layers of the pose MLP of a bf16 net, two layers per launch (f16)
 *  31     ws 256 x 128 tile 16-bit
 *  33     ws 256 x 128 tile bf16x3                   34 / 35 / 36  ws 64 x 256 four-multiply-wave tile bf16x3 / 16-bit / f32
 *  37 / 38 upconv_combine_kernel 16-bit / 4-byte storage                39  upconv_final_kernel
 *  40 / 41 conv_igemm_m32_kernel<T, 128, 64 / 128 / 256>: the 128-pixel tail and small-batch launches of rows 31 / 33 (16-bit / bf16x3;
 *          rows 31 / 33 are conv_igemm_m32_kernel<T, 256, 256> under the default gemm_kernel = 2, conv_igemm_ws_kernel<T, wide> under gemm_kernel = 0)
 * stop synchronises on the recorded events. */
#define RGBM_PROF_ROWS 42
/* A/B switches for kernel benchmarking and the parity tests of the non-default kernel variants (0 = normal operation; bits OR together):
 *      8  no persistent ws kernels (generic tiles)
 *     16  treat every conv as non-uniform taps (v3 / generic kernels)                          64  v3 kernel instead of the ws kernel
 *    128  no ws64 kernel      256  ws64 without the row-halo variant      512  generic resize instead of the x2 kernel
 *     32  no border-class tiles: dilated 3 x 3 layers on the 256 x 256 tiles run row-major tiles and multiply the padding taps
 *          (default: rgbm_conv_border_plan; same bits either way)
 *  32768  layer2's 128-channel layers at one to four poses on the 64 x 256 tile of conv_igemm_ws_kernel as before (default since round 6:
 *          64-channel x 128-pixel tiles of conv_igemm_m32_kernel with the K split, residual added in the epilogue)
 *  16384  no K split of the 256-channel GEMM's launches of few tiles (small batches; default since round 6: the K loop of a 64 / 128-channel x
 *          128-pixel tile is cut into up to four parts, one workgroup each, when the tiles fill at most half the CUs; fixed-order fp32 sum)
 *   2048  per-point NOCS branch as in rounds 1-5: a gather launch and six fp32 1x1 GEMM launches (default since round 6: point_mlp_kernel)
 *   1024  PSP stage as in rounds 1-5: copy, pooling, four 1x1 GEMM launches, four resize launches (default since round 6: one concat launch;
 *          up to 32 views also pooling + the four 1x1 convs in one launch on the vector pipe)
 *   4096  halo-tile conv0 instead of the plane-sweep kernels             65536  128 x 256 ws tile even where the 256-channel tiles apply
 *          (4 / 8192 / 131072 selected the register-staged kernel, the 256 x 256 two-group kernel and the row-halo wide tile of rounds
 *          1-2: measured slower, removed in round 6; the bits are ignored)
 * 262144  generic tile instead of the 64 x 256 four-wave ws tile         1048576  ws request waves walk K taps outer, channel blocks inner
 *                                                                                  (default since round 3: channel block outer, taps inner)
 * 2097152  plane sweep of a bf16 feature map (option sweep_f16 = 0): blend on fp32 FMAs from inline asm; fp16 nets: the packed-f16 blend
 *          instead of their fp32-accumulating one                        4194304  bf16 feature map: v_perm + v_dot2_f32_bf16 (8-bit bilinear
 *                                                                                  weights; the round-4 default; since round 5: plain fp32 blend)
 * 8388608  one-workgroup-per-pose post-processing even with scratch      16777216  no 64 x 256 tile for small persistent launches
 * 33554432 post-processing: generic fp64 radix selection of the median only (the fall-back of the default selection on fp32
 *          approximations; same result bit for bit)                    67108864  post-processing: guard band in every even-count pose
 * 134217728 implicit-GEMM request waves: 64-bit global addresses + zero page instead of buffer descriptors (the form before round 5)
 * 268435456 plane sweep of an f16 feature map (bf16 nets, sweep_f16 = 1; fp16 nets since round 6): one workgroup per tile instead of the
 *          persistent kernel            536870912  sparse tail: the round-3..5 point kernel instead of prob_sparse2_kernel
 * 1073741824 256-channel GEMM: tail and small launches on 256-channel x 128-pixel tiles / the 64 x 256 ws tile as in round 5
 *  524288  pose MLP of a bf16 net as per-layer launches: conversion, four 1x1 GEMMs, two mean kernels (default: pose_mlp1_kernel + pose_mlp2_kernel) */
int rgbm_debug_flags(int flags);
/* Kernel choice - tile shape, and with it the order of the fp32 sums - depends on a launch's GEMM rows, i.e. on the batch size: the
 * same pose in batches of different sizes agrees to the storage type's rounding (1e-6 .. 1e-5 relative in fp32 / bf16x3), not bit for
 * bit.  Equal-sized batches (and the two half batches of split_streams) are bit-identical.
 * dispatch thresholds (process-wide, like the debug flags).  "ws_min_rows": GEMM rows (output pixels of a conv launch) from which
 * the persistent role-specialised implicit-GEMM kernels are used instead of the generic tiles; 0 (default) = 1024 (measured at
 * B = 1 .. 8 in every storage type; rounds 1-3 used 65536).  Launches whose 64-channel x 256-pixel tiles fit one round of the
 * persistent grid take that tile shape (debug flag 16777216 disables it).
 * "gemm_kernel": kernel of the launches whose output channels are a multiple of 256 (layer3 / layer4 / up_1) in the 16-bit storage
 * types: 0 = conv_igemm_ws_kernel (16x16x32 MFMAs, 256 x 128 tile), 1 = conv_igemm_m32_kernel on 256 x 128 tiles (32x32x16 MFMAs,
 * one multiply wave per SIMD), 2 (default) = whole rounds of 256 x 256 tiles + a 256 x 128 tail launch.  1 and 2 add a pre-activation
 * residual on the matrix pipe (identity K steps) and give bit-identical results; 0 differs from them in the last bit of a few
 * residual sums per million.  Debug flag 134217728: the persistent kernels' request waves use 64-bit global addresses and a zero page
 * instead of buffer descriptors (A/B). */
int rgbm_set_tuning(const char* key, long long value);
/* Achievable-peak probes (the peaks the box reaches, next to the datasheet ones; no reference counterpart).  Asynchronous:
 * the caller times them with events on `stream`.  rgbm_microbench_mfma: a bare v_mfma_f32_16x16x32_bf16 stream, 8 waves per CU on
 * every CU, `iters` x 32 MFMAs per wave on constant (random_operands = 0) or pseudo-random operands; `scratch` holds
 * rgbm_microbench_mfma_scratch_floats floats; *flops = the flops the launch executes.  rgbm_microbench_copy: grid-stride 16-byte copy. */
int rgbm_microbench_mfma_scratch_floats(int* n);
int rgbm_microbench_mfma(float* scratch, int iters, int random_operands, double* flops, void* stream);
int rgbm_microbench_copy(const void* src, void* dst, size_t bytes, void* stream);
int rgbm_prof_rows(void);
int rgbm_prof_start(void);
int rgbm_prof_stop(double* stats);
/* Restrict the per-launch events to one row of the table (-1 = every row, the default): two events per launch cost ~3.5 us, i.e.
 * 0.35 ms per 256-pose forward when every launch is bracketed; bench.py brackets only the dominant kernel inside its timed region. */
int rgbm_prof_select(int row);

#ifdef __cplusplus
}
#endif
#endif /* RGBM_H_ */
