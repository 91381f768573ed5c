// Host-side launchers of the helper kernels (misc_kernels.hip, head_kernels.hip, postproc.hip, ppo_kernels.hip).
#pragma once
#include <vector>

#include "common.h"

namespace rgbm {

// misc_kernels.hip
int launch_nchw_to_nhwc_pad(int dtype, const float* in, void* out, int V, int C, int H, int W, int Cp, hipStream_t s);
int launch_maxpool3x3s2(int dtype, const void* in, void* out, int V, int H, int W, int C, hipStream_t s);
int launch_resize_bilinear_ac(int dtype, const void* in, void* out, int V, int Hs, int Ws, int C, int Ho, int Wo, int ldo,
                              int ch_off, hipStream_t s);
int launch_copy_channels(int dtype, const void* in, void* out, long long npix, int C, int ldo, int ch_off, hipStream_t s);
int launch_adaptive_avgpool(int dtype, const void* in, void* out, int V, int H, int W, int C, int S, hipStream_t s);
int launch_adaptive_avgpool_multi(int dtype, const void* in, void* const* outs, const int* bins, int nb, int V, int H, int W, int C,
                                  hipStream_t s);
// PSP stage of small batches (misc_kernels.hip): pooling + the four 512 -> 128 1x1 convs in one launch (small batches); the whole concat (copy + four resizes) in one
int launch_psp_pool_conv(int dtype, const void* in, int ldi, const void* const* w, void* const* outs, const int* bins, int V, int H, int W,
                         int act, float slope, hipStream_t s);
int launch_psp_resize_cat(int dtype, const void* f, const void* const* stages, const int* bins, void* out, int V, int Ho, int Wo, hipStream_t s);
int launch_homography(const float* P_views, float* out, int V, int B, hipStream_t s);
// How the plane sweep fuses a view's feature with its warped partner, a compile-time parameter of every kernel that builds voxels:
// FUSION_SUM ref + warped (network_v5.py:429-430), FUSION_VARIANCE -2 ref warped = ref^2 + warped^2 - (ref + warped)^2
// (network_realworld.py:145-166) - one fp32 product of the bilinear sum, rounded once to the voxel's storage; 0 where the partner
// view projects outside the image.  The packed-f16 forms have no variance (a product of two features squares their range).
enum { FUSION_SUM = 0, FUSION_VARIANCE = 1 };
int launch_build_volume(int dtype, const void* feat, const float* homog, const float* depths, void* vol, int v0, int Vc, int V,
                        int B, int D, int H, int W, hipStream_t s, int fusion = FUSION_SUM);

// upconv.hip — tap-combining half of PSPUpsample evaluated as a low-resolution 1x1 GEMM (layers.h, UpConvLayer):
// z [V][h][w][9*Co] (tap-major) -> out [V][2h][2w][ldo] = act(bias + sum_t bilinear(z_t)(p + t))
// drop (optional): Dropout2d factors of this site, drop[v * kDropoutPerView + c], multiplied in after the activation (dropout.hip)
int launch_upconv_combine(int dtype, const void* z, const float* bias, void* out, int V, int h, int w, int Co, int ldo, int act,
                          float slope, hipStream_t s, const float* drop = nullptr);
// up_3 + final of the PSPNet tail in one kernel (upconv_final.hip): x [V][h][w][64] -> out [V][2h][2w][32]
int launch_upconv_final(int dtype, const void* x, const void* wz, const float* bias, float slope, const void* wf, const float* biasf,
                        void* out, int out_f32, int V, int h, int w, hipStream_t s, const void* wf_f16 = nullptr);      // wf_f16: `final` weights in f16 (out_f32 == 2)

// dropout.hip — seeded Dropout2d of PSPNet (up_1: 256 channels, up_2: 64): factors masks[V][kDropoutPerView] (up_1's channels, then
// up_2's), each 0 or dropout_scale(p); pose index = state[0] + the pose's place in the batch, state[0] += B when `advance`
constexpr int kDropoutPerView = 256 + 64;
unsigned dropout_threshold(float p);
float dropout_scale(float p);
int launch_dropout_masks(float* masks, unsigned long long* state, int B, float p, unsigned long long seed, int advance, hipStream_t s);

// bn_kernels.hip — per-sample (train-mode, batch 1) BatchNorm3d + ReLU + skip add, in place on the un-normalised conv output
size_t bn_scratch_bytes(int V);
int launch_bn_per_sample(int dtype, void* y, const void* res, const float* gamma, const float* beta, void* scratch, int V,
                         long long nvox, int C, int relu, hipStream_t s);

int launch_to_f32(int dtype, const void* in, float* out, long long n, hipStream_t s);

// head_kernels.hip
int launch_gather_points(int dtype, const void* feat, const int* choose, float* out, int V, int P, int HW, int C, hipStream_t s);
int launch_prob_softmax_depth(int dtype, const void* u11, const float* wprob, const int* choose, const float* depths,
                              float* prob, float* depth_out, int v0, int Vc, int B, int P, int D, int H, int W, int classmajor,
                              hipStream_t s);
// dense_depth.hip: the same prob conv + softmax + expected depth at EVERY pixel of views v0 .. v0 + Vc - 1 (u11 of that chunk, either
// layout) -> depth_map / conf_map [views][H][W] fp32 (conf = max_d p; conf_map may be null); depths [B][D], view v reads row v % B
int launch_dense_depth(int dtype, const void* u11, const float* wprob, const float* depths, float* depth_map, float* conf_map,
                       int v0, int Vc, int B, int D, int H, int W, int classmajor, hipStream_t s);
// depth_points.hip: depth [n][S][S] fp32, Kcrop [n][3][3] / E [n][4][4] fp64 -> world-frame points [n][S][S][3] fp32
int launch_depth_to_points(const float* depth, const double* Kc, const double* E, int n, int S, float* points, hipStream_t s);
// depth_consistency.hip: the two-view check of view a's map [n][S][S] against view b's (conf_a fp32 / mask_a uint8 / reproj / rel may be
// null) -> fused / reproj / rel fp32, keep uint8; and the ordered compaction of the kept pixels of view 1, then view 2 (the view-2
// arguments null together: one view) into cloud [n][cap][3] fp32, index [n][cap] i32 (view * S * S + pixel), count [n][2] i32
int launch_depth_consistency(const float* depth_a, const float* conf_a, const unsigned char* mask_a, const double* Ka, const double* Ea,
                             const float* depth_b, const double* Kb, const double* Eb, int n, int S, double px_max, double rel_max,
                             float conf_min, float* fused, float* reproj, float* rel, unsigned char* keep, hipStream_t s);
int launch_cloud_pack(const float* fused1, const unsigned char* keep1, const double* K1, const double* E1, const float* fused2,
                      const unsigned char* keep2, const double* K2, const double* E2, int n, int S, int cap, float* cloud, int* index,
                      int* count, hipStream_t s);
// depth_fusion.hip: the check over V views of a pose (depth / conf / mask [n][V][S][S], Kcrop [n][V][3][3], E [n][V][4][4]; conf, mask,
// agree may be null) -> fused fp32, keep / nviews uint8, agree uint16; the ordered compaction of the kept pixels of views 0 .. V - 1 into
// cloud [n][cap][3], index [n][cap] (view * S * S + pixel), count [n][V]; and the rows of maps [n][V][S2][C] at such indices
int launch_depth_fusion(const float* depth, const float* conf, const unsigned char* mask, const double* Kc, const double* E, int n, int V,
                        int S, double px_max, double rel_max, float conf_min, int n_min, float* fused, unsigned char* keep,
                        unsigned char* nviews, unsigned short* agree, hipStream_t s);
int launch_cloud_pack_views(const float* fused, const unsigned char* keep, const double* Kc, const double* E, int n, int V, int S, int cap,
                            float* cloud, int* index, int* count, hipStream_t s);
int launch_cloud_gather_views(const float* maps, const int* index, int n, int V, int S2, int C, int cap, float* out, hipStream_t s);
int launch_fuse_points(int dtype, const void* feat, const float* homog, const float* depths, const int* choose,
                       const float* prob, float* out, int V, int B, int P, int D, int H, int W, int ldo, int ch_off,
                       hipStream_t s, int Vn = -1);      // Vn: views 0 .. Vn - 1 only (default: all V)
int launch_mean_points(int dtype, const void* in, float* out, float* scratch, int V, int P, int C, hipStream_t s);      // dtype of `in`: F32 or F16
int launch_f32_to_f16(const float* in, void* out, long long n, hipStream_t s);
// ResNet stem in one kernel (stem.hip): NCHW fp32 images -> maxpool3x3s2(relu(conv7x7s2)) [V][S/4][S/4][64]
void stem_pack(const float* w, std::vector<float>& packed);
int launch_stem(int dtype, const float* img1, const float* img2, const void* wpk, void* out, int B, int V, int S, hipStream_t s);
// the same kernel on V views (any V >= 1) of ONE image array [V][3][S][S]
int launch_stem_views(int dtype, const float* img, const void* wpk, void* out, int V, int S, hipStream_t s);
// feature_cache.hip — records of the PSPNet's feature map in a caller-owned pool.  A record is `record_bytes` long; a part of it
// ([part_off, part_off + part_bytes), all multiples of 16) is copied per launch.  store: view v of `src` ([V][part_bytes]) -> record
// slots[v]; gather: record slot1[b] / slot2[b] -> view b / B + b of `dst` ([2B][part_bytes]).  A slot outside [0, pool_records) is
// neither written nor read: the gather fills the view with zeros and launch_feature_bad_slot_nan turns the pose's outputs into NaN.
int launch_feature_store(const void* src, void* pool, const int* slots, int V, int pool_records, size_t part_off, size_t part_bytes,
                         size_t record_bytes, hipStream_t s);
int launch_feature_gather(const void* pool, void* dst, const int* slot1, const int* slot2, int B, int pool_records, size_t part_off,
                          size_t part_bytes, size_t record_bytes, hipStream_t s);
// out[k]: the k-th output tensor [B][per_pose[k]] fp32
int launch_feature_bad_slot_nan(const int* slot1, const int* slot2, int B, int pool_records, float* const out[10], const int per_pose[10],
                                hipStream_t s);
// content key of V prepared crops of n_words 32-bit words each (include/rgbm.h: rgbm_crop_fingerprint): keys_out [V][2], zeroed here
int launch_crop_fingerprint(const float* img, int V, int n_words, unsigned long long* keys_out, hipStream_t s);
int launch_f32_to_bx3(const float* in, void* out, long long n, hipStream_t s);     // plain fp32 -> split pairs (n % 4 == 0; in place allowed)
int launch_view_linear(const float* x, const float* W, const float* bias, float* out, int V, int I, int O, int ldw, int i0,
                       int relu, hipStream_t s);
// head_kernels.hip: gather + the six per-point layers of the NOCS branch in one launch
struct PointMlpDesc {
  const float* table;      // device: point_mlp_table_floats() floats from point_mlp_pack (weights in MFMA-fragment order, then biases)
  const void* feat;        // [V][HW][32] in the feature map's storage type
  const int* choose;       // [V * P]
  float* nocs4;            // [V * P][4]
  float* pf;               // channel 0 of the 64 output channels, row stride ldpf
  int ldpf, P, HW;
  long long N;             // V * P, a multiple of 64
};
int point_mlp_table_floats();
void point_mlp_pack(const float* const w[6], const float* const b[6], float* table);      // host; w[l]: [Cout][Cin] row-major fp32 of instance_color.0, nocs_head.0/2/4, nocs_pts_mlp.0/2
int launch_point_mlp(int feat_dtype, const PointMlpDesc& d, hipStream_t s);
// the same table's layers 0..3 on every pixel: feat [N][32] (bf16 / f16 / fp32) -> out [N][3] fp32, N % 64 == 0
int launch_dense_nocs(int feat_dtype, const float* table, const void* feat, float* out, long long N, hipStream_t s);
// head_kernels.hip: the pose rows of the real-world network (network_realworld.py:201-209) in one launch.  Row of point p of view v < Vh
// (views [view-1 crops ; view-2 crops] of B poses): channels 0-63 camera_pts_mlp(coor[p][0], coor[p][1], depth[p]), channels 64-127
// nocs_pts_mlp(nocs4[p][0..2]); both Conv1d 3 -> 32 -> 64 with ReLU, fp32, weights in LDS.  coor1 / coor2 [B][P][2] hold x / W, y / H.
constexpr int kPoseRowsMlpFloats = 32 * 4 + 32 + 32 * 64 + 64;      // one MLP: W0 [32][4] (column 3 zero), b0 [32], W1 transposed [32][64], b1 [64]
constexpr int kPoseRowsFloats = 2 * kPoseRowsMlpFloats;             // camera_pts_mlp, then nocs_pts_mlp
void pose_rows_pack(const float* const w[4], const float* const b[4], float* table);      // host; camera_pts_mlp.0 / .2, nocs_pts_mlp.0 / .2 as [Cout][Cin]
int launch_pose_rows(const float* table, const float* nocs4, const float* coor1, const float* coor2, const float* depth, float* rows, int B,
                     int P, int Vh, hipStream_t s);
// v2_head.hip: the per-point plane-sweep head of the v2 network (network_v2.py:152-184) in one launch.  For point p of view v < Vh (views
// [view-1 crops ; view-2 crops] of B poses, partners among all V = 2B): ref + warped at pixel choose[v][p] over the D = 24 planes ->
// volume_conv (BatchNorm folded) -> fuse_conv -> pose_mlp1 -> rows [Vh * P][64] fp32.  fuse64 [Vh * P][64] (fuse_conv's output) and
// planes [Vh * P][24] (volume_conv's) are written when not null.  feat: fp32, bf16 or f16 maps [V][H][W][32]; homog: launch_homography's.
struct V2HeadWeights {         // host fp32, [Cout][Cin] row-major
  const float* vc_w[3];        // volume_conv.{0,1,2}.conv.weight: 16 x 32, 8 x 16, 1 x 8
  const float* vc_scale[3];    // their eval BatchNorm as scale / shift per output channel
  const float* vc_shift[3];
  const float *fc_w[2], *fc_b[2];      // fuse_conv.0 (32 x 24), fuse_conv.2 (64 x 32)
  const float *pm_w[2], *pm_b[2];      // pose_mlp1.0 / .2 (64 x 64)
};
constexpr int kV2HeadFloats = (16 * 32 + 16) + (8 * 16 + 8) + (8 + 4) + (24 * 32 + 32) + (32 * 64 + 64) + 2 * (64 * 64 + 64);
void v2_head_pack(const V2HeadWeights& m, float* table);
int launch_v2_point_rows(int feat_dtype, const float* table, const void* feat, const float* homog, const float* depths, const int* choose,
                         float* rows, float* fuse64, float* planes, int V, int B, int P, int D, int H, int W, int Vh, hipStream_t s);
// v1_head.hip: stage A of the v1 network's heads (network.py:167-177) in one launch.  For point p of view v < Vh (views and partners as
// above): planes = volume_conv(ref + warped) over the D = 24 planes, fused32 = relu(ref + fuse_conv.2(relu(fuse_conv.0(planes)))) ->
// fused32 [Vh * P][32] fp32, and planes [Vh * P][24] when not null.  feat, fused32 and planes 16-byte aligned.
struct V1HeadWeights {         // host fp32, [Cout][Cin] row-major
  const float* vc_w[3];        // volume_conv.{0,1,2}.conv.weight: 16 x 32, 8 x 16, 1 x 8
  const float* vc_scale[3];    // their eval BatchNorm as scale / shift per output channel
  const float* vc_shift[3];
  const float *fc_w[2], *fc_b[2];      // fuse_conv.0 (32 x 24), fuse_conv.2 (32 x 32)
};
constexpr int kV1HeadFloats = (16 * 32 + 16) + (8 * 16 + 8) + (8 + 4) + (24 * 32 + 32) + (32 * 32 + 32);
void v1_head_pack(const V1HeadWeights& m, float* table);
int launch_v1_fused_points(int feat_dtype, const float* table, const void* feat, const float* homog, const float* depths, const int* choose,
                           float* fused32, float* planes, int V, int B, int P, int D, int H, int W, int Vh, hipStream_t s);
// head_kernels.hip: stage B, the six layers of point_mlp_kernel on contiguous fp32 rows x [N][32] (no choose, no map), N % 64 == 0 ->
// nocs4 [N][4] and the pose rows pf [N][128]: channels 0-63 instance_color's output (layer 0), 64-127 nocs_pts_mlp's (layer 5)
int launch_point_mlp_rows(const float* table, const float* x, float* nocs4, float* pf, long long N, hipStream_t s);
// coor[i] = (pts2d[i][0] / W, pts2d[i][1] / H) in IEEE float32 division (interface_realworld.py:264-269), n points
int launch_pts2d_to_coor(const float* pts2d, float* coor, long long n, int W, int H, hipStream_t s);
int launch_ortho6d(const float* r6, float* R, int V, hipStream_t s);
// consumers that finish a mean over points themselves (one launch less per mean): launch_mean_points_partial writes the slices' sums
int launch_mean_points_partial(int dtype, const void* in, float* scratch, int V, int P, int C, hipStream_t s);
int launch_view_linear_mean(const float* partial, int P, float* mean_out, const float* W, const float* bias, float* out, int V, int I, int O,
                            int ldw, int i0, int relu, hipStream_t s);
int launch_pose_heads_mean(const float* partial, int P, float* mean_out, float* R, float* const w[3][3], float* const b[3][3],
                           float* const out[3], const int odim[3], int V, hipStream_t s);
constexpr int kMeanSplit = 8;      // slices of P / kMeanSplit points per view whose sums launch_mean_points_partial writes: [V][kMeanSplit][C]
// pose_mlp.hip: the four per-point layers of the pose MLP of a bf16 net (f16 storage) in two launches.  launch_pose_mlp1: PF96 ->
// pose_mlp1.0 -> pose_mlp1.2 -> q128 + its slices' column sums (part128); launch_pose_mlp2: q128 -> pose_mlp2.0 (+ vbias) -> pose_mlp2.2 ->
// the slices' column sums of the f16-rounded result (part256) only.  Both sums in launch_mean_points_partial's layout.
constexpr int kPoseMlpSlab = 128;      // points a workgroup carries through both layers at a time; a slab never straddles a slice
struct PoseMlpDesc {
  const float* pf96;       // [V * P][96] fp32
  const void* w[4];        // f16 weights [Cout][ldw] of pose_mlp1.0 (96 -> 128), pose_mlp1.2 (128 -> 128), pose_mlp2.0's per-point half (128 -> 256), pose_mlp2.2 (256 -> 256)
  int ldw[4];
  const float* bias[4];    // fp32; bias[2] is not read (vbias holds pose_mlp2.0's)
  const float* vbias;      // [V][256]
  void* q128;              // [V * P][128] f16
  float* part128;          // [V][kMeanSplit][128]
  float* part256;          // [V][kMeanSplit][256]
  int V, P;
};
bool pose_mlp_fits(int P);      // P is a whole number of slabs per slice
int launch_pose_mlp1(const PoseMlpDesc& d, hipStream_t s);
int launch_pose_mlp2(const PoseMlpDesc& d, hipStream_t s);
// the three regression heads (3 x Linear + ReLU each) of every view in one launch; out[h] is [V][odim[h]]
int launch_pose_heads(const float* pf2, float* const w[3][3], float* const b[3][3], float* const out[3], const int odim[3], int V,
                      hipStream_t s);
// input / output staging of AdaPose::forward in one launch each
int launch_stage_in(const float* P1, const float* P2, const int* c1, const int* c2, float* Pviews, int* choose, int B, int P, hipStream_t s);
int launch_stage_out(const float* nocs4, const float* depth, const float* R, const float* tv, const float* sv, float* const nocs[2],
                     float* const dep[2], float* const r[2], float* const t[2], float* const sz[2], int B, int P, int view2, hipStream_t s);
int launch_copy_cols(const float* in, float* out, long long rows, int ldi, int ldo, int n, hipStream_t s);

// conv3d_tile.hip — halo-tiled 3-D conv for the cost-regularisation stack
struct Conv3dTileDesc {
  const void* in; const void* wgt; void* out; const float* bias; const void* res;
  int N, Di, Hi, Wi;            // input tensor [N][Di][Hi][Wi][CIN]
  int Do, Ho, Wo;               // output tensor dims
  int Dq, Hq, Wq;               // tile-enumeration grid (= output dims; = input dims for transposed)
  int ntd, nth, ntw;            // filled by the launcher
  int Cout, relu;
  const void* feat; const float* homog; const float* depths; int v0, V, B;   // fused-warp mode only
  int prof_variant; double algo_flops, algo_bytes;
  int out_classmajor;           // transposed only: write each sub-pixel class as its own dense [N][Dq][Hq][Wq][C] volume
  int feat_f16;      // depth-sweeping conv0 of a bf16 net: `feat` and `wgt` are f16 (AdaPose::feat_f16()), the output stays bf16
  const int* tile_list; const int* tile_count;      // depth-sweeping conv0 only: walk tile_list[0 .. tile_count[0]) instead of all tiles
  int tile_mask_stride;             // bytes between consecutive views' masks (0: nth * ntw)
  int fusion;                       // fused-warp mode and the depth-sweeping conv0: FUSION_* (0 = sum)
  const unsigned char* tile_mask;   // optional [N][nth][ntw]: a workgroup whose (view, row tile, column tile) byte is 0 returns at once (its
                                    // output tile is never read: sparse decoder, see launch_decoder_tile_masks); all depth tiles share a byte
};
// bits of g_debug_flags (rgbm_debug_flags): what each one switches is described in the table at rgbm_debug_flags in include/rgbm.h
enum DebugFlag {
  DBG_NO_WS = 8, DBG_NONUNIFORM_TAPS = 16, DBG_V3_FOR_WS = 64, DBG_NO_WS64 = 128, DBG_NO_ROWHALO = 256, DBG_GENERIC_RESIZE = 512,
  DBG_PSP_STAGE_R5 = 1024, DBG_POINT_MLP_R5 = 2048, DBG_TILE_CONV0 = 4096, DBG_NO_KSPLIT = 16384, DBG_L2_SLIM_TILE = 32768,
  DBG_WS_128x256 = 65536, DBG_NO_SLIM64 = 262144, DBG_KORDER_TAPS_OUTER = 1 << 20, DBG_SWEEP_ALT_BLEND = 1 << 21, DBG_SWEEP_DOT2 = 1 << 22,
  DBG_PP_ONE_KERNEL = 1 << 23, DBG_NO_SLIM_SMALL = 1 << 24, DBG_PP_GENERIC_SELECT = 1 << 25, DBG_PP_GUARD = 1 << 26, DBG_GLOBAL_ADDR = 1 << 27,
  DBG_SWEEP_PER_TILE = 1 << 28, DBG_SPARSE_TAIL_R5 = 1 << 29, DBG_M32_TAILS_R5 = 1 << 30, DBG_POSE_MLP_R6 = 1 << 19, DBG_NO_BORDER_TILES = 32,
};
extern int g_debug_flags;      // the four settings: conv_launch.cpp
extern long long g_ws_min_rows;
extern int g_tuning_version;
extern int g_gemm_kernel;
long long border_launch_count();      // launches of conv_igemm_m32_kernel on border-class tiles since the library was loaded (igemm_m32.hip)
void conv3d_tile_pack(const float* w, const float* scale, int Cin, int Cout, int coutp, bool transposed, int dtype,
                      std::vector<float>& packed);
int launch_conv3d_tile(int layer, int dtype, const Conv3dTileDesc& d, hipStream_t s);
// prob_sparse.hip: sparse cost regularisation — tile masks of every 3-D layer from the chosen pixels' dependency cones, and the
// compacted tile list of the depth-sweeping conv0 (layer ids as launch_conv3d_tile's; 0 = the sweep)
int sparse_mask_bytes_per_view(int S);
int sparse_mask_offset(int S, int layer);
int launch_sparse_masks(const int* choose, int v0, int Vc, int P, int S, unsigned char* masks, int* sweep_list, int* sweep_count,
                        hipStream_t s);
// tile grid of a layer's halo-tile kernel in the given storage type (for sizing Conv3dTileDesc::tile_mask)
int conv3d_tile_dims(int layer, int dtype, int* TD, int* TH, int* TW);

// conv0_sweep.hip — conv0 + fused plane sweep, depth-sweeping producer/consumer kernel (bf16 only)
void conv0_sweep_pack(const float* w, const float* scale, std::vector<float>& packed);
int launch_conv0_sweep(const Conv3dTileDesc& d, int dtype, hipStream_t s);      // dtype BF16 or F16

// conv0_sweep_x3.hip — the same for the BF16X3 mode: fp32 feature map in, split-pair c0 out, three MFMAs per product
int conv0_sweep_x3_upload(const std::vector<float>& packed, void** dev);      // packed: conv0_sweep_pack's fp32 fragment order
int launch_conv0_sweep_x3(const Conv3dTileDesc& d, hipStream_t s);           // d.feat: fp32 [V][H][W][32]; d.wgt: the uploaded array
int launch_bx3_to_f32(const void* in, float* out, long long n, hipStream_t s);   // misc_kernels.hip: split-pair tensor -> plain fp32 (n % 4 == 0)

// prob_sparse.hip — conv11 + skip + prob conv + softmax + depth on the neighbourhoods of the chosen pixels (bf16)
int launch_prob_sparse(const void* u9, const void* c0, const void* w11_packed, const float* bias11, const float* wprob,
                       const int* choose, const float* depths, float* prob, float* depth_out, int v0, int Vc, int B, int P,
                       int D, int H, int W, int dtype, hipStream_t s, const void* w11_taps = nullptr);
// conv11 weights [16][8][27] (x BN scale) -> the nine in-plane-tap A operands of prob_sparse2_kernel, fp32 [9][16][4][8] (prob_sparse.hip)
void prob_sparse_pack(const float* w, const float* scale, std::vector<float>& packed);

// prepare.hip — batched device-side AdaPoseEstimator_v5.prepare_model_input
int launch_prepare_inputs(const float* rgb, const unsigned char* mask, const double* K, const int* frame_map, int N, int H, int W, int S, int P,
                          unsigned seed, float* img, int* choose, float* pts2d, double* Kcrop, int* window, int* valid,
                          unsigned char* small_scratch, hipStream_t s, int frame0 = 0);
// the same on 8-bit frames [M,H,W,3]: byte b is the pixel value fl32(b / 255), everything after the tap load is the float path's
int launch_prepare_inputs_u8(const unsigned char* rgb, const unsigned char* mask, const double* K, const int* frame_map, int N, int H, int W,
                             int S, int P, unsigned seed, float* img, int* choose, float* pts2d, double* Kcrop, int* window, int* valid,
                             unsigned char* small_scratch, hipStream_t s, int frame0 = 0);
// either of the two above (pixel_type 0: float32 frames, 1: 8-bit frames), with (normalize 1) or without (0) the ImageNet mean / std step
int launch_prepare_inputs_opt(const void* rgb, int pixel_type, int normalize, const unsigned char* mask, const double* K, const int* frame_map,
                              int N, int H, int W, int S, int P, unsigned seed, float* img, int* choose, float* pts2d, double* Kcrop,
                              int* window, int* valid, unsigned char* small_scratch, hipStream_t s, int frame0 = 0);
// launch_prepare_inputs_opt with the 1024 points drawn from the frame mask at native resolution inside the crop window and mapped into the
// S x S crop afterwards (interface_v2.py:74-98; prepare.hip choose_native_kernel); img, Kcrop and window are launch_prepare_inputs_opt's
int launch_prepare_inputs_native(const void* rgb, int pixel_type, int normalize, const unsigned char* mask, const double* K, const int* frame_map,
                                 int N, int H, int W, int S, int P, unsigned seed, float* img, int* choose, float* pts2d, double* Kcrop,
                                 int* window, int* valid, unsigned char* small_scratch, hipStream_t s, int frame0 = 0);
// launch_prepare_inputs_opt from crop windows the host has cut out and packed back to back (pix / mask_pix at the element offsets `offset`,
// `window` = the windows mask_window_kernel would derive, valid_in 0 = an empty mask); same img / choose / pts2d / Kcrop / valid, bit for bit
int launch_prepare_inputs_windows(const void* pix, int pixel_type, int normalize, const unsigned char* mask_pix, const long long* offset,
                                  const int* window, const int* valid_in, const double* K, int frame0, int N, int H, int W, int S, int P,
                                  unsigned seed, float* img, int* choose, float* pts2d, double* Kcrop, int* valid, unsigned char* small_scratch,
                                  hipStream_t s);
// dst[i] = min(max(rint(src[i] * 255), 0), 255), NaN -> 0: float frames into an 8-bit view queue (any n, src 4-byte / dst 1-byte aligned)
int launch_quantize_frames(const float* src, unsigned char* dst, size_t n, hipStream_t s);

int launch_umeyama_ransac(const float* nocs, const float* depth, const int* choose, const double* Kc, const double* E1,
                          double* bbox, double* srt, int* valid, int B, int P, int img, unsigned seed, hipStream_t s);

// cloud_fit.hip — per-pixel map look-ups of the packed cloud's rows, and the similarity RANSAC over them (include/rgbm.h)
int launch_cloud_gather(const float* map1, const float* map2, const int* index, int n, int S2, int C, int cap, float* out, hipStream_t s);
size_t cloud_similarity_scratch_bytes(int n, int cap);
int launch_cloud_similarity(const float* nocs, const float* cloud, const int* count, int n, int cap, unsigned seed, double* bbox, double* srt,
                            int* info, int* valid, void* scratch, size_t scratch_bytes, hipStream_t s);

int launch_projection(const double* Kc, const double* E, float* P, int n, hipStream_t s);      // prepare.hip
// pnp.hip — the use_depth: False tail of predict (NOCS matches -> triangulation -> scale -> EPnP-RANSAC -> VVS -> world bbox)
int launch_pnp_ransac(const float* nocs1, const float* pts1, const float* nocs2, const float* pts2, const double* K, const double* E1,
                      const double* E2, double* bbox, double* srt, int* info, int* valid, int B, int P, unsigned seed, hipStream_t s);

// the real-world tail (interface_realworld.py:295-320): scale = ||s1|| in float32, then launch_pnp_ransac's steps from EPnP-RANSAC on
// with view 1's points alone (no NOCS matching, no triangulation); info = {P, RANSAC ok, inliers, hypotheses examined}
int launch_pnp_scaled(const float* nocs1, const float* pts1, const float* s1, const double* K, const double* E1, double* bbox, double* srt,
                      int* info, int* valid, int B, int P, unsigned seed, hipStream_t s);

int launch_mask_extent(const unsigned char* mask, int N, int H, int W, int* ext, int* count, hipStream_t s);

// postproc.hip
int launch_postprocess(const float* nocs, const float* depth, const float* rot, const int* choose, const double* Kc,
                       const double* E1, double* bbox, double* ts_out, int* valid, int B, int P, int img, hipStream_t s,
                       void* scratch = nullptr, size_t scratch_bytes = 0);
// postproc_regressed.hip: the adapose_v4 direct-regression tail (translation and scale from the network's heads, no pair median)
int launch_postprocess_regressed(const float* nocs, const float* rot, const float* tr, const float* sv, const double* E1, double* bbox,
                                 double* ts_out, int* valid, int B, int P, hipStream_t s);
// microbench.hip: achievable-peak probes for bench.py
int launch_microbench_mfma(float* scratch, int iters, int random_operands, double* flops, hipStream_t s);
int microbench_mfma_scratch_floats(int* n);
int launch_microbench_copy(const void* src, void* dst, size_t bytes, hipStream_t s);
size_t postprocess_scratch_bytes(int B);      // device scratch of the split (small-batch) form, per call
int postprocess_slices(int B);                // workgroups per pose the split form would use (1 = one-kernel form)

// ppo_kernels.hip
int launch_gae(int T, int N, const float* rewards, const unsigned char* dones, const float* values, const float* last_values,
               float gamma, float lam, float* returns, float* adv, double* sums, hipStream_t s);
int launch_adv_normalise(long long n_local, float* adv, const double* sums, double count_total, hipStream_t s);

// policy_kernels.hip — PPO actor-critic (flat fp32 parameter vector in the reference's state_dict order)
struct PolicyLayout { int dims[5]; int log_std; int w[2][4]; int b[2][4]; int total; };   // net 0 = actor, 1 = critic
struct PolicyOptState { int t; int n_updates; float lr; float last_kl; float last_norm; float pad_; double sum_surr; double sum_vloss; };
int launch_policy_forward(const float* params, const PolicyLayout& L, int n, int mode, const float* obs, const float* noise,
                          float* actions, float* logp, float* value, float* mu, hipStream_t s);
int policy_partial_floats(const PolicyLayout& L, int n);
int launch_ppo_minibatch(const float* params, const PolicyLayout& L, int n, const float* obs, const float* actions,
                         const float* old_logp, const float* adv, const float* returns, const float* old_values,
                         const float* old_mu, const float* old_sigma, float clip, float vcoef, float ecoef, float* partial,
                         float* grads, hipStream_t s);
// General descriptor (rgbm_policy_desc in rgbm.h): per-net hidden widths, activation id, optional second input for the critic.
constexpr int POLICY_MAX_HIDDEN = 6, POLICY_MAX_WIDTH = 512, POLICY_MAX_ACT = 32;
enum { PACT_ELU = 0, PACT_SELU = 1, PACT_RELU = 2, PACT_LRELU = 3, PACT_TANH = 4, PACT_SIGMOID = 5 };
struct PolicyDesc {
  int obs_dim, state_dim, act_dim, activation, asymmetric;
  int n_hidden[2];
  int hidden[2][POLICY_MAX_HIDDEN];
  int w[2][POLICY_MAX_HIDDEN + 1];
  int b[2][POLICY_MAX_HIDDEN + 1];
  int log_std, total;
};
// These forward to the kernels of the shipped shape when the descriptor is that shape, else run the general kernels.
int launch_policy_forward_ex(const float* params, const PolicyDesc& D, int n, int mode, const float* obs, const float* states,
                             const float* noise, float* actions, float* logp, float* value, float* mu, hipStream_t s);
int ppo_scratch_floats_ex(const PolicyDesc& D, int n, int clipped_vloss, size_t* count);
int launch_ppo_minibatch_ex(const float* params, const PolicyDesc& D, int n, const float* obs, const float* states,
                            const float* actions, const float* old_logp, const float* adv, const float* returns,
                            const float* old_values, const float* old_mu, const float* old_sigma, float clip, float vcoef, float ecoef,
                            int clipped_vloss, float* scratch, float* grads, hipStream_t s);
int launch_ppo_adam(float* params, const float* grads, float* m, float* v, PolicyOptState* st, int total, float inv_world,
                    float max_norm, float desired_kl, float lr_min, float lr_max, int adaptive, hipStream_t s);

}  // namespace rgbm
