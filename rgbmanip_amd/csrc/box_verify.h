// box_verify.hip — how well a box agrees with the evidence it was computed from (include/rgbm.h: rgbm_box_silhouette,
// rgbm_cloud_in_box): the silhouette of S boxes against V masks, and the share of a packed cloud a box contains.
#pragma once
#include "common.h"

namespace rgbm {

constexpr int kVerifyBoxesMax = 64;            // boxes per pose
constexpr int kVerifyViewsMax = 16;            // views per pose
constexpr int kVerifyRecordsMax = 1 << 24;     // n * S * V per launch
constexpr int kVerifyCountColsMax = 16;        // columns of a cloud's count

struct BoxSilhouetteOut {
  int *area_box, *inter;      // [n][S][V]
  int* area_mask;             // [n][V]
  int* rect;                  // [n][S][V][4]
  int* flags;                 // [n][S][V]
};

// bytes of the scratch launch_box_silhouette needs: one record and one pixel bound per (pose, view, box)
size_t box_silhouette_scratch_bytes(int n, int S, int V);
// boxes [n][S][8][3] f64 world frame, ok [n][S] u8 or NULL, K [n][V][3][3], E [n][V][4][4] f64, mask [n][V][H][W] u8
int launch_box_silhouette(const double* boxes, const unsigned char* ok, const double* K, const double* E, const unsigned char* mask, int n,
                          int S, int V, int H, int W, const BoxSilhouetteOut& out, void* scratch, size_t scratch_bytes, hipStream_t s);
// cloud [n][cap][3] f32, count [n][count_cols] i32, boxes [n][S][8][3] f64, ok [n][S] u8 or NULL -> inside [n][S], total [n] i32
int launch_cloud_in_box(const float* cloud, const int* count, int count_cols, const double* boxes, const unsigned char* ok, int n, int S,
                        int cap, double inflate, int* inside, int* total, hipStream_t s);

}  // namespace rgbm
