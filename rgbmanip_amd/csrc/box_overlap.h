// box_overlap.hip — how far two oriented boxes are from each other as boxes (include/rgbm.h: rgbm_box_agreement,
// rgbm_box_iou_matrix): exact intersection volume and IoU of two parallelepipeds, and the centre, corner, extent and rotation errors.
#pragma once
#include "common.h"

namespace rgbm {

constexpr int kBoxPairsMax = 1 << 24;     // pairs per launch of the agreement kernel
constexpr int kBoxMatrixMax = 64;         // boxes per pose and side of the IoU matrix

struct BoxAgreementOut {
  int* valid;                                                    // [n] i32
  double *iou, *inter_volume, *volume_a, *volume_b;              // [n]
  double *center_dist, *center_delta /*[n][3]*/, *corner_dist;
  double *extent_a, *extent_b, *axis_angle_deg, *axis_fold_deg;  // [n][3]
  double* rot_deg;                                               // [n]
};

// a, b [n][8][3] f64 corners in get_3d_bbox's order, ok_a / ok_b [n] u8 or NULL (every box may count) -> the metrics of pair i =
// (a[i], b[i]), all f64 but valid.  A pair with an unusable box (a non-finite coordinate, volume not > 0, ok = 0): valid 0, NaN elsewhere.
int launch_box_agreement(const double* a, const double* b, const unsigned char* ok_a, const unsigned char* ok_b, int n,
                         const BoxAgreementOut& out, hipStream_t s);
// a [n][P][8][3], b [n][Q][8][3], ok_a [n][P] / ok_b [n][Q] u8 or NULL -> iou [n][P][Q] f64, NaN where either box is unusable
int launch_box_iou_matrix(const double* a, const double* b, const unsigned char* ok_a, const unsigned char* ok_b, int n, int P, int Q,
                          double* iou, hipStream_t s);

}  // namespace rgbm
