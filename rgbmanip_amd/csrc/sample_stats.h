// sample_stats.hip — what the estimator makes of S Dropout2d samples per pose (include/rgbm.h: rgbm_sample_box_stats,
// rgbm_sample_point_stats), and the row tiling AdaPose::forward_samples stages its per-pose inputs with.
#pragma once
#include "common.h"

namespace rgbm {

constexpr int kSampleMax = 64;            // samples per pose of the box statistics (one lane of a wavefront each)
constexpr int kSampleBoxPoses = 65535;    // poses per launch of the box statistics

// boxes [S][n][8][3] f64, ok [S][n] u8 -> per pose, over the counted samples (ok set, 24 finite coordinates) in ascending s:
// count [n] i32, bbox_mean / bbox_std [n][8][3], center_mean [n][3], center_cov [n][3][3], extent_mean / extent_std [n][3],
// axis_spread_deg [n][3] (all f64; edges in the order x, y, z of the box frame: corner 0 -> corners 2, 4, 1 of get_3d_bbox)
int launch_sample_box_stats(const double* boxes, const unsigned char* ok, int n, int S, int* count, double* bbox_mean, double* bbox_std,
                            double* center_mean, double* center_cov, double* extent_mean, double* extent_std, double* axis_spread_deg,
                            hipStream_t s);
// x [S][n][M] f32 -> mean / std [n][M] f32: per element over s ascending, two passes in f64, one rounding; NaN propagates
int launch_sample_point_stats(const float* x, int n, int S, long long M, float* mean, float* std, hipStream_t s);
// dst [S][words] = src [words] repeated S times (4-byte words)
int launch_tile_words(const void* src, void* dst, long long words, int S, hipStream_t s);

}  // namespace rgbm
