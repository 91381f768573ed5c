// The cost-regularisation net (network_v5.py CostRegNet) described once: the ten 3-D layers in the halo-tile kernel's layer-id order,
// 0..6 = conv0..conv6, 7..9 = conv7 / conv9 / conv11.  Host only.  What builds the layers (AdaPose::create_cost), sizes their outputs
// (AdaPose::plan), walks them (AdaPose::cost_volume) and taps them (capi.cpp) reads this table; the kernel side's own table
// (conv3d_tile_table.h) is checked against it below.
#pragma once
#include <stddef.h>

namespace rgbm {

struct Cost3dLayer {
  const char* name;      // state-dict name below "cost_regularization."
  int cin, cout;
  int stride;            // of the module: 2 for the transposed layers (ConvTranspose3d k3 s2 p1 op1)
  bool transposed;
  int in_div;            // the input grid is (D, S, S) / in_div
  int skip;              // row whose output is added behind the ReLU (network_v5.py:287-289), -1: none
};

constexpr int kCost3dLayers = 10;
constexpr Cost3dLayer kCost3d[kCost3dLayers] = {
    {"conv0", 32, 8, 1, false, 1, -1},  {"conv1", 8, 16, 2, false, 1, -1},  {"conv2", 16, 16, 1, false, 2, -1}, {"conv3", 16, 32, 2, false, 2, -1},
    {"conv4", 32, 32, 1, false, 4, -1}, {"conv5", 32, 64, 2, false, 4, -1}, {"conv6", 64, 64, 1, false, 8, -1}, {"conv7", 64, 32, 2, true, 8, 4},
    {"conv9", 32, 16, 2, true, 4, 2},   {"conv11", 16, 8, 2, true, 2, 0}};

// output channels as the halo-tile kernel pads them (weights and bias; the tensor itself holds cout)
constexpr int cost3d_coutp(int l) { return kCost3d[l].cout < 16 ? 16 : kCost3d[l].cout; }
// the output grid is (D, S, S) / cost3d_out_div(l)
constexpr int cost3d_out_div(int l) { return kCost3d[l].transposed ? kCost3d[l].in_div / kCost3d[l].stride : kCost3d[l].in_div * kCost3d[l].stride; }
// elements of layer l's output for Vc views (D and S multiples of 8)
constexpr size_t cost3d_out_elems(int l, int Vc, int D, int S) {
  return (size_t)Vc * ((size_t)D * S * S / ((size_t)cost3d_out_div(l) * cost3d_out_div(l) * cost3d_out_div(l))) * kCost3d[l].cout;
}

// every layer reads what the one before it writes, and a skip tensor has the shape of the output it is added to
constexpr bool cost3d_chain_ok() {
  for (int l = 1; l < kCost3dLayers; ++l) {
    if (kCost3d[l].cin != kCost3d[l - 1].cout || kCost3d[l].in_div != cost3d_out_div(l - 1)) return false;
    const int k = kCost3d[l].skip;
    if (k >= 0 && (k >= l || kCost3d[k].cout != kCost3d[l].cout || cost3d_out_div(k) != cost3d_out_div(l))) return false;
  }
  return kCost3d[0].in_div == 1 && cost3d_out_div(kCost3dLayers - 1) == 1;
}
static_assert(cost3d_chain_ok(), "cost-regularisation table: a layer's input is not its predecessor's output, or a skip tensor does not fit");

// the kernel side: input channels, padded output channels, stride over the output positions a tile walks (the input grid q of a
// transposed layer, so 1 there) and the transposed flag of every layer id; id 10 is conv0 with the plane sweep fused in
#define C3_CASE(L, CIN, COUTP, TDB, THB, TWB, TDF, THF, TWF, STRIDE, TR, WARP, WCB, WCF)                                                 \
  static_assert(kCost3d[(L) == 10 ? 0 : (L)].cin == (CIN) && cost3d_coutp((L) == 10 ? 0 : (L)) == (COUTP) &&                             \
                    (kCost3d[(L) == 10 ? 0 : (L)].transposed ? 1 : kCost3d[(L) == 10 ? 0 : (L)].stride) == (STRIDE) &&                   \
                    kCost3d[(L) == 10 ? 0 : (L)].transposed == (TR),                                                                     \
                "conv3d_tile_table.h and cost3d.h disagree about layer " #L);
#include "conv3d_tile_table.h"
#undef C3_CASE

}  // namespace rgbm
