// Who owns the device memory that implicit-GEMM launches depend on: ConvLayer and ConvScratch (rgbmanip_amd/csrc/layers.h) against the
// HIP stand-in (tests/asan/hip_stub.cpp: device memory is host memory, launches do nothing, 256 CUs), which counts the allocations
// alive.  Host-only, its own main; built and run by tests/test_conv_scratch_host.py.  Exit status 0 = every check held.
#include <stdio.h>

#include <memory>
#include <vector>

#include "adapose.h"      // last_error_cstr
#include "kernels.h"      // border_launch_count
#include "layers.h"

extern "C" long long hip_stub_live_allocations(void);
extern "C" void hip_stub_set_capturing(hipStream_t s, int on);

using namespace rgbm;

#define CHECK(cond)                                                                                                          \
  do {                                                                                                                       \
    if (!(cond)) {                                                                                                           \
      fprintf(stderr, "FAILED line %d: %s  (live allocations %lld, last error \"%s\")\n", __LINE__, #cond, live(), last_error_cstr()); \
      return 1;                                                                                                              \
    }                                                                                                                        \
  } while (0)

static long long live() { return hip_stub_live_allocations(); }

// never dereferenced (the stand-in's launches do nothing); 16-byte aligned like every tensor the layers see
alignas(16) static char g_in[16], g_out[16], g_res[16];
static hipStream_t stream(int i) { static char handles[4]; return reinterpret_cast<hipStream_t>(&handles[i]); }

// 3 x 3, stride 1, pad = dilation, no bias, ReLU, bf16
static int make_layer(ConvLayer& L, int C, int dil, const std::shared_ptr<ConvScratch>& scratch) {
  ConvGeom g;
  g.Cin = g.Cout = C; g.KH = g.KW = 3; g.ph = g.pw = g.dilh = g.dilw = dil; g.act = ACT_RELU;
  const std::vector<float> w((size_t)C * C * 9, 0.01f);
  return L.init(BF16, g, w.data(), nullptr, nullptr, nullptr, C, C, scratch);
}
static int run(const ConvLayer& L, int views, bool residual, hipStream_t s) {
  return L.run(g_in, g_out, views, 1, 28, 28, L.Cout_pad, residual ? g_res : nullptr, RES_PRE_ACT, nullptr, 0, s);
}

int main() {
  const hipStream_t A = stream(0), B = stream(1), C = stream(2), D = stream(3);
  const long long before = live();
  {
    auto s1 = std::make_shared<ConvScratch>();
    // tests/test_small_batch_dispatch.py: at 256 CUs and 2 views of 28 x 28 these two run on 128-pixel tiles with their K loop in 4 and 2 parts
    ConvLayer l3, l2;
    CHECK(make_layer(l3, 256, 2, s1) == 0 && make_layer(l2, 128, 1, s1) == 0);
    const long long weights = live();
    CHECK(weights == before + 2);

    // 1. both layers on stream A: one scratch pair (partial sums, counters) and one identity (l3's pre-activation residual); the
    //    second run of either adds nothing; stream B adds a pair of its own and no second identity
    CHECK(run(l3, 2, true, A) == 0 && run(l2, 2, false, A) == 0);
    CHECK(live() == weights + 3);
    CHECK(run(l3, 2, true, A) == 0 && run(l2, 2, false, A) == 0);
    CHECK(live() == weights + 3);
    CHECK(run(l3, 2, true, B) == 0 && run(l2, 2, false, B) == 0);
    CHECK(live() == weights + 5);
    ConvScratch::KSplit a1, b1, a1_again;
    CHECK(s1->ksplit(A, false, &a1) == 0 && s1->ksplit(B, false, &b1) == 0 && s1->ksplit(A, false, &a1_again) == 0);
    CHECK(a1.scratch && a1.count && b1.scratch && b1.count && a1.scratch != b1.scratch && a1.count != b1.count);
    CHECK(a1.scratch == a1_again.scratch && a1.count == a1_again.count);

    // 2. a second ConvScratch on stream A hands out buffers of its own
    auto s2 = std::make_shared<ConvScratch>();
    ConvLayer m3;
    CHECK(make_layer(m3, 256, 2, s2) == 0);
    CHECK(run(m3, 2, true, A) == 0);
    CHECK(live() == weights + 5 + 1 + 3);
    ConvScratch::KSplit a2;
    const void *i1 = nullptr, *i2 = nullptr;
    CHECK(s2->ksplit(A, false, &a2) == 0 && s1->identity(BF16, &i1) == 0 && s2->identity(BF16, &i2) == 0);
    CHECK(a2.scratch && a2.scratch != a1.scratch && a2.count != a1.count && i1 && i2 && i1 != i2);
    CHECK(live() == weights + 9);

    // 3. (first half) a border shape: 86 views = 263 pixel tiles of 256, of which 256 run as the main launch on border-class tiles
    //    from the layer's table (one allocation, made once); the other 1888 rows run unsplit on 128-pixel tiles
    const long long launches = border_launch_count();
    CHECK(run(m3, 86, true, A) == 0);
    CHECK(live() == weights + 10 && border_launch_count() == launches + 1);
    CHECK(run(m3, 86, true, A) == 0);
    CHECK(live() == weights + 10 && border_launch_count() == launches + 2);

    // 4. a stream that is being captured before it has scratch: the launch succeeds and allocates nothing; once the capture is over
    //    the next launch allocates.  The same for a border table: row-major tiles inside the capture, the table after it.
    hip_stub_set_capturing(C, 1);
    CHECK(run(l3, 2, true, C) == 0 && run(l2, 2, false, C) == 0);
    ConvScratch::KSplit c1;
    CHECK(s1->ksplit(C, false, &c1) == 0 && !c1.scratch && !c1.count);
    CHECK(live() == weights + 10);
    CHECK(run(l3, 2, true, A) == 0 && live() == weights + 10);      // (other streams are not being captured, and have theirs)
    hip_stub_set_capturing(C, 0);
    CHECK(run(l3, 2, true, C) == 0);
    CHECK(live() == weights + 12);
    CHECK(s1->ksplit(C, false, &c1) == 0 && c1.scratch && c1.scratch != a1.scratch && c1.scratch != b1.scratch);

    hip_stub_set_capturing(D, 1);
    const long long row_major = border_launch_count();
    CHECK(run(l3, 86, true, D) == 0);      // l3 has no table yet (its identity exists: step 1)
    CHECK(live() == weights + 12 && border_launch_count() == row_major);
    hip_stub_set_capturing(D, 0);
    CHECK(run(l3, 86, true, D) == 0);
    CHECK(live() == weights + 13 && border_launch_count() == row_major + 1);
    hip_stub_set_capturing(D, 1);          // the table is there now: a capture uses it
    CHECK(run(l3, 86, true, D) == 0);
    CHECK(live() == weights + 13 && border_launch_count() == row_major + 2);
    hip_stub_set_capturing(D, 0);

    // a layer without a scratch refuses the launches that need one, and runs the others
    ConvLayer bare;
    CHECK(make_layer(bare, 256, 2, nullptr) == 0);
    CHECK(run(bare, 2, true, A) != 0);
    CHECK(run(bare, 86, false, A) == 0);
  }
  // 3. layers and scratches gone: weights, scratch pairs, identities and border tables with them
  CHECK(live() == before);
  printf("CONV_SCRATCH_OK\n");
  return 0;
}
