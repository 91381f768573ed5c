"""What the library plans (rgbm_conv_plan, csrc/conv_plan.cpp) for the small launches, and the conv cases of
tests/test_gpu_small_batch.py: the cases must keep reaching every tile, K-part count and residual path of the small launches, so that a
change of the thresholds cannot silently leave a path untested.  CPU only: the plan is asked for 256 CUs, not for a device."""
from gpu_util import KERNEL_M32, KERNEL_M32_SMALL, KERNEL_WS_SLIM, SMALL_CONV_CASES, conv_case_plan, conv_plan

from rgbmanip_amd import _lib

N_CU = 256      # MI355X: 256 CUs, persistent_grid_cus() = 256
DT16 = (_lib.BF16, _lib.F16, _lib.BF16X3)


def _plans():
    return [(c, d, conv_case_plan(c, d, N_CU)) for c in SMALL_CONV_CASES for d in DT16]


def _small(N, Cin, Cout, k, dil=1, res_mode=1, dtype=_lib.BF16):
    """(tile channels, tile pixels, K parts) of a bf16 conv on N 28 x 28 views (M = 784 N GEMM rows, KT = k * k * Cin / 64 K steps), or
    None where the library plans no small launch for it."""
    p = conv_plan(dtype, N, Cin, 28, 28, Cout, k, 1, dil * (k // 2), dil, False, res_mode, 1, N_CU)
    assert p["M"] == 784 * N and p["KT"] == k * k * Cin // 64
    small = p["kernel"] == KERNEL_M32_SMALL or (p["kernel"] == KERNEL_WS_SLIM and Cout > 64)
    return (p["bch"], p["bpix"], p["parts"]) if small else None


def test_plans_match_the_documented_launches():
    # layer3 / layer4 at one pose (igemm_m32.hip; tests/test_gpu_kernels.py::test_conv2d_k_split_is_stable_over_many_runs):
    # M = 1568, KT = 36 / 72: 52 tiles x 4 parts, 104 x 2
    assert _small(2, 256, 256, 3, 2) == (64, 128, 4)
    assert _small(2, 512, 512, 3, 4) == (64, 128, 2)
    # layer2's 128-channel layers at one pose (M = 1568, KT = 18): 64 x 128 tiles of the K-split kernel
    assert _small(2, 128, 128, 3) == (64, 128, 2)
    # enough tiles for the grid (M = 256 * 784, KT = 36): not a small launch
    assert _small(256, 256, 256, 3, 2) is None
    # every part keeps eight K steps: 13 pixel tiles (26 tiles of 64 channels; a conv of 13 such tiles would have 64 output channels and
    # is no small launch) with 15 K steps do not split, with 16 they split in two
    assert _small(2, 15 * 64, 128, 1) == (64, 128, 1)
    assert _small(2, 16 * 64, 128, 1) == (64, 128, 2)
    # no split on 256-channel tiles: 52 of them with 36 K steps (gemm_kernel = 1 puts every small launch on that tile), where the same
    # count of 64-channel tiles splits in four (above)
    lib = _lib.load()
    try:
        _lib.check(lib.rgbm_set_tuning(b"gemm_kernel", 1), "gemm_kernel")
        assert _small(2, 256, 1024, 3, 2) == (256, 128, 1)
    finally:
        lib.rgbm_set_tuning(b"gemm_kernel", 2)


def test_small_batch_cases_reach_every_branch():
    plans = _plans()
    tiles = {p["tile"] for _, _, p in plans}
    assert {(64, 128), (128, 128), (256, 128), (64, 256)} <= tiles, tiles
    parts = {p["parts"] for _, _, p in plans if p["tile"] and p["tile"][1] == 128}
    assert {1, 2, 3, 4} <= parts, parts
    ragged = [c[0] for c, _, p in plans if p["parts"] > 1 and p["KT"] % p["parts"]]
    assert ragged, "no case whose K loop splits into parts of different lengths"
    assert any(c[5] == 128 and c[12] and p["res"] == "epilogue" and p["parts"] > 1 for c, _, p in plans), "Cout = 128 epilogue residual"
    assert any(p["res"] == "identity" and p["parts"] > 1 for _, _, p in plans), "identity-step residual behind a K split"
    assert any(p["res"] == "identity" and p["tile"][0] == bch for _, _, p in plans for bch in (64, 128)), "identity-step residual"
    # the backbone's own shapes keep reaching the split at B = 1 .. 4 (N = 2 .. 8 views)
    assert any(c[0].startswith("l2_conv2_res_n8") and p["parts"] > 1 for c, _, p in plans)
    assert any(c[0].startswith("l3_conv2_res_n2") and p["parts"] == 4 for c, _, p in plans)


def test_debug_flags_steer_the_plan():
    """The switches the small-batch tests rely on.  16384 (no K split): every case plans one part, and the Cout = 128 cases leave the
    64 x 128 tile for the 64 x 256 tile of conv_igemm_ws_kernel - the unsplit reference of test_small_launch_conv_vs_float64.
    1073741824 (round-5 tails): no case plans a 128-pixel small tile."""
    lib = _lib.load()
    try:
        lib.rgbm_debug_flags(16384)
        for c, d, p in _plans():
            assert p["parts"] == 1, (c[0], d, p)
            if c[5] == 128:
                assert p["tile"] == (64, 256), (c[0], d, p)
        lib.rgbm_debug_flags(1 << 30)
        for c, d, p in _plans():
            assert p["tile"] is None or p["tile"][1] != 128, (c[0], d, p)
    finally:
        lib.rgbm_debug_flags(0)


def test_fp32_never_plans_a_small_launch():
    for c in SMALL_CONV_CASES:
        _, N, Cin, H, W, Cout, k, stride, pad, dil, has_bias, act, res_mode = c
        p = conv_plan(_lib.F32, N, Cin, H, W, Cout, k, stride, pad, dil, has_bias, res_mode, act, N_CU)
        assert p["kernel"] not in (KERNEL_M32, KERNEL_M32_SMALL) and p["parts"] == 1, (c[0], p)
