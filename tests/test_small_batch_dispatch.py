"""The small-batch dispatch mirror (tests/gpu_util.py::small_launch_plan) and the conv cases of tests/test_gpu_small_batch.py: the
cases must keep reaching every tile, K-part count and residual path of the small launches, so that a change of the thresholds
cannot silently leave a path untested.  CPU only."""
from gpu_util import SMALL_CONV_CASES, conv_case_plan, m32_ksplit_choice, small_launch_plan

from rgbmanip_amd import _lib

N_CU = 256      # MI355X: 256 CUs, persistent_grid_cus() = 256


def _plans():
    return [(c, d, conv_case_plan(c, d, N_CU)) for c in SMALL_CONV_CASES for d in (_lib.BF16, _lib.F16, _lib.BF16X3)]


def test_mirror_matches_the_documented_launches():
    # layer3 / layer4 at one pose (conv_igemm_m32.inc; tests/test_gpu_kernels.py::test_conv2d_k_split_is_stable_over_many_runs):
    # 52 tiles x 4 parts, 104 x 2
    assert small_launch_plan(1568, 256, 36, N_CU) == (64, 128, 4)
    assert small_launch_plan(1568, 512, 72, N_CU) == (64, 128, 2)
    # layer2's 128-channel layers at one pose: 64 x 128 tiles of the K-split kernel
    assert small_launch_plan(1568, 128, 18, N_CU) == (64, 128, 2)
    # enough tiles for the grid: not a small launch; fp32-sized K loops too short to split
    assert small_launch_plan(256 * 784, 256, 36, N_CU) is None
    assert m32_ksplit_choice(15, 13, N_CU, 64) == 1
    assert m32_ksplit_choice(16, 13, N_CU, 64) == 2
    assert m32_ksplit_choice(36, 52, N_CU, 256) == 1          # no split on 256-channel tiles


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
