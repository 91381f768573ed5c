"""CPU-only: the float64 numpy twins of the sample statistics (`samples.box_stats_ref` / `point_stats_ref`) on hand-made cases, and the
calls `estimate_samples` refuses, on an estimator around a stubbed net (the pattern of tests/test_want_host.py)."""
import types

import numpy as np
import pytest

import samples_cases as cases
from rgbmanip_amd import samples
from rgbmanip_amd.config import ADAPOSE_CFGS, adapose_cfg
from rgbmanip_amd.estimator import AdaPoseEstimator_baseline, AdaPoseEstimator_v4, AdaPoseEstimator_v5

# twin (sequential sums over s) against numpy's own reductions (pairwise / other order) on <= 4 samples of O(1) coordinates: a few
# roundings of 2^-53 relative; 1e-13 leaves two orders of magnitude
ORDER_TOL = 1e-13


def test_box_stats_ref_hand_cases():
    boxes, ok, counts = cases.hand_boxes()
    r = samples.box_stats_ref(boxes, ok)
    assert set(r) == set(samples.BOX_KEYS)
    assert r["count"].dtype == np.int32
    np.testing.assert_array_equal(r["count"], counts)
    for b in (0, 1):
        cnt, mean, std, cmean, ccov, emean, estd = cases.numpy_box_stats(boxes[:, b], ok[:, b])
        assert cnt == counts[b]
        for key, want in (("bbox_mean", mean), ("bbox_std", std), ("center_mean", cmean), ("center_cov", ccov), ("extent_mean", emean),
                          ("extent_std", estd)):
            np.testing.assert_allclose(r[key][b], want, rtol=0, atol=ORDER_TOL * 2.0, err_msg=f"pose {b} {key}")
        assert np.isfinite(r["axis_spread_deg"][b]).all() and (r["axis_spread_deg"][b] > 0).all()
    # the uncounted samples of pose 1 do not leak in: the same statistics from its two counted samples alone
    alone = samples.box_stats_ref(boxes[[1, 3]][:, 1:2], np.ones((2, 1)))
    for key in samples.BOX_KEYS:
        np.testing.assert_array_equal(alone[key][0], r[key][1], err_msg=key)
    for key in samples.BOX_KEYS[1:]:
        assert np.isnan(r[key][2]).all(), key                  # none counted: every statistic is NaN
    # extents are the box's sizes in the order x, y, z
    np.testing.assert_allclose(r["extent_mean"][0], [0.4 + 0.01 * 1.5, 0.3, 0.2], rtol=0, atol=1e-12)


def test_axis_spread_of_a_box_rotated_about_one_axis():
    boxes, ok = cases.rotated_boxes()
    r = samples.box_stats_ref(boxes, ok)
    np.testing.assert_array_equal(r["count"], [4, 4, 4])
    for b in range(3):
        for e in range(3):
            if e == b:
                assert r["axis_spread_deg"][b, e] == 0.0       # that edge is the same vector in every sample: dot product exactly 1
            else:
                # unit vectors and their dot product carry a few roundings of 2^-53; acos at 10 degrees amplifies by 1 / sin = 5.8:
                # about 1e-14 rad = 6e-13 degrees
                assert abs(r["axis_spread_deg"][b, e] - cases.THETA) < 1e-10, (b, e, r["axis_spread_deg"][b, e])
    np.testing.assert_allclose(r["extent_std"], 0.0, atol=1e-15)
    np.testing.assert_allclose(r["center_cov"], 0.0, atol=1e-30)


def test_one_counted_sample_has_zero_spread():
    boxes, ok = cases.single_boxes()
    r = samples.box_stats_ref(boxes, ok)
    np.testing.assert_array_equal(r["count"], [1, 1])
    np.testing.assert_array_equal(r["bbox_mean"][0], boxes[3, 0])
    np.testing.assert_array_equal(r["bbox_mean"][1], boxes[0, 1])
    for key in ("bbox_std", "center_cov", "extent_std", "axis_spread_deg"):
        np.testing.assert_array_equal(r[key], np.zeros_like(r[key]), err_msg=key)


def test_box_stats_ref_refuses_bad_shapes():
    with pytest.raises(ValueError):
        samples.box_stats_ref(np.zeros((65, 1, 8, 3)), np.ones((65, 1)))
    with pytest.raises(ValueError):
        samples.box_stats_ref(np.zeros((2, 1, 8, 2)), np.ones((2, 1)))
    with pytest.raises(ValueError):
        samples.box_stats_ref(np.zeros((2, 3, 8, 3)), np.ones((2, 2)))


def test_point_stats_ref():
    rng = np.random.default_rng(3)
    x = rng.normal(size=(4, 3, 5, 3)).astype(np.float32)
    x[1, 2, 4, 0] = np.nan
    x[2, 0, 0, 1] = np.inf
    mean, std = samples.point_stats_ref(x)
    assert mean.dtype == np.float32 and std.dtype == np.float32 and mean.shape == (3, 5, 3) and std.shape == (3, 5, 3)
    fin = np.isfinite(x).all(axis=0)
    x64 = x.astype(np.float64)
    with np.errstate(invalid="ignore"):
        np.testing.assert_allclose(mean[fin], x64.mean(axis=0)[fin], rtol=2e-7, atol=1e-7)       # one float32 rounding
        np.testing.assert_allclose(std[fin], x64.std(axis=0)[fin], rtol=2e-7, atol=1e-7)
    assert np.isnan(mean[2, 4, 0]) and np.isnan(std[2, 4, 0])                  # NaN propagates
    assert np.isinf(mean[0, 0, 1]) and np.isnan(std[0, 0, 1])                  # inf - inf
    assert fin.sum() == fin.size - 2
    one = samples.point_stats_ref(x[:1])
    np.testing.assert_array_equal(one[0], x[0])
    assert (one[1][np.isfinite(x[0])] == 0).all()


# ---------------------------------------------------------------------------------------------------------------- refusals, no GPU
def _est(cls=AdaPoseEstimator_v5, dropout=0.0, **cfg):
    net = types.SimpleNamespace(options={"view2_heads": 0}, dropout=dropout, dropout_seed=0, device="cpu", feature_bytes=64, arch="v5")
    return cls(None, dict(ADAPOSE_CFGS["adapose_cabinet"], load=False, **cfg), None, net=net)


ARGS = (np.zeros((1, 3, 3)), np.zeros((1, 4, 4, 3), np.float32), np.zeros((1, 4, 4), np.uint8), np.zeros((1, 4, 4)),
        np.zeros((1, 4, 4, 3), np.float32), np.zeros((1, 4, 4), np.uint8), np.zeros((1, 4, 4)))


@pytest.mark.parametrize("method", ["estimate_samples", "estimate_samples_device"])
def test_estimate_samples_refusals(method):
    with pytest.raises(ValueError, match="hip_dropout"):
        getattr(_est(), method)(*ARGS)
    with pytest.raises(ValueError, match="hip_dropout"):
        getattr(_est(AdaPoseEstimator_v4), method)(*ARGS, samples=4)
    with pytest.raises(ValueError, match="hip_feature_cache"):
        getattr(_est(hip_feature_cache=True), method)(*ARGS)
    on = _est(dropout=0.15, hip_dropout=0.15)
    for bad in (0, 65, -1, 2.5):
        with pytest.raises(ValueError, match="samples"):
            getattr(on, method)(*ARGS, samples=bad)
    with pytest.raises(ValueError, match="hip_prepare"):
        getattr(_est(dropout=0.15, hip_dropout=0.15, hip_prepare="host"), method)(*ARGS)


@pytest.mark.parametrize("method", ["estimate_samples", "estimate_samples_device"])
def test_baseline_estimator_has_no_samples(method):
    net = types.SimpleNamespace(options={"view2_heads": 0}, dropout=0.0, dropout_seed=0, device="cpu", feature_bytes=64, arch="baseline")
    est = AdaPoseEstimator_baseline(None, dict(adapose_cfg(load=False, name="adapose_baseline")), None, net=net)
    with pytest.raises(NotImplementedError, match=method):
        getattr(est, method)(*ARGS)


def test_existing_surface_is_untouched():
    """estimate_samples is a method of its own: `estimate` keeps its seven arguments, and v4 inherits the new calls."""
    import inspect
    assert list(inspect.signature(AdaPoseEstimator_v5.estimate).parameters)[1:] == [
        "camera_intrinsic_batch", "rgb1_batch", "view1_mask_batch", "view1_extrinsic_batch", "rgb2_batch", "view2_mask_batch", "view2_extrinsic_batch"]
    assert inspect.signature(AdaPoseEstimator_v5.estimate_samples).parameters["samples"].default == 8
    assert AdaPoseEstimator_v4.estimate_samples is AdaPoseEstimator_v5.estimate_samples
    assert AdaPoseEstimator_v4.estimate_samples_device is AdaPoseEstimator_v5.estimate_samples_device
