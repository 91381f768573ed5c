"""-m gpu: the box agreement kernels of csrc/box_overlap.hip against their float64 numpy twins (rgbmanip_amd/boxes.py), the refusals of
the C entry points, and the two helpers on results of `estimate_cloud_pose_device` and `estimate_samples_device`."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import box_cases as cases  # noqa: E402
from rgbmanip_amd import boxes, synth  # noqa: E402

LENGTH_KEYS = ("inter_volume", "volume_a", "volume_b", "center_dist", "center_delta", "corner_dist", "extent_a", "extent_b")
ANGLE_KEYS = ("iou", "axis_angle_deg", "axis_fold_deg", "rot_deg")


def _big(*arrays):
    return max(float(np.abs(x[np.isfinite(x)]).max()) for x in arrays)


def _assert_agreement(a, b, ok_a=None, ok_b=None):
    """Device against twin: valid exact, the same NaN pattern, values within 1e-10: absolute for iou and the angles, relative to the
    largest coordinate for lengths and volumes (tests/test_gpu_samples.py::_assert_box_stats)."""
    ref = boxes.box_agreement_ref(a, b, ok_a, ok_b)
    got = {k: v.cpu().numpy() for k, v in boxes.box_agreement(a, b, ok_a, ok_b).items()}
    torch.cuda.synchronize()
    big = _big(a, b)
    assert sorted(got) == sorted(boxes.AGREEMENT_KEYS)
    np.testing.assert_array_equal(got["valid"], ref["valid"])
    assert got["valid"].dtype == np.int32
    for k in LENGTH_KEYS + ANGLE_KEYS:
        assert got[k].shape == ref[k].shape and got[k].dtype == np.float64, k
        np.testing.assert_array_equal(np.isnan(got[k]), np.isnan(ref[k]), err_msg=k)
        bound = 1e-10 * (big if k in LENGTH_KEYS else 1.0)
        err = np.nanmax(np.abs(got[k] - ref[k]), initial=0.0)
        print(f"box_agreement n = {len(a)} {k}: max abs err {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (k, err)
    return got


def _assert_matrix(a, b, ok_a=None, ok_b=None):
    ref = boxes.box_iou_matrix_ref(a, b, ok_a, ok_b)
    got = boxes.box_iou_matrix(a, b, ok_a, ok_b).cpu().numpy()
    torch.cuda.synchronize()
    assert got.shape == ref.shape and got.dtype == np.float64
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    err = np.nanmax(np.abs(got - ref), initial=0.0)
    print(f"box_iou_matrix {ref.shape}: max abs err {err:.3e}, {int(np.isnan(ref).sum())} NaN, {int((ref > 1e-3).sum())} overlapping")
    assert err <= 1e-10
    return got


# ------------------------------------------------------------------------------------------------------------------ the agreement kernel
def test_agreement_kernel_on_the_hand_cases():
    named = cases.iou_cases()
    a, b, iou, inter = cases.stacked(named)                  # n = 13: two passes of 5 pairs and a remainder of 3
    got = _assert_agreement(a, b)
    for i, name in enumerate(named):
        assert abs(got["iou"][i] - iou[i]) <= 1e-12 and abs(got["inter_volume"][i] - inter[i]) <= 1e-12, name
    a, b, ok_a, ok_b, valid = cases.unusable_cases()
    got = _assert_agreement(a, b, ok_a, ok_b)
    np.testing.assert_array_equal(got["valid"], valid)
    for k in LENGTH_KEYS + ANGLE_KEYS:
        assert np.isnan(got[k][:3]).all() and np.isfinite(got[k][3]).all(), k
    a, b = cases.rotation_cases()
    got = _assert_agreement(a, b)
    for e in range(3):
        assert abs(got["rot_deg"][e] - cases.THETA) <= 1e-10
        for ax in range(3):
            if ax != e:
                assert abs(got["axis_angle_deg"][e, ax] - cases.THETA) <= 1e-10, (e, ax)


@pytest.mark.parametrize("n", [1, 5, 6, 64, 65])
def test_agreement_kernel_on_golden_and_random_pairs(n):
    """n = 5 pairs fill a wavefront pass, 6 leave a remainder of one, 64 / 65 are 13 passes with remainders of 4 and 0; half of the pairs
    come from the golden file (whose intersection volumes the kernel must reach too), half are seeded pairs with unusable boxes."""
    ga, gb, gi = cases.golden()
    k = (n + 1) // 2
    ra, rb, oka, okb = cases.random_pairs(n - k, seed=n) if n > k else (ga[:0], gb[:0], np.ones(0, np.uint8), np.ones(0, np.uint8))
    a, b = np.concatenate([ga[:k], ra]), np.concatenate([gb[:k], rb])
    ok_a, ok_b = np.concatenate([np.ones(k, np.uint8), oka]), np.concatenate([np.ones(k, np.uint8), okb])
    got = _assert_agreement(a, b, ok_a, ok_b)
    err = np.abs(got["inter_volume"][:k] - gi[:k]) / np.minimum(got["volume_a"][:k], got["volume_b"][:k])
    print(f"n = {n}: kernel against the golden volumes, max {err.max():.3e} of the smaller box")
    assert err.max() <= 1e-10
    if n >= 12:
        assert got["valid"].sum() == n - 4
    # without ok arrays (NULL): only the geometry decides
    got = _assert_agreement(a, b)
    if n >= 12:
        assert got["valid"].sum() == n - 2


# ------------------------------------------------------------------------------------------------------------------ the matrix kernel
@pytest.mark.parametrize("shape", [(2, 3, 5), (1, 64, 64), (3, 7, 1)])
def test_matrix_kernel_equals_the_twin(shape):
    """The smallest mixed shape, the largest P and Q (eight row blocks per pose, 103 passes each), and a single column."""
    n, P, Q = shape
    a, b, ok_a, ok_b = cases.random_sets(n, P, Q, seed=P + Q)
    got = _assert_matrix(a, b, ok_a, ok_b)
    assert np.isnan(got[0, P - 1]).all() and np.isnan(got[n - 1, :, 0]).all()
    assert (got[np.isfinite(got)] >= 0).all() and (got[np.isfinite(got)] <= 1).all() and (got > 0.05).sum() > got.size // 4


def test_self_matrix():
    a, _, ok_a, _ = cases.random_sets(2, 9, 1, seed=4)        # 9 rows: a full row block and a block of one
    ref = boxes.box_iou_matrix_ref(a, None, ok_a)
    got = boxes.box_iou_matrix(a, None, ok_a).cpu().numpy()
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    assert np.nanmax(np.abs(got - ref)) <= 1e-10
    d = np.diagonal(got, axis1=1, axis2=2)
    assert np.isnan(d[0, 8]) and (np.abs(d[1] - 1.0) <= 1e-12).all()
    np.testing.assert_array_equal(got, boxes.box_iou_matrix(a, a, ok_a, ok_a).cpu().numpy())
    # rows of the matrix are the agreement kernel's pairs
    pair = boxes.box_agreement(a[:, 2], a[:, 5], ok_a[:, 2], ok_a[:, 5])["iou"].cpu().numpy()
    np.testing.assert_array_equal(got[:, 2, 5], pair)


def test_two_calls_give_the_same_bytes():
    a, b, ok_a, ok_b = cases.random_pairs(65, seed=7)
    one, two = boxes.box_agreement(a, b, ok_a, ok_b), boxes.box_agreement(a, b, ok_a, ok_b)
    for k in one:
        assert torch.equal(one[k].view(torch.uint8), two[k].view(torch.uint8)), k
    a, b, ok_a, ok_b = cases.random_sets(2, 11, 6, seed=8)
    assert torch.equal(boxes.box_iou_matrix(a, b, ok_a, ok_b).view(torch.uint8), boxes.box_iou_matrix(a, b, ok_a, ok_b).view(torch.uint8))


def test_more_work_than_the_grid_has_workgroups():
    """Both launches are capped at 8192 workgroups and walk the rest with a grid stride: 45 500 pairs are 9100 passes of the agreement
    kernel, 4200 poses of 9 rows are 8400 row blocks of the matrix kernel.  The inputs are the small sets above tiled, so the answer is
    the small answer tiled, bit for bit."""
    a, b, ok_a, ok_b = cases.random_pairs(65, seed=7)
    small = {k: v.cpu().numpy() for k, v in boxes.box_agreement(a, b, ok_a, ok_b).items()}
    t = 700
    big = boxes.box_agreement(np.tile(a, (t, 1, 1)), np.tile(b, (t, 1, 1)), np.tile(ok_a, t), np.tile(ok_b, t))
    for k, v in small.items():
        np.testing.assert_array_equal(big[k].cpu().numpy(), np.tile(v, (t,) + (1,) * (v.ndim - 1)), err_msg=k)
    a, _, ok_a, _ = cases.random_sets(2, 9, 1, seed=4)
    small = boxes.box_iou_matrix(a, None, ok_a).cpu().numpy()
    t = 2100
    big = boxes.box_iou_matrix(np.tile(a, (t, 1, 1, 1)), None, np.tile(ok_a, (t, 1))).cpu().numpy()
    np.testing.assert_array_equal(big, np.tile(small, (t, 1, 1)))


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refused_calls_leave_their_outputs_untouched():
    from rgbmanip_amd import _lib
    lib = _lib.load()
    with pytest.raises(ValueError, match="box_iou_matrix"):
        boxes.box_iou_matrix(np.zeros((1, 65, 8, 3)))
    with pytest.raises(ValueError, match="box_agreement"):
        boxes.box_agreement(np.zeros((2, 8, 3)), np.zeros((3, 8, 3)))
    box = torch.from_numpy(np.tile(cases.corners([1, 1, 1]), (65 * 65, 1, 1))).cuda()
    out = torch.full((65 * 65 * 3,), 7.0, dtype=torch.float64, device="cuda")
    flag = torch.full((64,), 7, dtype=torch.int32, device="cuda")
    p, null, st = _lib.ptr(box), _lib.ptr(None), _lib.stream_ptr()
    outs = [_lib.ptr(out)] * 12
    for n in (0, -1, (1 << 24) + 1):
        assert lib.rgbm_box_agreement(p, p, null, null, n, _lib.ptr(flag), *outs, st) != 0
        assert b"box_agreement" in lib.rgbm_last_error()
    assert lib.rgbm_box_agreement(p, p, null, null, 1, _lib.ptr(flag), *outs[:11], null, st) != 0       # a NULL output
    assert b"box_agreement" in lib.rgbm_last_error()
    assert lib.rgbm_box_agreement(p, null, null, null, 1, _lib.ptr(flag), *outs, st) != 0
    for n, P, Q in ((0, 1, 1), (1, 65, 1), (1, 1, 65), (1, 0, 1), (1 << 30, 2, 1)):
        assert lib.rgbm_box_iou_matrix(p, p, null, null, n, P, Q, _lib.ptr(out), st) != 0
        assert b"box_iou_matrix" in lib.rgbm_last_error()
    assert lib.rgbm_box_iou_matrix(p, p, null, null, 1, 1, 1, null, st) != 0
    assert b"box_iou_matrix" in lib.rgbm_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((flag == 7).all())
    # and the same buffers are written by a call that is accepted
    assert lib.rgbm_box_iou_matrix(p, p, null, null, 1, 2, 2, _lib.ptr(out), st) == 0
    torch.cuda.synchronize()
    assert bool((out[:4] == 1.0).all()) and bool((out[4:] == 7.0).all())


# ------------------------------------------------------------------------------------------------------------------ the helpers
def _scene():
    from test_gpu_cloud import _scene as scene
    return scene()


def _estimator(**kw):
    from test_gpu_cloud import _estimator as estimator, _net
    return estimator(_net(view2_heads=1), hip_view2_heads=True, **kw)


LOOSE = dict(px_max=60.0, rel_max=0.5, conf_min=0.05)       # tests/test_gpu_cloud.py: lets a share of a synthetic net's pixels through


def _close(got, ref, big):
    for k in ref:
        np.testing.assert_array_equal(np.isnan(got[k]), np.isnan(ref[k]), err_msg=k)
        bound = 1e-10 * (big if k in LENGTH_KEYS else 1.0)
        assert np.nanmax(np.abs(got[k] - ref[k]), initial=0.0) <= bound, k


def test_cloud_pose_agreement_on_an_estimator_result():
    s = _scene()
    est = _estimator(hip_ransac_seed=5)
    dev = [torch.from_numpy(s["u1"]).cuda(), torch.from_numpy(s["m1"]).cuda(), torch.from_numpy(s["u2"]).cuda(), torch.from_numpy(s["m2"]).cuda()]
    d = est.estimate_cloud_pose_device(s["K"], dev[0], dev[1], s["E1"], dev[2], dev[3], s["E2"], max_points=6000, **LOOSE)
    before = {k: v.clone() for k, v in d.items()}
    g = boxes.cloud_pose_agreement(d)
    torch.cuda.synchronize()
    assert sorted(g) == sorted(boxes.AGREEMENT_KEYS) and all(isinstance(v, torch.Tensor) and v.is_cuda for v in g.values())
    for k in d:
        assert torch.equal(d[k].view(torch.uint8), before[k].view(torch.uint8)), k
    h = {k: v.cpu().numpy() for k, v in d.items()}
    ref = boxes.box_agreement_ref(h["bbox"], h["bbox_cloud"], h["valid"], h["valid_cloud"])
    got = {k: v.cpu().numpy() for k, v in g.items()}
    np.testing.assert_array_equal(got["valid"], ref["valid"])
    np.testing.assert_array_equal(got["valid"], (h["valid"] != 0) & (h["valid_cloud"] != 0))
    assert got["valid"][1] == 0 and np.isnan(got["iou"][1])      # the pose with the empty mask
    _close(got, ref, _big(h["bbox"], h["bbox_cloud"]))
    print("cloud_pose_agreement: valid", got["valid"].tolist(), "iou", got["iou"].tolist(), "center_dist", got["center_dist"].tolist())
    # a dict of numpy arrays gives numpy arrays with the same bytes
    gh = boxes.cloud_pose_agreement(h)
    for k in got:
        assert isinstance(gh[k], np.ndarray)
        np.testing.assert_array_equal(gh[k], got[k])


def test_samples_overlap_on_an_estimator_result():
    from rgbmanip_amd.config import ADAPOSE_CFGS
    from rgbmanip_amd.estimator import AdaPoseEstimator_v5
    n, S, H, W = 2, 3, 480, 640
    rng = np.random.default_rng(2)
    rgb = rng.random((n, H, W, 3), dtype=np.float32)
    yy, xx = np.mgrid[0:H, 0:W]
    mask = np.zeros((n, H, W), np.uint8)
    mask[0] = (((yy - 250) / 120.0) ** 2 + ((xx - 300) / 170.0) ** 2) < 1.0
    mask[1] = (((yy - 200) / 90.0) ** 2 + ((xx - 350) / 110.0) ** 2) < 1.0
    K = np.tile(np.array([[439.31, 0, 320.0], [0, 439.31, 240.0], [0, 0, 1.0]]), (n, 1, 1))
    inp = synth.adapose_inputs(n, seed=2)
    cfg = dict(ADAPOSE_CFGS["adapose_cabinet"], load=False, hip_prepare="device", hip_dropout=0.15, hip_dropout_seed=11)
    est = AdaPoseEstimator_v5(None, cfg, None, state_dict=synth.adapose_state_dict(seed=0, prefix="module."), dtype="bf16x3")
    cu = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()      # noqa: E731
    d = est.estimate_samples_device(K, cu(rgb), cu(mask), inp["E1"].astype(np.float64), cu(rgb[:, :, ::-1]), cu(mask[:, :, ::-1]),
                                    inp["E2"].astype(np.float64), samples=S)
    g = boxes.samples_overlap(d)
    torch.cuda.synchronize()
    assert sorted(g) == ["iou_mean", "iou_min", "iou_pairs", "iou_to_mean"] and all(v.is_cuda and v.dtype == torch.float64 for v in g.values())
    assert tuple(g["iou_pairs"].shape) == (n, S, S) and tuple(g["iou_to_mean"].shape) == (n, S) and tuple(g["iou_mean"].shape) == (n,)
    h = {k: v.cpu().numpy() for k, v in d.items()}
    ref = boxes.samples_overlap(h, ref=True)
    got = {k: v.cpu().numpy() for k, v in g.items()}
    for k in ref:
        np.testing.assert_array_equal(np.isnan(got[k]), np.isnan(ref[k]), err_msg=k)
        assert np.nanmax(np.abs(got[k] - ref[k]), initial=0.0) <= 1e-10, k
    np.testing.assert_array_equal(h["count"], [S] * n)
    assert np.isfinite(got["iou_pairs"]).all() and (np.abs(np.diagonal(got["iou_pairs"], axis1=1, axis2=2) - 1.0) <= 1e-12).all()
    assert (got["iou_min"] <= got["iou_mean"]).all() and (got["iou_mean"] < 1.0).all() and (got["iou_min"] >= 0.0).all()
    print("samples_overlap: iou_mean", got["iou_mean"].tolist(), "iou_min", got["iou_min"].tolist(), "iou_to_mean", got["iou_to_mean"].tolist())
    gh = boxes.samples_overlap(h)
    for k in got:
        assert isinstance(gh[k], np.ndarray)
        np.testing.assert_array_equal(gh[k], got[k])
