"""CPU: the float64 numpy twins of the box agreement (rgbmanip_amd/boxes.py) on hand cases with analytic answers and against the
intersection volumes that scipy gave for tests/golden/box_overlap.npz (tools/make_box_overlap_golden.py); the refusals; the two
helpers on hand-made result dicts through the twins."""
import numpy as np
import pytest

import box_cases as cases
from rgbmanip_amd import boxes
from rgbmanip_amd.cloud import DEFAULT_BBOX
from samples_cases import corners, rot

TOL = 1e-12      # the twins against the analytic values of the hand cases, angles in degrees included


def test_hand_cases_have_their_analytic_values():
    named = cases.iou_cases()
    a, b, iou, inter = cases.stacked(named)
    r = boxes.box_agreement_ref(a, b)
    np.testing.assert_array_equal(r["valid"], 1)
    for i, name in enumerate(named):
        print(f"{name}: iou {r['iou'][i]!r} (want {iou[i]!r}), inter {r['inter_volume'][i]!r}")
        assert abs(r["iou"][i] - iou[i]) <= 1e-12, name
        assert abs(r["inter_volume"][i] - inter[i]) <= 1e-12, name
    i = list(named).index("half turn")
    # a half turn about x: the unit-edge dot products are exactly 1, -1, -1 (a sign flip is exact), so nothing sits beside acos' edge
    print(f"half turn: axis_angle_deg {r['axis_angle_deg'][i].tolist()}, axis_fold_deg {r['axis_fold_deg'][i].tolist()}")
    np.testing.assert_allclose(r["axis_angle_deg"][i], [0.0, 180.0, 180.0], rtol=0, atol=TOL)
    np.testing.assert_allclose(r["axis_fold_deg"][i], [0.0, 0.0, 0.0], rtol=0, atol=TOL)
    assert abs(r["rot_deg"][i] - 180.0) <= TOL
    i = list(named).index("mirrored against itself")
    assert abs(r["volume_a"][i] - 1.0) <= 1e-12 and r["center_dist"][i] <= 1e-12


def test_shifts_along_a_face_normal():
    a, b, iou = cases.shift_cases()
    r = boxes.box_agreement_ref(a, b)
    print("shift errors", (r["iou"] - iou).tolist())
    assert (np.abs(r["iou"] - iou) <= 1e-12).all()


def test_unusable_boxes_give_nan_and_valid_0():
    a, b, ok_a, ok_b, valid = cases.unusable_cases()
    r = boxes.box_agreement_ref(a, b, ok_a, ok_b)
    np.testing.assert_array_equal(r["valid"], valid)
    assert r["valid"].dtype == np.int32
    for k in boxes.AGREEMENT_KEYS[1:]:
        assert np.isnan(r[k][:3]).all() and np.isfinite(r[k][3]).all(), k
    assert abs(r["iou"][3] - 1.0 / 3.0) <= 1e-12


def test_pose_errors_of_known_rotations():
    a, b = cases.rotation_cases()
    r = boxes.box_agreement_ref(a, b)
    for e in range(3):
        for ax in range(3):
            want = 0.0 if ax == e else cases.THETA
            print(f"turn about axis {e}: axis_angle_deg[{ax}] = {r['axis_angle_deg'][e, ax]!r} (want {want})")
            assert abs(r["axis_angle_deg"][e, ax] - want) <= TOL, (e, ax, r["axis_angle_deg"][e, ax])
        assert abs(r["rot_deg"][e] - cases.THETA) <= TOL, (e, r["rot_deg"][e])
    np.testing.assert_allclose(r["axis_fold_deg"], np.minimum(r["axis_angle_deg"], 180 - r["axis_angle_deg"]), rtol=0, atol=0)
    np.testing.assert_allclose(r["extent_a"], np.tile([0.5, 0.3, 0.2], (3, 1)), rtol=0, atol=1e-12)
    np.testing.assert_allclose(r["extent_b"], r["extent_a"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(r["center_delta"], np.tile([0.01, 0.02, -0.03], (3, 1)), rtol=0, atol=1e-12)
    np.testing.assert_allclose(r["center_dist"], np.sqrt(0.0014), rtol=0, atol=1e-12)
    assert (r["iou"] > 0.3).all() and (r["iou"] < 1.0).all()
    # corner_dist against numpy's own norm
    np.testing.assert_allclose(r["corner_dist"], np.linalg.norm(a - b, axis=2).mean(axis=1), rtol=0, atol=1e-12)
    # an obtuse angle folds: the box turned by 180 - 25 degrees
    c = corners([0.5, 0.3, 0.2], rot(2, 155.0))[None]
    f = boxes.box_agreement_ref(corners([0.5, 0.3, 0.2])[None], c)
    np.testing.assert_allclose(f["axis_angle_deg"][0], [155.0, 155.0, 0.0], rtol=0, atol=TOL)
    np.testing.assert_allclose(f["axis_fold_deg"][0], [25.0, 25.0, 0.0], rtol=0, atol=TOL)


def test_twin_matches_the_golden_intersection_volumes():
    """|inter - golden| <= 1e-10 of the smaller box's volume (the project's fp64 bound between a kernel-order computation and an
    independent one); observed 2.3e-15."""
    a, b, want = cases.golden()
    assert len(a) >= 200
    r = boxes.box_agreement_ref(a, b)
    np.testing.assert_array_equal(r["valid"], 1)
    small = np.minimum(r["volume_a"], r["volume_b"])
    err = np.abs(r["inter_volume"] - want) / small
    iou = want / (r["volume_a"] + r["volume_b"] - want)
    print(f"golden: {len(a)} pairs, {(iou > 1e-3).sum()} overlapping, max |inter - golden| / min volume = {err.max():.3e}")
    assert (iou > 1e-3).sum() * 2 >= len(a) and (iou > 0.5).sum() >= 20
    assert err.max() <= 1e-10
    assert (np.abs(r["iou"] - iou) <= 1e-10).all()


def test_iou_is_symmetric():
    a, b, _ = cases.golden()
    ha, hb, _, _ = cases.stacked(cases.iou_cases())
    a, b = np.concatenate([a, ha]), np.concatenate([b, hb])
    d = np.abs(boxes.box_agreement_ref(a, b)["iou"] - boxes.box_agreement_ref(b, a)["iou"])
    print(f"max |iou(a,b) - iou(b,a)| = {d.max():.3e}")
    assert d.max() <= 1e-12


def test_matrix_twin_equals_the_pairwise_twin():
    a, b, ok_a, ok_b = cases.random_sets(2, 3, 5, seed=3)
    m = boxes.box_iou_matrix_ref(a, b, ok_a, ok_b)
    assert m.shape == (2, 3, 5) and m.dtype == np.float64
    for p in range(3):
        for q in range(5):
            want = boxes.box_agreement_ref(a[:, p], b[:, q], ok_a[:, p], ok_b[:, q])["iou"]
            np.testing.assert_array_equal(m[:, p, q], want)
    assert np.isnan(m[0, 2]).all() and np.isnan(m[0, :, 1]).all() and np.isnan(m[1, :, 0]).all() and np.isfinite(m[1, :, 1:]).all()
    s = boxes.box_iou_matrix_ref(a, None, ok_a)
    np.testing.assert_array_equal(s, boxes.box_iou_matrix_ref(a, a, ok_a, ok_a))
    assert (np.abs(np.diagonal(s, axis1=1, axis2=2)[1] - 1.0) <= 1e-12).all()


def test_refusals_name_the_function():
    z = np.zeros((2, 8, 3))
    with pytest.raises(ValueError, match="box_agreement_ref"):
        boxes.box_agreement_ref(np.zeros((2, 8, 2)), z)
    with pytest.raises(ValueError, match="box_agreement_ref"):
        boxes.box_agreement_ref(z, np.zeros((3, 8, 3)))
    with pytest.raises(ValueError, match="box_agreement_ref"):
        boxes.box_agreement_ref(np.zeros((0, 8, 3)), np.zeros((0, 8, 3)))
    with pytest.raises(ValueError, match="box_agreement_ref: ok_a"):
        boxes.box_agreement_ref(z, z, np.ones(3))
    with pytest.raises(ValueError, match="box_iou_matrix_ref"):
        boxes.box_iou_matrix_ref(np.zeros((1, 65, 8, 3)))
    with pytest.raises(ValueError, match="box_iou_matrix_ref"):
        boxes.box_iou_matrix_ref(np.zeros((1, 2, 8, 3)), np.zeros((2, 2, 8, 3)))
    with pytest.raises(ValueError, match="box_iou_matrix_ref"):
        boxes.box_iou_matrix_ref(np.zeros((1, 0, 8, 3)))
    with pytest.raises(ValueError, match="box_iou_matrix_ref: ok_b"):
        boxes.box_iou_matrix_ref(np.zeros((1, 2, 8, 3)), np.zeros((1, 3, 8, 3)), None, np.ones((1, 2)))
    with pytest.raises(ValueError, match="cloud_pose_agreement"):
        boxes.cloud_pose_agreement({"bbox": z}, ref=True)
    with pytest.raises(ValueError, match="samples_overlap"):
        boxes.samples_overlap({"bbox": z}, ref=True)


def test_cloud_pose_agreement_on_a_hand_made_result():
    cube = corners([1, 1, 1], t=cases.T0)
    r = {"bbox": np.stack([cube, cube, cube]), "bbox_cloud": np.stack([corners([1, 1, 1], t=cases.T0 + [0.5, 0, 0]), DEFAULT_BBOX, cube]),
         "valid": np.array([1, 1, 0], dtype=np.int32), "valid_cloud": np.array([1, 0, 1], dtype=np.int32), "cloud": np.zeros((3, 4, 3))}
    g = boxes.cloud_pose_agreement(r, ref=True)
    assert sorted(g) == sorted(boxes.AGREEMENT_KEYS)
    np.testing.assert_array_equal(g["valid"], [1, 0, 0])
    assert abs(g["iou"][0] - 1.0 / 3.0) <= 1e-12 and abs(g["center_dist"][0] - 0.5) <= 1e-12 and np.isnan(g["iou"][1:]).all()
    want = boxes.box_agreement_ref(r["bbox"], r["bbox_cloud"], r["valid"], r["valid_cloud"])
    for k in g:
        np.testing.assert_array_equal(g[k], want[k])


def test_samples_overlap_on_a_hand_made_result():
    """n = 3, S = 3: pose 0 with three shifted cubes; pose 1 with one usable sample (a default box and a NaN sample beside it); pose 2
    with none."""
    cube = lambda dx: corners([1, 1, 1], t=cases.T0 + [dx, 0, 0])      # noqa: E731
    bad = cube(0.0).copy()
    bad[3, 1] = np.nan
    samples = np.stack([np.stack([cube(0.0), cube(0.5), cube(0.25)]), np.stack([DEFAULT_BBOX, cube(0.0), bad]), np.stack([DEFAULT_BBOX] * 3)])
    r = {"bbox_samples": samples, "bbox": np.stack([cube(0.25), cube(0.0), DEFAULT_BBOX]), "valid": np.array([1, 1, 0], dtype=np.int32)}
    g = boxes.samples_overlap(r, ref=True)
    assert sorted(g) == ["iou_mean", "iou_min", "iou_pairs", "iou_to_mean"]
    assert g["iou_pairs"].shape == (3, 3, 3) and g["iou_to_mean"].shape == (3, 3) and g["iou_mean"].shape == (3,) and g["iou_min"].shape == (3,)
    iou = lambda s: (1 - s) / (1 + s)      # noqa: E731
    want = np.array([[1.0, iou(0.5), iou(0.25)], [iou(0.5), 1.0, iou(0.25)], [iou(0.25), iou(0.25), 1.0]])
    np.testing.assert_allclose(g["iou_pairs"][0], want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(g["iou_to_mean"][0], [iou(0.25), iou(0.25), 1.0], rtol=0, atol=1e-12)
    assert abs(g["iou_mean"][0] - (iou(0.5) + 2 * iou(0.25)) / 3) <= 1e-12 and abs(g["iou_min"][0] - iou(0.5)) <= 1e-12
    # one usable sample: it overlaps itself and the mean box, and there is no pair to average
    keep = np.zeros((3, 3), dtype=bool)
    keep[1, 1] = True
    assert np.isnan(g["iou_pairs"][1][~keep]).all() and abs(g["iou_pairs"][1, 1, 1] - 1.0) <= 1e-12
    assert np.isnan(g["iou_to_mean"][1, [0, 2]]).all() and abs(g["iou_to_mean"][1, 1] - 1.0) <= 1e-12
    assert np.isnan(g["iou_mean"][1:]).all() and np.isnan(g["iou_min"][1:]).all()
    assert np.isnan(g["iou_pairs"][2]).all() and np.isnan(g["iou_to_mean"][2]).all()
    np.testing.assert_array_equal(g["iou_pairs"], boxes.box_iou_matrix_ref(samples, None, np.array([[1, 1, 1], [0, 1, 0], [0, 0, 0]])))


def test_samples_overlap_leaves_a_draw_without_volume_out_of_the_summary():
    """A draw that is finite and not DEFAULT_BBOX counts for `estimate_samples`, but with no volume the box model refuses it: its pairs
    are NaN in `iou_pairs` and stay out of `iou_mean` / `iou_min`, which are those of the other draws."""
    cube = lambda dx: corners([1, 1, 1], t=cases.T0 + [dx, 0, 0])      # noqa: E731
    flat = corners([1.0, 0.0, 1.0], t=cases.T0)
    r = {"bbox_samples": np.stack([np.stack([cube(0.0), flat, cube(0.5), cube(0.25)]), np.stack([flat, cube(0.0), flat, flat])]),
         "bbox": np.stack([cube(0.25), cube(0.0)]), "valid": np.array([1, 1], dtype=np.int32)}
    g = boxes.samples_overlap(r, ref=True)
    iou = lambda s: (1 - s) / (1 + s)      # noqa: E731
    assert np.isnan(g["iou_pairs"][0, 1]).all() and np.isnan(g["iou_pairs"][0, :, 1]).all() and np.isnan(g["iou_to_mean"][0, 1])
    assert np.isfinite(g["iou_pairs"][0][np.ix_([0, 2, 3], [0, 2, 3])]).all()
    assert abs(g["iou_mean"][0] - (iou(0.5) + 2 * iou(0.25)) / 3) <= TOL and abs(g["iou_min"][0] - iou(0.5)) <= TOL
    # one draw with volume: no pair
    assert np.isnan(g["iou_mean"][1]) and np.isnan(g["iou_min"][1]) and abs(g["iou_pairs"][1, 1, 1] - 1.0) <= TOL
