"""CPU: the float64 numpy twins of the box verification ops (rgbmanip_amd/verify.py), the selection rule and the two helpers for
estimator results, and the silhouette twin against the twin of the synthetic renderer (oracle/synth_env_ref.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import verify_cases as vc  # noqa: E402


def test_module_and_symbols_exist():
    """The feature's surface: rgbmanip_amd.verify, its re-export through adapose.py, and the C ABI symbols in the binding table."""
    from rgbmanip_amd import _lib, adapose, verify
    for name in ("rgbm_box_silhouette", "rgbm_box_silhouette_scratch_bytes", "rgbm_cloud_in_box"):
        assert name in _lib.SIGNATURES
    assert adapose.box_silhouette is verify.box_silhouette and adapose.cloud_in_box is verify.cloud_in_box
    for name in ("box_silhouette_ref", "cloud_in_box_ref", "select_by_mask", "samples_verify", "cloud_pose_verify"):
        assert callable(getattr(verify, name))


def test_analytic_rectangle():
    """Case (a): dyadic numbers throughout, so the silhouette is the pixel rectangle worked out by hand, ties included."""
    from rgbmanip_amd import verify
    H, W = vc.ANALYTIC_HW
    mask = np.zeros((1, H, W), dtype=np.uint8)
    mask[0, 22:40, 30:50] = 7
    r = verify.box_silhouette_ref(vc.ANALYTIC_BOX[None], vc.ANALYTIC_K[None], np.eye(4)[None], mask)
    assert r["area_box"].shape == (1, 1, 1) and r["rect"].shape == (1, 1, 1, 4)
    assert tuple(r["rect"][0, 0, 0]) == vc.ANALYTIC_RECT
    assert r["area_box"][0, 0, 0] == vc.ANALYTIC_AREA
    inter = (32 - 22 + 1) * (36 - 30 + 1)
    assert r["inter"][0, 0, 0] == inter and r["area_mask"][0, 0] == 18 * 20
    assert r["flags"][0, 0, 0] == verify.USABLE and r["valid"][0, 0, 0] == 1
    assert r["iou"][0, 0, 0] == inter / (vc.ANALYTIC_AREA + 18 * 20 - inter)
    assert r["coverage"][0, 0, 0] == inter / (18 * 20) and r["precision"][0, 0, 0] == inter / vc.ANALYTIC_AREA


def test_flags_nan_rules_and_empty_rect():
    """Cases (c) to (g): border, behind the camera, straddling the camera plane, the camera inside, and the four ways to be unusable."""
    from rgbmanip_amd import verify
    boxes, ok, names = vc.special_boxes()
    H, W = vc.ANALYTIC_HW
    S = len(names)
    mask = np.full((2, H, W), 255, dtype=np.uint8)
    K = np.stack([vc.ANALYTIC_K, vc.ANALYTIC_K])
    K[1, 0, 0] = 0.0
    r = verify.box_silhouette_ref(np.stack([boxes, boxes]), K, np.stack([np.eye(4)] * 2), mask, ok=np.stack([ok, ok]))
    at = {name: k for k, name in enumerate(names)}
    flags, empty = r["flags"][0, :, 0], np.asarray([H, W, -1, -1])
    assert flags[at["axis_aligned"]] == verify.USABLE
    assert flags[at["sheared_negative_det"]] == verify.USABLE and r["area_box"][0, at["sheared_negative_det"], 0] > 0
    for name, edge in (("border_left", 1), ("border_right", 3), ("border_top", 0), ("border_bottom", 2)):
        k = at[name]
        assert flags[k] == verify.USABLE | verify.BORDER, name
        assert r["rect"][0, k, 0, edge] == (0, 0, H - 1, W - 1)[edge], name
        assert 0 < r["area_box"][0, k, 0] < H * W
    k = at["behind"]
    assert flags[k] == verify.USABLE | verify.BEHIND and r["area_box"][0, k, 0] == 0 and (r["rect"][0, k, 0] == empty).all()
    assert np.isnan(r["precision"][0, k, 0]) and r["iou"][0, k, 0] == 0.0 and r["coverage"][0, k, 0] == 0.0
    k = at["straddles_camera_plane"]
    assert flags[k] == verify.USABLE | verify.BEHIND | verify.BORDER and r["area_box"][0, k, 0] > 0
    k = at["camera_inside"]
    assert flags[k] == verify.USABLE | verify.BEHIND | verify.CAMERA_INSIDE and r["area_box"][0, k, 0] == 0
    for name in ("zero_volume", "nan_corner", "not_ok"):
        k = at[name]
        assert flags[k] == 0 and r["valid"][0, k, 0] == 0 and r["area_box"][0, k, 0] == 0 and r["inter"][0, k, 0] == 0, name
        assert (r["rect"][0, k, 0] == empty).all() and all(np.isnan(r[key][0, k, 0]) for key in ("iou", "coverage", "precision")), name
    # K00 = 0: every box of the pose is unusable, the mask is still counted
    assert (r["flags"][1] == 0).all() and (r["area_box"][1] == 0).all() and (r["rect"][1] == empty).all() and np.isnan(r["iou"][1]).all()
    assert r["area_mask"][1, 0] == H * W
    # an empty mask: coverage has no denominator, iou is 0 where the silhouette is not empty
    r0 = verify.box_silhouette_ref(boxes[None], vc.ANALYTIC_K[None], np.eye(4)[None], np.zeros((1, H, W), np.uint8), ok=ok[None])
    assert np.isnan(r0["coverage"]).all() and r0["iou"][0, at["axis_aligned"], 0] == 0.0 and np.isnan(r0["iou"][0, at["behind"], 0])


def test_argument_checks():
    from rgbmanip_amd import verify
    box, K, E, m = vc.ANALYTIC_BOX[None], vc.ANALYTIC_K[None], np.eye(4)[None], np.zeros((1, 8, 8), np.uint8)
    with pytest.raises(ValueError, match="S <= 64"):
        verify.box_silhouette_ref(np.zeros((1, 65, 8, 3)), K, E, m)
    with pytest.raises(ValueError, match="V <= 16"):
        verify.box_silhouette_ref(box, K, np.zeros((1, 17, 4, 4)), np.zeros((1, 17, 8, 8), np.uint8))
    with pytest.raises(ValueError, match="boxes"):
        verify.box_silhouette_ref(np.zeros((1, 8, 2)), K, E, m)
    with pytest.raises(ValueError, match="K "):
        verify.box_silhouette_ref(box, np.zeros((1, 2, 3, 3)), E, m)
    with pytest.raises(ValueError, match="inflate"):
        verify.cloud_in_box_ref(np.zeros((1, 4, 3), np.float32), np.zeros((1, 2), np.int32), box, inflate=-0.1)
    with pytest.raises(ValueError, match="count"):
        verify.cloud_in_box_ref(np.zeros((1, 4, 3), np.float32), np.zeros((2, 2), np.int32), box)


def test_cloud_in_box_twin():
    """Case (k): the counts, the NaN rows, and the points on and just outside the faces of the unit cube."""
    from rgbmanip_amd import verify
    case = vc.cloud_cases()[0]
    r0 = verify.cloud_in_box_ref(case["cloud"], case["count"], case["boxes"], case["ok"], inflate=0.0)
    r5 = verify.cloud_in_box_ref(case["cloud"], case["count"], case["boxes"], case["ok"], inflate=0.05)
    cap = case["cloud"].shape[1]
    assert r0["total"].tolist() == [0, 1, cap, cap, 1000, 1500]
    assert np.isnan(r0["share"][0]).all() and (r0["inside"][0] == 0).all()                      # no rows
    assert (r0["valid"][:, 2] == 0).all() and np.isnan(r0["share"][:, 2]).all()                 # the box without volume
    assert r0["valid"][1, 3] == 0 and r0["valid"][0, 3] == 1                                    # ok = 0
    # pose 2, the unit cube, by brute force: closed faces
    p = case["cloud"][2].astype(np.float64)
    brute = lambda g: int((np.isfinite(p).all(1) & (p >= -g).all(1) & (p <= 1.0 + g).all(1)).sum())      # noqa: E731
    assert r0["inside"][2, 0] == brute(0.0) and r5["inside"][2, 0] == brute(0.05)
    assert r5["inside"][2, 0] - r0["inside"][2, 0] >= 4                                          # the rows 1/32 outside a face
    assert r0["share"][2, 0] == r0["inside"][2, 0] / cap
    # the 8 rows on faces, edges and corners of the cube are inside at inflate 0; the NaN and inf rows of pose 4 never are
    one = verify.cloud_in_box_ref(case["cloud"][2:3, 1:9], np.asarray([8], np.int32), case["boxes"][2:3, 0])
    assert one["inside"][0, 0] == 8 and one["total"][0] == 8 and one["share"][0, 0] == 1.0
    bad = verify.cloud_in_box_ref(case["cloud"][4:5, [5, 40]], np.asarray([[2, 0]], np.int32), case["boxes"][4:5, 0], inflate=1e6)
    assert bad["inside"][0, 0] == 0 and bad["total"][0] == 2
    assert (r5["inside"] >= r0["inside"]).all() and r0["inside"][:, 1].max() > 0              # the sheared box, det < 0, holds points


def _sil(iou, area_mask, valid=None):
    iou = np.asarray(iou, dtype=np.float64)
    return {"iou": iou, "area_mask": np.asarray(area_mask, dtype=np.int32),
            "valid": np.ones(iou.shape, np.int32) if valid is None else np.asarray(valid, np.int32)}


def test_select_by_mask_rules():
    from rgbmanip_amd import verify
    nan = np.nan
    sil = _sil([[[0.2, 0.4], [0.5, 0.1], [nan, nan], [0.3, 0.3]],          # a tie between boxes 0, 1 and 3: the lowest index
                [[nan, 0.9], [0.1, 0.2], [0.4, 0.0], [0.0, 0.6]],          # view 0 of box 0 is NaN: it never wins, whatever view 1 says
                [[nan, nan]] * 4,                                           # nothing to choose from
                [[0.5, 0.9], [0.6, 0.1], [0.7, 0.2], [0.1, 0.3]]],         # view 1 has an empty mask: only view 0 counts
               [[10, 10], [10, 10], [10, 10], [10, 0]])
    sil["valid"][0, 2] = 0
    sil["valid"][1, 0, 0] = 0
    sil["valid"][2] = 0
    out = verify.select_by_mask(sil)
    np.testing.assert_array_equal(out["best"], [0, 3, -1, 2])
    assert out["best"].dtype == np.int64
    np.testing.assert_array_equal(out["score"][0], [(0.2 + 0.4) / 2, (0.5 + 0.1) / 2, nan, (0.3 + 0.3) / 2])
    assert np.isnan(out["score"][1, 0]) and np.isnan(out["score"][2]).all()
    np.testing.assert_array_equal(out["score"][3], [0.5, 0.6, 0.7, 0.1])
    none = verify.select_by_mask(_sil([[[0.5, 0.5]]], [[0, 0]]))           # no view shows the handle
    assert np.isnan(none["score"]).all() and none["best"][0] == -1


def _two_view_scene():
    """Camera 0 of the analytic case and a second, moved camera; each mask is the pixel rectangle of the analytic box's silhouette in
    its view (in view 0 the silhouette is that rectangle, in view 1 the rectangle is a little larger)."""
    from rgbmanip_amd import verify
    H, W = vc.ANALYTIC_HW
    rng = np.random.default_rng(3)
    E1, E2 = np.eye(4)[None], vc.extrinsic(rng, 0.1, 0.2)[None]
    K = vc.ANALYTIC_K[None]
    truth = vc.ANALYTIC_BOX[None]
    masks = []
    for E in (E1, E2):
        r = verify.box_silhouette_ref(truth, K, E, np.zeros((1, H, W), np.uint8))
        rows, cols = np.arange(H)[:, None], np.arange(W)[None, :]
        y1, x1, y2, x2 = r["rect"][0, 0, 0]
        masks.append(((rows >= y1) & (rows <= y2) & (cols >= x1) & (cols <= x2)).astype(np.uint8)[None])
    return K, E1, masks[0], E2, masks[1], truth


def test_samples_verify_on_a_hand_built_result():
    from rgbmanip_amd import verify
    from rgbmanip_amd.cloud import DEFAULT_BBOX
    K, E1, m1, E2, m2, truth = _two_view_scene()
    shifted = truth + [0.3, 0.0, 0.0]
    far = truth + [0.0, 0.0, 40.0]
    samples = np.stack([shifted[0], DEFAULT_BBOX, truth[0], far[0]])[None]                  # [1, 4, 8, 3]
    r = {"bbox_samples": samples, "bbox": shifted * 0.5 + truth * 0.5, "valid": np.ones(1, np.int32)}
    out = verify.samples_verify(r, K, E1, m1, E2, m2, ref=True)
    assert out["iou"].shape == (1, 5, 2) and out["score"].shape == (1, 5) and out["area_mask"].shape == (1, 2)
    assert out["best"][0] == 2 and (out["bbox_best"][0] == truth[0]).all()
    assert out["valid"][0, 1].tolist() == [0, 0] and np.isnan(out["score"][0, 1])           # the +10 cube is no draw
    assert out["score"][0, 2] > out["score"][0, 4] > out["score"][0, 0] > out["score"][0, 3] >= 0.0
    assert out["iou"][0, 2, 0] == 1.0                                                        # view 0: the mask is exactly the rectangle
    each = verify.box_silhouette_ref(samples[:, 2:3], K, E2, m2)
    np.testing.assert_array_equal(out["inter"][:, 2:3, 1:2], each["inter"])
    # nothing usable: best -1 and the +10 cube
    none = verify.samples_verify({"bbox_samples": samples[:, 1:2], "bbox": DEFAULT_BBOX[None], "valid": np.zeros(1, np.int32)}, K, E1, m1, E2, m2,
                                 ref=True)
    assert none["best"][0] == -1 and (none["bbox_best"][0] == DEFAULT_BBOX).all()
    with pytest.raises(ValueError, match="bbox_samples"):
        verify.samples_verify({"bbox": truth, "valid": np.ones(1)}, K, E1, m1, E2, m2, ref=True)


def test_cloud_pose_verify_on_a_hand_built_result():
    from rgbmanip_amd import verify
    from rgbmanip_amd.cloud import DEFAULT_BBOX
    K, E1, m1, E2, m2, truth = _two_view_scene()
    rng = np.random.default_rng(4)
    pts = (rng.uniform(0.0, 1.0, (1, 64, 3)) * [0.75, 0.75, 1.0] + [-0.5, -0.25, 2.0]).astype(np.float32)      # inside the true box
    pts[0, 50:] = np.nan
    r = {"bbox": truth + [0.25, 0.0, 0.0], "bbox_cloud": truth, "valid": np.ones(1, np.int32), "valid_cloud": np.ones(1, np.int32),
         "cloud": pts, "count": np.asarray([[30, 20]], np.int32)}
    out = verify.cloud_pose_verify(r, K, E1, m1, E2, m2, inflate=0.01, ref=True)
    assert out["iou"].shape == (1, 2, 2) and out["score"].shape == (1, 2) and out["share"].shape == (1, 2)
    assert out["best"][0] == 1 and out["total"][0] == 50 and out["inside"][0, 1] == 50 and out["share"][0, 1] == 1.0
    assert out["share"][0, 0] < 1.0
    r["valid_cloud"] = np.zeros(1, np.int32)
    r["bbox_cloud"] = DEFAULT_BBOX[None]
    out = verify.cloud_pose_verify(r, K, E1, m1, E2, m2, ref=True)
    assert out["best"][0] == 0 and np.isnan(out["score"][0, 1]) and np.isnan(out["share"][0, 1])


def test_twin_against_the_renderers_twin():
    """24 seeded scenes of the synthetic camera: the silhouette of the ground-truth corners under camera_ref's K and E against
    render_ref's mask.  The two use different but equivalent arithmetic (box coordinates with half extents there, camera-frame normals
    here), so single boundary ties may differ: at most 2 pixels of symmetric difference per 480 x 640 view."""
    from oracle import synth_env_ref as sr
    from rgbmanip_amd import synthetic_env as se, verify
    N, f = 24, se.CAM_F
    robots, boxes, cam = vc.hand_camera_scenes(N)
    K, E, rays = sr.camera_ref(cam, robots, boxes, f, f, 320.0, 240.0)
    _, mask = sr.render_ref(rays, boxes, f, f, 320.0, 240.0, 480, 640)
    r = verify.box_silhouette_ref(sr.box_corners(boxes), K, E, mask)
    area_mask = mask.reshape(N, -1).sum(1)
    assert area_mask.min() > 500                                               # every handle is in view
    np.testing.assert_array_equal(r["area_mask"][:, 0], area_mask)
    diff = (r["area_box"][:, 0, 0] - r["inter"][:, 0, 0]) + (r["area_mask"][:, 0] - r["inter"][:, 0, 0])
    print("symmetric difference per scene:", diff.tolist(), "mask pixels:", int(area_mask.min()), "to", int(area_mask.max()))
    assert diff.max() <= 2
    assert (r["flags"][:, 0, 0] & ~verify.BORDER == verify.USABLE).all()


def test_estimator_keywords_on_the_host():
    """`select` is checked before anything else is read; the estimators that refuse the sampled and cloud-pose calls refuse them with the
    new keywords too."""
    from rgbmanip_amd import estimator
    est = object.__new__(estimator.AdaPoseEstimator_v5)
    with pytest.raises(ValueError, match="select"):
        est._samples_check(3, "nope")
    for cls in (estimator.AdaPoseEstimator_v2, estimator.AdaPoseEstimator_realworld, estimator.AdaPoseEstimator_baseline):
        other = object.__new__(cls)
        for name, kw in (("estimate_samples", {"select": "mask"}), ("estimate_samples_device", {"select": "mask"}),
                         ("estimate_cloud_pose", {"verify": True}), ("estimate_cloud_pose_device", {"verify": True})):
            with pytest.raises(NotImplementedError, match=name):
                getattr(other, name)(**kw)
