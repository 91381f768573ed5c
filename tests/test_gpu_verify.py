"""GPU: rgbm_box_silhouette / rgbm_cloud_in_box (csrc/box_verify.hip) against their float64 numpy twins, integer for integer; the
silhouette of the ground-truth box against the synthetic camera's own mask; `select="mask"` / `verify=True` of the estimator."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import verify_cases as vc  # noqa: E402

from rgbmanip_amd import _lib, synth, verify  # noqa: E402

pytestmark = pytest.mark.gpu

_CASES = {c["name"]: c for c in vc.silhouette_cases()}
_CLOUDS = {c["name"]: c for c in vc.cloud_cases()}
_REF = {}                                          # twin results, computed once per case and left unchanged
FLOAT_KEYS = ("iou", "coverage", "precision")


def _ref(name):
    if name not in _REF:
        c = _CASES[name]
        _REF[name] = verify.box_silhouette_ref(c["boxes"], c["K"], c["E"], c["masks"], c["ok"])
    return _REF[name]


def _device_mask(masks, offset):
    """The mask bytes on the device, contiguous, with a base address `offset` bytes past 4-byte alignment."""
    m = torch.from_numpy(np.ascontiguousarray(masks))
    buf = torch.empty(m.numel() + 8, dtype=torch.uint8, device="cuda")
    start = (-buf.data_ptr()) % 4 + offset
    out = buf[start:start + m.numel()].view(m.shape)
    out.copy_(m)
    assert out.data_ptr() % 4 == offset % 4 and out.is_contiguous()
    return out


def _equal(got, ref, what):
    for k in verify.INT_KEYS + ("valid",):
        g = got[k].cpu().numpy()
        assert g.dtype == np.int32 and g.shape == ref[k].shape, (what, k)
        np.testing.assert_array_equal(g, ref[k], err_msg=f"{what}: {k}")
    for k in FLOAT_KEYS:                            # the documented expressions of equal integers: the same bits
        g = got[k].cpu().numpy()
        assert g.dtype == np.float64
        assert g.tobytes() == ref[k].tobytes() or np.array_equal(g, ref[k], equal_nan=True), (what, k)


@pytest.mark.parametrize("name", list(_CASES))
def test_box_silhouette_equals_its_twin(name):
    c, ref = _CASES[name], _ref(name)
    got = verify.box_silhouette(c["boxes"], c["K"], c["E"], _device_mask(c["masks"], c["offset"]), c["ok"])
    torch.cuda.synchronize()
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in got.values())
    _equal(got, ref, name)
    if name == "analytic":
        assert tuple(ref["rect"][0, 0, 0]) == vc.ANALYTIC_RECT and ref["area_box"][0, 0, 0] == vc.ANALYTIC_AREA
    if name == "special_48x64":                    # the cases are what they claim to be
        f = ref["flags"]
        assert (f & verify.BORDER).any() and (f & verify.BEHIND).any() and (f & verify.CAMERA_INSIDE).any() and (f == 0).any()
        assert (f[2, :, 1] == 0).all() and ref["area_mask"][2, 1] > 0 and ref["area_mask"][0, 1] == 0
        assert ((f & verify.BEHIND) != 0)[ref["area_box"] > 0].any()          # a silhouette the projected corners do not bound
    # a second call gives the same bytes
    again = verify.box_silhouette(c["boxes"], c["K"], c["E"], _device_mask(c["masks"], c["offset"]), c["ok"])
    for k in got:
        assert torch.equal(got[k].view(torch.uint8), again[k].view(torch.uint8)), k


@pytest.mark.parametrize("name", ["s64_v16", "special_48x64"])
def test_one_box_per_launch_counts_what_sixty_four_count(name):
    """Sharing the mask read must not change a count: every box alone (S = 1) against the twin's column of the S-box call."""
    c, ref = _CASES[name], _ref(name)
    mask = _device_mask(c["masks"], 0)
    S = c["boxes"].shape[1]
    for s in range(S):
        got = verify.box_silhouette(c["boxes"][:, s], c["K"], c["E"], mask, None if c["ok"] is None else c["ok"][:, s:s + 1])
        for k in ("area_box", "inter", "rect", "flags"):
            np.testing.assert_array_equal(got[k].cpu().numpy(), ref[k][:, s:s + 1], err_msg=f"{name}: box {s}: {k}")
        np.testing.assert_array_equal(got["area_mask"].cpu().numpy(), ref["area_mask"])


def test_mask_offsets_past_two_gib():
    """7200 frames of 480 x 640 (2.2 GB of mask): the last pose's bytes lie past 2^31; the other poses have no foreground and ok = 0."""
    n, H, W = 7200, 480, 640
    c = _CASES["frame_480x640"]
    pick = np.argsort(-_ref("frame_480x640")["area_box"][0, :, 0], kind="stable")[:2]      # the two largest silhouettes of view 0
    c = dict(c, boxes=c["boxes"][:, pick], ok=c["ok"][:, pick])
    ref = verify.box_silhouette_ref(c["boxes"], c["K"][:, 0], c["E"][:, 0], c["masks"][:, 0], c["ok"])
    mask = torch.zeros(n, H, W, dtype=torch.uint8, device="cuda")
    mask[-1].copy_(torch.from_numpy(c["masks"][0, 0]))
    boxes = torch.from_numpy(np.broadcast_to(c["boxes"], (n, 2, 8, 3)).copy()).cuda()
    ok = torch.zeros(n, 2, dtype=torch.uint8, device="cuda")
    ok[-1] = torch.from_numpy(c["ok"][0]).cuda()
    K, E = np.broadcast_to(c["K"][:, 0], (n, 3, 3)), np.broadcast_to(c["E"][:, 0], (n, 4, 4))
    got = verify.box_silhouette(boxes, K.copy(), E.copy(), mask, ok)
    for k in verify.INT_KEYS:
        g = got[k].cpu().numpy()
        np.testing.assert_array_equal(g[-1:], ref[k], err_msg=k)
        if k != "rect":
            assert not g[:-1].any(), k
    assert ref["area_box"].min() > 0 and ref["inter"].max() > 0


@pytest.mark.parametrize("inflate", vc.INFLATES)
@pytest.mark.parametrize("name", list(_CLOUDS))
def test_cloud_in_box_equals_its_twin(name, inflate):
    c = _CLOUDS[name]
    ref = verify.cloud_in_box_ref(c["cloud"], c["count"], c["boxes"], c["ok"], inflate=inflate)
    got = verify.cloud_in_box(c["cloud"], c["count"], c["boxes"], c["ok"], inflate=inflate)
    for k in ("inside", "total", "valid"):
        g = got[k].cpu().numpy()
        assert g.dtype == np.int32
        np.testing.assert_array_equal(g, ref[k], err_msg=f"{name}: {k}")
    assert np.array_equal(got["share"].cpu().numpy(), ref["share"], equal_nan=True)
    assert ref["inside"].max() > 0
    if name == "two_view_counts" and inflate == 0.0:          # the 8 rows on faces, edges and corners of the unit cube, alone
        one = verify.cloud_in_box(c["cloud"][2:3, 1:9], np.asarray([8], np.int32), c["boxes"][2:3, 0])
        assert one["inside"].tolist() == [[8]] and one["total"].tolist() == [8]


def test_refused_arguments_launch_nothing():
    lib = _lib.load()
    st = _lib.stream_ptr()
    box = torch.from_numpy(vc.ANALYTIC_BOX.copy()).cuda()
    K, E = torch.from_numpy(vc.ANALYTIC_K.copy()).cuda(), torch.eye(4, dtype=torch.float64, device="cuda")
    mask = torch.ones(8, 8, dtype=torch.uint8, device="cuda")
    out = [torch.full((64,), 7, dtype=torch.int32, device="cuda") for _ in range(5)]
    scratch = torch.empty(1 << 16, dtype=torch.float64, device="cuda")
    p = _lib.ptr
    call = lambda n, S, V, H, W, nbytes=scratch.numel() * 8: lib.rgbm_box_silhouette(      # noqa: E731
        p(box), None, p(K), p(E), p(mask), n, S, V, H, W, *[p(o) for o in out], p(scratch), nbytes, st)
    for a in ((0, 1, 1, 8, 8), (1, 0, 1, 8, 8), (1, 65, 1, 8, 8), (1, 1, 17, 8, 8), (1 << 20, 64, 1, 8, 8), (1, 1, 1, 0, 8), (1, 1, 1, 1 << 16, 1 << 15)):
        assert call(*a) != 0, a
        assert b"box_silhouette" in lib.rgbm_last_error()
    assert call(1, 1, 1, 8, 8, nbytes=8) != 0 and b"scratch" in lib.rgbm_last_error()
    cloud, count = torch.zeros(4, 3, dtype=torch.float32, device="cuda"), torch.ones(2, dtype=torch.int32, device="cuda")
    for S, cols, cap, inflate in ((0, 1, 4, 0.0), (65, 1, 4, 0.0), (1, 0, 4, 0.0), (1, 17, 4, 0.0), (1, 1, -1, 0.0), (1, 1, 4, -1.0), (1, 1, 4, float("nan"))):
        assert lib.rgbm_cloud_in_box(p(cloud), p(count), cols, p(box), None, 1, S, cap, inflate, p(out[0]), p(out[1]), st) != 0
        assert b"cloud_in_box" in lib.rgbm_last_error()
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in out)
    with pytest.raises(ValueError, match="S <= 64"):
        verify.box_silhouette(np.zeros((1, 65, 8, 3)), vc.ANALYTIC_K[None], np.eye(4)[None], np.zeros((1, 8, 8), np.uint8))


# ------------------------------------------------------------------------------------------------------------------ the synthetic camera
@pytest.mark.parametrize("color_dtype", ["float32", "uint8"])
def test_ground_truth_box_matches_the_rendered_mask(color_dtype):
    from rgbmanip_amd import synthetic_env as se
    N = 4
    robots, boxes, cam = vc.hand_camera_scenes(N)
    env = se.SyntheticMultiVecEnv(N, "cuda", seed=0, color_dtype=color_dtype)
    env._robot.copy_(torch.from_numpy(robots)); env._box.copy_(torch.from_numpy(boxes)); env._cam.copy_(torch.from_numpy(cam))
    img = env.get_image()["camera0"]
    truth = env.get_observation(gt=True)["handle_bbox"]
    K, E, mask = img["Intrinsic"], img["Extrinsic"], img["Mask"]
    sil = verify.box_silhouette(truth, K, E, mask)
    area_mask = sil["area_mask"][:, 0].cpu().numpy()
    assert area_mask.min() > 500
    diff = ((sil["area_box"] - sil["inter"])[:, 0, 0] + (sil["area_mask"][:, 0] - sil["inter"][:, 0, 0])).cpu().numpy()
    iou = sil["iou"][:, 0, 0].cpu().numpy()
    print("symmetric difference", diff.tolist(), "iou", iou.tolist(), "mask pixels", area_mask.tolist())
    assert diff.max() <= 2
    assert (1.0 - iou <= 2.0 / area_mask).all()
    # the long edge is the box's x axis (half extent 0: the largest): shifts of 2 cm and 10 cm along it score strictly less
    axis = torch.from_numpy(boxes[:, 3:6]).cuda()
    far, near = truth + 0.10 * axis[:, None], truth + 0.02 * axis[:, None]
    cube = torch.from_numpy(np.broadcast_to(verify.DEFAULT_BBOX, (N, 8, 3)).copy()).cuda()
    hyp = torch.stack([far, near, truth, cube], 1)
    sel = verify.select_by_mask(verify.box_silhouette(hyp, K, E, mask))
    score = sel["score"].cpu().numpy()
    print("score", score.tolist())
    assert (score[:, 2] > score[:, 1]).all() and (score[:, 1] > score[:, 0]).all()
    assert sel["best"].tolist() == [2] * N and sel["best"].dtype == torch.int64
    # the same on numpy inputs through the twin
    ref = verify.select_by_mask(verify.box_silhouette_ref(hyp.cpu().numpy()[:1], K.cpu().numpy()[:1], E.cpu().numpy()[:1], mask.cpu().numpy()[:1]))
    assert np.array_equal(ref["score"], score[:1], equal_nan=True) and ref["best"].tolist() == [2]


# ------------------------------------------------------------------------------------------------------------------ the estimator
def _sample_frames():
    from test_gpu_samples import _frames
    rgb, mask, K, E1, E2 = _frames()
    return rgb, mask, K, E1, E2, rgb[:, :, ::-1].copy(), mask[:, :, ::-1].copy()


def _sample_estimator(**kw):
    from rgbmanip_amd.config import ADAPOSE_CFGS
    from rgbmanip_amd.estimator import AdaPoseEstimator_v5
    cfg = dict(ADAPOSE_CFGS["adapose_cabinet"], load=False, hip_prepare="device", hip_dropout=0.15, hip_dropout_seed=11, **kw)
    return AdaPoseEstimator_v5(None, cfg, None, state_dict=synth.adapose_state_dict(seed=0, prefix="module."), dtype="bf16x3")


def test_estimate_samples_select_mask():
    rgb, mask, K, E1, E2, rgb2, mask2 = _sample_frames()
    est, S, n = _sample_estimator(), 3, rgb.shape[0]
    runs = {}
    for key, kw in (("plain", {}), ("mask", {"select": "mask"})):
        est.estimator.set_dropout(0.15, 11)
        runs[key] = est.estimate_samples(K, rgb, mask, E1, rgb2, mask2, E2, samples=S, **kw)
    plain, sel = runs["plain"], runs["mask"]
    new = ["bbox_best", "best", "mask_score", "mask_iou"]
    assert sorted(sel) == sorted(list(plain) + new)
    for k in plain:                                                                 # every existing key, bit for bit
        assert sel[k].dtype == plain[k].dtype and sel[k].tobytes() == plain[k].tobytes(), k
    by_hand = verify.samples_verify(plain, K, E1, mask, E2, mask2)
    assert sel["mask_iou"].shape == (n, S + 1, 2) and sel["mask_score"].shape == (n, S + 1) and sel["best"].dtype == np.int64
    for new_key, key in (("bbox_best", "bbox_best"), ("best", "best"), ("mask_score", "score"), ("mask_iou", "iou")):
        assert np.array_equal(sel[new_key], by_hand[key], equal_nan=True), new_key
    twin = verify.samples_verify(plain, K, E1, mask, E2, mask2, ref=True)
    for k in verify.INT_KEYS:
        np.testing.assert_array_equal(by_hand[k], twin[k], err_msg=k)
    np.testing.assert_array_equal(by_hand["best"], twin["best"])
    hyp = np.concatenate([plain["bbox_samples"], plain["bbox"][:, None]], 1)
    for i in range(n):
        assert sel["best"][i] >= 0 and np.array_equal(sel["bbox_best"][i], hyp[i, sel["best"][i]])
    print("mask_score", sel["mask_score"].tolist(), "best", sel["best"].tolist())
    # the device form: the same tensors
    est.estimator.set_dropout(0.15, 11)
    cu = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()      # noqa: E731
    d = est.estimate_samples_device(K, cu(rgb), cu(mask), E1, cu(rgb2), cu(mask2), E2, samples=S, select="mask")
    assert sorted(d) == sorted(sel)
    for k in sel:
        assert isinstance(d[k], torch.Tensor) and d[k].is_cuda and np.array_equal(d[k].cpu().numpy(), sel[k], equal_nan=True), k
    # window upload holds no frame masks on the device: one upload of them, the same numbers
    from rgbmanip_amd.estimator import AdaPoseEstimator_v5
    win = AdaPoseEstimator_v5(None, dict(est.cfg, hip_upload="windows"), None, net=est.estimator)
    est.estimator.set_dropout(0.15, 11)
    w = win.estimate_samples(K, rgb, mask, E1, rgb2, mask2, E2, samples=S, select="mask")
    for k in sel:
        assert np.array_equal(w[k], sel[k], equal_nan=True), k
    for call in (est.estimate_samples, est.estimate_samples_device):
        with pytest.raises(ValueError, match="select"):
            call(K, rgb, mask, E1, rgb2, mask2, E2, samples=S, select="nope")


def test_estimate_cloud_pose_verify():
    from test_gpu_cloud import LOOSE, _estimator, _net, _scene
    s = _scene()
    est = _estimator(_net(view2_heads=1), hip_view2_heads=True, hip_ransac_seed=5)
    args = (s["K"], s["u1"], s["m1"], s["E1"], s["u2"], s["m2"], s["E2"])
    kw = dict(max_points=6000, **LOOSE)
    plain = est.estimate_cloud_pose(*args, **kw)
    got = est.estimate_cloud_pose(*args, verify=True, **kw)
    new = ["mask_iou", "mask_score", "cloud_share", "best"]
    assert sorted(got) == sorted(list(plain) + new)
    for k in plain:
        assert got[k].dtype == plain[k].dtype and got[k].tobytes() == plain[k].tobytes(), k
    n = s["K"].shape[0]
    assert got["mask_iou"].shape == (n, 2, 2) and got["mask_score"].shape == (n, 2) and got["cloud_share"].shape == (n, 2) and got["best"].shape == (n,)
    by_hand = verify.cloud_pose_verify(plain, s["K"], s["E1"], s["m1"], s["E2"], s["m2"])
    for new_key, key in (("mask_iou", "iou"), ("mask_score", "score"), ("cloud_share", "share"), ("best", "best")):
        assert np.array_equal(got[new_key], by_hand[key], equal_nan=True), new_key
    twin = verify.cloud_pose_verify(plain, s["K"], s["E1"], s["m1"], s["E2"], s["m2"], ref=True)
    for k in verify.INT_KEYS + ("inside", "total"):
        np.testing.assert_array_equal(by_hand[k], twin[k], err_msg=k)
    assert got["best"][1] == -1 and np.isnan(got["mask_score"][1]).all() and np.isnan(got["cloud_share"][1]).all()      # the empty mask
    print("mask_score", got["mask_score"].tolist(), "cloud_share", got["cloud_share"].tolist(), "best", got["best"].tolist())
    cu = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()      # noqa: E731
    d = est.estimate_cloud_pose_device(s["K"], cu(s["u1"]), cu(s["m1"]), s["E1"], cu(s["u2"]), cu(s["m2"]), s["E2"], verify=True, **kw)
    assert sorted(d) == sorted(got)
    for k in got:
        assert isinstance(d[k], torch.Tensor) and d[k].is_cuda and np.array_equal(d[k].cpu().numpy(), got[k], equal_nan=True), k


def test_other_estimators_still_refuse():
    from rgbmanip_amd import estimator
    for cls in (estimator.AdaPoseEstimator_v2, estimator.AdaPoseEstimator_realworld):
        est = object.__new__(cls)                   # the refusals read nothing of the instance
        for name, kw in (("estimate_samples", {"select": "mask"}), ("estimate_samples_device", {"select": "mask"}),
                         ("estimate_cloud_pose", {"verify": True}), ("estimate_cloud_pose_device", {"verify": True})):
            with pytest.raises(NotImplementedError, match=name):
                getattr(est, name)(**kw)
