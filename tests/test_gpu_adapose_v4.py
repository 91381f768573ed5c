"""-m gpu: the adapose_v4 plugin — `rgbm_prepare_inputs_opt` (crop kernels with and without the ImageNet step),
`rgbm_adapose_postprocess_regressed` (box tail from the network's own translation / size heads) and `AdaPoseEstimator_v4` end to end.
References: tests/golden/postproc_v4.npz (the reference's own results) and tests/postproc_v4_ref.py (its numpy restatement)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import postproc_v4_ref  # noqa: E402
from rgbmanip_amd import _lib, synth  # noqa: E402
from rgbmanip_amd.adapose import postprocess_regressed, prepare_inputs  # noqa: E402

KEYS = ("img", "choose", "pts2d", "Kcrop", "window", "valid")
SEED = 77
_CACHE = {}


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "postproc_v4.npz"))


def _frames():
    """Three 480x640 8-bit frames (synth.crop_frames + an empty mask): more than 1024 mask pixels (hash subset), fewer (wrap padding, a
    window shifted back into the frame), none.  Built once, never written."""
    if "frames" not in _CACHE:
        u8, mask, K = synth.crop_frames(seed=0)
        u8 = np.concatenate([u8, u8[:1, ::-1]])
        mask = np.concatenate([mask, np.zeros_like(mask[:1])])
        K = np.concatenate([K, K[:1]])
        f32 = u8.astype(np.float32) / np.float32(255)
        assert mask[0].sum() > 1024 > mask[1].sum() > 0 and mask[2].sum() == 0
        _CACHE["frames"] = dict(u8=_cuda(u8), f32=_cuda(f32), mask=_cuda(mask), K=_cuda(K))
    return _CACHE["frames"]


def _call(fn, rgb, mask, K, head, S=224, P=1024, N=None, fill=None):
    """One of the rgbm_prepare_inputs_* entry points through the C ABI: `head` = the arguments between K and N."""
    lib = _lib.load()
    N = N or K.shape[0]
    H, W = rgb.shape[1:3]
    out = dict(img=torch.empty(N, 3, S, S, dtype=torch.float32, device="cuda"), choose=torch.empty(N, P, dtype=torch.int32, device="cuda"),
               pts2d=torch.empty(N, P, 2, dtype=torch.float32, device="cuda"), Kcrop=torch.empty(N, 3, 3, dtype=torch.float64, device="cuda"),
               window=torch.empty(N, 4, dtype=torch.int32, device="cuda"), valid=torch.empty(N, dtype=torch.int32, device="cuda"))
    if fill is not None:
        for v in out.values():
            v.fill_(fill)
    scratch = torch.empty(N * S * S, dtype=torch.uint8, device="cuda")
    rc = getattr(lib, fn)(*head(_lib.ptr(rgb), _lib.ptr(mask), _lib.ptr(K)), N, H, W, S, P, SEED, *[_lib.ptr(out[k]) for k in KEYS],
                          _lib.ptr(scratch), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in out.items()}


def _opt(pixel_type, normalize, frame0=0):
    return lambda r, m, k: (r, pixel_type, normalize, m, k, None, frame0)


# ------------------------------------------------------------------------------------------------------------------ 1. the crop kernels
@pytest.mark.parametrize("pixel_type", [0, 1])
def test_prepare_opt_normalised_is_the_existing_entry_point(pixel_type):
    """normalize = 1: every output bit for bit what rgbm_prepare_inputs_ex (float frames) / rgbm_prepare_inputs_u8 (bytes) write."""
    c = _frames()
    rgb = c["u8"] if pixel_type else c["f32"]
    old = "rgbm_prepare_inputs_u8" if pixel_type else "rgbm_prepare_inputs_ex"
    for frame0 in (0, 5):
        rc0, ref = _call(old, rgb, c["mask"], c["K"], lambda r, m, k: (r, m, k, None, frame0))
        rc1, got = _call("rgbm_prepare_inputs_opt", rgb, c["mask"], c["K"], _opt(pixel_type, 1, frame0))
        assert rc0 == 0 and rc1 == 0
        for k in KEYS:
            assert got[k].dtype == ref[k].dtype and np.array_equal(_bits(got[k]), _bits(ref[k])), (k, frame0)
        assert ref["valid"].tolist() == [1, 1, 0]
        assert len(np.unique(ref["choose"][0])) == 1024 and len(np.unique(ref["choose"][1])) < 1024       # subset branch, wrap padding


def test_prepare_opt_unnormalised_reproduces_the_reference_crop(golden):
    """normalize = 0 against the crop the reference's v4 `prepare_model_input` returns for frame 0 (task one_door_cabinet, plain
    ToTensor), error = max|a - b| / max|b|.  Bound: tests/test_gpu_adapose.py::test_prepare_inputs_bit_exact_vs_oracle holds the
    normalising path to bit equality with the same resize arithmetic, and what runs in front of the normalisation is the same code:
    the error must be 0.  Everything but the image equals the normalize = 1 call; bytes equal the float frames fl32(b / 255)."""
    c = _frames()
    assert int(golden["crop0_size"]) == 224
    rc, norm = _call("rgbm_prepare_inputs_opt", c["f32"], c["mask"], c["K"], _opt(0, 1))
    rc_f, got = _call("rgbm_prepare_inputs_opt", c["f32"], c["mask"], c["K"], _opt(0, 0))
    rc_b, got8 = _call("rgbm_prepare_inputs_opt", c["u8"], c["mask"], c["K"], _opt(1, 0))
    assert rc == 0 and rc_f == 0 and rc_b == 0
    ref = golden["crop0_img"].astype(np.float64)
    err = float(np.abs(got["img"][0].astype(np.float64) - ref).max() / np.abs(ref).max())
    print("un-normalised crop vs the reference's: normalised error", err)
    assert err == 0.0
    assert np.array_equal(got["Kcrop"][0], golden["crop0_K"])
    for k in ("choose", "pts2d", "Kcrop", "window", "valid"):
        assert np.array_equal(_bits(got[k]), _bits(norm[k])), k
    for k in KEYS:
        assert np.array_equal(_bits(got8[k]), _bits(got[k])), k
    # the normalised image is the un-normalised one through (v - mean) / std, rounded once more: close, and really another image
    mean, std = np.float32([0.485, 0.456, 0.406])[:, None, None], np.float32([0.229, 0.224, 0.225])[:, None, None]
    np.testing.assert_array_equal(norm["img"][:2], ((got["img"][:2] - mean) / std).astype(np.float32))
    assert got["img"][:2].min() >= 0.0 and got["img"][:2].max() <= 1.0 and np.isfinite(got["img"]).all()


def test_prepare_opt_refuses_other_switch_values():
    """pixel_type / normalize outside {0, 1}: an argument error, nothing is launched (the outputs keep their fill)."""
    c = _frames()
    for pt, nm in ((2, 1), (0, 2), (-1, 0), (1, -1)):
        rc, got = _call("rgbm_prepare_inputs_opt", c["f32"], c["mask"], c["K"], _opt(pt, nm), fill=7)
        assert rc != 0 and b"pixel_type" in _lib.load().rgbm_last_error(), (pt, nm)
        assert (got["valid"] == 7).all() and (got["img"] == 7).all() and (got["choose"] == 7).all()


# ------------------------------------------------------------------------------------------------------------------ 2. the regressed tail
def _tail(nocs, r, t, s, E):
    out = postprocess_regressed(_cuda(nocs), _cuda(r), _cuda(t), _cuda(s), _cuda(E))
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in out]


def test_regressed_tail_matches_reference_golden(golden):
    """Every golden pose in one call and again one pose per call: bit-identical (no cross-pose state).  Against the reference's boxes
    the bound is the one tests/test_gpu_kernels.py::test_postprocess_matches_golden holds the v5 tail to (rtol 1e-6, atol 1e-7): the
    kernel follows the reference's float32 steps (norm, size, the sgemm's fma chain), so it is met with float64 room."""
    g = golden
    n = len(g["bbox"])
    box, ts, valid = _tail(g["nocs"], g["r"], g["t"], g["s"], g["E1"])
    for i in range(n):
        b1, t1, v1 = _tail(g["nocs"][i:i + 1], g["r"][i:i + 1], g["t"][i:i + 1], g["s"][i:i + 1], g["E1"][i:i + 1])
        assert np.array_equal(_bits(b1[0]), _bits(box[i])) and np.array_equal(_bits(t1[0]), _bits(ts[i])) and v1[0] == valid[i], i
    worst = 0.0
    for i in range(n):
        is_default = np.array_equal(g["bbox"][i], postproc_v4_ref.DEFAULT_BBOX)
        assert bool(valid[i]) == (not is_default), (i, str(g["kinds"][i]))
        worst = max(worst, float(np.abs(box[i] - g["bbox"][i]).max() / np.abs(g["bbox"][i]).max()))
    print("regressed tail vs golden: largest normalised error", worst)
    for i in range(n):
        np.testing.assert_allclose(box[i], g["bbox"][i], rtol=1e-6, atol=1e-7, err_msg=f"case {i} {g['kinds'][i]}")
    assert np.array_equal(ts[:, 3].astype(np.float32), g["scale"], equal_nan=True)           # the float32 norm, exactly (NaN where the golden's is)
    assert np.array_equal(ts[:, :3], g["t"].astype(np.float64))
    assert valid.sum() == n - 4


def _poses(B, P, seed):
    g = np.random.default_rng(seed)
    nocs = g.uniform(-0.45, 0.45, (B, P, 3)).astype(np.float32)
    r = np.stack([np.linalg.qr(g.normal(size=(3, 3)))[0] for _ in range(B)]).astype(np.float32)
    t = (np.array([0.0, 0.0, 0.8]) + g.normal(0, 0.2, (B, 3))).astype(np.float32)
    s = g.normal(0, 0.3, (B, 3)).astype(np.float32)
    E = np.tile(np.eye(4), (B, 1, 1))
    for b in range(B):
        E[b, :3, :3] = np.linalg.qr(g.normal(size=(3, 3)))[0]
        E[b, :3, 3] = g.normal(size=3)
    return nocs, r, t, s, E


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("P", [1, 5, 1023, 1024])
def test_regressed_tail_edge_cases(P, B):
    """P = 1 (one thread holds the only point), 5, 1023 (a ragged last round of the 256 threads), 1024; B = 1 and 3.  Clean poses
    against the restatement; then one defect at a time — NaN in s1 (pose 1 of 3), a singular E1, an inf in nocs1: exactly that pose
    returns the default box and valid = 0, its neighbours keep the clean run's bits.
    Bound against the restatement: its float32 part is the kernel's arithmetic bit for bit; the float64 world transform differs by the
    summation order of 4-term dot products and Gauss-Jordan against LAPACK's LU on orthonormal extrinsics (condition number < 10):
    some tens of float64 roundings, eps64 * 30 * 10 = 7e-14 relative to the box magnitude -> 1e-12."""
    nocs, r, t, s, E = _poses(B, P, 100 * P + B)
    box, ts, valid = _tail(nocs, r, t, s, E)
    exp, scale, ok = postproc_v4_ref.bbox_world_batch(nocs, r, t, s, E)
    assert ok.all() and valid.tolist() == [1] * B
    assert np.array_equal(_bits(ts[:, 3].astype(np.float32)), _bits(scale))
    for b in range(B):
        err = float(np.abs(box[b] - exp[b]).max() / np.abs(exp[b]).max())
        assert err < 1e-12, (b, err)
    defects = {"nan_s": min(1, B - 1), "singular_E": 0, "inf_nocs": B - 1}
    for kind, bad in defects.items():
        n2, s2, E2 = nocs.copy(), s.copy(), E.copy()
        if kind == "nan_s":
            s2[bad, 2] = np.nan
        elif kind == "singular_E":
            E2[bad, 1] = 0.0
        else:
            n2[bad, P - 1, 1] = -np.inf
        b2, t2, v2 = _tail(n2, r, t, s2, E2)
        assert v2.tolist() == [0 if b == bad else 1 for b in range(B)], kind
        assert np.array_equal(b2[bad], postproc_v4_ref.DEFAULT_BBOX), kind
        assert postproc_v4_ref.bbox_world(n2[bad], r[bad], t[bad], s2[bad], E2[bad])[2] == 0, kind          # the restatement agrees
        for b in range(B):
            if b != bad:
                assert np.array_equal(_bits(b2[b]), _bits(box[b])) and np.array_equal(_bits(t2[b]), _bits(ts[b])), (kind, b)


def test_regressed_tail_refuses_bad_shapes():
    nocs, r, t, s, E = _poses(1, 4, 0)
    lib = _lib.load()
    d = [_cuda(x) for x in (nocs, r, t, s, E)]
    out = (torch.empty(1, 8, 3, dtype=torch.float64, device="cuda"), torch.empty(1, 4, dtype=torch.float64, device="cuda"),
           torch.empty(1, dtype=torch.int32, device="cuda"))
    for B, P in ((0, 4), (1, 0), (1, 1025)):
        assert lib.rgbm_adapose_postprocess_regressed(B, P, *[_lib.ptr(x) for x in d], *[_lib.ptr(x) for x in out], _lib.stream_ptr()) != 0


# ------------------------------------------------------------------------------------------------------------------ 3. the plugin
def _scene():
    """Two poses: 480x640 8-bit frames with elliptical masks (more than 1024 resized pixels each), the extrinsics of
    synth.adapose_inputs(2, seed=0)."""
    if "scene" not in _CACHE:
        g = np.random.default_rng(3)
        n = 2
        yy, xx = np.mgrid[0:480, 0:640]
        K = np.tile(np.array([[439.31, 0, 320.0], [0, 439.31, 240.0], [0, 0, 1.0]])[None], (n, 1, 1))
        base = synth.adapose_inputs(n, seed=0)
        f1 = np.clip(0.5 + 0.25 * np.cos(xx / 37.0)[None, :, :, None] + 0.2 * g.random((n, 480, 640, 3)), 0, 1)
        f2 = np.clip(0.5 + 0.25 * np.sin(yy / 29.0)[None, :, :, None] + 0.2 * g.random((n, 480, 640, 3)), 0, 1)
        u1, u2 = (np.rint(f * 255.0).astype(np.uint8) for f in (f1, f2))
        m1 = np.stack([((yy - 240) / 60.0) ** 2 + ((xx - 300 - 10 * i) / 90.0) ** 2 <= 1 for i in range(n)]).astype(np.uint8)
        m2 = np.stack([((yy - 250) / 70.0) ** 2 + ((xx - 340 + 10 * i) / 80.0) ** 2 <= 1 for i in range(n)]).astype(np.uint8)
        deq = lambda u: u.astype(np.float32) / np.float32(255)      # noqa: E731
        _CACHE["scene"] = dict(K=_cuda(K), u1=_cuda(u1), u2=_cuda(u2), f1=_cuda(deq(u1)), f2=_cuda(deq(u2)), m1=_cuda(m1), m2=_cuda(m2),
                               E1=_cuda(base["E1"].astype(np.float64)), E2=_cuda(base["E2"].astype(np.float64)))
    return _CACHE["scene"]


def _net(view2_heads=0):
    from rgbmanip_amd.adapose import AdaPoseNet
    key = ("net", view2_heads)
    if key not in _CACHE:
        _CACHE[key] = AdaPoseNet(synth.adapose_state_dict(seed=0, prefix="module."), dtype="fp32", options={"view2_heads": view2_heads})
    return _CACHE[key]


def _est(task, view2_heads=0, **cfg):
    from rgbmanip_amd.config import adapose_cfg
    from rgbmanip_amd.estimator import AdaPoseEstimator_v4
    cfg = dict(adapose_cfg(task, load=False, name="adapose_v4"), hip_prepare="device", hip_prepare_seed=9, hip_view2_heads=bool(view2_heads), **cfg)
    return AdaPoseEstimator_v4(None, cfg, None, net=_net(view2_heads))


def _by_hand(task, rgb1, rgb2):
    """prepare_inputs(normalize=task == "pots") -> a plain AdaPoseNet forward -> postprocess_regressed, as the issue spells the v4 path."""
    from rgbmanip_amd.estimator import DEFAULT_BBOX
    c, net, lib = _scene(), _net(0), _lib.load()
    a = prepare_inputs(rgb1, c["m1"], c["K"], 224, 1024, 9, normalize=task == "pots")
    b = prepare_inputs(rgb2, c["m2"], c["K"], 224, 1024, 10, normalize=task == "pots")
    P = []
    for Kc, E in ((a["Kcrop"], c["E1"]), (b["Kcrop"], c["E2"])):
        p = torch.empty(2, 4, 4, dtype=torch.float32, device="cuda")
        _lib.check(lib.rgbm_projection(_lib.ptr(Kc), _lib.ptr(E), _lib.ptr(p), 2, _lib.stream_ptr()))
        P.append(p)
    depths = _cuda(np.tile(np.arange(0.1, 0.1 * (24 - 0.5) + 0.1, 0.1, dtype=np.float32)[None], (2, 1)))
    pred = net(a["img"], a["choose"], b["img"], b["choose"], P[0], P[1], depths)
    box, ts, valid = postprocess_regressed(pred["view1_nocs"], pred["view1_r"], pred["view1_t"], pred["view1_s"], c["E1"])
    torch.cuda.synchronize()
    assert (a["valid"] == 1).all() and (b["valid"] == 1).all() and (valid == 1).all()
    box = box.cpu().numpy()
    assert not np.array_equal(box[0], DEFAULT_BBOX) and np.isfinite(box).all()
    return box, a["img"].cpu().numpy()


@pytest.mark.parametrize("task", ["one_door_cabinet", "pots"])
def test_v4_estimator_end_to_end_batch2(task):
    """`AdaPoseEstimator_v4.estimate_device` at batch 2 (seeded weights, fp32 net) bit for bit equals the pipeline built by hand; the
    same from 8-bit frames, with the content-keyed feature cache (second call: every crop hits, the PSPNet does not run), with the
    view-2 heads on, through the numpy-facing `estimate`, and the two tasks feed the network different crops."""
    c = _scene()
    want, img = _by_hand(task, c["f1"], c["f2"])
    if task == "pots":
        assert img.min() < -0.5                                     # ImageNet-normalised
    else:
        assert img.min() >= 0.0 and img.max() <= 1.0                # the crop itself
    est = _est(task)
    got = est.estimate_device(c["K"], c["f1"], c["m1"], c["E1"], c["f2"], c["m2"], c["E2"]).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want))
    got8 = est.estimate_device(c["K"], c["u1"], c["m1"], c["E1"], c["u2"], c["m2"], c["E2"]).cpu().numpy()
    assert np.array_equal(_bits(got8), _bits(want)) and est.frames_u8_native == 4
    host = est.estimate(c["K"].cpu().numpy(), c["u1"].cpu().numpy(), c["m1"].cpu().numpy(), c["E1"].cpu().numpy(), c["u2"].cpu().numpy(),
                        c["m2"].cpu().numpy(), c["E2"].cpu().numpy())
    assert np.array_equal(_bits(host), _bits(want))
    # hip_feature_cache: "content"
    cached = _est(task, hip_feature_cache="content")
    first = cached.estimate_device(c["K"], c["f1"], c["m1"], c["E1"], c["f2"], c["m2"], c["E2"]).cpu().numpy()
    computed = cached.feature_views_computed
    second = cached.estimate_device(c["K"], c["u1"], c["m1"], c["E1"], c["u2"], c["m2"], c["E2"]).cpu().numpy()
    assert computed == 4 and cached.feature_views_computed == computed and cached.feature_cache_bypassed == 0
    assert np.array_equal(_bits(first), _bits(want)) and np.array_equal(_bits(second), _bits(want))
    # hip_view2_heads: the regressed tail reads view-1 outputs only, and they are computed in either mode.  Four instead of two views in
    # the heads may cross a kernel-selection threshold (another summation order): both runs are pinned to the generic tiles, as in
    # tests/test_gpu_adapose.py::test_view1_only_heads_equal_the_full_forward, and then agree bit for bit
    heads = _est(task, view2_heads=1)
    assert heads.view2_heads and not est.view2_heads
    _lib.check(_lib.load().rgbm_set_tuning(b"ws_min_rows", 1 << 30))
    try:
        got_h = heads.estimate_device(c["K"], c["f1"], c["m1"], c["E1"], c["f2"], c["m2"], c["E2"]).cpu().numpy()
        got_0 = est.estimate_device(c["K"], c["f1"], c["m1"], c["E1"], c["f2"], c["m2"], c["E2"]).cpu().numpy()
    finally:
        _lib.check(_lib.load().rgbm_set_tuning(b"ws_min_rows", 0))
    assert np.array_equal(_bits(got_h), _bits(got_0)) and np.isfinite(got_h).all()
    # default selection: the same boxes up to the summation order of an fp32 net (the view-1 outputs agree to 1e-5 there; ten times that)
    assert float(np.abs(got_h - want).max() / np.abs(want).max()) < 1e-4


def test_v4_crops_differ_from_v5_only_off_pots():
    """The same frames through AdaPoseEstimator_v5 (always normalised, median tail): other boxes than v4's for both tasks; v4's pots
    crops are v5's crops."""
    from rgbmanip_amd.config import adapose_cfg
    from rgbmanip_amd.estimator import AdaPoseEstimator_v5
    c = _scene()
    v5 = AdaPoseEstimator_v5(None, dict(adapose_cfg("pots", load=False), hip_prepare="device", hip_prepare_seed=9, hip_view2_heads=False), None,
                             net=_net(0))
    b5 = v5.estimate_device(c["K"], c["f1"], c["m1"], c["E1"], c["f2"], c["m2"], c["E2"]).cpu().numpy()
    b4 = _est("pots").estimate_device(c["K"], c["f1"], c["m1"], c["E1"], c["f2"], c["m2"], c["E2"]).cpu().numpy()
    assert np.isfinite(b5).all() and not np.array_equal(b5, b4)
    a5 = v5._prepare(c["f1"], c["m1"], c["K"], 224, 1024, 9)["img"]
    a4 = _est("pots")._prepare(c["f1"], c["m1"], c["K"], 224, 1024, 9)["img"]
    a4c = _est("mugs")._prepare(c["f1"], c["m1"], c["K"], 224, 1024, 9)["img"]
    assert torch.equal(a5, a4) and not torch.equal(a5, a4c)


@pytest.mark.parametrize("queue_dtype", ["float32", "uint8"])
def test_v4_through_the_device_control_queue(queue_dtype):
    """One `ControlInterface.queue_only` round trip: the queue hands its frame pool to `estimate_device_indexed`; the boxes are the
    ones `estimate_device` gives for the two selected views gathered by hand, bit for bit (same crops, same network batch)."""
    from rgbmanip_amd.control_interface import ControlInterface
    from rgbmanip_amd.estimator import DEFAULT_BBOX
    N = 2
    est = _est("one_door_cabinet")
    ci = ControlInterface.queue_only(N, est, 5, queue_dtype=queue_dtype)
    for t in range(3):
        img, pose, gt = synth.control_view(N, t, seed=6)
        ci.add_view(img, pose)
        ci.accumulate_steps += 1
    got = ci.get_estimation().cpu().numpy()
    idx, has = ci.select_views()
    sel = lambda q, s: ci._gather(q, idx[s], has[s])      # noqa: E731
    ref = est.estimate_device(sel(ci.intrinsic_queue, 0), sel(ci.image_queue, 0), sel(ci.mask_queue, 0), sel(ci.extrinsic_queue, 0),
                              sel(ci.image_queue, 1), sel(ci.mask_queue, 1), sel(ci.extrinsic_queue, 1)).cpu().numpy()
    assert got.shape == (N, 8, 3) and np.array_equal(_bits(got), _bits(ref))
    # synth.control_view empties env 1's mask at step 2, and the queue (like the reference) still selects that view: default box there
    assert not np.array_equal(got[0], DEFAULT_BBOX) and np.isfinite(got[0]).all() and np.array_equal(got[1], DEFAULT_BBOX)
