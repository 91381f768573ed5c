"""-m gpu: S Dropout2d samples per pose from one backbone pass (rgbm_adapose_forward_samples), the statistics kernels of
csrc/sample_stats.hip against their float64 numpy twins, and `estimate_samples` end to end."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dropout_ref  # noqa: E402
import samples_cases as cases  # noqa: E402
from rgbmanip_amd import samples, synth  # noqa: E402

OUT_KEYS = ["view1_nocs", "view2_nocs", "view1_depth", "view2_depth", "view1_r", "view2_r", "view1_t", "view2_t", "view1_s", "view2_s"]
P, SEED = 0.15, 11


class _generic_kernels_only:
    """conv launches on the generic tiles while inside (rgbm_set_tuning ws_min_rows), as in tests/test_gpu_dropout.py: batches of
    different sizes then sum in the same order, so their outputs can be compared bit for bit"""
    def __enter__(self):
        from rgbmanip_amd import _lib
        _lib.check(_lib.load().rgbm_set_tuning(b"ws_min_rows", 1 << 30))

    def __exit__(self, *a):
        from rgbmanip_amd import _lib
        _lib.check(_lib.load().rgbm_set_tuning(b"ws_min_rows", 0))


def _net(dtype, **kw):
    from rgbmanip_amd.adapose import AdaPoseNet
    return AdaPoseNet(synth.adapose_state_dict(seed=0, prefix="module."), dtype=dtype, **kw)


ARGS = ("img1", "choose1", "img2", "choose2", "P1", "P2", "depths")


def _plain(net, inp):
    out = net(*[inp[k] for k in ARGS])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _sampled(net, inp, S):
    out = net.forward_samples(*[inp[k] for k in ARGS], samples=S)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _tiled(inp, S):
    return {k: np.tile(v, (S,) + (1,) * (v.ndim - 1)) for k, v in inp.items()}


def _assert_equals_tiled(net, inp, S, view2=True):
    """forward_samples after a reset of the mask sequence == the plain forward of the tiled batch after the same reset, bit for bit."""
    B = len(inp["img1"])
    net.set_dropout(P, SEED)
    want = _plain(net, _tiled(inp, S))
    net.set_dropout(P, SEED)
    got = _sampled(net, inp, S)
    for k in OUT_KEYS:
        assert got[k].shape == (S, B) + want[k].shape[1:], k
        np.testing.assert_array_equal(got[k].reshape(want[k].shape), want[k], err_msg=k)
        if k.startswith("view1") or view2:
            assert np.isfinite(got[k]).all(), k
        else:
            assert np.isnan(got[k]).all(), k
    return got


# ------------------------------------------------------------------------------------------------------------------ 1. the definition
@pytest.mark.parametrize("dtype", ["bf16", "bf16x3"])
def test_forward_samples_equals_the_tiled_plain_forward(dtype):
    B, S = 2, 3
    inp = synth.adapose_inputs(B, seed=4)
    net = _net(dtype, dropout=P, dropout_seed=SEED)
    with _generic_kernels_only():
        got = _assert_equals_tiled(net, inp, S)
        np.testing.assert_array_equal(net.dropout_masks(S * B).cpu().numpy(), dropout_ref.masks(P, SEED, S * B, first_pose=0))
        again = _sampled(net, inp, S)                          # the counter has advanced by S * B
        np.testing.assert_array_equal(net.dropout_masks(S * B).cpu().numpy(), dropout_ref.masks(P, SEED, S * B, first_pose=S * B))
    assert not np.array_equal(again["view1_nocs"], got["view1_nocs"])
    for b in range(B):
        for s, t in ((0, 1), (0, 2), (1, 2)):
            for k in ("view1_nocs", "view1_depth", "view1_r"):
                assert not np.array_equal(got[k][s, b], got[k][t, b]), (k, b, s, t)


def test_loaded_masks_are_honoured_once():
    B, S = 1, 2
    inp = synth.adapose_inputs(B, seed=6)
    net = _net("bf16")                                          # dropout off: only the loaded masks make it a dropout forward
    masks = dropout_ref.masks(P, 5, S * B, first_pose=40)
    with _generic_kernels_only():
        net.set_dropout_masks(masks)
        want = _plain(net, _tiled(inp, S))
        net.set_dropout_masks(masks)
        got = _sampled(net, inp, S)
    np.testing.assert_array_equal(net.dropout_masks(S * B).cpu().numpy(), masks)
    for k in OUT_KEYS:
        np.testing.assert_array_equal(got[k].reshape(want[k].shape), want[k], err_msg=k)
    assert not np.array_equal(got["view1_nocs"][0], got["view1_nocs"][1])
    from rgbmanip_amd import _lib
    with pytest.raises(_lib.RgbmError, match="Dropout2d is off"):      # used once: the next call has nothing to sample
        _sampled(net, inp, S)
    net.set_dropout_masks(masks)
    with pytest.raises(_lib.RgbmError, match="for batch 2"):           # loaded for S * B = 2, asked for 3
        _sampled(net, inp, 3)


# ------------------------------------------------------------------------------------------------------------------ 2. edges, refusals
def test_one_sample_is_the_plain_forward():
    inp = synth.adapose_inputs(2, seed=5)
    net = _net("bf16", dropout=P, dropout_seed=SEED)
    want = _plain(net, inp)
    net.set_dropout(P, SEED)
    got = _sampled(net, inp, 1)
    for k in OUT_KEYS:
        np.testing.assert_array_equal(got[k][0], want[k], err_msg=k)


@pytest.mark.parametrize("case", ["norm_mode1", "view2_heads0", "fp32", "fp16"])
def test_forward_samples_other_configurations(case):
    inp = synth.adapose_inputs(1, seed=7)
    kw = {"norm_mode1": dict(dtype="bf16x3", norm_mode=1), "view2_heads0": dict(dtype="bf16", options={"view2_heads": 0}),
          "fp32": dict(dtype="fp32"), "fp16": dict(dtype="fp16")}[case]
    net = _net(dropout=P, dropout_seed=SEED, **kw)
    with _generic_kernels_only():
        got = _assert_equals_tiled(net, inp, 2, view2=case != "view2_heads0")
    assert not np.array_equal(got["view1_nocs"][0], got["view1_nocs"][1])


def test_cost_volume_chunking_changes_nothing():
    inp = synth.adapose_inputs(1, seed=8)
    got = []
    with _generic_kernels_only():
        for chunk in (512, 2):                                 # 3 samples x 2 views: one chunk / three chunks of 2 views
            net = _net("bf16", dropout=P, dropout_seed=SEED, max_chunk_views=chunk)
            got.append(_sampled(net, inp, 3))
    for k in OUT_KEYS:
        np.testing.assert_array_equal(got[0][k], got[1][k], err_msg=k)


def test_refusals_leave_the_handle_as_it_was():
    from rgbmanip_amd import _lib
    from rgbmanip_amd.adapose import AdaPoseNet
    lib = _lib.load()
    inp = synth.adapose_inputs(1, seed=9)
    # dropout off, no masks loaded
    off = _net("bf16")
    before = _plain(off, inp)
    with pytest.raises(_lib.RgbmError, match="Dropout2d is off"):
        _sampled(off, inp, 2)
    after = _plain(off, inp)
    for k in OUT_KEYS:
        np.testing.assert_array_equal(before[k], after[k], err_msg=k)
    # S = 0, the upconv A/B paths and a short workspace, on a net with dropout: the pose counter does not move
    net = _net("bf16", dropout=P, dropout_seed=SEED)
    _plain(net, inp)                                           # pose 0
    with pytest.raises(_lib.RgbmError, match="S >= 1"):
        _sampled(net, inp, 0)
    t = [net._prep(inp[k], torch.int32 if k.startswith("choose") else torch.float32) for k in ("img1", "img2", "choose1", "choose2", "P1", "P2", "depths")]
    out = net._empty_outputs(2)
    o = _lib.AdaposeOut(*[out[n].data_ptr() for n, _ in _lib.AdaposeOut._fields_])
    ws = torch.empty(4096 + 256, dtype=torch.uint8, device="cuda")
    ws_ptr, _ = net._aligned(ws)
    rc = lib.rgbm_adapose_forward_samples(net._h, 1, 2, *[_lib.ptr(x) for x in t], C.c_void_p(ws_ptr), 4096, C.byref(o), _lib.stream_ptr())
    assert rc != 0 and b"workspace too small" in lib.rgbm_last_error()
    ab = _net("bf16", options={"upconv": 4}, dropout=P, dropout_seed=SEED)
    with pytest.raises(_lib.RgbmError, match="upconv"):
        _sampled(ab, inp, 2)
    _plain(net, inp)                                           # pose 1: the refused calls drew nothing
    np.testing.assert_array_equal(net.dropout_masks(1).cpu().numpy(), dropout_ref.masks(P, SEED, 1, first_pose=1))
    # the baseline network
    base = AdaPoseNet(synth.baseline_state_dict(seed=0), dtype="bf16", arch="baseline")
    before = _plain(base, inp)
    with pytest.raises(_lib.RgbmError, match="baseline"):
        _sampled(base, inp, 2)
    after = _plain(base, inp)
    for k in before:
        np.testing.assert_array_equal(before[k], after[k], err_msg=k)


# ------------------------------------------------------------------------------------------------------------------ 3. statistics kernels
def _assert_box_stats(boxes, ok):
    """Device against twin: count exact, the same NaN pattern, values within 1e-10 relative to the largest coordinate (both sides
    float64 in the same order: the bound between device and oracle of the project's fp64 tails)."""
    ref = samples.box_stats_ref(boxes, ok)
    got = {k: v.cpu().numpy() for k, v in samples.box_stats(boxes, ok).items()}
    torch.cuda.synchronize()
    big = float(np.abs(boxes[np.isfinite(boxes)]).max())
    np.testing.assert_array_equal(got["count"], ref["count"])
    assert got["count"].dtype == np.int32
    for k in samples.BOX_KEYS[1:]:
        assert got[k].shape == ref[k].shape and got[k].dtype == np.float64, k
        np.testing.assert_array_equal(np.isnan(got[k]), np.isnan(ref[k]), err_msg=k)
        err = np.nanmax(np.abs(got[k] - ref[k]), initial=0.0)
        print(f"box_stats {k}: max abs err {err:.3e} (bound {1e-10 * big:.3e})")
        assert err <= 1e-10 * big, (k, err)
    return got


def test_box_stats_kernel_on_the_hand_cases():
    boxes, ok, counts = cases.hand_boxes()
    got = _assert_box_stats(boxes, ok)
    np.testing.assert_array_equal(got["count"], counts)
    assert all(np.isnan(got[k][2]).all() for k in samples.BOX_KEYS[1:])
    got = _assert_box_stats(*cases.rotated_boxes())
    for b in range(3):
        for e in range(3):
            want = 0.0 if e == b else cases.THETA
            assert abs(got["axis_spread_deg"][b, e] - want) < 1e-10, (b, e, got["axis_spread_deg"][b, e])
    got = _assert_box_stats(*cases.single_boxes())
    np.testing.assert_array_equal(got["count"], [1, 1])
    for k in ("bbox_std", "center_cov", "extent_std", "axis_spread_deg"):
        np.testing.assert_array_equal(got[k], np.zeros_like(got[k]), err_msg=k)


def test_box_stats_kernel_on_random_boxes():
    boxes, ok = cases.random_boxes(n=5, S=7, seed=0, extent=10.0)
    got = _assert_box_stats(boxes, ok)
    np.testing.assert_array_equal(got["count"], [6, 6, 7, 5, 6])
    _assert_box_stats(*cases.random_boxes(n=3, S=64, seed=1))          # the most samples a call takes
    _assert_box_stats(*cases.random_boxes(n=2, S=1, seed=2))


def test_box_stats_refuses_out_of_range_calls():
    with pytest.raises(ValueError, match="S <= 64"):
        samples.box_stats(np.zeros((65, 1, 8, 3)), np.ones((65, 1)))
    from rgbmanip_amd import _lib
    lib = _lib.load()
    z = torch.zeros(64, dtype=torch.float64, device="cuda")
    for n, S in ((1, 65), (1, 0), (65536, 1), (0, 1)):
        assert lib.rgbm_sample_box_stats(_lib.ptr(z), _lib.ptr(z), n, S, *[_lib.ptr(z)] * 8, _lib.stream_ptr()) != 0
        assert b"sample_box_stats" in lib.rgbm_last_error()
    assert lib.rgbm_sample_point_stats(_lib.ptr(z), 1, 0, 1, _lib.ptr(z), _lib.ptr(z), _lib.stream_ptr()) != 0


@pytest.mark.parametrize("shape", [(7, 5, 37), (3, 2, 1024, 3), (1, 3, 5), (64, 1, 3), (2, 1, 600001)])
def test_point_stats_kernel_equals_the_twin(shape):
    """Equal to the twin after the twin's single rounding to float32.  Shapes: an odd element count below one workgroup, the
    estimator's NOCS rows, one sample, 64 samples, and more elements than the grid has threads (2048 x 256: the stride loop)."""
    rng = np.random.default_rng(sum(shape))
    x = (rng.normal(size=shape) * rng.choice([1e-3, 1.0, 50.0], size=shape)).astype(np.float32)
    x.reshape(shape[0], -1)[0, 1] = np.nan
    x.reshape(shape[0], -1)[-1, 2] = np.inf
    mean, std = samples.point_stats(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    rm, rs = samples.point_stats_ref(x)
    assert mean.dtype == torch.float32 and tuple(mean.shape) == shape[1:] and tuple(std.shape) == shape[1:]
    np.testing.assert_array_equal(mean.cpu().numpy(), rm)
    np.testing.assert_array_equal(std.cpu().numpy(), rs)
    assert np.isnan(rm.reshape(-1)[1]) and np.isnan(rs.reshape(-1)[1]) and np.isnan(rs.reshape(-1)[2])


# ------------------------------------------------------------------------------------------------------------------ 4. estimate_samples
N, H, W, S_EST = 2, 480, 640, 3
STAT_KEYS = ("bbox_std", "center_cov", "extent_mean", "extent_std", "axis_spread_deg")


def _frames():
    rng = np.random.default_rng(2)
    rgb = rng.random((N, H, W, 3), dtype=np.float32)
    yy, xx = np.mgrid[0:H, 0:W]
    mask = np.zeros((N, H, W), np.uint8)
    mask[0] = (((yy - 250) / 120.0) ** 2 + ((xx - 300) / 170.0) ** 2) < 1.0
    mask[1] = (((yy - 200) / 90.0) ** 2 + ((xx - 350) / 110.0) ** 2) < 1.0
    K = np.tile(np.array([[439.31, 0, 320.0], [0, 439.31, 240.0], [0, 0, 1.0]]), (N, 1, 1))
    inp = synth.adapose_inputs(N, seed=2)
    return rgb, mask, K, inp["E1"].astype(np.float64), inp["E2"].astype(np.float64)


@pytest.fixture(scope="module")
def estimator():
    from rgbmanip_amd.config import ADAPOSE_CFGS
    from rgbmanip_amd.estimator import AdaPoseEstimator_v5
    cfg = dict(ADAPOSE_CFGS["adapose_cabinet"], load=False, hip_prepare="device", hip_dropout=P, hip_dropout_seed=SEED)
    return AdaPoseEstimator_v5(None, cfg, None, state_dict=synth.adapose_state_dict(seed=0, prefix="module."), dtype="bf16x3")


def _check_result(r, n, S):
    shapes = {"bbox": (n, 8, 3), "bbox_samples": (n, S, 8, 3), "count": (n,), "bbox_std": (n, 8, 3), "center_cov": (n, 3, 3), "extent_mean": (n, 3),
              "extent_std": (n, 3), "axis_spread_deg": (n, 3), "nocs_mean": (n, 1024, 3), "nocs_std": (n, 1024, 3), "depth_mean": (n, 1024),
              "depth_std": (n, 1024), "valid": (n,)}
    assert set(r) == set(shapes)
    for k, shp in shapes.items():
        assert tuple(r[k].shape) == shp, (k, r[k].shape)
    assert r["bbox"].dtype == np.float64 and r["count"].dtype == np.int32 and r["valid"].dtype == np.int32 and r["nocs_mean"].dtype == np.float32


@pytest.mark.parametrize("frames", ["float32", "uint8"])
def test_estimate_samples_end_to_end(estimator, frames):
    from rgbmanip_amd.cloud import DEFAULT_BBOX
    est = estimator
    rgb, mask, K, E1, E2 = _frames()
    if frames == "uint8":
        rgb = np.round(rgb * 255).astype(np.uint8)
    rgb2, mask2 = rgb[:, :, ::-1].copy(), mask[:, :, ::-1].copy()
    with _generic_kernels_only():
        est.estimator.set_dropout(P, SEED)
        singles = [est.estimate(K, rgb, mask, E1, rgb2, mask2, E2) for _ in range(S_EST)]
        est.estimator.set_dropout(P, SEED)
        r = est.estimate_samples(K, rgb, mask, E1, rgb2, mask2, E2, samples=S_EST)
        est.estimator.set_dropout(P, SEED)
        d = est.estimate_samples_device(K, torch.from_numpy(rgb).cuda(), torch.from_numpy(mask).cuda(), E1, torch.from_numpy(rgb2).cuda(),
                                        torch.from_numpy(mask2).cuda(), E2, samples=S_EST)
        torch.cuda.synchronize()
    _check_result(r, N, S_EST)
    for s in range(S_EST):
        np.testing.assert_array_equal(r["bbox_samples"][:, s], singles[s], err_msg=f"sample {s}")
        assert not np.array_equal(singles[s], np.repeat(DEFAULT_BBOX[None], N, axis=0))
    assert not np.array_equal(singles[0], singles[1])
    np.testing.assert_array_equal(r["count"], [S_EST] * N)
    np.testing.assert_array_equal(r["valid"], [1] * N)
    ref = samples.box_stats_ref(r["bbox_samples"].transpose(1, 0, 2, 3), np.ones((S_EST, N)))
    big = float(np.abs(r["bbox_samples"]).max())
    for k, want in [("bbox", ref["bbox_mean"])] + [(k, ref[k]) for k in STAT_KEYS]:
        assert np.abs(r[k] - want).max() <= 1e-10 * big, k
    assert (r["bbox_std"] > 0).all() and np.isfinite(r["nocs_mean"]).all() and np.isfinite(r["depth_mean"]).all()
    assert (r["nocs_std"] > 0).any() and (r["depth_std"] > 0).any()
    for k in r:
        assert isinstance(d[k], torch.Tensor) and d[k].is_cuda, k
        np.testing.assert_array_equal(d[k].cpu().numpy(), r[k], err_msg=k)


@pytest.mark.parametrize("frames", ["float32", "uint8"])
def test_estimate_samples_window_upload_gives_the_same_numbers(estimator, frames):
    """hip_upload: "windows" (only each frame's crop window is uploaded) on the same net: every array of the result, bit for bit."""
    from rgbmanip_amd.estimator import AdaPoseEstimator_v5
    rgb, mask, K, E1, E2 = _frames()
    if frames == "uint8":
        rgb = np.round(rgb * 255).astype(np.uint8)
    rgb2, mask2 = rgb[:, :, ::-1].copy(), mask[:, :, ::-1].copy()
    win = AdaPoseEstimator_v5(None, dict(estimator.cfg, hip_upload="windows"), None, net=estimator.estimator)
    got = []
    for est in (estimator, win):
        est.estimator.set_dropout(P, SEED)
        got.append(est.estimate_samples(K, rgb, mask, E1, rgb2, mask2, E2, samples=2))
    assert 0 < win.upload_bytes_last_call < estimator.upload_bytes_last_call
    for k in got[0]:
        np.testing.assert_array_equal(got[0][k], got[1][k], err_msg=k)
    np.testing.assert_array_equal(got[1]["count"], [2, 2])


def test_estimate_samples_chunks_draw_their_own_mask_blocks(estimator, monkeypatch):
    """More poses than fit one forward_samples call (here: room for 3 network poses, S = 3, so one pose per chunk): every chunk is a call
    of its own, i.e. the result rows equal those of one call per pose, in order, on the running mask sequence."""
    rgb, mask, K, E1, E2 = _frames()
    dev = lambda x: torch.from_numpy(x).cuda()      # noqa: E731
    a = (dev(rgb), dev(mask), dev(rgb[:, :, ::-1].copy()), dev(mask[:, :, ::-1].copy()))
    call = lambda lo, hi, **kw: estimator.estimate_samples_device(K[lo:hi], a[0][lo:hi], a[1][lo:hi], E1[lo:hi], a[2][lo:hi], a[3][lo:hi], E2[lo:hi],      # noqa: E731
                                                                  samples=S_EST, **kw)
    estimator.estimator.set_dropout(P, SEED)
    parts = [call(0, 1), call(1, 2, frame0=1)]
    monkeypatch.setattr(estimator, "_SAMPLE_ROWS", S_EST)
    estimator.estimator.set_dropout(P, SEED)
    whole = call(0, N)
    torch.cuda.synchronize()
    for k in whole:
        np.testing.assert_array_equal(whole[k].cpu().numpy(), np.concatenate([p[k].cpu().numpy() for p in parts]), err_msg=k)
    np.testing.assert_array_equal(estimator.estimator.dropout_masks(S_EST).cpu().numpy(), dropout_ref.masks(P, SEED, S_EST, first_pose=S_EST))


def test_estimate_samples_empty_mask_and_v4(estimator):
    from rgbmanip_amd.cloud import DEFAULT_BBOX
    from rgbmanip_amd.config import adapose_cfg
    from rgbmanip_amd.estimator import AdaPoseEstimator_v4
    rgb, mask, K, E1, E2 = _frames()
    mask = mask.copy()
    mask[1] = 0
    rgb2, mask2 = rgb[:, :, ::-1].copy(), mask[:, :, ::-1].copy()
    r = estimator.estimate_samples(K, rgb, mask, E1, rgb2, mask2, E2, samples=S_EST)
    _check_result(r, N, S_EST)
    np.testing.assert_array_equal(r["count"], [S_EST, 0])
    np.testing.assert_array_equal(r["valid"], [1, 0])
    np.testing.assert_array_equal(r["bbox"][1], DEFAULT_BBOX)
    np.testing.assert_array_equal(r["bbox_samples"][1], np.repeat(DEFAULT_BBOX[None], S_EST, axis=0))
    for k in STAT_KEYS + ("nocs_mean", "nocs_std", "depth_mean", "depth_std"):
        assert np.isnan(r[k][1]).all() and np.isfinite(r[k][0]).all(), k
    # v4 with direct_regression (the regressed tail) on the same net: it runs and counts every sample of the valid pose
    cfg = dict(adapose_cfg(load=False, name="adapose_v4"), hip_prepare="device", hip_dropout=P, hip_dropout_seed=SEED, direct_regression=True)
    v4 = AdaPoseEstimator_v4(None, cfg, None, net=estimator.estimator)
    r4 = v4.estimate_samples(K, rgb, mask, E1, rgb2, mask2, E2, samples=2)
    _check_result(r4, N, 2)
    np.testing.assert_array_equal(r4["count"], [2, 0])
    assert np.isfinite(r4["bbox"]).all() and not np.array_equal(r4["bbox_samples"][0, 0], r4["bbox_samples"][0, 1])
