"""-m gpu: cfg hip_upload: "windows" — `rgbm_prepare_inputs_windows` on host-packed crop windows against `rgbm_prepare_inputs_opt` on
the whole frames, and `estimate()` with the window upload against the whole-frame upload.  Everything is compared bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import postproc_ref  # noqa: E402
from rgbmanip_amd import _lib, synth, upload  # noqa: E402

H, W = 480, 640
SEED, FRAME0 = 77, 3
GUARD = 4099                          # pixels of guard in front of, between and behind the two views' packed windows
_CACHE = {}


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _case():
    """Six 480 x 640 frames of seeded noise per view.  View 1: one pixel at (0, 0), one at (479, 639), synth.crop_frames' ellipse
    (a 360 window, more than 1024 mask pixels at S = 224) and sliver (an 80 window shifted back into the frame), rows 5..474 x
    columns 100..139 (the 440 clamp: the window is smaller than the mask), an empty mask.  View 2: the same mirrored left to right.
    Built once, read by every test, never written."""
    if "case" not in _CACHE:
        g = np.random.default_rng(11)
        crop = synth.crop_frames(seed=0)[1]
        mask = np.zeros((6, H, W), np.uint8)
        mask[0, 0, 0] = mask[1, H - 1, W - 1] = 1
        mask[2], mask[3] = crop[0], crop[1]
        mask[4, 5:475, 100:140] = 1
        u8 = g.integers(0, 256, (6, H, W, 3), dtype=np.uint8)
        f32 = g.random((6, H, W, 3), dtype=np.float32)
        K = np.tile(np.array([[439.31, 0, 320.0], [0, 439.31, 240.0], [0, 0, 1.0]]), (6, 1, 1))
        K[:, 0, 2] += np.arange(6) * 1.5
        mir = lambda a: np.ascontiguousarray(a[:, :, ::-1])      # noqa: E731
        views = [dict(u8=u8, f32=f32, mask=mask), dict(u8=mir(u8), f32=mir(f32), mask=mir(mask))]
        for v in views:
            v["window"], v["valid"] = upload.mask_windows(v["mask"])
            v["offset"], v["total"] = upload.window_offsets(v["window"])
            v["dev"] = {k: _cuda(v[k]) for k in ("u8", "f32", "mask", "window", "valid", "offset")}
        assert views[0]["window"].tolist() == [[0, 40, 0, 40], [440, 480, 600, 640], [70, 430, 120, 480], [160, 240, 560, 640], [19, 459, 0, 440],
                                               [0, 40, 0, 40]] and views[0]["valid"].tolist() == [1, 1, 1, 1, 1, 0]
        assert tuple(views[0]["window"][4]) == postproc_ref.get_bbox((5, 100, 474, 139))
        _CACHE["case"] = dict(views=views, K=_cuda(K))
    return _CACHE["case"]


def _packed(kind):
    """Both views' windows packed by the host into ONE device allocation per array: guard | view 1 | guard | view 2 | guard, the guards
    NaN (float32 pixels) or 0xFF (byte pixels, mask bytes).  Returns (pix, mask_pix, [pixel offset of view v's first window])."""
    key = ("packed", kind)
    if key not in _CACHE:
        views = _case()["views"]
        px = np.float32 if kind == "f32" else np.uint8
        size = 3 * GUARD + views[0]["total"] + views[1]["total"]
        pix = np.full(3 * size, np.nan if kind == "f32" else 0xFF, dtype=px)
        mpix = np.full(size, 0xFF, dtype=np.uint8)
        bases, at = [], GUARD
        for v in views:
            upload.pack_windows(pix[3 * at:], mpix[at:], v[kind], v["mask"], 0, 6, v["window"], v["offset"])
            bases.append(at)
            at += v["total"] + GUARD
        assert at == size
        if kind == "f32":
            assert np.isnan(pix[:3 * GUARD]).all() and np.isnan(pix[3 * (bases[1] - GUARD): 3 * bases[1]]).all() and np.isnan(pix[-3 * GUARD:]).all()
            assert not np.isnan(pix[3 * bases[0]: 3 * (bases[0] + views[0]["total"])]).any()
        _CACHE[key] = (_cuda(pix), _cuda(mpix), bases)
    return _CACHE[key]


def _outputs(N, S, P, fill=None):
    out = dict(img=torch.empty(N, 3, S, S, dtype=torch.float32, device="cuda"), choose=torch.empty(N, P, dtype=torch.int32, device="cuda"),
               pts2d=torch.empty(N, P, 2, dtype=torch.float32, device="cuda"), Kcrop=torch.empty(N, 3, 3, dtype=torch.float64, device="cuda"),
               valid=torch.empty(N, dtype=torch.int32, device="cuda"))
    if fill is not None:
        for t in out.values():
            t.fill_(fill)
    return out, torch.empty(N * S * S, dtype=torch.uint8, device="cuda")


def _windows_call(pix_ptr, mask_ptr, d, K, pixel_type, normalize, S, P, fill=None, window="window"):
    out, scratch = _outputs(6, S, P, fill)
    p = _lib.ptr
    rc = _lib.load().rgbm_prepare_inputs_windows(C.c_void_p(pix_ptr), pixel_type, normalize, C.c_void_p(mask_ptr), p(d["offset"]),
                                                 p(d[window]) if window else None, p(d["valid"]), p(K), FRAME0, 6, H, W, S, P, SEED, p(out["img"]),
                                                 p(out["choose"]), p(out["pts2d"]), p(out["Kcrop"]), p(out["valid"]), p(scratch), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, out


# ------------------------------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("S,P", [(32, 64), (224, 1024)])
@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("pixel_type", [0, 1])
def test_packed_windows_equal_whole_frames(pixel_type, normalize, S, P):
    """img, choose, pts2d, Kcrop and valid of rgbm_prepare_inputs_windows on the host-packed buffers (between NaN / 0xFF guards) equal
    those of rgbm_prepare_inputs_opt on the whole frames, for both views and every frame, the empty mask's included; the windows the
    device derives are the ones the host packed."""
    c = _case()
    kind = "u8" if pixel_type else "f32"
    pix, mpix, bases = _packed(kind)
    p = _lib.ptr
    for v, view in enumerate(c["views"]):
        d = view["dev"]
        ref, scratch = _outputs(6, S, P)
        win = torch.empty(6, 4, dtype=torch.int32, device="cuda")
        _lib.check(_lib.load().rgbm_prepare_inputs_opt(p(d[kind]), pixel_type, normalize, p(d["mask"]), p(c["K"]), None, FRAME0, 6, H, W, S, P, SEED,
                                                       p(ref["img"]), p(ref["choose"]), p(ref["pts2d"]), p(ref["Kcrop"]), p(win), p(ref["valid"]),
                                                       p(scratch), _lib.stream_ptr()), "rgbm_prepare_inputs_opt")
        rc, got = _windows_call(pix.data_ptr() + 3 * bases[v] * pix.element_size(), mpix.data_ptr() + bases[v], d, c["K"], pixel_type, normalize, S, P)
        assert rc == 0, _lib.load().rgbm_last_error()
        assert torch.equal(win, d["window"]), v
        for k in ("img", "choose", "pts2d", "Kcrop", "valid"):
            assert got[k].dtype == ref[k].dtype and torch.equal(got[k], ref[k]), (v, k)
        assert torch.isfinite(got["img"]).all()
        assert ref["valid"][5] == 0 and ref["valid"][2] == 1 and torch.equal(ref["Kcrop"][5], torch.eye(3, dtype=torch.float64, device="cuda"))
        if S == 224:                                             # the ellipse takes the hash-subset branch, the sliver wrap padding
            assert len(torch.unique(ref["choose"][2])) == P and 1 < len(torch.unique(ref["choose"][3])) < P
            assert ref["valid"].tolist() == [1, 1, 1, 1, 1, 0]


def test_argument_errors_launch_nothing():
    """pixel_type / normalize outside {0, 1}, a null table, frames below 440 and a negative frame0: an error code, outputs keep their fill."""
    c = _case()
    pix, mpix, bases = _packed("f32")
    d = c["views"][0]["dev"]
    at = (pix.data_ptr() + 12 * bases[0], mpix.data_ptr() + bases[0])
    lib = _lib.load()
    for pt, nm in ((2, 1), (-1, 0), (0, 2), (1, -1)):
        rc, got = _windows_call(*at, d, c["K"], pt, nm, 32, 64, fill=7)
        assert rc != 0 and b"pixel_type" in lib.rgbm_last_error(), (pt, nm)
        assert all((t == 7).all() for t in got.values())
    rc, got = _windows_call(*at, d, c["K"], 0, 1, 32, 64, fill=7, window=None)
    assert rc != 0 and all((t == 7).all() for t in got.values())
    rc, got = _windows_call(0, at[1], d, c["K"], 0, 1, 32, 64, fill=7)
    assert rc != 0 and all((t == 7).all() for t in got.values())
    out, scratch = _outputs(6, 32, 64, 7)
    p = _lib.ptr
    tail = (p(out["img"]), p(out["choose"]), p(out["pts2d"]), p(out["Kcrop"]), p(out["valid"]), p(scratch), _lib.stream_ptr())
    head = (C.c_void_p(at[0]), 0, 1, C.c_void_p(at[1]), p(d["offset"]), p(d["window"]), p(d["valid"]), p(c["K"]))
    for frame0, N, h, w, S, P in ((-1, 6, H, W, 32, 64), (0, 0, H, W, 32, 64), (0, 6, 439, W, 32, 64), (0, 6, H, 439, 32, 64), (0, 6, H, W, 257, 64),
                                  (0, 6, H, W, 32, 0)):
        assert lib.rgbm_prepare_inputs_windows(*head, frame0, N, h, w, S, P, SEED, *tail) != 0, (frame0, N, h, w, S, P)
    torch.cuda.synchronize()
    assert all((t == 7).all() for t in out.values())


# ------------------------------------------------------------------------------------------------------------------ 2. estimate()
def _net():
    if "net" not in _CACHE:
        from rgbmanip_amd.adapose import AdaPoseNet
        _CACHE["net"] = AdaPoseNet(synth.adapose_state_dict(seed=0, prefix="module."), dtype="bf16", options={"view2_heads": 1})
    return _CACHE["net"]


def _scene():
    """Three poses of float64 host frames with elliptical masks (more than 1024 resized mask pixels each); pose 1's view-2 mask is empty."""
    if "scene" not in _CACHE:
        g = np.random.default_rng(3)
        n = 3
        yy, xx = np.mgrid[0:H, 0:W]
        K = np.tile(np.array([[439.31, 0, 320.0], [0, 439.31, 240.0], [0, 0, 1.0]])[None], (n, 1, 1))
        base = synth.adapose_inputs(n, seed=0)
        f1 = np.clip(0.5 + 0.25 * np.cos(xx / 37.0)[None, :, :, None] + 0.2 * g.random((n, H, W, 3)), 0, 1)
        f2 = np.clip(0.5 + 0.25 * np.sin(yy / 29.0)[None, :, :, None] + 0.2 * g.random((n, H, W, 3)), 0, 1)
        m1 = np.stack([((yy - 240) / 60.0) ** 2 + ((xx - 300 - 10 * i) / 90.0) ** 2 <= 1 for i in range(n)])
        m2 = np.stack([((yy - 250) / 70.0) ** 2 + ((xx - 340 + 10 * i) / 80.0) ** 2 <= 1 for i in range(n)]).astype(np.float64)
        m2[1] = 0
        assert f1.dtype == np.float64 and m1.dtype == np.bool_
        q = lambda f: np.rint(f * 255.0).astype(np.uint8)      # noqa: E731
        _CACHE["scene"] = dict(K=K, E1=base["E1"].astype(np.float64), E2=base["E2"].astype(np.float64), f1=f1, f2=f2, u1=q(f1), u2=q(f2), m1=m1, m2=m2)
    return _CACHE["scene"]


def _estimators(cls="v5", task="cabinet", **kw):
    """The same cfg with hip_upload: "frames" and "windows", on the shared bf16 net."""
    from rgbmanip_amd.config import ADAPOSE_CFGS, adapose_cfg
    from rgbmanip_amd.estimator import AdaPoseEstimator_v4, AdaPoseEstimator_v5
    base = adapose_cfg(task, load=False, name="adapose_v4") if cls == "v4" else ADAPOSE_CFGS["adapose_cabinet"]
    make = AdaPoseEstimator_v4 if cls == "v4" else AdaPoseEstimator_v5
    cfg = dict(base, load=False, hip_dtype="bf16", hip_prepare="device", hip_prepare_seed=9, **kw)
    return [make(None, dict(cfg, hip_upload=mode), None, net=_net()) for mode in ("frames", "windows")]


def _window_bytes(masks, px_bytes):
    return sum(int(((w[:, 1] - w[:, 0]) * (w[:, 3] - w[:, 2])).sum()) for w in (upload.mask_windows(np.asarray(m) != 0)[0] for m in masks)) * (3 * px_bytes + 1)


def _run(est, frames="f"):
    s = _scene()
    return est.estimate(s["K"], s[frames + "1"], s["m1"], s["E1"], s[frames + "2"], s["m2"], s["E2"])


SETTINGS = {"unchunked": dict(hip_upload_chunk=32), "three_chunks": dict(hip_upload_chunk=1), "uint8_frames": dict(hip_upload_chunk=32),
            "uint8_three_chunks": dict(hip_upload_chunk=1), "content_cache": dict(hip_feature_cache="content"),
            "content_cache_three_chunks": dict(hip_feature_cache="content", hip_upload_chunk=1),
            "v4_pots": dict(cls="v4", task="pots"), "v4_one_door_cabinet": dict(cls="v4", task="one_door_cabinet"),
            "pnp_branch": dict(direct_regression=False, use_depth=False)}


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_estimate_boxes_equal_the_whole_frame_upload(setting):
    """Boxes of hip_upload: "windows" against "frames" (same cfg otherwise, same chunking), three poses of host frames; pose 1 has an
    empty view-2 mask and returns the default box.  upload_bytes_last_call is the formula of either mode; byte frames are counted in
    frames_u8_native; with the content cache a second identical call computes no feature view."""
    from rgbmanip_amd.estimator import DEFAULT_BBOX
    s, n = _scene(), 3
    frames = "u" if setting.startswith("uint8") else "f"
    px = 1 if frames == "u" else 4
    ref, est = _estimators(**SETTINGS[setting])
    assert (ref.upload_mode, est.upload_mode) == ("frames", "windows")
    if setting == "pnp_branch":
        with pytest.warns(RuntimeWarning):
            want = _run(ref, frames)
        with pytest.warns(RuntimeWarning):
            got = _run(est, frames)
    else:
        want, got = _run(ref, frames), _run(est, frames)
    assert got.shape == (n, 8, 3) and got.dtype == np.float64 and np.array_equal(got, want)
    assert np.array_equal(got[1], DEFAULT_BBOX)
    if setting != "pnp_branch":                                  # (the PnP tail's RANSAC may reject a pose of a seeded-weights net)
        assert np.isfinite(got).all() and not np.array_equal(got[0], DEFAULT_BBOX) and not np.array_equal(got[2], DEFAULT_BBOX)
    assert ref.upload_bytes_last_call == 2 * n * H * W * (3 * px + 1) and ref.upload_table_bytes_last_call == 0
    assert est.upload_bytes_last_call == _window_bytes((s["m1"], s["m2"]), px) < ref.upload_bytes_last_call // 3
    assert est.upload_table_bytes_last_call > 0
    assert est.frames_u8_native == ref.frames_u8_native == (2 * n if frames == "u" else 0)
    if "content_cache" in setting:
        seen = est.feature_views_computed
        assert 0 < seen <= 2 * n and seen == ref.feature_views_computed and est.feature_cache_bypassed == 0
        again = _run(est, frames)
        assert est.feature_views_computed == seen and np.array_equal(again, want)


def test_cuda_frames_take_the_whole_frame_path():
    """Any of the four arrays on the device: hip_upload: "windows" falls back to today's path (nothing to pack on the host)."""
    s = _scene()
    ref, est = _estimators()
    want = _run(ref)
    got = est.estimate(s["K"], torch.from_numpy(s["f1"]).float().cuda(), s["m1"], s["E1"], torch.from_numpy(s["f2"]).float().cuda(), s["m2"], s["E2"])
    assert np.array_equal(got, want)
    assert est.upload_bytes_last_call == 2 * 3 * H * W and est._wring is None       # the two host masks, a byte per pixel
