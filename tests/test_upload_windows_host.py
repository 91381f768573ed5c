"""CPU-only: the host side of cfg hip_upload: "windows" — `upload.mask_windows` against the oracle's get_bbox, the packed layout of
`upload.pack_windows` / `upload.WindowRing`, the byte accounting of `estimator.upload_bytes_last_call` on a stubbed device side, the
cfg validation and the C ABI of `rgbm_prepare_inputs_windows`.  Everything is compared exactly."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from oracle import postproc_ref
from rgbmanip_amd import synth, upload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 480, 640


def _named_masks():
    """name -> (mask [H,W] uint8, expected window or None = whatever the oracle says, valid)"""
    crop = synth.crop_frames(seed=0)[1]
    one = lambda y, x: np.pad(np.ones((1, 1), np.uint8), ((y, H - 1 - y), (x, W - 1 - x)))      # noqa: E731
    tall = np.zeros((H, W), np.uint8)
    tall[5:475, 100:140] = 1
    return {"pixel_0_0": (one(0, 0), None, 1), "pixel_479_639": (one(H - 1, W - 1), None, 1),
            "crop_frames_0": (crop[0], (70, 430, 120, 480), 1), "crop_frames_1": (crop[1], (160, 240, 560, 640), 1),
            "clamp_440": (tall, None, 1), "empty": (np.zeros((H, W), np.uint8), (0, 40, 0, 40), 0)}


def _oracle_window(mask):
    ys, xs = np.nonzero(mask)
    return tuple(int(v) for v in postproc_ref.get_bbox((ys.min(), xs.min(), ys.max(), xs.max())))


def _check_square_inside(window):
    h, w = window[:, 1] - window[:, 0], window[:, 3] - window[:, 2]
    assert (h == w).all() and (h % 40 == 0).all() and (h >= 40).all() and (h <= 440).all()
    assert (window[:, 0] >= 0).all() and (window[:, 2] >= 0).all() and (window[:, 1] <= H).all() and (window[:, 3] <= W).all()


# ------------------------------------------------------------------------------------------------------------------ 1. mask_windows
def test_mask_windows_equals_get_bbox_on_random_rectangles():
    """2 000 seeded rectangles in 480 x 640 (from single pixels to the whole frame), in batches of 100 masks."""
    g = np.random.default_rng(20)
    ya, yb = np.sort(g.integers(0, H, (2, 2000)), axis=0)
    xa, xb = np.sort(g.integers(0, W, (2, 2000)), axis=0)
    ya[:4], yb[:4], xa[:4], xb[:4] = (0, 0, H - 1, 7), (H - 1, 0, H - 1, 7), (0, 0, W - 1, 9), (W - 1, W - 1, W - 1, 9)
    sides = set()
    for lo in range(0, 2000, 100):
        mask = np.zeros((100, H, W), np.uint8)
        for i in range(100):
            mask[i, ya[lo + i]:yb[lo + i] + 1, xa[lo + i]:xb[lo + i] + 1] = 1 + (i % 3) * 127      # any non-zero value is object
        window, valid = upload.mask_windows(mask)
        assert window.dtype == np.int32 and valid.dtype == np.int32 and window.shape == (100, 4) and valid.tolist() == [1] * 100
        want = [postproc_ref.get_bbox((ya[lo + i], xa[lo + i], yb[lo + i], xb[lo + i])) for i in range(100)]
        assert window.tolist() == [list(map(int, w)) for w in want], lo
        _check_square_inside(window)
        sides.update((window[:, 1] - window[:, 0]).tolist())
    assert sides == set(range(40, 441, 40))                      # every window size occurs


def test_mask_windows_named_cases():
    cases = _named_masks()
    window, valid = upload.mask_windows(np.stack([m for m, _, _ in cases.values()]))
    _check_square_inside(window)
    for (name, (mask, want, ok)), got, v in zip(cases.items(), window.tolist(), valid.tolist()):
        assert v == ok, name
        if ok:
            assert tuple(got) == _oracle_window(mask), name
        if want is not None:
            assert tuple(got) == want, name
    tall = dict(zip(cases, window.tolist()))["clamp_440"]
    assert tall[1] - tall[0] == 440 < 470                        # the 440 clamp: the window is smaller than the mask
    # bool masks are the same bytes; a row length that is no multiple of 8 and a non-contiguous view take the plain reduction
    stack = np.stack([m for m, _, _ in cases.values()])
    assert np.array_equal(upload.mask_windows(stack.astype(bool))[0], window)
    odd = np.zeros((2, 450, 445), np.uint8)
    odd[0, 400:449, 3:5] = 1
    odd[1, 7, 444] = 1
    w_odd, v_odd = upload.mask_windows(odd)
    assert w_odd.tolist() == [[370, 450, 0, 80], [0, 40, 405, 445]] and v_odd.tolist() == [1, 1]
    assert np.array_equal(upload.mask_windows(np.pad(stack, ((0, 0), (0, 0), (0, 8)))[:, :, :W])[0], window)
    # the pieces the upload threads look through give the same tables
    many = np.concatenate([stack, stack[::-1]] * 3)
    w_pool, v_pool = upload.gather_windows(upload.mask_windows_pooled(many, upload._host_pool()))
    assert len(upload.mask_windows_pooled(many, upload._host_pool())) > 1
    assert np.array_equal(w_pool, upload.mask_windows(many)[0]) and np.array_equal(v_pool, upload.mask_windows(many)[1])
    with pytest.raises(ValueError, match="440"):
        upload.mask_windows(np.ones((1, 400, 640), np.uint8))
    with pytest.raises(TypeError):
        upload.mask_windows(np.ones((1, H, W), np.float64))


# ------------------------------------------------------------------------------------------------------------------ 2. pack_windows
def _frames(dtype, n=3):
    """crop_frames' two frames and one with an empty mask: (frames [3,H,W,3] of dtype, mask [3,H,W] uint8 with 0 / 1 / 200)"""
    u8, mask, _ = synth.crop_frames(seed=0)
    u8 = np.concatenate([u8, u8[:1, ::-1]])
    mask = np.concatenate([mask, np.zeros_like(mask[:1])])
    mask[0] *= 200
    if dtype == np.uint8:
        return u8, mask
    g = np.random.default_rng(8)
    return (u8.astype(np.float64) / 255.0 + g.uniform(0, 1e-3, u8.shape)).astype(dtype), mask        # float64 values that float32 rounds


def _unpack(pix, mpix, window, offset, f):
    rmin, rmax, cmin, cmax = window[f]
    h, w, off = rmax - rmin, cmax - cmin, int(offset[f])
    return pix[3 * off: 3 * (off + h * w)].reshape(h, w, 3), mpix[off: off + h * w].reshape(h, w)


@pytest.mark.parametrize("frame_dtype", [np.float64, np.float32, np.uint8])
@pytest.mark.parametrize("mask_dtype", [np.bool_, np.uint8, np.float64])
def test_pack_windows_round_trip(frame_dtype, mask_dtype):
    frames, m8 = _frames(frame_dtype)
    masks = (m8 != 0) if mask_dtype == np.bool_ else m8.astype(mask_dtype)
    window, valid = upload.mask_windows(m8)
    offset, total = upload.window_offsets(window)
    area = (window[:, 1] - window[:, 0]) * (window[:, 3] - window[:, 2])
    assert valid.tolist() == [1, 1, 0] and offset.dtype == np.int64
    assert offset.tolist() == [0, int(area[0]), int(area[0] + area[1])] and total == int(area.sum()) == 136000 + 1600
    px = np.uint8 if frame_dtype == np.uint8 else np.float32
    for pool in (None, upload._host_pool()):
        guard = 7
        pix = np.full(3 * total + guard, 99, dtype=px)
        mpix = np.full(total + guard, 99, dtype=np.uint8)
        for fut in upload.pack_windows(pix, mpix, frames, masks, 0, 3, window, offset, pool):
            fut.result()
        for f in range(3):
            rmin, rmax, cmin, cmax = window[f]
            got, gotm = _unpack(pix, mpix, window, offset, f)
            want = frames[f, rmin:rmax, cmin:cmax]
            assert got.dtype == px and np.array_equal(got, want if px == np.uint8 else want.astype(np.float32)), f
            assert np.array_equal(gotm, (masks[f, rmin:rmax, cmin:cmax] != 0).astype(np.uint8)), f
        assert (pix[3 * total:] == 99).all() and (mpix[total:] == 99).all()          # nothing behind the used prefix
    # a sub-range: frames [1, 3) with tables of their own
    off2, tot2 = upload.window_offsets(window[1:])
    pix, mpix = np.zeros(3 * tot2, dtype=px), np.zeros(tot2, dtype=np.uint8)
    upload.pack_windows(pix, mpix, frames, masks, 1, 3, window[1:], off2)
    got, _ = _unpack(pix, mpix, window[1:], off2, 1)
    assert np.array_equal(got, frames[2, :40, :40].astype(px))                     # the empty mask's 40 x 40 corner


def test_window_ring_packs_the_control_view_steps():
    """`WindowRing` on host memory (no device): synth.control_view's steps 0 .. 4 as view 1 and the next step as view 2 (env 1 has an
    empty mask at step 2, every env at step 4), float32 frames and bool masks, two poses per slot in two slots."""
    n = 2
    views = [synth.control_view(n, t, seed=6)[0]["camera0"] for t in range(6)]
    ring = upload.WindowRing(n, (torch.float32, torch.float32), "cpu")
    assert ring.pinned_bytes == 2 * (2 * n * 440 * 440 * (3 * 4 + 1) + 2 * n * 28)
    empties = 0
    for t in range(5):
        srcs = [views[t]["Color"], views[t + 1]["Color"], views[t]["Mask"], views[t + 1]["Mask"]]
        before = ring.payload_bytes
        ring.wait(t & 1)
        ring.stage(t & 1, srcs, 0, n)
        d = ring.copy(t & 1, n)
        assert (d.H, d.W) == (H, W)
        pixels = 0
        for v in (0, 1):
            window, valid = upload.mask_windows(srcs[2 + v])
            offset, total = upload.window_offsets(window)
            assert np.array_equal(d.window[v].numpy(), window) and np.array_equal(d.valid[v].numpy(), valid)
            assert np.array_equal(d.offset[v].numpy(), offset) and d.offset[v].dtype == torch.int64
            for f in range(n):
                rmin, rmax, cmin, cmax = window[f]
                got, gotm = _unpack(d.pix[v].numpy(), d.mask[v].numpy(), window, offset, f)
                assert np.array_equal(got, srcs[v][f, rmin:rmax, cmin:cmax]) and np.array_equal(gotm, srcs[2 + v][f, rmin:rmax, cmin:cmax])
                if not valid[f]:
                    assert tuple(window[f]) == (0, 40, 0, 40) and not gotm.any()
                    empties += 1
            pixels += total
        assert ring.payload_bytes - before == pixels * 13
    assert empties == 1 + 1 + n + n                               # step 2 (as view 2, then as view 1), step 4 (as view 2, then as view 1)
    assert ring.table_bytes == 5 * 2 * n * 28
    # float64 masks go through bytes first; a ring asked to serve more poses than it has rows is replaced, a smaller call may reuse it
    srcs = [views[0]["Color"], views[1]["Color"], views[0]["Mask"].astype(np.float64) * 0.25, views[1]["Mask"].astype(np.float64)]
    ring.stage(0, srcs, 1, 2)
    d = ring.copy(0, 1)
    assert np.array_equal(d.window[0].numpy(), upload.mask_windows(views[0]["Mask"][1:])[0])
    assert upload.WindowRing.matching(ring, 1, srcs, "cpu", grow=True) is ring and upload.WindowRing.matching(ring, 1, srcs, "cpu") is not ring
    assert upload.WindowRing.matching(ring, 3, srcs, "cpu", grow=True).rows == 3


# ------------------------------------------------------------------------------------------------------------------ 3. the estimator
def _stub_est(**kw):
    from rgbmanip_amd.config import ADAPOSE_CFGS
    from rgbmanip_amd.estimator import AdaPoseEstimator_v5
    net = types.SimpleNamespace(options={"view2_heads": 0}, dropout=0.0, dropout_seed=0, device="cpu", feature_bytes=64)
    return AdaPoseEstimator_v5(None, dict(ADAPOSE_CFGS["adapose_cabinet"], load=False, **kw), None, net=net)


@pytest.mark.parametrize("frame_dtype", [np.float64, np.uint8])
def test_upload_bytes_last_call_formulas(frame_dtype, monkeypatch):
    """Host packing only: the device side (`_prepare_windows`, the network) is stubbed.  Windows mode: sum over both views of
    h * w * (3 px_bytes + 1), tables apart; frames mode: 2 n H W (3 px_bytes + 1)."""
    frames, m8 = _frames(frame_dtype)
    n, px = len(frames), 1 if frame_dtype == np.uint8 else 4
    rgb2, mask2 = np.ascontiguousarray(frames[::-1]), np.ascontiguousarray(m8[::-1]).astype(bool)
    K, E = np.tile(np.eye(3), (n, 1, 1)), np.tile(np.eye(4), (n, 1, 1))
    est = _stub_est(hip_upload="windows")
    seen = []
    monkeypatch.setattr(est, "_prepare_windows", lambda d, v, Kd, *a, **kw: seen.append((v, d.window[v].numpy().copy(), kw["frame0"])) or {})
    monkeypatch.setattr(est, "_estimate_prepared", lambda a, b, E1, E2, K=None, cached=None, want=None: torch.zeros(len(E1), 8, 3, dtype=torch.float64))
    assert est.upload_bytes_last_call == 0
    box = est.estimate(K, frames, m8, E, rgb2, mask2, E)
    assert box.shape == (n, 8, 3) and [s[0] for s in seen] == [0, 1] and seen[0][2] == 0
    pixels = sum(int(((w[:, 1] - w[:, 0]) * (w[:, 3] - w[:, 2])).sum()) for _, w, _ in seen)
    assert pixels == 2 * (136000 + 1600)
    assert est.upload_bytes_last_call == pixels * (3 * px + 1)
    assert est.upload_table_bytes_last_call == 2 * n * 28
    est.estimate(K[:1], frames[:1], m8[:1], E[:1], rgb2[:1], mask2[:1], E[:1])       # the figure is the LAST call's
    assert est.upload_bytes_last_call == (129600 + 1600) * (3 * px + 1)
    # frames mode (and windows mode handed a list of frames: still host arrays)
    ref = _stub_est()
    assert ref.upload_mode == "frames"
    monkeypatch.setattr(ref, "estimate_device", lambda K, *a, **kw: torch.zeros(len(K), 8, 3, dtype=torch.float64))
    monkeypatch.setattr(ref, "_upload_frames", lambda x: x)
    monkeypatch.setattr(ref, "_upload_masks", lambda x: x)
    ref.estimate(K, frames, m8, E, rgb2, mask2, E)
    assert ref.upload_bytes_last_call == 2 * n * H * W * (3 * px + 1) and ref.upload_table_bytes_last_call == 0
    ref.estimate(K, list(frames), list(m8), E, list(rgb2), list(mask2), E)
    assert ref.upload_bytes_last_call == 2 * n * H * W * (3 * px + 1)
    est.estimate(K, list(frames), list(m8), E, list(rgb2), list(mask2), E)
    assert est.upload_bytes_last_call == pixels * (3 * px + 1)


def test_cfg_validation():
    for bad in ("window", "crops", "", None, True):
        with pytest.raises(ValueError, match="hip_upload"):
            _stub_est(hip_upload=bad)
    with pytest.raises(ValueError, match="hip_prepare"):
        _stub_est(hip_upload="windows", hip_prepare="host")
    assert _stub_est(hip_upload="windows", hip_prepare="device").upload_mode == "windows"
    assert _stub_est(hip_upload="frames", hip_prepare="host").upload_mode == "frames"
    assert _stub_est().upload_mode == "frames"                   # the default


# ------------------------------------------------------------------------------------------------------------------ 4. the C ABI
def test_entry_point_is_declared_exported_and_bound():
    from rgbmanip_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbm.h")).read(), flags=re.S)
    name = "rgbm_prepare_inputs_windows"
    decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", src)
    assert decl, f"{name} is not declared in include/rgbm.h"
    params = [re.sub(r"\s+", " ", p).strip() for p in decl.group(1).split(",")]
    assert params == ["const void* pix_dev", "int pixel_type", "int normalize", "const uint8_t* mask_pix_dev", "const int64_t* offset_dev",
                      "const int32_t* window_dev", "const int32_t* valid_in_dev", "const double* K_dev", "int frame0", "int N", "int H", "int W",
                      "int S", "int P", "uint32_t seed", "float* img_out", "int32_t* choose_out", "float* pts2d_out", "double* Kcrop_out",
                      "int32_t* valid_out", "uint8_t* scratch", "void* stream"]
    assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.SIGNATURES"
    vp, i = C.c_void_p, C.c_int
    fn = getattr(_lib.load(), name)                              # AttributeError: the built library does not export it
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == [vp, i, i, vp, vp, vp, vp, vp, i, i, i, i, i, i, C.c_uint32, vp, vp, vp, vp, vp, vp, vp]
    assert len(fn.argtypes) == len(params)
