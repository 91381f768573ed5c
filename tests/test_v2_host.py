"""CPU-only checks of the v2 network's restatement, fixture, schema, prepare restatement, path selection and import surface (no GPU)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import v2_ref  # noqa: E402
from forward_paths_ref import BF16, BF16X3, F16, F32, FACTS, PATHS, paths as ref_paths  # noqa: E402
from test_forward_paths import FI, PI, lib_paths, product  # noqa: E402
from test_realworld_host import COST_AXES, FRONT_AXES, _groups  # noqa: E402

from oracle import postproc_ref  # noqa: E402
from rgbmanip_amd import synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAPS = [f"v{v}_{k}_slice" for v in (1, 2) for k in v2_ref.TAP_KEYS]


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "adapose_v2_b2.npz"))


def _forward(dtype):
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    sd = v2_ref.to_sd(synth.v2_state_dict(seed=0), dtype)
    inp = synth.adapose_inputs(2, seed=0)
    taps = {}
    out = v2_ref.v2_forward(sd, inp["img1"], inp["choose1"], inp["img2"], inp["choose2"], inp["P1"], inp["P2"], inp["depths"], taps=taps)
    got = {k: v.numpy() for k, v in out.items()}
    for v in (1, 2):
        for k in v2_ref.TAP_KEYS:
            got[f"v{v}_{k}_slice"] = v2_ref.points_slice(taps[f"v{v}_{k}"]).numpy()
    return got, taps


@pytest.fixture(scope="module")
def ref64(golden):
    """The float64 restatement on the golden batch, once: e_ref64 per tensor = the reference's own float32 rounding."""
    got, taps = _forward(torch.float64)
    errs = {k: v2_ref.rel_err(golden[k], got[k]) for k in v2_ref.OUT_KEYS + TAPS}
    print("e_ref64 per tensor:", errs)
    return got, taps, errs


def test_fixture_can_fail(golden):
    """The conditions the generator asserts, on the stored numbers: every ReLU of the stereo part clips some and passes some of what it
    sees at the chosen points, the rows depend on the point, the size output depends on the view, and the warp leaves the partner image
    for some (point, plane) pairs and stays inside for others."""
    for v in (1, 2):
        clip = golden[f"v{v}_clip"]
        assert clip.shape == (4,) and np.all(clip >= 0.05) and np.all(clip <= 0.95), (v, clip)
        assert 0.05 <= float(golden[f"v{v}_outside"]) <= 0.95
        assert float(golden[f"v{v}_rows_spread"]) >= 0.25
        rows = golden[f"v{v}_rows_slice"].astype(np.float64)      # the same measure on the stored points
        assert rows.shape == (2, 128, 64) and float(rows.std(axis=1, ddof=1).mean() / np.abs(rows).mean()) >= 0.25
        planes = golden[f"v{v}_planes_slice"]
        assert planes.shape == (2, 128, 24) and 0.05 <= float((planes == 0).mean()) <= 0.95
        assert golden[f"v{v}_fuse_slice"].shape == (2, 128, 64)
    s1, s2 = golden["view1_s"], golden["view2_s"]
    assert float(np.abs(s1 - s2).max() / max(np.abs(s1).max(), np.abs(s2).max())) >= 0.02
    assert set(k for k in golden.files if k.startswith("view")) == set(v2_ref.OUT_KEYS)


def test_restatement_float32_against_the_golden(golden, ref64):
    """The float32 restatement against the reference class's golden: the NOCS branch is the realworld restatement's code and is bit-equal;
    the stereo part is evaluated at the chosen pixels only (another matmul shape than the reference's full grid), so those tensors are
    reported, and held to the project's float32 rule max(8 e_ref64, 3e-6)."""
    got, _ = _forward(torch.float32)
    e64 = ref64[2]
    e32 = {k: v2_ref.rel_err(got[k], golden[k]) for k in v2_ref.OUT_KEYS + TAPS}
    print("e_ref32 per tensor:", e32)
    for v in (1, 2):
        assert np.array_equal(got[f"view{v}_nocs"], golden[f"view{v}_nocs"])
    for k in v2_ref.OUT_KEYS + TAPS:
        assert np.isfinite(got[k]).all() and e32[k] <= max(8 * e64[k], 3e-6), (k, e32[k], e64[k])


def test_restatement_float64_records_the_reference_rounding(golden, ref64):
    """e_ref64, printed per tensor; bounded only by the sanity that float32 cannot be worse than 1e-4 on a conditioned fixture.  The
    statistics stored beside the slices are those of the restatement's full tensors."""
    got, taps, errs = ref64
    assert 0 < max(errs.values()) < 1e-4, errs
    for v in (1, 2):
        assert np.allclose(taps[f"v{v}_clip"], golden[f"v{v}_clip"], atol=2e-4)
        assert taps[f"v{v}_outside"] == pytest.approx(float(golden[f"v{v}_outside"]), abs=2e-4)
        for k in v2_ref.TAP_KEYS:
            assert float(taps[f"v{v}_{k}"].abs().max()) == pytest.approx(float(golden[f"v{v}_{k}_absmax"]), rel=1e-4)


def test_schema_is_the_reference_classs(golden):
    sd = synth.v2_state_dict(seed=0)
    assert list(sd.keys()) == list(golden["sd_keys"])
    assert ["x".join(str(d) for d in np.asarray(v).shape) for v in sd.values()] == list(golden["sd_shapes"])
    assert [(n, tuple(s)) for n, s, _ in synth.v2_schema()] == [(k, tuple(np.asarray(v).shape)) for k, v in sd.items()]
    v5 = synth.adapose_state_dict(seed=0)
    shared = [k for k in sd if k.startswith(("img_extractor.", "instance_color.", "nocs_head."))]
    assert shared and all(np.array_equal(sd[k], v5[k]) for k in shared)
    assert sd["pose_mlp1.0.weight"].shape == (64, 64, 1) and sd["pose_mlp2.0.weight"].shape == (128, 128, 1) and sd["size_estimator.4.weight"].shape == (3, 64)
    again = synth.adapose_state_dict(seed=0)      # drawing the v2 dict leaves v5's what it was
    assert all(np.array_equal(v5[k], again[k]) for k in v5)
    # the named constants of the draw
    assert (synth.V2_VC2_BN_GAIN, synth.V2_VC2_BN_SHIFT, synth.V2_FUSE_GAIN) == (16.0, 8.3, 4.0)
    assert 8.0 <= float(sd["volume_conv.2.bn.weight"][0]) <= 24.0 and abs(float(sd["volume_conv.2.bn.bias"][0]) - 8.3) < 0.5
    assert float(np.abs(sd["fuse_conv.0.weight"]).max()) > 1.0 / np.sqrt(24)


# ------------------------------------------------------------------------------------------------ prepare_model_input (interface_v2.py:74-118)
def _literal_prepare(rgb_shape, mask, K, size, keep):
    """interface_v2.py:61-118 transcribed line by line in numpy (no cv2: the image is not part of it), the random keep-mask replaced by
    `keep(choose)` -> the candidates to keep."""
    ys, xs = np.nonzero(mask)
    if len(ys) == 0:
        return None, None, None
    y1, y2 = np.min(ys, initial=rgb_shape[0]), np.max(ys, initial=0)
    x1, x2 = np.min(xs, initial=rgb_shape[1]), np.max(xs, initial=0)
    rmin, rmax, cmin, cmax = postproc_ref.get_bbox([y1, x1, y2, x2])
    choose = mask[rmin:rmax, cmin:cmax].flatten().nonzero()[0]
    if len(choose) > 1024:
        choose = keep(choose)
    elif len(choose) == 0:
        return None, None, None
    else:
        choose = np.pad(choose, (0, 1024 - len(choose)), 'wrap')
    xmap = np.array([[i for i in range(rgb_shape[1])] for j in range(rgb_shape[0])])
    ymap = np.array([[j for i in range(rgb_shape[1])] for j in range(rgb_shape[0])])
    xmap_masked = xmap[rmin:rmax, cmin:cmax].flatten()[choose][:, np.newaxis]
    ymap_masked = ymap[rmin:rmax, cmin:cmax].flatten()[choose][:, np.newaxis]
    view_pts2d = np.concatenate((xmap_masked, ymap_masked), axis=-1)
    crop_w = rmax - rmin
    ratio = size / crop_w
    col_idx = choose % crop_w
    row_idx = choose // crop_w
    choose = (np.floor(row_idx * ratio) * size + np.floor(col_idx * ratio)).astype(np.int64)
    crop_center = [float(cmin + cmax) / 2, float(rmin + rmax) / 2]
    crop_size = [float(cmax - cmin + 1), float(rmax - rmin + 1)]
    new_intrinsic = np.eye(3)
    new_intrinsic[0, 0] = K[0, 0] * ratio
    new_intrinsic[1, 1] = K[1, 1] * ratio
    new_intrinsic[0, 2] = (K[0, 2] - (crop_center[0] - crop_size[0] / 2)) * ratio
    new_intrinsic[1, 2] = (K[1, 2] - (crop_center[1] - crop_size[1] / 2)) * ratio
    return choose, view_pts2d, new_intrinsic


def prepare_masks():
    """name -> [480, 640] uint8 masks shared with tests/test_gpu_v2.py: a 40-window, the full 440-window (193 600 candidates), n = 1, 1024
    and 1025, a mask touching the frame's edges, an ellipse."""
    H, W = 480, 640
    m = {}
    z = lambda: np.zeros((H, W), np.uint8)      # noqa: E731
    a = z(); a[100:130, 200:225] = 1; m["window40"] = a
    a = z(); a[:, :] = 1; m["window440_full"] = a
    a = z(); a[17, 333] = 1; m["n1"] = a
    a = z(); a[200:232, 300:332] = 1; m["n1024"] = a
    a = z(); a[200:232, 300:332] = 1; a[232, 300] = 1; m["n1025"] = a
    a = z(); a[0:90, 560:640] = 1; a[3, 600] = 0; m["edge"] = a
    yy, xx = np.mgrid[:H, :W]
    m["ellipse"] = ((((yy - 250) / 120.0) ** 2 + ((xx - 300) / 170.0) ** 2) <= 1.0).astype(np.uint8)
    return m


@pytest.mark.parametrize("name", list(prepare_masks()))
def test_prepare_restatement_is_the_literal_transcription(name):
    mask = prepare_masks()[name]
    K = np.array([[439.3, 0, 320.0], [0, 439.3, 240.0], [0, 0, 1]])
    rgb = np.zeros((480, 640, 3), np.float32)
    seed, frame = 5, 3
    view, choose, pts2d, Kn, window = v2_ref.prepare_model_input(rgb, mask, K, 224, seed=seed, frame=frame)
    want = _literal_prepare(rgb.shape, mask, K, 224, lambda c: postproc_ref.choose_subset_hash(c, 1024, seed, frame))
    assert np.array_equal(choose, want[0]) and choose.dtype == np.int64 and np.array_equal(pts2d, want[1]) and np.array_equal(Kn, want[2])
    assert view.shape == (3, 224, 224) and choose.shape == (1024,) and 0 <= choose.min() and choose.max() < 224 * 224
    n = int(mask[window[0]:window[1], window[2]:window[3]].sum())
    if name == "window440_full":
        assert n == 193600 and window[1] - window[0] == 440 and len(np.unique(choose)) < 1024      # native indices beyond 16 bits; duplicates
    if name in ("n1", "n1024", "n1025"):
        assert n == int(name[1:])
    assert np.all(mask[pts2d[:, 1], pts2d[:, 0]] == 1)


def test_prepare_restatement_of_an_empty_mask():
    assert v2_ref.prepare_model_input(np.zeros((480, 640, 3), np.float32), np.zeros((480, 640), np.uint8), np.eye(3))[0] is None


# ------------------------------------------------------------------------------------------------ path selection (rgbm_forward_paths)
def test_paths_of_the_v2_arch_have_no_3d_paths():
    """Arch 3: the PSPNet's paths are v5's; nothing of the cost regularisation is answered whatever its options say; a split-pair net
    writes the plain-fp32 map only (nothing reads split pairs); the point MLP follows v5's rule and the fused pose MLP is never taken."""
    for g in _groups((3,)):
        got = lib_paths(g)
        p = {k: got[:, i] for k, i in PI.items()}
        for k in ("cost_body", "conv0", "conv6_igemm", "mask_level", "sweep_list", "tail_sparse", "vol", "bn_scratch", "pose_mlp", "feat_copy"):
            assert not np.any(p[k]), k
        assert np.array_equal(p["feat_form"], (g[:, FI["dtype"]] == BF16X3).astype(np.int32))
        as_v5 = g.copy()
        as_v5[:, FI["arch"]] = 0
        want = ref_paths(as_v5)
        for k in ("stem", "psp_stage", "up1", "up2", "up3", "point_mlp"):
            assert np.array_equal(p[k], want[:, PI[k]]), k
    row = product(dict(arch=(3,), dtype=(BF16,)))
    d = dict(zip(PATHS, lib_paths(row)[0]))
    assert (d["stem"], d["up3"], d["feat_form"], d["cost_body"], d["point_mlp"], d["pose_mlp"]) == (1, 2, 0, 0, 1, 0)


def test_paths_of_the_existing_archs_are_unchanged():
    """Archs 0 and 1 as tests/forward_paths_ref.py says; arch 2 as tests/test_realworld_host.py derives it from that reference."""
    for g in _groups((0, 1)):
        assert np.array_equal(lib_paths(g), ref_paths(g))
    for g in _groups((2,)):
        for k in ("sweep_w", "w11_taps"):
            g[:, FI[k]] = (g[:, FI["dtype"]] != F32).astype(np.int32)
        as_v5 = g.copy()
        as_v5[:, FI["arch"]] = 0
        as_v5[:, FI["sweep_w_f16"]] = 0
        assert np.array_equal(lib_paths(g), ref_paths(as_v5))
    assert set(COST_AXES["dtype"]) == {F32, BF16, F16, BF16X3} and "flags" in FRONT_AXES and len(FACTS) == 28


# ------------------------------------------------------------------------------------------------ imports and refusals
def test_compat_serves_the_reference_import_path():
    from rgbmanip_amd import compat, estimator
    compat.install()
    try:
        from models.pose_estimator.AdaPose.interface_v2 import AdaPoseEstimator_v2, BasePoseEstimator
        assert AdaPoseEstimator_v2 is estimator.AdaPoseEstimator_v2 and BasePoseEstimator is estimator.BasePoseEstimator
    finally:
        compat.uninstall()
    assert issubclass(estimator.AdaPoseEstimator_v2, estimator.AdaPoseEstimator_v5)


def test_config_names_the_v2_estimator():
    from rgbmanip_amd import config
    cfg = config.adapose_cfg(name="adapose_v2")
    assert cfg["name"] == "adapose_v2" and cfg["n_pts"] == 1024


def test_header_declares_and_library_exports_the_new_symbols():
    import re
    from rgbmanip_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbm.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in ("rgbm_adapose_create_v2", "rgbm_v2_point_rows", "rgbm_prepare_inputs_native"):
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None


@pytest.mark.parametrize("key,val", [("hip_feature_cache", True), ("hip_dropout", 0.15), ("hip_as_shipped", True), ("hip_graph", True),
                                     ("hip_norm_mode", 1), ("hip_prepare", "host"), ("hip_upload", "windows")])
def test_estimator_refuses_unsupported_keys_by_name(key, val):
    from rgbmanip_amd import config, estimator
    cfg = dict(config.adapose_cfg(name="adapose_v2", load=False), **{key: val})
    with pytest.raises(ValueError, match=key):
        estimator.AdaPoseEstimator_v2(None, cfg, None)


def test_estimator_refuses_the_sampled_and_dense_calls_by_name():
    from rgbmanip_amd import estimator
    est = object.__new__(estimator.AdaPoseEstimator_v2)      # the refusals read nothing of the instance
    for name in ("estimate_samples", "estimate_samples_device", "estimate_depth", "estimate_depth_device", "estimate_cloud", "estimate_cloud_device",
                 "estimate_cloud_pose", "estimate_cloud_pose_device", "estimate_cloud_views", "estimate_cloud_views_device"):
        with pytest.raises(NotImplementedError, match=name):
            getattr(est, name)()


def test_net_refuses_what_the_v2_network_has_not_by_name():
    """Before anything touches a device: refused in the constructor's own checks."""
    from rgbmanip_amd import _lib
    from rgbmanip_amd.adapose import AdaPoseNet
    for key, val in (("graph", 1), ("dropout", 0.15), ("norm_mode", 1), ("split_streams", True), ("cost_impl", 2), ("sparse_tail", 0)):
        with pytest.raises(_lib.RgbmError, match=key):
            AdaPoseNet({}, dtype="bf16", arch="v2", **{key: val})
    with pytest.raises(ValueError, match="v2"):
        AdaPoseNet({}, arch="v3")

