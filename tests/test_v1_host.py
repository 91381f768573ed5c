"""CPU-only checks of the v1 network's restatement, fixture, schema, conditioning, path selection and import surface (no GPU)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import v1_ref  # noqa: E402
from forward_paths_ref import BF16, BF16X3, F32, FACTS, PATHS, paths as ref_paths  # noqa: E402
from test_forward_paths import FI, PI, lib_paths, product  # noqa: E402
from test_realworld_host import _groups  # noqa: E402

from rgbmanip_amd import synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAPS = [f"v{v}_{k}_slice" for v in (1, 2) for k in v1_ref.TAP_KEYS]


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "adapose_v1_b2.npz"))


def _forward(dtype):
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    sd = v1_ref.to_sd(synth.v1_state_dict(seed=0), dtype)
    inp = synth.adapose_inputs(2, seed=0)
    taps = {}
    out = v1_ref.v1_forward(sd, inp["img1"], inp["choose1"], inp["img2"], inp["choose2"], inp["P1"], inp["P2"], inp["depths"], taps=taps)
    got = {k: v.numpy() for k, v in out.items()}
    for v in (1, 2):
        for k in v1_ref.TAP_KEYS:
            got[f"v{v}_{k}_slice"] = v1_ref.points_slice(taps[f"v{v}_{k}"]).numpy()
    return got, taps, sd, inp


@pytest.fixture(scope="module")
def ref64(golden):
    """The float64 restatement on the golden batch, once: e_ref64 per tensor = the reference's own float32 rounding."""
    got, taps, sd, inp = _forward(torch.float64)
    errs = {k: v1_ref.rel_err(golden[k], got[k]) for k in v1_ref.OUT_KEYS + TAPS}
    print("e_ref64 per tensor:", errs)
    return got, taps, errs, sd, inp


def test_fixture_can_fail(golden):
    """The conditions the generator asserts, on the stored numbers: every ReLU of the stereo part, the residual one included, clips
    between 5 % and 95 % of what it sees at the chosen points; some warps leave the partner image and some stay inside; the size output
    depends on the view; r is a rotation."""
    for v in (1, 2):
        clip = golden[f"v{v}_clip"]
        assert clip.shape == (len(v1_ref.RELU_NAMES),) and np.all(clip >= 0.05) and np.all(clip <= 0.95), (v, clip)
        assert 0.0 < float(golden[f"v{v}_outside"]) < 1.0
        planes, fused, rows = (golden[f"v{v}_{k}_slice"] for k in v1_ref.TAP_KEYS)
        assert planes.shape == (2, 128, 24) and fused.shape == (2, 128, 32) and rows.shape == (2, 128, 128)
        assert 0.05 <= float((planes == 0).mean()) <= 0.95 and 0.05 <= float((fused == 0).mean()) <= 0.95      # the same shares on the stored points
        r = golden[f"view{v}_r"].astype(np.float64)
        assert np.abs(np.swapaxes(r, 1, 2) @ r - np.eye(3)).max() < 1e-5 and np.all(np.linalg.det(r) > 0.999)
    s1, s2 = golden["view1_s"], golden["view2_s"]
    assert not np.array_equal(s1, s2) and float(np.abs(s1 - s2).max() / max(np.abs(s1).max(), np.abs(s2).max())) >= 1e-3
    assert set(k for k in golden.files if k.startswith("view")) == set(v1_ref.OUT_KEYS)


def test_restatement_float32_against_the_golden(golden, ref64):
    """The float32 restatement against the reference class's golden, per tensor, at the project's float32 rule max(8 e_ref64, 3e-6):
    the restatement evaluates the stereo part at the chosen pixels only (another matmul shape than the reference's full grid)."""
    got = _forward(torch.float32)[0]
    e64 = ref64[2]
    e32 = {k: v1_ref.rel_err(got[k], golden[k]) for k in v1_ref.OUT_KEYS + TAPS}
    print("e_ref32 per tensor:", e32)
    for k in v1_ref.OUT_KEYS + TAPS:
        assert np.isfinite(got[k]).all() and e32[k] <= max(8 * e64[k], 3e-6), (k, e32[k], e64[k])


def test_restatement_float64_records_the_reference_rounding(golden, ref64):
    """e_ref64, printed per tensor, below 1e-4.  The statistics stored beside the slices are those of the restatement's full tensors."""
    got, taps, errs = ref64[:3]
    assert 0 < max(errs.values()) < 1e-4, errs
    for v in (1, 2):
        assert np.allclose(taps[f"v{v}_clip"], golden[f"v{v}_clip"], atol=2e-4)
        assert taps[f"v{v}_outside"] == pytest.approx(float(golden[f"v{v}_outside"]), abs=2e-4)
        for k in v1_ref.TAP_KEYS:
            assert float(taps[f"v{v}_{k}"].abs().max()) == pytest.approx(float(golden[f"v{v}_{k}_absmax"]), rel=1e-4)


def _round_rel17(x):
    """x rounded to 17 significant bits: a relative error of at most 2^-17, what a split pair keeps of a float32"""
    m, e = np.frexp(np.asarray(x, dtype=np.float64))
    return np.ldexp(np.rint(m * 2.0 ** 17) / 2.0 ** 17, e)


def test_conditioning_of_the_fixture(ref64):
    """Asserted here so that the GPU gates need no widening.  The float64 restatement with its feature maps rounded to bfloat16: every
    output moves by less than 400 x that rounding's own size (x4 margin included, the rule of tests/test_gpu_v2.py).  With the maps
    rounded to 2^-17 relative (split pairs) every output moves by less than 2.5e-5, a quarter of the project's 1e-4 for bf16x3."""
    got, taps, _, sd, inp = ref64
    feat = torch.cat((taps["feat1"], taps["feat2"]))

    def moved(rounded):
        out = v1_ref.heads_on_maps(sd, rounded[:2], rounded[2:], inp["choose1"], inp["choose2"], inp["P1"], inp["P2"], inp["depths"])
        return {k: v1_ref.rel_err(out[k].numpy(), got[k]) for k in v1_ref.OUT_KEYS}

    bf = feat.float().to(torch.bfloat16).double()
    fe = v1_ref.rel_err(bf.numpy(), feat.numpy())
    amp = {k: 4 * e / fe for k, e in moved(bf).items()}
    print("bf16 feature rounding", fe, "amplification factors (x4 margin included):", amp)
    assert all(np.isfinite(a) and a < 400 for a in amp.values()), amp
    r17 = torch.from_numpy(_round_rel17(feat.numpy()))
    assert float(((r17 - feat).abs() / feat.abs().clamp_min(1e-300)).max()) <= 2.0 ** -17
    m17 = moved(r17)
    print("maps rounded to 2^-17 relative: outputs move by", m17)
    assert all(e < 2.5e-5 for e in m17.values()), m17


def test_schema_is_the_reference_classs(golden):
    sd = synth.v1_state_dict(seed=0)
    assert list(sd.keys()) == list(golden["sd_keys"])
    assert ["x".join(str(d) for d in np.asarray(v).shape) for v in sd.values()] == list(golden["sd_shapes"])
    assert [(n, tuple(s)) for n, s, _ in synth.v1_schema()] == [(k, tuple(np.asarray(v).shape)) for k, v in sd.items()]
    v5, v2 = synth.adapose_state_dict(seed=0), synth.v2_state_dict(seed=0)
    shared = [k for k in sd if k.startswith(("img_extractor.", "instance_color.", "nocs_head.", "nocs_pts_mlp.", "pose_mlp2.", "rotation_estimator."))]
    assert shared and all(np.array_equal(sd[k], v5[k]) for k in shared)
    assert all(np.array_equal(sd[k], v2[k]) for k in sd if k.startswith(("volume_conv.", "fuse_conv.0.")))
    assert sd["fuse_conv.2.weight"].shape == (32, 32, 1, 1) and sd["pose_mlp1.0.weight"].shape == (128, 128, 1) and sd["size_estimator.4.weight"].shape == (3, 128)
    assert not any(k.startswith(("cost_regularization.", "camera_pts_mlp.")) for k in sd)
    again5, again2 = synth.adapose_state_dict(seed=0), synth.v2_state_dict(seed=0)      # drawing the v1 dict leaves the others what they were
    assert all(np.array_equal(v5[k], again5[k]) for k in v5) and all(np.array_equal(v2[k], again2[k]) for k in v2)


# ------------------------------------------------------------------------------------------------ path selection (rgbm_forward_paths)
def test_paths_of_the_v1_arch_have_no_3d_paths():
    """Arch 4: the PSPNet's paths are v5's; nothing of the cost regularisation is answered whatever its options say; a split-pair net
    writes the plain-fp32 map only; the point MLP follows v5's rule and the fused pose MLP is never taken."""
    for g in _groups((4,)):
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
        as_v2 = g.copy()
        as_v2[:, FI["arch"]] = 3
        assert np.array_equal(got, lib_paths(as_v2))      # no new path entry: the rows are arch 3's
    row = product(dict(arch=(4,), dtype=(BF16,)))
    d = dict(zip(PATHS, lib_paths(row)[0]))
    assert (d["stem"], d["up3"], d["feat_form"], d["cost_body"], d["point_mlp"], d["pose_mlp"]) == (1, 2, 0, 0, 1, 0)


def test_paths_of_the_existing_archs_are_unchanged():
    """Archs 0 and 1 as tests/forward_paths_ref.py says, byte for byte; arch 2 as tests/test_realworld_host.py derives it from that
    reference; arch 3 as tests/test_v2_host.py derives it."""
    for g in _groups((0, 1)):
        assert lib_paths(g).tobytes() == ref_paths(g).astype(lib_paths(g).dtype).tobytes()
    for g in _groups((2,)):
        for k in ("sweep_w", "w11_taps"):
            g[:, FI[k]] = (g[:, FI["dtype"]] != F32).astype(np.int32)
        as_v5 = g.copy()
        as_v5[:, FI["arch"]] = 0
        as_v5[:, FI["sweep_w_f16"]] = 0
        assert np.array_equal(lib_paths(g), ref_paths(as_v5))
    for g in _groups((3,)):
        got = lib_paths(g)
        p = {k: got[:, i] for k, i in PI.items()}
        as_v5 = g.copy()
        as_v5[:, FI["arch"]] = 0
        want = ref_paths(as_v5)
        for k in PI:
            if k in ("stem", "psp_stage", "up1", "up2", "up3", "point_mlp"):
                assert np.array_equal(p[k], want[:, PI[k]]), k
            elif k == "feat_form":
                assert np.array_equal(p[k], (g[:, FI["dtype"]] == BF16X3).astype(np.int32))
            else:
                assert not np.any(p[k]), k
    assert len(FACTS) == 28 and len(PATHS) == 17


# ------------------------------------------------------------------------------------------------ imports and refusals
def test_compat_serves_the_reference_import_path():
    from rgbmanip_amd import compat, estimator
    compat.install()
    try:
        from models.pose_estimator.AdaPose.interface import AdaPoseEstimator, BasePoseEstimator
        assert AdaPoseEstimator is estimator.AdaPoseEstimator_v1 and BasePoseEstimator is estimator.BasePoseEstimator
    finally:
        compat.uninstall()
    assert issubclass(estimator.AdaPoseEstimator_v1, estimator.AdaPoseEstimator_v2)


def test_header_declares_and_library_exports_the_new_symbols():
    import re
    from rgbmanip_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbm.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in ("rgbm_adapose_create_v1", "rgbm_v1_point_rows"):
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None


@pytest.mark.parametrize("key,val", [("hip_feature_cache", True), ("hip_dropout", 0.15), ("hip_as_shipped", True), ("hip_graph", True),
                                     ("hip_norm_mode", 1), ("hip_prepare", "host"), ("hip_upload", "windows")])
def test_estimator_refuses_unsupported_keys_by_name(key, val):
    from rgbmanip_amd import config, estimator
    cfg = dict(config.adapose_cfg(name="adapose", load=False), **{key: val})
    with pytest.raises(ValueError, match=key) as e:
        estimator.AdaPoseEstimator_v1(None, cfg, None)
    assert "AdaPoseEstimator_v1" in str(e.value) and "v2" not in str(e.value)


def test_estimator_refuses_the_sampled_and_dense_calls_by_name():
    from rgbmanip_amd import estimator
    est = object.__new__(estimator.AdaPoseEstimator_v1)      # the refusals read nothing of the instance
    for name in ("estimate_samples", "estimate_samples_device", "estimate_depth", "estimate_depth_device", "estimate_cloud", "estimate_cloud_device",
                 "estimate_cloud_pose", "estimate_cloud_pose_device", "estimate_cloud_views", "estimate_cloud_views_device"):
        with pytest.raises(NotImplementedError, match="AdaPoseEstimator_v1." + name):
            getattr(est, name)()
    # the class it derives from still speaks under its own name
    with pytest.raises(NotImplementedError, match="AdaPoseEstimator_v2.estimate_depth"):
        object.__new__(estimator.AdaPoseEstimator_v2).estimate_depth()


def test_net_refuses_what_the_v1_network_has_not_by_name():
    """Before anything touches a device: refused in the constructor's own checks."""
    from rgbmanip_amd import _lib
    from rgbmanip_amd.adapose import AdaPoseNet
    for key, val in (("graph", 1), ("dropout", 0.15), ("norm_mode", 1), ("split_streams", True), ("cost_impl", 2), ("sparse_tail", 0)):
        with pytest.raises(_lib.RgbmError, match=key) as e:
            AdaPoseNet({}, dtype="bf16", arch="v1", **{key: val})
        assert "v1" in str(e.value)
    with pytest.raises(ValueError, match="'v1'") as e:
        AdaPoseNet({}, arch="v3")
    assert "'v2'" in str(e.value)
