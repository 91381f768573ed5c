"""CPU-only checks of the real-world network's restatement, fixture, schema, path selection and import surface (no GPU)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import realworld_ref as rr  # noqa: E402
from forward_paths_ref import BF16, BF16X3, F16, F32, FACTS, PATHS, paths as ref_paths  # noqa: E402
from test_forward_paths import FI, PI, lib_paths, product  # noqa: E402

from rgbmanip_amd import synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = (F32, BF16, F16, BF16X3)
TAPS = [f"v{v}_{k}" for v in (1, 2) for k in ("vol_slice", "c0_slice", "rows_slice")]


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "adapose_realworld_b2.npz"))


def _forward(dtype, golden):
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    sd = rr.to_sd(synth.realworld_state_dict(seed=0), dtype)
    inp = synth.adapose_inputs(2, seed=0)
    taps = {}
    out = rr.realworld_forward(sd, inp["img1"], inp["choose1"], golden["coor1"], inp["img2"], inp["choose2"], golden["coor2"], inp["P1"], inp["P2"],
                               inp["depths"], taps=taps)
    got = {k: v.numpy() for k, v in out.items()}
    for v in (1, 2):
        got[f"v{v}_vol_slice"] = taps[f"v{v}_vol_slice"].numpy()
        got[f"v{v}_c0_slice"] = taps[f"v{v}_c0_slice"].numpy()
        got[f"v{v}_rows_slice"] = rr.rows_slice(taps[f"v{v}_rows"]).numpy()
    return got, taps


@pytest.fixture(scope="module")
def ref64(golden):
    """The float64 restatement on the golden batch, once: e_ref64 per tensor = the reference's own float32 rounding."""
    got, taps = _forward(torch.float64, golden)
    errs = {k: rr.rel_err(golden[k], got[k]) for k in rr.OUT_KEYS + TAPS}
    print("e_ref64 per tensor:", errs)
    return got, taps, errs


def test_restatement_float32_sits_within_the_references_rounding(golden, ref64):
    """The float32 restatement against the reference class's golden, tensor by tensor, held to the rounding distance measured here: 8 x the
    golden's own distance to the float64 restatement of that tensor (the factor the project gives a float32 computation over the
    reference's float32 rounding), floor 3e-6.  Measured e_ref64 / e_ref32: see the printed dicts (the variance volume's slices: the
    reference forms three squares and subtracts, |vol| reaches 351)."""
    got, _ = _forward(torch.float32, golden)
    e64 = ref64[2]
    e32 = {k: rr.rel_err(got[k], golden[k]) for k in rr.OUT_KEYS + TAPS}
    print("e_ref32 per tensor:", e32)
    for k in rr.OUT_KEYS + TAPS:
        assert np.isfinite(got[k]).all() and e32[k] <= max(8 * e64[k], 3e-6), (k, e32[k], e64[k])


def test_restatement_float64_records_the_reference_rounding(golden, ref64):
    """e_ref64, printed per tensor; bounded only by the sanity that float32 cannot be worse than 1e-4 on a conditioned fixture."""
    errs = ref64[2]
    assert 0 < max(errs.values()) < 1e-4, errs
    for v in (1, 2):      # the statistics stored beside the slices are those of the restatement's full tensors
        assert ref64[1][f"v{v}_vol_absmean"] == pytest.approx(float(golden[f"v{v}_vol_absmean"]), rel=1e-4)
        assert ref64[1][f"v{v}_c0_absmean"] == pytest.approx(float(golden[f"v{v}_c0_absmean"]), rel=1e-4)
        assert ref64[1][f"v{v}_outside_share"] == pytest.approx(float(golden[f"v{v}_outside_share"]), abs=1e-4)


def test_fixture_is_not_degenerate(golden):
    """On the stored numbers: both views' volumes have at least 5 % of their voxels warped outside the partner image (exact zeros) and at
    least 5 % inside, in the whole volume and in the stored slice, and |max| >= 10 |mean| (351 / 16 on view 1)."""
    for v in (1, 2):
        for key in (f"v{v}_outside_share", f"v{v}_outside_share_slice"):
            share = float(golden[key])
            assert 0.05 <= share <= 0.95, (key, share)
        assert float(golden[f"v{v}_vol_absmax"]) >= 10 * float(golden[f"v{v}_vol_absmean"])
        sl = golden[f"v{v}_vol_slice"]
        assert sl.shape == (2, 4, 8, 13, 13) and 0.05 <= float((sl == 0).mean()) <= 0.95
        assert golden[f"v{v}_c0_slice"].shape == (2, 4, 8, 13, 13) and golden[f"v{v}_rows_slice"].shape == (2, 64, 128)
    wh = golden["frame_wh"].astype(np.float32)
    assert tuple(golden["frame_wh"]) == (640, 480)
    for v in (1, 2):      # the stored coordinates are the stored pixels divided in float32
        assert np.array_equal(golden[f"coor{v}"], golden[f"pts2d{v}"] / wh) and golden[f"coor{v}"].dtype == np.float32


def test_schema_is_the_reference_classs(golden):
    sd = synth.realworld_state_dict(seed=0)
    assert list(sd.keys()) == list(golden["sd_keys"])
    assert ["x".join(str(d) for d in np.asarray(v).shape) for v in sd.values()] == list(golden["sd_shapes"])
    v5 = synth.adapose_state_dict(seed=0)
    assert set(sd) - set(v5) == {f"camera_pts_mlp.{i}.{p}" for i in (0, 2) for p in ("weight", "bias")} and not set(v5) - set(sd)
    assert sd["pose_mlp1.0.weight"].shape == (128, 128, 1) and v5["pose_mlp1.0.weight"].shape == (128, 96, 1)
    for k, a in v5.items():
        if k != "pose_mlp1.0.weight":
            assert np.array_equal(sd[k], a), k
    again = synth.adapose_state_dict(seed=0)      # drawing the real-world dict leaves v5's what it was
    assert all(np.array_equal(v5[k], again[k]) for k in v5)


# ------------------------------------------------------------------------------------------------ path selection (rgbm_forward_paths)
COST_AXES = dict(dtype=DTYPES, norm_mode=(0, 1), cost_impl=(0, 1, 2, 3), sparse_tail=(0, 1), sparse_dec=(0, 1, 2), sweep_f16=(0, 1), igemm_conv6=(0, 1),
                 upconv=(3, 7), flags=(0, 4096), dense=(0, 1), sweep_w_f16=(0, 1), tail_f16_ready=(0, 1), w11_x3=(0, 1))
FRONT_AXES = dict(dtype=DTYPES, stem=(0, 1), upconv=tuple(range(8)), fuse_final=(0, 1),
                  flags=tuple(a | b | c for a in (0, 1024) for b in (0, 2048) for c in (0, 524288)), V=(2, 32, 34), n_pts=(1024, 1000),
                  pmlp_table=(0, 1), psp_shape_ok=(0, 1), pose_shape_ok=(0, 1))


def _groups(archs):
    """The two cross products tests/test_forward_paths.py sweeps, for these archs."""
    cost = product(dict(arch=archs, **COST_AXES))
    front = product(dict(arch=archs, **FRONT_AXES))
    front[:, FI["Vh"]] = front[:, FI["V"]]
    return cost, front


def test_paths_of_the_realworld_arch_never_take_the_f16_forms():
    """Arch 2 answers what arch 0 answers for a handle without the f16 sweep pack - v5's paths with FEAT_F16 and CONV0_SWEEP16_F16 taken
    out - on every option and flag combination the existing path test sweeps (base_facts builds arch 2's packs as a baseline handle's, so
    the packs create_cost builds are switched on here); `vol` follows cost_impl."""
    for g in _groups((2,)):
        for k in ("sweep_w", "w11_taps"):
            g[:, FI[k]] = (g[:, FI["dtype"]] != F32).astype(np.int32)
        got = lib_paths(g)
        p = {k: got[:, i] for k, i in PI.items()}
        assert not np.any(p["feat_form"] == 2) and not np.any(p["conv0"] == 4)
        assert np.array_equal(p["vol"] == 1, ~((g[:, FI["cost_impl"]] >= 2) & (g[:, FI["norm_mode"]] == 0)))
        assert np.all(p["cost_body"] != 0)
        as_v5 = g.copy()
        as_v5[:, FI["arch"]] = 0
        as_v5[:, FI["sweep_w_f16"]] = 0
        want = ref_paths(as_v5)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, (len(bad), dict(zip(FACTS, g[bad[0]])), dict(zip(PATHS, got[bad[0]])), dict(zip(PATHS, want[bad[0]])))
    # the default bf16 handle: bf16 feature map, the 16-bit sweep with the fp32 blend, everything behind it as v5
    row = product(dict(arch=(2,), dtype=(BF16,)))
    row[:, FI["sweep_w"]] = row[:, FI["w11_taps"]] = 1
    d = dict(zip(PATHS, lib_paths(row)[0]))
    assert (d["feat_form"], d["conv0"], d["mask_level"], d["tail_sparse"], d["conv6_igemm"]) == (0, 3, 2, 1, 1)


def test_paths_of_the_existing_archs_are_unchanged():
    for g in _groups((0, 1)):
        assert np.array_equal(lib_paths(g), ref_paths(g))


# ------------------------------------------------------------------------------------------------ imports and refusals
def test_compat_serves_the_reference_import_path():
    from rgbmanip_amd import compat, estimator
    compat.install()
    try:
        from models.pose_estimator.AdaPose.interface_realworld import AdaPoseEstimator_realworld, BasePoseEstimator
        assert AdaPoseEstimator_realworld is estimator.AdaPoseEstimator_realworld and BasePoseEstimator is estimator.BasePoseEstimator
    finally:
        compat.uninstall()


def test_config_names_the_realworld_estimator():
    from rgbmanip_amd import config
    cfg = config.adapose_cfg(name="adapose_realworld")
    assert cfg["name"] == "adapose_realworld" and cfg["n_pts"] == 1024


def test_header_declares_and_library_exports_the_new_symbols():
    import re
    from rgbmanip_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbm.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in ("rgbm_adapose_create_realworld", "rgbm_adapose_forward_realworld", "rgbm_adapose_postprocess_pnp_scaled", "rgbm_pts2d_to_coor",
                 "rgbm_build_volume_fusion"):
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None


@pytest.mark.parametrize("key,val", [("hip_feature_cache", True), ("hip_dropout", 0.15), ("hip_as_shipped", True), ("hip_graph", True),
                                     ("hip_norm_mode", 1), ("hip_prepare", "host"), ("hip_dtype", "fp16")])
def test_estimator_refuses_unsupported_keys_by_name(key, val):
    from rgbmanip_amd import config, estimator
    cfg = dict(config.adapose_cfg(name="adapose_realworld", load=False), **{key: val})
    with pytest.raises(ValueError, match=key):
        estimator.AdaPoseEstimator_realworld(None, cfg, None)


def test_estimator_refuses_the_sampled_and_dense_calls_by_name():
    from rgbmanip_amd import estimator
    est = object.__new__(estimator.AdaPoseEstimator_realworld)      # the refusals read nothing of the instance
    for name in ("estimate_samples", "estimate_samples_device", "estimate_depth", "estimate_depth_device", "estimate_cloud", "estimate_cloud_device",
                 "estimate_cloud_pose", "estimate_cloud_pose_device", "estimate_cloud_views", "estimate_cloud_views_device"):
        with pytest.raises(NotImplementedError, match=name):
            getattr(est, name)()


def test_net_refuses_fp16_by_name():
    """Before anything touches a device: the storage type is refused in the constructor's own checks."""
    from rgbmanip_amd import _lib
    from rgbmanip_amd.adapose import AdaPoseNet
    with pytest.raises(_lib.RgbmError, match="fp16"):
        AdaPoseNet({}, dtype="fp16", arch="realworld")
    for key in ("graph", "dropout"):
        with pytest.raises(_lib.RgbmError, match=key):
            AdaPoseNet({}, dtype="bf16", arch="realworld", **{key: 1})
