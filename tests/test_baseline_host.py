"""CPU-only checks of the baseline network's restatement, fixtures, schema and import surface (no GPU)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import baseline_ref as br  # noqa: E402

from rgbmanip_amd import adapose, synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT_KEYS = [f"view{v}_{k}" for k in ("nocs", "depth", "r", "t", "s") for v in (1, 2)]
E_REF32_MAX = 1e-5


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "adapose_baseline_b2.npz"))


@pytest.fixture(scope="module")
def small(golden_dir):
    return np.load(os.path.join(golden_dir, "view_fusion_small.npz"))


def _forward(dtype):
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    sd = br.to_sd(synth.baseline_state_dict(seed=0), dtype)
    inp = synth.adapose_inputs(2, seed=0)
    taps, stats = {}, {}
    out = br.baseline_forward(sd, inp["img1"], inp["choose1"], inp["img2"], inp["choose2"], taps=taps, stats=stats)
    return out, taps, stats


def test_restatement_float32_reproduces_the_reference(golden):
    """e_ref32 = max over the ten outputs and fused1 / fused2 of max|a - b| / max|b| between tests/baseline_ref.py in float32 and the
    reference class's golden: measured 5.0e-7 (view1_depth; the NOCS, t, s outputs and the fused rows are bit-equal).  Required <= 1e-5."""
    out, taps, stats = _forward(torch.float32)
    errs = {k: br.rel_err(out[k].numpy(), golden[k]) for k in OUT_KEYS}
    errs.update({k: br.rel_err(taps[k].numpy(), golden[k]) for k in ("fused1", "fused2")})
    print("e_ref32 per tensor:", errs)
    assert max(errs.values()) <= E_REF32_MAX, errs
    np.testing.assert_allclose(stats["rowmax"], golden["rowmax_mean"], rtol=1e-4)


def test_restatement_float64_records_the_reference_rounding(golden):
    """e_ref64: the reference's own float32 rounding, i.e. the golden against the float64 restatement.  Measured 2.8e-6 over the ten
    outputs (view1_depth) and 4.5e-6 over the fused rows (fused2); the scores of the golden batch reach |s| = 394.  Recorded, and
    bounded only by the sanity that float32 cannot be worse than 1e-4 on a conditioned fixture."""
    out, taps, _ = _forward(torch.float64)
    errs = {k: br.rel_err(golden[k], out[k].numpy()) for k in OUT_KEYS}
    errs.update({k: br.rel_err(golden[k], taps[k].numpy()) for k in ("fused1", "fused2")})
    print("e_ref64 per tensor:", errs)
    assert 0 < max(errs.values()) < 1e-4, errs


@pytest.mark.parametrize("B,P", [(3, 96), (1, 32)])
def test_view_fusion_twin_float64_against_the_reference_module(small, B, P):
    """adapose.view_fusion_ref (float64 numpy) against the reference ViewFusion's float32 outputs: measured 7.1e-7 / 5.3e-7."""
    sd = synth.baseline_state_dict(seed=0)
    t = f"b{B}_p{P}_"
    x1, x2 = synth.view_fusion_inputs(B, P, seed=0)
    np.testing.assert_array_equal(x1, small[t + "x1"])
    np.testing.assert_array_equal(x2, small[t + "x2"])
    y1, y2 = adapose.view_fusion_ref(sd, x1, x2)
    assert br.rel_err(small[t + "y1"], y1) <= E_REF32_MAX and br.rel_err(small[t + "y2"], y2) <= E_REF32_MAX
    # every block's outputs, through the torch restatement in float64
    blocks = []
    br.view_fusion(torch.from_numpy(x1).double(), torch.from_numpy(x2).double(), br.to_sd(sd, torch.float64), blocks_out=blocks)
    for i, (b1, b2) in enumerate(blocks):
        assert br.rel_err(small[t + f"blk{i}_y1"], b1.numpy()) <= E_REF32_MAX, i
        assert br.rel_err(small[t + f"blk{i}_y2"], b2.numpy()) <= E_REF32_MAX, i
    # the last block's outputs are the stack's, and the two twins agree
    assert br.rel_err(blocks[-1][0].numpy(), y1) < 1e-12 and br.rel_err(blocks[-1][1].numpy(), y2) < 1e-12


@pytest.mark.parametrize("regress_pose", [True, False])
def test_synth_schema_is_the_reference_state_dict(golden, regress_pose):
    tag = "" if regress_pose else "_nopose"
    keys, shapes = [str(k) for k in golden["sd_keys" + tag]], [str(s) for s in golden["sd_shapes" + tag]]
    sd = synth.baseline_state_dict(seed=0, regress_pose=regress_pose)
    assert list(sd.keys()) == keys
    assert ["x".join(str(d) for d in np.asarray(v).shape) for v in sd.values()] == shapes
    assert ("pose_mlp1.0.weight" in sd) == regress_pose
    # the tensors shared with v5 are the same draw; the query / key gain is the constant
    v5 = synth.adapose_state_dict(seed=0)
    for k in ("img_extractor.final.weight", "nocs_head.2.bias", "instance_color.0.weight"):
        np.testing.assert_array_equal(sd[k], v5[k])
    w = sd["view_fusion.blocks.2.fusion2.linears.1.weight"]
    assert np.abs(w).max() <= synth.BASELINE_QK_GAIN / np.sqrt(32) and np.abs(w).max() > 0.9 * synth.BASELINE_QK_GAIN / np.sqrt(32)
    assert np.abs(sd["view_fusion.blocks.2.fusion2.linears.2.weight"]).max() <= 1 / np.sqrt(32)


def test_golden_attention_is_neither_flat_nor_one_hot(golden):
    rm = golden["rowmax_mean"]
    assert rm.shape == (8,) and (rm >= 0.2).all() and (rm <= 0.9).all(), rm
    assert (golden["view1_depth"] > 0).any() and np.isfinite(golden["fused1"]).all()


def test_compat_serves_the_baseline_interface():
    from rgbmanip_amd import compat, estimator
    compat.install()
    try:
        from models.pose_estimator.AdaPose.interface_baseline import AdaPoseEstimator_baseline
        assert AdaPoseEstimator_baseline is estimator.AdaPoseEstimator_baseline
        assert issubclass(AdaPoseEstimator_baseline, estimator.AdaPoseEstimator_v5)
    finally:
        compat.uninstall()


def test_config_names_the_baseline_estimator():
    from rgbmanip_amd import config
    cfg = config.adapose_cfg(name="adapose_baseline")
    assert cfg["name"] == "adapose_baseline" and cfg["n_pts"] == 1024


def test_header_declares_and_library_exports_the_new_symbols():
    from rgbmanip_amd import _lib
    src = open(os.path.join(ROOT, "include", "rgbm.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load()
    for name in ("rgbm_adapose_create_baseline", "rgbm_view_fusion", "rgbm_view_fusion_scratch_bytes", "rgbm_depth_head"):
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    import ctypes as C
    n = C.c_size_t()
    assert lib.rgbm_view_fusion_scratch_bytes(256, 1024, C.byref(n)) == 0
    assert 0 < n.value <= 16 * 256 * 1024 * 32 * 4
    assert lib.rgbm_view_fusion_scratch_bytes(1, 48, C.byref(n)) != 0 and b"multiple of 32" in lib.rgbm_last_error()


def test_estimator_refuses_unsupported_keys_by_name():
    from rgbmanip_amd import config, estimator
    for key, val in (("hip_feature_cache", True), ("hip_dropout", 0.15), ("hip_as_shipped", True), ("hip_graph", True)):
        cfg = dict(config.adapose_cfg(name="adapose_baseline", load=False), **{key: val})
        with pytest.raises(ValueError, match=key):
            estimator.AdaPoseEstimator_baseline(None, cfg, None)
