"""CPU: the adapose_v4 plugin's import path, the numpy restatement of its regressed box tail pinned to the reference's own results
(tests/golden/postproc_v4.npz, tools/make_goldens.py postproc_v4), and the host preparation with and without the ImageNet step."""
import os

import numpy as np
import pytest

import postproc_v4_ref
from rgbmanip_amd import _lib, compat, config, estimator, host_prepare, synth


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "postproc_v4.npz"))


def test_compat_serves_interface_v4():
    """train.py:36 / heuristic_pose.py:10 / homing.py:10 import the v4 estimator by this path; train.py:234-236 builds it for
    pose_estimator.name == "adapose_v4"."""
    compat.install()
    try:
        from models.pose_estimator.AdaPose.interface_v4 import AdaPoseEstimator_v4
        from models.pose_estimator.AdaPose.interface_v5 import AdaPoseEstimator_v5
        assert AdaPoseEstimator_v4 is estimator.AdaPoseEstimator_v4
        assert issubclass(AdaPoseEstimator_v4, estimator.BasePoseEstimator) and AdaPoseEstimator_v4 is not AdaPoseEstimator_v5
    finally:
        compat.uninstall()
    assert config.adapose_cfg(name="adapose_v4")["name"] == "adapose_v4" and config.adapose_cfg()["name"] == "adapose_v5"


def test_v4_hooks_follow_the_task_name():
    """interface_v4.py:52-58: ImageNet Normalize for task "pots" only; v5 always normalises (interface_v5.py:52-54)."""
    for cls, task, want in ((estimator.AdaPoseEstimator_v4, "pots", True), (estimator.AdaPoseEstimator_v4, "one_door_cabinet", False),
                            (estimator.AdaPoseEstimator_v4, "mugs", False), (estimator.AdaPoseEstimator_v5, "mugs", True)):
        est = cls.__new__(cls)                                   # host logic only: no device net
        est.cfg = config.adapose_cfg(task)
        assert est._normalize is want, (cls.__name__, task)


def test_new_entry_points_are_declared_and_bound():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rgbm.h")).read()
    for name in ("rgbm_prepare_inputs_opt", "rgbm_adapose_postprocess_regressed"):
        assert f"int {name}(" in src and name in _lib.SIGNATURES
    # rgbm_prepare_inputs_ex's arguments behind (rgb, pixel_type, normalize)
    ex, opt = _lib.SIGNATURES["rgbm_prepare_inputs_ex"][1], _lib.SIGNATURES["rgbm_prepare_inputs_opt"][1]
    assert opt[0] == ex[0] and opt[3:] == ex[1:] and len(opt) == len(ex) + 2


def test_restatement_reproduces_the_reference_boxes(golden):
    """Not exact, near 1e-16: scale and the float32 camera-frame box are restated bit for bit (the scale is compared exactly below); the
    float64 world transform sums its three products in another order than the reference's matrix product.  Measured here: largest
    normalised error 2.3e-16 (one float64 rounding); bound 2e-15."""
    g = golden
    assert len(g["bbox"]) == 12
    box, scale, valid = postproc_v4_ref.bbox_world_batch(g["nocs"], g["r"], g["t"], g["s"], g["E1"])
    assert np.array_equal(scale.view(np.uint32), g["scale"].view(np.uint32))
    worst = 0.0
    for i in range(len(box)):
        is_default = np.array_equal(g["bbox"][i], postproc_v4_ref.DEFAULT_BBOX)
        assert bool(valid[i]) == (not is_default), (i, str(g["kinds"][i]))
        worst = max(worst, float(np.abs(box[i] - g["bbox"][i]).max() / np.abs(g["bbox"][i]).max()))
    print("restatement vs golden: largest normalised error", worst)
    assert worst < 2e-15
    assert [str(k) for k in g["kinds"][valid == 0]] == ["nan_s", "inf_nocs", "nan_nocs", "nan_E"]
    # a singular extrinsic (np.linalg.inv raises in the reference) is a default box here
    E = g["E1"][2].copy()
    E[2] = 0.0
    b, _, v = postproc_v4_ref.bbox_world(g["nocs"][2], g["r"][2], g["t"][2], g["s"][2], E)
    assert v == 0 and np.array_equal(b, postproc_v4_ref.DEFAULT_BBOX)


def test_host_prepare_without_normalisation_reproduces_the_reference_crop(golden):
    """Frame 0, task one_door_cabinet: plain ToTensor.  host_prepare's bilinear resize is the float32 arithmetic of the resize the
    reference ran, and nothing follows it: the crop is reproduced bit for bit, from float frames and from the bytes."""
    g = golden
    rgb8, mask, K = synth.crop_frames(seed=0)
    S = int(g["crop0_size"])
    assert str(g["crop0_task"]) == "one_door_cabinet" and int(g["crop0_n_distinct"]) == 1024          # the random-subset branch
    for frames in (rgb8[0].astype(np.float32) / np.float32(255.0), rgb8[0]):
        view, choose, _, Kn = host_prepare.prepare_model_input(frames, mask[0], K[0], S, np.random.default_rng(0), normalize=False)
        assert view.dtype.is_floating_point and np.array_equal(view.numpy(), g["crop0_img"])
        assert np.array_equal(Kn, g["crop0_K"]) and len(np.unique(choose)) == 1024
    # the estimator method takes the switch from the task name
    est = estimator.AdaPoseEstimator_v4.__new__(estimator.AdaPoseEstimator_v4)
    est.cfg = dict(config.adapose_cfg("one_door_cabinet"), name="adapose_v4")
    est.rng = np.random.default_rng(0)
    assert np.array_equal(est.prepare_model_input(rgb8[0], mask[0], K[0], S)[0].numpy(), g["crop0_img"])
    assert float(g["crop0_img"].min()) >= 0.0 and float(g["crop0_img"].max()) <= 1.0


def test_host_prepare_normalises_for_pots(golden):
    """Frame 1, task pots: ToTensor + Normalize, within the bound tests/test_host_logic.py holds host_prepare to (rtol 1e-6, atol 1e-6);
    fewer than 1024 mask pixels, so the wrap-padded indices are deterministic and compared too."""
    g = golden
    rgb8, mask, K = synth.crop_frames(seed=0)
    S = int(g["crop1_size"])
    assert str(g["crop1_task"]) == "pots" and int(g["crop1_n_distinct"]) < 1024
    est = estimator.AdaPoseEstimator_v4.__new__(estimator.AdaPoseEstimator_v4)
    est.cfg = dict(config.adapose_cfg("pots"), name="adapose_v4")
    est.rng = np.random.default_rng(0)
    view, choose, pts2d, Kn = est.prepare_model_input(rgb8[1].astype(np.float32) / np.float32(255.0), mask[1], K[1], S)
    print("pots crop: largest difference", float(np.abs(view.numpy() - g["crop1_img"]).max()))
    np.testing.assert_allclose(view.numpy(), g["crop1_img"], rtol=1e-6, atol=1e-6)
    assert np.array_equal(choose, g["crop1_choose"])
    np.testing.assert_allclose(pts2d, g["crop1_pts2d"], rtol=1e-6)
    np.testing.assert_allclose(Kn, g["crop1_K"])
    plain = host_prepare.prepare_model_input(rgb8[1], mask[1], K[1], S, np.random.default_rng(0), normalize=False)[0].numpy()
    assert np.abs(plain - g["crop1_img"]).max() > 0.5              # the switch is not a no-op
