"""The `direct_regression: False`, `use_depth: False` branch of AdaPoseEstimator_v5.predict (interface_v5.py:340-346): NOCS matches ->
triangulation -> scale -> EPnP-RANSAC -> VVS refinement.

PARITY UNPINNED against OpenCV itself (oracle/pnp_ref.py says why): the CPU tests check the restatement against ground truth it
must recover on seeded two-view cases and against the algebra it restates; the GPU test checks csrc/pnp.hip against the restatement
under the shared hash stream."""
import numpy as np
import pytest

from oracle import pnp_ref
from rgbmanip_amd import synth


def _run_oracle(case, seed=5):
    c = synth.pnp_case(case)
    bbox, info = pnp_ref.pnp_bbox_world(c["nocs1"], c["pts1"], c["nocs2"], c["pts2"], c["K"], c["E1"], c["E2"], seed=seed, pose=case)
    return c, bbox, info


def test_oracle_recovers_the_ground_truth_pose_without_outliers():
    c, bbox, info = _run_oracle(0)
    assert info["n_matches"] > 500 and abs(info["scale"] - c["scale"]) < 2e-3 * c["scale"]
    assert info["ransac_ok"] and info["n_inliers"] > 1000
    assert np.abs(info["R"] - c["R"]).max() < 2e-3 and np.abs(info["t"] - c["t"]).max() < 2e-3
    # the box: corners of size 2 * max|nocs| * scale under (R, t), taken to the world by inv(E1)
    half = np.abs(c["nocs1"]).max(axis=0) * info["scale"]
    corners = np.array([[sx, sy, sz] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)], dtype=np.float64)
    cam = (corners * half) @ info["R"].T + info["t"]
    Ei = np.linalg.inv(c["E1"])
    expect = cam @ Ei[:3, :3].T + Ei[:3, 3]
    # same corner set (the reference's sign table orders them differently)
    d = np.abs(bbox[:, None, :] - expect[None, :, :]).max(axis=2)
    assert (d.min(axis=1) < 1e-5).all()


def test_oracle_epnp_is_exact_on_noise_free_points():
    rng = np.random.default_rng(3)
    K = np.array([[439.0, 0, 320.0], [0, 439.0, 240.0], [0, 0, 1.0]])
    for n in (5, 6, 40):
        pw = rng.uniform(-0.2, 0.2, (n, 3))
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] *= -1
        t = np.array([0.05, -0.03, 0.8])
        cam = pw @ q.T + t
        uv = (cam @ K.T)[:, :2] / cam[:, 2:3]
        R, tt = pnp_ref.epnp(pw, uv, K)
        assert np.abs(R - q).max() < 1e-6 and np.abs(tt - t).max() < 1e-6, n


def test_oracle_triangulation_and_refinement():
    c = synth.pnp_case(0)
    K, E1, E2 = c["K"], c["E1"], c["E2"]
    X = np.array([[0.02, -0.01, 0.41, 1.0], [-0.1, 0.05, 0.35, 1.0]]).T
    P1, P2 = K @ E1[:3], K @ E2[:3]
    x1, x2 = P1 @ X, P2 @ X
    Xh = pnp_ref.triangulate_points(P1, P2, x1[:2] / x1[2], x2[:2] / x2[2])
    assert np.abs(Xh / Xh[3] - X).max() < 1e-9
    # VVS pulls a perturbed pose back to the exact one on noise-free pixels
    pw = c["nocs1"].astype(np.float64) * c["scale"]
    cam = pw @ c["R"].T + c["t"]
    uv = (cam @ K.T)[:, :2] / cam[:, 2:3]
    dR = pnp_ref.rodrigues_to_R(np.array([0.02, -0.015, 0.01]))
    R, t = pnp_ref.refine_vvs(pw, uv, K, dR @ c["R"], c["t"] + np.array([0.01, -0.005, 0.02]))
    assert np.abs(R - c["R"]).max() < 1e-6 and np.abs(t - c["t"]).max() < 1e-6


def test_oracle_no_match_gives_the_default_box():
    c, bbox, info = _run_oracle(3)
    assert info["n_matches"] == 0 and np.allclose(bbox, pnp_ref.DEFAULT_BBOX)


@pytest.mark.gpu
def test_device_pnp_branch_matches_the_restatement():
    """csrc/pnp.hip (one workgroup per pose) against oracle/pnp_ref.py on five seeded cases in one batch, same hash stream: match
    count and scale exactly / to 1e-12, the RANSAC bookkeeping, and the refined pose and world box to 5e-6 / 1e-5 (both sides run
    the same Gauss-Newton iteration from EPnP starts that agree to rounding — their small dense solvers differ, Jacobi / QR vs
    LAPACK — and stop by the same rule, 1e-6 on the change of the residual, which leaves either side ~1e-6 from the fixed point)."""
    import torch
    from rgbmanip_amd.adapose import postprocess_pnp
    cases = [synth.pnp_case(k) for k in range(5)]
    st = lambda k, dt: torch.from_numpy(np.stack([c[k] for c in cases]).astype(dt)).cuda()  # noqa: E731
    seed = 5
    bbox, srt, info, valid = postprocess_pnp(st("nocs1", np.float32), st("pts1", np.float32), st("nocs2", np.float32), st("pts2", np.float32),
                                             st("K", np.float64), st("E1", np.float64), st("E2", np.float64), seed=seed)
    torch.cuda.synchronize()
    bbox, srt, info, valid = bbox.cpu().numpy(), srt.cpu().numpy(), info.cpu().numpy(), valid.cpu().numpy()
    for k, c in enumerate(cases):
        eb, ei = pnp_ref.pnp_bbox_world(c["nocs1"], c["pts1"], c["nocs2"], c["pts2"], c["K"], c["E1"], c["E2"], seed=seed, pose=k)
        assert info[k, 0] == ei["n_matches"], (k, info[k], ei)
        if not np.isfinite(ei["scale"]):
            assert valid[k] == 0 and np.allclose(bbox[k], pnp_ref.DEFAULT_BBOX)
            continue
        assert abs(srt[k, 0] - ei["scale"]) <= 1e-12 * ei["scale"], (k, srt[k, 0], ei["scale"])
        assert info[k, 1] == int(ei["ransac_ok"]) and valid[k] == 1
        assert info[k, 3] == ei["n_examined"], (k, info[k], ei["n_examined"])
        assert abs(int(info[k, 2]) - ei["n_inliers"]) <= 2, (k, info[k], ei["n_inliers"])        # points on the 3-pixel edge may flip
        assert np.abs(srt[k, 1:10].reshape(3, 3) - ei["R"]).max() < 5e-6, (k, np.abs(srt[k, 1:10].reshape(3, 3) - ei["R"]).max())
        assert np.abs(srt[k, 10:13] - ei["t"]).max() < 5e-6
        assert np.abs(bbox[k] - eb).max() < 1e-5, (k, np.abs(bbox[k] - eb).max())


@pytest.mark.gpu
def test_estimator_plugin_pnp_branch_runs_end_to_end():
    """cfg direct_regression: False, use_depth: False through `AdaPoseEstimator_v5.estimate` (host preparation) and
    `estimate_device`: the branch no longer raises; with random-init weights the two views' NOCS rarely match, so the result is the
    default box or a finite box — either way finite and of the right shape, and both preparation paths agree."""
    import torch
    from rgbmanip_amd.config import ADAPOSE_CFGS
    from rgbmanip_amd.estimator import AdaPoseEstimator_v5
    cfg = dict(ADAPOSE_CFGS["adapose_cabinet"], load=False, direct_regression=False, use_depth=False, hip_prepare_seed=3)
    sd = synth.adapose_state_dict(seed=0, prefix="module.")
    n = 2
    yy, xx = np.mgrid[0:480, 0:640]
    g = np.random.default_rng(1)
    rgb1 = g.random((n, 480, 640, 3), dtype=np.float32)
    rgb2 = g.random((n, 480, 640, 3), dtype=np.float32)
    m1 = np.stack([((yy - 240) / 70.0) ** 2 + ((xx - 300 - 10 * i) / 90.0) ** 2 <= 1 for i in range(n)])
    m2 = np.stack([((yy - 250) / 60.0) ** 2 + ((xx - 330 + 10 * i) / 80.0) ** 2 <= 1 for i in range(n)])
    K = np.tile(np.array([[439.31, 0, 320.0], [0, 439.31, 240.0], [0, 0, 1.0]])[None], (n, 1, 1))
    base = synth.adapose_inputs(n, seed=9)
    host = AdaPoseEstimator_v5(None, dict(cfg, hip_prepare="host"), None, state_dict=sd, dtype="fp32")
    host.rng = ("hash", 3)
    dev = AdaPoseEstimator_v5(None, dict(cfg, hip_prepare="device"), None, state_dict=sd, dtype="fp32")
    bh = host.estimate(K, rgb1, m1, base["E1"], rgb2, m2, base["E2"])
    bd = dev.estimate(K, rgb1, m1, base["E1"], rgb2, m2, base["E2"])
    assert bh.shape == (n, 8, 3) and np.isfinite(bh).all() and np.isfinite(bd).all()
    np.testing.assert_allclose(bd, bh, rtol=1e-6, atol=1e-6)
