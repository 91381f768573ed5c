"""CPU-only: the seeded Dropout2d generator (numpy restatement, tests/dropout_ref.py) and the estimator's cfg keys for it."""
import numpy as np
import pytest

from dropout_ref import keep_bits, masks, mix64, scale, threshold
from rgbmanip_amd import estimator


def test_mix64_is_splitmix64_finaliser():
    # splitmix64 with state 0: first output 0xE220A8397B1DCDAF = mix64(0 + 0x9E3779B97F4A7C15)
    assert int(mix64(np.uint64(0x9E3779B97F4A7C15))) == 0xE220A8397B1DCDAF
    assert int(mix64(np.uint64(0))) == 0


def test_keep_fraction_and_factor_values():
    p = 0.15
    m = masks(p, seed=7, B=2048)                 # 2048 poses x 2 views x 320 channels = 1.3e6 draws
    assert m.size >= 10 ** 6
    vals = set(np.unique(m).tolist())
    assert vals <= {0.0, float(np.float32(1 / 0.85))}, vals
    assert scale(p) == np.float32(1 / 0.85)
    q = 1 - threshold(p) / 2.0 ** 24
    frac = float((m != 0).mean())
    sigma = np.sqrt(q * (1 - q) / m.size)
    assert abs(frac - 0.85) < 4 * sigma, (frac, sigma)
    assert abs(q - 0.85) < 1e-7


def test_keys_are_distinct_and_independent():
    # every (pose, view, site, channel) of a batch has its own uniform: no two of 64 poses' 4 x 320 keys collide in 24 bits more
    # often than chance allows, and neighbouring keys are uncorrelated
    pose, view, ch = np.meshgrid(np.arange(64), np.arange(2), np.arange(256), indexing="ij")
    u0 = keep_bits(3, pose, view, 0, ch).astype(np.float64) / 2 ** 24
    u1 = keep_bits(3, pose, view, 1, ch).astype(np.float64) / 2 ** 24
    for a, b in ((u0, u1), (u0[:, 0], u0[:, 1]), (u0[:-1], u0[1:]), (u0[..., :-1], u0[..., 1:])):
        c = np.corrcoef(a.ravel(), b.ravel())[0, 1]
        assert abs(c) < 0.05, c
    assert len(np.unique(u0)) > 0.99 * u0.size
    # seeds: different seeds give unrelated masks, the same seed the same ones
    a, b = masks(0.15, 0, 64), masks(0.15, 1, 64)
    assert np.array_equal(a, masks(0.15, 0, 64))
    agree = float(((a != 0) == (b != 0)).mean())
    assert abs(agree - (0.85 ** 2 + 0.15 ** 2)) < 0.02, agree


def test_masks_do_not_depend_on_batching():
    one = masks(0.15, 5, 8)
    two = [masks(0.15, 5, 4, first_pose=0), masks(0.15, 5, 4, first_pose=4)]
    for view in range(2):
        joined = np.concatenate([t[view * 4:(view + 1) * 4] for t in two])
        assert np.array_equal(one[view * 8:(view + 1) * 8], joined)


def test_estimator_dropout_cfg():
    assert estimator.dropout_cfg({}) == ("eval", 0.0, 0)
    assert estimator.dropout_cfg({"hip_as_shipped": True}) == ("per_sample", 0.15, 0)
    assert estimator.dropout_cfg({"hip_as_shipped": True, "hip_dropout_seed": 9}) == ("per_sample", 0.15, 9)
    assert estimator.dropout_cfg({"hip_dropout": 0.3, "hip_dropout_seed": 2}) == ("eval", 0.3, 2)
    assert estimator.dropout_cfg({"hip_as_shipped": True, "hip_dropout": 0.0}) == ("per_sample", 0.0, 0)
    with pytest.raises(ValueError):
        estimator.dropout_cfg({"hip_dropout": 1.0})


def test_mixed_object_net_refuses_dropout():
    from rgbmanip_amd.mixed import MixedObjectNet
    with pytest.raises(ValueError, match="Dropout2d"):
        MixedObjectNet({0: {}}, dropout=0.15)


def test_as_shipped_golden_masks_are_reference_dropout(golden_dir):
    import os
    g = np.load(os.path.join(golden_dir, "adapose_b2_dropout.npz"))
    m = g["masks"]
    assert m.shape == (4, 320) and m.dtype == np.float32
    assert set(np.unique(m).tolist()) <= {0.0, float(np.float32(1.0) / np.float32(0.85))}
    assert 0 < (m == 0).sum() < m.size
