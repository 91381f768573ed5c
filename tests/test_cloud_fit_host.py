"""CPU-only checks of the dense NOCS map / cloud fit feature: the C ABI declares, binds and exports the new entry
points, their argument errors come back without a device, and the float64 twin `cloud_similarity_ref` agrees with the oracle's
similarity RANSAC on planted similarities whose residuals stay clear of the inlier threshold."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cloud_fit_cases import CASES, SEED, oracle_fit, planted
from rgbmanip_amd import _lib
from rgbmanip_amd.cloud import cloud_similarity_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rgbm_adapose_forward_maps", "rgbm_nocs_map", "rgbm_cloud_gather", "rgbm_cloud_similarity", "rgbm_cloud_similarity_scratch_bytes")


def test_library_exports_the_new_entry_points():
    src = open(os.path.join(ROOT, "include", "rgbm.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(rgbm_[a-z0-9_]+)\s*\(", src))
    lib = _lib.load()
    for n in NEW_SYMBOLS:
        assert n in declared, f"{n} is not declared in include/rgbm.h"
        assert n in _lib.SIGNATURES, f"{n} is not bound in _lib.SIGNATURES"
        assert getattr(lib, n) is not None


@pytest.mark.parametrize("k", range(len(CASES)), ids=[c[0] for c in CASES])
def test_twin_matches_the_oracle_and_the_inputs_keep_their_margin(k):
    name, m, cap, outliers, mirror, special = CASES[k]
    nocs, cloud, count = planted(k, m, cap, outliers, mirror, special)
    pose = 1                                             # the second pose of a call: the sample stream depends on the pose index
    N2, C2, ct2 = np.stack([nocs, nocs]), np.stack([cloud, cloud]), np.stack([count, count])
    bbox, srt, info, valid = cloud_similarity_ref(N2, C2, ct2, seed=SEED)
    want, s, R, t, margin, scan = oracle_fit(nocs, cloud, count, SEED, pose)
    print(f"{name}: smallest relative distance of a residual to its threshold {margin:.3e}, scan {scan}, scale {s}")
    # a condition on the inputs: no residual so close to its threshold that the last bits of a hypothesis decide an inlier count
    assert margin > 1e-9, (name, margin)
    used = int(min(cap, int(count.sum())))
    assert info[pose, 0] == used
    assert tuple(info[pose, 1:]) == scan, (name, info[pose], scan)
    if s is None:
        assert valid[pose] == 0 and np.isnan(srt[pose, 0])
        np.testing.assert_array_equal(bbox[pose], want)
        assert np.all(bbox[pose] >= 10.0)
        return
    assert valid[pose] == 1
    np.testing.assert_allclose(srt[pose, 0], s, rtol=1e-12, atol=0)
    np.testing.assert_allclose(srt[pose, 1:10].reshape(3, 3), R, rtol=0, atol=1e-12)
    np.testing.assert_allclose(srt[pose, 10:], t, rtol=0, atol=1e-12)
    np.testing.assert_allclose(bbox[pose], want, rtol=0, atol=1e-12)


def test_cases_cover_what_they_are_meant_to():
    out = {}
    for k, (name, m, cap, outliers, mirror, special) in enumerate(CASES):
        nocs, cloud, count = planted(k, m, cap, outliers, mirror, special)
        out[name] = cloud_similarity_ref(nocs[None], cloud[None], count[None], seed=SEED)
    for name in ("m5", "m37", "m1024_clean", "m1024_o20", "m1024_o45", "m1024_mirror", "m4099_o20", "m4099_o45", "count_over_cap"):
        assert out[name][3][0] == 1, name
    for name in ("m1024_none", "m4", "nan_row"):
        assert out[name][3][0] == 0, name
    assert out["m4"][2][0].tolist() == [4, -1, 0, 0] and out["nan_row"][2][0].tolist() == [200, -1, 0, 0]
    assert out["m1024_none"][2][0, 1] == -1 and out["m1024_none"][2][0, 3] == 128      # scanned everything, kept nothing
    assert out["count_over_cap"][2][0, 0] == 300
    R = out["m1024_mirror"][1][0, 1:10].reshape(3, 3)
    assert abs(np.linalg.det(R) - 1) < 1e-9                                          # a rotation, although the data are mirrored
    s = out["m1024_clean"][1][0, 0]
    assert 0.1 <= s <= 0.4


def test_argument_errors_need_no_device():
    lib = _lib.load()
    buf = (C.c_double * 8)()
    p = C.cast(buf, C.c_void_p)
    # forward_maps: all three maps NULL, or a confidence map without a depth map
    assert lib.rgbm_adapose_forward_maps(None, 1, p, p, p, p, p, p, p, p, 1024, None, None, None, None, None) < 0
    assert b"NULL" in lib.rgbm_last_error()
    assert lib.rgbm_adapose_forward_maps(None, 1, p, p, p, p, p, p, p, p, 1024, None, None, p, p, None) < 0
    assert b"conf_map" in lib.rgbm_last_error()
    assert lib.rgbm_adapose_forward_maps(None, 1, p, p, p, p, p, p, p, p, 1024, None, None, None, p, None) < 0
    assert b"forward_maps arguments" in lib.rgbm_last_error()
    assert lib.rgbm_nocs_map(None, p, 1, 64, p, None) < 0 and b"nocs_map arguments" in lib.rgbm_last_error()
    for kw in (dict(C_=0), dict(C_=5), dict(S2=0), dict(cap=-1), dict(n=-1)):
        a = dict(n=1, S2=4, C_=3, cap=2)
        a.update(kw)
        assert lib.rgbm_cloud_gather(p, None, p, a["n"], a["S2"], a["C_"], a["cap"], p, None) < 0 and b"cloud_gather" in lib.rgbm_last_error(), kw
    assert lib.rgbm_cloud_gather(None, None, p, 1, 4, 3, 2, p, None) < 0 and b"cloud_gather arguments" in lib.rgbm_last_error()
    assert lib.rgbm_cloud_gather(None, None, None, 1, 4, 3, 0, None, None) == 0      # nothing to do
    nb = C.c_size_t()
    assert lib.rgbm_cloud_similarity_scratch_bytes(2, 100352, C.byref(nb)) == 0 and nb.value > 0 and nb.value % 8 == 0
    one = nb.value
    assert lib.rgbm_cloud_similarity_scratch_bytes(4, 100352, C.byref(nb)) == 0 and nb.value == 2 * one
    assert lib.rgbm_cloud_similarity_scratch_bytes(1, 0, C.byref(nb)) < 0
    sim = lambda n=1, cap=8, nocs=p, scratch=p, nbytes=1 << 20: lib.rgbm_cloud_similarity(nocs, p, p, n, cap, 0, p, p, p, p, scratch, nbytes, None)  # noqa: E731
    assert sim(cap=0) < 0 and b"cap" in lib.rgbm_last_error()
    assert sim(nocs=None) < 0 and b"cloud_similarity arguments" in lib.rgbm_last_error()
    assert sim(nbytes=8) < 0 and b"scratch" in lib.rgbm_last_error()
    assert sim(n=65536, nbytes=1 << 40) < 0 and b"65535" in lib.rgbm_last_error()
    assert sim(n=0) == 0


def test_python_argument_errors():
    with pytest.raises(ValueError, match="nocs and cloud"):
        cloud_similarity_ref(np.zeros((1, 4, 3)), np.zeros((1, 5, 3)), np.zeros((1, 2), dtype=np.int32))
    with pytest.raises(ValueError, match="count"):
        cloud_similarity_ref(np.zeros((2, 4, 3)), np.zeros((2, 4, 3)), np.zeros((1, 2), dtype=np.int32))
    from rgbmanip_amd.estimator import AdaPoseEstimator_v4, AdaPoseEstimator_v5
    for cls in (AdaPoseEstimator_v5, AdaPoseEstimator_v4):
        assert callable(cls.estimate_cloud_pose) and callable(cls.estimate_cloud_pose_device)
    est = AdaPoseEstimator_v5.__new__(AdaPoseEstimator_v5)      # the option checks precede any device work
    est.cfg = {"img_size": 224, "hip_ransac_seed": 7}
    est.prepare_mode, est.view2_heads = "host", True
    with pytest.raises(ValueError, match="hip_prepare"):
        est.estimate_cloud_pose(None, [], [], [], [], [], [])
    est.prepare_mode, est.view2_heads = "device", False
    with pytest.raises(ValueError, match="hip_view2_heads"):
        est.estimate_cloud_pose_device(None, None, None, None, None, None, None)
    est.view2_heads = True
    with pytest.raises(ValueError, match="max_points"):
        est.estimate_cloud_pose_device(None, None, None, None, None, None, None, max_points=-1)
    assert est._cloud_options(1.0, 0.01, 0.0, True, None, fit_seed=None).fit_seed == 7
    assert est._cloud_options(1.0, 0.01, 0.0, True, None, fit_seed=3).fit_seed == 3
    assert est._cloud_options(1.0, 0.01, 0.0, True, None).fit_seed is None
