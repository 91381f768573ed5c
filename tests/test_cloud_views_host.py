"""CPU-only checks of the multi-view depth fusion: the C ABI declares, binds and exports the three entry points,
their bounds come back as error codes naming the function, the float64 twin `depth_fusion_ref` is `depth_consistency_ref` at V = 2, and
the sphere scenes of the GPU tests hold the preconditions those tests rest on."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cloud_views_cases import SCENES, assert_scene_preconditions, sphere_ref, sphere_views
from rgbmanip_amd import _lib, synth
from rgbmanip_amd.cloud import depth_consistency_ref, depth_fusion_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rgbm_depth_fusion", "rgbm_cloud_pack_views", "rgbm_cloud_gather_views")


def test_library_exports_the_views_entry_points():
    src = open(os.path.join(ROOT, "include", "rgbm.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(rgbm_[a-z0-9_]+)\s*\(", src))
    lib = _lib.load()
    for n in NEW_SYMBOLS:
        assert n in declared, f"{n} is not declared in include/rgbm.h"
        assert n in _lib.SIGNATURES, f"{n} is not bound in _lib.SIGNATURES"
        assert getattr(lib, n) is not None
    assert lib.rgbm_version() == 100


def test_bounds_are_refused_before_any_launch():
    """Plain ctypes on the built library, no device: every check precedes the launch."""
    lib = _lib.load()
    buf = (C.c_double * 4)()
    p = C.cast(buf, C.c_void_p)

    def fuse(depth=p, K=p, E=p, n=1, V=3, s=8, px=1.0, rel=0.01, cmin=0.0, n_min=1, fused=p, keep=p, nviews=p):
        return lib.rgbm_depth_fusion(depth, None, None, K, E, n, V, s, px, rel, cmin, n_min, fused, keep, nviews, None, None)
    cases = [dict(V=1), dict(V=17), dict(n_min=0), dict(n_min=3), dict(V=2, n_min=2), dict(n=0), dict(n=21846), dict(n=4096, V=16),
             dict(s=0), dict(s=4097), dict(depth=None), dict(K=None), dict(E=None), dict(fused=None), dict(keep=None), dict(nviews=None),
             dict(px=-1.0), dict(px=float("nan")), dict(rel=-0.5), dict(rel=float("inf")), dict(cmin=-1.0), dict(cmin=float("nan"))]
    for kw in cases:
        assert fuse(**kw) != 0 and b"depth_fusion" in lib.rgbm_last_error(), kw

    def pack(fused=p, keep=p, K=p, E=p, n=1, V=3, s=8, cap=4, cloud=p, index=p, count=p):
        return lib.rgbm_cloud_pack_views(fused, keep, K, E, n, V, s, cap, cloud, index, count, None)
    cases = [dict(fused=None), dict(keep=None), dict(K=None), dict(E=None), dict(count=None), dict(V=0), dict(V=17), dict(n=0), dict(n=65536),
             dict(s=0), dict(s=4097), dict(cap=-1), dict(cloud=None), dict(index=None)]
    for kw in cases:
        assert pack(**kw) != 0 and b"cloud_pack_views" in lib.rgbm_last_error(), kw

    def gather(maps=p, index=p, n=1, V=3, S2=4, C_=3, cap=2, out=p):
        return lib.rgbm_cloud_gather_views(maps, index, n, V, S2, C_, cap, out, None)
    for kw in (dict(maps=None), dict(index=None), dict(out=None), dict(V=0), dict(V=17), dict(S2=0), dict(C_=0), dict(C_=5), dict(cap=-1),
               dict(n=-1)):
        assert gather(**kw) != 0 and b"cloud_gather_views" in lib.rgbm_last_error(), kw
    assert gather(maps=None, index=None, out=None, cap=0) == 0      # nothing to do


def test_twin_at_two_views_is_the_two_view_twin():
    """V = 2, n_min = 1 on the sphere scene: view 0 is depth_consistency_ref(a = 0, b = 1), view 1 the opposite direction — the same
    float64 numbers, with and without confidence and mask."""
    inp = synth.adapose_inputs(3, seed=5)
    d1, d2 = synth.sphere_depth(inp["K1"], inp["E1"]), synth.sphere_depth(inp["K2"], inp["E2"])
    depth, K, E = np.stack([d1, d2], 1), np.stack([inp["K1"], inp["K2"]], 1), np.stack([inp["E1"], inp["E2"]], 1)
    g = np.random.default_rng(3)
    conf = g.random(depth.shape, dtype=np.float32)
    mask = (g.random(depth.shape) < 0.8).astype(np.uint8)
    for kw in ({}, dict(conf=conf, mask=mask, conf_min=0.4)):
        r = depth_fusion_ref(depth, K, E, n_min=1, **kw)
        assert r["fused"].dtype == np.float64 and r["keep"].dtype == bool and r["nviews"].dtype == np.uint8 and r["agree"].dtype == np.uint16
        for a, b in ((0, 1), (1, 0)):
            pk = {} if not kw else dict(conf_a=conf[:, a], mask_a=mask[:, a], conf_min=0.4)
            two = depth_consistency_ref(depth[:, a], K[:, a], E[:, a], depth[:, b], K[:, b], E[:, b], **pk)
            assert two["keep"].sum() > 3000      # not an empty comparison: >= 3 x 4000 sampled pixels, 95 % kept, about half of them past conf and mask
            assert np.array_equal(r["keep"][:, a], two["keep"])
            assert np.array_equal(r["fused"][:, a], two["fused"], equal_nan=True)
            # nviews / agree ignore conf and mask; margin is the distance of reproj / rel from the thresholds, where sampled
            agrees = two["sampled"] & (two["reproj"] < 1.0) & (two["rel"] < 0.01)
            assert np.array_equal(r["nviews"][:, a], agrees.astype(np.uint8)) and np.array_equal(r["agree"][:, a], agrees.astype(np.uint16) << b)
            assert np.array_equal(np.isfinite(r["margin"][:, a, b, ..., 0]), two["sampled"])
            assert np.array_equal(r["margin"][:, a, b, ..., 0][two["sampled"]], np.abs(two["reproj"] - 1.0)[two["sampled"]])
            assert np.array_equal(r["margin"][:, a, b, ..., 1][two["sampled"]], np.abs(two["rel"] - 0.01)[two["sampled"]])
            assert np.isnan(r["margin"][:, a, a]).all()


@pytest.mark.parametrize("V", sorted(SCENES))
def test_sphere_scene_preconditions_and_n_min_monotonicity(V):
    rarest = assert_scene_preconditions(V)
    print(f"V={V}: rarest nviews value occurs {rarest} times")
    prev = None
    for n_min in range(1, V):
        r = sphere_ref(V, n_min, False)
        assert np.array_equal(r["keep"], r["nviews"] >= n_min)                       # no conf, no mask
        assert np.array_equal(np.isfinite(r["fused"]), r["keep"])
        assert np.array_equal(r["nviews"], sphere_ref(V, 1, False)["nviews"]) and np.array_equal(r["agree"], sphere_ref(V, 1, False)["agree"])
        if prev is not None:
            assert not (r["keep"] & ~prev).any() and r["keep"].sum() < prev.sum()     # keep(n_min + 1) is a strict subset here
        prev = r["keep"]
    r = sphere_ref(V, 1, False)
    bits = sum(((r["agree"] >> b) & 1).astype(np.uint8) for b in range(V))
    assert np.array_equal(bits, r["nviews"])
    for a in range(V):
        assert not ((r["agree"][:, a] >> a) & 1).any()                               # a view is not its own witness
    k = r["keep"]
    depth = sphere_views(V)[0]
    assert np.abs(r["fused"][k] / depth[k].astype(np.float64) - 1).max() < 0.01       # a mean of depths within rel_max of d


def test_twin_argument_errors():
    d = np.ones((1, 3, 4, 4), dtype=np.float32)
    K, E = np.tile(np.eye(3), (1, 3, 1, 1)), np.tile(np.eye(4), (1, 3, 1, 1))
    for kw in (dict(n_min=0), dict(n_min=3)):
        with pytest.raises(ValueError, match="n_min"):
            depth_fusion_ref(d, K, E, **kw)
    with pytest.raises(ValueError, match="V"):
        depth_fusion_ref(d[:, :1], K[:, :1], E[:, :1])


def test_estimator_refusals_need_no_device():
    from rgbmanip_amd.estimator import AdaPoseEstimator_baseline, AdaPoseEstimator_v4, AdaPoseEstimator_v5
    for cls in (AdaPoseEstimator_v5, AdaPoseEstimator_v4):
        assert callable(cls.estimate_cloud_views) and callable(cls.estimate_cloud_views_device)
    est = AdaPoseEstimator_v5.__new__(AdaPoseEstimator_v5)      # the option checks precede any device work
    est.cfg = {"img_size": 224, "hip_ransac_seed": 7}
    est.prepare_mode, est.upload_mode = "host", "frames"
    with pytest.raises(ValueError, match="hip_prepare"):
        est.estimate_cloud_views(None, None, None, None)
    est.prepare_mode, est.upload_mode = "device", "windows"
    for call in (est.estimate_cloud_views, est.estimate_cloud_views_device):
        with pytest.raises(ValueError, match="hip_upload"):
            call(None, None, None, None)
    est.upload_mode = "frames"
    with pytest.raises(ValueError, match="max_points"):
        est.estimate_cloud_views_device(None, None, None, None, max_points=-1)
    assert est._views_options(1, 1.0, 0.01, 0.0, True, None, True, None).fit_seed == 7
    assert est._views_options(1, 1.0, 0.01, 0.0, True, None, False, 3).fit_seed is None
    base = AdaPoseEstimator_baseline.__new__(AdaPoseEstimator_baseline)
    for name in ("estimate_cloud_views", "estimate_cloud_views_device"):
        with pytest.raises(NotImplementedError, match=name):
            getattr(base, name)(None, None, None, None)
