"""CPU-only checks of the two-view consistency check and the packed cloud: the C ABI declares, binds and exports
the two entry points, their argument errors come back as negative codes with text, and the float64 twin `depth_consistency_ref` follows
rules 1-5 on scenes whose answer is known."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from rgbmanip_amd import _lib, synth
from rgbmanip_amd.cloud import depth_consistency_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rgbm_depth_consistency", "rgbm_cloud_pack")
S = 224


def test_library_exports_the_cloud_entry_points():
    src = open(os.path.join(ROOT, "include", "rgbm.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(rgbm_[a-z0-9_]+)\s*\(", src))
    lib = _lib.load()
    for n in NEW_SYMBOLS:
        assert n in declared, f"{n} is not declared in include/rgbm.h"
        assert n in _lib.SIGNATURES, f"{n} is not bound in _lib.SIGNATURES"
        assert getattr(lib, n) is not None


def test_argument_errors_are_negative_codes_with_text():
    """Plain ctypes on the built library, no device: every check precedes the launch."""
    lib = _lib.load()
    buf = (C.c_double * 4)()
    p = C.cast(buf, C.c_void_p)

    def cons(da=p, fused=p, keep=p, n=1, s=8, px=1.0, rel=0.01, cmin=0.0):
        return lib.rgbm_depth_consistency(da, None, None, p, p, p, p, p, n, s, px, rel, cmin, fused, None, None, keep, None)
    for kw in (dict(da=None), dict(fused=None), dict(keep=None)):
        assert cons(**kw) < 0 and b"depth_consistency arguments" in lib.rgbm_last_error(), kw
    for kw in (dict(n=0), dict(n=65536), dict(s=0), dict(s=4097)):
        assert cons(**kw) < 0 and b"65535" in lib.rgbm_last_error(), kw
    for kw in (dict(px=-1.0), dict(px=float("nan")), dict(rel=float("inf")), dict(rel=-0.5), dict(cmin=-1.0), dict(cmin=float("nan"))):
        assert cons(**kw) < 0 and b"finite" in lib.rgbm_last_error(), kw

    def pack(f1=p, k1=p, K1=p, E1=p, f2=None, k2=None, K2=None, E2=None, n=1, s=8, cap=4, cloud=p, index=p, count=p):
        return lib.rgbm_cloud_pack(f1, k1, K1, E1, f2, k2, K2, E2, n, s, cap, cloud, index, count, None)
    for kw in (dict(f1=None), dict(k1=None), dict(K1=None), dict(E1=None), dict(count=None)):
        assert pack(**kw) < 0 and b"cloud_pack arguments" in lib.rgbm_last_error(), kw
    for kw in (dict(f2=p), dict(f2=p, k2=p, K2=p), dict(E2=p)):
        assert pack(**kw) < 0 and b"together" in lib.rgbm_last_error(), kw
    for kw in (dict(n=0), dict(n=65536), dict(s=0), dict(s=4097)):
        assert pack(**kw) < 0 and b"65535" in lib.rgbm_last_error(), kw
    assert pack(cap=-1) < 0 and b"cap" in lib.rgbm_last_error()
    assert pack(cloud=None) < 0 and b"NULL" in lib.rgbm_last_error()
    assert pack(index=None) < 0 and b"NULL" in lib.rgbm_last_error()


def _smooth_depth(n):
    y, x = np.mgrid[0:S, 0:S]
    return np.stack([0.6 + 0.2 * np.sin(x / 31.0 + i) * np.cos(y / 47.0) for i in range(n)]).astype(np.float32)


def _exact_rig(n, size=S):
    """Cameras whose round trip is exact in binary floating point: E = identity and power-of-two focal lengths, so that
    ((x - cx) d / f) f / d is x itself and u, v land on the integers 0 .. S - 1, both borders included."""
    K = np.tile(np.array([[256.0, 0, size / 2], [0, 256.0, size / 2], [0, 0, 1.0]])[None], (n, 1, 1))
    return K, np.tile(np.eye(4)[None], (n, 1, 1))


def test_twin_identical_cameras_keep_every_pixel():
    """View b = view a.  On the exact rig every pixel comes back to itself and is kept, the border rows and columns included.  On the
    general cameras of synth.adapose_inputs the round trip is exact to rounding only, so a border pixel may land 1e-14 outside
    [0, S - 1] and go by rule 2, which has no tolerance: there every interior pixel is kept and the errors of every sampled pixel hold
    the same bounds."""
    d = _smooth_depth(2)
    K, E = _exact_rig(2)
    r = depth_consistency_ref(d, K, E, d, K, E)
    assert r["fused"].dtype == r["reproj"].dtype == r["rel"].dtype == np.float64 and r["keep"].dtype == bool
    assert r["keep"].all()
    assert r["reproj"].max() < 1e-9 and r["rel"].max() < 1e-12
    np.testing.assert_allclose(r["fused"], d, rtol=1e-12)
    inp = synth.adapose_inputs(2, seed=0)
    r = depth_consistency_ref(d, inp["K1"], inp["E1"], d, inp["K1"], inp["E1"])
    assert r["keep"][:, 1:-1, 1:-1].all() and np.array_equal(r["keep"], r["sampled"])
    assert np.nanmax(r["reproj"]) < 1e-9 and np.nanmax(r["rel"]) < 1e-12


@pytest.mark.parametrize("B,seed", [(2, 0), (3, 5)])
def test_twin_sphere_scene(B, seed):
    """A sphere of radius 0.12 at (0, 0, 0.5) seen by both cameras: the maps are consistent wherever view b sees the point too, up to the
    bilinear sampling of a curved surface.  Lowest kept share measured in float64: 97.0 %; sampled counts 4 141 .. 21 876."""
    inp = synth.adapose_inputs(B, seed=seed)
    d1, d2 = synth.sphere_depth(inp["K1"], inp["E1"]), synth.sphere_depth(inp["K2"], inp["E2"])
    assert d1.dtype == np.float32 and np.isnan(d1).any() and (d1[np.isfinite(d1)] > 0).all()
    v1, v2 = (d1, inp["K1"], inp["E1"]), (d2, inp["K2"], inp["E2"])
    for a, b in ((v1, v2), (v2, v1)):
        r = depth_consistency_ref(*a, *b)
        for i in range(B):
            s, k = r["sampled"][i], r["keep"][i]
            share = k.sum() / s.sum()
            print(f"B={B} seed={seed} pose {i}: sampled {s.sum()} kept {share:.4f}")
            assert s.sum() >= 4000 and share >= 0.95
            assert not (k & ~s).any() and np.array_equal(np.isfinite(r["fused"][i]), k) and np.array_equal(np.isfinite(r["reproj"][i]), s)
            assert np.abs(r["fused"][i][k] / a[0][i][k].astype(np.float64) - 1).max() < 0.01


def test_twin_depth_patch_changes_exactly_the_pixels_that_tap_it():
    """A 20 x 20 patch of depth_b times 1.05, default thresholds.  The scene is chosen so that the statement is exact: a fronto-parallel
    plane at depth 0.5 seen by the exact rig and by the same camera with its principal point moved by half a pixel both ways.  Every
    view-a pixel then samples view b at (x + 0.5, y + 0.5), all four weights are 1/4, and the unchanged maps agree exactly (reproj = rel
    = 0).  A pixel with j >= 1 taps in the patch reads a depth 1.25 j % off, which is beyond rel_max = 1 %: every pixel that touches the
    patch changes and is dropped, every other pixel stays as it was.  (With general weights a pixel that touches the patch with a weight
    below 0.2 changes by less than 1 % and is rightly kept: the sphere variant below.)"""
    Ka, E = _exact_rig(1)
    Kb = Ka.copy()
    Kb[:, :2, 2] += 0.5
    d = np.full((1, S, S), 0.5, dtype=np.float32)
    base = depth_consistency_ref(d, Ka, E, d, Kb, E)
    assert base["keep"][0, :-1, :-1].all() and not base["keep"][0, -1].any() and not base["keep"][0, :, -1].any()      # u = S - 0.5: rule 2
    assert np.nanmax(base["reproj"]) == 0 and np.nanmax(base["rel"]) == 0
    dp = d.copy()
    dp[0, 100:120, 60:80] *= np.float32(1.05)
    got = depth_consistency_ref(d, Ka, E, dp, Kb, E)
    touches = np.zeros((S, S), dtype=bool)
    touches[99:120, 59:80] = True                           # taps (y, y + 1) x (x, x + 1)
    changed = ~((got["rel"][0] == base["rel"][0]) | (np.isnan(got["rel"][0]) & np.isnan(base["rel"][0])))
    assert np.array_equal(changed, touches)
    assert not got["keep"][0][changed].any()
    assert np.isclose(got["rel"][0][changed].min(), 0.0125, rtol=1e-6) and np.isclose(got["rel"][0][changed].max(), 0.05, rtol=1e-6)
    for k in ("fused", "reproj", "keep"):
        assert np.array_equal(got[k][0][~changed], base[k][0][~changed], equal_nan=True), k


def test_twin_depth_patch_on_the_sphere_scene():
    """The same on general cameras and a curved surface: exactly the pixels with a tap in the patch change; those whose four taps all lie
    in it read a depth 5 % off and go; nothing else moves."""
    inp = synth.adapose_inputs(2, seed=0)
    d1, d2 = synth.sphere_depth(inp["K1"], inp["E1"]), synth.sphere_depth(inp["K2"], inp["E2"])
    a, Kb, Eb = (d1, inp["K1"], inp["E1"]), inp["K2"], inp["E2"]
    base = depth_consistency_ref(*a, d2, Kb, Eb)
    # a 20 x 20 patch of view b where pose 0's sampled pixels land
    ys, xs = np.nonzero(np.isfinite(d2[0]))
    y0, x0 = int(np.median(ys)) - 10, int(np.median(xs)) - 10
    patch = np.zeros((S, S), dtype=bool)
    patch[y0:y0 + 20, x0:x0 + 20] = True
    assert np.isfinite(d2[0][patch]).all()
    d2p = d2.copy()
    d2p[0][patch] *= np.float32(1.05)
    got = depth_consistency_ref(*a, d2p, Kb, Eb)
    # which view-a pixels of pose 0 have a tap in the patch: the taps of rule 3, restated
    d = d1[0].astype(np.float64)
    yy, xx = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64), indexing="ij")
    Ka, Ea = inp["K1"][0], inp["E1"][0]
    with np.errstate(invalid="ignore"):
        cam = np.stack([(xx - Ka[0, 2]) * d / Ka[0, 0], (yy - Ka[1, 2]) * d / Ka[1, 1], d], axis=-1)
        X = (cam - Ea[:3, 3]) @ Ea[:3, :3]                      # inv of a rigid transform: R^T (cam - t)
        c = X @ Eb[0][:3, :3].T + Eb[0][:3, 3]
        u, v = Kb[0][0, 0] * c[..., 0] / c[..., 2] + Kb[0][0, 2], Kb[0][1, 1] * c[..., 1] / c[..., 2] + Kb[0][1, 2]
    s = base["sampled"][0]
    ux, vy = np.floor(np.where(s, u, 0)).astype(int), np.floor(np.where(s, v, 0)).astype(int)
    ux1, vy1 = np.minimum(ux + 1, S - 1), np.minimum(vy + 1, S - 1)
    touches = s & (patch[vy, ux] | patch[vy, ux1] | patch[vy1, ux] | patch[vy1, ux1])
    assert touches.sum() > 300
    changed = ~np.isclose(got["rel"][0], base["rel"][0], rtol=0, atol=1e-9, equal_nan=True)
    assert np.array_equal(changed, touches)
    assert np.array_equal(got["sampled"], base["sampled"])
    inside = s & patch[vy, ux] & patch[vy, ux1] & patch[vy1, ux] & patch[vy1, ux1]      # sampled depth 5 % off, base rel < 1 % where kept
    assert inside.sum() > 100 and not got["keep"][0][inside].any()
    for k in ("fused", "reproj", "rel", "keep"):              # every other pixel, and pose 1, is untouched
        assert np.array_equal(got[k][0][~changed], base[k][0][~changed], equal_nan=True), k
        assert np.array_equal(got[k][1], base[k][1], equal_nan=True), k


def test_twin_invalid_pixels_follow_rule_1():
    d = _smooth_depth(2)
    K, E = _exact_rig(2)
    bad = {(0, 3, 4): np.nan, (0, 9, 200): np.inf, (0, 100, 7): -np.inf, (0, 50, 50): 0.0, (0, 223, 223): -0.3}
    da = d.copy()
    for k, val in bad.items():
        da[k] = val
    r = depth_consistency_ref(da, K, E, d, K, E)
    for k in bad:
        assert not r["keep"][k] and np.isnan(r["fused"][k]) and np.isnan(r["reproj"][k]) and np.isnan(r["rel"][k]), k
    assert int((~r["keep"]).sum()) == len(bad) and int(np.isnan(r["reproj"]).sum()) == len(bad)
    # a bad tap in view b: every view-a pixel that reads it goes, no other
    db = d.copy()
    db[1, 10, 10] = np.nan
    r = depth_consistency_ref(d, K, E, db, K, E)
    gone = np.argwhere(~r["keep"])
    assert len(gone) >= 1 and (gone[:, 0] == 1).all() and (np.abs(gone[:, 1:] - 10) <= 1).all() and not r["keep"][1, 10, 10]
    # a singular extrinsic on either side: the whole pose goes, the other pose stays
    for side in (0, 1):
        Es = E.copy()
        Es[1, 2] = 0.0
        r = depth_consistency_ref(d, K, Es if side == 0 else E, d, K, Es if side == 1 else E)
        assert r["keep"][0].all() and not r["keep"][1].any()
        assert np.isnan(r["fused"][1]).all() and np.isnan(r["reproj"][1]).all() and np.isnan(r["rel"][1]).all()
