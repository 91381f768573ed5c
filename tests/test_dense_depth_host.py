"""CPU-only checks of the dense depth entry points (DESIGN.md "Dense depth maps"): the C ABI declares, binds and exports them, their
argument errors come back as negative codes with text, and the float64 twin of `depth_to_points` is the reference's back-projection."""
import ctypes as C
import os
import re

import numpy as np

from rgbmanip_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rgbm_adapose_dense_workspace_bytes", "rgbm_adapose_forward_dense", "rgbm_depth_to_points")


def test_library_exports_the_dense_depth_entry_points():
    src = open(os.path.join(ROOT, "include", "rgbm.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(rgbm_[a-z0-9_]+)\s*\(", src))
    lib = _lib.load()
    for n in NEW_SYMBOLS:
        assert n in declared, f"{n} is not declared in include/rgbm.h"
        assert n in _lib.SIGNATURES, f"{n} is not bound in _lib.SIGNATURES"
        assert getattr(lib, n) is not None


def test_argument_errors_are_negative_codes_with_text():
    """Plain ctypes on the built library, no device: a NULL depth_map is named before anything else is looked at, a NULL handle and
    NULL buffers are argument errors.  (The workspace-size error needs a handle, i.e. a device: tests/test_gpu_dense_depth.py.)"""
    lib = _lib.load()
    n = C.c_size_t(0)
    buf = (C.c_float * 4)()
    p = C.cast(buf, C.c_void_p)
    assert lib.rgbm_adapose_forward_dense(None, 1, p, p, p, p, p, p, p, p, 1024, None, None, p, None) < 0
    assert b"depth_map" in lib.rgbm_last_error()
    assert lib.rgbm_adapose_forward_dense(None, 1, p, p, p, p, p, p, p, p, 1024, None, p, None, None) < 0
    assert b"forward_dense arguments" in lib.rgbm_last_error()
    assert lib.rgbm_adapose_dense_workspace_bytes(None, 1, C.byref(n)) < 0 and b"dense_workspace_bytes" in lib.rgbm_last_error()
    assert lib.rgbm_depth_to_points(None, p, p, 1, 224, p, None) < 0 and b"depth_to_points" in lib.rgbm_last_error()
    assert lib.rgbm_depth_to_points(p, p, p, 0, 224, p, None) < 0 and b"depth_to_points" in lib.rgbm_last_error()
    assert lib.rgbm_depth_to_points(p, p, p, 65536, 224, p, None) < 0 and b"65535" in lib.rgbm_last_error()


def test_depth_to_points_twin_is_the_reference_back_projection():
    """The numpy twin at the chosen pixels against the statements of interface_v5.py:323-336 (xmap / ymap gathered at `choose`, pt0 / pt1 /
    pt2) followed by ex_inv of :369-372."""
    from rgbmanip_amd.adapose import depth_to_points_ref
    inp = synth.adapose_inputs(2, seed=0)
    S = 224
    g = np.random.default_rng(5)
    depth = g.uniform(0.1, 2.4, (2, S, S)).astype(np.float32)
    pts = depth_to_points_ref(depth, inp["K1"], inp["E1"])
    assert pts.shape == (2, S, S, 3) and pts.dtype == np.float64
    xmap = np.array([[i for i in range(S)] for j in range(S)])
    ymap = np.array([[j for i in range(S)] for j in range(S)])
    for b in range(2):
        choose = inp["choose1"][b]
        K = inp["K1"][b]
        pt2 = depth[b].flatten()[choose][:, np.newaxis].astype(np.float64)
        pt0 = (xmap.flatten()[choose][:, np.newaxis] - K[0, 2]) * pt2 / K[0, 0]
        pt1 = (ymap.flatten()[choose][:, np.newaxis] - K[1, 2]) * pt2 / K[1, 1]
        cam = np.concatenate((pt0, pt1, pt2), axis=1)
        ex_inv = np.linalg.inv(inp["E1"][b])
        world = (ex_inv[:3, :3] @ cam.T + ex_inv[:3, 3:4]).T
        np.testing.assert_allclose(pts[b].reshape(-1, 3)[choose], world, rtol=1e-12, atol=1e-12)
    depth[0, 3, 4] = np.nan
    assert np.isnan(depth_to_points_ref(depth, inp["K1"], inp["E1"])[0, 3, 4]).all()
