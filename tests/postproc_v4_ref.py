"""numpy restatement of the `direct_regression: True` tail of `AdaPoseEstimator_v4.predict` (interface_v4.py:322-325, 358-378 with
lib/utils.py:40-74), which rgbmanip_amd/csrc/postproc_regressed.hip runs on the device.  tests/test_postproc_v4_host.py pins it to
tests/golden/postproc_v4.npz (the reference's own numpy calls); the GPU tests compare the kernel against it at other shapes.

The reference's two float32 BLAS calls are written out as elementwise IEEE operations, so that the result does not depend on which
BLAS kernel a CPU selects:
  * `np.linalg.norm(s)` = sqrt(s.dot(s)): the float32 dot of a short vector rounds every product to float32 and adds the products in
    double; the sum is rounded to float32, the root is a float32 root.
  * `sRT @ [bbox; 1]` in float32: per element one chain of fused multiply-adds over k = 0..3 that starts from the rounded first product.
    A float32 fma is restated as the float64 product (exact: 24 + 24 bits) plus the addend, rounded to float32 — equal to the fused
    result unless the float64 sum lands exactly on a float32 rounding boundary (about one case in 2^29).
The float64 world transform is written with explicit three-term sums; `np.linalg.inv` stays LAPACK's."""
import numpy as np

DEFAULT_BBOX = np.asarray([[0, 0, 0], [0, 0, 1], [0, 1, 0], [0, 1, 1], [1, 0, 0], [1, 0, 1], [1, 1, 0], [1, 1, 1]], dtype=np.float64) + 10.0
BBOX_SIGNS = np.array([[+1, +1, +1], [+1, +1, -1], [-1, +1, +1], [-1, +1, -1], [+1, -1, +1], [+1, -1, -1], [-1, -1, +1], [-1, -1, -1]],
                      dtype=np.float32)


def _fma32(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def scale_of(s):
    """ts = np.linalg.norm(view1_s) on a float32 vector -> float32 scalar"""
    s = np.asarray(s, dtype=np.float32)
    q = (s * s).astype(np.float64)
    return np.sqrt(np.float32((q[0] + q[1]) + q[2]))


def camera_box(nocs, r, t, scale):
    """interface_v4.py:359-366: float32 [3,8] corners in the camera frame"""
    nocs, r, t = np.asarray(nocs, np.float32), np.asarray(r, np.float32), np.asarray(t, np.float32).reshape(3)
    half = np.max(np.abs(nocs), axis=0)                              # NaN propagates
    size = (np.float32(2) * half) * np.float32(scale)
    p = (BBOX_SIGNS * (size / np.float32(2))[None, :]).T            # [3,8]
    acc = r[:, 0:1] * p[0:1]                                         # the rounded first product
    acc = _fma32(r[:, 1:2], p[1:2], acc)
    acc = _fma32(r[:, 2:3], p[2:3], acc)
    acc = _fma32(t[:, None], np.float32(1), acc)
    # row 3 of sRT is (0, 0, 0, 1): the homogeneous coordinate is 1 for finite corners, NaN for the others
    w = _fma32(np.float32(1), np.float32(1), _fma32(np.float32(0), p[2:3], _fma32(np.float32(0), p[1:2], np.float32(0) * p[0:1])))
    return acc / w


def bbox_world(nocs, r, t, s, E1):
    """One pose -> ([8,3] float64 box, float32 scale, valid).  Singular E1: `np.linalg.inv` raises in the reference; here it is the
    default box, as for a non-finite inverse."""
    with np.errstate(all="ignore"):
        scale = scale_of(s)
        cam = camera_box(nocs, r, t, scale).astype(np.float64)
        try:
            inv = np.linalg.inv(np.asarray(E1, dtype=np.float64))
        except np.linalg.LinAlgError:
            return DEFAULT_BBOX.copy(), scale, 0
        if not (np.isfinite(inv).all() and np.isfinite(cam).all()):
            return DEFAULT_BBOX.copy(), scale, 0
        world = ((inv[:3, 0:1] * cam[0:1] + inv[:3, 1:2] * cam[1:2]) + inv[:3, 2:3] * cam[2:3]) + inv[:3, 3:4]
        return world.T.copy(), scale, 1


def bbox_world_batch(nocs, r, t, s, E1):
    out = [bbox_world(nocs[b], r[b], t[b], s[b], E1[b]) for b in range(len(nocs))]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.float32), np.array([o[2] for o in out], np.int32)
