"""Hand-made box pairs with known answers for the box agreement (rgbmanip_amd/boxes.py, csrc/box_overlap.hip), shared by the CPU test
of the numpy twins and the GPU test of the kernels against them."""
import os

import numpy as np

from samples_cases import corners, rot

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "box_overlap.npz")
MIRROR = [1, 0, 3, 2, 5, 4, 7, 6]        # corner order of a box mirrored in its z axis: det[ex ey ez] < 0
THETA = 25.0
T0 = np.array([3.0, -4.0, 5.0])          # the hand cases sit metres from the origin; the offsets below are exact in binary
UNIT = [1.0, 1.0, 1.0]


def iou_cases():
    """name -> (a [8,3], b [8,3], IoU, intersection volume): the analytic values."""
    cube = corners(UNIT, t=T0)
    small = [0.5, 0.5, 0.5]
    c = {
        "identical": (cube, cube.copy(), 1.0, 1.0),
        "half shift on three axes": (cube, corners(UNIT, t=T0 + 0.5), 1.0 / 15.0, 0.125),
        "shift along one edge": (cube, corners(UNIT, t=T0 + [0.5, 0, 0]), 1.0 / 3.0, 0.5),                      # four shared planes
        "face touch": (cube, corners(UNIT, t=T0 + [1.0, 0, 0]), 0.0, 0.0),
        "edge touch": (cube, corners(UNIT, t=T0 + [1.0, 1.0, 0]), 0.0, 0.0),
        "corner touch": (cube, corners(UNIT, t=T0 + [1.0, 1.0, 1.0]), 0.0, 0.0),
        "nested": (cube, corners(small, t=T0), 0.125, 0.125),
        "nested with a shared face": (cube, corners(small, t=T0 + [0.25, 0, 0]), 0.125, 0.125),
        "45 degree turn": (cube, corners(UNIT, rot(2, 45.0), T0), (2 * (np.sqrt(2) - 1)) / (2 - 2 * (np.sqrt(2) - 1)), 2 * (np.sqrt(2) - 1)),
        "mirrored corner order": (cube[MIRROR], corners(UNIT, t=T0 + [0.5, 0, 0]), 1.0 / 3.0, 0.5),
        "mirrored against itself": (cube[MIRROR], cube, 1.0, 1.0),
        "far apart": (cube, corners(UNIT, t=T0 + [5.0, 0, 0]), 0.0, 0.0),
        "half turn": (corners([0.5, 0.25, 0.125], t=T0), corners([0.5, 0.25, 0.125], rot(0, 180.0), T0), 1.0, 0.5 * 0.25 * 0.125),
    }
    return c


def stacked(cases):
    a = np.stack([v[0] for v in cases.values()])
    b = np.stack([v[1] for v in cases.values()])
    return a, b, np.array([v[2] for v in cases.values()]), np.array([v[3] for v in cases.values()])


def unusable_cases():
    """(a [4,8,3], b, ok_a [4], ok_b [4], valid [4]): a box of no volume, a NaN corner, ok = 0, and one good pair."""
    cube = corners(UNIT, t=T0)
    a, b = np.stack([cube] * 4), np.stack([corners(UNIT, t=T0 + [0.5, 0, 0])] * 4)
    a[0] = corners([1.0, 0.0, 1.0], t=T0)
    b[1, 6, 1] = np.nan
    ok_a, ok_b = np.ones(4, dtype=np.uint8), np.array([1, 1, 0, 1], dtype=np.uint8)
    return a, b, ok_a, ok_b, np.array([0, 0, 0, 1], dtype=np.int32)


def rotation_cases():
    """Pair e: a box against itself turned by THETA degrees about its own axis e: axis_angle_deg is THETA on the two other axes and
    0 on axis e, rot_deg is THETA.  (a [3,8,3], b [3,8,3])"""
    size, R0 = [0.5, 0.3, 0.2], rot(2, 30.0) @ rot(0, -20.0)
    a = np.stack([corners(size, R0, T0)] * 3)
    b = np.stack([corners(size, R0 @ rot(e, THETA), T0 + [0.01, 0.02, -0.03]) for e in range(3)])
    return a, b


def shift_cases():
    """Unit cubes shifted by s along a face normal: IoU (1 - s) / (1 + s).  With tau = 1e-12 and L = sqrt(3) the planes count as
    coincident up to s = 1.7e-12, where the answer is 1 instead: off by 2 s.  The shifts are those for which that is below 1e-12, and
    those beyond the rule's reach.  Boxes at the origin: T0 + s would round s away.  (a, b, iou)"""
    s = np.array([1e-17, 1e-15, 1e-13, 1e-11, 1e-9, 1e-6, 1e-3])
    a = np.stack([corners(UNIT)] * len(s))
    b = np.stack([corners(UNIT, t=[x, 0, 0]) for x in s])
    return a, b, (1 - s) / (1 + s)


def golden():
    g = np.load(GOLDEN)
    return g["a"], g["b"], g["inter_volume"]


def random_pairs(n, seed, extent=10.0):
    """n seeded pairs in general position (no planes near coincidence), a few of them unusable.  (a, b, ok_a, ok_b)"""
    rng = np.random.default_rng(seed)
    a, b = np.empty((n, 8, 3)), np.empty((n, 8, 3))
    for i in range(n):
        size, t = rng.uniform(0.1, 1.0, size=3), rng.uniform(-0.6 * extent, 0.6 * extent, size=3)
        Ra = rot(0, rng.uniform(-180, 180)) @ rot(1, rng.uniform(-90, 90)) @ rot(2, rng.uniform(-180, 180))
        Rb = Ra @ rot(0, rng.normal() * 10) @ rot(1, rng.normal() * 10) @ rot(2, rng.normal() * 10)
        a[i] = corners(size, Ra, t)
        b[i] = corners(size * rng.uniform(0.7, 1.3, size=3), Rb, t + size * rng.uniform(-0.4, 0.4, size=3))
    ok_a, ok_b = np.ones(n, dtype=np.uint8), np.ones(n, dtype=np.uint8)
    if n >= 6:
        ok_a[1] = 0
        ok_b[n - 1] = 0
        b[3, 2, 0] = np.inf
        a[4] = a[4, 0]                      # every corner the same point: no volume
    return a, b, ok_a, ok_b


def random_sets(n, P, Q, seed):
    """Seeded [n,P,8,3] and [n,Q,8,3] boxes around one box per pose, some unusable.  (a, b, ok_a, ok_b)"""
    rng = np.random.default_rng(seed)
    a, b = np.empty((n, P, 8, 3)), np.empty((n, Q, 8, 3))
    for i in range(n):
        size, t = rng.uniform(0.2, 1.0, size=3), rng.uniform(-6.0, 6.0, size=3)
        R0 = rot(0, rng.uniform(-180, 180)) @ rot(1, rng.uniform(-90, 90)) @ rot(2, rng.uniform(-180, 180))
        for dst, m in ((a, P), (b, Q)):
            for j in range(m):
                Rj = R0 @ rot(0, rng.normal() * 8) @ rot(1, rng.normal() * 8) @ rot(2, rng.normal() * 8)
                dst[i, j] = corners(size * rng.uniform(0.8, 1.2, size=3), Rj, t + size * rng.uniform(-0.3, 0.3, size=3))
    ok_a, ok_b = np.ones((n, P), dtype=np.uint8), np.ones((n, Q), dtype=np.uint8)
    ok_a[0, P - 1] = 0
    b[n - 1, 0, 5, 2] = np.nan
    if Q > 1:
        ok_b[0, 1] = 0
    return a, b, ok_a, ok_b
