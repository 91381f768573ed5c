#!/usr/bin/env python3
"""Writes tests/golden/box_overlap.npz: seeded random pairs of oriented boxes with the intersection volume that scipy gives for them
(scipy.spatial.HalfspaceIntersection of the 12 half-spaces, then the volume of the ConvexHull of its vertices).  Run once by hand;
scipy is needed here and nowhere else: the tests read the file (tests/test_boxes_host.py, tests/test_gpu_boxes.py).

Boxes: edge lengths 0.05 .. 1 m, random rotations, centres 0 .. 12 m from the origin, the second box offset by up to a box size; every
fourth pair is a box against a slightly turned, shifted and resized copy of itself (high IoU).  The half-spaces are derived here with
numpy's own cross / norm in coordinates relative to the first box's centre, independently of rgbmanip_amd/boxes.py.
"""
import os
import sys

import numpy as np
from scipy.optimize import linprog
from scipy.spatial import ConvexHull, HalfspaceIntersection

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIGNS = np.array([[1, 1, 1], [1, 1, -1], [-1, 1, 1], [-1, 1, -1], [1, -1, 1], [1, -1, -1], [-1, -1, 1], [-1, -1, -1]], dtype=np.float64)
N_PAIRS, SEED = 240, 20240


def corners(size, R, t):
    return (SIGNS * size / 2) @ R.T + t


def rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def small_rotation(rng, deg):
    w = rng.normal(size=3)
    w = w / np.linalg.norm(w) * np.deg2rad(deg)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    th = np.linalg.norm(w)
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K


def halfspaces(c):
    """[8,3] corners -> [6,4] rows (n, -d) of n . x - d <= 0 with unit outward normals."""
    o, e = c[0], [c[2] - c[0], c[4] - c[0], c[1] - c[0]]
    inside = o + (e[0] + e[1] + e[2]) / 2
    rows = []
    for ax in range(3):
        n = np.cross(e[(ax + 1) % 3], e[(ax + 2) % 3])
        n = n / np.linalg.norm(n)
        for p in (o, o + e[ax]):
            s = 1.0 if n @ (p - inside) > 0 else -1.0
            rows.append(np.append(s * n, -s * (n @ p)))
    return np.array(rows)


def intersection_volume(a, b):
    ctr = a.mean(axis=0)
    hs = np.vstack([halfspaces(a - ctr), halfspaces(b - ctr)])
    # Chebyshev centre: the point deepest inside all half-spaces; no interior, no volume
    res = linprog([0, 0, 0, -1], A_ub=np.hstack([hs[:, :3], np.ones((12, 1))]), b_ub=-hs[:, 3], bounds=[(None, None)] * 3 + [(0, None)],
                  method="highs")
    if res.status != 0 or res.x[3] <= 1e-9:
        return 0.0
    pts = HalfspaceIntersection(hs, res.x[:3]).intersections
    return float(ConvexHull(pts).volume)


def main():
    rng = np.random.default_rng(SEED)
    a, b, inter = np.empty((N_PAIRS, 8, 3)), np.empty((N_PAIRS, 8, 3)), np.empty(N_PAIRS)
    for i in range(N_PAIRS):
        size, R = rng.uniform(0.05, 1.0, size=3), rotation(rng)
        d = rng.normal(size=3)
        t = d / np.linalg.norm(d) * rng.uniform(0.0, 12.0)
        a[i] = corners(size, R, t)
        if i % 4 == 0:
            b[i] = corners(size * rng.uniform(0.9, 1.1, size=3), small_rotation(rng, rng.uniform(1.0, 8.0)) @ R, t + size * rng.uniform(-0.08, 0.08, size=3))
        else:
            size_b = rng.uniform(0.05, 1.0, size=3)
            b[i] = corners(size_b, rotation(rng), t + rng.uniform(-0.5, 0.5, size=3) * np.maximum(size, size_b))
        inter[i] = intersection_volume(a[i], b[i])
    vol = lambda c: abs(np.linalg.det(np.stack([c[:, 2] - c[:, 0], c[:, 4] - c[:, 0], c[:, 1] - c[:, 0]], axis=1)))      # noqa: E731
    va, vb = vol(a), vol(b)
    iou = inter / (va + vb - inter)
    print(f"{N_PAIRS} pairs: {(iou > 1e-3).sum()} with IoU > 1e-3, {(iou > 0.5).sum()} with IoU > 0.5, largest coordinate {np.abs(a).max():.2f} m")
    assert N_PAIRS >= 200 and (iou > 1e-3).sum() * 2 >= N_PAIRS and (iou > 0.5).sum() >= 20
    assert (inter <= np.minimum(va, vb) * (1 + 1e-12)).all()
    out = os.path.join(ROOT, "tests", "golden", "box_overlap.npz")
    np.savez_compressed(out, a=a, b=b, inter_volume=inter)
    print(f"wrote {out}: {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
