"""Hand-made inputs of the sample statistics (rgbmanip_amd/samples.py, csrc/sample_stats.hip), shared by the CPU test of the numpy twins
and the GPU test of the kernels against them."""
import numpy as np

SIGNS = np.array([[1, 1, 1], [1, 1, -1], [-1, 1, 1], [-1, 1, -1], [1, -1, 1], [1, -1, -1], [-1, -1, 1], [-1, -1, -1]], dtype=np.float64)
EDGE_CORNER = (2, 4, 1)          # far ends of the x, y, z edges that leave corner 0


def corners(size, R=np.eye(3), t=(0.0, 0.0, 0.0)):
    """get_3d_bbox(size) (lib/utils.py:49-56) rotated by R and shifted by t: [8, 3] float64."""
    return (SIGNS * np.asarray(size, dtype=np.float64) / 2) @ np.asarray(R, dtype=np.float64).T + np.asarray(t, dtype=np.float64)


def rot(axis, deg):
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def hand_boxes():
    """n = 3, S = 4: pose 0 with all four samples counted; pose 1 with a NaN corner in sample 2 and ok = 0 in sample 0 (count 2); pose 2
    with none counted (ok 0, 0, and an infinite / a NaN coordinate in the two others).  Returns (boxes [4,3,8,3], ok [4,3], counts)."""
    rng = np.random.default_rng(7)
    boxes = np.empty((4, 3, 8, 3))
    for s in range(4):
        for b in range(3):
            boxes[s, b] = corners([0.4 + 0.01 * s, 0.3 + 0.02 * b, 0.2 + 0.015 * s * b], rot(b, 5.0 * s - 6.0) @ rot((b + 1) % 3, 20.0 * b + s),
                                  rng.normal(size=3) * 0.02 + [0.5, -0.25 * b, 1.0 + b])
    ok = np.ones((4, 3), dtype=np.uint8)
    boxes[2, 1, 5, 1] = np.nan
    ok[0, 1] = 0
    ok[0, 2] = ok[1, 2] = 0
    boxes[2, 2, 0, 0] = np.inf
    boxes[3, 2, 7, 2] = np.nan
    return boxes, ok, np.array([4, 2, 0], dtype=np.int32)


THETA = 10.0


def rotated_boxes():
    """n = 3, S = 4: pose b is one box rotated by +THETA, -THETA, +THETA, -THETA degrees about box axis b: axis_spread_deg is THETA on the
    two other axes and 0 on axis b.  Returns (boxes [4,3,8,3], ok)."""
    boxes = np.empty((4, 3, 8, 3))
    for s in range(4):
        for b in range(3):
            boxes[s, b] = corners([0.5, 0.3, 0.2], rot(b, THETA if s % 2 == 0 else -THETA), [0.25, -0.5, 1.5])
    return boxes, np.ones((4, 3), dtype=np.uint8)


def single_boxes():
    """n = 2, S = 4, one counted sample per pose (sample 3 / sample 0): every spread is 0.  Returns (boxes, ok)."""
    boxes, _, _ = hand_boxes()
    boxes = np.ascontiguousarray(boxes[:, :2])
    boxes[2, 1, 5, 1] = 0.125
    ok = np.zeros((4, 2), dtype=np.uint8)
    ok[3, 0] = ok[0, 1] = 1
    return boxes, ok


def random_boxes(n=5, S=7, seed=0, extent=10.0):
    """Seeded boxes with coordinates up to `extent` metres: per pose a random box, per sample a small random rotation, shift and
    change of size; from S = 7, n = 5 on a few samples not ok or not finite.  Returns (boxes [S,n,8,3], ok [S,n])."""
    rng = np.random.default_rng(seed)
    boxes = np.empty((S, n, 8, 3))
    for b in range(n):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        R0 = q * np.sign(np.linalg.det(q))
        size, t = rng.uniform(0.1, 2.0, size=3), rng.uniform(-0.7 * extent, 0.7 * extent, size=3)
        for s in range(S):
            Rs = rot(0, rng.normal() * 8) @ rot(1, rng.normal() * 8) @ rot(2, rng.normal() * 8)
            boxes[s, b] = corners(size * (1 + 0.05 * rng.normal(size=3)), Rs @ R0, t + 0.05 * rng.normal(size=3))
    assert np.abs(boxes).max() <= extent
    ok = np.ones((S, n), dtype=np.uint8)
    if S >= 7 and n >= 5:
        ok[1, 0] = ok[4, 3] = ok[6, 3] = 0
        boxes[2, 1, 3, 0] = np.nan
        boxes[5, 4, 6, 2] = -np.inf
    return boxes, ok


def numpy_box_stats(box, ok):
    """One pose [S,8,3] with numpy's own reductions (np.mean / np.std / np.cov, another summation order than the twin's loops) ->
    (count, bbox_mean, bbox_std, center_mean, center_cov, extent_mean, extent_std)."""
    keep = (np.asarray(ok) != 0) & np.isfinite(box.reshape(len(box), -1)).all(axis=1)
    x = box[keep]
    ctr = x.mean(axis=1)
    ext = np.stack([np.linalg.norm(x[:, c] - x[:, 0], axis=1) for c in EDGE_CORNER], axis=1)
    return int(keep.sum()), x.mean(axis=0), x.std(axis=0), ctr.mean(axis=0), np.cov(ctr.T, bias=True), ext.mean(axis=0), ext.std(axis=0)
