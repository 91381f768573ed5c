"""Statistics over S Dropout2d samples per pose: the device kernels of csrc/sample_stats.hip (`box_stats`, `point_stats`; C ABI
rgbm_sample_box_stats / rgbm_sample_point_stats in include/rgbm.h) and their float64 numpy twins (`box_stats_ref`, `point_stats_ref`),
which sum in the kernels' order.  `AdaPoseEstimator_v5.estimate_samples` feeds them the boxes, the NOCS rows and the depths that one
`AdaPoseNet.forward_samples` gives for every pose.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib

MAX_SAMPLES = 64                  # kSampleMax (csrc/sample_stats.h)
MAX_BOX_POSES = 65535
BOX_KEYS = ("count", "bbox_mean", "bbox_std", "center_mean", "center_cov", "extent_mean", "extent_std", "axis_spread_deg")
_EDGE_CORNER = (2, 4, 1)          # the corners at the far end of the x, y, z edges that leave corner 0 (get_3d_bbox, lib/utils.py:49-56)
_BOX_SHAPES = {"bbox_mean": (8, 3), "bbox_std": (8, 3), "center_mean": (3,), "center_cov": (3, 3), "extent_mean": (3,), "extent_std": (3,),
               "axis_spread_deg": (3,)}


def box_stats(boxes, ok, stream=None) -> dict:
    """boxes [S, n, 8, 3] (read as float64), ok [S, n] (non-zero: the sample may count) -> dict of CUDA tensors over the counted samples
    of every pose (ok set and 24 finite coordinates), ascending s, float64, two passes: `count` [n] i32, `bbox_mean` / `bbox_std`
    [n,8,3], `center_mean` [n,3], `center_cov` [n,3,3], `extent_mean` / `extent_std` [n,3] (edges x, y, z of the box frame),
    `axis_spread_deg` [n,3].  count 0: NaN everywhere; count 1: zero spreads.  1 <= S <= 64, 1 <= n <= 65535."""
    lib = _lib.load()
    boxes = torch.as_tensor(boxes)
    dev = boxes.device if boxes.is_cuda else torch.device("cuda", torch.cuda.current_device())
    boxes = boxes.to(device=dev, dtype=torch.float64).contiguous()
    if boxes.dim() != 4 or tuple(boxes.shape[2:]) != (8, 3):
        raise ValueError(f"box_stats: boxes [S, n, 8, 3], got {tuple(boxes.shape)}")
    S, n = int(boxes.shape[0]), int(boxes.shape[1])
    if not 1 <= S <= MAX_SAMPLES or not 1 <= n <= MAX_BOX_POSES:
        raise ValueError(f"box_stats: 1 <= S <= {MAX_SAMPLES} samples of 1 <= n <= {MAX_BOX_POSES} poses, got S = {S}, n = {n}")
    ok = torch.as_tensor(ok).to(device=dev)
    ok = (ok if ok.dtype == torch.uint8 else (ok != 0).to(torch.uint8)).contiguous()
    if tuple(ok.shape) != (S, n):
        raise ValueError(f"box_stats: ok [S, n] = {(S, n)}, got {tuple(ok.shape)}")
    out = {"count": torch.empty(n, dtype=torch.int32, device=dev)}
    out.update({k: torch.empty(n, *shp, dtype=torch.float64, device=dev) for k, shp in _BOX_SHAPES.items()})
    if stream is not None:
        for t in (boxes, ok, *out.values()):
            t.record_stream(stream)
    _lib.check(lib.rgbm_sample_box_stats(_lib.ptr(boxes), _lib.ptr(ok), n, S, *[_lib.ptr(out[k]) for k in BOX_KEYS], _lib.stream_ptr(stream)),
               "rgbm_sample_box_stats")
    return out


def point_stats(x, stream=None):
    """x [S, n, ...] (read as float32) -> (mean, std) [n, ...] float32 CUDA: per element over s ascending, accumulated in float64 in two
    passes (population std), rounded once; NaN propagates."""
    lib = _lib.load()
    x = torch.as_tensor(x)
    dev = x.device if x.is_cuda else torch.device("cuda", torch.cuda.current_device())
    x = x.to(device=dev, dtype=torch.float32).contiguous()
    if x.dim() < 2 or x.numel() == 0:
        raise ValueError(f"point_stats: x [S, n, ...] with at least one element, got {tuple(x.shape)}")
    S, n = int(x.shape[0]), int(x.shape[1])
    M = x[0, 0].numel()
    mean = torch.empty(x.shape[1:], dtype=torch.float32, device=dev)
    std = torch.empty_like(mean)
    if stream is not None:
        for t in (x, mean, std):
            t.record_stream(stream)
    _lib.check(lib.rgbm_sample_point_stats(_lib.ptr(x), n, S, M, _lib.ptr(mean), _lib.ptr(std), _lib.stream_ptr(stream)),
               "rgbm_sample_point_stats")
    return mean, std


# ------------------------------------------------------------------------------------------------------------------ float64 numpy twins
def _box_stats_pose(box, ok):
    """One pose: box [S, 8, 3] float64, ok [S] -> the statistics, summed sample by sample in ascending s like the kernel's lanes."""
    S = box.shape[0]
    flat = box.reshape(S, 24)
    idx = [s for s in range(S) if ok[s] and np.all(np.isfinite(flat[s]))]
    cnt = len(idx)
    out = {"count": np.int32(cnt)}
    if cnt == 0:
        out.update({k: np.full(shp, np.nan) for k, shp in _BOX_SHAPES.items()})
        return out
    dc = np.float64(cnt)

    def mean_of(v):                                   # v [S, ...]: sequential sum over the counted samples / count
        a = np.zeros(v.shape[1:])
        for s in idx:
            a = a + v[s]
        return a / dc

    def dev2(v, mv, w, mw):
        a = np.zeros(v.shape[1:])
        for s in idx:
            a = a + (v[s] - mv) * (w[s] - mw)
        return a
    with np.errstate(invalid="ignore", divide="ignore"):
        ctr = np.zeros((S, 3))
        for k in range(8):
            ctr = ctr + box[:, k, :]
        ctr = ctr / 8.0
        edge = np.stack([box[:, c, :] - box[:, 0, :] for c in _EDGE_CORNER], axis=1)              # [S, 3 edges, xyz]
        length = np.sqrt(edge[..., 0] * edge[..., 0] + edge[..., 1] * edge[..., 1] + edge[..., 2] * edge[..., 2])
        unit = edge / length[..., None]
        m = mean_of(flat)
        out["bbox_mean"] = m.reshape(8, 3)
        out["bbox_std"] = np.sqrt(dev2(flat, m, flat, m) / dc).reshape(8, 3)
        cm = mean_of(ctr)
        out["center_mean"] = cm
        out["center_cov"] = np.array([[dev2(ctr[:, i], cm[i], ctr[:, j], cm[j]) / dc for j in range(3)] for i in range(3)])
        em = mean_of(length)
        out["extent_mean"] = em
        out["extent_std"] = np.sqrt(dev2(length, em, length, em) / dc)
        spread = np.empty(3)
        for e in range(3):
            u = unit[:, e, :]
            msum = np.zeros(3)
            for s in idx:
                msum = msum + u[s]
            if cnt == 1:                              # one direction has no spread (0, or NaN for an edge of no length)
                spread[e] = 0.0 * ((msum[0] + msum[1]) + msum[2])
                continue
            d = msum / np.sqrt(msum[0] * msum[0] + msum[1] * msum[1] + msum[2] * msum[2])
            a = 0.0
            for s in idx:
                c = u[s, 0] * d[0] + u[s, 1] * d[1] + u[s, 2] * d[2]
                c = 1.0 if c > 1.0 else -1.0 if c < -1.0 else c
                ang = math.acos(c) if c == c else float("nan")
                a = a + ang * ang
            spread[e] = np.sqrt(a / dc) * (180.0 / math.pi)
        out["axis_spread_deg"] = spread
    return out


def box_stats_ref(boxes, ok) -> dict:
    """float64 numpy twin of `box_stats`: boxes [S, n, 8, 3], ok [S, n] -> the same dict as numpy arrays."""
    boxes = np.asarray(boxes, dtype=np.float64)
    ok = np.asarray(ok) != 0
    if boxes.ndim != 4 or boxes.shape[2:] != (8, 3) or ok.shape != boxes.shape[:2]:
        raise ValueError(f"box_stats_ref: boxes [S, n, 8, 3] and ok [S, n], got {boxes.shape} and {ok.shape}")
    S, n = boxes.shape[:2]
    if not 1 <= S <= MAX_SAMPLES or not 1 <= n <= MAX_BOX_POSES:
        raise ValueError(f"box_stats_ref: 1 <= S <= {MAX_SAMPLES} samples of 1 <= n <= {MAX_BOX_POSES} poses, got S = {S}, n = {n}")
    rows = [_box_stats_pose(boxes[:, b], ok[:, b]) for b in range(n)]
    return {k: np.stack([r[k] for r in rows]) for k in BOX_KEYS}


def point_stats_ref(x):
    """float64 numpy twin of `point_stats`: x [S, n, ...] -> (mean, std) [n, ...] float32 (float64 sums over s ascending, one rounding)."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    S = x.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.zeros(x.shape[1:])
        for s in range(S):
            a = a + x[s]
        m = a / np.float64(S)
        q = np.zeros(x.shape[1:])
        for s in range(S):
            d = x[s] - m
            q = q + d * d
        return m.astype(np.float32), np.sqrt(q / np.float64(S)).astype(np.float32)
