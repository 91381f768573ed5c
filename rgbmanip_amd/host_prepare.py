"""The reference's per-frame input preparation in numpy (`interface_v5.py:58-170`): crop window, nearest / linear resize, the
1024-pixel subset, the crop's intrinsics.  Pure host arithmetic: no estimator state, no device."""
from __future__ import annotations

import numpy as np
import torch

_MEAN = np.array([0.485, 0.456, 0.406])
_STD = np.array([0.229, 0.224, 0.225])


def get_bbox(bbox):
    """Square crop window: side = multiple of 40 (<= 440), clamped into the 480x640 frame (lib/utils.py:10-38)."""
    y1, x1, y2, x2 = bbox
    win = min((max(y2 - y1, x2 - x1) // 40 + 1) * 40, 440)
    half = int(win / 2)
    cy, cx = (y1 + y2) // 2, (x1 + x2) // 2
    rmin, rmax, cmin, cmax = cy - half, cy + half, cx - half, cx + half
    if rmin < 0:
        rmin, rmax = 0, rmax - rmin
    if cmin < 0:
        cmin, cmax = 0, cmax - cmin
    if rmax > 480:
        rmin, rmax = rmin - (rmax - 480), 480
    if cmax > 640:
        cmin, cmax = cmin - (cmax - 640), 640
    return rmin, rmax, cmin, cmax


def _resize_nearest(img, size):
    h, w = img.shape[:2]
    ys = np.minimum((np.arange(size) * (h / size)).astype(np.int64), h - 1)
    xs = np.minimum((np.arange(size) * (w / size)).astype(np.int64), w - 1)
    return img[ys][:, xs]


def _resize_linear(img, size):
    """OpenCV INTER_LINEAR arithmetic for float images (half-pixel centres, edge clamp, no antialias)."""
    h, w = img.shape[:2]

    def taps(n_src):
        f = (np.arange(size) + 0.5) * (n_src / size) - 0.5
        i0 = np.floor(f).astype(np.int64)
        a = (f - i0).astype(np.float32)
        a = np.where(i0 < 0, 0.0, a)
        i0 = np.maximum(i0, 0)
        a = np.where(i0 >= n_src - 1, 0.0, a).astype(np.float32)
        i0 = np.minimum(i0, n_src - 1)
        return i0, np.minimum(i0 + 1, n_src - 1), a
    y0, y1, ay = taps(h)
    x0, x1, ax = taps(w)
    img = img.astype(np.float32)
    ax = ax[None, :, None]
    ay = ay[:, None, None]
    top = img[y0][:, x0] * (1 - ax) + img[y0][:, x1] * ax
    bot = img[y1][:, x0] * (1 - ax) + img[y1][:, x1] * ax
    return top * (1 - ay) + bot * ay


def _mix32(seed, frame, idx):
    """Seeded subset hash of csrc/prepare.hip (murmur3 finaliser), uint32 arithmetic."""
    with np.errstate(over="ignore"):
        h = np.uint32(seed) ^ (np.uint32(frame) * np.uint32(0x9E3779B9)) ^ (np.asarray(idx, dtype=np.uint32) * np.uint32(0x85EBCA6B))
        h = h ^ (h >> np.uint32(16)); h = h * np.uint32(0x85EBCA6B)
        h = h ^ (h >> np.uint32(13)); h = h * np.uint32(0xC2B2AE35)
        h = h ^ (h >> np.uint32(16))
    return h.astype(np.uint32)


def _subset(choose, rng, frame):
    """1024 of more than 1024 mask pixels.  `rng` is a numpy generator or the global `np.random` (the reference shuffles a keep
    vector, interface_v5.py:126-130), or ("hash", seed): the device path's reproducible subset of frame `frame`, on the host."""
    if isinstance(rng, tuple):
        keys = _mix32(rng[1], frame, choose).astype(np.uint64)
        return choose[np.sort(np.lexsort((np.arange(len(choose)), keys))[:1024])]
    keep = np.zeros(len(choose), dtype=int)
    keep[:1024] = 1
    rng.shuffle(keep)
    return choose[keep.nonzero()]


def prepare_model_input(rgb, mask, intrinsic, resize_size, rng, frame=0, normalize=True):
    """(view [3,S,S] tensor, choose [1024], pts2d [1024,2], K of the crop), or four Nones for an empty mask.  `normalize=False`: the
    view is the resized crop itself (plain `ToTensor`, `interface_v4.py:56-57`) instead of the ImageNet-normalised one."""
    rgb = np.asarray(rgb)
    if rgb.dtype == np.uint8:           # transforms.ToTensor scales uint8 images to [0, 1] (interface_v5.py:52-54,149); floats pass as they are
        rgb = rgb.astype(np.float32) / np.float32(255.0)
    elif rgb.dtype.kind != "f":
        raise TypeError(f"prepare_model_input: rgb must be a float image in [0, 1] or uint8, got {rgb.dtype}")
    ys, xs = np.nonzero(mask)
    if len(ys) == 0:
        return None, None, None, None
    rmin, rmax, cmin, cmax = get_bbox([int(ys.min()), int(xs.min()), int(ys.max()), int(xs.max())])
    small = _resize_nearest(mask[rmin:rmax, cmin:cmax].astype(np.float32), resize_size)
    choose = small.flatten().nonzero()[0]
    if len(choose) > 1024:
        choose = _subset(choose, rng, frame)
    elif len(choose) == 0:
        return None, None, None, None
    else:
        choose = np.pad(choose, (0, 1024 - len(choose)), "wrap")
    ratio = resize_size / (rmax - rmin)
    pts2d = np.stack(((choose % resize_size).astype(np.float32) / ratio + cmin,
                      (choose // resize_size).astype(np.float32) / ratio + rmin), axis=-1)
    crop = _resize_linear(rgb[rmin:rmax, cmin:cmax, :], resize_size).astype(rgb.dtype)
    view = np.transpose(crop, (2, 0, 1))
    if normalize:
        view = (view - _MEAN.astype(rgb.dtype)[:, None, None]) / _STD.astype(rgb.dtype)[:, None, None]
    K = np.eye(3)
    K[0, 0], K[1, 1] = intrinsic[0, 0] * ratio, intrinsic[1, 1] * ratio
    K[0, 2] = (intrinsic[0, 2] - (float(cmin + cmax) / 2 - float(cmax - cmin + 1) / 2)) * ratio
    K[1, 2] = (intrinsic[1, 2] - (float(rmin + rmax) / 2 - float(rmax - rmin + 1) / 2)) * ratio
    return torch.from_numpy(np.ascontiguousarray(view)), choose, pts2d, K
