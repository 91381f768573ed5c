"""Box verification without ground truth: how well a box agrees with the inputs it was computed from.  `box_silhouette` counts the
pixels of the silhouettes of S boxes against the V masks of a pose, `cloud_in_box` the rows of a packed handle cloud that S boxes
contain (csrc/box_verify.hip, C ABI rgbm_box_silhouette / rgbm_cloud_in_box in include/rgbm.h); `box_silhouette_ref` and
`cloud_in_box_ref` are their float64 numpy twins, which evaluate the same expressions in the same order, so that every integer output
is equal.  `select_by_mask` scores the boxes of a pose by their mean mask IoU and picks one; `samples_verify` and `cloud_pose_verify`
feed them the dicts that `estimate_samples` and `estimate_cloud_pose` return.

The box model is the one of boxes.py: [8, 3] corners read as o + a e0 + b e1 + c e2 with o = corner 0 and e0, e1, e2 = corner 2, 4, 1
- corner 0.  In a frame: n_k = e_{k+1} x e_{k+2}, det = e0 . n0, lo = min(0, det), hi = max(0, det); x is inside iff
lo <= n_k . (x - o) <= hi for k = 0, 1, 2.  Pixel (v, u) of a camera K, E (X_cam = E X_world) looks along (xn, yn, 1),
xn = (u - K02) / K00, yn = (v - K12) / K11, and is inside the silhouette iff that ray meets the box at t > 0 by the slab rule of the
synthetic camera (csrc/synth_env.hip): a box that contains the camera has an empty silhouette and flag 2.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .boxes import _check_ok, _device_of, _is_numpy, _ok_tensor, _to_numpy
from .cloud import DEFAULT_BBOX

MAX_BOXES = 64                    # kVerifyBoxesMax (csrc/box_verify.h)
MAX_VIEWS = 16                    # kVerifyViewsMax
MAX_RECORDS = 1 << 24             # kVerifyRecordsMax: n * S * V
MAX_COUNT_COLS = 16
MAX_CAP = 1 << 30
USABLE, CAMERA_INSIDE, BORDER, BEHIND = 1, 2, 4, 8          # bits of `flags`
INT_KEYS = ("area_box", "inter", "area_mask", "rect", "flags")
_EDGE_CORNER = (2, 4, 1)


def _silhouette_shapes(name, boxes, K, E, masks):
    """The shapes of the four arguments -> (n, S, V, H, W, K has a view axis); [n,8,3] boxes are S = 1, [n,H,W] masks with [n,4,4] E V = 1."""
    b, k, e, m = tuple(boxes), tuple(K), tuple(E), tuple(masks)
    if len(b) == 3:
        b = (b[0], 1) + b[1:]
    if len(b) != 4 or b[2:] != (8, 3):
        raise ValueError(f"{name}: boxes [n, S, 8, 3] or [n, 8, 3], got {tuple(boxes)}")
    n, S = int(b[0]), int(b[1])
    if len(m) == 3 and len(e) == 3:
        m, e = (m[0], 1) + m[1:], (e[0], 1) + e[1:]
    if len(m) != 4 or len(e) != 4 or e[2:] != (4, 4) or m[0] != n or e[:2] != m[:2]:
        raise ValueError(f"{name}: masks [n, V, H, W] with E [n, V, 4, 4], or [n, H, W] with E [n, 4, 4], got {tuple(masks)} and {tuple(E)}")
    V, H, W = int(m[1]), int(m[2]), int(m[3])
    if k not in ((n, 3, 3), (n, V, 3, 3)):
        raise ValueError(f"{name}: K [n, 3, 3] or [n, V, 3, 3], got {tuple(K)}")
    if not 1 <= S <= MAX_BOXES:
        raise ValueError(f"{name}: 1 <= S <= {MAX_BOXES} boxes per pose, got S = {S}")
    if not 1 <= V <= MAX_VIEWS:
        raise ValueError(f"{name}: 1 <= V <= {MAX_VIEWS} views per pose, got V = {V}")
    if n < 1 or n * S * V > MAX_RECORDS:
        raise ValueError(f"{name}: n >= 1 and n * S * V <= 2^24, got n = {n}, S = {S}, V = {V}")
    if H < 1 or W < 1 or H * W >= 2 ** 31:
        raise ValueError(f"{name}: H, W >= 1 and H * W < 2^31, got H = {H}, W = {W}")
    return n, S, V, H, W, len(k) == 4


def _mask_bytes(masks, dev):
    """masks as contiguous uint8 on dev; uint8 (and bool) masks are used where they lie, byte for byte."""
    m = torch.as_tensor(masks)
    if m.dtype == torch.bool:
        m = m.view(torch.uint8)
    elif m.dtype != torch.uint8:
        m = m.ne(0).view(torch.uint8)
    return m.to(device=dev).contiguous()


def _ratios(out, xp):
    """iou, coverage, precision and valid from the integer outputs: the documented expressions, NaN where the denominator is 0 or the
    box is unusable.  xp: numpy or torch."""
    f64 = np.float64 if xp is np else torch.float64
    i32 = np.int32 if xp is np else torch.int32
    to = (lambda a, t: a.astype(t)) if xp is np else (lambda a, t: a.to(t))
    inter, box, mask = to(out["inter"], f64), to(out["area_box"], f64), to(out["area_mask"], f64)[:, None, :]
    usable = (out["flags"] & USABLE) != 0
    nan = xp.full_like(inter, float("nan"))

    def ratio(den):
        den = den + xp.zeros_like(inter)
        keep = usable & (den != 0)
        one = xp.ones_like(inter)
        return xp.where(keep, inter / xp.where(keep, den, one), nan)

    out["iou"], out["coverage"], out["precision"] = ratio((box + mask) - inter), ratio(mask), ratio(box)
    out["valid"] = to(usable, i32)
    return out


def box_silhouette(boxes, K, E, masks, ok=None, stream=None) -> dict:
    """boxes [n,S,8,3] world frame (read as float64; numpy or CUDA; [n,8,3]: S = 1), K [n,3,3] (every view's) or [n,V,3,3], E [n,V,4,4]
    world -> camera, masks [n,V,H,W] (uint8 / bool are read where they lie, any non-zero byte is foreground; [n,H,W] with E [n,4,4]:
    V = 1), ok [n,S] or None -> dict of CUDA tensors, int32: `area_box` [n,S,V] (silhouette pixels inside the frame), `inter` [n,S,V]
    (those inside the mask), `area_mask` [n,V], `rect` [n,S,V,4] (row min, col min, row max, col max; (H, W, -1, -1) when empty), `flags`
    [n,S,V] (1 usable, 2 camera inside the box, 4 the silhouette touches the frame border, 8 a corner at z_cam <= 0), `valid` [n,S,V];
    float64: `iou` = inter / (area_box + area_mask - inter), `coverage` = inter / area_mask, `precision` = inter / area_box, each NaN
    where its denominator is 0 or the box is unusable.  1 <= S <= 64, 1 <= V <= 16, n S V <= 2^24, H W < 2^31."""
    lib = _lib.load()
    boxes = torch.as_tensor(boxes)
    dev = _device_of(boxes)
    boxes, Kd, Ed = (torch.as_tensor(x).to(device=dev, dtype=torch.float64) for x in (boxes, K, E))
    masks = torch.as_tensor(masks)
    n, S, V, H, W, k_views = _silhouette_shapes("box_silhouette", boxes.shape, Kd.shape, Ed.shape, masks.shape)
    boxes, Ed = boxes.reshape(n, S, 8, 3).contiguous(), Ed.reshape(n, V, 4, 4).contiguous()
    Kd = (Kd if k_views else Kd[:, None].expand(n, V, 3, 3)).contiguous()
    m = _mask_bytes(masks, dev).view(n, V, H, W)
    ok = _ok_tensor(ok, (n, S), dev, "box_silhouette: ok")
    out = {k: torch.empty(*shp, dtype=torch.int32, device=dev) for k, shp in
           (("area_box", (n, S, V)), ("inter", (n, S, V)), ("area_mask", (n, V)), ("rect", (n, S, V, 4)), ("flags", (n, S, V)))}
    need = C.c_size_t(0)
    _lib.check(lib.rgbm_box_silhouette_scratch_bytes(n, S, V, C.byref(need)), "rgbm_box_silhouette_scratch_bytes")
    scratch = torch.empty((need.value + 7) // 8, dtype=torch.float64, device=dev)
    if stream is not None:
        for t in (boxes, Kd, Ed, m, ok, scratch, *out.values()):
            if t is not None:
                t.record_stream(stream)
    _lib.check(lib.rgbm_box_silhouette(_lib.ptr(boxes), _lib.ptr(ok), _lib.ptr(Kd), _lib.ptr(Ed), _lib.ptr(m), n, S, V, H, W,
                                       *[_lib.ptr(out[k]) for k in INT_KEYS], _lib.ptr(scratch), scratch.numel() * 8, _lib.stream_ptr(stream)),
               "rgbm_box_silhouette")
    if stream is not None:
        with torch.cuda.stream(stream):
            return _ratios(out, torch)
    return _ratios(out, torch)


def _cloud_shapes(name, cloud, count, boxes):
    c, k, b = tuple(cloud), tuple(count), tuple(boxes)
    if len(b) == 3:
        b = (b[0], 1) + b[1:]
    if len(b) != 4 or b[2:] != (8, 3):
        raise ValueError(f"{name}: boxes [n, S, 8, 3] or [n, 8, 3], got {tuple(boxes)}")
    n, S = int(b[0]), int(b[1])
    if len(c) != 3 or c[0] != n or c[2] != 3:
        raise ValueError(f"{name}: cloud [n, cap, 3], got {tuple(cloud)}")
    if len(k) == 1:
        k = k + (1,)
    if len(k) != 2 or k[0] != n or not 1 <= k[1] <= MAX_COUNT_COLS:
        raise ValueError(f"{name}: count [n] or [n, C] with 1 <= C <= {MAX_COUNT_COLS}, got {tuple(count)}")
    if not 1 <= S <= MAX_BOXES:
        raise ValueError(f"{name}: 1 <= S <= {MAX_BOXES} boxes per pose, got S = {S}")
    if n < 1 or n * S > MAX_RECORDS:
        raise ValueError(f"{name}: n >= 1 and n * S <= 2^24, got n = {n}, S = {S}")
    if c[1] > MAX_CAP:
        raise ValueError(f"{name}: cap <= 2^30, got {c[1]}")
    return n, S, int(c[1]), int(k[1])


def _check_inflate(name, inflate):
    inflate = float(inflate)
    if not (0.0 <= inflate < float("inf")):
        raise ValueError(f"{name}: inflate must be finite and >= 0, got {inflate}")
    return inflate


def _world_model(c, xp):
    """c [..., 8, 3] float64 -> (o, n [..., 3, 3], det, finite) of the box model in the frame of c, every product and sum rounded on its
    own (numpy and torch elementwise operations do that; the kernels are built without contraction)."""
    o = c[..., 0, :]
    e = [c[..., k, :] - o for k in _EDGE_CORNER]
    nn = []
    for d in range(3):
        u, v = e[(d + 1) % 3], e[(d + 2) % 3]
        nn.append(xp.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                            u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1))
    det = (e[0][..., 0] * nn[0][..., 0] + e[0][..., 1] * nn[0][..., 1]) + e[0][..., 2] * nn[0][..., 2]
    fin = xp.isfinite(c).reshape(*c.shape[:-2], 24).all(-1)
    return o, xp.stack(nn, -2), det, fin


def cloud_in_box(cloud, count, boxes, ok=None, inflate: float = 0.0, stream=None) -> dict:
    """cloud [n,cap,3] f32 and count [n,2] i32 as `cloud_pack` returns them ([n,V] of `cloud_pack_views` or a flat [n] alike: the first
    min(sum of the counts, cap) rows of a pose hold its points), boxes [n,S,8,3] world frame (float64; [n,8,3]: S = 1), ok [n,S] or None,
    inflate >= 0 -> dict of CUDA tensors: `inside` [n,S] i32 (rows p with lo - inflate |det| <= n_k . (p - o) <= hi + inflate |det| for
    k = 0, 1, 2: the box grown by `inflate` edge lengths on every side; a non-finite row is never inside), `total` [n] i32 (the rows
    counted), `valid` [n,S] i32 and `share` [n,S] f64 = inside / total, NaN when total is 0 or the box is unusable."""
    lib = _lib.load()
    boxes = torch.as_tensor(boxes)
    dev = _device_of(boxes)
    boxes = boxes.to(device=dev, dtype=torch.float64)
    cloud = torch.as_tensor(cloud).to(device=dev, dtype=torch.float32).contiguous()
    count = torch.as_tensor(count).to(device=dev, dtype=torch.int32).contiguous()
    n, S, cap, cols = _cloud_shapes("cloud_in_box", cloud.shape, count.shape, boxes.shape)
    inflate = _check_inflate("cloud_in_box", inflate)
    boxes = boxes.reshape(n, S, 8, 3).contiguous()
    ok = _ok_tensor(ok, (n, S), dev, "cloud_in_box: ok")
    inside = torch.empty(n, S, dtype=torch.int32, device=dev)
    total = torch.empty(n, dtype=torch.int32, device=dev)
    if stream is not None:
        for t in (boxes, cloud, count, ok, inside, total):
            if t is not None:
                t.record_stream(stream)
    _lib.check(lib.rgbm_cloud_in_box(_lib.ptr(cloud) if cap else None, _lib.ptr(count), cols, _lib.ptr(boxes), _lib.ptr(ok), n, S, cap, inflate,
                                     _lib.ptr(inside), _lib.ptr(total), _lib.stream_ptr(stream)), "rgbm_cloud_in_box")
    ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream(dev))
    with ctx:
        _, _, det, fin = _world_model(boxes, torch)
        usable = fin & (det.abs() > 0.0)
        if ok is not None:
            usable = usable & (ok != 0)
        return _share({"inside": inside, "total": total}, usable, torch)


def _share(out, usable, xp):
    f64 = np.float64 if xp is np else torch.float64
    i32 = np.int32 if xp is np else torch.int32
    to = (lambda a, t: a.astype(t)) if xp is np else (lambda a, t: a.to(t))
    ins = to(out["inside"], f64)
    tot = to(out["total"], f64)[:, None] + xp.zeros_like(ins)
    keep = usable & (tot != 0)
    out["valid"] = to(usable, i32)
    out["share"] = xp.where(keep, ins / xp.where(keep, tot, xp.ones_like(ins)), xp.full_like(ins, float("nan")))
    return out


# ------------------------------------------------------------------------------------------------------------------ float64 numpy twins
def box_silhouette_ref(boxes, K, E, masks, ok=None) -> dict:
    """float64 numpy twin of `box_silhouette`: the same dict as numpy arrays.  Every pixel of every frame is tested against every usable
    box (no bound, no culling), with the kernel's expressions in the kernel's order."""
    boxes, K, E = (np.asarray(x, dtype=np.float64) for x in (boxes, K, E))
    masks = np.asarray(masks)
    n, S, V, H, W, k_views = _silhouette_shapes("box_silhouette_ref", boxes.shape, K.shape, E.shape, masks.shape)
    boxes, E, masks = boxes.reshape(n, S, 8, 3), E.reshape(n, V, 4, 4), masks.reshape(n, V, H, W) != 0
    K = K if k_views else np.broadcast_to(K[:, None], (n, V, 3, 3))
    ok = _check_ok(ok, (n, S), "box_silhouette_ref: ok")
    out = {"area_box": np.zeros((n, S, V), np.int32), "inter": np.zeros((n, S, V), np.int32), "area_mask": np.zeros((n, V), np.int32),
           "rect": np.tile(np.asarray([H, W, -1, -1], np.int32), (n, S, V, 1)), "flags": np.zeros((n, S, V), np.int32)}
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        x, y, z = (boxes[:, :, None, :, None, a] for a in range(3))                              # [n, S, 1, 8, 1]
        R = E[:, None, :, None, :3, :]                                                           # [n, 1, V, 1, 3, 4]
        cam = ((R[..., 0] * x + R[..., 1] * y) + R[..., 2] * z) + R[..., 3]                      # [n, S, V, 8, 3]
        o, nn, det, _ = _world_model(cam, np)
        lo, hi = np.where(det < 0.0, det, 0.0), np.where(det > 0.0, det, 0.0)
        q0 = -((nn[..., 0] * o[..., None, 0] + nn[..., 1] * o[..., None, 1]) + nn[..., 2] * o[..., None, 2])      # [n, S, V, 3]
        fx, cx, fy, cy = K[:, :, 0, 0], K[:, :, 0, 2], K[:, :, 1, 1], K[:, :, 1, 2]
        fin_cam = np.isfinite(E[:, :, :3, :]).reshape(n, V, 12).all(-1) & np.isfinite(fx) & np.isfinite(fy) & np.isfinite(cx) & np.isfinite(cy) \
            & (fx != 0.0) & (fy != 0.0)
        fin_box = np.isfinite(boxes).reshape(n, S, 24).all(-1)
        usable = fin_box[:, :, None] & fin_cam[:, None, :] & ok[:, :, None] & (np.abs(det) > 0.0)
        inside = ((lo[..., None] <= q0) & (q0 <= hi[..., None])).all(-1)
        behind = (cam[..., 2] <= 0.0).any(-1)
        out["flags"][:] = np.where(usable, USABLE | np.where(inside, CAMERA_INSIDE, 0) | np.where(behind, BEHIND, 0), 0)
        cols, rows = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
        for i in range(n):
            for v in range(V):
                fg = masks[i, v]
                out["area_mask"][i, v] = int(fg.sum())
                xn, yn = ((cols - cx[i, v]) / fx[i, v])[None, :], ((rows - cy[i, v]) / fy[i, v])[:, None]
                for s in range(S):
                    if not usable[i, s, v]:
                        continue
                    l, h = lo[i, s, v], hi[i, s, v]
                    tmin, tmax = np.full((H, W), -np.inf), np.full((H, W), np.inf)
                    for k in range(3):
                        q = q0[i, s, v, k]
                        dq = (nn[i, s, v, k, 0] * xn + nn[i, s, v, k, 1] * yn) + nn[i, s, v, k, 2]
                        t1, t2 = (l - q) / dq, (h - q) / dq
                        nz = dq != 0.0
                        tn = np.where(nz, np.fmin(t1, t2), -np.inf if l <= q <= h else np.inf)
                        tf = np.where(nz, np.fmax(t1, t2), np.inf)
                        tmin = np.where(tn > tmin, tn, tmin)
                        tmax = np.fmin(tmax, tf)
                    hit = (tmax >= tmin) & (tmin > 0.0)
                    area = int(hit.sum())
                    out["area_box"][i, s, v] = area
                    out["inter"][i, s, v] = int((hit & fg).sum())
                    if area:
                        r, c = np.nonzero(hit.any(axis=1))[0], np.nonzero(hit.any(axis=0))[0]
                        out["rect"][i, s, v] = (r[0], c[0], r[-1], c[-1])
                        if r[0] == 0 or c[0] == 0 or r[-1] == H - 1 or c[-1] == W - 1:
                            out["flags"][i, s, v] |= BORDER
    return _ratios(out, np)


def cloud_in_box_ref(cloud, count, boxes, ok=None, inflate: float = 0.0) -> dict:
    """float64 numpy twin of `cloud_in_box`: the same dict as numpy arrays."""
    cloud, count, boxes = np.asarray(cloud, dtype=np.float32), np.asarray(count, dtype=np.int32), np.asarray(boxes, dtype=np.float64)
    n, S, cap, cols = _cloud_shapes("cloud_in_box_ref", cloud.shape, count.shape, boxes.shape)
    inflate = _check_inflate("cloud_in_box_ref", inflate)
    boxes, count = boxes.reshape(n, S, 8, 3), count.reshape(n, cols).astype(np.int64)
    ok = _check_ok(ok, (n, S), "cloud_in_box_ref: ok")
    inside, total = np.zeros((n, S), np.int32), np.minimum(np.maximum(count, 0).sum(axis=1), cap).astype(np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        o, nn, det, fin = _world_model(boxes, np)
        m = inflate * np.abs(det)
        lo, hi = np.where(det < 0.0, det, 0.0) - m, np.where(det > 0.0, det, 0.0) + m
        usable = fin & ok & (np.abs(det) > 0.0)
        for i in range(n):
            p = cloud[i, :total[i]].astype(np.float64)
            live = np.isfinite(p).all(axis=1)
            for s in range(S):
                if not usable[i, s]:
                    continue
                d = p - o[i, s]
                inn = live
                for k in range(3):
                    a = (nn[i, s, k, 0] * d[:, 0] + nn[i, s, k, 1] * d[:, 1]) + nn[i, s, k, 2] * d[:, 2]
                    inn = inn & (lo[i, s] <= a) & (a <= hi[i, s])
                inside[i, s] = int(inn.sum())
    return _share({"inside": inside, "total": total}, usable, np)


# ------------------------------------------------------------------------------------------------------------------ selection
def select_by_mask(sil) -> dict:
    """sil: the dict of `box_silhouette` (CUDA tensors) or of `box_silhouette_ref` (numpy) -> `score` [n,S] f64, the mean of `iou` over
    the views with area_mask > 0, summed over the views in ascending order (NaN when there is no such view, or the box is unusable in
    one of them), and `best` [n] i64, the index of the largest score: NaN never wins, ties go to the lowest index, -1 when every score
    of the pose is NaN."""
    xp = torch if isinstance(sil["iou"], torch.Tensor) else np
    iou, seen = sil["iou"], sil["area_mask"][:, None, :] > 0
    n, S, V = iou.shape
    seen = seen & (xp.zeros_like(iou) == 0)                                   # [n, S, V]
    zero = xp.zeros_like(iou[:, :, 0])
    total, views = zero, zero
    bad = zero != 0
    for v in range(V):
        total = total + xp.where(seen[:, :, v], iou[:, :, v], zero)          # a NaN of a seen view makes the score NaN
        views = views + xp.where(seen[:, :, v], zero + 1.0, zero)
        bad = bad | (sil["valid"][:, :, v] == 0)
    nan = xp.full_like(zero, float("nan"))
    keep = (views > 0) & ~bad
    score = xp.where(keep, total / xp.where(keep, views, zero + 1.0), nan)
    low = xp.where(xp.isnan(score), xp.full_like(zero, -float("inf")), score)
    if xp is np:
        top = low.max(axis=1)
        first = np.where(low == top[:, None], np.arange(S)[None, :], S).min(axis=1).astype(np.int64)
        return {"score": score, "best": np.where(np.isnan(score).all(axis=1), -1, first)}
    top = low.max(dim=1).values
    index = torch.arange(S, device=low.device)[None, :].expand(n, S)
    first = torch.where(low == top[:, None], index, torch.full_like(index, S)).min(dim=1).values
    return {"score": score, "best": torch.where(torch.isnan(score).all(dim=1), torch.full_like(first, -1), first)}


# ------------------------------------------------------------------------------------------------------------------ estimator results
def _hypotheses(name, hyp, ok, K, E1, mask1, E2, mask2, ref):
    """The silhouettes of hyp [n,P,8,3] (ok [n,P]) in the two views of a call, each view's mask read where it lies (no [n,2,H,W] copy):
    the dict of `box_silhouette` with V = 2.  P may exceed 64: the boxes then go in groups."""
    P = hyp.shape[1]
    parts = []
    for E, mask in ((E1, mask1), (E2, mask2)):
        groups = []
        for lo in range(0, P, MAX_BOXES):
            a = (hyp[:, lo:lo + MAX_BOXES], K, E, mask, ok[:, lo:lo + MAX_BOXES])
            groups.append(box_silhouette_ref(*a) if ref else box_silhouette(*a))
        parts.append(groups)
    xp = np if ref else torch
    cat = np.concatenate if ref else torch.cat
    out = {}
    for k in parts[0][0]:
        if k == "area_mask":
            out[k] = cat([parts[0][0][k], parts[1][0][k]], 1)
        else:
            out[k] = cat([cat([g[k] for g in view], 1) for view in parts], 2)
    assert out["iou"].shape == (hyp.shape[0], P, 2) and xp is not None, name
    return out


def _result_inputs(name, r, keys, ref):
    for k in keys:
        if k not in r:
            raise ValueError(f"{name}: the result holds no `{k}`")
    if ref:
        return [_to_numpy(r[k]) for k in keys]
    dev = _device_of(torch.as_tensor(r[keys[0]]))
    return [torch.as_tensor(r[k]).to(dev) for k in keys]


def _host(out, r, keys, ref):
    return {k: v.cpu().numpy() for k, v in out.items()} if not ref and _is_numpy(r, keys) else out


def samples_verify(r, K, E1, mask1, E2, mask2, ref: bool = False) -> dict:
    """r: the dict of `estimate_samples` / `estimate_samples_device`; K [n,3,3], E1 / E2 [n,4,4] and mask1 / mask2 [n,H,W]: the cameras
    and masks of that call.  The hypotheses of a pose are its S draws `bbox_samples` (usable when finite and not DEFAULT_BBOX, the
    condition `estimate_samples` counts with) followed by the mean box `bbox` at index S (ok: `valid`).  Returns the dict of
    `box_silhouette` for them ([n,S+1,2] per key, `area_mask` [n,2]) plus `score` [n,S+1] and `best` [n] of `select_by_mask` and
    `bbox_best` [n,8,3] f64, the chosen hypothesis (DEFAULT_BBOX where best is -1).  A dict of numpy arrays gives numpy arrays, one of
    CUDA tensors CUDA tensors; `ref`: the numpy twins instead of the kernel (numpy in and out)."""
    keys = ("bbox_samples", "bbox", "valid")
    box, mean, valid = _result_inputs("samples_verify", r, keys, ref)
    xp = np if ref else torch
    if box.ndim != 4 or tuple(box.shape[2:]) != (8, 3):
        raise ValueError(f"samples_verify: bbox_samples [n, S, 8, 3], got {tuple(box.shape)}")
    n, S = int(box.shape[0]), int(box.shape[1])
    if ref:
        box, mean = box.astype(np.float64), np.asarray(mean, dtype=np.float64)
        dflt = DEFAULT_BBOX
        ok = np.isfinite(box.reshape(n, S, 24)).all(axis=2) & ~(box == dflt).all(axis=3).all(axis=2)
        hyp, ok = np.concatenate([box, mean[:, None]], 1), np.concatenate([ok, (valid != 0)[:, None]], 1)
    else:
        box, mean = box.to(torch.float64), mean.to(torch.float64)
        dflt = torch.from_numpy(DEFAULT_BBOX).to(box.device)
        ok = torch.isfinite(box.reshape(n, S, 24)).all(dim=2) & ~(box == dflt).all(dim=3).all(dim=2)
        hyp, ok = torch.cat([box, mean[:, None]], 1), torch.cat([ok, (valid != 0)[:, None]], 1)
    out = _hypotheses("samples_verify", hyp, ok, K, E1, mask1, E2, mask2, ref)
    out.update(select_by_mask(out))
    best = out["best"]
    pick = hyp[xp.arange(n) if ref else torch.arange(n, device=hyp.device), xp.where(best < 0, xp.zeros_like(best), best)]
    out["bbox_best"] = xp.where((best >= 0).reshape(n, 1, 1), pick, dflt[None] + xp.zeros_like(pick))
    return _host(out, r, keys, ref)


def cloud_pose_verify(r, K, E1, mask1, E2, mask2, inflate: float = 0.0, ref: bool = False) -> dict:
    """r: the dict of `estimate_cloud_pose` / `estimate_cloud_pose_device`; K, E1, mask1, E2, mask2: the cameras and masks of that call.
    The hypotheses of a pose are the network's box `bbox` (index 0, ok: `valid`) and the box fitted to the cloud `bbox_cloud` (index 1,
    ok: `valid_cloud`).  Returns the dict of `box_silhouette` for them ([n,2,2] per key), `inside` [n,2], `total` [n] and `share` [n,2] of
    `cloud_in_box` on `cloud` / `count` with `inflate`, and `score` [n,2] / `best` [n] of `select_by_mask`.  numpy in, numpy out; CUDA
    in, CUDA out; `ref`: the numpy twins instead of the kernels (numpy in and out)."""
    keys = ("bbox", "bbox_cloud", "valid", "valid_cloud", "cloud", "count")
    a, b, va, vb, cloud, count = _result_inputs("cloud_pose_verify", r, keys, ref)
    if ref:
        hyp, ok = np.stack([np.asarray(a, np.float64), np.asarray(b, np.float64)], 1), np.stack([va != 0, vb != 0], 1)
    else:
        hyp, ok = torch.stack([a.to(torch.float64), b.to(torch.float64)], 1), torch.stack([va != 0, vb != 0], 1)
    out = _hypotheses("cloud_pose_verify", hyp, ok, K, E1, mask1, E2, mask2, ref)
    out.update(select_by_mask(out))
    share = (cloud_in_box_ref if ref else cloud_in_box)(cloud, count, hyp, ok, inflate)
    out.update(inside=share["inside"], total=share["total"], share=share["share"])
    return _host(out, r, keys, ref)
