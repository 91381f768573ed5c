"""Agreement of two oriented boxes: exact 3-D IoU of two parallelepipeds and the centre, corner, extent and rotation errors between
them.  `box_agreement` and `box_iou_matrix` run the kernels of csrc/box_overlap.hip (C ABI rgbm_box_agreement / rgbm_box_iou_matrix in
include/rgbm.h); `box_agreement_ref` and `box_iou_matrix_ref` are their float64 numpy twins, which evaluate the same expressions in
the same order, the rule for coincident planes included.  `cloud_pose_agreement` and `samples_overlap` feed them the dicts that
`estimate_cloud_pose` and `estimate_samples` return.

The box model: [8, 3] corners in get_3d_bbox's order, read as o + a ex + b ey + c ez, 0 <= a, b, c <= 1, with o = corner 0 and
ex, ey, ez = corner 2, 4, 1 - corner 0.  The other four corners enter the finiteness check, the centre (mean of the 8) and
`corner_dist` only.  volume = |det[ex ey ez]|.  A box is unusable when a coordinate is not finite, its volume is not > 0 or its ok is
0; every metric of a pair with an unusable box is NaN and its `valid` is 0.  Edge lengths are meant to lie within 1e-60 .. 1e60 (boxes
are metres): the face normals go through products of four edge lengths, which overflow or vanish outside that range, and the results
are then not defined.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .cloud import DEFAULT_BBOX

MAX_PAIRS = 1 << 24               # kBoxPairsMax (csrc/box_overlap.h)
MAX_MATRIX = 64                   # kBoxMatrixMax
MAX_MATRIX_PAIRS = 2 ** 31 - 1
TAU = 1e-12                       # coincident planes: 1 - TAU on the normals, TAU * L on the offsets
AGREEMENT_KEYS = ("valid", "iou", "inter_volume", "volume_a", "volume_b", "center_dist", "center_delta", "corner_dist", "extent_a",
                  "extent_b", "axis_angle_deg", "axis_fold_deg", "rot_deg")
_SHAPES = {"iou": (), "inter_volume": (), "volume_a": (), "volume_b": (), "center_dist": (), "center_delta": (3,), "corner_dist": (),
           "extent_a": (3,), "extent_b": (3,), "axis_angle_deg": (3,), "axis_fold_deg": (3,), "rot_deg": ()}
_EDGE_CORNER = (2, 4, 1)          # far ends of the x, y, z edges that leave corner 0
_MAXV = 10                        # vertices of a quad clipped by 6 planes


def _device_of(t):
    return t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())


def _ok_tensor(ok, shape, dev, name):
    if ok is None:
        return None
    ok = torch.as_tensor(ok).to(device=dev)
    ok = (ok if ok.dtype == torch.uint8 else (ok != 0).to(torch.uint8)).contiguous()
    if tuple(ok.shape) != tuple(shape):
        raise ValueError(f"{name} {list(shape)}, got {tuple(ok.shape)}")
    return ok


def box_agreement(a, b, ok_a=None, ok_b=None, stream=None) -> dict:
    """a, b [n, 8, 3] (read as float64; numpy or CUDA), ok_a / ok_b [n] or None (non-zero: the box may count) -> dict of CUDA tensors
    for pair i = (a[i], b[i]), float64 unless noted: `valid` [n] i32 (both boxes usable), `iou`, `inter_volume`, `volume_a`, `volume_b`
    [n], `center_dist` [n], `center_delta` [n,3] (b - a), `corner_dist` [n] (mean over the 8 corners of |a_k - b_k|), `extent_a` /
    `extent_b` [n,3] (edge lengths x, y, z), `axis_angle_deg` [n,3] (between the unit edges, 0..180), `axis_fold_deg` [n,3]
    (min(angle, 180 - angle): handles are symmetric under half turns), `rot_deg` [n] (acos((sum of the three unit-edge dot products
    - 1) / 2)).  1 <= n <= 2^24."""
    lib = _lib.load()
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    dev = _device_of(a)
    a = a.to(device=dev, dtype=torch.float64).contiguous()
    b = b.to(device=dev, dtype=torch.float64).contiguous()
    if a.dim() != 3 or tuple(a.shape[1:]) != (8, 3) or tuple(b.shape) != tuple(a.shape):
        raise ValueError(f"box_agreement: a and b [n, 8, 3], got {tuple(a.shape)} and {tuple(b.shape)}")
    n = int(a.shape[0])
    if not 1 <= n <= MAX_PAIRS:
        raise ValueError(f"box_agreement: 1 <= n <= {MAX_PAIRS} pairs, got n = {n}")
    ok_a = _ok_tensor(ok_a, (n,), dev, "box_agreement: ok_a")
    ok_b = _ok_tensor(ok_b, (n,), dev, "box_agreement: ok_b")
    out = {"valid": torch.empty(n, dtype=torch.int32, device=dev)}
    out.update({k: torch.empty(n, *shp, dtype=torch.float64, device=dev) for k, shp in _SHAPES.items()})
    if stream is not None:
        for t in (a, b, ok_a, ok_b, *out.values()):
            if t is not None:
                t.record_stream(stream)
    _lib.check(lib.rgbm_box_agreement(_lib.ptr(a), _lib.ptr(b), _lib.ptr(ok_a), _lib.ptr(ok_b), n, *[_lib.ptr(out[k]) for k in AGREEMENT_KEYS],
                                      _lib.stream_ptr(stream)), "rgbm_box_agreement")
    return out


def _matrix_shapes(name, a_shape, b_shape):
    if len(a_shape) != 4 or tuple(a_shape[2:]) != (8, 3) or len(b_shape) != 4 or tuple(b_shape[2:]) != (8, 3) or b_shape[0] != a_shape[0]:
        raise ValueError(f"{name}: a [n, P, 8, 3] and b [n, Q, 8, 3], got {tuple(a_shape)} and {tuple(b_shape)}")
    n, P, Q = int(a_shape[0]), int(a_shape[1]), int(b_shape[1])
    if not (1 <= P <= MAX_MATRIX and 1 <= Q <= MAX_MATRIX):
        raise ValueError(f"{name}: 1 <= P, Q <= {MAX_MATRIX} boxes per pose, got P = {P}, Q = {Q}")
    if not 1 <= n or n * P * Q > MAX_MATRIX_PAIRS:
        raise ValueError(f"{name}: n >= 1 and n * P * Q <= 2^31 - 1 pairs, got n = {n}, P = {P}, Q = {Q}")
    return n, P, Q


def box_iou_matrix(a, b=None, ok_a=None, ok_b=None, stream=None):
    """a [n, P, 8, 3], b [n, Q, 8, 3] (read as float64; numpy or CUDA; b = None: b = a and ok_b = ok_a), ok_a [n, P] / ok_b [n, Q] or
    None -> iou [n, P, Q] float64 CUDA, the `iou` of `box_agreement` for every pair of a pose, NaN where either box is unusable.
    1 <= P, Q <= 64, n P Q <= 2^31 - 1."""
    lib = _lib.load()
    a = torch.as_tensor(a)
    dev = _device_of(a)
    a = a.to(device=dev, dtype=torch.float64).contiguous()
    if b is None:
        b, ok_b = a, ok_a
    else:
        b = torch.as_tensor(b).to(device=dev, dtype=torch.float64).contiguous()
    n, P, Q = _matrix_shapes("box_iou_matrix", a.shape, b.shape)
    ok_a = _ok_tensor(ok_a, (n, P), dev, "box_iou_matrix: ok_a")
    ok_b = _ok_tensor(ok_b, (n, Q), dev, "box_iou_matrix: ok_b")
    iou = torch.empty(n, P, Q, dtype=torch.float64, device=dev)
    if stream is not None:
        for t in (a, b, ok_a, ok_b, iou):
            if t is not None:
                t.record_stream(stream)
    _lib.check(lib.rgbm_box_iou_matrix(_lib.ptr(a), _lib.ptr(b), _lib.ptr(ok_a), _lib.ptr(ok_b), n, P, Q, _lib.ptr(iou), _lib.stream_ptr(stream)),
               "rgbm_box_iou_matrix")
    return iou


# ------------------------------------------------------------------------------------------------------------------ float64 numpy twins
def _dot3(x, y):
    return x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1] + x[..., 2] * y[..., 2]


def _derive(c, ok):
    """derive_box of the kernel file for N boxes: c [N, 8, 3], ok [N] bool -> the record as a dict of arrays."""
    N = c.shape[0]
    fin = np.isfinite(c.reshape(N, 24)).all(axis=1)
    s = np.zeros((N, 3))
    for k in range(8):
        s = s + c[:, k]
    ctr = s / 8.0
    e = np.stack([c[:, k] - c[:, 0] for k in _EDGE_CORNER], axis=1)                      # [N, edge, xyz]
    nn = np.empty((N, 3, 3))                                                             # ey x ez, ez x ex, ex x ey
    for d in range(3):
        u, v = e[:, (d + 1) % 3], e[:, (d + 2) % 3]
        nn[:, d, 0] = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
        nn[:, d, 1] = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
        nn[:, d, 2] = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
    det = _dot3(e[:, 0], nn[:, 0])
    vol = np.abs(det)
    sg = np.where(det < 0.0, -1.0, 1.0)
    length = np.sqrt(_dot3(nn, nn))
    g = e[:, 0] + e[:, 1] + e[:, 2]
    return {"c": ctr, "o": c[:, 0] - ctr, "e": e, "n": sg[:, None, None] * nn / length[:, :, None], "vol": vol, "diag": np.sqrt(_dot3(g, g)),
            "ok": np.asarray(ok, dtype=bool) & fin & (vol > 0.0)}


def _take(rec, idx):
    return {k: v[idx] for k, v in rec.items()}


def _inter_volume(A, B):
    """pair_faces + pair_inter of the kernel file for M pairs of usable boxes (records A, B) -> inter [M]."""
    M = A["vol"].shape[0]
    if M == 0:
        return np.zeros(0)
    normal, offset = np.empty((M, 12, 3)), np.empty((M, 12))
    poly = np.zeros((M, 12, _MAXV, 3))
    for f in range(12):
        side, fi = divmod(f, 6)
        ax, hi = fi >> 1, fi & 1
        own = B if side else A
        base = own["o"]
        if side:
            base = base + (B["c"] - A["c"])
        if hi:
            base = base + own["e"][:, ax]
        nf = own["n"][:, ax] if hi else -own["n"][:, ax]
        normal[:, f], offset[:, f] = nf, _dot3(nf, base)
        u, v = own["e"][:, (ax + 1) % 3], own["e"][:, (ax + 2) % 3]
        poly[:, f, 0], poly[:, f, 1], poly[:, f, 2], poly[:, f, 3] = base, base + u, (base + u) + v, base + v
    tol = TAU * np.maximum(A["diag"], B["diag"])
    drop, opp = np.zeros((M, 6), dtype=bool), np.zeros((M, 6), dtype=bool)
    for j in range(6):
        for i in range(6):
            dot = _dot3(normal[:, i], normal[:, 6 + j])
            drop[:, j] |= (dot >= 1.0 - TAU) & (np.abs(offset[:, i] - offset[:, 6 + j]) <= tol)
            opp[:, j] |= (dot <= -(1.0 - TAU)) & (np.abs(offset[:, i] + offset[:, 6 + j]) <= tol)
    # the 12 face lanes of every pair, flattened
    K = M * 12
    rows = np.arange(K)
    poly = poly.reshape(K, _MAXV, 3)
    cnt = np.full((M, 12), 4)
    cnt[:, 6:][drop] = 0
    cnt = cnt.reshape(K)
    is_a = np.tile(np.arange(12) < 6, M)
    for j in range(6):
        q = np.concatenate([np.broadcast_to(normal[:, 6 + j, None], (M, 6, 3)), np.broadcast_to(normal[:, j, None], (M, 6, 3))], axis=1).reshape(K, 3)
        q3 = np.concatenate([np.broadcast_to(offset[:, 6 + j, None], (M, 6)), np.broadcast_to(offset[:, j, None], (M, 6))], axis=1).reshape(K)
        active = (cnt > 0) & ~(is_a & np.repeat(drop[:, j], 12))
        s = (q[:, None, 0] * poly[:, :, 0] + q[:, None, 1] * poly[:, :, 1] + q[:, None, 2] * poly[:, :, 2]) - q3[:, None]
        new, m = np.zeros_like(poly), np.zeros(K, dtype=np.int64)
        for i in range(_MAXV):
            sel = active & (i < cnt)
            if not sel.any():
                break
            k = np.where(i + 1 == cnt, 0, np.minimum(i + 1, _MAXV - 1))
            P, Q, sP, sQ = poly[:, i], poly[rows, k], s[:, i], s[rows, k]
            inP, inQ = sP <= 0.0, sQ <= 0.0
            w = sel & inP & (m < _MAXV)
            new[w, m[w]] = P[w]
            m[w] += 1
            w = sel & (inP != inQ) & (m < _MAXV)
            t = sP[w] / (sP[w] - sQ[w])
            new[w, m[w]] = P[w] + t[:, None] * (Q[w] - P[w])
            m[w] += 1
        poly = np.where(active[:, None, None], new, poly)
        cnt = np.where(active, m, cnt)
    v0 = poly[:, 0]
    a = poly[:, 1] - v0
    s = np.zeros((K, 3))
    for i in range(2, _MAXV):
        sel = i < cnt
        c = poly[:, i] - v0
        term = np.stack([a[:, 1] * c[:, 2] - a[:, 2] * c[:, 1], a[:, 2] * c[:, 0] - a[:, 0] * c[:, 2], a[:, 0] * c[:, 1] - a[:, 1] * c[:, 0]], axis=1)
        s = np.where(sel[:, None], s + term, s)
        a = np.where(sel[:, None], c, a)
    area = np.where(cnt >= 3, 0.5 * np.abs(_dot3(normal.reshape(K, 3), s)), 0.0)
    part = (offset.reshape(K) * area).reshape(M, 12)
    total = np.zeros(M)
    for f in range(12):
        total = total + part[:, f]
    total = total / 3.0
    lim = np.minimum(A["vol"], B["vol"])
    return np.where(opp.any(axis=1), 0.0, np.where(total < 0.0, 0.0, np.where(total > lim, lim, total)))


def _iou_of_records(A, B):
    """records of N pairs -> (usable [N] bool, inter [N], iou [N]); NaN where a box is unusable."""
    usable = A["ok"] & B["ok"]
    idx = np.nonzero(usable)[0]
    inter = np.full(usable.shape[0], np.nan)
    inter[idx] = _inter_volume(_take(A, idx), _take(B, idx))
    with np.errstate(invalid="ignore"):
        return usable, inter, inter / ((A["vol"] + B["vol"]) - inter)


def _acos_deg(c):
    c = np.where(c > 1.0, 1.0, np.where(c < -1.0, -1.0, c))
    return np.arccos(c) * (180.0 / 3.14159265358979323846)


def _check_ok(ok, shape, name):
    if ok is None:
        return np.ones(shape, dtype=bool)
    ok = np.asarray(ok) != 0
    if ok.shape != tuple(shape):
        raise ValueError(f"{name} {list(shape)}, got {ok.shape}")
    return ok


def box_agreement_ref(a, b, ok_a=None, ok_b=None) -> dict:
    """float64 numpy twin of `box_agreement`: the same dict as numpy arrays."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.ndim != 3 or a.shape[1:] != (8, 3) or b.shape != a.shape:
        raise ValueError(f"box_agreement_ref: a and b [n, 8, 3], got {a.shape} and {b.shape}")
    n = a.shape[0]
    if not 1 <= n <= MAX_PAIRS:
        raise ValueError(f"box_agreement_ref: 1 <= n <= {MAX_PAIRS} pairs, got n = {n}")
    ok_a, ok_b = _check_ok(ok_a, (n,), "box_agreement_ref: ok_a"), _check_ok(ok_b, (n,), "box_agreement_ref: ok_b")
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        A, B = _derive(a, ok_a), _derive(b, ok_b)
        usable, inter, iou = _iou_of_records(A, B)
        delta = B["c"] - A["c"]
        diff = a - b
        corner = np.zeros(n)
        for k in range(8):
            corner = corner + np.sqrt(_dot3(diff[:, k], diff[:, k]))
        la, lb = np.sqrt(_dot3(A["e"], A["e"])), np.sqrt(_dot3(B["e"], B["e"]))                # [n, 3]
        dots = _dot3(A["e"] / la[:, :, None], B["e"] / lb[:, :, None])
        angle = _acos_deg(dots)
        out = {"iou": iou, "inter_volume": inter, "volume_a": A["vol"], "volume_b": B["vol"], "center_dist": np.sqrt(_dot3(delta, delta)),
               "center_delta": delta, "corner_dist": corner / 8.0, "extent_a": la, "extent_b": lb, "axis_angle_deg": angle,
               "axis_fold_deg": np.fmin(angle, 180.0 - angle), "rot_deg": _acos_deg((((dots[:, 0] + dots[:, 1]) + dots[:, 2]) - 1.0) / 2.0)}
    out = {k: np.where(usable.reshape((n,) + (1,) * (v.ndim - 1)), v, np.nan) for k, v in out.items()}
    return {"valid": usable.astype(np.int32), **out}


def box_iou_matrix_ref(a, b=None, ok_a=None, ok_b=None):
    """float64 numpy twin of `box_iou_matrix`: [n, P, Q] float64."""
    a = np.asarray(a, dtype=np.float64)
    if b is None:
        b, ok_b = a, ok_a
    b = np.asarray(b, dtype=np.float64)
    n, P, Q = _matrix_shapes("box_iou_matrix_ref", a.shape, b.shape)
    ok_a, ok_b = _check_ok(ok_a, (n, P), "box_iou_matrix_ref: ok_a"), _check_ok(ok_b, (n, Q), "box_iou_matrix_ref: ok_b")
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        A, B = _derive(a.reshape(n * P, 8, 3), ok_a.reshape(n * P)), _derive(b.reshape(n * Q, 8, 3), ok_b.reshape(n * Q))
        pose, p, q = np.meshgrid(np.arange(n), np.arange(P), np.arange(Q), indexing="ij")
        return _iou_of_records(_take(A, (pose * P + p).reshape(-1)), _take(B, (pose * Q + q).reshape(-1)))[2].reshape(n, P, Q)


# ------------------------------------------------------------------------------------------------------------------ estimator results
def _is_numpy(r, keys):
    return not any(isinstance(r[k], torch.Tensor) for k in keys)


def cloud_pose_agreement(r, ref: bool = False) -> dict:
    """r: the dict of `estimate_cloud_pose` / `estimate_cloud_pose_device` (or of `estimate_cloud_views(fit=True)`) -> `box_agreement`
    of the network's box `bbox` (ok: `valid`) and the box fitted to the cloud `bbox_cloud` (ok: `valid_cloud`).  A dict of numpy arrays
    gives numpy arrays, one of CUDA tensors CUDA tensors; `ref`: the numpy twin instead of the kernel (numpy in and out)."""
    keys = ("bbox", "bbox_cloud", "valid", "valid_cloud")
    for k in keys:
        if k not in r:
            raise ValueError(f"cloud_pose_agreement: the result holds no `{k}`")
    if ref:
        return box_agreement_ref(*[_to_numpy(r[k]) for k in keys])
    out = box_agreement(r["bbox"], r["bbox_cloud"], ok_a=r["valid"], ok_b=r["valid_cloud"])
    return {k: v.cpu().numpy() for k, v in out.items()} if _is_numpy(r, keys) else out


def _to_numpy(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _pair_summary(iou, ok, xp):
    """iou [n, S, S], ok [n, S] bool -> (mean, min) [n] over the off-diagonal pairs of usable samples: every row summed over t
    ascending, then the rows over s ascending; NaN with fewer than 2 usable samples.  A sample that `ok` lets through but the box
    model refuses (finite corners without volume) has NaN in `iou` and is no more usable than the others: a pair counts only where its
    IoU is a number.  xp: numpy or torch."""
    n, S = ok.shape
    eye = xp.eye(S, dtype=bool) if xp is np else torch.eye(S, dtype=torch.bool, device=ok.device)
    use = ok[:, :, None] & ok[:, None, :] & ~eye & ~xp.isnan(iou)
    zero = xp.zeros_like(iou[:, :, 0])
    row = zero
    for t in range(S):
        row = row + xp.where(use[:, :, t], iou[:, :, t], zero)
    total = xp.zeros_like(iou[:, 0, 0])
    for s in range(S):
        total = total + row[:, s]
    pairs = use.sum(1).sum(1)
    inf = xp.full_like(iou, float("inf"))
    low = xp.where(use, iou, inf)
    low = low.reshape(n, S * S).min(1) if xp is np else low.reshape(n, S * S).min(dim=1).values
    nan = xp.full_like(total, float("nan"))
    some = pairs > 0
    if xp is np:
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(some, total / pairs, nan), np.where(some, low, nan)
    return torch.where(some, total / pairs.to(total.dtype), nan), torch.where(some, low, nan)


def samples_overlap(r, ref: bool = False) -> dict:
    """r: the dict of `estimate_samples` / `estimate_samples_device` -> how far the S draws of a pose overlap: `iou_pairs` [n,S,S]
    (`box_iou_matrix` of `bbox_samples` with itself), `iou_to_mean` [n,S] (every sample against the mean box `bbox`, ok: `valid`),
    `iou_mean` / `iou_min` [n] over the off-diagonal pairs of usable samples in a fixed order (NaN with fewer than 2).  A sample is
    usable when it is finite and is not DEFAULT_BBOX, the condition `estimate_samples` counts with; one that has no volume besides
    is NaN in `iou_pairs` and `iou_to_mean` and stays out of `iou_mean` / `iou_min`.  numpy in, numpy out; CUDA in, CUDA out; `ref`: the numpy twins instead of the kernels (numpy in and out)."""
    keys = ("bbox", "bbox_samples", "valid")
    for k in keys:
        if k not in r:
            raise ValueError(f"samples_overlap: the result holds no `{k}`")
    if ref:
        mean, box, valid = [_to_numpy(r[k]) for k in keys]
        box = np.asarray(box, dtype=np.float64)
        if box.ndim != 4 or box.shape[2:] != (8, 3):
            raise ValueError(f"samples_overlap: bbox_samples [n, S, 8, 3], got {box.shape}")
        n, S = box.shape[:2]
        ok = np.isfinite(box.reshape(n, S, 24)).all(axis=2) & ~(box == DEFAULT_BBOX).all(axis=3).all(axis=2)
        pairs = box_iou_matrix_ref(box, None, ok)
        to_mean = box_agreement_ref(box.reshape(n * S, 8, 3), np.repeat(np.asarray(mean, dtype=np.float64), S, axis=0), ok.reshape(n * S),
                                    np.repeat(np.asarray(valid) != 0, S))["iou"].reshape(n, S)
        m, low = _pair_summary(pairs, ok, np)
        return {"iou_pairs": pairs, "iou_to_mean": to_mean, "iou_mean": m, "iou_min": low}
    box = torch.as_tensor(r["bbox_samples"])
    dev = _device_of(box)
    box = box.to(device=dev, dtype=torch.float64).contiguous()
    if box.dim() != 4 or tuple(box.shape[2:]) != (8, 3):
        raise ValueError(f"samples_overlap: bbox_samples [n, S, 8, 3], got {tuple(box.shape)}")
    n, S = int(box.shape[0]), int(box.shape[1])
    mean = torch.as_tensor(r["bbox"]).to(device=dev, dtype=torch.float64)
    valid = torch.as_tensor(r["valid"]).to(device=dev) != 0
    dflt = torch.from_numpy(DEFAULT_BBOX).to(dev)
    ok = torch.isfinite(box.reshape(n, S, 24)).all(dim=2) & ~(box == dflt).all(dim=3).all(dim=2)
    pairs = box_iou_matrix(box, None, ok)
    to_mean = box_agreement(box.reshape(n * S, 8, 3), mean.repeat_interleave(S, dim=0), ok.reshape(n * S), valid.repeat_interleave(S))["iou"]
    m, low = _pair_summary(pairs, ok, torch)
    out = {"iou_pairs": pairs, "iou_to_mean": to_mean.reshape(n, S), "iou_mean": m, "iou_min": low}
    return {k: v.cpu().numpy() for k, v in out.items()} if _is_numpy(r, keys) else out
