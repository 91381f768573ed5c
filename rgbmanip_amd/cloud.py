"""Dense geometry behind the depth maps (DESIGN.md sections 5k / 5l / 5n): back-projection, the two-view consistency check, V-view
fusion, the packed point cloud, gathers at its indices and the similarity fit — host wrappers of the HIP kernels (the C ABI in
include/rgbm.h), each beside its float64 numpy twin (tests, documentation).  PyTorch is used only for device memory and streams."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

DEFAULT_BBOX = np.asarray([[0, 0, 0], [0, 0, 1], [0, 1, 0], [0, 1, 1], [1, 0, 0], [1, 0, 1], [1, 1, 0], [1, 1, 1]], dtype=np.float64) + 10.0
_BBOX_SIGNS = np.asarray([[1, 1, 1], [1, 1, -1], [-1, 1, 1], [-1, 1, -1], [1, -1, 1], [1, -1, -1], [-1, -1, 1], [-1, -1, -1]], dtype=np.float64)


# ------------------------------------------------------------------ argument plumbing of every wrapper below
def _device(*xs):
    """The device of the first CUDA tensor among xs, else the current device."""
    return next((x.device for x in xs if isinstance(x, torch.Tensor) and x.is_cuda), None) or torch.device("cuda", torch.cuda.current_device())


def _maps(x, dev, what, ranks=(), square=False, like=None):
    """x as a contiguous float32 tensor on dev, of one of `ranks` (`square`: S x S in its last two dimensions) or of the shape of `like`."""
    t = torch.as_tensor(x).to(device=dev, dtype=torch.float32).contiguous()
    if (ranks and t.dim() not in ranks) or (square and t.dim() >= 2 and t.shape[-1] != t.shape[-2]):
        raise ValueError(f"{what}, got {tuple(t.shape)}")
    if like is not None and t.shape != like.shape:
        raise ValueError(f"{what} has the maps' shape, got {tuple(t.shape)} and {tuple(like.shape)}")
    return t


def _cameras(Kcrop, E, dev, lead, what):
    """Kcrop lead + [3, 3] and E lead + [4, 4] as contiguous float64 tensors on dev."""
    K = torch.as_tensor(Kcrop).to(device=dev, dtype=torch.float64).contiguous()
    Ed = torch.as_tensor(E).to(device=dev, dtype=torch.float64).contiguous()
    if tuple(K.shape) != lead + (3, 3) or tuple(Ed.shape) != lead + (4, 4):
        raise ValueError(f"{what}: Kcrop {list(lead + (3, 3))} and E {list(lead + (4, 4))}, got {tuple(K.shape)} and {tuple(Ed.shape)}")
    return K, Ed


def _bytes(x, dev, like, what):
    """A mask or keep map as contiguous uint8 on dev (a uint8 tensor as it is: the kernels test for non-zero), of the shape of `like`."""
    x = torch.as_tensor(x).to(device=dev)
    x = (x if x.dtype == torch.uint8 else (x != 0).to(torch.uint8)).contiguous()
    if x.shape != like.shape:
        raise ValueError(f"{what} has the maps' shape, got {tuple(x.shape)} and {tuple(like.shape)}")
    return x


def _cap(max_points, worst, name):
    cap = worst if max_points is None else int(max_points)
    if cap < 0:
        raise ValueError(f"{name}: max_points >= 0, got {max_points}")
    return cap


def depth_to_points(depth_map, K_crop, E, stream=None):
    """World-frame points of a crop's depth map (rgbm_depth_to_points): depth_map [n,S,S] float32, K_crop [n,3,3] (cropped intrinsics),
    E [n,4,4] (world -> camera) -> [n,S,S,3] float32 CUDA: inv(E) applied to the back-projection of interface_v5.py:329-336 at every
    pixel — the per-pixel `Position` image of the simulator camera.  A pixel whose depth is not finite yields NaN."""
    lib = _lib.load()
    dev = _device(depth_map)
    d = _maps(depth_map, dev, "depth_to_points: depth_map [n, S, S]", ranks=(3,), square=True)
    n, S = d.shape[0], d.shape[1]
    K, Ed = _cameras(K_crop, E, dev, (n,), "depth_to_points")
    pts = torch.empty(n, S, S, 3, dtype=torch.float32, device=dev)
    if n:
        _lib.check(lib.rgbm_depth_to_points(_lib.ptr(d), _lib.ptr(K), _lib.ptr(Ed), n, S, _lib.ptr(pts), _lib.stream_ptr(stream)),
                   "rgbm_depth_to_points")
    return pts


def depth_to_points_ref(depth_map, K_crop, E):
    """float64 numpy twin of `depth_to_points` (tests, documentation): the arithmetic of interface_v5.py:329-336, 369-372 per pixel."""
    d = np.asarray(depth_map, dtype=np.float64)
    K, E = np.asarray(K_crop, dtype=np.float64), np.asarray(E, dtype=np.float64)
    n, S = d.shape[0], d.shape[1]
    y, x = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64), indexing="ij")
    out = np.empty((n, S, S, 3))
    for i in range(n):
        ex_inv = np.linalg.inv(E[i])
        with np.errstate(invalid="ignore"):                   # a non-finite depth: NaN below
            cam = np.stack([(x - K[i, 0, 2]) * d[i] / K[i, 0, 0], (y - K[i, 1, 2]) * d[i] / K[i, 1, 1], d[i]], axis=-1)
            out[i] = cam @ ex_inv[:3, :3].T + ex_inv[:3, 3]
        out[i][~np.isfinite(d[i])] = np.nan
    return out


def depth_consistency(depth_a, Kcrop_a, E_a, depth_b, Kcrop_b, E_b, conf_a=None, mask_a=None, px_max: float = 1.0, rel_max: float = 0.01,
                      conf_min: float = 0.0, stream=None, want_diagnostics: bool = True):
    """Two-view geometric consistency of view a's depth map against view b's (rgbm_depth_consistency): every pixel
    of depth_a [n,S,S] is back-projected, projected into view b, depth_b is sampled there bilinearly, back-projected and projected back
    into view a; the pixel is kept when it lands within `px_max` pixels of where it started at a depth within `rel_max` (relative), its
    confidence (conf_a [n,S,S], optional) is at least `conf_min` and its mask byte (mask_a [n,S,S], optional) is set.  Kcrop_* [n,3,3],
    E_* [n,4,4] world -> camera.  Returns a dict of CUDA tensors [n,S,S]: `fused` f32 (mean of the two depths where kept, NaN elsewhere),
    `reproj` f32 (pixels) and `rel` f32 (NaN where the pixel could not be sampled; None with want_diagnostics=False), `keep` uint8."""
    lib = _lib.load()
    dev = _device(depth_a, depth_b)
    da = _maps(depth_a, dev, "depth_consistency: depth_a [n, S, S]", ranks=(3,), square=True)
    db = _maps(depth_b, dev, "depth_consistency: depth_b", like=da)
    n, S = da.shape[0], da.shape[1]
    Ka, Ea = _cameras(Kcrop_a, E_a, dev, (n,), "depth_consistency, view a")
    Kb, Eb = _cameras(Kcrop_b, E_b, dev, (n,), "depth_consistency, view b")
    conf = None if conf_a is None else _maps(conf_a, dev, "depth_consistency: conf_a", like=da)
    mask = None if mask_a is None else _bytes(mask_a, dev, da, "depth_consistency: mask_a")
    fused = torch.empty(n, S, S, dtype=torch.float32, device=dev)
    reproj, rel = (torch.empty_like(fused), torch.empty_like(fused)) if want_diagnostics else (None, None)
    keep = torch.empty(n, S, S, dtype=torch.uint8, device=dev)
    if n:
        _lib.check(lib.rgbm_depth_consistency(_lib.ptr(da), _lib.ptr(conf), _lib.ptr(mask), _lib.ptr(Ka), _lib.ptr(Ea), _lib.ptr(db), _lib.ptr(Kb),
                                              _lib.ptr(Eb), n, S, float(px_max), float(rel_max), float(conf_min), _lib.ptr(fused),
                                              _lib.ptr(reproj), _lib.ptr(rel), _lib.ptr(keep), _lib.stream_ptr(stream)), "rgbm_depth_consistency")
    return {"fused": fused, "reproj": reproj, "rel": rel, "keep": keep}


def _consistency_pair_ref(d, Ka, Ea, inv_a, db, Kb, Eb, inv_b, xx, yy):
    """Rules 1-4 of DESIGN.md section 5k for one pose and one direction, in float64: view a's map d [S,S] against view b's db, inv_* the
    inverses of E_*.  Returns (ok, reproj, rel, dr): ok = the pixel passed rules 1-3 (the other three are numbers there), dr = d'.  The
    arithmetic `depth_consistency_ref` and `depth_fusion_ref` share."""
    S = d.shape[0]

    def back(inv, K, x, y, z):                             # pixel at depth z -> world
        cam = np.stack([(x - K[0, 2]) * z / K[0, 0], (y - K[1, 2]) * z / K[1, 1], z], axis=-1)
        return cam @ inv[:3, :3].T + inv[:3, 3]

    def project(E, K, X):                                  # world -> (u, v, z)
        c = X @ E[:3, :3].T + E[:3, 3]
        return K[0, 0] * c[..., 0] / c[..., 2] + K[0, 2], K[1, 1] * c[..., 1] / c[..., 2] + K[1, 2], c[..., 2]

    with np.errstate(all="ignore"):
        ok = np.isfinite(d) & (d > 0)                                                                   # rule 1
        dz = np.where(ok, d, 1.0)
        u, v, z = project(Eb, Kb, back(inv_a, Ka, xx, yy, dz))
        ok &= (z > 0) & (u >= 0) & (u <= S - 1) & (v >= 0) & (v <= S - 1)                               # rule 2
        us, vs = np.where(ok, u, 0.0), np.where(ok, v, 0.0)
        x0, y0 = np.floor(us).astype(np.int64), np.floor(vs).astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, S - 1), np.minimum(y0 + 1, S - 1)
        t00, t01, t10, t11 = db[y0, x0], db[y0, x1], db[y1, x0], db[y1, x1]
        for t in (t00, t01, t10, t11):
            ok &= np.isfinite(t) & (t > 0)                                                              # rule 3
        ax, ay = us - x0, vs - y0
        samp = (t00 * (1 - ax) + t01 * ax) * (1 - ay) + (t10 * (1 - ax) + t11 * ax) * ay
        xr, yr, dr = project(Ea, Ka, back(inv_b, Kb, us, vs, samp))                                    # rule 4
        reproj, rel = np.hypot(xr - xx, yr - yy), np.abs(dr - d) / d
    return ok, reproj, rel, dr


def _finite_inverse(E):
    """inv(E), or None where E has no finite inverse."""
    try:
        inv = np.linalg.inv(E)
    except np.linalg.LinAlgError:
        return None
    return inv if np.isfinite(inv).all() else None


def depth_consistency_ref(depth_a, Kcrop_a, E_a, depth_b, Kcrop_b, E_b, conf_a=None, mask_a=None, px_max: float = 1.0, rel_max: float = 0.01,
                          conf_min: float = 0.0):
    """float64 numpy twin of `depth_consistency` (tests, documentation): rules 1-5 of DESIGN.md section 5k.  Returns dict(fused, reproj,
    rel [n,S,S] float64, keep [n,S,S] bool).  Also returns `sampled` (bool: the pixel passed rules 1-3, i.e. reproj / rel are numbers)."""
    da, db = np.asarray(depth_a, dtype=np.float64), np.asarray(depth_b, dtype=np.float64)
    Ka, Kb = np.asarray(Kcrop_a, dtype=np.float64), np.asarray(Kcrop_b, dtype=np.float64)
    Ea, Eb = np.asarray(E_a, dtype=np.float64), np.asarray(E_b, dtype=np.float64)
    n, S = da.shape[0], da.shape[1]
    yy, xx = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64), indexing="ij")
    out = {k: np.full((n, S, S), np.nan) for k in ("fused", "reproj", "rel")}
    out["keep"] = np.zeros((n, S, S), dtype=bool)
    out["sampled"] = np.zeros((n, S, S), dtype=bool)
    for i in range(n):
        inv_a, inv_b = _finite_inverse(Ea[i]), _finite_inverse(Eb[i])
        if inv_a is None or inv_b is None:
            continue
        d = da[i]
        ok, reproj, rel, dr = _consistency_pair_ref(d, Ka[i], Ea[i], inv_a, db[i], Kb[i], Eb[i], inv_b, xx, yy)
        with np.errstate(all="ignore"):
            keep = ok & (reproj < px_max) & (rel < rel_max)                                             # rule 5
            if conf_a is not None:
                keep &= np.asarray(conf_a[i], dtype=np.float32) >= np.float32(conf_min)
            if mask_a is not None:
                keep &= np.asarray(mask_a[i]) != 0
        out["reproj"][i][ok], out["rel"][i][ok] = reproj[ok], rel[ok]
        with np.errstate(all="ignore"):
            out["fused"][i][keep] = ((d + dr) / 2)[keep]
        out["keep"][i], out["sampled"][i] = keep, ok
    return out


def depth_fusion(depth, Kcrop, E, conf=None, mask=None, px_max: float = 1.0, rel_max: float = 0.01, conf_min: float = 0.0, n_min: int = 1,
                 stream=None, want_agree: bool = True):
    """Multi-view fusion of the V depth maps of every pose (rgbm_depth_fusion): every pixel of every view of depth
    [n,V,S,S] is checked against each of the other V - 1 views with the arithmetic of `depth_consistency`; a source agrees when the pixel
    comes back within `px_max` pixels at a depth within `rel_max` (relative).  A pixel is kept when at least `n_min` sources agree, its
    confidence (conf [n,V,S,S], optional) is at least `conf_min` and its mask byte (mask [n,V,S,S], optional) is set; its fused depth is
    the mean of its own depth and the agreeing sources' depths.  Kcrop [n,V,3,3], E [n,V,4,4] world -> camera; 2 <= V <= 16, 1 <= n_min
    <= V - 1.  Returns a dict of CUDA tensors [n,V,S,S]: `fused` f32 (NaN where not kept), `keep` uint8, `nviews` uint8 (agreeing sources,
    whatever `keep` says) and `agree` int16 (the bit set of the agreeing views: bit b = view b; None with want_agree=False).  At V = 2,
    n_min = 1 `fused` / `keep` are the bits of the two directions of `depth_consistency`."""
    lib = _lib.load()
    dev = _device(depth)
    d = _maps(depth, dev, "depth_fusion: maps [n, V, S, S]", ranks=(4,), square=True)
    n, V, S = int(d.shape[0]), int(d.shape[1]), int(d.shape[2])
    K, Ed = _cameras(Kcrop, E, dev, (n, V), "depth_fusion")
    c = None if conf is None else _maps(conf, dev, "depth_fusion: conf", like=d)
    m = None if mask is None else _bytes(mask, dev, d, "depth_fusion: mask")
    fused = torch.empty(n, V, S, S, dtype=torch.float32, device=dev)
    keep = torch.empty(n, V, S, S, dtype=torch.uint8, device=dev)
    nviews = torch.empty(n, V, S, S, dtype=torch.uint8, device=dev)
    agree = torch.empty(n, V, S, S, dtype=torch.int16, device=dev) if want_agree else None      # 16 bits, V <= 16: bit 15 is the sign
    if n:
        _lib.check(lib.rgbm_depth_fusion(_lib.ptr(d), _lib.ptr(c), _lib.ptr(m), _lib.ptr(K), _lib.ptr(Ed), n, V, S, float(px_max), float(rel_max),
                                         float(conf_min), int(n_min), _lib.ptr(fused), _lib.ptr(keep), _lib.ptr(nviews), _lib.ptr(agree),
                                         _lib.stream_ptr(stream)), "rgbm_depth_fusion")
    return {"fused": fused, "keep": keep, "nviews": nviews, "agree": agree}


def depth_fusion_ref(depth, Kcrop, E, conf=None, mask=None, px_max: float = 1.0, rel_max: float = 0.01, conf_min: float = 0.0, n_min: int = 1):
    """float64 numpy twin of `depth_fusion` (tests, documentation): rules 0-3 of DESIGN.md section 5n on the per-source arithmetic of
    `depth_consistency_ref`.  Returns dict(fused [n,V,S,S] float64, keep bool, nviews uint8, agree uint16) and `margin` [n,V,V,S,S,2]
    float64: margin[i, a, b, y, x] = (|reproj - px_max| in pixels, |rel - rel_max|) of pixel (x, y) of reference view a against source
    b, i.e. how far that pair's decision is from flipping; NaN where the pair was not sampled (rules 1-3 of section 5k, b = a, a view
    without a finite inverse).  Tests assert on it that no pair sits on a threshold."""
    dd = np.asarray(depth, dtype=np.float64)
    K, Ev = np.asarray(Kcrop, dtype=np.float64), np.asarray(E, dtype=np.float64)
    n, V, S = dd.shape[0], dd.shape[1], dd.shape[2]
    if not 2 <= V <= 16 or not 1 <= n_min <= V - 1:
        raise ValueError(f"depth_fusion_ref: 2 <= V <= 16 and 1 <= n_min <= V - 1, got V = {V}, n_min = {n_min}")
    yy, xx = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64), indexing="ij")
    out = {"fused": np.full((n, V, S, S), np.nan), "keep": np.zeros((n, V, S, S), dtype=bool), "nviews": np.zeros((n, V, S, S), dtype=np.uint8),
           "agree": np.zeros((n, V, S, S), dtype=np.uint16), "margin": np.full((n, V, V, S, S, 2), np.nan)}
    for i in range(n):
        inv = [_finite_inverse(Ev[i, v]) for v in range(V)]
        for a in range(V):
            if inv[a] is None:
                continue                                                                                # rule 0
            d = dd[i, a]
            total, c, bits = d.copy(), np.zeros((S, S), dtype=np.int64), np.zeros((S, S), dtype=np.uint16)
            for b in range(V):                                                                          # rule 1, in increasing b
                if b == a or inv[b] is None:
                    continue
                ok, reproj, rel, dr = _consistency_pair_ref(d, K[i, a], Ev[i, a], inv[a], dd[i, b], K[i, b], Ev[i, b], inv[b], xx, yy)
                with np.errstate(all="ignore"):
                    yes = ok & (reproj < px_max) & (rel < rel_max)
                    total = np.where(yes, total + dr, total)
                out["margin"][i, a, b][ok] = np.stack([np.abs(reproj - px_max), np.abs(rel - rel_max)], axis=-1)[ok]
                c += yes
                bits |= (yes.astype(np.uint16) << np.uint16(b))
            keep = c >= n_min                                                                           # rules 2, 3
            if conf is not None:
                keep &= np.asarray(conf[i][a], dtype=np.float32) >= np.float32(conf_min)
            if mask is not None:
                keep &= np.asarray(mask[i][a]) != 0
            with np.errstate(all="ignore"):
                out["fused"][i, a][keep] = (total / (1 + c))[keep]
            out["keep"][i, a], out["nviews"][i, a], out["agree"][i, a] = keep, c, bits
    return out


def cloud_pack_views(fused, keep, Kcrop, E, max_points=None, stream=None):
    """Packed world-frame point cloud of the kept pixels of V views (rgbm_cloud_pack_views): `cloud_pack` for fused
    / keep [n,V,S,S], Kcrop [n,V,3,3], E [n,V,4,4] — for pose i the kept pixels of view 0 in row-major order, then view 1's, and so on, each
    back-projected exactly as `depth_to_points` does.  Returns CUDA tensors (cloud [n,cap,3] f32, index [n,cap] i32 = view * S * S +
    pixel, count [n,V] i32 = pixels kept per view, whatever cap is); rows past the kept pixels hold NaN / -1.  cap = max_points, default
    the worst case V S S.  1 <= V <= 16.  At V = 2 (V = 1) the outputs are byte for byte those of `cloud_pack` (of its one-view form)."""
    lib = _lib.load()
    dev = _device(fused)
    f = _maps(fused, dev, "cloud_pack_views: maps [n, V, S, S]", ranks=(4,), square=True)
    n, V, S = int(f.shape[0]), int(f.shape[1]), int(f.shape[2])
    K, Ed = _cameras(Kcrop, E, dev, (n, V), "cloud_pack_views")
    k = _bytes(keep, dev, f, "cloud_pack_views: keep")
    cap = _cap(max_points, V * S * S, "cloud_pack_views")
    cloud = torch.empty(n, cap, 3, dtype=torch.float32, device=dev)
    index = torch.empty(n, cap, dtype=torch.int32, device=dev)
    count = torch.empty(n, V, dtype=torch.int32, device=dev)
    if n:
        _lib.check(lib.rgbm_cloud_pack_views(_lib.ptr(f), _lib.ptr(k), _lib.ptr(K), _lib.ptr(Ed), n, V, S, cap, _lib.ptr(cloud), _lib.ptr(index),
                                             _lib.ptr(count), _lib.stream_ptr(stream)), "rgbm_cloud_pack_views")
    return cloud, index, count


def cloud_pack(fused1, keep1, Kcrop1, E1, fused2=None, keep2=None, Kcrop2=None, E2=None, max_points=None, stream=None):
    """Packed world-frame point cloud of the kept pixels (rgbm_cloud_pack): for pose i the pixels of view 1 with
    keep1 != 0 in row-major order, then those of view 2 (all four view-2 arguments, or none for a one-view cloud), each back-projected
    exactly as `depth_to_points` does.  Returns CUDA tensors (cloud [n,cap,3] f32, index [n,cap] i32 = view * S * S + pixel, count [n,2]
    i32 = pixels kept per view, whatever cap is); rows past the kept pixels hold NaN / -1.  cap = max_points, default the worst case
    (2 S S, or S S for one view).  The order is fixed: two calls give the same bytes."""
    lib = _lib.load()
    two = [x is not None for x in (fused2, keep2, Kcrop2, E2)]
    if any(two) != all(two):
        raise ValueError("cloud_pack: fused2, keep2, Kcrop2 and E2 are given together or not at all")
    dev = _device(fused1, fused2)
    f1 = _maps(fused1, dev, "cloud_pack: fused1 [n, S, S]", ranks=(3,), square=True)
    n, S = f1.shape[0], f1.shape[1]
    K1, E1d = _cameras(Kcrop1, E1, dev, (n,), "cloud_pack, view 1")
    k1 = _bytes(keep1, dev, f1, "cloud_pack: keep1")
    f2 = K2 = E2d = k2 = None
    if all(two):
        f2 = _maps(fused2, dev, "cloud_pack: fused2", like=f1)
        K2, E2d = _cameras(Kcrop2, E2, dev, (n,), "cloud_pack, view 2")
        k2 = _bytes(keep2, dev, f1, "cloud_pack: keep2")
    cap = _cap(max_points, (2 if all(two) else 1) * S * S, "cloud_pack")
    cloud = torch.empty(n, cap, 3, dtype=torch.float32, device=dev)
    index = torch.empty(n, cap, dtype=torch.int32, device=dev)
    count = torch.empty(n, 2, dtype=torch.int32, device=dev)
    if n:
        _lib.check(lib.rgbm_cloud_pack(_lib.ptr(f1), _lib.ptr(k1), _lib.ptr(K1), _lib.ptr(E1d), _lib.ptr(f2), _lib.ptr(k2), _lib.ptr(K2),
                                       _lib.ptr(E2d), n, S, cap, _lib.ptr(cloud), _lib.ptr(index), _lib.ptr(count), _lib.stream_ptr(stream)),
                   "rgbm_cloud_pack")
    return cloud, index, count


def _gather_args(index, dev, n, Cc, name):
    """index [n, cap] as contiguous int32 on dev, cap, and the uninitialised [n, cap, Cc] float32 result."""
    ix = torch.as_tensor(index).to(device=dev, dtype=torch.int32).contiguous()
    if ix.dim() != 2 or ix.shape[0] != n:
        raise ValueError(f"{name}: index [n, cap], got {tuple(ix.shape)} for n = {n}")
    return ix, int(ix.shape[1]), torch.empty(n, int(ix.shape[1]), Cc, dtype=torch.float32, device=dev)


def cloud_gather(map1, map2, index, stream=None):
    """Rows of per-pixel maps at a packed cloud's indices (rgbm_cloud_gather): map1 / map2 [n, S2, C] or [n, S, S, C] float32 (map2 may
    be None), index [n, cap] int32 as `cloud_pack` returns it -> [n, cap, C] float32 CUDA, out[i, r] = map{1 + index // S2}[i, index % S2].
    Rows with index < 0, index >= 2 S2, or a view-2 index without map2 hold NaN.  1 <= C <= 4."""
    lib = _lib.load()
    dev = _device(map1, map2, index)
    m1 = _maps(map1, dev, "cloud_gather: map1 [n, S2, C] or [n, S, S, C]", ranks=(3, 4))
    n, Cc = int(m1.shape[0]), int(m1.shape[-1])
    S2 = int(m1.shape[1]) if m1.dim() == 3 else int(m1.shape[1] * m1.shape[2])
    if not 1 <= Cc <= 4 or S2 < 1:
        raise ValueError(f"cloud_gather: 1 <= C <= 4 and S2 >= 1, got C = {Cc}, S2 = {S2}")
    m2 = None if map2 is None else _maps(map2, dev, "cloud_gather: map2", like=m1)
    ix, cap, out = _gather_args(index, dev, n, Cc, "cloud_gather")
    if n and cap:
        _lib.check(lib.rgbm_cloud_gather(_lib.ptr(m1), _lib.ptr(m2), _lib.ptr(ix), n, S2, Cc, cap, _lib.ptr(out), _lib.stream_ptr(stream)),
                   "rgbm_cloud_gather")
    return out


def cloud_gather_views(maps, index, stream=None):
    """Rows of the per-pixel maps of V views at a packed cloud's indices (rgbm_cloud_gather_views): maps [n, V, S2, C] or [n, V, S, S, C]
    float32, index [n, cap] int32 as `cloud_pack_views` returns it -> [n, cap, C] float32 CUDA, out[i, r] = maps[i, index // S2, index %
    S2].  Rows with an index outside [0, V S2) hold NaN.  1 <= V <= 16, 1 <= C <= 4."""
    lib = _lib.load()
    dev = _device(maps, index)
    m = _maps(maps, dev, "cloud_gather_views: maps [n, V, S2, C] or [n, V, S, S, C]", ranks=(4, 5))
    n, V, Cc = int(m.shape[0]), int(m.shape[1]), int(m.shape[-1])
    S2 = int(m.shape[2]) if m.dim() == 4 else int(m.shape[2] * m.shape[3])
    if not 1 <= Cc <= 4 or S2 < 1 or not 1 <= V <= 16:
        raise ValueError(f"cloud_gather_views: 1 <= C <= 4, S2 >= 1 and 1 <= V <= 16, got C = {Cc}, S2 = {S2}, V = {V}")
    ix, cap, out = _gather_args(index, dev, n, Cc, "cloud_gather_views")
    if n and cap:
        _lib.check(lib.rgbm_cloud_gather_views(_lib.ptr(m), _lib.ptr(ix), n, V, S2, Cc, cap, _lib.ptr(out), _lib.stream_ptr(stream)),
                   "rgbm_cloud_gather_views")
    return out


def _fit_shapes(nocs, cloud, count):
    if nocs.ndim != 3 or nocs.shape[2] != 3 or tuple(cloud.shape) != tuple(nocs.shape):
        raise ValueError(f"cloud_similarity: nocs and cloud [n, cap, 3], got {tuple(nocs.shape)} and {tuple(cloud.shape)}")
    if tuple(count.shape) != (nocs.shape[0], 2):
        raise ValueError(f"cloud_similarity: count [n, 2], got {tuple(count.shape)}")
    return int(nocs.shape[0]), int(nocs.shape[1])


def cloud_similarity(nocs, cloud, count, seed: int = 0, stream=None):
    """The reference's similarity RANSAC (lib/align.py:10-104) between a packed cloud's object-space rows nocs [n, cap, 3] and its
    world-frame rows cloud [n, cap, 3] (rgbm_cloud_similarity): over the first m = min(cap, count.sum(1)) rows of
    pose b, 128 five-point hypotheses drawn by the seeded hash (sample k of hypothesis i = mix32(seed, 128 b + i, k) % m), the reference's
    scan and the final Umeyama fit over the kept hypothesis's inliers, then the box of `bbox_from_srt` without a world transform.  Returns
    CUDA tensors (bbox [n,8,3] f64, srt [n,13] f64 = scale, R, t, info [n,4] i32 = m, kept hypothesis or -1, its inliers, hypotheses
    examined, valid [n] i32).  m < 5, a NaN row, no consensus: valid 0, the +10 cube, srt[:, 0] NaN.  Two calls give the same bytes."""
    lib = _lib.load()
    dev = _device(nocs, cloud, count)
    nc, cl = _maps(nocs, dev, "cloud_similarity: nocs"), _maps(cloud, dev, "cloud_similarity: cloud")
    ct = torch.as_tensor(count).to(device=dev, dtype=torch.int32).contiguous()
    n, cap = _fit_shapes(nc, cl, ct)
    bbox = torch.from_numpy(DEFAULT_BBOX).to(dev).expand(n, 8, 3).contiguous()
    srt = torch.zeros(n, 13, dtype=torch.float64, device=dev)
    info = torch.zeros(n, 4, dtype=torch.int32, device=dev)
    valid = torch.zeros(n, dtype=torch.int32, device=dev)
    if n and cap:
        nb = C.c_size_t()
        _lib.check(lib.rgbm_cloud_similarity_scratch_bytes(n, cap, C.byref(nb)), "rgbm_cloud_similarity_scratch_bytes")
        scratch = torch.empty(max(nb.value // 8, 1), dtype=torch.int64, device=dev)
        if stream is not None:
            scratch.record_stream(stream)
        _lib.check(lib.rgbm_cloud_similarity(_lib.ptr(nc), _lib.ptr(cl), _lib.ptr(ct), n, cap, int(seed) & 0xFFFFFFFF, _lib.ptr(bbox), _lib.ptr(srt),
                                             _lib.ptr(info), _lib.ptr(valid), _lib.ptr(scratch), nb.value, _lib.stream_ptr(stream)),
                   "rgbm_cloud_similarity")
    elif n:                                                   # no rows at all: every pose is invalid
        srt[:, 0] = float("nan")
        srt[:, 1] = srt[:, 5] = srt[:, 9] = 1.0
        info[:, 1] = -1
    return bbox, srt, info, valid


def _mix32(seed: int, frame: int, idx: int) -> int:
    M = 0xFFFFFFFF
    h = (seed ^ ((frame * 0x9E3779B9) & M) ^ ((idx * 0x85EBCA6B) & M)) & M
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M
    h ^= h >> 16
    return h


def _umeyama_ref(src, tgt):
    """lib/align.py:10-41 on rows src / tgt [k, 3] float64 -> (scale, R, t)."""
    ms, mt = src.mean(axis=0), tgt.mean(axis=0)
    cs, ct = src - ms, tgt - mt
    cov = ct.T @ cs / src.shape[0]
    if np.isnan(cov).any():
        raise RuntimeError("NaN covariance")
    U, D, Vh = np.linalg.svd(cov, full_matrices=True)
    if np.linalg.det(U) * np.linalg.det(Vh) < 0.0:
        D[-1] = -D[-1]
        U[:, -1] = -U[:, -1]
    R = U @ Vh
    with np.errstate(all="ignore"):
        scale = 1 / np.var(src, axis=0).sum() * np.sum(D)
    return scale, R, mt - ms.dot(scale * R.T)


def cloud_similarity_ref(nocs, cloud, count, seed: int = 0):
    """float64 numpy twin of `cloud_similarity` (tests, documentation): the semantics of include/rgbm.h restated per pose.  Returns numpy
    arrays (bbox [n,8,3] f64, srt [n,13] f64, info [n,4] i32, valid [n] i32)."""
    nocs, cloud, count = np.asarray(nocs, dtype=np.float32), np.asarray(cloud, dtype=np.float32), np.asarray(count)
    n, cap = _fit_shapes(nocs, cloud, count)
    bbox = np.tile(DEFAULT_BBOX, (n, 1, 1))
    srt = np.zeros((n, 13))
    srt[:, 0], srt[:, 1], srt[:, 5], srt[:, 9] = np.nan, 1.0, 1.0, 1.0
    info, valid = np.zeros((n, 4), dtype=np.int32), np.zeros(n, dtype=np.int32)
    seed = int(seed) & 0xFFFFFFFF
    for b in range(n):
        m = int(min(cap, max(0, int(count[b, 0]) + int(count[b, 1]))))
        info[b] = (m, -1, 0, 0)
        s, t = nocs[b, :m].astype(np.float64), cloud[b, :m].astype(np.float64)
        if m < 5 or np.isnan(s).any() or np.isnan(t).any():
            continue
        thr = 2 * np.sqrt(((s - s.mean(axis=0)) ** 2).sum(axis=1)).max() / 10.0
        best, best_h, best_inl, examined, failed = 0.0, -1, None, 0, False
        for i in range(128):
            idx = [_mix32(seed, 128 * b + i, k) % m for k in range(5)]
            try:
                sc, R, tr = _umeyama_ref(s[idx], t[idx])
            except RuntimeError:
                failed = True
                break
            examined = i + 1
            with np.errstate(all="ignore"):
                inl = np.sqrt(((t - (s @ (sc * R).T + tr)) ** 2).sum(axis=1)) < sc * thr
            ratio = int(inl.sum()) / m
            if ratio > best:
                best, best_h, best_inl = ratio, i, inl
            b5 = (best * best) * (best * best) * best
            if (1 - (1 - b5) ** i) > 0.99:
                break
        if failed:
            continue
        if best < 0.1:
            info[b] = (m, -1, 0, examined)
            continue
        info[b] = (m, best_h, int(best_inl.sum()), examined)
        try:
            sc, R, tr = _umeyama_ref(s[best_inl], t[best_inl])
        except RuntimeError:
            continue
        srt[b, 1:10], srt[b, 10:13] = R.reshape(9), tr
        with np.errstate(all="ignore"):
            size = 2 * np.abs(s).max(axis=0) * sc
            corners = (_BBOX_SIGNS * (size[None, :] / 2)) @ R.astype(np.float32).astype(np.float64).T + tr.astype(np.float32).astype(np.float64)
        if np.isfinite(corners).all():
            bbox[b], srt[b, 0], valid[b] = corners, sc, 1
    return bbox, srt, info, valid
