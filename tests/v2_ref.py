"""CPU restatement of the v2 network (lib/network_v2.py:144-197), of its box tail (interface_v2.py:242-266) and of its
prepare_model_input (interface_v2.py:60-120), written from the formulas:

    fused_v[c, d, pix]  = feat_v[c, pix] + warped[c, d, pix]     warped = homo_warping of the partner view's feature map, zero padding per tap
    plane[d, pix]       = volume_conv(fused_v)                    three 1x1x1 Conv3d + eval BatchNorm + ReLU, 32 -> 16 -> 8 -> 1
    fuse[:, pix]        = fuse_conv(plane[:, pix])                1x1 Conv2d 24 -> 32, ReLU, 32 -> 64 (no ReLU behind the last)
    rows                = pose_mlp1(fuse gathered at choose)      64 -> 64 -> 64, ReLU each
    s                   = size_estimator(mean(pose_mlp2(cat(rows, mean(rows)))))
    nocs                = tanh(nocs_head(instance_color(feat gathered at choose)))       as in v5
    tail                : ts = ||view1_s|| (float32), EPnP-RANSAC + VVS on (nocs1 ts, pts2d of view 1, K): realworld_ref.pnp_scaled_bbox_world

Nothing between the feature map and the gather mixes pixels, so the stereo part is evaluated at the chosen pixels only - the project's
own kernel does the same; the reference materialises the whole volume.  torch, in the dtype of the state dict it is given (float32 or
float64).  The PSPNet and the MLP helpers come from oracle.adapose_ref.  Rows are point-major ([B, P, C]) here, as in the kernel."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import adapose_ref, postproc_ref
from realworld_ref import pnp_scaled_bbox_world, rel_err, to_sd      # noqa: F401  (re-exported: the tail and the helpers are shared)

OUT_KEYS = [f"view{v}_{k}" for v in (1, 2) for k in ("nocs", "s")]
TAP_KEYS = ("planes", "fuse", "rows")      # [B, P, 24], [B, P, 64], [B, P, 64] per view


def points_slice(t):
    """[B, P, C] -> [B, P / 8, C]: the points of the per-point tensors that tests/golden/adapose_v2_b2.npz stores (tools/make_goldens.py)"""
    return t[:, ::8]


def warp_grid_at(src_proj, ref_proj, depth_values, choose, H, W, dt):
    """The reference's sampling coordinates (network_v2.py:116-136) at the chosen pixels only: un-normalised (ix, iy) [B, D, P] as
    grid_sample (align_corners=False) reads them, and the normalised grid [B, D, P, 2]."""
    proj = torch.matmul(src_proj.to(dt), torch.inverse(ref_proj.to(dt)))
    rot, trans = proj[:, :3, :3], proj[:, :3, 3:4]
    choose = choose.long()
    x, y = (choose % W).to(dt), torch.div(choose, W, rounding_mode="floor").to(dt)
    xyz = torch.stack((x, y, torch.ones_like(x)), dim=1)                            # [B, 3, P]
    rot_xyz = torch.matmul(rot, xyz)
    B, D = depth_values.shape
    proj_xyz = rot_xyz.unsqueeze(2) * depth_values.to(dt).view(B, 1, D, 1) + trans.view(B, 3, 1, 1)
    proj_xy = proj_xyz[:, :2] / proj_xyz[:, 2:3]
    gx = proj_xy[:, 0] / ((W - 1) / 2) - 1
    gy = proj_xy[:, 1] / ((H - 1) / 2) - 1
    ix, iy = ((gx + 1) * W - 1) / 2, ((gy + 1) * H - 1) / 2
    return ix, iy, torch.stack((gx, gy), dim=3)


def taps_inside(ix, iy, H, W):
    """How many of the four bilinear taps of each (point, plane) lie inside the partner image: int64 [B, D, P]; 0 for a non-finite
    projection."""
    fin = torch.isfinite(ix) & torch.isfinite(iy)
    x0 = torch.floor(torch.where(fin, ix, torch.zeros_like(ix))).clamp(-4, 1e6).long()
    y0 = torch.floor(torch.where(fin, iy, torch.zeros_like(iy))).clamp(-4, 1e6).long()
    n = torch.zeros_like(x0)
    for dx in (0, 1):
        for dy in (0, 1):
            n += (((x0 + dx) >= 0) & ((x0 + dx) < W) & ((y0 + dy) >= 0) & ((y0 + dy) < H)).long()
    return torch.where(fin, n, torch.zeros_like(n))


def _conv_bn_relu(x, sd, p):
    """network_v2.py:26-32 with kernel size 1: conv (no bias) -> BatchNorm3d (running statistics) -> ReLU"""
    return F.relu(adapose_ref._bn(F.conv3d(x, sd[p + "conv.weight"]), sd, p + "bn."))


def stereo_rows(feat_v, feat_o, P_v, P_o, depth_values, choose, sd, stats=None):
    """planes [B, P, D], fuse [B, P, 64], rows [B, P, 64] of one view v with partner o.  stats (a dict) receives the ReLU clip shares
    and the share of (point, plane) pairs whose warp leaves the partner image."""
    dt = feat_v.dtype
    B, C, H, W = feat_v.shape
    D, P = depth_values.shape[1], choose.shape[1]
    choose = choose.long()
    ix, iy, grid = warp_grid_at(P_o, P_v, depth_values, choose, H, W, dt)
    warped = F.grid_sample(feat_o, grid, mode="bilinear", padding_mode="zeros", align_corners=False)      # [B, C, D, P]
    ref = torch.gather(feat_v.reshape(B, C, -1), 2, choose.unsqueeze(1).expand(B, C, P))
    x = (ref.unsqueeze(2) + warped).unsqueeze(-1)                                                       # [B, C, D, P, 1]
    clip = []
    for l in range(3):
        x = _conv_bn_relu(x, sd, f"volume_conv.{l}.")
        clip.append(float((x == 0).double().mean()))
    planes = x.reshape(B, D, P)
    h = F.relu(F.conv1d(planes, sd["fuse_conv.0.weight"].reshape(32, D, 1), sd["fuse_conv.0.bias"]))
    clip.append(float((h == 0).double().mean()))
    fuse = F.conv1d(h, sd["fuse_conv.2.weight"].reshape(64, 32, 1), sd["fuse_conv.2.bias"])
    rows = adapose_ref._mlp1d(fuse, sd, "pose_mlp1", (0, 2))
    if stats is not None:
        stats["clip"] = clip
        stats["outside"] = float((taps_inside(ix, iy, H, W) == 0).double().mean())
    return planes.transpose(1, 2).contiguous(), fuse.transpose(1, 2).contiguous(), rows.transpose(1, 2).contiguous()


def size_branch(rows, sd):
    """rows [B, P, 64] -> s [B, 3] (network_v2.py:184-188)"""
    f = rows.transpose(1, 2)
    f1 = torch.cat([f, f.mean(2, keepdim=True).expand_as(f)], 1)
    f2 = adapose_ref._mlp1d(f1, sd, "pose_mlp2", (0, 2)).mean(2)
    return adapose_ref._mlp(f2, sd, "size_estimator")


def nocs_branch(feat, choose, sd):
    B, C = feat.shape[:2]
    P = choose.shape[1]
    x = torch.gather(feat.reshape(B, C, -1), 2, choose.long().unsqueeze(1).expand(B, C, P))
    x = adapose_ref._mlp1d(x, sd, "instance_color", (0,))
    return torch.tanh(adapose_ref._mlp1d(x, sd, "nocs_head", (0, 2, 4), last_act=False)).permute(0, 2, 1).contiguous()


@torch.no_grad()
def heads_on_maps(sd, feat1, feat2, choose1, choose2, P1, P2, depths, taps=None, views=(1, 2)):
    """Everything behind the PSPNet on given feature maps [B, 32, H, W] (sd's dtype)."""
    dt = next(iter(sd.values())).dtype
    as_t = lambda a: torch.as_tensor(a)      # noqa: E731
    feat = {1: as_t(feat1).to(dt), 2: as_t(feat2).to(dt)}
    P = {1: as_t(P1), 2: as_t(P2)}
    choose = {1: as_t(choose1), 2: as_t(choose2)}
    dep = as_t(depths).to(dt)
    out = {}
    for v in views:
        o = 3 - v
        stats = {} if taps is not None else None
        planes, fuse, rows = stereo_rows(feat[v], feat[o], P[v], P[o], dep, choose[v], sd, stats)
        out[f"view{v}_nocs"] = nocs_branch(feat[v], choose[v], sd)
        out[f"view{v}_s"] = size_branch(rows, sd)
        if taps is not None:
            taps.update({f"v{v}_planes": planes, f"v{v}_fuse": fuse, f"v{v}_rows": rows, f"v{v}_clip": stats["clip"], f"v{v}_outside": stats["outside"]})
    return out


@torch.no_grad()
def v2_forward(sd, img1, choose1, img2, choose2, P1, P2, depths, taps=None, feat_round=None, views=(1, 2)):
    """Full forward in sd's dtype; the reference's argument order (network_v2.py:144).  taps: per view v1_ / v2_ the planes, fuse and rows
    tensors, the four ReLU clip shares and the outside share, plus feat1 / feat2.  feat_round: optional function applied to both feature
    maps before anything reads them (a round trip through a 16-bit storage type)."""
    dt = next(iter(sd.values())).dtype
    f1 = adapose_ref.pspnet(torch.as_tensor(img1).to(dt), sd)
    f2 = adapose_ref.pspnet(torch.as_tensor(img2).to(dt), sd)
    if feat_round is not None:
        f1, f2 = feat_round(f1), feat_round(f2)
    if taps is not None:
        taps["feat1"], taps["feat2"] = f1, f2
    return heads_on_maps(sd, f1, f2, choose1, choose2, P1, P2, depths, taps, views)


# ------------------------------------------------------------------------------------------------ interface_v2.py:60-120
def prepare_model_input(rgb, mask, K, size=224, n_pts=1024, seed=0, frame=0):
    """interface_v2.py:60-120 on oracle.postproc_ref: the crop window, the resized and normalised image and the cropped intrinsics are
    interface_v5's; the points are drawn from the mask at native resolution inside the window (the device path's seeded subset standing
    in for np.random.shuffle) and mapped into the crop afterwards.  Returns (view [3, S, S], choose [P] int64, pts2d [P, 2] int64,
    Kcrop, window) or five Nones for an empty mask."""
    ys, xs = np.nonzero(mask)
    if len(ys) == 0:
        return None, None, None, None, None
    rmin, rmax, cmin, cmax = postproc_ref.get_bbox([ys.min(), xs.min(), ys.max(), xs.max()])
    native = np.asarray(mask)[rmin:rmax, cmin:cmax].flatten().nonzero()[0]
    if len(native) > n_pts:
        native = postproc_ref.choose_subset_hash(native, n_pts, seed, frame)
    else:
        native = np.pad(native, (0, n_pts - len(native)), "wrap")
    crop_w = rmax - rmin
    ratio = size / crop_w
    col, row = native % crop_w, native // crop_w
    pts2d = np.stack((cmin + col, rmin + row), axis=-1)
    choose = (np.floor(row * ratio) * size + np.floor(col * ratio)).astype(np.int64)
    view, _, _, Kn = postproc_ref.prepare_model_input(rgb, mask, K, size, rng=("hash", seed, frame))
    return view, choose, pts2d, Kn, (rmin, rmax, cmin, cmax)
