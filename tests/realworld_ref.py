"""CPU restatement of the real-world network (lib/network_realworld.py:133-232) and of its box tail (interface_realworld.py:295-320),
written from the formulas:

    volume_v   = ref^2 + warped^2 - (ref + warped)^2          per view, channel by channel (= -2 ref warped); warped = homo_warping of
                                                              the partner view's feature map, zero where it projects outside the image
    depth      = sum_d softmax_d(CostRegNet(volume) at the chosen pixels) depth_d
    pose row   = camera_pts_mlp(x / W, y / H, depth) [64] | nocs_pts_mlp(nocs) [64]      both Conv1d 3 -> 32 -> 64 with ReLUs
    pose_mlp1 (128 -> 128 -> 128), mean, pose_mlp2, mean, the three heads: as in v5
    tail       : ts = ||view1_s|| (float32), EPnP-RANSAC + VVS on (nocs1 ts, pixels of view 1, K), box of 2 max|nocs1| ts under [R | t],
                 world frame through inv(E1)

torch, in the dtype of the state dict it is given (float32 or float64).  The PSPNet, CostRegNet and the heads shared with v5 come from
oracle.adapose_ref, the PnP routines and the box from oracle.pnp_ref / oracle.align_ref.  Pose rows are point-major ([B, P, 128]) here, as
in the kernel; the reference's [B, 128, P] is the transpose."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import adapose_ref, align_ref, pnp_ref

OUT_KEYS = [f"view{v}_{k}" for k in ("nocs", "depth", "r", "t", "s") for v in (1, 2)]
FRAME_W, FRAME_H = 640, 480


def to_sd(sd, dtype=torch.float32):
    """synth state dict (numpy) -> torch tensors of `dtype` (integer entries dropped), `module.` stripped."""
    out = {}
    for k, v in sd.items():
        a = np.asarray(v)
        if a.dtype.kind != "f":
            continue
        out[k[7:] if k.startswith("module.") else k] = torch.from_numpy(a).to(dtype)
    return out


def rel_err(a, b):
    """The project's measure: max|a - b| / max|b|."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


# the strided slices of the big tensors that tests/golden/adapose_realworld_b2.npz stores (tools/make_goldens.py: gen_adapose_realworld)
def vol_slice(v):
    """variance volume [B, 32, D, H, W] -> [B, 4, 8, 13, 13]"""
    return v[:, ::8, ::3, 3::17, 5::17]


def c0_slice(c):
    """conv0 output [B, 8, D, H, W] -> [B, 4, 8, 13, 13]"""
    return c[:, ::2, ::3, 3::17, 5::17]


def rows_slice(r):
    """pose rows [B, P, 128] -> [B, P / 16, 128]"""
    return r[:, ::16]


def homo_warping(src_fea, src_proj, ref_proj, depth_values, want_outside=False):
    """network_realworld.py:98-131 (= network_v5.py:378-416) in src_fea's dtype.  want_outside: also the mask [B, D, H, W] of the voxels
    whose four bilinear corners all lie outside the source image (the warped feature is the zero padding) or whose projection is not
    finite."""
    dt = src_fea.dtype
    B, C, H, W = src_fea.shape
    D = depth_values.shape[1]
    proj = torch.matmul(src_proj.to(dt), torch.inverse(ref_proj.to(dt)))
    rot, trans = proj[:, :3, :3], proj[:, :3, 3:4]
    y, x = torch.meshgrid(torch.arange(H, dtype=dt), torch.arange(W, dtype=dt), indexing="ij")
    xyz = torch.stack((x.reshape(-1), y.reshape(-1), torch.ones(H * W, dtype=dt)))[None].repeat(B, 1, 1)
    rot_xyz = torch.matmul(rot, xyz)
    proj_xyz = rot_xyz.unsqueeze(2) * depth_values.to(dt).view(B, 1, D, 1) + trans.view(B, 3, 1, 1)
    proj_xy = proj_xyz[:, :2] / proj_xyz[:, 2:3]
    gx = proj_xy[:, 0] / ((W - 1) / 2) - 1
    gy = proj_xy[:, 1] / ((H - 1) / 2) - 1
    grid = torch.stack((gx, gy), dim=3)
    warped = F.grid_sample(src_fea, grid.view(B, D * H, W, 2), mode="bilinear", padding_mode="zeros", align_corners=False).view(B, C, D, H, W)
    if not want_outside:
        return warped
    ix, iy = ((gx + 1) * W - 1) / 2, ((gy + 1) * H - 1) / 2          # grid_sample's un-normalisation (align_corners=False)
    outside = ~(torch.isfinite(ix) & torch.isfinite(iy)) | (ix <= -1) | (ix >= W) | (iy <= -1) | (iy >= H)
    return warped, outside.view(B, D, H, W)


def variance_volume(ref, warped):
    """network_realworld.py:145-166 with its operator order: (ref^2 + warped^2) - (ref + warped)^2."""
    ref_vol = ref.unsqueeze(2).expand_as(warped)
    sq = ref_vol ** 2 + warped ** 2
    return sq.sub_((ref_vol + warped).pow_(2))


def pose_rows(nocs, coor, depth, sd):
    """nocs [B, 3, P], coor [B, P, 2], depth [B, P] -> [B, 128, P] (network_realworld.py:198-209)"""
    pts3d = torch.cat((coor, depth.unsqueeze(-1)), dim=-1).permute(0, 2, 1).contiguous()
    cam = adapose_ref._mlp1d(pts3d, sd, "camera_pts_mlp", (0, 2))
    return torch.cat((cam, adapose_ref._mlp1d(nocs, sd, "nocs_pts_mlp", (0, 2))), dim=1)


def view_heads(feat, volume, choose, coor, depth_values, sd, taps=None, tag=""):
    B, C, H, W = feat.shape
    D, P = depth_values.shape[1], choose.shape[1]
    choose = choose.long()
    nocs_feat = torch.gather(feat.reshape(B, C, -1), 2, choose.unsqueeze(1).expand(B, C, P))
    nocs_feat = adapose_ref._mlp1d(nocs_feat, sd, "instance_color", (0,))
    nocs = torch.tanh(adapose_ref._mlp1d(nocs_feat, sd, "nocs_head", (0, 2, 4), last_act=False))
    ct = {} if taps is not None else None
    prob_full = adapose_ref.cost_reg_net(volume, sd, taps=ct).squeeze(1)
    pre = torch.gather(prob_full.view(B, D, -1), 2, choose.unsqueeze(1).expand(B, D, P))
    depth = torch.sum(F.softmax(pre, dim=1) * depth_values.view(B, D, 1), 1)
    rows = pose_rows(nocs, coor, depth, sd)
    pf = adapose_ref._mlp1d(rows, sd, "pose_mlp1", (0, 2))
    pf1 = torch.cat([pf, pf.mean(2, keepdim=True).expand_as(pf)], 1)
    pf2 = adapose_ref._mlp1d(pf1, sd, "pose_mlp2", (0, 2)).mean(2)
    r6 = adapose_ref._mlp(pf2, sd, "rotation_estimator")
    r = adapose_ref.ortho6d_to_mat(r6[:, :3].contiguous(), r6[:, 3:].contiguous())
    t = adapose_ref._mlp(pf2, sd, "translation_estimator")
    s = adapose_ref._mlp(pf2, sd, "size_estimator")
    if taps is not None:
        taps[tag + "vol_slice"] = vol_slice(volume).clone()
        taps[tag + "vol_absmean"] = float(volume.abs().mean())
        taps[tag + "vol_absmax"] = float(volume.abs().max())
        taps[tag + "c0_slice"] = c0_slice(ct["c0"]).clone()
        taps[tag + "c0_absmean"] = float(ct["c0"].abs().mean())
        taps[tag + "rows"] = rows.transpose(1, 2).contiguous()
    return nocs.permute(0, 2, 1).contiguous(), depth, r, t, s


@torch.no_grad()
def realworld_forward(sd, img1, choose1, coor1, img2, choose2, coor2, P1, P2, depths, taps=None, feat_round=None, views=(1, 2)):
    """Full forward in sd's dtype; the reference's argument order (network_realworld.py:133).  taps: receives per view v1_ / v2_ the
    slices and statistics of the variance volume and of conv0's output, the pose rows [B, P, 128] and the share of outside voxels, plus
    feat1 / feat2.  feat_round: optional function applied to both feature maps before anything reads them (a round trip through a 16-bit
    storage type).  views: which views' heads to run."""
    dt = next(iter(sd.values())).dtype
    as_t = lambda a: torch.as_tensor(a)      # noqa: E731
    feat = {1: adapose_ref.pspnet(as_t(img1).to(dt), sd), 2: adapose_ref.pspnet(as_t(img2).to(dt), sd)}
    if feat_round is not None:
        feat = {v: feat_round(f) for v, f in feat.items()}
    if taps is not None:
        taps["feat1"], taps["feat2"] = feat[1], feat[2]
    P = {1: as_t(P1), 2: as_t(P2)}
    choose = {1: as_t(choose1), 2: as_t(choose2)}
    coor = {1: as_t(coor1).to(dt), 2: as_t(coor2).to(dt)}
    dep = as_t(depths).to(dt)
    out = {}
    for v in views:
        o = 3 - v
        warped, outside = homo_warping(feat[o], P[o], P[v], dep, want_outside=True)
        volume = variance_volume(feat[v], warped)
        del warped
        if taps is not None:
            taps[f"v{v}_outside_share"] = float(outside.double().mean())
        n, d, r, t, s = view_heads(feat[v], volume, choose[v], coor[v], dep, sd, taps, f"v{v}_")
        del volume
        out.update({f"view{v}_nocs": n, f"view{v}_depth": d, f"view{v}_r": r, f"view{v}_t": t, f"view{v}_s": s})
    return out


# ------------------------------------------------------------------------------------------------ interface_realworld.py:295-320
def pnp_scaled_bbox_world(nocs1, pts2d1, s1, K, E1, seed=0, pose=0):
    """The tail for one pose: (bbox [8, 3], dict of intermediates).  As the device tail (include/rgbm.h), no consensus or a non-finite
    pose is the default box; the reference has no `success` check here."""
    nocs1 = np.asarray(nocs1, dtype=np.float32)
    ts = np.linalg.norm(np.asarray(s1, dtype=np.float32))                        # float32, interface_realworld.py:295
    info = {"scale": ts}
    pw = (nocs1 * ts).astype(np.float64)                                         # align.py:105 on float32 operands
    uv = np.asarray(pts2d1, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        ok, R, t, mask = pnp_ref.solve_pnp_ransac(pw, uv, K, seed, pose, info)
    info["ransac_ok"] = ok
    if not ok:
        return pnp_ref.DEFAULT_BBOX.copy(), info
    info.update(n_inliers=int(mask.sum()), R0=R, t0=t)
    with np.errstate(all="ignore"):
        R, t = pnp_ref.refine_vvs(pw, uv, K, R, t)
    info.update(R=R, t=t)
    if not (np.isfinite(R).all() and np.isfinite(t).all()):
        return pnp_ref.DEFAULT_BBOX.copy(), info
    return align_ref.bbox_from_srt(nocs1, ts, R, t, E1), info                    # size = 2 max|nocs1| ts in float32 (:302-303)
