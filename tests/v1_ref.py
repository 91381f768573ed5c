"""CPU restatement of the v1 network (lib/network.py:159-218), written from the formulas:

    fused_v[c, d, pix]  = feat_v[c, pix] + warped[c, d, pix]     warped = homo_warping of the partner view's ORIGINAL map, zero padding per tap
    plane[d, pix]       = volume_conv(fused_v)                    three 1x1x1 Conv3d + eval BatchNorm + ReLU, 32 -> 16 -> 8 -> 1
    new[:, pix]         = relu(feat_v[:, pix] + fuse_conv(plane[:, pix]))      1x1 Conv2d 24 -> 32, ReLU, 32 -> 32; a residual, one ReLU behind the sum
    x                   = instance_color(new gathered at choose)               32 -> 64, ReLU
    nocs                = tanh(nocs_head(x))                                   64 -> 128 -> 64 -> 3
    rows                = cat(x, nocs_pts_mlp(nocs))                           128 channels
    r, t, s             = the three heads on mean(pose_mlp2(cat(pose_mlp1(rows), mean(pose_mlp1(rows))))), Ortho6d on r

Nothing between the feature map and the gather mixes pixels, so everything is evaluated at the chosen pixels only - the project's kernels
do the same; the reference materialises two volumes and two new feature maps.  torch, in the dtype of the state dict it is given
(float32 or float64).  The warp, the tap count and the helpers are tests/v2_ref.py's; the PSPNet and the MLP helpers come from
oracle.adapose_ref.  Rows are point-major ([B, P, C]) here, as in the kernels."""
import torch
import torch.nn.functional as F

from oracle import adapose_ref
from v2_ref import points_slice, prepare_model_input, rel_err, taps_inside, to_sd, warp_grid_at      # noqa: F401  (re-exported)

OUT_KEYS = [f"view{v}_{k}" for v in (1, 2) for k in ("nocs", "r", "t", "s")]
TAP_KEYS = ("planes", "fused", "rows")      # [B, P, 24], [B, P, 32], [B, P, 128] per view
RELU_NAMES = ("volume_conv.0", "volume_conv.1", "volume_conv.2", "fuse_conv.1", "residual")


def _conv_bn_relu(x, sd, p):
    """network.py:24-31 with kernel size 1: conv (no bias) -> BatchNorm3d (running statistics) -> ReLU"""
    return F.relu(adapose_ref._bn(F.conv3d(x, sd[p + "conv.weight"]), sd, p + "bn."))


def fused_rows(feat_v, feat_o, P_v, P_o, depth_values, choose, sd, stats=None):
    """planes [B, P, D] and the new feature rows fused [B, P, 32] of one view v with partner o, at the chosen pixels.  stats (a dict)
    receives the five ReLU clip shares (RELU_NAMES), the share of (point, plane) pairs whose warp leaves the partner image and the
    per-pair tap counts."""
    dt = feat_v.dtype
    B, C, H, W = feat_v.shape
    D, P = depth_values.shape[1], choose.shape[1]
    choose = choose.long()
    ix, iy, grid = warp_grid_at(P_o, P_v, depth_values, choose, H, W, dt)
    warped = F.grid_sample(feat_o, grid, mode="bilinear", padding_mode="zeros", align_corners=False)      # [B, C, D, P]
    ref = torch.gather(feat_v.reshape(B, C, -1), 2, choose.unsqueeze(1).expand(B, C, P))                # [B, C, P]
    x = (ref.unsqueeze(2) + warped).unsqueeze(-1)                                                       # [B, C, D, P, 1]
    clip = []
    for l in range(3):
        x = _conv_bn_relu(x, sd, f"volume_conv.{l}.")
        clip.append(float((x == 0).double().mean()))
    planes = x.reshape(B, D, P)
    h = F.relu(F.conv1d(planes, sd["fuse_conv.0.weight"].reshape(32, D, 1), sd["fuse_conv.0.bias"]))
    clip.append(float((h == 0).double().mean()))
    fused = F.relu(ref + F.conv1d(h, sd["fuse_conv.2.weight"].reshape(32, 32, 1), sd["fuse_conv.2.bias"]))
    clip.append(float((fused == 0).double().mean()))
    if stats is not None:
        n = taps_inside(ix, iy, H, W)
        stats["clip"] = clip
        stats["outside"] = float((n == 0).double().mean())
        stats["taps"] = n
    return planes.transpose(1, 2).contiguous(), fused.transpose(1, 2).contiguous()


def point_branch(fused, sd):
    """fused [B, P, 32] -> nocs [B, P, 3], rows [B, P, 128] (network.py:183-197)"""
    x = adapose_ref._mlp1d(fused.transpose(1, 2), sd, "instance_color", (0,))
    nocs = torch.tanh(adapose_ref._mlp1d(x, sd, "nocs_head", (0, 2, 4), last_act=False))
    rows = torch.cat((x, adapose_ref._mlp1d(nocs, sd, "nocs_pts_mlp", (0, 2))), dim=1)
    return nocs.permute(0, 2, 1).contiguous(), rows.transpose(1, 2).contiguous()


def pose_branch(rows, sd):
    """rows [B, P, 128] -> r [B, 3, 3], t [B, 3], s [B, 3] (network.py:199-206)"""
    pf = adapose_ref._mlp1d(rows.transpose(1, 2), sd, "pose_mlp1", (0, 2))
    pf1 = torch.cat([pf, pf.mean(2, keepdim=True).expand_as(pf)], 1)
    pf2 = adapose_ref._mlp1d(pf1, sd, "pose_mlp2", (0, 2)).mean(2)
    r6 = adapose_ref._mlp(pf2, sd, "rotation_estimator")
    r = adapose_ref.ortho6d_to_mat(r6[:, :3].contiguous(), r6[:, 3:].contiguous())
    return r, adapose_ref._mlp(pf2, sd, "translation_estimator"), adapose_ref._mlp(pf2, sd, "size_estimator")


@torch.no_grad()
def heads_on_maps(sd, feat1, feat2, choose1, choose2, P1, P2, depths, taps=None, views=(1, 2), pose=True):
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
        planes, fused = fused_rows(feat[v], feat[o], P[v], P[o], dep, choose[v], sd, stats)
        nocs, rows = point_branch(fused, sd)
        out[f"view{v}_nocs"] = nocs
        if pose:
            out[f"view{v}_r"], out[f"view{v}_t"], out[f"view{v}_s"] = pose_branch(rows, sd)
        if taps is not None:
            taps.update({f"v{v}_planes": planes, f"v{v}_fused": fused, f"v{v}_rows": rows, f"v{v}_clip": stats["clip"],
                         f"v{v}_outside": stats["outside"], f"v{v}_taps": stats["taps"]})
    return out


@torch.no_grad()
def v1_forward(sd, img1, choose1, img2, choose2, P1, P2, depths, taps=None, feat_round=None, views=(1, 2)):
    """Full forward in sd's dtype; the reference's argument order (network.py:159).  taps: per view v1_ / v2_ the planes, fused and rows
    tensors, the five ReLU clip shares and the outside share, plus feat1 / feat2.  feat_round: optional function applied to both feature
    maps before anything reads them (a round trip through a 16-bit storage type)."""
    dt = next(iter(sd.values())).dtype
    f1 = adapose_ref.pspnet(torch.as_tensor(img1).to(dt), sd)
    f2 = adapose_ref.pspnet(torch.as_tensor(img2).to(dt), sd)
    if feat_round is not None:
        f1, f2 = feat_round(f1), feat_round(f2)
    if taps is not None:
        taps["feat1"], taps["feat2"] = f1, f2
    return heads_on_maps(sd, f1, f2, choose1, choose2, P1, P2, depths, taps, views)
