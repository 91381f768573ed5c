"""CPU restatement of the baseline network (lib/network_baseline.py:523-669, lib/fusion.py:11-82), written from the formulas:

    per block:  y1 = W4a concat_h softmax_k((W1a x1 + b)(W2a x2 + b)^T / sqrt(8)) (W3a x2 + b) + b4a + x1      (fusion1)
                y2 = W4b concat_h softmax_k((W1b x2 + b)(W2b x1 + b)^T / sqrt(8)) (W3b x1 + b) + b4b + x2      (fusion2)
                (x1, x2) <- (y1, y2)                                   both directions read the block's inputs
    depth = relu(W4 relu(W2 relu(W0 fused + b0) + b2) + b4)            per point

torch, in the dtype of the state dict it is given (float32 or float64).  The PSPNet and the heads shared with v5 come from
oracle.adapose_ref.  Rows are point-major ([B, P, 32]) here, as in the kernels; the reference's [B, 32, P] is the transpose."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import adapose_ref

HEADS, DK, BLOCKS = 4, 8, 4


def to_sd(sd, dtype=torch.float32):
    """synth state dict (numpy) -> torch tensors of `dtype` (integer entries dropped), `module.` stripped."""
    out = {}
    for k, v in sd.items():
        a = np.asarray(v)
        if a.dtype.kind != "f":
            continue
        out[k[7:] if k.startswith("module.") else k] = torch.from_numpy(a).to(dtype)
    return out


def cross_attention(xq, xkv, sd, p, stats=None):
    """One MultiHeadedAttention(query = xq, key = value = xkv) of prefix p, rows [B, P, 32]."""
    B, P, C = xq.shape

    def lin(i, x):
        return F.linear(x, sd[f"{p}.linears.{i}.weight"], sd[f"{p}.linears.{i}.bias"])
    q = lin(0, xq).view(B, P, HEADS, DK).transpose(1, 2)
    k = lin(1, xkv).view(B, P, HEADS, DK).transpose(1, 2)
    v = lin(2, xkv).view(B, P, HEADS, DK).transpose(1, 2)
    s = q @ k.transpose(-2, -1) / math.sqrt(DK)                    # [B, H, P, P]
    pr = torch.softmax(s, dim=-1)
    if stats is not None:
        stats.setdefault("rowmax", []).append(float(pr.max(dim=-1).values.mean()))
        stats.setdefault("score_absmax", []).append(float(s.abs().max()))
    o = (pr @ v).transpose(1, 2).reshape(B, P, C)
    return lin(3, o)


def view_fusion(x1, x2, sd, prefix="view_fusion.", stats=None, blocks_out=None):
    """The four blocks on rows x1 / x2 [B, P, 32] -> (y1, y2).  stats: per attention (fusion1 then fusion2 of every block) the mean row
    maximum of the probabilities and the largest |score|; blocks_out: list that receives every block's (y1, y2)."""
    for blk in range(BLOCKS):
        p = f"{prefix}blocks.{blk}."
        y1 = cross_attention(x1, x2, sd, p + "fusion1", stats) + x1
        y2 = cross_attention(x2, x1, sd, p + "fusion2", stats) + x2
        x1, x2 = y1, y2
        if blocks_out is not None:
            blocks_out.append((y1, y2))
    return x1, x2


def depth_head(x, sd, p="depth_head"):
    """rows [..., 32] -> [...]"""
    h = F.relu(F.linear(x, sd[p + ".0.weight"].squeeze(-1), sd[p + ".0.bias"]))
    h = F.relu(F.linear(h, sd[p + ".2.weight"].squeeze(-1), sd[p + ".2.bias"]))
    return F.relu(F.linear(h, sd[p + ".4.weight"].squeeze(-1), sd[p + ".4.bias"])).squeeze(-1)


def gather_rows(feat, choose):
    """feat [B, 32, H, W], choose [B, P] -> rows [B, P, 32]"""
    B, C = feat.shape[:2]
    emb = feat.reshape(B, C, -1)
    return torch.gather(emb, 2, choose.long().unsqueeze(1).expand(B, C, choose.shape[1])).transpose(1, 2).contiguous()


@torch.no_grad()
def heads_from_rows(sd, rows1, rows2, regress_pose=True, taps=None, stats=None):
    """Everything behind the gather: rows [B, P, 32] of both views -> the reference's output dict."""
    out = {}
    f1, f2 = view_fusion(rows1, rows2, sd, stats=stats)
    if taps is not None:
        taps["fused1"], taps["fused2"] = f1, f2
    for v, rows, fused in ((1, rows1, f1), (2, rows2, f2)):
        x = adapose_ref._mlp1d(rows.transpose(1, 2), sd, "instance_color", (0,))
        nocs = torch.tanh(adapose_ref._mlp1d(x, sd, "nocs_head", (0, 2, 4), last_act=False))          # [B, 3, P]
        out[f"view{v}_nocs"] = nocs.permute(0, 2, 1).contiguous()
        out[f"view{v}_depth"] = depth_head(fused, sd)
        if regress_pose:
            pts = adapose_ref._mlp1d(nocs, sd, "nocs_pts_mlp", (0, 2))
            pf = adapose_ref._mlp1d(torch.cat((fused.transpose(1, 2), pts), dim=1), sd, "pose_mlp1", (0, 2))
            pf1 = torch.cat([pf, pf.mean(2, keepdim=True).expand_as(pf)], 1)
            pf2 = adapose_ref._mlp1d(pf1, sd, "pose_mlp2", (0, 2)).mean(2)
            r6 = adapose_ref._mlp(pf2, sd, "rotation_estimator")
            out[f"view{v}_r"] = adapose_ref.ortho6d_to_mat(r6[:, :3].contiguous(), r6[:, 3:].contiguous())
            out[f"view{v}_t"] = adapose_ref._mlp(pf2, sd, "translation_estimator")
            out[f"view{v}_s"] = adapose_ref._mlp(pf2, sd, "size_estimator")
    return out


@torch.no_grad()
def baseline_forward(sd, img1, choose1, img2, choose2, regress_pose=True, taps=None, stats=None, feat_round=None):
    """Full forward in sd's dtype.  feat_round: optional function applied to both feature maps (e.g. a round trip through a 16-bit
    type) before the gather."""
    dt = next(iter(sd.values())).dtype
    feat1 = adapose_ref.pspnet(torch.as_tensor(img1).to(dt), sd)
    feat2 = adapose_ref.pspnet(torch.as_tensor(img2).to(dt), sd)
    if feat_round is not None:
        feat1, feat2 = feat_round(feat1), feat_round(feat2)
    if taps is not None:
        taps["feat1"], taps["feat2"] = feat1, feat2
    rows1 = gather_rows(feat1, torch.as_tensor(choose1))
    rows2 = gather_rows(feat2, torch.as_tensor(choose2))
    return heads_from_rows(sd, rows1, rows2, regress_pose, taps, stats)


def rel_err(a, b):
    """The project's measure: max|a - b| / max|b|."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))
