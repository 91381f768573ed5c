#!/usr/bin/env python3
"""Generate tests/golden/*.npz by importing the REFERENCE modules from /root/reference.

Runs only in the build container (the reference never travels to the GPU box; only the
small .npz outputs written here are committed).  Recipe = SURVEY.md Appendix C:
stub torchvision/cv2/ipdb/gym/sapien/tensorboard, make Tensor.cuda the identity
(rotation_utils.py:6 hard-codes .cuda()), put the net in .eval().

Inputs and weights come from rgbmanip_amd.synth (seeded; regenerated identically by tests).
"""
import copy
import os
import sys
import types

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF = "/root/reference"
sys.path.insert(1, REF)

import numpy as np
import torch
import yaml


def stub(name, **kw):
    m = types.ModuleType(name)
    m.__dict__.update(kw)
    sys.modules[name] = m
    return m


class _Space:
    pass


class _Box(_Space):
    def __init__(self, low, high, shape=None, dtype=np.float32):
        self.shape = tuple(shape) if shape is not None else np.asarray(low).shape
        self.low = np.full(self.shape, low, dtype=np.float32) if np.isscalar(low) else np.asarray(low)
        self.high = np.full(self.shape, high, dtype=np.float32) if np.isscalar(high) else np.asarray(high)
        self.dtype = dtype


class _Dict(_Space):
    def __init__(self, spaces=None):
        self.spaces = spaces or {}


class _SW:
    def __init__(self, *a, **k):
        pass

    def add_scalar(self, *a, **k):
        pass


def install_stubs():
    stub("torchvision", models=stub("torchvision.models"))
    stub("cv2")
    stub("ipdb")
    spaces = stub("gym.spaces", Space=_Space, Box=_Box, Dict=_Dict)
    gv = stub("gym.vector")
    gvu = stub("gym.vector.utils", shared_memory=stub("gym.vector.utils.shared_memory"))
    gv.utils = gvu
    stub("gym", spaces=spaces, vector=gv, Env=object)
    sc = stub("sapien.core", Pose=object)
    stub("sapien", core=sc)
    stub("torch.utils.tensorboard", SummaryWriter=_SW)
    stub("env.my_vec_env", MultiVecEnv=object)
    torch.Tensor.cuda = lambda self, *a, **k: self


def strided(t, n=64):
    f = t.reshape(-1)
    step = max(1, f.numel() // n)
    return f[::step][:n].clone().numpy()


def gen_adapose(out_dir):
    from models.pose_estimator.AdaPose.lib.network_v5 import StereoPoseNet_with_depth
    from rgbmanip_amd import synth

    net = StereoPoseNet_with_depth(n_cat=1, nv_pts=1024, regress_pose=True).eval()
    sd = synth.adapose_state_dict(seed=0)
    missing = net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    print("load_state_dict:", missing)
    B = 2
    inp = synth.adapose_inputs(B, seed=0)
    tin = {k: torch.from_numpy(v) for k, v in inp.items()}
    inter = {}

    def hook(name):
        def f(mod, i, o):
            inter.setdefault(name, o.detach())
        return f
    ie = net.img_extractor
    hs = [ie.feats.conv1.register_forward_hook(hook("v1_conv1_raw")),
          ie.feats.maxpool.register_forward_hook(hook("v1_pool")),
          ie.feats.layer1.register_forward_hook(hook("v1_layer1")),
          ie.feats.layer2.register_forward_hook(hook("v1_layer2")),
          ie.feats.layer3.register_forward_hook(hook("v1_layer3")),
          ie.feats.layer4.register_forward_hook(hook("v1_layer4")),
          ie.psp.register_forward_hook(hook("v1_psp")),
          ie.up_1.register_forward_hook(hook("v1_up_1")),
          ie.up_2.register_forward_hook(hook("v1_up_2")),
          ie.up_3.register_forward_hook(hook("v1_up_3")),
          ie.register_forward_hook(hook("feat1")),
          net.cost_regularization.conv0.register_forward_hook(hook("v1_c0")),
          net.cost_regularization.conv2.register_forward_hook(hook("v1_c2")),
          net.cost_regularization.conv4.register_forward_hook(hook("v1_c4")),
          net.cost_regularization.conv6.register_forward_hook(hook("v1_c6")),
          net.cost_regularization.conv7.register_forward_hook(hook("v1_d7")),
          net.cost_regularization.conv9.register_forward_hook(hook("v1_d9")),
          net.cost_regularization.conv11.register_forward_hook(hook("v1_d11")),
          net.cost_regularization.prob.register_forward_hook(hook("v1_probvol"))]
    with torch.no_grad():
        out = net(tin["img1"], tin["choose1"], tin["img2"], tin["choose2"], tin["P1"], tin["P2"], tin["depths"])
        # run twice: eval mode must be deterministic
        out2 = net(tin["img1"], tin["choose1"], tin["img2"], tin["choose2"], tin["P1"], tin["P2"], tin["depths"])
    for h in hs:
        h.remove()
    for k in out:
        assert torch.equal(out[k], out2[k]), k
    save = {k: v.numpy() for k, v in out.items()}
    for k, v in inter.items():
        save["slice_" + k] = strided(v)
        save["absmean_" + k] = np.array(v.abs().mean().item(), dtype=np.float64)
    np.savez_compressed(os.path.join(out_dir, "adapose_b2.npz"), **save)
    for k, v in out.items():
        print(k, tuple(v.shape), float(v.abs().mean()), bool(torch.isfinite(v).all()))
    print("depth range", out["view1_depth"].min().item(), out["view1_depth"].max().item())

    # reduced-shape layer fixtures straight from reference sub-modules
    g = np.random.default_rng(5)
    with torch.no_grad():
        x = torch.from_numpy(g.normal(size=(2, 3, 64, 64)).astype(np.float32))
        y = ie(x)
        vol = torch.from_numpy(g.normal(size=(1, 32, 8, 16, 16)).astype(np.float32))
        pv = net.cost_regularization(vol)
        fea = torch.from_numpy(g.normal(size=(2, 32, 16, 16)).astype(np.float32))
        K = np.array([[20.0, 0, 8, 0], [0, 20.0, 8, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
        E1 = np.eye(4)
        E2 = np.eye(4)
        E2[0, 3] = -0.1
        E2[2, 3] = 0.02
        Pa = torch.from_numpy(np.stack([K @ E1, K @ E1]).astype(np.float32))
        Pb = torch.from_numpy(np.stack([K @ E2, K @ E2]).astype(np.float32))
        dv = torch.from_numpy(np.tile(np.arange(0.1, 0.85, 0.1, dtype=np.float32)[None], (2, 1)))
        wv = net.homo_warping(fea, Pb, Pa, dv)
    np.savez_compressed(os.path.join(out_dir, "adapose_layers.npz"),
                        psp_in=x.numpy(), psp_out=y.numpy(), cr_in=vol.numpy(), cr_out=pv.numpy(),
                        warp_fea=fea.numpy(), warp_Psrc=Pb.numpy(), warp_Pref=Pa.numpy(), warp_depths=dv.numpy(),
                        warp_out=wv.numpy())
    return out, inp


def gen_adapose_baseline(out_dir):
    """The baseline network (lib/network_baseline.py) on the golden batch, and the attention stack alone on two small shapes."""
    from models.pose_estimator.AdaPose.lib.network_baseline import StereoPoseNet_with_depth_baseline
    from models.pose_estimator.AdaPose.lib.fusion import ViewFusion
    from rgbmanip_amd import synth

    net = StereoPoseNet_with_depth_baseline(n_cat=1, nv_pts=1024, regress_pose=True).eval()
    sd = synth.baseline_state_dict(seed=0)
    print("load_state_dict:", net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True))
    B = 2
    inp = synth.adapose_inputs(B, seed=0)
    tin = {k: torch.from_numpy(v) for k, v in inp.items()}
    inter = {}

    def hook(name):
        def f(mod, i, o):
            inter.setdefault(name, o.detach())
        return f
    ie = net.img_extractor
    hs = [ie.feats.conv1.register_forward_hook(hook("v1_conv1_raw")), ie.feats.maxpool.register_forward_hook(hook("v1_pool")),
          ie.feats.layer1.register_forward_hook(hook("v1_layer1")), ie.feats.layer2.register_forward_hook(hook("v1_layer2")),
          ie.feats.layer3.register_forward_hook(hook("v1_layer3")), ie.feats.layer4.register_forward_hook(hook("v1_layer4")),
          ie.psp.register_forward_hook(hook("v1_psp")), ie.up_1.register_forward_hook(hook("v1_up_1")),
          ie.up_2.register_forward_hook(hook("v1_up_2")), ie.up_3.register_forward_hook(hook("v1_up_3")),
          ie.register_forward_hook(hook("feat1"))]
    fused = {}
    hs.append(net.view_fusion.register_forward_hook(lambda mod, i, o: fused.update(fused1=o[0].detach(), fused2=o[1].detach())))

    def rowmax():      # mean largest probability per softmax row: fusion1 then fusion2 of every block
        return np.array([float(f.attn.max(dim=-1).values.mean()) for blk in net.view_fusion.blocks for f in (blk.fusion1, blk.fusion2)])
    args = (tin["img1"], tin["choose1"], tin["img2"], tin["choose2"], tin["P1"], tin["P2"], tin["depths"])
    with torch.no_grad():
        out = net(*args)
        rm = rowmax()
        out2 = net(*args)
    for h in hs:
        h.remove()
    for k in out:
        assert torch.equal(out[k], out2[k]), k
    print("row-maximum means per attention:", rm)
    assert (rm >= 0.2).all() and (rm <= 0.9).all(), "adjust synth.BASELINE_QK_GAIN: the golden batch's attention is too flat or too peaked"
    save = {k: v.numpy() for k, v in out.items()}
    save["fused1"] = fused["fused1"].transpose(1, 2).contiguous().numpy()       # [B, P, 32], point-major
    save["fused2"] = fused["fused2"].transpose(1, 2).contiguous().numpy()
    save["rowmax_mean"] = rm
    for k, v in inter.items():
        save["slice_" + k] = strided(v)
        save["absmean_" + k] = np.array(v.abs().mean().item(), dtype=np.float64)
    for tag, rp in (("", True), ("_nopose", False)):
        ref_sd = StereoPoseNet_with_depth_baseline(n_cat=1, nv_pts=1024, regress_pose=rp).state_dict()
        save["sd_keys" + tag] = np.array(list(ref_sd.keys()))
        save["sd_shapes" + tag] = np.array(["x".join(str(d) for d in v.shape) for v in ref_sd.values()])
    np.savez_compressed(os.path.join(out_dir, "adapose_baseline_b2.npz"), **save)
    for k, v in out.items():
        print(k, tuple(v.shape), float(v.abs().mean()), bool(torch.isfinite(v).all()))

    # the attention stack alone: the reference module with the same constructed weights on two small shapes
    vf = ViewFusion(embed_dim=32, num_heads=4, depth=4).eval()
    vf.load_state_dict({k[len("view_fusion."):]: torch.from_numpy(v) for k, v in sd.items() if k.startswith("view_fusion.")}, strict=True)
    small = {}
    for Bs, Ps in ((3, 96), (1, 32)):
        x1, x2 = synth.view_fusion_inputs(Bs, Ps, seed=0)
        blocks = []
        hb = [blk.register_forward_hook(lambda mod, i, o: blocks.append(o)) for blk in vf.blocks]
        with torch.no_grad():
            y1, y2 = vf(torch.from_numpy(x1).transpose(1, 2).contiguous(), torch.from_numpy(x2).transpose(1, 2).contiguous())
        for h in hb:
            h.remove()
        t = f"b{Bs}_p{Ps}_"
        small[t + "x1"], small[t + "x2"] = x1, x2
        small[t + "y1"], small[t + "y2"] = y1.transpose(1, 2).contiguous().numpy(), y2.transpose(1, 2).contiguous().numpy()
        for i, (o1, o2) in enumerate(blocks):
            small[t + f"blk{i}_y1"], small[t + f"blk{i}_y2"] = o1.transpose(1, 2).contiguous().numpy(), o2.transpose(1, 2).contiguous().numpy()
    np.savez_compressed(os.path.join(out_dir, "view_fusion_small.npz"), **small)


def gen_adapose_realworld(out_dir):
    """The real-world network (lib/network_realworld.py) on the golden batch.  Data only: the ten outputs, the seeded point coordinates,
    strided slices and statistics of both variance volumes, of conv0's output and of the 128-channel pose rows, the share of voxels whose
    warp falls outside the partner image, and the class's state-dict keys and shapes.  The shipped interface_realworld.py:287 calls the
    network without the coordinates it computes at :264-269 (a TypeError); the network itself is sound and is called here with them."""
    from models.pose_estimator.AdaPose.lib.network_realworld import StereoPoseNet_with_depth_for_realdemo
    from rgbmanip_amd import synth
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import realworld_ref as rr

    net = StereoPoseNet_with_depth_for_realdemo(n_cat=1, nv_pts=1024, regress_pose=True).eval()
    sd = synth.realworld_state_dict(seed=0)
    print("load_state_dict:", net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True))
    B = 2
    inp = synth.adapose_inputs(B, seed=0)
    pts1, pts2, coor1, coor2 = synth.realworld_coor(B, seed=0)
    tin = {k: torch.from_numpy(v) for k, v in inp.items()}
    vols, c0s, rows = [], [], []
    hs = [net.cost_regularization.register_forward_pre_hook(lambda mod, i: vols.append(i[0].detach())),
          net.cost_regularization.conv0.register_forward_hook(lambda mod, i, o: c0s.append(o.detach())),
          net.pose_mlp1.register_forward_pre_hook(lambda mod, i: rows.append(i[0].detach()))]
    args = (tin["img1"], tin["choose1"], torch.from_numpy(coor1), tin["img2"], tin["choose2"], torch.from_numpy(coor2), tin["P1"], tin["P2"],
            tin["depths"])
    with torch.no_grad():
        out = net(*args)
        save = {k: v.numpy() for k, v in out.items()}
        for v in (1, 2):      # view 1's volume, c0 and rows come first in the forward
            vol, c0, row = vols[v - 1], c0s[v - 1], rows[v - 1]
            save[f"v{v}_vol_slice"] = rr.vol_slice(vol).contiguous().numpy()
            save[f"v{v}_vol_absmean"] = np.array(vol.abs().mean().item(), dtype=np.float64)
            save[f"v{v}_vol_absmax"] = np.array(vol.abs().max().item(), dtype=np.float64)
            save[f"v{v}_c0_slice"] = rr.c0_slice(c0).contiguous().numpy()
            save[f"v{v}_c0_absmean"] = np.array(c0.abs().mean().item(), dtype=np.float64)
            save[f"v{v}_rows_slice"] = rr.rows_slice(row.transpose(1, 2)).contiguous().numpy()      # [B, P / 16, 128], point-major
            save[f"v{v}_rows_absmean"] = np.array(row.abs().mean().item(), dtype=np.float64)
        del vols[:], c0s[:], rows[:]
        out2 = net(*args)
        for h in hs:
            h.remove()
        for k in out:
            assert torch.equal(out[k], out2[k]), k
        # where the warp leaves the partner image (all four bilinear corners outside): per view, from the restatement's float32 grid
        feat = {1: net.img_extractor(tin["img1"]), 2: net.img_extractor(tin["img2"])}
        for v in (1, 2):
            o = 3 - v
            _, outside = rr.homo_warping(feat[o], tin[f"P{o}"], tin[f"P{v}"], tin["depths"], want_outside=True)
            save[f"v{v}_outside_share"] = np.array(outside.double().mean().item(), dtype=np.float64)
            save[f"v{v}_outside_share_slice"] = np.array(outside[:, ::3, 3::17, 5::17].double().mean().item(), dtype=np.float64)
            print(f"view {v}: outside share {float(save[f'v{v}_outside_share']):.4f} (in the slice {float(save[f'v{v}_outside_share_slice']):.4f}), "
                  f"|vol| max {float(save[f'v{v}_vol_absmax']):.1f} mean {float(save[f'v{v}_vol_absmean']):.2f}")
            # the fixture conditions tests/test_realworld_host.py asserts: if the rig misses one, add a second seeded rig, do not loosen them
            assert 0.05 <= save[f"v{v}_outside_share"] <= 0.95 and 0.05 <= save[f"v{v}_outside_share_slice"] <= 0.95, "degenerate rig"
            assert save[f"v{v}_vol_absmax"] >= 10 * save[f"v{v}_vol_absmean"]
    save["pts2d1"], save["pts2d2"] = pts1, pts2
    save["coor1"], save["coor2"] = coor1, coor2
    save["frame_wh"] = np.array([rr.FRAME_W, rr.FRAME_H], dtype=np.int64)
    ref_sd = net.state_dict()
    save["sd_keys"] = np.array(list(ref_sd.keys()))
    save["sd_shapes"] = np.array(["x".join(str(d) for d in v.shape) for v in ref_sd.values()])
    path = os.path.join(out_dir, "adapose_realworld_b2.npz")
    np.savez_compressed(path, **save)
    print("wrote", path, os.path.getsize(path), "bytes")
    for k, v in out.items():
        print(k, tuple(v.shape), float(v.abs().mean()), bool(torch.isfinite(v).all()))


def gen_adapose_v2(out_dir):
    """The v2 network (lib/network_v2.py: StereoPoseNet) on the golden batch.  Data only: the four outputs; for both views, at the chosen
    pixels, volume_conv's 24 values, fuse_conv's 64 channels and pose_mlp1's output (every 8th point, and the whole tensor's largest
    magnitude: 128 of the 1024 points per view and pose, which keeps the file at 251 KB); as scalars measured here on all points, not
    recomputable from the stored slices except the planes' zero share, the clip share of the four ReLUs in front of them and
    the share of (point, plane) pairs whose warp leaves the partner image; the class's state-dict keys and shapes.  The forward runs view
    2's volume_conv / fuse_conv first (network_v2.py:158-159) and view 1's pose_mlp1 first (:184, :190)."""
    from models.pose_estimator.AdaPose.lib.network_v2 import StereoPoseNet
    from rgbmanip_amd import synth
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import v2_ref

    net = StereoPoseNet(n_cat=1).eval()
    sd = synth.v2_state_dict(seed=0)
    print("load_state_dict:", net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True))
    B = 2
    inp = synth.adapose_inputs(B, seed=0)
    tin = {k: torch.from_numpy(v) for k, v in inp.items()}
    choose = {1: tin["choose1"].long(), 2: tin["choose2"].long()}
    vc = [[], [], []]
    fc_relu, fc_out, pm1 = [], [], []

    def at_choose(t, v):      # [B, C, (D,) H, W] -> [B, P, C (, D)] at view v's chosen pixels
        t = t.reshape(t.shape[0], t.shape[1], -1, t.shape[-2] * t.shape[-1])
        g = torch.stack([t[b][:, :, choose[v][b]] for b in range(t.shape[0])])      # [B, C, D', P]
        return g.permute(0, 3, 1, 2).contiguous()

    # view 2's chain comes first: call k of these hooks belongs to view 2 - k
    hs = [net.volume_conv[l].register_forward_hook(lambda mod, i, o, l=l: vc[l].append(at_choose(o.detach(), 2 - len(vc[l])))) for l in range(3)]
    hs.append(net.fuse_conv[1].register_forward_hook(lambda mod, i, o: fc_relu.append(at_choose(o.detach(), 2 - len(fc_relu)))))
    hs.append(net.fuse_conv.register_forward_hook(lambda mod, i, o: fc_out.append(at_choose(o.detach(), 2 - len(fc_out)))))
    hs.append(net.pose_mlp1.register_forward_hook(lambda mod, i, o: pm1.append(o.detach().transpose(1, 2).contiguous())))      # view 1 first
    args = (tin["img1"], tin["choose1"], tin["img2"], tin["choose2"], tin["P1"], tin["P2"], tin["depths"])
    with torch.no_grad():
        out = net(*args)
        for h in hs:
            h.remove()
        out2 = net(*args)
        for k in out:
            assert torch.equal(out[k], out2[k]), k
        save = {k: v.numpy() for k, v in out.items()}
        feat = {1: net.img_extractor(tin["img1"]), 2: net.img_extractor(tin["img2"])}
        for v in (1, 2):
            o, k = 3 - v, 2 - v      # k: position of view v in the lists of the hooks that see view 2 first
            planes = vc[2][k][:, :, 0, :]                                      # [B, P, 24]
            fuse = fc_out[k][:, :, :, 0]                                       # [B, P, 64]
            rows = pm1[v - 1]                                                  # [B, P, 64]
            for name, t in (("planes", planes), ("fuse", fuse), ("rows", rows)):      # every 8th point: [B, P / 8, C]
                save[f"v{v}_{name}_slice"] = v2_ref.points_slice(t).contiguous().numpy()
                save[f"v{v}_{name}_absmax"] = np.array(float(t.abs().max()), dtype=np.float64)
            clip = [float((vc[l][k] == 0).double().mean()) for l in range(3)] + [float((fc_relu[k] == 0).double().mean())]
            ix, iy, _ = v2_ref.warp_grid_at(tin[f"P{o}"], tin[f"P{v}"], tin["depths"], choose[v], feat[v].shape[2], feat[v].shape[3], torch.float32)
            outside = float((v2_ref.taps_inside(ix, iy, feat[v].shape[2], feat[v].shape[3]) == 0).double().mean())
            spread = float(rows.std(dim=1).mean() / rows.abs().mean())
            save[f"v{v}_clip"] = np.array(clip, dtype=np.float64)
            save[f"v{v}_outside"] = np.array(outside, dtype=np.float64)
            save[f"v{v}_rows_spread"] = np.array(spread, dtype=np.float64)
            print(f"view {v}: clip shares {['%.3f' % c for c in clip]}, outside share {outside:.3f}, rows' std over points / mean |row| {spread:.3f}")
            # the fixture conditions tests/test_v2_host.py re-asserts: if the draw misses one, change the draw or add a second seeded rig
            assert all(0.05 <= c <= 0.95 for c in clip), "a ReLU that clips (almost) nothing or everything"
            assert 0.05 <= outside <= 0.95, "degenerate rig"
            assert spread >= 0.25, "rows that do not depend on the point"
        s1, s2 = out["view1_s"], out["view2_s"]
        sdiff = float((s1 - s2).abs().max() / torch.maximum(s1.abs().max(), s2.abs().max()))
        print(f"max|s1 - s2| / max|s| {sdiff:.4f}")
        assert sdiff >= 0.02, "a size output that does not depend on the view"
    ref_sd = net.state_dict()
    save["sd_keys"] = np.array(list(ref_sd.keys()))
    save["sd_shapes"] = np.array(["x".join(str(d) for d in v.shape) for v in ref_sd.values()])
    path = os.path.join(out_dir, "adapose_v2_b2.npz")
    np.savez_compressed(path, **save)
    print("wrote", path, os.path.getsize(path), "bytes")
    for k, v in out.items():
        print(k, tuple(v.shape), float(v.abs().mean()), bool(torch.isfinite(v).all()))


def gen_adapose_v1(out_dir):
    """The v1 network (lib/network.py: StereoPoseNet) on the golden batch.  Data only: the eight outputs; for both views, at every 8th
    chosen point (v2_ref.points_slice), volume_conv's 24 values, the new feature rows relu(feat + fuse_conv(planes)) and the 128-channel
    pose rows, with each whole tensor's largest magnitude; as scalars measured here on all points, the clip shares of the five ReLUs of the
    stereo part (the residual one last) and the share of (point, plane) pairs whose warp leaves the partner image; the class's state-dict
    keys and shapes.  The forward runs view 2's volume_conv first (network.py:173-174) and view 1's heads first."""
    from models.pose_estimator.AdaPose.lib.network import StereoPoseNet
    from rgbmanip_amd import synth
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import v2_ref

    net = StereoPoseNet(n_cat=1).eval()
    sd = synth.v1_state_dict(seed=0)
    print("load_state_dict:", net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True))
    B = 2
    inp = synth.adapose_inputs(B, seed=0)
    tin = {k: torch.from_numpy(v) for k, v in inp.items()}
    choose = {1: tin["choose1"].long(), 2: tin["choose2"].long()}
    vc = [[], [], []]
    fc_relu, inst_in, pm1_in = [], [], []

    def at_choose(t, v):      # [B, C, (D,) H, W] -> [B, P, C (, D)] at view v's chosen pixels
        t = t.reshape(t.shape[0], t.shape[1], -1, t.shape[-2] * t.shape[-1])
        g = torch.stack([t[b][:, :, choose[v][b]] for b in range(t.shape[0])])      # [B, C, D', P]
        return g.permute(0, 3, 1, 2).contiguous()

    # volume_conv sees view 2 first, fuse_conv view 1 first; instance_color and pose_mlp1 see view 1 first: their inputs are the gathered
    # new feature rows and the pose rows
    hs = [net.volume_conv[l].register_forward_hook(lambda mod, i, o, l=l: vc[l].append(at_choose(o.detach(), 2 - len(vc[l])))) for l in range(3)]
    hs.append(net.fuse_conv[1].register_forward_hook(lambda mod, i, o: fc_relu.append(at_choose(o.detach(), 1 + len(fc_relu)))))
    hs.append(net.instance_color.register_forward_pre_hook(lambda mod, i: inst_in.append(i[0].detach().transpose(1, 2).contiguous())))
    hs.append(net.pose_mlp1.register_forward_pre_hook(lambda mod, i: pm1_in.append(i[0].detach().transpose(1, 2).contiguous())))
    args = (tin["img1"], tin["choose1"], tin["img2"], tin["choose2"], tin["P1"], tin["P2"], tin["depths"])
    with torch.no_grad():
        out = net(*args)
        for h in hs:
            h.remove()
        out2 = net(*args)
        for k in out:
            assert torch.equal(out[k], out2[k]), k
        save = {k: v.numpy() for k, v in out.items()}
        feat = {1: net.img_extractor(tin["img1"]), 2: net.img_extractor(tin["img2"])}
        for v in (1, 2):
            o, k = 3 - v, 2 - v      # k: position of view v in the lists of volume_conv's hooks, which see view 2 first
            planes = vc[2][k][:, :, 0, :]                                      # [B, P, 24]
            fused = inst_in[v - 1]                                             # [B, P, 32]
            rows = pm1_in[v - 1]                                               # [B, P, 128]
            for name, t in (("planes", planes), ("fused", fused), ("rows", rows)):      # every 8th point: [B, P / 8, C]
                save[f"v{v}_{name}_slice"] = v2_ref.points_slice(t).contiguous().numpy()
                save[f"v{v}_{name}_absmax"] = np.array(float(t.abs().max()), dtype=np.float64)
            clip = [float((vc[l][k] == 0).double().mean()) for l in range(3)] + [float((fc_relu[v - 1] == 0).double().mean()),
                                                                                 float((fused == 0).double().mean())]
            H, W = feat[v].shape[2], feat[v].shape[3]
            ix, iy, _ = v2_ref.warp_grid_at(tin[f"P{o}"], tin[f"P{v}"], tin["depths"], choose[v], H, W, torch.float32)
            outside = float((v2_ref.taps_inside(ix, iy, H, W) == 0).double().mean())
            save[f"v{v}_clip"] = np.array(clip, dtype=np.float64)
            save[f"v{v}_outside"] = np.array(outside, dtype=np.float64)
            print(f"view {v}: clip shares {['%.3f' % c for c in clip]}, outside share {outside:.3f}")
            # the fixture conditions tests/test_v1_host.py re-asserts: if the draw misses one, change the draw, not the condition
            assert all(0.05 <= c <= 0.95 for c in clip), "a ReLU that clips (almost) nothing or everything"
            assert 0.0 < outside < 1.0, "every warp leaves the partner image, or none does"
            r = out[f"view{v}_r"].double()
            assert float((r.transpose(1, 2) @ r - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-5 and bool((torch.linalg.det(r) > 0.999).all()), "r is no rotation"
        s1, s2 = out["view1_s"], out["view2_s"]
        sdiff = float((s1 - s2).abs().max() / torch.maximum(s1.abs().max(), s2.abs().max()))
        print(f"max|s1 - s2| / max|s| {sdiff:.4f}")
        assert not torch.equal(s1, s2) and sdiff >= 1e-3, "a size output that does not depend on the view"
    ref_sd = net.state_dict()
    save["sd_keys"] = np.array(list(ref_sd.keys()))
    save["sd_shapes"] = np.array(["x".join(str(d) for d in v.shape) for v in ref_sd.values()])
    path = os.path.join(out_dir, "adapose_v1_b2.npz")
    np.savez_compressed(path, **save)
    print("wrote", path, os.path.getsize(path), "bytes")
    for k, v in out.items():
        print(k, tuple(v.shape), float(v.abs().mean()), bool(torch.isfinite(v).all()))


def gen_adapose_trainbn(out_dir):
    """The as-shipped normalisation (interface_v5.py:39-56 never calls .eval()): the reference module in .train()
    with only its Dropout2d modules in .eval() (their masks are random), run the way the estimator runs it — ONE pose per call —
    so that every BatchNorm3d normalises with the statistics of that pose's own volume.  Deterministic; pins norm_mode = 1."""
    from models.pose_estimator.AdaPose.lib.network_v5 import StereoPoseNet_with_depth
    from rgbmanip_amd import synth

    net = StereoPoseNet_with_depth(n_cat=1, nv_pts=1024, regress_pose=True)
    sd = synth.adapose_state_dict(seed=0)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    net.train()
    n_drop = 0
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout2d):
            m.eval()
            n_drop += 1
    assert n_drop == 1, n_drop          # pspnet.py:122: one Dropout2d module, applied twice (pspnet.py:150,154)
    B = 2
    inp = synth.adapose_inputs(B, seed=0)
    tin = {k: torch.from_numpy(v) for k, v in inp.items()}
    outs = []
    with torch.no_grad():
        for b in range(B):
            one = lambda k: tin[k][b:b + 1]  # noqa: E731
            o = net(one("img1"), one("choose1"), one("img2"), one("choose2"), one("P1"), one("P2"), one("depths"))
            o2 = net(one("img1"), one("choose1"), one("img2"), one("choose2"), one("P1"), one("P2"), one("depths"))
            for k in o:
                assert torch.equal(o[k], o2[k]), k          # batch statistics of a fixed input: deterministic
            outs.append(o)
    save = {k: torch.cat([o[k] for o in outs]).numpy() for k in outs[0]}
    np.savez_compressed(os.path.join(out_dir, "adapose_b2_trainbn.npz"), **save)
    for k, v in save.items():
        print("trainbn", k, v.shape, float(np.abs(v).mean()), bool(np.isfinite(v).all()))


def gen_adapose_dropout(out_dir):
    """The as-shipped estimator in full: the reference module in .train() with its Dropout2d ACTIVE, one pose per call (as
    gen_adapose_trainbn).  Torch's random stream is not reproducible on the device, so every call of PSPNet.drop is wrapped: the keep
    mask of the call is recorded (the module run on a ones tensor under the saved RNG state), the RNG state restored, the module run
    on the real input, and the two checked to agree.  Saves the masks in the C ABI's order (rgbm_adapose_set_dropout_masks:
    masks[V][up_1's 256 channels, then up_2's 64], views = the view-1 crops of the batch, then the view-2 crops) and the ten outputs."""
    from models.pose_estimator.AdaPose.lib.network_v5 import StereoPoseNet_with_depth
    from rgbmanip_amd import synth

    torch.manual_seed(1234)
    net = StereoPoseNet_with_depth(n_cat=1, nv_pts=1024, regress_pose=True)
    sd = synth.adapose_state_dict(seed=0)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    net.train()
    drop = net.img_extractor.drop
    assert isinstance(drop, torch.nn.Dropout2d) and drop.p == 0.15
    inner = drop.forward
    calls = []

    def recording_forward(x):
        state = torch.get_rng_state()
        m = inner(torch.ones_like(x))
        torch.set_rng_state(state)
        y = inner(x)
        mc = m[:, :, 0, 0]
        assert torch.equal(m, mc[:, :, None, None].expand_as(m))          # one factor per (sample, channel)
        assert torch.equal(y, x * mc[:, :, None, None])
        calls.append(mc[0].clone())
        return y

    drop.forward = recording_forward
    B = 2
    inp = synth.adapose_inputs(B, seed=0)
    tin = {k: torch.from_numpy(v) for k, v in inp.items()}
    outs = []
    masks = np.zeros((2 * B, 320), np.float32)
    with torch.no_grad():
        for b in range(B):
            one = lambda k: tin[k][b:b + 1]  # noqa: E731
            calls.clear()
            outs.append(net(one("img1"), one("choose1"), one("img2"), one("choose2"), one("P1"), one("P2"), one("depths")))
            # img_extractor(view1) then img_extractor(view2) (network_v5.py:423-424), each: drop after up_1, drop after up_2
            assert [c.numel() for c in calls] == [256, 64, 256, 64], [c.numel() for c in calls]
            for side in range(2):
                masks[side * B + b, :256] = calls[2 * side].numpy()
                masks[side * B + b, 256:] = calls[2 * side + 1].numpy()
    assert set(np.unique(masks).tolist()) <= {0.0, float(np.float32(1.0) / np.float32(0.85))}, np.unique(masks)
    save = {k: torch.cat([o[k] for o in outs]).numpy() for k in outs[0]}
    save["masks"] = masks
    np.savez_compressed(os.path.join(out_dir, "adapose_b2_dropout.npz"), **save)
    print("dropout keep fraction", float((masks != 0).mean()))
    for k, v in save.items():
        print("dropout", k, v.shape, float(np.abs(v).mean()), bool(np.isfinite(v).all()))


def gen_postproc(out_dir, net_out, inp):
    from models.pose_estimator.AdaPose.lib import utils as U

    cases = {}
    g = np.random.default_rng(11)

    def run_case(nocs, depth, R, choose, K, E1):
        # glue = interface_v5.py:318-321,354-374 around the reference's own lib/utils.py functions
        default_bbox = np.asarray([[0, 0, 0], [0, 0, 1], [0, 1, 0], [0, 1, 1],
                                   [1, 0, 0], [1, 0, 1], [1, 1, 0], [1, 1, 1]]) + 10.0
        with np.errstate(all="ignore"):
            tt, ts = U.compute_scale_and_translation(depth, nocs, choose, K, 224, R)
            half = np.max(abs(nocs), axis=0)
            size = 2 * half * ts
            bbox = U.get_3d_bbox(size)
            sRT = np.eye(4).astype(np.float32)
            sRT[:3, :3] = R
            sRT[:3, 3] = tt.flatten()
            bbox = U.transform_coordinates_3d(bbox, sRT)
            ex_inv = np.linalg.inv(E1)
            if np.isfinite(ex_inv).all() and np.isfinite(bbox).all():
                return (ex_inv[:3, :3] @ bbox + ex_inv[:3, 3:4]).T, tt, ts
            return default_bbox, tt, ts

    idx = 0
    # cases 0,1: the network outputs of the golden forward
    for b in range(2):
        nocs = net_out["view1_nocs"][b].numpy()
        depth = net_out["view1_depth"][b].numpy()
        R = net_out["view1_r"][b].numpy()
        bb, tt, ts = run_case(nocs, depth, R, inp["choose1"][b], inp["K1"][b], inp["E1"][b])
        cases[f"c{idx}_in_nocs"], cases[f"c{idx}_in_depth"], cases[f"c{idx}_in_R"] = nocs, depth, R
        cases[f"c{idx}_in_choose"], cases[f"c{idx}_in_K"], cases[f"c{idx}_in_E"] = inp["choose1"][b], inp["K1"][b], inp["E1"][b]
        cases[f"c{idx}_bbox"], cases[f"c{idx}_t"], cases[f"c{idx}_s"] = bb, np.asarray(tt), np.asarray(ts)
        idx += 1
    # random well-posed cases + degenerate ones
    for kind in ("rand", "rand", "rand", "even", "empty_valid", "nan_depth"):
        nocs = g.uniform(-0.45, 0.45, size=(1024, 3)).astype(np.float32)
        depth = g.uniform(0.5, 0.8, size=(1024,)).astype(np.float32)
        q, _ = np.linalg.qr(g.normal(size=(3, 3)))
        R = q.astype(np.float32)
        choose = np.sort(g.choice(224 * 224, size=1024, replace=False)).astype(np.int64)
        K = np.array([[300.0, 0, 112.0], [0, 300.0, 112.0], [0, 0, 1]])
        E = np.eye(4)
        E[:3, :3] = np.linalg.qr(g.normal(size=(3, 3)))[0]
        E[:3, 3] = g.normal(size=3)
        if kind == "even":
            choose[512:] = choose[:512]           # duplicates (wrap padding, Appendix B-15)
            nocs[512:] = nocs[:512]
            depth[512:] = depth[:512]
        if kind == "empty_valid":
            nocs[:] = nocs[0]                     # all nocs distances 0 -> empty set -> nan -> default bbox
        if kind == "nan_depth":
            depth[3] = np.nan
        bb, tt, ts = run_case(nocs, depth, R, choose, K, E)
        cases[f"c{idx}_in_nocs"], cases[f"c{idx}_in_depth"], cases[f"c{idx}_in_R"] = nocs, depth, R
        cases[f"c{idx}_in_choose"], cases[f"c{idx}_in_K"], cases[f"c{idx}_in_E"] = choose, K, E
        cases[f"c{idx}_bbox"], cases[f"c{idx}_t"], cases[f"c{idx}_s"] = bb, np.asarray(tt), np.asarray(ts)
        print("postproc case", idx, kind, "scale", ts, "bbox0", bb[0])
        idx += 1
    cases["n_cases"] = np.array(idx)
    # get_bbox table
    gb_in, gb_out = [], []
    for _ in range(64):
        y1, x1 = int(g.integers(0, 470)), int(g.integers(0, 630))
        y2, x2 = int(g.integers(y1, 480)), int(g.integers(x1, 640))
        gb_in.append([y1, x1, y2, x2])
        gb_out.append(list(U.get_bbox([y1, x1, y2, x2])))
    cases["get_bbox_in"] = np.array(gb_in)
    cases["get_bbox_out"] = np.array(gb_out)
    np.savez_compressed(os.path.join(out_dir, "postproc.npz"), **cases)


def gen_postproc_v4(out_dir):
    """tests/golden/postproc_v4.npz: the `adapose_v4` interface where it differs from v5 (interface_v4.py:52-58, 322-325, 358-378).

    Poses: the `direct_regression: True` tail on a dozen poses — glue = interface_v4.py:322-325, 358-378 around the reference's own
    get_3d_bbox / transform_coordinates_3d and the numpy calls of the interface, in its dtypes (ts is a float32 scalar, so the box stays
    float32 up to the world transform).  Poses 0, 1 are the golden forward's outputs (adapose_b2.npz), the rest seeded.
    Crops: `AdaPoseEstimator_v4.prepare_model_input` of the reference class itself (built by its own constructor, which chooses the
    transform from cfg["task_name"]) on the frames of rgbmanip_amd.synth.crop_frames: frame 0 for task one_door_cabinet (plain ToTensor:
    the un-normalised crop, img_size 224), frame 1 for task pots (ToTensor + Normalize, img_size 112 — the file has to stay small).
    The build image has neither OpenCV nor torchvision: `cv2.resize` is the documented INTER_NEAREST / INTER_LINEAR arithmetic of
    oracle/postproc_ref.py (as everywhere in this repository, "parity unpinned" at that step), `transforms.ToTensor / Normalize /
    Compose` are the stand-ins below, which follow torchvision's documented semantics."""
    from oracle import postproc_ref
    from rgbmanip_amd import synth

    def cv2_resize(img, dsize, interpolation):
        assert dsize[0] == dsize[1]
        return (postproc_ref.resize_nearest if interpolation == 0 else postproc_ref.resize_linear)(img, dsize[0])

    class ToTensor:
        def __call__(self, pic):                    # HWC ndarray -> CHW tensor; uint8 is scaled to [0, 1], floats keep dtype and values
            t = torch.from_numpy(np.ascontiguousarray(np.transpose(pic, (2, 0, 1))))
            return t.to(torch.float32).div(255) if pic.dtype == np.uint8 else t

    class Normalize:
        def __init__(self, mean, std):
            self.mean, self.std = mean, std

        def __call__(self, t):
            mean = torch.as_tensor(self.mean, dtype=t.dtype)[:, None, None]
            std = torch.as_tensor(self.std, dtype=t.dtype)[:, None, None]
            return t.clone().sub_(mean).div_(std)

    class Compose:
        def __init__(self, ts):
            self.ts = ts

        def __call__(self, x):
            for t in self.ts:
                x = t(x)
            return x

    sys.modules["cv2"].resize, sys.modules["cv2"].INTER_NEAREST, sys.modules["cv2"].INTER_LINEAR = cv2_resize, 0, 1
    sys.modules["torchvision"].transforms = stub("torchvision.transforms", ToTensor=ToTensor, Normalize=Normalize, Compose=Compose)
    stub("env.base_sapien_env", BaseEnv=object)
    stub("env.sapien_envs.open_cabinet", OpenCabinetEnv=object)
    stub("env.sapien_envs", open_cabinet=sys.modules["env.sapien_envs.open_cabinet"])
    from models.pose_estimator.AdaPose.interface_v4 import AdaPoseEstimator_v4
    from models.pose_estimator.AdaPose.lib import utils as U

    default_bbox = np.asarray([[0, 0, 0], [0, 0, 1], [0, 1, 0], [0, 1, 1], [1, 0, 0], [1, 0, 1], [1, 1, 0], [1, 1, 1]]) + 10.0

    def run_case(nocs, r, t, s, E1):
        with np.errstate(all="ignore"):
            tr, tt, ts = r, t, np.linalg.norm(s)                               # interface_v4.py:323-325
            half_size = np.max(abs(nocs), axis=0)                              # :359-361
            size = 2 * half_size * ts
            bbox = U.get_3d_bbox(size)
            sRT = np.eye(4).astype(np.float32)                                 # :363-366
            sRT[:3, :3] = tr
            sRT[:3, 3] = tt.flatten()
            bbox = U.transform_coordinates_3d(bbox, sRT)
            assert ts.dtype == np.float32 and bbox.dtype == np.float32, (ts.dtype, bbox.dtype)
            ex_inv = np.linalg.inv(E1)                                         # :373-378
            if np.isfinite(ex_inv).all() and np.isfinite(bbox).all():
                return (ex_inv[:3, :3] @ bbox + ex_inv[:3, 3:4]).T, ts
            return default_bbox, ts

    g = np.random.default_rng(44)
    net = np.load(os.path.join(out_dir, "adapose_b2.npz"))
    inp = synth.adapose_inputs(2, seed=0)
    cases = []
    for b in range(2):
        cases.append(("net", net["view1_nocs"][b], net["view1_r"][b], net["view1_t"][b], net["view1_s"][b], inp["E1"][b].astype(np.float64)))
    for kind in ("rand", "rand", "rand", "rand", "far", "tiny", "nan_s", "inf_nocs", "nan_nocs", "nan_E"):
        nocs = g.uniform(-0.45, 0.45, size=(1024, 3)).astype(np.float32)
        r = np.linalg.qr(g.normal(size=(3, 3)))[0].astype(np.float32)
        t = (np.array([0.0, 0.0, 0.8]) + g.normal(0, 0.2, 3)).astype(np.float32)
        s = g.normal(0, 0.3, 3).astype(np.float32)
        E = np.eye(4)
        E[:3, :3] = np.linalg.qr(g.normal(size=(3, 3)))[0]
        E[:3, 3] = g.normal(size=3)
        if kind == "far":
            t, s = t * np.float32(40), s * np.float32(25)
        if kind == "tiny":
            s = s * np.float32(1e-3)
        if kind == "nan_s":
            s[1] = np.nan
        if kind == "inf_nocs":
            nocs[700, 2] = np.inf
        if kind == "nan_nocs":
            nocs[5, 0] = np.nan
        if kind == "nan_E":
            E[1, 2] = np.nan
        cases.append((kind, nocs, r, t, s, E))
    save = {"kinds": np.array([c[0] for c in cases])}
    boxes, scales = [], []
    for i, (kind, nocs, r, t, s, E) in enumerate(cases):
        bb, ts = run_case(nocs, r, t, s, E)
        boxes.append(bb)
        scales.append(ts)
        print("postproc_v4 case", i, kind, "scale", ts, "bbox0", bb[0])
    for j, name in enumerate(("nocs", "r", "t", "s", "E1")):
        save[name] = np.stack([c[1 + j] for c in cases])
    save["bbox"], save["scale"] = np.stack(boxes), np.array(scales, dtype=np.float32)

    rgb8, mask, K = synth.crop_frames(seed=0)
    rgb = rgb8.astype(np.float32) / np.float32(255.0)                           # float frames holding fl32(b / 255)
    for f, (task, S) in enumerate((("one_door_cabinet", 224), ("pots", 112))):
        cfg = {"name": "adapose_v4", "task_name": task, "load": False, "checkpoint_path": "", "img_size": S, "use_depth": True,
               "n_pts": 1024, "direct_regression": True, "real_world": False}
        est = AdaPoseEstimator_v4(None, cfg, None)
        assert isinstance(est.transform, Compose) == (task == "pots")
        np.random.seed(400 + f)
        view, choose, pts2d, Kn = est.prepare_model_input(rgb[f], mask[f], K[f], S)
        view = view.float().numpy()                                             # interface_v4.py:263
        assert view.shape == (3, S, S) and choose.shape == (1024,)
        save[f"crop{f}_task"], save[f"crop{f}_size"] = np.array(task), np.array(S)
        save[f"crop{f}_img"], save[f"crop{f}_K"], save[f"crop{f}_n_distinct"] = view, Kn, np.array(len(np.unique(choose)))
        if len(np.unique(choose)) < 1024:                                       # wrap padding: no random subset, the indices are pinned too
            save[f"crop{f}_choose"], save[f"crop{f}_pts2d"] = choose, pts2d
        print("postproc_v4 crop", f, task, S, "range", float(view.min()), float(view.max()), "distinct choose", len(np.unique(choose)))
    path = os.path.join(out_dir, "postproc_v4.npz")
    np.savez_compressed(path, **save)
    print("postproc_v4.npz:", os.path.getsize(path), "bytes")


def gen_ppo(out_dir):
    from algo.ppo.ppo import PPO, ActorCritic, RolloutStorage
    from rgbmanip_amd import synth

    cfg = yaml.safe_load(open(os.path.join(REF, "cfg/controller/rl.yaml")))
    cfg["learn"]["device"] = "cpu"
    cfg["learn"]["log_dir"] = "/tmp/rgbm_gold_logs"
    cfg["learn"]["save_dir"] = "/tmp/rgbm_gold_saves"
    save = {}
    for N in (32, 512):
        T = cfg["learn"]["num_transitions_per_env"]

        class FakeEnv:
            num_envs = N
            observation_space = _Box(-1.5, 1.5, (60,))
            state_space = _Box(-1.5, 1.5, (75,))
            action_space = _Box(-1.5, 1.5, (12,))
        ppo = PPO(FakeEnv(), cfg)
        sd = synth.policy_state_dict(seed=0)
        ppo.actor_critic.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        roll = synth.ppo_rollout(T, N, seed=0)
        tr = {k: torch.from_numpy(v) for k, v in roll.items()}
        # act with a recorded noise draw
        torch.manual_seed(123)
        a, logp, v, mu, sig = ppo.actor_critic.act(tr["observations"][0], tr["states"][0])
        torch.manual_seed(123)
        eps = torch.randn(N, 12)
        recon = mu + torch.exp(2 * ppo.actor_critic.log_std.detach()) * eps
        print(f"N={N} act sample reconstruction max err", (recon - a).abs().max().item())
        tag = f"n{N}_"
        if N == 32:
            save.update({tag + "act_eps": eps.numpy(), tag + "act_a": a.numpy(), tag + "act_logp": logp.numpy(),
                         tag + "act_v": v.numpy(), tag + "act_mu": mu.numpy()})
        # fill the storage: actions from the rollout, logp/mu/sigma from evaluate of the *initial* policy with an offset
        with torch.no_grad():
            for t in range(T):
                lp, ent, vv, mm, ss, _ = ppo.actor_critic.evaluate(tr["observations"][t], None, tr["actions"][t])
                mm = mm + 0.02 * torch.sin(torch.arange(12.0))[None]      # pretend the behaviour policy differed a bit
                ppo.storage.add_transitions(tr["observations"][t], tr["states"][t], tr["actions"][t],
                                            tr["rewards"][t].view(-1), tr["dones"][t].view(-1), tr["values"][t],
                                            lp - 0.01, mm, ss - 0.005)
                if N == 32 and t == 0:
                    save.update({tag + "eval_logp": lp.numpy(), tag + "eval_ent": ent.numpy(), tag + "eval_v": vv.numpy()})
        ppo.storage.compute_returns(tr["last_values"], cfg["learn"]["gamma"], cfg["learn"]["lam"])
        st = ppo.storage
        rec = {"returns": st.returns, "advantages": st.advantages, "actions_log_prob": st.actions_log_prob,
               "mu": st.mu, "sigma": st.sigma}
        mvl, msl = ppo.update(0)
        flat = torch.cat([p.detach().reshape(-1) for p in ppo.actor_critic.state_dict().values()])
        print(f"N={N} update: value_loss {mvl:.6f} surrogate {msl:.6f} lr {ppo.step_size}")
        if N == 32:
            for k, val in rec.items():
                save[tag + k] = val.numpy()
            save[tag + "params_after"] = flat.numpy()
        else:
            save[tag + "returns_sum"] = np.array(rec["returns"].double().sum().item())
            save[tag + "adv_abs_sum"] = np.array(rec["advantages"].double().abs().sum().item())
            save[tag + "returns_slice"] = strided(rec["returns"])
            save[tag + "adv_slice"] = strided(rec["advantages"])
            save[tag + "params_after_slice"] = strided(flat, 256)
        save[tag + "mvl"] = np.array(mvl)
        save[tag + "msl"] = np.array(msl)
        save[tag + "lr_after"] = np.array(ppo.step_size)
    np.savez_compressed(os.path.join(out_dir, "ppo.npz"), **save)


def gen_ppo_variants(out_dir):
    """The reference's `ActorCritic` / `PPO` for every variant of rgbmanip_amd.synth.PPO_VARIANTS (hidden-size lists, activations,
    asymmetric critic, plain-MSE value loss): state_dict keys and shapes, a strided slice of the seeded initialisation, `act` with
    a recorded noise draw, `evaluate`, and one `PPO.update` at N = 32 filled as gen_ppo fills it.  Parameters after the update are
    stored as a strided slice of 2048 (the 256-wide default has 300 k of them)."""
    from algo.ppo.ppo import PPO
    from rgbmanip_amd import synth

    base = yaml.safe_load(open(os.path.join(REF, "cfg/controller/rl.yaml")))
    base["learn"].update(device="cpu", log_dir="/tmp/rgbm_gold_logs", save_dir="/tmp/rgbm_gold_saves")
    N, save = 32, {}
    T = base["learn"]["num_transitions_per_env"]
    roll = synth.ppo_rollout(T, N, seed=0)
    tr = {k: torch.from_numpy(v) for k, v in roll.items()}

    class FakeEnv:
        num_envs = N
        observation_space = _Box(-1.5, 1.5, (60,))
        state_space = _Box(-1.5, 1.5, (75,))
        action_space = _Box(-1.5, 1.5, (12,))
    for name, (mcfg, asym, clipped) in synth.PPO_VARIANTS.items():
        cfg = copy.deepcopy(base)
        cfg["learn"].update(asymmetric=asym, use_clipped_value_loss=clipped)
        cfg["policy"] = dict(actor_critic_class="ActorCritic", **mcfg) if mcfg is not None else None
        if mcfg is None:      # PPO reads policy["actor_critic_class"] and hands the same dict to ActorCritic: None only directly
            cfg["policy"] = dict(actor_critic_class="ActorCritic", pi_hid_sizes=[256] * 3, vf_hid_sizes=[256] * 3, activation="selu")
            from algo.ppo.ppo import ActorCritic
            torch.manual_seed(1234)
            direct = ActorCritic((60,), (75,), (12,), 0.6, None, asymmetric=False)
        torch.manual_seed(1234)
        ppo = PPO(FakeEnv(), cfg)
        ac = ppo.actor_critic
        sd0 = ac.state_dict()
        if mcfg is None:      # the class default builds what the explicit 256x3 SELU cfg builds
            assert list(direct.state_dict().keys()) == list(sd0.keys())
            assert all(torch.equal(a, b) for a, b in zip(direct.state_dict().values(), sd0.values()))
        tag = name + "_"
        save[tag + "keys"] = np.array(list(sd0.keys()))
        save[tag + "shapes"] = np.array([list(v.shape) + [0] * (2 - v.dim()) for v in sd0.values()], dtype=np.int64)
        save[tag + "init_slice"] = strided(torch.cat([v.reshape(-1) for v in sd0.values()]), 256)
        sd = synth.policy_variant_state_dict(name, seed=0)
        ac.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        torch.manual_seed(123)
        a, logp, v, mu, sig = ac.act(tr["observations"][0], tr["states"][0])
        torch.manual_seed(123)
        eps = torch.randn(N, 12)
        recon = mu + torch.exp(2 * ac.log_std.detach()) * eps
        assert (recon - a).abs().max().item() < 1e-6
        save.update({tag + "act_eps": eps.numpy(), tag + "act_a": a.numpy(), tag + "act_logp": logp.numpy(),
                     tag + "act_v": v.numpy(), tag + "act_mu": mu.numpy()})
        with torch.no_grad():
            for t in range(T):
                lp, ent, vv, mm, ss, _ = ac.evaluate(tr["observations"][t], tr["states"][t], tr["actions"][t])
                mm = mm + 0.02 * torch.sin(torch.arange(12.0))[None]
                ppo.storage.add_transitions(tr["observations"][t], tr["states"][t], tr["actions"][t],
                                            tr["rewards"][t].view(-1), tr["dones"][t].view(-1), tr["values"][t],
                                            lp - 0.01, mm, ss - 0.005)
                if t == 0:
                    save.update({tag + "eval_logp": lp.numpy(), tag + "eval_ent": ent.numpy(), tag + "eval_v": vv.numpy()})
        ppo.storage.compute_returns(tr["last_values"], cfg["learn"]["gamma"], cfg["learn"]["lam"])
        mvl, msl = ppo.update(0)
        flat = torch.cat([p.detach().reshape(-1) for p in ac.state_dict().values()])
        print(f"{name}: {flat.numel()} parameters; update: value_loss {mvl:.6f} surrogate {msl:.6f} lr {ppo.step_size}")
        save[tag + "params_after_slice"] = strided(flat, 2048)
        save[tag + "mvl"] = np.array(mvl)
        save[tag + "msl"] = np.array(msl)
        save[tag + "lr_after"] = np.array(ppo.step_size)
    np.savez_compressed(os.path.join(out_dir, "ppo_variants.npz"), **save)


def gen_ppo_run(out_dir):
    """`PPO.run` of the reference (ppo.py:203-312, log: 356-447) for two learning iterations on rgbmanip_amd.synth.StubVecEnv:
    the class as shipped, a recording SummaryWriter, the policy noise reproduced from the seed.  Saved: the noise draws, every
    action the env received, every scalar `log()` wrote, the parameters and learning rate at the end."""
    from algo.ppo.ppo import PPO
    from rgbmanip_amd import synth

    cfg = yaml.safe_load(open(os.path.join(REF, "cfg/controller/rl.yaml")))
    cfg["learn"].update(device="cpu", log_dir="/tmp/rgbm_gold_logs", save_dir="/tmp/rgbm_gold_saves", print_log=True, testing=False)
    # schedule "fixed": with the shipped "adaptive" schedule the first minibatches of an on-policy rollout have KL = +-1e-7 (the
    # stored and the current policy are the same), and `kl_mean > 0.0` (ppo.py:485) then decides by rounding noise whether the
    # learning rate starts to grow 1.5x per step: the reference's own trajectory changes with the BLAS thread count.  The adaptive
    # rule itself is pinned by gen_ppo (KL well away from zero).
    cfg["learn"].update(schedule="fixed", learning_rate=3.0e-4)
    N, iters = 32, 2
    T = cfg["learn"]["num_transitions_per_env"]
    env = synth.StubVecEnv(N, _Box, seed=0)
    ppo = PPO(env, cfg)
    ppo.actor_critic.load_state_dict({k: torch.from_numpy(v) for k, v in synth.policy_state_dict(seed=0).items()}, strict=True)
    scalars = {}

    class Rec:
        def add_scalar(self, tag, value, step=None, *a, **k):
            scalars.setdefault(tag, []).append((float(step) if step is not None else -1.0, float(value)))
    ppo.writer = Rec()
    # `RolloutStorage.get_statistics` (storage.py:66-72) does `done = self.dones.cpu(); done[-1] = 1`.  On the reference's own device
    # (rl.yaml: cuda) `.cpu()` is a copy; with device="cpu", as here, it is the storage tensor itself, and the GAE that run() computes
    # next would see every env's last transition as terminal.  Keep the cuda behaviour: restore the tensor after the call.
    stats0 = ppo.storage.get_statistics

    def stats_without_aliasing():
        keep = ppo.storage.dones.clone()
        out = stats0()
        ppo.storage.dones.copy_(keep)
        return out
    ppo.storage.get_statistics = stats_without_aliasing
    torch.manual_seed(777)
    ppo.run(iters, log_interval=1, save_interval=1000)
    n_calls = iters * (T + 1)
    torch.manual_seed(777)
    eps = torch.stack([torch.randn(N, 12) for _ in range(n_calls)])
    acts = torch.stack(env.action_log)
    assert acts.shape[0] == iters * T
    # the draws are the policy's noise: the first action is mu + std^2 * eps0 of the initial policy
    ppo0 = PPO(synth.StubVecEnv(N, _Box, seed=0), cfg)
    ppo0.actor_critic.load_state_dict({k: torch.from_numpy(v) for k, v in synth.policy_state_dict(seed=0).items()}, strict=True)
    with torch.no_grad():
        mu0 = ppo0.actor_critic.act_inference(env.reset())
        recon = mu0 + torch.exp(2 * ppo0.actor_critic.log_std) * eps[0]
    err = (recon - acts[0]).abs().max().item()
    print("ppo_run: first action reconstructed from the seeded noise, max err", err)
    assert err < 1e-6
    save = {"eps": eps.numpy(), "actions": acts.numpy(), "lr_after": np.array(ppo.step_size),
            "params_after": torch.cat([p.detach().reshape(-1) for p in ppo.actor_critic.state_dict().values()]).numpy()}
    # tags whose x axis is wall-clock time are recorded by the reference too; their values duplicate Train/mean_*: keep the rest
    for tag, rows in scalars.items():
        if tag.endswith("/time"):
            continue
        save["scalar:" + tag] = np.array([v for _, v in rows], dtype=np.float64)
        print(f"  {tag}: {[round(v, 5) for _, v in rows]}")
    np.savez_compressed(os.path.join(out_dir, "ppo_run.npz"), **save)


def gen_control(out_dir):
    """View queue / encoders / view selection of the reference ControlInterface (rl_pose.py:14-223) on the seeded view
    stream of rgbmanip_amd.synth.control_view: the class is imported as shipped; only the modules it drags in for the
    simulator are replaced by name stubs, and the env / estimator are recording fakes."""
    from rgbmanip_amd import synth
    stub("env.sapien_envs.open_cabinet", CAMERA_INTRINSIC=[0.05, 100, 1, 640, 480])
    stub("env.sapien_envs", open_cabinet=sys.modules["env.sapien_envs.open_cabinet"])
    stub("models.manipulation.open_cabinet", OpenCabinetManipulation=object)
    stub("models.controller.base_controller", BaseController=object)
    stub("models.pose_estimator.base_estimator", BasePoseEstimator=object)      # the real one imports the SAPIEN env base
    cwd = os.getcwd()
    os.chdir("/tmp")                                   # ControlInterface.__init__ creates saves/third_stage in the cwd
    try:
        from models.controller.rl_pose import ControlInterface
        N, seed = 3, 4

        class FakeEnv:
            num_envs = N

            def __init__(self):
                self.t = 0
                self.cur = None

            def cam_move_to(self, *a, **k):
                return np.ones(N), np.ones(N)

            def get_image(self):
                self.cur = synth.control_view(N, self.t, seed)
                self.t += 1
                return self.cur[0]

            def camera_pose(self, robot_frame=True):
                return self.cur[1]

        class FakeEstimator:
            def __init__(self, task):
                self.cfg = {"task_name": task}
                self.calls = []

            def estimate(self, K, rgb1, m1, E1, rgb2, m2, E2):
                self.calls.append(dict(id1=rgb1[:, 0, 0, 0].copy(), id2=rgb2[:, 0, 0, 0].copy(), m1=m1.sum((1, 2)), m2=m2.sum((1, 2)),
                                       K=K.copy(), E1=E1.copy(), E2=E2.copy()))
                base = np.arange(24, dtype=np.float64).reshape(1, 8, 3)
                return base + (m1.sum((1, 2)) * 1e-3 + rgb2[:, 0, 0, 0])[:, None, None]

        cfg = {"controller": {"max_steps": 4, "action_type": "pose", "pose_min": [0.1, -0.4, 0.5], "pose_max": [0.5, 0.4, 1.1]}}
        save = {}
        for task in ("cabinet", "mugs"):
            env, est = FakeEnv(), FakeEstimator(task)
            ci = ControlInterface(env, est, None, cfg)
            obs, states, boxes = [ci.get_observation().numpy()], [ci.get_state().numpy()], []
            for step in range(7):
                ci.add_view(env.get_image(), env.camera_pose(robot_frame=True))
                pred = ci.get_estimation()
                ci.add_bbox(pred, env.cur[2])
                boxes.append(pred.copy())
                obs.append(ci.get_observation().numpy())
                states.append(ci.get_state().numpy())
                ci.accumulate_steps += 1
                if ci.accumulate_steps == 6:             # exercise reset_queue + a fresh first view mid-stream
                    ci.reset_queue()
                    ci.add_view(env.get_image(), env.camera_pose(robot_frame=True))
                    ci.accumulate_steps += 1
            save[task + "_obs"] = np.stack(obs)
            save[task + "_state"] = np.stack(states)
            save[task + "_pred"] = np.stack(boxes)
            for key in ("id1", "id2", "m1", "m2", "K", "E1", "E2"):
                save[task + "_" + key] = np.stack([c[key] for c in est.calls])
            save[task + "_available"] = ci.available.copy()
            save[task + "_available_num"] = ci.available_num.copy()
            save[task + "_bbox_queue"] = ci.bbox_queue.copy()
        np.savez_compressed(os.path.join(out_dir, "control.npz"), **save)
        print("control golden:", {k: v.shape for k, v in save.items() if k.startswith("cabinet")})
    finally:
        os.chdir(cwd)


REWARD_KEYS = ["REW:diff", "REW:move_success", "REW:move_period", "REW:far", "REW:ori_rew", "REW:xyz_lookat", "REW:bbox_penalty",
               "REW:bbox_boundary_penalty", "REW:have_bbox", "REW:center_rew", "REW:open_rew", "REW:view_rew",
               "REW:view_norm_penalty", "REW:success", "LOSS:center_diff", "LOSS:open_diff", "LOSS:far"]


def gen_control_step(out_dir):
    """`ControlInterface.step` / `get_reward` / `get_done` / `reset` / `reset_robot` / `call_manipulation`
    (rl_pose.py:99-116, 225-462) of the reference class itself, driven through 2+ episodes by
    rgbmanip_amd.synth.ReplayVecEnv, seeded actions and the same recording fake estimator as gen_control."""
    from rgbmanip_amd import synth
    stub("env.sapien_envs.open_cabinet", CAMERA_INTRINSIC=[0.05, 100, 1, 640, 480])
    stub("env.sapien_envs", open_cabinet=sys.modules["env.sapien_envs.open_cabinet"])
    stub("models.manipulation.open_cabinet", OpenCabinetManipulation=object)
    stub("models.controller.base_controller", BaseController=object)
    stub("models.pose_estimator.base_estimator", BasePoseEstimator=object)
    cwd = os.getcwd()
    os.chdir("/tmp")
    try:
        from models.controller.rl_pose import ControlInterface
        from utils.transform import lookat_quat
        N, seed = 3, 4

        class FakeEstimator:
            def __init__(self, task):
                self.cfg = {"task_name": task}

            def estimate(self, K, rgb1, m1, E1, rgb2, m2, E2):
                base = np.arange(24, dtype=np.float64).reshape(1, 8, 3) * 0.01
                return base + (m1.sum((1, 2)) * 1e-5 + rgb2[:, 0, 0, 0])[:, None, None] + np.sin(np.arange(24.0)).reshape(1, 8, 3) * E1[:, 0, 3, None, None]

        class Manip:
            def __init__(self):
                self.calls = []

            def plan_pathway(self, center, direction, eval):
                self.calls.append((center.copy(), direction.copy(), bool(eval)))

        save = {}
        for task, succ in (("cabinet", 0.0), ("mugs", 0.0), ("pots", 1.5)):
            cfg = synth.control_cfg(task, succ)
            env, est, man = synth.ReplayVecEnv(N, seed), FakeEstimator(task), Manip()
            ci = ControlInterface(env, est, man, cfg)
            rec = {k: [] for k in ("obs", "reward", "done", "target", "terms", "state")}
            rec["obs"].append(ci.get_observation().numpy())
            for step in range(10):
                a = torch.from_numpy(synth.control_actions(N, step, seed))
                obs, rew, done, info = ci.step(a, eval=False)
                rec["obs"].append(obs.numpy()); rec["reward"].append(rew.numpy()); rec["done"].append(done.numpy())
                rec["target"].append(ci.last_pose_target.copy())
                rec["terms"].append(np.stack([info[k].numpy().astype(np.float64) for k in REWARD_KEYS]))
                rec["state"].append(ci.get_state().numpy())
            for k, v in rec.items():
                save[f"{task}_{k}"] = np.stack(v)
            save[f"{task}_resets"] = np.array(env.resets)
            save[f"{task}_move_pose"] = np.stack([np.broadcast_to(m["pose"], (N, 7)) for m in env.moves])
            save[f"{task}_move_ndim"] = np.array([m["pose"].ndim for m in env.moves])
            save[f"{task}_move_flags"] = np.array([[m["skip_move"], m["no_collision_with_front"], m["robot_frame"]] for m in env.moves])
            save[f"{task}_move_tw"] = np.array([[m["time"], m["wait"]] for m in env.moves])
            if man.calls:
                save[f"{task}_manip_center"] = np.stack([c[0] for c in man.calls])
                save[f"{task}_manip_direction"] = np.stack([c[1] for c in man.calls])
                save[f"{task}_manip_eval"] = np.array([c[2] for c in man.calls])
        # lookat_quat (utils/transform.py:50-99) on directions covering its three per-row branches
        d = np.random.default_rng(11).normal(size=(64, 3))
        d[0] = [0, 0, 1.0]; d[1] = [0, 0, -2.0]; d[2] = [1, 0, 0]; d[3] = [1e-4, 0, 1.0]; d[4] = [3, -4, 0]
        save["lookat_dir"] = d
        save["lookat_quat"] = lookat_quat(d)
        np.savez_compressed(os.path.join(out_dir, "control_step.npz"), **save)
        print("control_step golden:", {k: v.shape for k, v in save.items() if k.startswith("pots") or k.startswith("lookat")})
    finally:
        os.chdir(cwd)


def gen_control_save(out_dir):
    """`ControlInterface._save_data` (rl_pose.py:56-83): the eval-time dataset export the reference runs in the step that
    brings `accumulate_steps` to `max_steps - 1` when `eval` is set (:446-447; `RLPoseController.run` always steps with
    eval=True).  The reference class is driven through two eval episodes on the ReplayVecEnv in a scratch directory and the
    files it wrote are summarised: relative path, shape, dtype, float64 sum and a strided sample (the frames themselves are
    22 MB per file)."""
    import tempfile
    from rgbmanip_amd import synth
    stub("env.sapien_envs.open_cabinet", CAMERA_INTRINSIC=[0.05, 100, 1, 640, 480])
    stub("env.sapien_envs", open_cabinet=sys.modules["env.sapien_envs.open_cabinet"])
    stub("models.manipulation.open_cabinet", OpenCabinetManipulation=object)
    stub("models.controller.base_controller", BaseController=object)
    stub("models.pose_estimator.base_estimator", BasePoseEstimator=object)
    cwd = os.getcwd()
    tmp = tempfile.mkdtemp(prefix="rgbm_save_")
    os.chdir(tmp)
    try:
        from models.controller.rl_pose import ControlInterface
        N, seed = 3, 4

        class FakeEstimator:
            def __init__(self, task):
                self.cfg = {"task_name": task}

            def estimate(self, K, rgb1, m1, E1, rgb2, m2, E2):
                base = np.arange(24, dtype=np.float64).reshape(1, 8, 3) * 0.01
                return base + (m1.sum((1, 2)) * 1e-5 + rgb2[:, 0, 0, 0])[:, None, None] + np.sin(np.arange(24.0)).reshape(1, 8, 3) * E1[:, 0, 3, None, None]

        class Manip:
            def plan_pathway(self, center, direction, eval):
                pass

        cfg = synth.control_cfg("cabinet", 0.0)
        env = synth.ReplayVecEnv(N, seed)
        ci = ControlInterface(env, FakeEstimator("cabinet"), Manip(), cfg)
        for step in range(9):                                   # two full episodes (4 steps each) and one step of a third
            ci.step(torch.from_numpy(synth.control_actions(N, step, seed)), eval=True)
        save = {}
        paths = []
        for root, _, files in sorted(os.walk("saves")):
            for f in sorted(files):
                paths.append(os.path.join(root, f))
        for i, pth in enumerate(paths):
            z = np.load(pth)
            assert list(z.keys()) == ["arr_0"], (pth, list(z.keys()))
            a = z["arr_0"]
            flat = a.reshape(-1).astype(np.float64)
            save[f"f{i}_shape"] = np.array(a.shape)
            save[f"f{i}_dtype"] = np.array(str(a.dtype))
            save[f"f{i}_sum"] = np.array(flat.sum())
            save[f"f{i}_sample"] = flat[::max(1, flat.size // 2048)].copy()
        save["paths"] = np.array(paths)
        np.savez_compressed(os.path.join(out_dir, "control_save.npz"), **save)
        print("control_save golden:", len(paths), "files;", paths[:3], "...")
    finally:
        os.chdir(cwd)
        import shutil
        shutil.rmtree(tmp, ignore_errors=True)


def gen_align(out_dir):
    """lib/align.py::estimateSimilarityTransform (the reference function itself, global np.random seeded per case) on the
    seeded cases of rgbmanip_amd.synth.align_case, plus the bbox tail of interface_v5.py:348-374 built from the reference's
    get_3d_bbox / transform_coordinates_3d."""
    from rgbmanip_amd import synth
    from models.pose_estimator.AdaPose.lib.align import estimateSimilarityTransform
    from models.pose_estimator.AdaPose.lib.utils import get_3d_bbox, transform_coordinates_3d
    save = {}
    for case in range(5):
        nocs, pts = synth.align_case(case)
        np.random.seed(100 + case)
        ts, tr, tt, T = estimateSimilarityTransform(nocs, pts)
        save[f"c{case}_ok"] = np.array(ts is not None)
        if ts is None:
            continue
        save[f"c{case}_s"], save[f"c{case}_R"], save[f"c{case}_t"] = np.array(ts), tr, tt
        size = 2 * np.max(abs(nocs), axis=0) * ts
        bbox = get_3d_bbox(size)
        sRT = np.eye(4).astype(np.float32)
        sRT[:3, :3] = tr
        sRT[:3, 3] = tt.flatten()
        save[f"c{case}_bbox_cam"] = transform_coordinates_3d(bbox, sRT)
    np.savez_compressed(os.path.join(out_dir, "align.npz"), **save)
    print("align golden:", {k: np.asarray(v).shape for k, v in save.items()})


def gen_cv2(out_dir):
    """The OpenCV pin (round-3 verdict): wherever `import cv2` works, record what the reference's three OpenCV call sites return on
    seeded inputs — `cv2.resize` INTER_NEAREST / INTER_LINEAR of crop windows (interface_v5.py:91-94, 136-139) and
    `cv2.triangulatePoints`, `cv2.solvePnPRansac(flags=SOLVEPNP_EPNP)`, `cv2.solvePnPRefineVVS` on the cases of
    rgbmanip_amd.synth.pnp_case (lib/utils.py:121-195, lib/align.py:104-115) — into tests/golden/cv2_pin.npz.  The build image has
    no OpenCV, so there this target prints why it did nothing; tests/test_oracle_golden.py::test_cv2_pin compares the
    restatements (oracle/postproc_ref.py resize_*, oracle/pnp_ref.py) with the file whenever it exists."""
    try:
        import importlib
        sys.modules.pop("cv2", None)                       # the name stub of install_stubs() is not OpenCV
        cv2 = importlib.import_module("cv2")
        if not hasattr(cv2, "solvePnPRansac"):
            raise ImportError("cv2 is the import stub")
    except ImportError as e:
        print(f"cv2 golden: OpenCV is not importable here ({e}); nothing written.  Run `python tools/make_goldens.py cv2` in an "
              f"environment with opencv-python and commit tests/golden/cv2_pin.npz")
        return
    from rgbmanip_amd import synth
    save = {"cv2_version": np.array(cv2.__version__)}
    rng = np.random.default_rng(4242)
    for i, win in enumerate((200, 240, 280, 440)):
        img = rng.random((win, win, 3)).astype(np.float32)
        msk = (rng.random((win, win)) < 0.3).astype(np.float32)
        save[f"r{i}_img"], save[f"r{i}_mask"] = img, msk
        save[f"r{i}_linear"] = cv2.resize(img, (224, 224), interpolation=cv2.INTER_LINEAR)
        save[f"r{i}_nearest"] = cv2.resize(msk, (224, 224), interpolation=cv2.INTER_NEAREST)
    for case in range(5):
        c = synth.pnp_case(case)
        P1, P2 = c["K"] @ c["E1"][:3], c["K"] @ c["E2"][:3]
        X = cv2.triangulatePoints(P1, P2, c["pts1"][:64].T.astype(np.float64), c["pts2"][:64].T.astype(np.float64))
        save[f"p{case}_tri"] = X
        pw = (c["nocs1"].astype(np.float64) * c["scale"])
        cv2.setRNGSeed(100 + case)
        ok, rvec, tvec, inl = cv2.solvePnPRansac(pw, c["pts1"].astype(np.float64), c["K"], None, flags=cv2.SOLVEPNP_EPNP)
        save[f"p{case}_ok"] = np.array(bool(ok))
        if ok:
            rv, tv = cv2.solvePnPRefineVVS(pw[inl[:, 0]], c["pts1"].astype(np.float64)[inl[:, 0]], c["K"], None, rvec, tvec)
            save[f"p{case}_rvec"], save[f"p{case}_tvec"], save[f"p{case}_inliers"] = rvec, tvec, inl[:, 0]
            save[f"p{case}_rvec_vvs"], save[f"p{case}_tvec_vvs"] = rv, tv
    np.savez_compressed(os.path.join(out_dir, "cv2_pin.npz"), **save)
    print("cv2 golden:", cv2.__version__, {k: np.asarray(v).shape for k, v in save.items() if k != "cv2_version"})


if __name__ == "__main__":
    if sys.argv[1:] == ["cv2"]:                 # needs OpenCV, not the reference: no import stubs
        out_dir = os.path.join(ROOT, "tests", "golden")
        os.makedirs(out_dir, exist_ok=True)
        gen_cv2(out_dir)
        sys.exit(0)
    install_stubs()
    out_dir = os.path.join(ROOT, "tests", "golden")
    os.makedirs(out_dir, exist_ok=True)
    torch.set_num_threads(8)
    which = sys.argv[1:] or ["adapose", "adapose_trainbn", "postproc", "ppo", "ppo_run", "control", "control_step", "control_save", "align",
                             "ppo_variants", "adapose_dropout"]
    if "adapose_trainbn" in which:
        gen_adapose_trainbn(out_dir)
    net_out = inp = None
    if "adapose" in which or "postproc" in which:
        net_out, inp = gen_adapose(out_dir)
    if "postproc" in which:
        gen_postproc(out_dir, net_out, inp)
    if "ppo" in which:
        gen_ppo(out_dir)
    if "ppo_run" in which:
        gen_ppo_run(out_dir)
    if "ppo_variants" in which:
        gen_ppo_variants(out_dir)
    if "control" in which:
        gen_control(out_dir)
    if "control_step" in which:
        gen_control_step(out_dir)
    if "control_save" in which:
        gen_control_save(out_dir)
    if "align" in which:
        gen_align(out_dir)
    if "postproc_v4" in which:            # on request only: it reads the committed adapose_b2.npz and replaces cv2.resize / transforms
        gen_postproc_v4(out_dir)
    if "adapose_baseline" in which:       # on request only
        gen_adapose_baseline(out_dir)
    if "adapose_realworld" in which:      # on request only
        gen_adapose_realworld(out_dir)
    if "adapose_v2" in which:             # on request only
        gen_adapose_v2(out_dir)
    if "adapose_v1" in which:             # on request only
        gen_adapose_v1(out_dir)
    if "adapose_dropout" in which:       # last: its torch.manual_seed cannot reach the generators above
        gen_adapose_dropout(out_dir)
    print("done")
