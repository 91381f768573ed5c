"""Seeded synthetic weights and inputs for the AdaPose / PPO hot path.

There are no checkpoints in the container (reference `install.sh:1-16` downloads them), so
parity fixtures, GPU tests and bench.py all use weights generated here from numpy PCG64
streams keyed by the state_dict entry name.  The schema (names, shapes) is the one of the
reference module `StereoPoseNet_with_depth(n_cat=1, nv_pts=1024, regress_pose=True)`
(`models/pose_estimator/AdaPose/lib/network_v5.py:301-376`, `lib/pspnet.py:33-126`) and
of `ActorCritic` (`algo/ppo/ppo/module.py:8-67`); SURVEY.md Appendix A lists it.

The distributions mimic the reference's own initialisers so activations stay well scaled:
backbone Conv2d ~ N(0, sqrt(2/(k*k*out))) (`pspnet.py:45-48`), everything else PyTorch's
default U(+-1/sqrt(fan_in)); BatchNorm3d gets non-trivial affine/running stats so that
BN folding is really exercised.
"""
from __future__ import annotations

import zlib
from collections import OrderedDict

import numpy as np

IMG = 224
N_PTS = 1024
N_DEPTH = 24
IMAGENET_MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float64)
IMAGENET_STD = np.array([0.229, 0.224, 0.225], dtype=np.float64)


def _rng(name: str, seed: int) -> np.random.Generator:
    return np.random.default_rng((zlib.crc32(name.encode()) ^ (seed * 0x9E3779B1)) & 0xFFFFFFFF)


# --------------------------------------------------------------------------------------
# AdaPose schema
# --------------------------------------------------------------------------------------
def adapose_schema():
    """List of (name, shape, kind) in the reference's state_dict order."""
    s = []
    fe = "img_extractor.feats."
    s.append((fe + "conv1.weight", (64, 3, 7, 7), "bb"))
    inpl = 64
    for li, (planes, blocks) in enumerate(((64, 3), (128, 4), (256, 6), (512, 3)), start=1):
        for b in range(blocks):
            cin = inpl if b == 0 else planes
            s.append((f"{fe}layer{li}.{b}.conv1.weight", (planes, cin, 3, 3), "bb"))
            s.append((f"{fe}layer{li}.{b}.conv2.weight", (planes, planes, 3, 3), "bb"))
            if b == 0 and cin != planes:
                s.append((f"{fe}layer{li}.{b}.downsample.0.weight", (planes, cin, 1, 1), "bb"))
        inpl = planes
    for i in range(4):
        s.append((f"img_extractor.psp.stages.{i}.1.weight", (128, 512, 1, 1), "w"))
    for nm, cin, cout in (("up_1", 1024, 256), ("up_2", 256, 64), ("up_3", 64, 64)):
        s.append((f"img_extractor.{nm}.conv.0.weight", (cout, cin, 3, 3), "w"))
        s.append((f"img_extractor.{nm}.conv.0.bias", (cout,), "b:%d" % (cin * 9)))
        s.append((f"img_extractor.{nm}.conv.1.weight", (1,), "prelu"))
    s.append(("img_extractor.final.weight", (32, 64, 1, 1), "w"))
    s.append(("img_extractor.final.bias", (32,), "b:64"))
    s.append(("instance_color.0.weight", (64, 32, 1), "w"))
    s.append(("instance_color.0.bias", (64,), "b:32"))
    cr = "cost_regularization."

    def bn(prefix, c):
        return [(prefix + ".bn.weight", (c,), "bn_g"), (prefix + ".bn.bias", (c,), "bn_b"),
                (prefix + ".bn.running_mean", (c,), "bn_m"), (prefix + ".bn.running_var", (c,), "bn_v"),
                (prefix + ".bn.num_batches_tracked", (), "nbt")]

    for nm, cin, cout in (("conv0", 32, 8), ("conv1", 8, 16), ("conv2", 16, 16), ("conv3", 16, 32),
                          ("conv4", 32, 32), ("conv5", 32, 64), ("conv6", 64, 64)):
        s.append((f"{cr}{nm}.conv.weight", (cout, cin, 3, 3, 3), "w"))
        s += bn(cr + nm, cout)
    for nm, cin, cout in (("conv7", 64, 32), ("conv9", 32, 16), ("conv11", 16, 8)):
        # ConvTranspose3d weight is [in, out, k, k, k]; PyTorch's fan_in uses dim 1
        s.append((f"{cr}{nm}.conv.weight", (cin, cout, 3, 3, 3), "wT"))
        s += bn(cr + nm, cout)
    s.append((cr + "prob.weight", (1, 8, 3, 3, 3), "w"))

    def mlp(prefix, dims, idx, conv1d=True):
        out = []
        for i, (a, b) in zip(idx, zip(dims[:-1], dims[1:])):
            out.append((f"{prefix}.{i}.weight", (b, a, 1) if conv1d else (b, a), "w"))
            out.append((f"{prefix}.{i}.bias", (b,), "b:%d" % a))
        return out

    s += mlp("nocs_head", (64, 128, 64, 3), (0, 2, 4))
    s += mlp("nocs_pts_mlp", (3, 32, 64), (0, 2))
    s += mlp("pose_mlp1", (96, 128, 128), (0, 2))
    s += mlp("pose_mlp2", (256, 256, 256), (0, 2))
    s += mlp("rotation_estimator", (256, 256, 128, 6), (0, 2, 4), conv1d=False)
    s += mlp("translation_estimator", (256, 256, 128, 3), (0, 2, 4), conv1d=False)
    s += mlp("size_estimator", (256, 256, 128, 3), (0, 2, 4), conv1d=False)
    return s


def adapose_state_dict(seed: int = 0, prefix: str = "") -> "OrderedDict[str, np.ndarray]":
    """Synthetic checkpoint: name -> fp32 ndarray (int64 for num_batches_tracked)."""
    return _draw_state_dict(adapose_schema(), seed, prefix)


# Gain on the query and key projections (linears.0 / linears.1) of the baseline network's attention stack.  At torch's default init the
# softmax rows are all but uniform (mean largest probability 0.003 against 0.001 for uniform attention at 1024 keys), which cannot tell a
# correct softmax from none; the golden generator (tools/make_goldens.py: gen_adapose_baseline) asserts on the golden batch that the mean
# row maximum of every block lies in [0.2, 0.9] with this constant.
BASELINE_QK_GAIN = 4.0
BASELINE_DEPTH_BIAS = 0.5      # added to depth_head.4.bias: depths of the golden batch around 0.5, a few rows still zeroed by the ReLU


def baseline_schema(regress_pose: bool = True):
    """(name, shape, kind) of StereoPoseNet_with_depth_baseline (lib/network_baseline.py:523-607) in its state_dict order: v5's PSPNet,
    instance_color and nocs_head, then view_fusion, depth_head and - with regress_pose - the pose branch."""
    v5 = adapose_schema()
    by_prefix = lambda *pre: [e for e in v5 if e[0].startswith(pre)]
    s = by_prefix("img_extractor.", "instance_color.", "nocs_head.")
    for blk in range(4):
        for f in (1, 2):
            for l in range(4):
                p = f"view_fusion.blocks.{blk}.fusion{f}.linears.{l}"
                s.append((p + ".weight", (32, 32), "qk" if l < 2 else "w"))
                s.append((p + ".bias", (32,), "b:32"))
    for i, (a, b) in zip((0, 2, 4), ((32, 64), (64, 32), (32, 1))):
        s.append((f"depth_head.{i}.weight", (b, a, 1), "w"))
        # the last bias is shifted up: at the default draw the final ReLU zeroes every depth of the golden batch
        s.append((f"depth_head.{i}.bias", (b,), "b:%d" % a if i < 4 else "b+:%d" % a))
    if regress_pose:
        s += by_prefix("nocs_pts_mlp.", "pose_mlp1.", "pose_mlp2.", "rotation_estimator.", "translation_estimator.", "size_estimator.")
    return s


def baseline_state_dict(seed: int = 0, regress_pose: bool = True, prefix: str = "") -> "OrderedDict[str, np.ndarray]":
    """Synthetic checkpoint of the baseline network.  Every tensor it shares with `adapose_state_dict` is the same draw (the generator
    is keyed by the tensor's name), so the PSPNet goldens' distribution carries over; the attention stack's query / key weights are the
    default draw times BASELINE_QK_GAIN."""
    return _draw_state_dict(baseline_schema(regress_pose), seed, prefix)


def realworld_schema():
    """(name, shape, kind) of StereoPoseNet_with_depth_for_realdemo (lib/network_realworld.py:10-96) in its state_dict order: v5's
    entries with camera_pts_mlp in front of nocs_pts_mlp and pose_mlp1.0 reading 128 channels."""
    s = []
    for name, shape, kind in adapose_schema():
        if name == "nocs_pts_mlp.0.weight":
            for i, (a, b) in zip((0, 2), ((3, 32), (32, 64))):
                s.append((f"camera_pts_mlp.{i}.weight", (b, a, 1), "w"))
                s.append((f"camera_pts_mlp.{i}.bias", (b,), "b:%d" % a))
        if name == "pose_mlp1.0.weight":
            shape = (128, 128, 1)
        s.append((name, shape, kind))
    return s


def realworld_state_dict(seed: int = 0, prefix: str = "") -> "OrderedDict[str, np.ndarray]":
    """Synthetic checkpoint of the real-world network.  The generator is keyed by the tensor's name, so every tensor it shares with
    `adapose_state_dict(seed)` - all of v5's but pose_mlp1.0.weight, which is [128, 128, 1] here - is the same draw, and
    `adapose_state_dict` returns what it did."""
    return _draw_state_dict(realworld_schema(), seed, prefix)


# The v2 network's draw.  At the plain draw volume_conv.2's ReLU zeroes every value of the golden batch (and none at seed 1), and
# view1_s == view2_s to four decimals: a fixture that cannot tell a correct stereo part from none.  A gain on volume_conv.2.bn.weight, a
# shift on its bias and a gain on the two fuse_conv weights bring the last ReLU's clip share near one half and let the size output depend
# on the plane values; the golden generator (tools/make_goldens.py: gen_adapose_v2) asserts the resulting conditions on the golden batch.
V2_VC2_BN_GAIN = 16.0
V2_VC2_BN_SHIFT = 8.3
V2_FUSE_GAIN = 4.0


def v2_schema():
    """(name, shape, kind) of StereoPoseNet (lib/network_v2.py:40-102) in its state_dict order: v5's PSPNet and instance_color, then
    volume_conv, fuse_conv, nocs_head and the 64 / 128 wide size branch."""
    v5 = adapose_schema()
    by_prefix = lambda *pre: [e for e in v5 if e[0].startswith(pre)]      # noqa: E731
    s = by_prefix("img_extractor.", "instance_color.")
    for i, (a, b) in enumerate(((32, 16), (16, 8), (8, 1))):
        p = f"volume_conv.{i}"
        last = i == 2
        s.append((p + ".conv.weight", (b, a, 1, 1, 1), "w"))
        s += [(p + ".bn.weight", (b,), "v2_bn_g" if last else "bn_g"), (p + ".bn.bias", (b,), "v2_bn_b" if last else "bn_b"),
              (p + ".bn.running_mean", (b,), "bn_m"), (p + ".bn.running_var", (b,), "bn_v"), (p + ".bn.num_batches_tracked", (), "nbt")]
    for i, (a, b) in zip((0, 2), ((24, 32), (32, 64))):
        s.append((f"fuse_conv.{i}.weight", (b, a, 1, 1), "v2_fw"))
        s.append((f"fuse_conv.{i}.bias", (b,), "b:%d" % a))
    s += by_prefix("nocs_head.")
    for pre, dims, idx, conv1d in (("pose_mlp1", (64, 64, 64), (0, 2), True), ("pose_mlp2", (128, 128, 128), (0, 2), True),
                                   ("size_estimator", (128, 128, 64, 3), (0, 2, 4), False)):
        for i, (a, b) in zip(idx, zip(dims[:-1], dims[1:])):
            s.append((f"{pre}.{i}.weight", (b, a, 1) if conv1d else (b, a), "w"))
            s.append((f"{pre}.{i}.bias", (b,), "b:%d" % a))
    return s


def v2_state_dict(seed: int = 0, prefix: str = "") -> "OrderedDict[str, np.ndarray]":
    """Synthetic checkpoint of the v2 network.  The generator is keyed by the tensor's name, so the tensors it shares with
    `adapose_state_dict(seed)` (PSPNet, instance_color, nocs_head) are the same draws, and `adapose_state_dict` returns what it did."""
    return _draw_state_dict(v2_schema(), seed, prefix)


def v1_schema():
    """(name, shape, kind) of StereoPoseNet (lib/network.py:39-117) in its state_dict order: v5's PSPNet and instance_color, v2's
    volume_conv and fuse_conv (the latter ending in 32 channels), then v5's nocs_head, nocs_pts_mlp and pose branch with pose_mlp1.0
    reading 128 channels.  volume_conv and fuse_conv carry the v2 draw's offsets (V2_VC2_BN_GAIN, V2_VC2_BN_SHIFT, V2_FUSE_GAIN), for
    the same reason; the golden generator (tools/make_goldens.py: gen_adapose_v1) asserts the fixture conditions on the golden batch."""
    v5 = adapose_schema()
    by_prefix = lambda *pre: [e for e in v5 if e[0].startswith(pre)]      # noqa: E731
    s = by_prefix("img_extractor.", "instance_color.")
    s += [e for e in v2_schema() if e[0].startswith("volume_conv.")]
    for i, (a, b) in zip((0, 2), ((24, 32), (32, 32))):
        s.append((f"fuse_conv.{i}.weight", (b, a, 1, 1), "v2_fw"))
        s.append((f"fuse_conv.{i}.bias", (b,), "b:%d" % a))
    s += by_prefix("nocs_head.", "nocs_pts_mlp.")
    s += [(n, (128, 128, 1) if n == "pose_mlp1.0.weight" else shp, k) for n, shp, k in by_prefix("pose_mlp1.")]
    s += by_prefix("pose_mlp2.", "rotation_estimator.", "translation_estimator.", "size_estimator.")
    return s


def v1_state_dict(seed: int = 0, prefix: str = "") -> "OrderedDict[str, np.ndarray]":
    """Synthetic checkpoint of the v1 network.  The generator is keyed by the tensor's name, so the tensors it shares with
    `adapose_state_dict(seed)` and `v2_state_dict(seed)` are the same draws, and both return what they did."""
    return _draw_state_dict(v1_schema(), seed, prefix)


def realworld_coor(B: int, seed: int = 0, n_pts: int = N_PTS, W: int = 640, H: int = 480):
    """Chosen points' pixel coordinates in a W x H frame for the real-world network's goldens: (pts2d1, pts2d2) [B, n_pts, 2] float32
    with whole-pixel values (what prepare_model_input emits), and the normalised (coor1, coor2) = pts2d / (W, H) in float32."""
    g = _rng(f"realworld_coor.{B}.{n_pts}", seed)
    out = []
    for _ in range(2):
        p = np.stack([g.integers(0, W, size=(B, n_pts)), g.integers(0, H, size=(B, n_pts))], axis=-1).astype(np.float32)
        out.append(p)
    wh = np.array([W, H], dtype=np.float32)
    return out[0], out[1], out[0] / wh, out[1] / wh


def view_fusion_inputs(B: int, P: int, seed: int = 0):
    """Rows for the attention stack alone: (x1, x2) [B, P, 32] float32, N(0, 1)."""
    g = _rng(f"view_fusion_inputs.{B}.{P}", seed)
    return (np.ascontiguousarray(g.normal(size=(B, P, 32)), dtype=np.float32),
            np.ascontiguousarray(g.normal(size=(B, P, 32)), dtype=np.float32))


def _draw_state_dict(schema, seed: int, prefix: str):
    sd = OrderedDict()
    for name, shape, kind in schema:
        g = _rng(name, seed)
        if kind == "bb":
            n = shape[2] * shape[3] * shape[0]
            v = g.normal(0.0, np.sqrt(2.0 / n), size=shape)
        elif kind == "w":
            fan_in = int(np.prod(shape[1:]))
            bound = 1.0 / np.sqrt(fan_in)
            v = g.uniform(-bound, bound, size=shape)
        elif kind == "qk":
            bound = BASELINE_QK_GAIN / np.sqrt(shape[1])
            v = g.uniform(-bound, bound, size=shape)
        elif kind == "wT":
            fan_in = int(shape[1] * np.prod(shape[2:]))
            bound = 1.0 / np.sqrt(fan_in)
            v = g.uniform(-bound, bound, size=shape)
        elif kind.startswith("b:"):
            bound = 1.0 / np.sqrt(int(kind[2:]))
            v = g.uniform(-bound, bound, size=shape)
        elif kind.startswith("b+:"):
            bound = 1.0 / np.sqrt(int(kind[3:]))
            v = g.uniform(-bound, bound, size=shape) + BASELINE_DEPTH_BIAS
        elif kind == "v2_fw":
            bound = V2_FUSE_GAIN / np.sqrt(int(np.prod(shape[1:])))
            v = g.uniform(-bound, bound, size=shape)
        elif kind == "v2_bn_g":
            v = g.uniform(0.5, 1.5, size=shape) * V2_VC2_BN_GAIN
        elif kind == "v2_bn_b":
            v = g.normal(0.0, 0.1, size=shape) + V2_VC2_BN_SHIFT
        elif kind == "prelu":
            v = np.full(shape, 0.25)
        elif kind == "bn_g":
            v = g.uniform(0.5, 1.5, size=shape)
        elif kind == "bn_b":
            v = g.normal(0.0, 0.1, size=shape)
        elif kind == "bn_m":
            v = g.normal(0.0, 0.1, size=shape)
        elif kind == "bn_v":
            v = g.uniform(0.5, 1.5, size=shape)
        elif kind == "nbt":
            sd[prefix + name] = np.array(0, dtype=np.int64)
            continue
        else:  # pragma: no cover
            raise ValueError(kind)
        sd[prefix + name] = np.ascontiguousarray(v, dtype=np.float32)
    return sd


# --------------------------------------------------------------------------------------
# Synthetic estimator inputs
# --------------------------------------------------------------------------------------
def _lookat_extrinsic(eye, target, up=np.array([0.0, 0.0, 1.0])):
    """World->camera 4x4 (OpenCV convention: +z forward, +x right, +y down)."""
    f = target - eye
    f = f / np.linalg.norm(f)
    r = np.cross(f, up)
    r = r / np.linalg.norm(r)
    d = np.cross(f, r)
    R = np.stack([r, d, f], axis=0)
    E = np.eye(4)
    E[:3, :3] = R
    E[:3, 3] = -R @ eye
    return E


def adapose_inputs(B: int, seed: int = 0, img: int = IMG, n_pts: int = N_PTS):
    """Network-level inputs for B poses (stereo pairs).

    Returns dict of float32/int64 ndarrays:
      img1,img2 [B,3,img,img] normalised; choose1,choose2 [B,n_pts] int64;
      P1,P2 [B,4,4] float32 (K'.E[:3] padded); depths [B,24] float32;
      K1 [B,3,3] float64 cropped intrinsics of view 1; E1,E2 [B,4,4] float64.
    """
    g = np.random.default_rng(1234567 + seed)
    yy, xx = np.meshgrid(np.arange(img), np.arange(img), indexing="ij")
    imgs = np.empty((B, 2, 3, img, img), dtype=np.float32)
    choose = np.empty((B, 2, n_pts), dtype=np.int64)
    P = np.empty((B, 2, 4, 4), dtype=np.float32)
    Kc = np.empty((B, 2, 3, 3), dtype=np.float64)
    E = np.empty((B, 2, 4, 4), dtype=np.float64)
    fx = fy = 240.0 / np.tan(0.5)
    for b in range(B):
        target = g.uniform(-0.05, 0.05, size=3) + np.array([0.0, 0.0, 0.5])
        base_dir = g.normal(size=3)
        base_dir[2] = abs(base_dir[2]) * 0.3
        base_dir /= np.linalg.norm(base_dir)
        dist = g.uniform(0.55, 0.9)
        eye1 = target + base_dir * dist
        side = np.cross(base_dir, np.array([0.0, 0.0, 1.0]))
        side /= np.linalg.norm(side)
        eye2 = eye1 + side * g.uniform(0.15, 0.35) + np.array([0, 0, g.uniform(-0.05, 0.05)])
        for v, eye in enumerate((eye1, eye2)):
            rgb = g.random((3, img, img))
            smooth = np.zeros((img, img))
            for _ in range(4):
                fxy = g.uniform(0.5, 3.0, size=2) * 2 * np.pi / img
                ph = g.uniform(0, 2 * np.pi)
                smooth += np.cos(fxy[0] * xx + fxy[1] * yy + ph)
            rgb = np.clip(0.5 * rgb + 0.5 * (0.5 + 0.125 * smooth)[None], 0.0, 1.0)
            rgb = (rgb - IMAGENET_MEAN[:, None, None]) / IMAGENET_STD[:, None, None]
            imgs[b, v] = rgb.astype(np.float32)
            cy, cx = g.uniform(80, 144, size=2) * img / 224.0
            ay, ax = g.uniform(30, 90, size=2) * img / 224.0
            mask = ((yy - cy) / ay) ** 2 + ((xx - cx) / ax) ** 2 <= 1.0
            idx = np.flatnonzero(mask.ravel())
            idx = idx[g.permutation(idx.size)]
            if idx.size >= n_pts:
                ch = np.sort(idx[:n_pts])
            else:
                ch = np.pad(np.sort(idx), (0, n_pts - idx.size), "wrap")
            choose[b, v] = ch
            # crop window of the 480x640 frame -> cropped intrinsics (interface_v5.py:153-168)
            w = float(g.integers(5, 12) * 40)  # 200..440
            ratio = img / w
            K = np.eye(3)
            K[0, 0] = fx * ratio
            K[1, 1] = fy * ratio
            # the look-at target sits on the optical axis; keep the cropped principal
            # point near the crop centre so the handle projects inside both crops
            K[0, 2] = img / 2 + g.uniform(-20, 20)
            K[1, 2] = img / 2 + g.uniform(-20, 20)
            Ex = _lookat_extrinsic(eye, target)
            Kc[b, v] = K
            E[b, v] = Ex
            Pm = np.eye(4)
            Pm[:3, :] = K @ Ex[:3, :]
            P[b, v] = Pm.astype(np.float32)
    depths = np.tile(np.arange(0.1, 0.1 * (N_DEPTH - 0.5) + 0.1, 0.1, dtype=np.float32)[None], (B, 1))
    return {
        "img1": np.ascontiguousarray(imgs[:, 0]), "img2": np.ascontiguousarray(imgs[:, 1]),
        "choose1": np.ascontiguousarray(choose[:, 0]), "choose2": np.ascontiguousarray(choose[:, 1]),
        "P1": np.ascontiguousarray(P[:, 0]), "P2": np.ascontiguousarray(P[:, 1]),
        "depths": depths,
        "K1": np.ascontiguousarray(Kc[:, 0]), "K2": np.ascontiguousarray(Kc[:, 1]),
        "E1": np.ascontiguousarray(E[:, 0]), "E2": np.ascontiguousarray(E[:, 1]),
    }


# --------------------------------------------------------------------------------------
# PPO
# --------------------------------------------------------------------------------------
def sphere_depth(K_crop, E, center=(0.0, 0.0, 0.5), radius: float = 0.12, img: int = IMG):
    """Depth maps of a sphere ray-cast into cameras: K_crop [n,3,3], E [n,4,4] (world -> camera) -> [n,img,img] float32, the camera z of
    the first intersection of every pixel's ray, NaN off the sphere.  The scene of the two-view consistency tests."""
    K, E = np.asarray(K_crop, dtype=np.float64), np.asarray(E, dtype=np.float64)
    n = K.shape[0]
    y, x = np.meshgrid(np.arange(img, dtype=np.float64), np.arange(img, dtype=np.float64), indexing="ij")
    out = np.full((n, img, img), np.nan, dtype=np.float32)
    for i in range(n):
        c = E[i, :3, :3] @ np.asarray(center, dtype=np.float64) + E[i, :3, 3]          # the centre in the camera frame
        r = np.stack([(x - K[i, 0, 2]) / K[i, 0, 0], (y - K[i, 1, 2]) / K[i, 1, 1], np.ones_like(x)], axis=-1)      # rays with z = 1
        a, b = (r * r).sum(-1), r @ c
        disc = b * b - a * (c @ c - radius * radius)
        with np.errstate(invalid="ignore"):
            z = (b - np.sqrt(disc)) / a                                                   # ray parameter = camera z
        hit = (disc >= 0) & (z > 0)
        out[i][hit] = z[hit].astype(np.float32)
    return out


def policy_state_dict(seed: int = 0, obs=60, act=12, hid=(96, 96, 32), init_std=0.6):
    """ActorCritic state_dict in the reference's key order (`module.py:24-54`)."""
    sd = OrderedDict()
    sd["log_std"] = np.full((act,), np.log(init_std), dtype=np.float32)
    for net, out_dim, gains in (("actor", act, [np.sqrt(2)] * len(hid) + [0.01]),
                                ("critic", 1, [np.sqrt(2)] * len(hid) + [1.0])):
        dims = (obs,) + tuple(hid) + (out_dim,)
        for li, (a, b) in enumerate(zip(dims[:-1], dims[1:])):
            g = _rng(f"{net}.{2 * li}", seed)
            m = g.normal(size=(max(a, b), min(a, b)))
            q, r = np.linalg.qr(m)
            q = q * np.sign(np.diag(r))[None]
            w = q if b >= a else q.T
            sd[f"{net}.{2 * li}.weight"] = np.ascontiguousarray(gains[li] * w[:b, :a], dtype=np.float32)
            bound = 1.0 / np.sqrt(a)
            sd[f"{net}.{2 * li}.bias"] = g.uniform(-bound, bound, size=(b,)).astype(np.float32)
    return sd


# the ActorCritic variants of tests/golden/ppo_variants.npz (tools/make_goldens.py::gen_ppo_variants): name -> (model_cfg or
# None for the class default, asymmetric, use_clipped_value_loss); observation 60, state 75, action 12 throughout
PPO_VARIANTS = OrderedDict([
    ("default", (None, False, True)),
    ("asym_tanh", (dict(pi_hid_sizes=[128, 64], vf_hid_sizes=[256, 128, 64, 32], activation="tanh"), True, True)),
    ("lrelu64_mse", (dict(pi_hid_sizes=[64], vf_hid_sizes=[64], activation="lrelu"), False, False)),
    ("relu", (dict(pi_hid_sizes=[96, 96, 32], vf_hid_sizes=[96, 96, 32], activation="relu"), False, True)),
    ("sigmoid", (dict(pi_hid_sizes=[96, 96, 32], vf_hid_sizes=[96, 96, 32], activation="sigmoid"), False, True)),
    ("selu", (dict(pi_hid_sizes=[96, 96, 32], vf_hid_sizes=[96, 96, 32], activation="selu"), False, True)),
    ("awkward", (dict(pi_hid_sizes=[33, 7, 130], vf_hid_sizes=[5], activation="elu"), False, True)),
])


def policy_variant_state_dict(name: str, seed: int = 0, obs=60, states=75, act=12, init_std=0.6):
    """Seeded state_dict of one of PPO_VARIANTS in the reference's key order: scaled orthogonal weights with the reference's
    gains, uniform biases (as `policy_state_dict` builds the shipped shape)."""
    cfg, asym, _ = PPO_VARIANTS[name]
    pi, vf = ([256] * 3, [256] * 3) if cfg is None else (cfg["pi_hid_sizes"], cfg["vf_hid_sizes"])
    sd = OrderedDict()
    sd["log_std"] = np.full((act,), np.log(init_std), dtype=np.float32)
    for net, in_dim, hid, out_dim, last in (("actor", obs, pi, act, 0.01), ("critic", states if asym else obs, vf, 1, 1.0)):
        dims = (in_dim,) + tuple(hid) + (out_dim,)
        gains = [np.sqrt(2)] * len(hid) + [last]
        for li, (a, b) in enumerate(zip(dims[:-1], dims[1:])):
            g = _rng(f"variant.{name}.{net}.{2 * li}", seed)
            q, r = np.linalg.qr(g.normal(size=(max(a, b), min(a, b))))
            q = q * np.sign(np.diag(r))[None]
            w = q if b >= a else q.T
            sd[f"{net}.{2 * li}.weight"] = np.ascontiguousarray(gains[li] * w[:b, :a], dtype=np.float32)
            bound = 1.0 / np.sqrt(a)
            sd[f"{net}.{2 * li}.bias"] = g.uniform(-bound, bound, size=(b,)).astype(np.float32)
    return sd


def ppo_rollout(T: int, N: int, seed: int = 0, obs=60, states=75, act=12):
    """A recorded rollout with plausible statistics (rewards ~ reference reward scale)."""
    g = np.random.default_rng(777 + seed)
    r = {
        "observations": g.uniform(-1.0, 1.0, size=(T, N, obs)).astype(np.float32),
        "states": g.uniform(-1.0, 1.0, size=(T, N, states)).astype(np.float32),
        "actions": g.normal(0, 0.5, size=(T, N, act)).astype(np.float32),
        "rewards": g.normal(2.0, 3.0, size=(T, N, 1)).astype(np.float32),
        "dones": (g.random((T, N, 1)) < 0.2).astype(np.uint8),
        "values": g.normal(1.0, 2.0, size=(T, N, 1)).astype(np.float32),
        "last_values": g.normal(1.0, 2.0, size=(N, 1)).astype(np.float32),
    }
    return r


# --------------------------------------------------------------------------- ControlInterface view stream
def control_view(num_envs: int, step: int, seed: int = 0, H: int = 480, W: int = 640):
    """One seeded `MultiVecEnv.get_image()` result + camera pose + GT box for the view-queue tests and goldens.

    Colour frames are a per-(step, env) constant plus a faint ramp so a captured frame identifies its origin; masks are
    rectangles, with env 1 empty at step 2 and every env empty at step 4 (the reference's global `if p_env.shape[0]` branch)."""
    rng = np.random.default_rng(seed * 1000 + step)
    color = np.empty((num_envs, H, W, 3), dtype=np.float32)
    ramp = (np.arange(W, dtype=np.float32) / (8.0 * W))[None, :, None]
    mask = np.zeros((num_envs, H, W), dtype=bool)
    for e in range(num_envs):
        color[e] = (step * 16 + e + 1) / 256.0 + ramp
        if step == 4 or (step == 2 and e == 1):
            continue
        r0, c0 = int(rng.integers(20, 300)), int(rng.integers(20, 400))
        mask[e, r0:r0 + int(rng.integers(30, 150)), c0:c0 + int(rng.integers(30, 200))] = True
    K = np.tile(np.array([[439.31, 0, 320.0], [0, 439.31, 240.0], [0, 0, 1.0]]), (num_envs, 1, 1)) + rng.normal(0, 0.1, (num_envs, 3, 3))
    E = np.tile(np.eye(4), (num_envs, 1, 1))
    E[:, :3, :] += rng.normal(0, 0.2, (num_envs, 3, 4))
    pose = rng.normal(0, 0.5, (num_envs, 7))
    gt = rng.normal(0, 0.3, (num_envs, 8, 3))
    image = {"camera0": {"Color": color, "Mask": mask, "Intrinsic": K, "Extrinsic": E}}
    return image, pose, gt


def crop_frames(seed: int = 0, H: int = 480, W: int = 640):
    """Two seeded 8-bit camera frames for the crop goldens and tests of the adapose_v4 transform (tests/golden/postproc_v4.npz):
    (rgb [2,H,W,3] uint8, mask [2,H,W] uint8, K [2,3,3]).  Frame 0: a large ellipse (more than 1024 resized mask pixels, a 440
    window); frame 1: a thin sliver at the right border (fewer than 1024: wrap padding, an 80 window shifted back into the frame)."""
    rng = np.random.default_rng(seed * 1000 + 4004)
    yy, xx = np.mgrid[0:H, 0:W]
    base = 128.0 + 60.0 * np.cos(xx / 23.0)[None, :, :, None] + 40.0 * np.sin(yy / 17.0)[None, :, :, None]
    rgb = np.clip(np.rint(base + rng.normal(0.0, 25.0, (2, H, W, 3))), 0, 255).astype(np.uint8)
    mask = np.zeros((2, H, W), dtype=np.uint8)
    mask[0] = (((yy - 250) / 120.0) ** 2 + ((xx - 300) / 170.0) ** 2) < 1.0
    mask[1] = (((yy - 200) / 22.0) ** 2 + ((xx - 630) / 1.6) ** 2) < 1.0
    K = np.tile(np.array([[439.31, 0, 320.0], [0, 439.31, 240.0], [0, 0, 1.0]]), (2, 1, 1))
    K[1, 0, 2] += 1.5
    return rgb, mask, K


CONTROL_REWARD_CFG = {            # cfg/controller/rl.yaml:11-26, verbatim
    "diff_coef": -0.5, "move_success_coef": 8.0, "move_period_coef": -0.0, "far_coef": -2.5, "ori_coef": 0.25,
    "xyz_lookat_coef": -0.05, "bbox_coef": -1.0, "bbox_boundary_coef": -1.0, "have_bbox_coef": 2.0, "center_coef": 12.0,
    "open_coef": 8.0, "view_coef": 0.5, "view_norm_coef": -0.3, "success_coef": 0.0,
}


def control_cfg(task: str = "cabinet", success_coef: float = 0.0):
    """The slice of the merged yaml config `ControlInterface` reads (cfg/controller/rl.yaml:3-26, cfg/task/*.yaml name)."""
    reward = dict(CONTROL_REWARD_CFG)
    reward["success_coef"] = success_coef
    return {"controller": {"max_steps": 4, "action_type": "pose", "pose_min": [-0.3, -0.3, 0.4], "pose_max": [0.3, 0.3, 1.0],
                           "early_stop": 4},
            "reward": reward, "task": {"name": task}}


def control_actions(num_envs: int, step: int, seed: int = 0, act: int = 12):
    """Seeded policy actions (float32, as `ActorCritic.act` returns them) for the ControlInterface.step goldens; row 0 of
    step 3 carries a large z offset so the pose clip of rl_pose.py:406 is exercised."""
    a = np.random.default_rng(seed * 1000 + 700 + step).normal(0, 0.6, (num_envs, act)).astype(np.float32)
    if step == 3:
        a[0, 2] = 2.5
    return a


class ReplayVecEnv:
    """Deterministic numpy stand-in for the slice of `MultiVecEnv` that `ControlInterface` calls (`env/my_vec_env.py:214,
    266, 281, 382, 466, 482`): every answer is a seeded function of the call count, so the reference class (golden
    generator), the oracle and the device implementation can be driven through identical episodes.  Calls are recorded."""

    def __init__(self, num_envs: int, seed: int = 0):
        self.num_envs, self.seed = num_envs, seed
        self.t = 0
        self.cur = None
        self.moves, self.resets = [], 0
        self._robot = np.random.default_rng(seed * 1000 + 900).normal(0, 0.2, (num_envs, 7))

    def cam_move_to(self, pose, time=2, wait=1, planner="ik", robot_frame=False, skip_move=False, no_collision_with_front=True):
        rng = np.random.default_rng(self.seed * 1000 + 500 + self.t)
        pose = pose.detach().cpu().numpy() if hasattr(pose, "detach") else pose
        self.moves.append(dict(pose=np.array(pose, dtype=np.float64), time=time, wait=wait, planner=planner,
                               robot_frame=robot_frame, skip_move=skip_move, no_collision_with_front=no_collision_with_front))
        return [(rng.random(self.num_envs) > 0.25), rng.integers(1, 2000, self.num_envs)]     # merge_obs of (bool, int) tuples

    def get_image(self, mask="handle"):
        self.cur = control_view(self.num_envs, self.t, self.seed)
        self.t += 1
        return self.cur[0]

    def camera_pose(self, robot_frame=False):
        return self.cur[1]

    def robot_pose(self):
        return self._robot

    def get_observation(self, gt=False):
        rng = np.random.default_rng(self.seed * 1000 + 300 + self.t)
        return {"handle_bbox": self.cur[2], "success": (rng.random((self.num_envs, 1)) > 0.5).astype(np.float64)}

    def reset(self, indices=None):
        self.resets += 1
        return None

    def get_attr(self, attr_name, indices=None):
        """`SubprocVecEnv.get_attr` (`env/my_vec_env.py:466`): one entry per env.  Only `current_obj_config` (read by the
        eval-time dataset export, `rl_pose.py:58`) is known: two object names that change with every reset."""
        if attr_name != "current_obj_config":
            raise AttributeError(attr_name)
        return [{"name": f"obj{(e + self.resets) % 2}"} for e in range(self.num_envs)]


# --------------------------------------------------------------------------- similarity alignment cases
def align_case(case: int, P: int = 1024):
    """Seeded (nocs, camera points) pair for the Umeyama-RANSAC tests: points = s R nocs + t + noise, a fraction of outliers.
    case 3 is pure noise (the reference returns None), case 4 has mirrored points so the SVD's reflection fix is taken."""
    rng = np.random.default_rng(4200 + case)
    nocs = rng.uniform(-0.5, 0.5, (P, 3)).astype(np.float32) * np.array([0.9, 0.5, 0.3], dtype=np.float32)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] *= -1
    s, t = rng.uniform(0.15, 0.5), rng.uniform(-0.3, 0.3, 3) + np.array([0, 0, 0.9])
    pts = s * nocs.astype(np.float64) @ q.T + t + rng.normal(0, 0.002, (P, 3))
    out_frac = [0.0, 0.2, 0.45, 1.0, 0.1][case % 5]
    bad = rng.random(P) < out_frac
    pts[bad] = rng.uniform(-0.5, 0.5, (int(bad.sum()), 3)) + np.array([0, 0, 0.9])
    if case % 5 == 4:
        pts[:, 0] = -pts[:, 0]
    return nocs, pts


def pnp_case(case: int, P: int = 1024):
    """Seeded two-view case for the `use_depth: False` (NOCS matches -> triangulation -> EPnP-RANSAC) branch of predict
    (interface_v5.py:340-346): an object of scale s at pose (R_o, t_o) in the world, seen by two look-at cameras; per view the
    predicted NOCS of P surface points (+ noise) and their pixels in the 480x640 frame.  View 2 re-observes most of view 1's
    points (so that mutual nearest neighbours in NOCS space exist) in another order; a fraction of view 1's pixels are outliers.
    case 3 has no common points (no match -> default bbox).  Returns a dict incl. the ground truth (scale, R, t) in camera 1."""
    rng = np.random.default_rng(7300 + case)
    dims = np.array([0.9, 0.5, 0.3], dtype=np.float32)
    nocs = (rng.uniform(-0.5, 0.5, (P, 3)).astype(np.float32) * dims)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] *= -1
    s = float(rng.uniform(0.25, 0.5))
    t_o = rng.uniform(-0.05, 0.05, 3) + np.array([0.0, 0.0, 0.4])
    world = s * nocs.astype(np.float64) @ q.T + t_o
    eye1 = t_o + np.array([0.75, 0.1, 0.25]) * rng.uniform(0.9, 1.1)
    eye2 = eye1 + np.array([-0.1, 0.3, 0.05]) * rng.uniform(0.8, 1.2)
    E1, E2 = _lookat_extrinsic(eye1, t_o), _lookat_extrinsic(eye2, t_o)
    f = 240.0 / np.tan(0.5)
    K = np.array([[f, 0, 320.0], [0, f, 240.0], [0, 0, 1.0]])

    def project(E, X):
        c = X @ E[:3, :3].T + E[:3, 3]
        uv = c @ K.T
        return uv[:, :2] / uv[:, 2:3]
    noise = [0.0005, 0.001, 0.002, 0.001, 0.001][case % 5]
    pix = [0.2, 0.4, 0.8, 0.4, 0.4][case % 5]
    nocs1 = (nocs + rng.normal(0, noise, nocs.shape)).astype(np.float32)
    pts1 = (project(E1, world) + rng.normal(0, pix, (P, 2))).astype(np.float32)
    bad = rng.random(P) < [0.0, 0.1, 0.25, 0.1, 0.05][case % 5]
    pts1[bad] = rng.uniform([100, 60], [540, 420], (int(bad.sum()), 2)).astype(np.float32)
    perm = rng.permutation(P)
    if case % 5 == 3:
        nocs_b = (rng.uniform(-0.5, 0.5, (P, 3)).astype(np.float32) * dims) + np.float32(2.0)      # nothing in common with view 1
        world_b = s * nocs_b.astype(np.float64) @ q.T + t_o
    else:
        nocs_b, world_b = nocs[perm], world[perm]
        fresh = rng.random(P) < 0.3                      # 30 % of view 2 are other surface points
        nocs_b = np.where(fresh[:, None], rng.uniform(-0.5, 0.5, (P, 3)).astype(np.float32) * dims, nocs_b).astype(np.float32)
        world_b = np.where(fresh[:, None], s * nocs_b.astype(np.float64) @ q.T + t_o, world_b)
    nocs2 = (nocs_b + rng.normal(0, noise, nocs_b.shape)).astype(np.float32)
    pts2 = (project(E2, world_b) + rng.normal(0, pix, (P, 2))).astype(np.float32)
    R_gt = E1[:3, :3] @ q
    t_gt = E1[:3, :3] @ t_o + E1[:3, 3]
    return dict(nocs1=nocs1, pts1=pts1, nocs2=nocs2, pts2=pts2, K=K, E1=E1, E2=E2, scale=s, R=R_gt, t=t_gt)


# --------------------------------------------------------------------------- a deterministic vec env for PPO.run
class StubVecEnv:
    """A closed-form stand-in for `MultiVecEnv` with the interface `PPO.run` uses (`reset`, `step`, `get_state`, `num_envs`, the three
    spaces): smooth dynamics in float32 on the CPU, per-env episode lengths, a reward, and an info dict with reward terms and the
    specially handled "success_rate" key.  The SAME class drives the reference's `PPO.run` when the golden file is generated
    (tools/make_goldens.py::gen_ppo_run) and the product's in tests/test_gpu_ppo.py, so both see identical environment arithmetic;
    every action it receives is recorded in `action_log`."""

    def __init__(self, num_envs, box, seed=0):
        import torch
        g = np.random.default_rng(4242 + seed)
        self.num_envs = num_envs
        self.observation_space, self.state_space, self.action_space = box(-1.5, 1.5, (60,)), box(-1.5, 1.5, (75,)), box(-1.5, 1.5, (12,))
        self.Wa = torch.from_numpy((g.normal(size=(12, 75)) * 0.3).astype(np.float32))
        self.Ws = torch.from_numpy((g.normal(size=(75, 75)) * (0.5 / np.sqrt(75.0))).astype(np.float32))
        self.Po = torch.from_numpy((g.normal(size=(75, 60)) * (1.0 / np.sqrt(75.0))).astype(np.float32))
        self.s0 = torch.from_numpy(g.uniform(-0.5, 0.5, size=(num_envs, 75)).astype(np.float32))
        self.ep_len = torch.tensor([5 + (e % 7) for e in range(num_envs)], dtype=torch.int64)
        self.s = self.s0.clone()
        self.cnt = torch.zeros(num_envs, dtype=torch.int64)
        self.action_log = []

    def _obs(self):
        import torch
        return torch.tanh(self.s @ self.Po)

    def reset(self):
        self.s = self.s0.clone()
        self.cnt.zero_()
        return self._obs()

    def get_state(self):
        return self.s.clone()

    def step(self, actions):
        import torch
        a = actions.detach().to("cpu", torch.float32)
        self.action_log.append(a.clone())
        a = a.clamp(-1.5, 1.5)
        self.s = 0.85 * self.s + 0.15 * torch.tanh(a @ self.Wa + self.s @ self.Ws)
        self.cnt += 1
        dist = (self.s[:, :3] ** 2).sum(1)
        rew = 1.0 - dist + 0.05 * a.mean(1)
        done = self.cnt >= self.ep_len
        infos = {"REW:dist": dist.clone(), "REW:act": a.abs().mean(1), "successes": (rew > 0.8).float(),
                 "success_rate": (dist < 0.2).float()}
        self.s = torch.where(done[:, None], self.s0, self.s)
        self.cnt = torch.where(done, torch.zeros_like(self.cnt), self.cnt)
        return self._obs(), rew, done.to(torch.int64), infos
