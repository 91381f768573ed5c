"""GPU: the v2 network (rgbm_adapose_create_v2) - point selection at native resolution, the per-point plane-sweep head alone, the forward
against the reference's golden in every storage type, and `AdaPoseEstimator_v2`.  References: tests/golden/adapose_v2_b2.npz (the
reference class itself) and tests/v2_ref.py (float64 network, numpy prepare)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import v2_ref  # noqa: E402
from test_v2_host import prepare_masks  # noqa: E402

from oracle.pnp_ref import DEFAULT_BBOX  # noqa: E402
from rgbmanip_amd import _lib, synth  # noqa: E402
from rgbmanip_amd.adapose import AdaPoseNet, postprocess_pnp_scaled, prepare_inputs  # noqa: E402

pytestmark = pytest.mark.gpu
B, S, D, P = 2, 224, 24, 1024
EPS = {"fp32": 2.0 ** -24, "bf16": 2.0 ** -9, "fp16": 2.0 ** -12, "bf16x3": 2.0 ** -17}      # half a unit in the last place of the storage type, relative
KINDS = v2_ref.TAP_KEYS
_CACHE = {}


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "adapose_v2_b2.npz"))


@pytest.fixture(scope="module")
def sd():
    return synth.v2_state_dict(seed=0)


@pytest.fixture(scope="module")
def inputs():
    return dict(synth.adapose_inputs(B, seed=0))


def _maps(feat_nhwc):
    """[2B, S, S, 32] (the kernels' layout, view-1 poses first) -> the restatement's (feat1, feat2) [B, 32, S, S]"""
    f = torch.as_tensor(feat_nhwc).permute(0, 3, 1, 2).contiguous()
    return f[: f.shape[0] // 2], f[f.shape[0] // 2:]


@pytest.fixture(scope="module")
def cpu_ref(sd, inputs, golden):
    """Computed once on the CPU.  e64[k]: the golden against the float64 restatement, per tensor (the reference's own float32 rounding);
    gate32(k) = max(8 e64[k], 3e-6), the project's bound for a float32 computation of that tensor; kind_gate(kind): the same from the
    smaller e64 of the two views' tensors of that kind, for the kernel on maps of its own.  amp[k]: how far the float64 restatement's
    output k moves when the feature maps are rounded to bfloat16, over that rounding's own size, times the project's margin of 4."""
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    sd64 = v2_ref.to_sd(sd, torch.float64)
    taps = {}
    out = v2_ref.v2_forward(sd64, inputs["img1"], inputs["choose1"], inputs["img2"], inputs["choose2"], inputs["P1"], inputs["P2"], inputs["depths"], taps=taps)
    ref = {k: v.numpy() for k, v in out.items()}
    for v in (1, 2):
        for kind in KINDS:
            ref[f"v{v}_{kind}"] = taps[f"v{v}_{kind}"].numpy()
            ref[f"v{v}_{kind}_slice"] = v2_ref.points_slice(taps[f"v{v}_{kind}"]).numpy()
    ref["feat"] = torch.cat((taps["feat1"], taps["feat2"])).permute(0, 2, 3, 1).contiguous().numpy()
    keys = v2_ref.OUT_KEYS + [f"v{v}_{kind}_slice" for v in (1, 2) for kind in KINDS]
    e64 = {k: v2_ref.rel_err(golden[k], ref[k]) for k in keys}
    rounded_feat = torch.from_numpy(ref["feat"]).float().to(torch.bfloat16).double()
    f1, f2 = _maps(rounded_feat)
    rounded = {k: v.numpy() for k, v in v2_ref.heads_on_maps(sd64, f1, f2, inputs["choose1"], inputs["choose2"], inputs["P1"], inputs["P2"],
                                                            inputs["depths"]).items()}
    fe = v2_ref.rel_err(rounded_feat.numpy(), ref["feat"])
    amp = {k: 4 * v2_ref.rel_err(rounded[k], ref[k]) / fe for k in v2_ref.OUT_KEYS}
    print("e_ref64 per tensor:", e64)
    print("bf16 feature rounding", fe, "amplification factors (x4 margin included):", amp)
    assert all(np.isfinite(a) and a < 400 for a in amp.values()), amp      # above that the fixture is ill-conditioned, not the kernels
    return dict(ref=ref, e64=e64, amp=amp, sd64=sd64, gate32=lambda k: max(8 * e64[k], 3e-6),
                kind_gate=lambda kind: max(8 * min(e64[f"v{v}_{kind}_slice"] for v in (1, 2)), 3e-6))


def _net(sd, dtype, **kw):
    key = (dtype, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _CACHE:
        _CACHE[key] = AdaPoseNet(sd, dtype=dtype, arch="v2", **kw)
    return _CACHE[key]


def _run(net, inp):
    out = net(inp["img1"], inp["choose1"], inp["img2"], inp["choose2"], inp["P1"], inp["P2"], inp["depths"])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _taps(net):
    """planes / fuse / rows of the last forward, [2B, P, C] each (views [view-1 poses ; view-2 poses])"""
    return {kind: net.fetch(B, "v2_" + kind, 2 * B * P * c).view(2 * B, P, c).cpu().numpy() for kind, c in zip(KINDS, (D, 64, 64))}


# ------------------------------------------------------------------------------------------------------------------ (a) prepare
PREP_SEED = 11


def _prep_case():
    """Eight 480 x 640 frames, one per mask of tests/test_v2_host.prepare_masks() plus an empty one: 8-bit pixels and their float32 values."""
    if "prep" not in _CACHE:
        masks = prepare_masks()
        names = list(masks) + ["empty"]
        m = np.stack([masks[n] if n in masks else np.zeros((480, 640), np.uint8) for n in names])
        g = np.random.default_rng(7)
        u8 = g.integers(0, 256, size=(len(names), 480, 640, 3), dtype=np.uint8)
        K = np.tile(np.array([[439.31, 0, 320.0], [0, 439.31, 240.0], [0, 0, 1.0]])[None], (len(names), 1, 1))
        K[:, 0, 2] += np.arange(len(names))
        f32 = u8.astype(np.float32) / np.float32(255)
        want = [v2_ref.prepare_model_input(f32[f], m[f], K[f], S, seed=PREP_SEED, frame=f) for f in range(len(names))]
        _CACHE["prep"] = dict(names=names, mask=m, u8=u8, f32=f32, K=K, want=want)
    return _CACHE["prep"]


def _prep_check(got, want, f, tag):
    view, choose, pts2d, Kn, window = want
    if view is None:
        assert got["valid"][f] == 0 and not got["choose"][f].any() and not got["pts2d"][f].any() and np.isfinite(got["img"][f]).all(), tag
        return
    assert got["valid"][f] == 1, tag
    assert np.array_equal(got["choose"][f], choose.astype(np.int32)), tag
    assert np.array_equal(_bits(got["pts2d"][f]), _bits(pts2d.astype(np.float32))), tag
    assert np.array_equal(got["Kcrop"][f], Kn) and tuple(got["window"][f]) == tuple(window), tag
    assert np.array_equal(_bits(got["img"][f]), _bits(view.astype(np.float32))), tag


@pytest.mark.parametrize("pixels", ["f32", "u8"])
def test_prepare_native_is_the_restatement_bit_for_bit(pixels):
    """prepare_inputs(sample="native") on float32 and on 8-bit frames against tests/v2_ref.prepare_model_input: a 40-window, the full
    440-window (193 600 candidates: native indices beyond 16 bits, duplicates in `choose`), n = 1, 1024 and 1025, a mask touching the frame's
    edge, an ellipse and an empty mask.  choose, pts2d, Kcrop, window, valid and the image, all bit for bit; image, Kcrop and window are
    also those of the resized-mask sampling."""
    c = _prep_case()
    rgb, mask, K = _cuda(c[pixels]), _cuda(c["mask"]), _cuda(c["K"])
    out = prepare_inputs(rgb, mask, K, S, P, PREP_SEED, want_pts2d=True, sample="native")
    old = prepare_inputs(rgb, mask, K, S, P, PREP_SEED, want_pts2d=True)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for f, name in enumerate(c["names"]):
        _prep_check(got, c["want"][f], f, name)
    for k in ("img", "Kcrop", "window"):
        assert np.array_equal(_bits(got[k]), _bits(old[k].cpu().numpy())), k
    full = c["names"].index("window440_full")
    assert len(np.unique(got["choose"][full])) < P and got["pts2d"][full].max() > 256
    assert got["valid"].tolist() == [1] * (len(c["names"]) - 1) + [0]


def test_prepare_native_frame_map_and_frame0():
    """A frame_map with a negative entry (a missing view: zeros, valid 0) that reads the pool out of order, and two calls with frame0
    that equal one call."""
    c = _prep_case()
    n = len(c["names"])
    rgb, mask, K = _cuda(c["u8"]), _cuda(c["mask"]), _cuda(c["K"])
    one = {k: v.cpu().numpy() for k, v in prepare_inputs(rgb, mask, K, S, P, PREP_SEED, want_pts2d=True, sample="native").items()}
    cut = 3
    a = prepare_inputs(rgb[:cut], mask[:cut], K[:cut], S, P, PREP_SEED, want_pts2d=True, sample="native")
    b = prepare_inputs(rgb[cut:], mask[cut:], K[cut:], S, P, PREP_SEED, want_pts2d=True, sample="native", frame0=cut)
    for k in one:
        assert np.array_equal(_bits(np.concatenate((a[k].cpu().numpy(), b[k].cpu().numpy()))), _bits(one[k])), k
    fmap = np.array([n - 2, -1, 0, 1], np.int32)      # the hash index stays the frame's place f, the pixels are entry frame_map[f]'s
    got = {k: v.cpu().numpy() for k, v in prepare_inputs(rgb, mask, K[:4], S, P, PREP_SEED, want_pts2d=True, sample="native", frame_map=_cuda(fmap)).items()}
    assert got["valid"].tolist() == [1, 0, 1, 1] and not got["choose"][1].any() and not got["pts2d"][1].any()
    for f, src in enumerate(fmap):
        if src >= 0:
            want = v2_ref.prepare_model_input(c["f32"][src], c["mask"][src], c["K"][f], S, seed=PREP_SEED, frame=f)
            _prep_check(got, want, f, f"frame_map {f} -> {src}")


# ------------------------------------------------------------------------------------------------------------------ (b) the kernel alone
def _kernel_rig():
    """Three poses on seeded smooth fp32 maps (28 x 28 noise of deviation 3 up-sampled by 8, like the PSPNet's own last step, on
    per-channel offsets of deviation 4: the golden batch's own maps have deviation 3.3 and channel means up to 7; at unit noise alone
    volume_conv.2's ReLU clips nothing), 200 points per view (no multiple of the 64 points a workgroup carries).  Pose 0: the golden batch's cameras.  Pose 1: two cameras a fraction of a pixel apart,
    so that a chosen pixel keeps the taps its place in the crop allows: the four corners one, the four borders two, the inside four.
    Pose 2: view 1's projection has a zero row - it cannot be inverted (NaN rows for that view), and as the partner's source it is finite."""
    if "rig" in _CACHE:
        return _CACHE["rig"]
    Bk, Pk = 3, 200
    g = np.random.default_rng(21)
    low = torch.from_numpy(g.normal(size=(2 * Bk, 32, S // 8, S // 8)))
    feat = (3 * F.interpolate(low, scale_factor=8, mode="bilinear", align_corners=True) + 4 * torch.from_numpy(np.random.default_rng(22).normal(size=(1, 32, 1, 1)))).float()      # [6, 32, S, S]
    base = synth.adapose_inputs(2, seed=0)
    P1, P2 = np.tile(np.eye(4, dtype=np.float32), (Bk, 1, 1)), np.tile(np.eye(4, dtype=np.float32), (Bk, 1, 1))
    P1[0], P2[0] = base["P1"][0], base["P2"][0]
    Kc = np.array([[300.0, 0, 112.0], [0, 300.0, 112.0], [0, 0, 1.0]])
    for Pm, t in ((P1, (0.0, 0.0, 0.0)), (P2, (1e-4, -1e-4, 0.0))):
        Pm[1, :3, :3], Pm[1, :3, 3] = Kc, Kc @ np.array(t)
    P1[2], P2[2] = base["P1"][1], base["P2"][1]
    P1[2, 1, :] = 0.0
    depths = np.tile(np.arange(1, D + 1, dtype=np.float32)[None] * np.float32(0.1), (Bk, 1))
    choose = g.integers(0, S * S, size=(2, Bk, Pk)).astype(np.int64)
    border = [0, S - 1, (S - 1) * S, S * S - 1, 57, 57 * S, (S - 1) * S + 99, 31 * S + S - 1]      # four corners, four borders
    choose[:, :, : len(border)] = border
    choose[:, :, 20:30] = choose[:, :, 30:40]      # duplicates
    rig = dict(B=Bk, P=Pk, feat=feat, P1=P1, P2=P2, depths=depths, choose1=choose[0], choose2=choose[1])
    _CACHE["rig"] = rig
    return rig


def _kernel_ref(sd64, rig, poses, views):
    sl = lambda a: a[poses]      # noqa: E731
    f1, f2 = rig["feat"][: rig["B"]][poses].double(), rig["feat"][rig["B"]:][poses].double()
    taps = {}
    v2_ref.heads_on_maps(sd64, f1, f2, sl(rig["choose1"]), sl(rig["choose2"]), sl(rig["P1"]), sl(rig["P2"]), sl(rig["depths"]), taps=taps, views=views)
    return taps


def test_point_rows_kernel_against_float64(sd, cpu_ref):
    """rgbm_v2_point_rows on the rig against tests/v2_ref.py in float64 on the same maps: volume_conv's 24 values, fuse_conv's output and
    pose_mlp1's rows, each at the project's fp32 rule max(8 e_ref64, 3e-6) with e_ref64 the golden's own distance to float64 (the smaller
    of the two views').  The rig holds chosen pixels on all four borders of the crop and (point, plane) pairs with 0, 1, 2 and 4 taps
    inside the partner image, asserted here on the CPU - three taps cannot occur: the taps inside are a product of 0, 1 or 2 columns and
    0, 1 or 2 rows.  The view whose projection cannot be inverted has NaN rows and no other view has; duplicate entries of `choose` give
    duplicate rows; views = B gives the first half's bytes."""
    rig = _kernel_rig()
    Bk, Pk = rig["B"], rig["P"]
    net = _net(sd, "fp32")
    H = W = S
    counts = set()
    for v, o in ((1, 2), (2, 1)):
        ix, iy, _ = v2_ref.warp_grid_at(torch.from_numpy(rig[f"P{o}"][:2]), torch.from_numpy(rig[f"P{v}"][:2]), torch.from_numpy(rig["depths"][:2]),
                                        torch.from_numpy(rig[f"choose{v}"][:2]), H, W, torch.float64)
        n = v2_ref.taps_inside(ix, iy, H, W)
        counts |= set(np.unique(n.numpy()).tolist())
        assert {1, 2, 4} <= set(np.unique(n[1].numpy()).tolist())      # the near-identity pose: corners, borders, inside
    assert counts == {0, 1, 2, 4}, counts
    for c in (rig["choose1"], rig["choose2"]):
        ys, xs = c // S, c % S
        assert (ys == 0).any() and (ys == S - 1).any() and (xs == 0).any() and (xs == S - 1).any()
    feat = _cuda(rig["feat"].permute(0, 2, 3, 1).contiguous().numpy())
    choose = _cuda(np.concatenate((rig["choose1"], rig["choose2"])).astype(np.int32))
    Pv = _cuda(np.concatenate((rig["P1"], rig["P2"])))
    got = [t.cpu().numpy() for t in net.v2_point_rows(feat, choose, Pv, _cuda(rig["depths"]))]
    half = [t.cpu().numpy() for t in net.v2_point_rows(feat, choose[:Bk], Pv, _cuda(rig["depths"]))]
    again = [t.cpu().numpy() for t in net.v2_point_rows(feat, choose, Pv, _cuda(rig["depths"]))]
    torch.cuda.synchronize()
    rows, fuse, planes = got
    for full, h, a in zip(got, half, again):
        assert np.array_equal(_bits(full[:Bk]), _bits(h)) and np.array_equal(_bits(full), _bits(a))
    bad = 2      # view index of pose 2's view 1
    for t in got:
        assert np.isnan(t[bad]).all() and np.isfinite(np.delete(t, bad, axis=0)).all()
    assert np.array_equal(_bits(rows[:, 20:30]), _bits(rows[:, 30:40])) and np.array_equal(_bits(planes[:, 20:30]), _bits(planes[:, 30:40]))
    ref = _kernel_ref(cpu_ref["sd64"], rig, slice(0, 2), (1, 2))
    ref2 = _kernel_ref(cpu_ref["sd64"], rig, slice(2, 3), (2,))
    dev = dict(planes=planes, fuse=fuse, rows=rows)
    for kind in KINDS:
        want = np.concatenate((ref[f"v1_{kind}"].numpy(), ref[f"v2_{kind}"].numpy(), ref2[f"v2_{kind}"].numpy()))
        have = np.concatenate((dev[kind][0:2], dev[kind][Bk:Bk + 2], dev[kind][2 * Bk - 1:]))
        e, gate = v2_ref.rel_err(have, want), cpu_ref["kind_gate"](kind)
        print(f"point rows kernel, {kind}: vs float64 {e:.3e}, gate {gate:.3e}")
        assert e <= gate, (kind, e, gate)
    for v in (1, 2):      # every ReLU of the stereo part clips some and passes some of what the rig feeds it
        assert all(0.05 <= c <= 0.95 for c in ref[f"v{v}_clip"]), ref[f"v{v}_clip"]
    assert 0.05 <= float((planes[np.isfinite(planes)] == 0).mean()) <= 0.95


# ------------------------------------------------------------------------------------------------------------------ (c) the forward
def test_fp32_forward_matches_the_reference_golden(sd, inputs, golden, cpu_ref):
    """The four outputs and the three stored intermediates of both views, each at max(8 e_ref64, 3e-6) of its own tensor; depth, r and t
    are NaN (this network has none)."""
    net = _net(sd, "fp32")
    out = _run(net, inputs)
    taps = _taps(net)
    got = dict(out)
    for v in (1, 2):
        for kind in KINDS:
            got[f"v{v}_{kind}_slice"] = v2_ref.points_slice(taps[kind][(v - 1) * B:v * B])
    errs = {k: v2_ref.rel_err(got[k], golden[k]) for k in cpu_ref["e64"]}
    print("v2 fp32 vs reference golden:", errs, "gates", {k: cpu_ref["gate32"](k) for k in errs})
    for k in errs:
        assert np.isfinite(got[k]).all() and errs[k] <= cpu_ref["gate32"](k), (k, errs[k], cpu_ref["gate32"](k))
    for k in ("depth", "r", "t"):
        assert np.isnan(out[f"view1_{k}"]).all() and np.isnan(out[f"view2_{k}"]).all(), k


def test_bf16x3_forward_inside_the_project_gate(sd, inputs, golden):
    """The project's 1e-4 on the four outputs, not widened for this network."""
    out = _run(_net(sd, "bf16x3"), inputs)
    errs = {k: v2_ref.rel_err(out[k], golden[k]) for k in v2_ref.OUT_KEYS}
    print("v2 bf16x3 vs reference golden:", errs)
    for k in v2_ref.OUT_KEYS:
        assert np.isfinite(out[k]).all() and errs[k] < 1e-4, (k, errs)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_16bit_forward(sd, inputs, golden, cpu_ref, dtype):
    """16-bit storage.  The head's arithmetic is fp32 and only its input is 16-bit: the net's own planes, fuse and rows against the
    float64 restatement ON THE NET'S OWN feature map (fetched) sit at the fp32 gate, and the fp32 kernel run on that fetched map gives
    the same.  The four outputs against the golden, each with its own factor: amp[k] x the measured error of the net's own feature maps
    (cpu_ref: the float64 restatement's response of output k to bfloat16-rounded feature maps, x4) plus one rounding of the storage type -
    the per-tensor rule of tests/test_gpu_realworld.py:169.  view*_s, the outputs that pass through the new kernel, have factors of 0.08 /
    0.06 (means over 1024 points), NOCS 5.2 / 4.5."""
    net = _net(sd, dtype)
    out = _run(net, inputs)
    taps = _taps(net)
    feat = net.fetch(B, "feat", 2 * B * S * S * 32).view(2 * B, S, S, 32)
    fe = v2_ref.rel_err(feat.cpu().numpy(), cpu_ref["ref"]["feat"])
    f1, f2 = _maps(feat.cpu().double())
    ref = {}
    v2_ref.heads_on_maps(cpu_ref["sd64"], f1, f2, inputs["choose1"], inputs["choose2"], inputs["P1"], inputs["P2"], inputs["depths"], taps=ref)
    choose = _cuda(np.concatenate((inputs["choose1"], inputs["choose2"])).astype(np.int32))
    alone = _net(sd, "fp32").v2_point_rows(feat, choose, _cuda(np.concatenate((inputs["P1"], inputs["P2"]))), _cuda(inputs["depths"]))
    alone = dict(rows=alone[0].cpu().numpy(), fuse=alone[1].cpu().numpy(), planes=alone[2].cpu().numpy())
    for kind in KINDS:
        want = np.concatenate((ref[f"v1_{kind}"].numpy(), ref[f"v2_{kind}"].numpy()))
        e_net, e_alone, gate = v2_ref.rel_err(taps[kind], want), v2_ref.rel_err(alone[kind], want), cpu_ref["kind_gate"](kind)
        print(f"{dtype} {kind} on the net's own feature map: in the forward {e_net:.3e}, the kernel alone {e_alone:.3e}, gate {gate:.3e}")
        assert np.isfinite(taps[kind]).all() and e_net <= gate and e_alone <= gate, (dtype, kind, e_net, e_alone, gate)
    errs = {k: v2_ref.rel_err(out[k], golden[k]) for k in v2_ref.OUT_KEYS}
    bound = {k: cpu_ref["amp"][k] * fe + EPS[dtype] for k in v2_ref.OUT_KEYS}
    print(f"v2 {dtype} vs reference golden:", errs, "feature error", fe, "bounds", bound)
    for k in v2_ref.OUT_KEYS:
        assert np.isfinite(out[k]).all() and errs[k] <= bound[k], (dtype, k, errs[k], bound[k])


@pytest.mark.parametrize("dtype", ["bf16", "bf16x3"])
def test_view2_heads_poison_and_repeat(sd, inputs, dtype):
    """view2_heads = 0 leaves the view-1 outputs bit for bit and fills view 2's with NaN; a poisoned workspace and a second run give
    identical bytes."""
    full = _run(_net(sd, dtype), inputs)
    again = _run(_net(sd, dtype), inputs)
    poisoned = _run(_net(sd, dtype, poison_workspace=True), inputs)
    half = _run(_net(sd, dtype, options={"view2_heads": 0}), inputs)
    for k in full:
        assert full[k].tobytes() == again[k].tobytes() == poisoned[k].tobytes(), k
    for k in v2_ref.OUT_KEYS:
        assert np.isfinite(full[k]).all(), k
        if k.startswith("view1"):
            assert np.array_equal(_bits(full[k]), _bits(half[k])), k
        else:
            assert np.isnan(half[k]).all(), k


def test_forward_refusals_name_what_is_missing(sd, inputs):
    net = _net(sd, "fp32")
    args = (inputs["img1"], inputs["choose1"], inputs["img2"], inputs["choose2"], inputs["P1"], inputs["P2"], inputs["depths"])
    with pytest.raises(_lib.RgbmError, match="dense"):
        net(*args, dense_depth=True)
    with pytest.raises(_lib.RgbmError, match="coor1"):
        net(*args, coor1=np.zeros((B, P, 2), np.float32), coor2=np.zeros((B, P, 2), np.float32))
    with pytest.raises(_lib.RgbmError, match="missing weight volume_conv.1.bn.running_var"):
        AdaPoseNet({k: v for k, v in sd.items() if k != "volume_conv.1.bn.running_var"}, dtype="fp32", arch="v2")
    for key in (b"cost_impl", b"sparse_dec"):
        assert net.lib.rgbm_adapose_set_option(net._h, key, 1) != 0 and key in net.lib.rgbm_last_error()
    assert net.lib.rgbm_adapose_set_dropout(net._h, 0.15, 0) != 0 and b"v2" in net.lib.rgbm_last_error()
    with pytest.raises(_lib.RgbmError, match="v2"):
        net.fetch(B, "c0", 16)
    # the kernel moves 16-byte pieces of the rows it is given: a misaligned buffer is refused before anything is launched
    feat = torch.zeros(2 * B, 8, 8, 32, dtype=torch.float32, device="cuda")
    ch = torch.zeros(2 * B, 64, dtype=torch.int32, device="cuda")
    Pv, dep = _cuda(np.concatenate((inputs["P1"], inputs["P2"]))), _cuda(inputs["depths"])
    hom = torch.empty(2 * B * 12, dtype=torch.float32, device="cuda")
    rows = torch.empty(2 * B * 64 * 64 + 4, dtype=torch.float32, device="cuda")
    rc = net.lib.rgbm_v2_point_rows(net._h, _lib.ptr(feat), _lib.ptr(ch), _lib.ptr(Pv), _lib.ptr(dep), _lib.ptr(hom), C.c_void_p(rows.data_ptr() + 4), None,
                                    None, B, 64, 8, 2 * B, _lib.stream_ptr(None))
    assert rc != 0 and b"16-byte aligned" in net.lib.rgbm_last_error()
    n = C.c_size_t()
    assert net.lib.rgbm_adapose_feature_bytes(net._h, C.byref(n)) != 0 and b"v2" in net.lib.rgbm_last_error()
    assert net.lib.rgbm_adapose_samples_workspace_bytes(net._h, B, 2, C.byref(n)) != 0 and b"v2" in net.lib.rgbm_last_error()


# ------------------------------------------------------------------------------------------------------------------ (d) the estimator
def _scene():
    """Two poses: 480 x 640 8-bit frames with elliptical masks (more than 1024 pixels each), the extrinsics of synth.adapose_inputs(2, seed=0)."""
    if "scene" not in _CACHE:
        g = np.random.default_rng(3)
        yy, xx = np.mgrid[0:480, 0:640]
        K = np.tile(np.array([[439.31, 0, 320.0], [0, 439.31, 240.0], [0, 0, 1.0]])[None], (B, 1, 1))
        base = synth.adapose_inputs(B, seed=0)
        f1 = np.clip(0.5 + 0.25 * np.cos(xx / 37.0)[None, :, :, None] + 0.2 * g.random((B, 480, 640, 3)), 0, 1)
        f2 = np.clip(0.5 + 0.25 * np.sin(yy / 29.0)[None, :, :, None] + 0.2 * g.random((B, 480, 640, 3)), 0, 1)
        u1, u2 = (np.rint(f * 255.0).astype(np.uint8) for f in (f1, f2))
        m1 = np.stack([((yy - 240) / 60.0) ** 2 + ((xx - 300 - 10 * i) / 90.0) ** 2 <= 1 for i in range(B)]).astype(np.uint8)
        m2 = np.stack([((yy - 250) / 70.0) ** 2 + ((xx - 340 + 10 * i) / 80.0) ** 2 <= 1 for i in range(B)]).astype(np.uint8)
        deq = lambda u: u.astype(np.float32) / np.float32(255)      # noqa: E731
        _CACHE["scene"] = dict(K=K, u1=u1, u2=u2, f1=deq(u1), f2=deq(u2), m1=m1, m2=m2, E1=base["E1"].astype(np.float64), E2=base["E2"].astype(np.float64))
    return _CACHE["scene"]


def _est(net=None, **cfg):
    from rgbmanip_amd.config import adapose_cfg
    from rgbmanip_amd.estimator import AdaPoseEstimator_v2
    cfg = dict(adapose_cfg("one_door_cabinet", load=False, name="adapose_v2"), hip_prepare_seed=9, hip_ransac_seed=5, hip_dtype="bf16x3", **cfg)
    return AdaPoseEstimator_v2(None, cfg, None, net=net)


def test_estimator_equals_the_composition_by_hand(sd):
    """`AdaPoseEstimator_v2.estimate()` and `estimate_device()` = prepare_inputs(sample="native") -> forward -> postprocess_pnp_scaled composed
    by hand, bit for bit: the boxes, and what reaches the tail (view1_nocs, view1_s and the pixels, captured at `_bbox_tail`).  float32
    and 8-bit frames give the same bytes; an empty mask gives the default box."""
    c = _scene()
    net = _net(sd, "bf16x3", options={"view2_heads": 0})
    d = {k: _cuda(v) for k, v in c.items()}
    a = prepare_inputs(d["f1"], d["m1"], d["K"], S, P, 9, want_pts2d=True, sample="native")
    b = prepare_inputs(d["f2"], d["m2"], d["K"], S, P, 10, want_pts2d=True, sample="native")
    est = _est(net=net)
    assert not est.view2_heads and est.estimator is net
    P1, P2 = est._projection(a["Kcrop"], d["E1"]), est._projection(b["Kcrop"], d["E2"])
    from rgbmanip_amd.estimator import _DEPTH_PLANES
    depths = _cuda(np.tile(_DEPTH_PLANES[None], (B, 1)))
    pred = net(a["img"], a["choose"], b["img"], b["choose"], P1, P2, depths)
    box, srt, info, valid = postprocess_pnp_scaled(pred["view1_nocs"], a["pts2d"], pred["view1_s"], d["K"], d["E1"], seed=5)
    want = box.cpu().numpy()
    print("hand-composed tail: valid", valid.tolist(), "info", info.tolist())
    assert np.isfinite(want).all() and np.isfinite(pred["view1_nocs"].cpu().numpy()).all() and np.isfinite(pred["view1_s"].cpu().numpy()).all()
    px = a["pts2d"].cpu().numpy()
    assert np.array_equal(px, np.rint(px)) and (c["m1"][0][px[0, :, 1].astype(int), px[0, :, 0].astype(int)] == 1).all()      # whole pixels of the frame, on the mask
    seen = []
    tail = est._bbox_tail

    def spy(pred_, choose, Kcrop, E1, pts2d=None, E2=None, K=None):
        seen.append((pred_["view1_nocs"].cpu().numpy(), pred_["view1_s"].cpu().numpy(), pts2d[0].cpu().numpy()))
        return tail(pred_, choose, Kcrop, E1, pts2d=pts2d, E2=E2, K=K)
    est._bbox_tail = spy
    for kind, (r1, r2) in {"float32": (c["f1"], c["f2"]), "uint8": (c["u1"], c["u2"])}.items():
        got = est.estimate(c["K"], r1, c["m1"], c["E1"], r2, c["m2"], c["E2"])
        assert np.array_equal(_bits(np.asarray(got)), _bits(want)), kind
        got = est.estimate_device(d["K"], _cuda(r1), d["m1"], d["E1"], _cuda(r2), d["m2"], d["E2"]).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(want)), kind + " (device)"
    assert len(seen) == 4
    for nocs, s1, pts in seen:
        assert np.array_equal(_bits(nocs), _bits(pred["view1_nocs"].cpu().numpy())) and np.array_equal(_bits(s1), _bits(pred["view1_s"].cpu().numpy()))
        assert np.array_equal(_bits(pts), _bits(px))
    empty = c["m1"].copy()
    empty[1] = 0
    got = np.asarray(est.estimate(c["K"], c["u1"], empty, c["E1"], c["u2"], c["m2"], c["E2"]))
    assert np.array_equal(got[1], DEFAULT_BBOX) and np.array_equal(_bits(got[0]), _bits(want[0]))
    with pytest.raises(NotImplementedError, match="estimate_depth"):
        est.estimate_depth(c["K"], c["u1"], c["m1"], c["E1"], c["u2"], c["m2"], c["E2"])
