"""GPU: the v1 network (rgbm_adapose_create_v1) - stages A and B of its heads alone against float64, the forward against the reference's
golden in every storage type, and `AdaPoseEstimator_v1`.  References: tests/golden/adapose_v1_b2.npz (the reference class itself) and
tests/v1_ref.py (the float64 restatement)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import v1_ref  # noqa: E402

from oracle.pnp_ref import DEFAULT_BBOX  # noqa: E402
from rgbmanip_amd import _lib, synth  # noqa: E402
from rgbmanip_amd.adapose import AdaPoseNet, postprocess_pnp_scaled, prepare_inputs  # noqa: E402

pytestmark = pytest.mark.gpu
B, S, D, P = 2, 224, 24, 1024
EPS = {"fp32": 2.0 ** -24, "bf16": 2.0 ** -9, "fp16": 2.0 ** -12, "bf16x3": 2.0 ** -17}      # half a unit in the last place of the storage type, relative
KINDS = v1_ref.TAP_KEYS                       # planes, fused, rows
WIDTH = dict(planes=D, fused=32, rows=128, nocs=3)
POINT_MLP_PER_LAYER = 2048                    # rgbm_debug_flags: the per-layer point MLP
_CACHE = {}


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "adapose_v1_b2.npz"))


@pytest.fixture(scope="module")
def sd():
    return synth.v1_state_dict(seed=0)


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
    smaller e64 of the two views' tensors of that kind, for the kernels on maps of their own.  amp[k]: how far the float64 restatement's
    output k moves when the feature maps are rounded to bfloat16, over that rounding's own size, times the project's margin of 4
    (tests/test_v1_host.py asserts every one below 400)."""
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    sd64 = v1_ref.to_sd(sd, torch.float64)
    taps = {}
    out = v1_ref.v1_forward(sd64, inputs["img1"], inputs["choose1"], inputs["img2"], inputs["choose2"], inputs["P1"], inputs["P2"], inputs["depths"], taps=taps)
    ref = {k: v.numpy() for k, v in out.items()}
    for v in (1, 2):
        for kind in KINDS:
            ref[f"v{v}_{kind}_slice"] = v1_ref.points_slice(taps[f"v{v}_{kind}"]).numpy()
    ref["feat"] = torch.cat((taps["feat1"], taps["feat2"])).permute(0, 2, 3, 1).contiguous().numpy()
    keys = v1_ref.OUT_KEYS + [f"v{v}_{kind}_slice" for v in (1, 2) for kind in KINDS]
    e64 = {k: v1_ref.rel_err(golden[k], ref[k]) for k in keys}
    rounded_feat = torch.from_numpy(ref["feat"]).float().to(torch.bfloat16).double()
    f1, f2 = _maps(rounded_feat)
    rounded = {k: v.numpy() for k, v in v1_ref.heads_on_maps(sd64, f1, f2, inputs["choose1"], inputs["choose2"], inputs["P1"], inputs["P2"],
                                                            inputs["depths"]).items()}
    fe = v1_ref.rel_err(rounded_feat.numpy(), ref["feat"])
    amp = {k: 4 * v1_ref.rel_err(rounded[k], ref[k]) / fe for k in v1_ref.OUT_KEYS}
    print("e_ref64 per tensor:", e64)
    print("bf16 feature rounding", fe, "amplification factors (x4 margin included):", amp)
    kind_e = dict({kind: min(e64[f"v{v}_{kind}_slice"] for v in (1, 2)) for kind in KINDS}, nocs=min(e64["view1_nocs"], e64["view2_nocs"]))
    return dict(ref=ref, e64=e64, amp=amp, sd64=sd64, gate32=lambda k: max(8 * e64[k], 3e-6), kind_gate=lambda kind: max(8 * kind_e[kind], 3e-6))


def _net(sd, dtype, **kw):
    key = (dtype, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _CACHE:
        _CACHE[key] = AdaPoseNet(sd, dtype=dtype, arch="v1", **kw)
    return _CACHE[key]


def _run(net, inp):
    out = net(inp["img1"], inp["choose1"], inp["img2"], inp["choose2"], inp["P1"], inp["P2"], inp["depths"])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _taps(net):
    """planes / fused / rows of the last forward, [2B, P, C] each (views [view-1 poses ; view-2 poses])"""
    return {kind: net.fetch(B, "v1_" + kind, 2 * B * P * WIDTH[kind]).view(2 * B, P, WIDTH[kind]).cpu().numpy() for kind in KINDS}


# ------------------------------------------------------------------------------------------------------------------ (a) stages A + B alone
def _kernel_rig():
    """tests/test_gpu_v2.py's kernel rig, rebuilt from the same seeds.  Three poses on seeded smooth fp32 maps (28 x 28 noise of deviation 3
    up-sampled by 8 on per-channel offsets of deviation 4), 200 points per view.  Pose 0: the golden batch's cameras.  Pose 1: two cameras
    1e-4 apart, so that a chosen pixel keeps the taps its place in the crop allows: the four corners one, the four borders two, the
    inside four.  Pose 2: view 1's projection has a zero row - it cannot be inverted (NaN rows for that view), and as the partner's source
    it is finite.  Chosen pixels on all four borders and the four corners; points 20..29 repeat points 30..39."""
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


def _kernel_ref(sd64, rig):
    """The float64 restatement on the rig, once: per kind [5 views][200][C] - views 1 and 2 of poses 0 and 1, view 2 of pose 2 (whose
    partner cannot be inverted, but is finite as a source) - with the ReLU clip shares and tap counts of poses 0 and 1."""
    if "rig_ref" in _CACHE:
        return _CACHE["rig_ref"]
    Bk = rig["B"]
    out = {}
    for poses, views, tag in ((slice(0, 2), (1, 2), "a"), (slice(2, 3), (2,), "b")):
        f1, f2 = rig["feat"][:Bk][poses].double(), rig["feat"][Bk:][poses].double()
        taps = {}
        o = v1_ref.heads_on_maps(sd64, f1, f2, rig["choose1"][poses], rig["choose2"][poses], rig["P1"][poses], rig["P2"][poses], rig["depths"][poses],
                                 taps=taps, views=views, pose=False)
        taps.update({f"v{v}_nocs": o[f"view{v}_nocs"] for v in views})
        out[tag] = taps
    a, b = out["a"], out["b"]
    want = {kind: np.concatenate((a[f"v1_{kind}"].numpy(), a[f"v2_{kind}"].numpy(), b[f"v2_{kind}"].numpy())) for kind in KINDS + ("nocs",)}
    ref = dict(want=want, clip={v: a[f"v{v}_clip"] for v in (1, 2)}, taps={v: a[f"v{v}_taps"].numpy() for v in (1, 2)})
    _CACHE["rig_ref"] = ref
    return ref


def _rig_views(t, Bk):
    """device result [2 Bk views][P][C] -> the five views _kernel_ref holds"""
    return np.concatenate((t[0:2], t[Bk:Bk + 2], t[2 * Bk - 1:]))


def _stages(net, rig, Pk, views=None, flags=0):
    """rgbm_v1_point_rows on the rig's first Pk points -> dict(planes, fused, nocs, rows), numpy"""
    Bk = rig["B"]
    feat = _cuda(rig["feat"].permute(0, 2, 3, 1).contiguous().numpy())
    choose = _cuda(np.concatenate((rig["choose1"][:, :Pk], rig["choose2"][:, :Pk])).astype(np.int32))
    Pv = _cuda(np.concatenate((rig["P1"], rig["P2"])))
    if views is not None:
        choose = choose[:views].contiguous()
    lib = _lib.load()
    lib.rgbm_debug_flags(flags)
    try:
        fused, nocs4, rows, planes = net.v1_point_rows(feat, choose, Pv, _cuda(rig["depths"]))
        torch.cuda.synchronize()
    finally:
        lib.rgbm_debug_flags(0)
    return dict(planes=planes.cpu().numpy(), fused=fused.cpu().numpy(), nocs=nocs4.cpu().numpy()[..., :3], rows=rows.cpu().numpy(), pad=nocs4.cpu().numpy()[..., 3])


def _check_against_float64(got, ref, Pk, Bk, cpu_ref, tag):
    for kind in KINDS + ("nocs",):
        want = ref["want"][kind][:, :Pk]
        have = _rig_views(got[kind], Bk)
        e, gate = v1_ref.rel_err(have, want), cpu_ref["kind_gate"](kind)
        print(f"{tag}, {kind}: vs float64 {e:.3e}, gate {gate:.3e}")
        assert e <= gate, (tag, kind, e, gate)
    bad = 2      # view index of pose 2's view 1: its projection cannot be inverted
    for kind in KINDS + ("nocs",):
        t = got[kind]
        assert np.isnan(t[bad]).all() and np.isfinite(np.delete(t, bad, axis=0)).all(), (tag, kind)


def test_rig_covers_every_tap_count_and_clips_every_relu(sd, cpu_ref):
    """On the CPU: (point, plane) pairs with 0, 1, 2 and 4 taps inside the partner image all occur (three cannot: the taps inside are a
    product of 0, 1 or 2 columns and 0, 1 or 2 rows), the near-identity pose alone holds 1, 2 and 4; the chosen pixels touch all four
    borders; every ReLU of the stereo part, the residual one included, clips between 5 % and 95 % of what the rig feeds it."""
    rig = _kernel_rig()
    ref = _kernel_ref(cpu_ref["sd64"], rig)
    counts = set()
    for v in (1, 2):
        n = ref["taps"][v]
        counts |= set(np.unique(n).tolist())
        assert {1, 2, 4} <= set(np.unique(n[1]).tolist())
        assert len(ref["clip"][v]) == len(v1_ref.RELU_NAMES) and all(0.05 <= c <= 0.95 for c in ref["clip"][v]), ref["clip"][v]
    assert counts == {0, 1, 2, 4}, counts
    for c in (rig["choose1"], rig["choose2"]):
        for cc in (c, c[:, :192]):
            ys, xs = cc // S, cc % S
            assert (ys == 0).any() and (ys == S - 1).any() and (xs == 0).any() and (xs == S - 1).any()


def test_stages_at_200_points_tail_pass_and_per_layer_b(sd, cpu_ref):
    """P = 200: views x P is no multiple of 64, so stage A ends in a partly filled pass and stage B runs per layer.  planes, fused32,
    nocs and the 128-channel rows against float64 at max(8 min_v e_ref64, 3e-6) per kind; the non-invertible view is all NaN and no
    other is; duplicate pixels give duplicate rows bit for bit; views = B gives the first half's bytes; two runs give equal bytes."""
    rig = _kernel_rig()
    Bk, Pk = rig["B"], 200
    assert (2 * Bk * Pk) % 64 and (Bk * Pk) % 64
    net = _net(sd, "fp32")
    got = _stages(net, rig, Pk)
    _check_against_float64(got, _kernel_ref(cpu_ref["sd64"], rig), Pk, Bk, cpu_ref, "P = 200")
    half, again = _stages(net, rig, Pk, views=Bk), _stages(net, rig, Pk)
    for kind in got:
        assert np.array_equal(_bits(got[kind][:Bk]), _bits(half[kind])), kind
        assert np.array_equal(_bits(got[kind]), _bits(again[kind])), kind
        assert np.array_equal(_bits(got[kind][:, 20:30]), _bits(got[kind][:, 30:40])), kind
    assert got["planes"].shape == (2 * Bk, Pk, D) and got["fused"].shape == (2 * Bk, Pk, 32) and got["rows"].shape == (2 * Bk, Pk, 128)
    ok = np.delete(got["planes"], 2, axis=0)
    assert 0.05 <= float((ok == 0).mean()) <= 0.95 and 0.05 <= float((np.delete(got["fused"], 2, axis=0) == 0).mean()) <= 0.95


@pytest.mark.parametrize("views", ["2B", "B"])
def test_stages_at_192_points_fused_b(sd, cpu_ref, views):
    """P = 192, the rig's first 192 points: views x P is a multiple of 64 at views = 2B and views = B, so stage B is the one-launch
    kernel.  The same checks; and the fused B and the per-layer B (debug flag 2048) agree within the same gate, with stage A's bytes equal."""
    rig = _kernel_rig()
    Bk, Pk = rig["B"], 192
    nv = 2 * Bk if views == "2B" else Bk
    assert (nv * Pk) % 64 == 0
    net = _net(sd, "fp32")
    ref = _kernel_ref(cpu_ref["sd64"], rig)
    got = _stages(net, rig, Pk, views=nv)
    layer = _stages(net, rig, Pk, views=nv, flags=POINT_MLP_PER_LAYER)
    again = _stages(net, rig, Pk, views=nv)
    full200 = _stages(net, rig, 200, views=nv)
    for kind in got:
        assert np.array_equal(_bits(got[kind]), _bits(again[kind])), kind
        assert np.array_equal(_bits(got[kind][:, 20:30]), _bits(got[kind][:, 30:40])), kind
    for kind in ("planes", "fused"):      # stage A does not depend on the point count or on B's form
        assert np.array_equal(_bits(got[kind]), _bits(layer[kind])) and np.array_equal(_bits(got[kind]), _bits(full200[kind][:, :Pk])), kind
    if views == "2B":
        _check_against_float64(got, ref, Pk, Bk, cpu_ref, "P = 192, fused B")
        _check_against_float64(layer, ref, Pk, Bk, cpu_ref, "P = 192, per-layer B")
    else:      # views = B: the view-1 crops of the three poses; pose 2's cannot be inverted
        for kind in KINDS + ("nocs",):
            want, gate = ref["want"][kind][0:2, :Pk], cpu_ref["kind_gate"](kind)
            for tag, t in (("fused B", got), ("per-layer B", layer)):
                e = v1_ref.rel_err(t[kind][0:2], want)
                print(f"P = 192, views = B, {tag}, {kind}: vs float64 {e:.3e}, gate {gate:.3e}")
                assert e <= gate and np.isnan(t[kind][2]).all() and np.isfinite(t[kind][:2]).all(), (tag, kind, e, gate)
    ok = [i for i in range(nv) if i != 2]
    for kind in ("nocs", "rows"):
        e, gate = v1_ref.rel_err(got[kind][ok], layer[kind][ok]), cpu_ref["kind_gate"](kind)
        print(f"P = 192, views = {views}, {kind}: fused B vs per-layer B {e:.3e}, gate {gate:.3e}")
        assert e <= gate, (kind, e, gate)
    assert not got["pad"][ok].any()      # channel 3 of nocs4 is tanh(0)


# ------------------------------------------------------------------------------------------------------------------ (b) .. (d) the forward
def test_fp32_forward_matches_the_reference_golden(sd, inputs, golden, cpu_ref):
    """The eight outputs and the three stored intermediates of both views, each at max(8 e_ref64, 3e-6) of its own tensor; depth is
    NaN (this network has none)."""
    net = _net(sd, "fp32")
    out = _run(net, inputs)
    taps = _taps(net)
    got = dict(out)
    for v in (1, 2):
        for kind in KINDS:
            got[f"v{v}_{kind}_slice"] = v1_ref.points_slice(taps[kind][(v - 1) * B:v * B])
    errs = {k: v1_ref.rel_err(got[k], golden[k]) for k in cpu_ref["e64"]}
    print("v1 fp32 vs reference golden:", errs, "gates", {k: cpu_ref["gate32"](k) for k in errs})
    for k in errs:
        assert np.isfinite(got[k]).all() and errs[k] <= cpu_ref["gate32"](k), (k, errs[k], cpu_ref["gate32"](k))
    assert np.isnan(out["view1_depth"]).all() and np.isnan(out["view2_depth"]).all()


def test_bf16x3_forward_inside_the_project_gate(sd, inputs, golden):
    """The project's 1e-4 on the eight outputs, not widened for this network."""
    out = _run(_net(sd, "bf16x3"), inputs)
    errs = {k: v1_ref.rel_err(out[k], golden[k]) for k in v1_ref.OUT_KEYS}
    print("v1 bf16x3 vs reference golden:", errs)
    for k in v1_ref.OUT_KEYS:
        assert np.isfinite(out[k]).all() and errs[k] < 1e-4, (k, errs)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_16bit_forward(sd, inputs, golden, cpu_ref, dtype):
    """16-bit storage.  The heads' arithmetic is fp32 and only their input is 16-bit: the net's own planes, fused rows and pose rows
    against the float64 restatement ON THE NET'S OWN feature map (fetched) sit at the fp32 gate, and the fp32 stages run alone on that
    fetched map give the same.  The eight outputs against the golden, each with its own factor: amp[k] x the measured error of the net's
    own feature maps plus one rounding of the storage type - the rule of tests/test_gpu_v2.py."""
    net = _net(sd, dtype)
    out = _run(net, inputs)
    taps = _taps(net)
    feat = net.fetch(B, "feat", 2 * B * S * S * 32).view(2 * B, S, S, 32)
    fe = v1_ref.rel_err(feat.cpu().numpy(), cpu_ref["ref"]["feat"])
    f1, f2 = _maps(feat.cpu().double())
    ref = {}
    v1_ref.heads_on_maps(cpu_ref["sd64"], f1, f2, inputs["choose1"], inputs["choose2"], inputs["P1"], inputs["P2"], inputs["depths"], taps=ref, pose=False)
    choose = _cuda(np.concatenate((inputs["choose1"], inputs["choose2"])).astype(np.int32))
    fused, _, rows, planes = _net(sd, "fp32").v1_point_rows(feat, choose, _cuda(np.concatenate((inputs["P1"], inputs["P2"]))), _cuda(inputs["depths"]))
    alone = dict(rows=rows.cpu().numpy(), fused=fused.cpu().numpy(), planes=planes.cpu().numpy())
    for kind in KINDS:
        want = np.concatenate((ref[f"v1_{kind}"].numpy(), ref[f"v2_{kind}"].numpy()))
        e_net, e_alone, gate = v1_ref.rel_err(taps[kind], want), v1_ref.rel_err(alone[kind], want), cpu_ref["kind_gate"](kind)
        print(f"{dtype} {kind} on the net's own feature map: in the forward {e_net:.3e}, the stages alone {e_alone:.3e}, gate {gate:.3e}")
        assert np.isfinite(taps[kind]).all() and e_net <= gate and e_alone <= gate, (dtype, kind, e_net, e_alone, gate)
    errs = {k: v1_ref.rel_err(out[k], golden[k]) for k in v1_ref.OUT_KEYS}
    bound = {k: cpu_ref["amp"][k] * fe + EPS[dtype] for k in v1_ref.OUT_KEYS}
    print(f"v1 {dtype} vs reference golden:", errs, "feature error", fe, "bounds", bound)
    for k in v1_ref.OUT_KEYS:
        assert np.isfinite(out[k]).all() and errs[k] <= bound[k], (dtype, k, errs[k], bound[k])


# ------------------------------------------------------------------------------------------------------------------ (e) heads, poison, refusals
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
    for k in v1_ref.OUT_KEYS:
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
    with pytest.raises(_lib.RgbmError, match="missing weight fuse_conv.2.bias"):
        AdaPoseNet({k: v for k, v in sd.items() if k != "fuse_conv.2.bias"}, dtype="fp32", arch="v1")
    for key in (b"cost_impl", b"sparse_dec"):
        assert net.lib.rgbm_adapose_set_option(net._h, key, 1) != 0 and key in net.lib.rgbm_last_error()
    assert net.lib.rgbm_adapose_set_dropout(net._h, 0.15, 0) != 0 and b"v1" in net.lib.rgbm_last_error()
    with pytest.raises(_lib.RgbmError, match="v1"):
        net.fetch(B, "c0", 16)
    # the kernels move 16-byte pieces of the rows they are given: a misaligned buffer is refused before anything is launched
    feat = torch.zeros(2 * B, 8, 8, 32, dtype=torch.float32, device="cuda")
    ch = torch.zeros(2 * B, 64, dtype=torch.int32, device="cuda")
    Pv, dep = _cuda(np.concatenate((inputs["P1"], inputs["P2"]))), _cuda(inputs["depths"])
    hom = torch.empty(2 * B * 12, dtype=torch.float32, device="cuda")
    fused = torch.empty(2 * B * 64 * 32 + 4, dtype=torch.float32, device="cuda")
    rc = net.lib.rgbm_v1_point_rows(net._h, _lib.ptr(feat), _lib.ptr(ch), _lib.ptr(Pv), _lib.ptr(dep), _lib.ptr(hom), C.c_void_p(fused.data_ptr() + 4), None,
                                    None, None, None, B, 64, 8, 2 * B, _lib.stream_ptr(None))
    assert rc != 0 and b"16-byte aligned" in net.lib.rgbm_last_error()
    n = C.c_size_t()
    assert net.lib.rgbm_adapose_feature_bytes(net._h, C.byref(n)) != 0 and b"v1" in net.lib.rgbm_last_error()
    assert net.lib.rgbm_adapose_samples_workspace_bytes(net._h, B, 2, C.byref(n)) != 0 and b"v1" in net.lib.rgbm_last_error()
    # a handle of another network is refused by rgbm_v1_point_rows, and this handle by rgbm_v2_point_rows
    rc = net.lib.rgbm_v2_point_rows(net._h, _lib.ptr(feat), _lib.ptr(ch), _lib.ptr(Pv), _lib.ptr(dep), _lib.ptr(hom), _lib.ptr(fused), None, None, B, 64, 8,
                                    2 * B, _lib.stream_ptr(None))
    assert rc != 0 and b"v2" in net.lib.rgbm_last_error()


# ------------------------------------------------------------------------------------------------------------------ (f) the estimator
def _scene():
    """The two-pose 480 x 640 ellipse scene of tests/test_gpu_v2.py: 8-bit frames with elliptical masks (more than 1024 pixels each), the
    extrinsics of synth.adapose_inputs(2, seed=0)."""
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
    from rgbmanip_amd.estimator import AdaPoseEstimator_v1
    cfg = dict(adapose_cfg("one_door_cabinet", load=False, name="adapose"), hip_prepare_seed=9, hip_ransac_seed=5, hip_dtype="bf16x3", **cfg)
    return AdaPoseEstimator_v1(None, cfg, None, net=net)


def test_estimator_equals_the_composition_by_hand(sd):
    """`AdaPoseEstimator_v1.estimate()` and `estimate_device()` = prepare_inputs(sample="native") -> forward -> postprocess_pnp_scaled composed
    by hand, bit for bit: the boxes, and what reaches the tail (view1_nocs, view1_s and the pixels, captured at `_bbox_tail`).  float32
    and 8-bit frames give the same bytes; an empty mask gives the default box; estimate_depth names itself."""
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
    with pytest.raises(NotImplementedError, match="AdaPoseEstimator_v1.estimate_depth"):
        est.estimate_depth(c["K"], c["u1"], c["m1"], c["E1"], c["u2"], c["m2"], c["E2"])
