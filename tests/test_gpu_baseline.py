"""GPU: the baseline network (rgbm_adapose_create_baseline) end to end against the reference's golden, its options and refusals, and
`AdaPoseEstimator_baseline`.  References: tests/golden/adapose_baseline_b2.npz (the reference class itself) and tests/baseline_ref.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import baseline_ref as br  # noqa: E402

from rgbmanip_amd import _lib, synth  # noqa: E402
from rgbmanip_amd.adapose import AdaPoseNet, postprocess, postprocess_ransac, prepare_inputs  # noqa: E402

pytestmark = pytest.mark.gpu
OUT_KEYS = [f"view{v}_{k}" for k in ("nocs", "depth", "r", "t", "s") for v in (1, 2)]
FOUR = ("view1_nocs", "view2_nocs", "view1_depth", "view2_depth")
# v5's end-to-end gates per storage type (tests/test_gpu_adapose.py)
V5_GATE = {"bf16": {"nocs": 2.7e-2, "depth": 1.0e-2, "r": 6.0e-3, "t": 3.5e-3, "s": 1.2e-3},
           "fp16": {"nocs": 2.4e-3, "depth": 1.7e-3, "r": 1.2e-4, "t": 3.0e-4, "s": 7.0e-5}}
_CACHE = {}


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "adapose_baseline_b2.npz"))


@pytest.fixture(scope="module")
def sd():
    return synth.baseline_state_dict(seed=0)


@pytest.fixture(scope="module")
def inputs():
    return synth.adapose_inputs(2, seed=0)


@pytest.fixture(scope="module")
def cpu_ref(sd, inputs, golden):
    """Computed once on the CPU: e_ref64 (the reference's float32 rounding over the ten outputs: the golden against the float64
    restatement; measured 2.8e-6) and, per 16-bit storage type, the amplification factor of the stages behind the PSPNet: the float64
    restatement's worst output error when its float32 feature maps are rounded to that type, over the rounding error of the feature
    maps, times a margin of 4.  Measured: bf16 5.6 x 4 = 22, fp16 7.2 x 4 = 29 (the depths are the worst output in both)."""
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    sd64 = br.to_sd(sd, torch.float64)
    out64 = br.baseline_forward(sd64, inputs["img1"], inputs["choose1"], inputs["img2"], inputs["choose2"])
    e_ref64 = max(br.rel_err(golden[k], out64[k].numpy()) for k in OUT_KEYS)
    taps = {}
    br.baseline_forward(br.to_sd(sd, torch.float32), inputs["img1"], inputs["choose1"], inputs["img2"], inputs["choose2"], taps=taps)
    feats = taps["feat1"], taps["feat2"]
    ch = torch.as_tensor(inputs["choose1"]), torch.as_tensor(inputs["choose2"])

    def heads(f1, f2):
        return br.heads_from_rows(sd64, br.gather_rows(f1.double(), ch[0]), br.gather_rows(f2.double(), ch[1]))
    base = heads(*feats)
    factor = {}
    for name, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        r = [f.to(dt).float() for f in feats]
        fe = max(br.rel_err(r[i].numpy(), feats[i].numpy()) for i in (0, 1))
        o = heads(*r)
        ratio = max(br.rel_err(o[k].numpy(), base[k].numpy()) for k in OUT_KEYS) / fe
        assert ratio <= 50, (name, ratio)            # above that the fixture's query / key gain is too high
        factor[name] = 4 * ratio
    print("e_ref64", e_ref64, "amplification factors (x4 margin included)", factor)
    return dict(e_ref64=e_ref64, fp32_gate=max(8 * e_ref64, 3e-6), factor=factor, sd64=sd64)


def _net(sd, dtype, **kw):
    key = (dtype, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _CACHE:
        _CACHE[key] = AdaPoseNet(sd, dtype=dtype, arch="baseline", **kw)
    return _CACHE[key]


def _run(net, inp):
    out = net(inp["img1"], inp["choose1"], inp["img2"], inp["choose2"], inp["P1"], inp["P2"], inp["depths"])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _raw_forward(net, inp, entry="rgbm_adapose_forward", null_cameras=True, fill=7.0, extra=()):
    """The C entry itself on pre-filled outputs (what a refused call must leave alone); P1 / P2 / depths NULL when asked."""
    lib = _lib.load()
    B = inp["img1"].shape[0]
    t = [net._prep(inp[k], d) for k, d in (("img1", torch.float32), ("img2", torch.float32), ("choose1", torch.int32), ("choose2", torch.int32),
                                           ("P1", torch.float32), ("P2", torch.float32), ("depths", torch.float32))]
    shapes = {"nocs": (B, 1024, 3), "depth": (B, 1024), "r": (B, 3, 3), "t": (B, 3), "s": (B, 3)}
    out = {f"view{v}_{k}": torch.full(shp, fill, dtype=torch.float32, device="cuda") for k, shp in shapes.items() for v in (1, 2)}
    o = _lib.AdaposeOut(*[out[n].data_ptr() for n, _ in _lib.AdaposeOut._fields_])
    ws_ptr, ws_bytes = net._workspace(B)
    ptrs = [_lib.ptr(x) for x in t]
    if null_cameras:
        ptrs[4] = ptrs[5] = ptrs[6] = None
    rc = getattr(lib, entry)(net._h, B, *ptrs, C.c_void_p(ws_ptr), ws_bytes, C.byref(o), *extra, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in out.items()}


# ------------------------------------------------------------------------------------------------------------------ 1. against the golden
def test_fp32_matches_the_reference_golden(sd, inputs, golden, cpu_ref):
    """All ten outputs at max(8 e_ref64, 3e-6): 8 x 2.8e-6 = 2.2e-5 (3e-6 is v5's fp32 figure for the shared PSPNet).  Measured: worst
    output view1_depth 1.0e-5, the pose outputs below 1e-6, the fused rows 8.5e-6 / 1.1e-5."""
    net = _net(sd, "fp32")
    out = _run(net, inputs)
    errs = {k: br.rel_err(out[k], golden[k]) for k in OUT_KEYS}
    B = 2
    f1 = net.fetch(B, "fused1", B * 1024 * 32).cpu().numpy().reshape(B, 1024, 32)
    f2 = net.fetch(B, "fused2", B * 1024 * 32).cpu().numpy().reshape(B, 1024, 32)
    errs["fused1"], errs["fused2"] = br.rel_err(f1, golden["fused1"]), br.rel_err(f2, golden["fused2"])
    print("baseline fp32 vs reference golden:", errs, "gate", cpu_ref["fp32_gate"])
    for k in OUT_KEYS:
        assert np.isfinite(out[k]).all() and errs[k] <= cpu_ref["fp32_gate"], (k, errs)
    # P1 / P2 / depths are not read: NULL gives the same bytes
    rc, raw = _raw_forward(net, inputs)
    assert rc == 0
    for k in OUT_KEYS:
        assert np.array_equal(_bits(raw[k]), _bits(out[k])), k


def test_bf16x3_inside_the_project_gate(sd, inputs, golden):
    """Measured: view1_depth 9.7e-5, view2_depth 7.9e-5 (the stack amplifies the split-pair feature error about six times into the
    depths), NOCS 1.7e-5, r / t / s below 7e-6."""
    out = _run(_net(sd, "bf16x3"), inputs)
    errs = {k: br.rel_err(out[k], golden[k]) for k in OUT_KEYS}
    print("baseline bf16x3 vs reference golden:", errs)
    for k in OUT_KEYS:
        assert np.isfinite(out[k]).all() and errs[k] < 1e-4, (k, errs)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_16_bit_storage(sd, inputs, golden, cpu_ref, dtype):
    """The new stages alone are fp32 whatever the storage: from the handle's own feature maps (fetched, gathered on the host) the float64
    restatement's fused rows and depths must agree at the fp32 bound.  End to end against the golden: v5's gate for the storage type
    times the amplification factor computed on the CPU (cpu_ref)."""
    net = _net(sd, dtype)
    out = _run(net, inputs)
    B, S = 2, 224
    feat = net.fetch(B, "feat", 2 * B * S * S * 32).cpu().double().reshape(2 * B, S * S, 32)
    f1 = net.fetch(B, "fused1", B * 1024 * 32).cpu().numpy().reshape(B, 1024, 32)
    f2 = net.fetch(B, "fused2", B * 1024 * 32).cpu().numpy().reshape(B, 1024, 32)
    ch1, ch2 = torch.as_tensor(inputs["choose1"]).long(), torch.as_tensor(inputs["choose2"]).long()
    rows1 = torch.gather(feat[:B], 1, ch1.unsqueeze(-1).expand(B, 1024, 32))
    rows2 = torch.gather(feat[B:], 1, ch2.unsqueeze(-1).expand(B, 1024, 32))
    taps = {}
    ref = br.heads_from_rows(cpu_ref["sd64"], rows1, rows2, taps=taps)
    stage = {"fused1": br.rel_err(f1, taps["fused1"].numpy()), "fused2": br.rel_err(f2, taps["fused2"].numpy()),
             "view1_depth": br.rel_err(out["view1_depth"], ref["view1_depth"].numpy()),
             "view2_depth": br.rel_err(out["view2_depth"], ref["view2_depth"].numpy()),
             "view1_nocs": br.rel_err(out["view1_nocs"], ref["view1_nocs"].numpy())}
    print(f"{dtype}: new stages from the handle's own features vs float64:", stage, "gate", cpu_ref["fp32_gate"])
    for k, e in stage.items():
        assert e <= cpu_ref["fp32_gate"], (k, stage)
    errs = {k: br.rel_err(out[k], golden[k]) for k in OUT_KEYS}
    factor = cpu_ref["factor"][dtype]
    print(f"{dtype} vs reference golden:", errs, "factor", factor)
    for k in OUT_KEYS:
        assert np.isfinite(out[k]).all() and errs[k] < V5_GATE[dtype][k.split("_")[1]] * factor, (k, errs, factor)


# ------------------------------------------------------------------------------------------------------------------ 2. handle behaviour
def test_without_pose_branch(inputs):
    sd4 = synth.baseline_state_dict(seed=0, regress_pose=False)
    net = AdaPoseNet(sd4, dtype="fp32", arch="baseline", regress_pose=False)
    out = _run(net, inputs)
    assert sorted(out) == sorted(FOUR)
    full = _run(_net(synth.baseline_state_dict(seed=0), "fp32"), inputs)
    for k in FOUR:
        assert np.isfinite(out[k]).all() and np.array_equal(_bits(out[k]), _bits(full[k])), k
    rc, raw = _raw_forward(net, inputs)
    assert rc == 0
    for k in OUT_KEYS:
        assert np.isnan(raw[k]).all() if k not in FOUR else np.array_equal(_bits(raw[k]), _bits(out[k])), k
    # a pose-branch state dict is needed for regress_pose=True: the missing weight is named
    with pytest.raises(_lib.RgbmError, match="missing weight nocs_pts_mlp.0.weight"):
        AdaPoseNet(sd4, dtype="fp32", arch="baseline", regress_pose=True)
    net.close()


def test_view1_only_heads(sd, inputs):
    """view2_heads = 0: the view-1 outputs are the full run's bit for bit, the view-2 outputs NaN.  Two instead of four views in the pose
    MLP may cross a kernel-selection threshold of an fp32 net (another summation order): both runs are pinned to the generic tiles, as
    in tests/test_gpu_adapose.py::test_view1_only_heads_equal_the_full_forward."""
    lib = _lib.load()
    _lib.check(lib.rgbm_set_tuning(b"ws_min_rows", 1 << 30))
    try:
        full = _run(_net(sd, "fp32"), inputs)
        one = _run(_net(sd, "fp32", options={"view2_heads": 0}), inputs)
    finally:
        _lib.check(lib.rgbm_set_tuning(b"ws_min_rows", 0))
    for k in OUT_KEYS:
        if k.startswith("view1"):
            assert np.array_equal(_bits(one[k]), _bits(full[k])), k
        else:
            assert np.isnan(one[k]).all(), k


def test_chunked_attention_is_bit_identical(sd):
    """B = 3 with max_chunk = 4 views (two poses, then one) against one chunk."""
    inp = synth.adapose_inputs(3, seed=1)
    a = _run(_net(sd, "bf16"), inp)
    b = _run(_net(sd, "bf16", options={"max_chunk": 4}), inp)
    for k in OUT_KEYS:
        assert np.isfinite(a[k]).all() and np.array_equal(_bits(a[k]), _bits(b[k])), k


def test_refused_calls_launch_nothing(sd, inputs):
    net = _net(sd, "fp32")
    lib = _lib.load()
    B = 2
    maps = torch.empty(2 * B, 224, 224, dtype=torch.float32, device="cuda")
    for entry, extra, word in (("rgbm_adapose_forward_dense", (_lib.ptr(maps), None), b"baseline"),
                               ("rgbm_adapose_forward_maps", (_lib.ptr(maps), None, None), b"baseline")):
        rc, raw = _raw_forward(net, inputs, entry, null_cameras=False, extra=extra)
        assert rc != 0 and word in lib.rgbm_last_error(), entry
        for k in OUT_KEYS:
            assert (raw[k] == 7.0).all(), (entry, k)
    with pytest.raises(_lib.RgbmError, match="baseline"):
        net.forward(inputs["img1"], inputs["choose1"], inputs["img2"], inputs["choose2"], inputs["P1"], inputs["P2"], inputs["depths"],
                    dense_depth=True)
    with pytest.raises(_lib.RgbmError, match="baseline"):
        net.forward(inputs["img1"], inputs["choose1"], inputs["img2"], inputs["choose2"], inputs["P1"], inputs["P2"], inputs["depths"],
                    dense_nocs=True)
    with pytest.raises(_lib.RgbmError, match="baseline"):
        net.set_dropout(0.15)
    with pytest.raises(_lib.RgbmError, match="baseline"):
        net.feature_bytes
    with pytest.raises(_lib.RgbmError, match="baseline"):
        net.fetch(B, "prob", 16)
    for key in ("cost_impl", "sparse_tail", "sparse_dec", "sweep_f16", "igemm_conv6"):
        assert lib.rgbm_adapose_set_option(net._h, key.encode(), 0) != 0 and key.encode() in lib.rgbm_last_error(), key
    for kw in (dict(graph=True), dict(norm_mode=1), dict(dropout=0.15), dict(cost_impl=0)):
        with pytest.raises(_lib.RgbmError, match=next(iter(kw))):
            AdaPoseNet(sd, dtype="fp32", arch="baseline", **kw)
    # a v5 handle has no attention stack
    v5 = AdaPoseNet(synth.adapose_state_dict(seed=0), dtype="bf16")
    with pytest.raises(_lib.RgbmError, match="attention stack"):
        v5.view_fusion(np.zeros((1, 32, 32), np.float32), np.zeros((1, 32, 32), np.float32))
    v5.close()
    # and the handle still works
    out = _run(net, inputs)
    assert all(np.isfinite(out[k]).all() for k in OUT_KEYS)


def test_forward_graph_is_refused(sd, inputs):
    net = _net(sd, "fp32")
    lib = _lib.load()
    B = 2
    t = [net._prep(inputs[k], d) for k, d in (("img1", torch.float32), ("img2", torch.float32), ("choose1", torch.int32),
                                              ("choose2", torch.int32), ("P1", torch.float32), ("P2", torch.float32), ("depths", torch.float32))]
    out = net._empty_outputs(B)
    for v in out.values():
        v.fill_(7.0)
    o = _lib.AdaposeOut(*[out[n].data_ptr() for n, _ in _lib.AdaposeOut._fields_])
    ws_ptr, ws_bytes = net._workspace(B)
    nodes, cap = C.c_int32(), C.c_int32()
    side = torch.cuda.Stream()
    rc = lib.rgbm_adapose_forward_graph(net._h, B, *[_lib.ptr(x) for x in t], C.c_void_p(ws_ptr), ws_bytes, C.byref(o),
                                        C.c_void_p(side.cuda_stream), C.byref(nodes), C.byref(cap))
    torch.cuda.synchronize()
    assert rc != 0 and b"baseline" in lib.rgbm_last_error()
    assert all((v == 7.0).all().item() for v in out.values())


# ------------------------------------------------------------------------------------------------------------------ 3. the plugin
def _scene():
    """Two poses: 480x640 8-bit frames with elliptical masks (more than 1024 resized pixels each), the extrinsics of
    synth.adapose_inputs(2, seed=0)."""
    if "scene" not in _CACHE:
        g = np.random.default_rng(3)
        n = 2
        yy, xx = np.mgrid[0:480, 0:640]
        K = np.tile(np.array([[439.31, 0, 320.0], [0, 439.31, 240.0], [0, 0, 1.0]])[None], (n, 1, 1))
        base = synth.adapose_inputs(n, seed=0)
        f1 = np.clip(0.5 + 0.25 * np.cos(xx / 37.0)[None, :, :, None] + 0.2 * g.random((n, 480, 640, 3)), 0, 1)
        f2 = np.clip(0.5 + 0.25 * np.sin(yy / 29.0)[None, :, :, None] + 0.2 * g.random((n, 480, 640, 3)), 0, 1)
        u1, u2 = (np.rint(f * 255.0).astype(np.uint8) for f in (f1, f2))
        m1 = np.stack([((yy - 240) / 60.0) ** 2 + ((xx - 300 - 10 * i) / 90.0) ** 2 <= 1 for i in range(n)]).astype(np.uint8)
        m2 = np.stack([((yy - 250) / 70.0) ** 2 + ((xx - 340 + 10 * i) / 80.0) ** 2 <= 1 for i in range(n)]).astype(np.uint8)
        deq = lambda u: u.astype(np.float32) / np.float32(255)      # noqa: E731
        _CACHE["scene"] = dict(K=_cuda(K), u1=_cuda(u1), u2=_cuda(u2), f1=_cuda(deq(u1)), f2=_cuda(deq(u2)), m1=_cuda(m1), m2=_cuda(m2),
                               E1=_cuda(base["E1"].astype(np.float64)), E2=_cuda(base["E2"].astype(np.float64)))
    return _CACHE["scene"]


def _est(net=None, **cfg):
    from rgbmanip_amd.config import adapose_cfg
    from rgbmanip_amd.estimator import AdaPoseEstimator_baseline
    cfg = dict(adapose_cfg("one_door_cabinet", load=False, name="adapose_baseline"), hip_prepare="device", hip_prepare_seed=9, hip_dtype="fp32", **cfg)
    return AdaPoseEstimator_baseline(None, cfg, None, net=net)


def test_estimator_end_to_end_batch2(sd):
    """`AdaPoseEstimator_baseline.estimate_device` equals the device tail applied to the AdaPoseNet outputs of the same crops, bit for
    bit; 8-bit and float frames agree; the numpy-facing `estimate` too, with whole-frame and crop-window uploads."""
    from rgbmanip_amd.estimator import DEFAULT_BBOX
    c = _scene()
    net = _net(sd, "fp32", options={"view2_heads": 0})
    a = prepare_inputs(c["f1"], c["m1"], c["K"], 224, 1024, 9)
    b = prepare_inputs(c["f2"], c["m2"], c["K"], 224, 1024, 10)
    z = torch.zeros(2, 4, 4, dtype=torch.float32, device="cuda")
    pred = net(a["img"], a["choose"], b["img"], b["choose"], z, z, torch.zeros(2, 24, dtype=torch.float32, device="cuda"))
    want = postprocess(pred["view1_nocs"], pred["view1_depth"], pred["view1_r"], a["choose"], a["Kcrop"], c["E1"])[0].cpu().numpy()
    assert np.isfinite(want).all() and not np.array_equal(want[0], DEFAULT_BBOX)
    est = _est(net=net)
    got = est.estimate_device(c["K"], c["f1"], c["m1"], c["E1"], c["f2"], c["m2"], c["E2"]).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want))
    got8 = est.estimate_device(c["K"], c["u1"], c["m1"], c["E1"], c["u2"], c["m2"], c["E2"]).cpu().numpy()
    assert np.array_equal(_bits(got8), _bits(want)) and est.frames_u8_native == 4
    host_args = [c[k].cpu().numpy() for k in ("K", "u1", "m1", "E1", "u2", "m2", "E2")]
    assert np.array_equal(_bits(est.estimate(*host_args)), _bits(want))
    win = _est(net=net, hip_upload="windows")
    assert np.array_equal(_bits(win.estimate(*host_args)), _bits(want))
    with pytest.raises(NotImplementedError, match="estimate_depth"):
        est.estimate_depth(*host_args)
    with pytest.raises(NotImplementedError, match="estimate_cloud_pose"):
        est.estimate_cloud_pose(*host_args)


def test_estimator_ransac_and_pnp_tails():
    """direct_regression: False builds the network without its pose branch (interface_baseline.py:42-46); the RANSAC tail is the device
    tail on its four outputs, and the PnP tail (use_depth: False) reads view2_nocs, so the view-2 heads are on."""
    from rgbmanip_amd.estimator import DEFAULT_BBOX
    c = _scene()
    est = _est(direct_regression=False, hip_ransac_seed=5)
    assert est.estimator.arch == "baseline" and not est.estimator.regress_pose and not est.view2_heads
    got = est.estimate_device(c["K"], c["f1"], c["m1"], c["E1"], c["f2"], c["m2"], c["E2"]).cpu().numpy()
    a = prepare_inputs(c["f1"], c["m1"], c["K"], 224, 1024, 9)
    b = prepare_inputs(c["f2"], c["m2"], c["K"], 224, 1024, 10)
    z = torch.zeros(2, 4, 4, dtype=torch.float32, device="cuda")
    pred = est.estimator(a["img"], a["choose"], b["img"], b["choose"], z, z, torch.zeros(2, 24, dtype=torch.float32, device="cuda"))
    assert sorted(pred) == sorted(FOUR)
    want = postprocess_ransac(pred["view1_nocs"], pred["view1_depth"], a["choose"], a["Kcrop"], c["E1"], img_size=224, seed=5)[0].cpu().numpy()
    assert got.shape == (2, 8, 3) and np.isfinite(got).all() and np.array_equal(_bits(got), _bits(want))
    with pytest.warns(RuntimeWarning):
        pnp = _est(direct_regression=False, use_depth=False)
        assert pnp.view2_heads
        box = pnp.estimate_device(c["K"], c["f1"], c["m1"], c["E1"], c["f2"], c["m2"], c["E2"]).cpu().numpy()
    assert box.shape == (2, 8, 3) and np.isfinite(box).all()


@pytest.mark.parametrize("key,val", [("hip_feature_cache", True), ("hip_feature_cache", "content"), ("hip_dropout", 0.15),
                                     ("hip_as_shipped", True), ("hip_graph", True)])
def test_estimator_refuses_unsupported_keys(key, val):
    with pytest.raises(ValueError, match=key):
        _est(**{key: val})
