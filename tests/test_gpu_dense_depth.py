"""-m gpu: dense depth and confidence maps from the cost volume (`AdaPoseNet.forward(..., dense_depth=True)`,
`rgbm_adapose_forward_dense`), `depth_to_points`, and `AdaPoseEstimator_v5.estimate_depth` (DESIGN.md "Dense depth maps")."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rgbmanip_amd import _lib, synth, upload  # noqa: E402
from rgbmanip_amd.adapose import AdaPoseNet, prepare_inputs  # noqa: E402
from rgbmanip_amd.cloud import depth_to_points, depth_to_points_ref  # noqa: E402

RTOL_FP32 = 1e-4            # the number tests/test_gpu_adapose.py applies to the point depth
OUT_KEYS = ["view1_nocs", "view2_nocs", "view1_depth", "view2_depth", "view1_r", "view2_r", "view1_t", "view2_t", "view1_s", "view2_s"]
MAP_KEYS = ["view1_depth_map", "view1_depth_conf", "view2_depth_map", "view2_depth_conf"]
H, W = 480, 640
_CACHE = {}


def _rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-12))


def _sd():
    return synth.adapose_state_dict(seed=0, prefix="module.")


def _net(dtype, **kw):
    key = (dtype, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _CACHE:
        _CACHE[key] = AdaPoseNet(_sd(), dtype=dtype, **kw)
    return _CACHE[key]


def _call(net, inp, **kw):
    out = net(inp["img1"], inp["choose1"], inp["img2"], inp["choose2"], inp["P1"], inp["P2"], inp["depths"], **kw)
    torch.cuda.synchronize()
    return out


def _inputs(B, seed):
    key = ("inputs", B, seed)
    if key not in _CACHE:
        _CACHE[key] = synth.adapose_inputs(B, seed=seed)
    return _CACHE[key]


@pytest.fixture(scope="module")
def golden_inputs():
    return _inputs(2, 0)        # the batch tests/golden/adapose_b2*.npz were recorded on


@pytest.fixture(scope="module")
def oracle_maps(golden_inputs, golden_dir):
    """The reference maps of the golden batch, built once: the oracle's feature maps and plane-sweep volumes (oracle.adapose_ref, the
    statements of adapose_forward), cost_reg_net on fused1 / fused2 for the full [B, D, H, W] logits in either norm mode, then softmax
    over D, the expectation with the depth values and the maximum in float64.  {norm_mode: {map key: [2, 224, 224] float64}}."""
    import os

    from oracle import adapose_ref
    sd = adapose_ref.to_torch_sd(synth.adapose_state_dict(seed=0))
    t = {k: torch.from_numpy(v) for k, v in golden_inputs.items()}
    D = t["depths"].shape[1]
    maps = {0: {}, 1: {}}
    with torch.no_grad():
        feat1, feat2 = adapose_ref.pspnet(t["img1"], sd), adapose_ref.pspnet(t["img2"], sd)
        fused = {1: feat1.unsqueeze(2).repeat(1, 1, D, 1, 1) + adapose_ref.homo_warping(feat2, t["P2"], t["P1"], t["depths"]),
                 2: feat2.unsqueeze(2).repeat(1, 1, D, 1, 1) + adapose_ref.homo_warping(feat1, t["P1"], t["P2"], t["depths"])}
        for v in (1, 2):
            for nm in (0, 1):
                logits = adapose_ref.cost_reg_net(fused[v], sd, norm_mode=nm).squeeze(1).double()      # [B, D, H, W]
                p = torch.softmax(logits, dim=1)
                maps[nm][f"view{v}_depth_map"] = (p * t["depths"].double().view(-1, D, 1, 1)).sum(1).numpy()
                maps[nm][f"view{v}_depth_conf"] = p.max(1).values.numpy()
    # the reference's own recorded point depths are these maps at the chosen pixels
    for nm, name in ((0, "adapose_b2.npz"), (1, "adapose_b2_trainbn.npz")):
        g = np.load(os.path.join(golden_dir, name))
        for v in (1, 2):
            at = np.take_along_axis(maps[nm][f"view{v}_depth_map"].reshape(2, -1), golden_inputs[f"choose{v}"], axis=1)
            assert _rel(at, g[f"view{v}_depth"]) < RTOL_FP32, (name, v)
    return maps


def _map_errors(out, ref):
    errs = {}
    for k in MAP_KEYS:
        a = out[k].cpu().numpy()
        assert a.shape == (2, 224, 224) and a.dtype == np.float32 and np.isfinite(a).all(), k
        errs[k] = float(np.abs(a - ref[k]).max()) if k.endswith("conf") else _rel(a, ref[k])
    return errs


# measured on an MI355X against the float64 oracle maps (profiles/dense_depth_ab.txt); the gates are twice these, the convention of
# tests/test_gpu_adapose.py for 16-bit storage
# (bf16: depth 4.65e-3 / 4.36e-3, conf 5.30e-3 / 5.64e-3 for views 1 / 2; fp16: depth 8.23e-4 / 7.07e-4, conf 9.40e-4 / 1.11e-3)
MEASURED_16BIT = {"bf16": {"map": 4.7e-3, "conf": 5.7e-3}, "fp16": {"map": 8.3e-4, "conf": 1.2e-3}}


# ------------------------------------------------------------------------------------------------------------------ 1. the oracle
@pytest.mark.parametrize("dtype", ["fp32", "bf16x3", "bf16", "fp16"])
def test_dense_maps_against_the_oracle(golden_inputs, oracle_maps, dtype):
    """view{1,2}_depth_map / _conf of the golden batch against the float64 oracle maps: every border pixel and both end planes are in
    the comparison, so the zero padding of all six faces is.  depth: max|a - b| / max|b|, conf: max|a - b|.  fp32 and bf16x3: 1e-4.
    bf16 / fp16: twice the measured errors (MEASURED_16BIT)."""
    out = _call(_net(dtype), golden_inputs, dense_depth=True)
    errs = _map_errors(out, oracle_maps[0])
    print(f"{dtype} dense maps vs oracle:", errs)
    for k, e in errs.items():
        gate = RTOL_FP32 if dtype in ("fp32", "bf16x3") else 2 * MEASURED_16BIT[dtype]["conf" if k.endswith("conf") else "map"]
        assert e < gate, (k, errs)


# ------------------------------------------------------------------------------------------------------------------ 2. norm_mode = 1
@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
def test_dense_maps_per_sample_batchnorm_against_the_oracle(golden_inputs, oracle_maps, dtype):
    """The same with per-sample BatchNorm3d statistics (norm_mode = 1: the generic convs write u11 in the plain layout)."""
    out = _call(_net(dtype, norm_mode=1), golden_inputs, dense_depth=True)
    errs = _map_errors(out, oracle_maps[1])
    print(f"{dtype} norm_mode=1 dense maps vs oracle:", errs)
    for k, e in errs.items():
        assert e < RTOL_FP32, (k, errs)


# ------------------------------------------------------------------------------------------------------------------ 3. the point kernel
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("dtype", ["fp32", "bf16x3", "bf16", "fp16"])
def test_map_at_the_chosen_pixels_is_the_point_depth(dtype, B):
    """One dense call: the map gathered at `choose` is the point kernel's depth on the same u11, bit for bit, for both views."""
    inp = _inputs(B, 5)
    out = _call(_net(dtype), inp, dense_depth=True)
    for v in (1, 2):
        ch = torch.from_numpy(inp[f"choose{v}"]).cuda()
        at = out[f"view{v}_depth_map"].flatten(1).gather(1, ch)
        assert torch.equal(at, out[f"view{v}_depth"]), (v, float((at - out[f"view{v}_depth"]).abs().max()))


def test_plain_layout_map_at_the_chosen_pixels_is_the_point_depth():
    """... and through the plain-layout u11 (cost_impl 0: the generic transposed conv writes it)."""
    inp = _inputs(1, 5)
    out = _call(_net("bf16", cost_impl=0), inp, dense_depth=True)
    at = out["view1_depth_map"].flatten(1).gather(1, torch.from_numpy(inp["choose1"]).cuda())
    assert torch.equal(at, out["view1_depth"])


# ------------------------------------------------------------------------------------------------------------------ 4. point outputs
@pytest.mark.parametrize("dtype", ["bf16", "bf16x3"])
def test_point_outputs_are_those_of_the_dense_options(golden_inputs, dtype):
    """The ten point outputs of a dense call on a default net equal a plain forward of a net built with sparse_dec = 0 and the
    dense tail, bit for bit."""
    out = _call(_net(dtype), golden_inputs, dense_depth=True)
    want = _call(_net(dtype, sparse_tail=0, options={"sparse_dec": 0}), golden_inputs)
    for k in OUT_KEYS:
        assert torch.equal(out[k], want[k]), k


# ------------------------------------------------------------------------------------------------------------------ 5. default path
def test_default_forward_is_untouched_by_a_dense_call(golden_inputs):
    """forward() before and after a dense call on the same net: identical tensors, and the sparse options still hold (a 3-D tap is
    refused under the sparse cost regularisation, as before the dense call)."""
    net = AdaPoseNet(_sd(), dtype="bf16")
    before = {k: v.clone() for k, v in _call(net, golden_inputs).items()}
    dense = _call(net, golden_inputs, dense_depth=True)
    assert sorted(dense) == sorted(OUT_KEYS + MAP_KEYS)
    after = _call(net, golden_inputs)
    assert sorted(after) == sorted(OUT_KEYS)
    for k in OUT_KEYS:
        assert torch.equal(before[k], after[k]), k
    assert net.options == {}
    with pytest.raises(_lib.RgbmError, match="sparse_dec"):
        net.fetch(2, "c0", 8)
    assert net.dense_workspace_bytes(2) >= net.workspace_bytes(2)


def test_dense_call_argument_errors(golden_inputs):
    """A workspace smaller than rgbm_adapose_dense_workspace_bytes and a NULL depth_map are refused with a message."""
    net = _net("bf16")
    lib = _lib.load()
    t = [torch.as_tensor(golden_inputs[k]).cuda().to(d).contiguous() for k, d in
         (("img1", torch.float32), ("img2", torch.float32), ("choose1", torch.int32), ("choose2", torch.int32), ("P1", torch.float32),
          ("P2", torch.float32), ("depths", torch.float32))]
    out = net._empty_outputs(2)
    o = _lib.AdaposeOut(*[out[n].data_ptr() for n, _ in _lib.AdaposeOut._fields_])
    maps = torch.zeros(2, 4, 224, 224, device="cuda")
    need = net.dense_workspace_bytes(2)
    ws = torch.empty(need + 256, dtype=torch.uint8, device="cuda")
    ptr, _ = net._aligned(ws)
    args = [net._h, 2] + [_lib.ptr(x) for x in t] + [C.c_void_p(ptr)]
    assert lib.rgbm_adapose_forward_dense(*args, need - 256, C.byref(o), _lib.ptr(maps[0]), _lib.ptr(maps[1]), _lib.stream_ptr()) < 0
    assert b"workspace too small" in lib.rgbm_last_error()
    assert lib.rgbm_adapose_forward_dense(*args, need, C.byref(o), None, _lib.ptr(maps[1]), _lib.stream_ptr()) < 0
    assert b"depth_map" in lib.rgbm_last_error()
    torch.cuda.synchronize()
    assert float(maps.abs().max()) == 0.0                       # nothing ran
    # conf_map may be NULL
    _lib.check(lib.rgbm_adapose_forward_dense(*args, need, C.byref(o), _lib.ptr(maps[0]), None, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert float(maps[0].abs().min()) > 0.0 and float(maps[1].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------------ 6. two chunks
def test_two_chunks_equal_single_pose_calls():
    """max_chunk (an existing option) = 2 views: the B = 2 call walks the chunk loop twice (views 0-1, then 2-3) and writes rows
    v0 .. v0 + Vc of the maps; row by row it equals single-pose calls, to the 1e-5 tests/test_gpu_adapose.py uses for that comparison."""
    inp = _inputs(2, 5)
    out = _call(_net("fp32", max_chunk_views=2), inp, dense_depth=True)
    net1 = _net("fp32")
    for b in range(2):
        o1 = _call(net1, {k: v[b:b + 1] for k, v in inp.items()}, dense_depth=True)
        for k in MAP_KEYS + OUT_KEYS:
            assert _rel(out[k][b:b + 1].cpu().numpy(), o1[k].cpu().numpy()) < 1e-5, (b, k)


# ------------------------------------------------------------------------------------------------------------------ 7. view2_heads = 0
class _generic_kernels_only:
    """Every conv launch on the generic tiles (rgbm_set_tuning ws_min_rows = 2^30), as tests/test_gpu_adapose.py pins the selection for
    its bit-for-bit comparison of 3 against 6 head views: half the views may cross a dispatch threshold of the persistent kernels,
    which sum in another order."""
    def __enter__(self):
        _lib.check(_lib.load().rgbm_set_tuning(b"ws_min_rows", 1 << 30))

    def __exit__(self, *a):
        _lib.check(_lib.load().rgbm_set_tuning(b"ws_min_rows", 0))


@pytest.mark.parametrize("dtype", ["bf16", "bf16x3"])
def test_view1_only_maps_equal_the_full_call(golden_inputs, dtype):
    """view2_heads = 0: only the view-1 maps come back, and they are the full call's view-1 maps bit for bit."""
    with _generic_kernels_only():
        full = _call(_net(dtype), golden_inputs, dense_depth=True)
        one = _call(_net(dtype, options={"view2_heads": 0}), golden_inputs, dense_depth=True)
    assert sorted(k for k in one if "depth_" in k) == ["view1_depth_conf", "view1_depth_map"]
    for k in ("view1_depth_map", "view1_depth_conf", "view1_depth"):
        assert one[k].shape == full[k].shape and torch.equal(one[k], full[k]), k


# ------------------------------------------------------------------------------------------------------------------ 8. depth_to_points
def test_depth_to_points_against_the_float64_twin(golden_inputs):
    g = np.random.default_rng(17)
    depth = g.uniform(0.1, 2.5, (2, 224, 224)).astype(np.float32)
    depth[1, 7, 200] = np.nan
    depth[0, 223, 0] = np.inf
    K, E = golden_inputs["K1"], golden_inputs["E1"]
    pts = depth_to_points(depth, K, E)
    torch.cuda.synchronize()
    got = pts.cpu().numpy()
    want = depth_to_points_ref(depth, K, E)
    assert got.shape == (2, 224, 224, 3) and got.dtype == np.float32
    assert np.isnan(got[1, 7, 200]).all() and np.isnan(got[0, 223, 0]).all() and np.isnan(want[1, 7, 200]).all()
    assert int(np.isnan(got).sum()) == 6
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-7, equal_nan=True)


# ------------------------------------------------------------------------------------------------------------------ 9. the estimator
def _scene():
    """Three poses of float64 host frames with elliptical masks; pose 1's view-1 mask is empty."""
    if "scene" not in _CACHE:
        g = np.random.default_rng(3)
        n = 3
        yy, xx = np.mgrid[0:H, 0:W]
        K = np.tile(np.array([[439.31, 0, 320.0], [0, 439.31, 240.0], [0, 0, 1.0]])[None], (n, 1, 1))
        base = synth.adapose_inputs(n, seed=0)
        f1 = np.clip(0.5 + 0.25 * np.cos(xx / 37.0)[None, :, :, None] + 0.2 * g.random((n, H, W, 3)), 0, 1)
        f2 = np.clip(0.5 + 0.25 * np.sin(yy / 29.0)[None, :, :, None] + 0.2 * g.random((n, H, W, 3)), 0, 1)
        m1 = np.stack([((yy - 240) / 60.0) ** 2 + ((xx - 300 - 10 * i) / 90.0) ** 2 <= 1 for i in range(n)])
        m2 = np.stack([((yy - 250) / 70.0) ** 2 + ((xx - 340 + 10 * i) / 80.0) ** 2 <= 1 for i in range(n)])
        m1[1] = False
        q = lambda f: np.rint(f * 255.0).astype(np.uint8)      # noqa: E731
        _CACHE["scene"] = dict(K=K, E1=base["E1"].astype(np.float64), E2=base["E2"].astype(np.float64), f1=f1, f2=f2, u1=q(f1), u2=q(f2), m1=m1, m2=m2)
    return _CACHE["scene"]


def _estimator(net, **kw):
    from rgbmanip_amd.config import ADAPOSE_CFGS
    from rgbmanip_amd.estimator import AdaPoseEstimator_v5
    cfg = dict(ADAPOSE_CFGS["adapose_cabinet"], load=False, hip_dtype="bf16", hip_prepare="device", hip_prepare_seed=9, **kw)
    return AdaPoseEstimator_v5(None, cfg, None, net=net)


@pytest.mark.parametrize("mode,chunk", [("frames", 32), ("frames", 2), ("windows", 32), ("windows", 2)])
@pytest.mark.parametrize("frames", ["f", "u"])
def test_estimate_depth(frames, mode, chunk):
    """estimate_depth on three 480 x 640 host frames (float64 or uint8; pose 1 has an empty mask), whole-frame and window upload, one
    call and the chunk pipeline."""
    from rgbmanip_amd.estimator import DEFAULT_BBOX
    s = _scene()
    est = _estimator(_net("bf16", options={"view2_heads": 0}), hip_upload=mode, hip_upload_chunk=chunk)
    args = (s["K"], s[frames + "1"], s["m1"], s["E1"], s[frames + "2"], s["m2"], s["E2"])
    r = est.estimate_depth(*args)
    assert all(isinstance(v, np.ndarray) for v in r.values())
    assert r["bbox"].shape == (3, 8, 3) and r["depth"].shape == r["conf"].shape == (3, 224, 224) and r["points"].shape == (3, 224, 224, 3)
    assert r["depth"].dtype == r["conf"].dtype == r["points"].dtype == np.float32 and r["window"].dtype == r["valid"].dtype == np.int32
    assert r["valid"].tolist() == [1, 0, 1]
    assert np.isnan(r["depth"][1]).all() and np.isnan(r["conf"][1]).all() and np.isnan(r["points"][1]).all()
    assert np.array_equal(r["bbox"][1], DEFAULT_BBOX)
    assert np.isfinite(r["depth"][[0, 2]]).all() and np.isfinite(r["points"][[0, 2]]).all()
    assert (r["depth"][[0, 2]] >= 0.1 - 1e-6).all() and (r["depth"][[0, 2]] <= 2.4 + 1e-6).all()         # an expectation over the planes
    assert (r["conf"][[0, 2]] >= 1 / 24 - 1e-6).all() and (r["conf"][[0, 2]] <= 1 + 1e-6).all()
    win, _ = upload.mask_windows(s["m1"])
    assert np.array_equal(r["window"], win)
    # the box: estimate() of an estimator whose net has the dense options
    dense_net = _net("bf16", sparse_tail=0, options={"sparse_dec": 0, "view2_heads": 0})
    want = _estimator(dense_net, hip_upload=mode, hip_upload_chunk=chunk).estimate(*args)
    assert np.array_equal(r["bbox"], want)
    assert not np.array_equal(want[0], DEFAULT_BBOX)
    # the points: depth_to_points of the returned depth with the crop's intrinsics
    u8 = frames == "u"
    rgb1 = torch.from_numpy(s["u1"] if u8 else s["f1"].astype(np.float32)).cuda()
    Kc = prepare_inputs(rgb1, torch.from_numpy(s["m1"]).cuda(), torch.from_numpy(s["K"]).cuda(), seed=9)["Kcrop"]
    assert np.array_equal(r["Kcrop"][[0, 2]], Kc.cpu().numpy()[[0, 2]])
    pts = depth_to_points(r["depth"], r["Kcrop"], s["E1"]).cpu().numpy()
    assert np.array_equal(pts, r["points"], equal_nan=True)
    # the device call, batched as the host call's pipeline batches (chunks of `chunk` poses, frame0 = the chunk's first pose: pieces of
    # other sizes may take other kernels, which sum in another order)
    dev = [rgb1, torch.from_numpy(s["m1"]).cuda(), torch.from_numpy(s["u2"] if u8 else s["f2"].astype(np.float32)).cuda(), torch.from_numpy(s["m2"]).cuda()]
    parts = []
    for a in range(0, 3, chunk):
        b = min(a + chunk, 3)
        parts.append(est.estimate_depth_device(s["K"][a:b], dev[0][a:b], dev[1][a:b], s["E1"][a:b], dev[2][a:b], dev[3][a:b], s["E2"][a:b], frame0=a))
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for d in parts for v in d.values()) and sorted(parts[0]) == sorted(r)
    for k in r:
        assert np.array_equal(torch.cat([d[k] for d in parts]).cpu().numpy(), r[k], equal_nan=True), k


def test_estimate_depth_bypasses_the_feature_cache_and_runs_on_v4():
    from rgbmanip_amd.config import adapose_cfg
    from rgbmanip_amd.estimator import AdaPoseEstimator_v4
    s = _scene()
    args = (s["K"], s["u1"], s["m1"], s["E1"], s["u2"], s["m2"], s["E2"])
    net = _net("bf16", options={"view2_heads": 0})
    est = _estimator(net, hip_feature_cache="content")
    want = _estimator(net).estimate_depth(*args)
    got = est.estimate_depth(*args)
    assert est.feature_cache_bypassed == 1 and est.feature_views_computed == 6
    for k in want:
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    v4 = AdaPoseEstimator_v4(None, dict(adapose_cfg("one_door_cabinet", load=False, name="adapose_v4"), hip_dtype="bf16", hip_prepare="device",
                                        hip_prepare_seed=9), None, net=net)
    r = v4.estimate_depth(*args)
    assert r["valid"].tolist() == [1, 0, 1] and np.isfinite(r["depth"][[0, 2]]).all() and np.array_equal(r["window"], want["window"])
