"""-m gpu: the two-view consistency check (`depth_consistency`, csrc/depth_consistency.hip) against its float64 twin, the ordered
compaction `cloud_pack` against `depth_to_points`, `prepare_inputs(..., want_mask=True)` and `AdaPoseEstimator_v5.estimate_cloud`
(DESIGN.md section 5k)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rgbmanip_amd import synth, upload  # noqa: E402
from rgbmanip_amd.adapose import AdaPoseNet, prepare_inputs, prepare_inputs_windows  # noqa: E402
from rgbmanip_amd.cloud import cloud_pack, depth_consistency, depth_consistency_ref, depth_to_points  # noqa: E402

S = 224
H, W = 480, 640
MAPS = ("fused", "reproj", "rel")
_CACHE = {}


def _host(r):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items() if v is not None}


def _sphere(B, seed):
    """The sphere scene of tests/test_cloud_host.py: both views' rendered maps and cameras.  Built once, never written."""
    key = ("sphere", B, seed)
    if key not in _CACHE:
        inp = synth.adapose_inputs(B, seed=seed)
        _CACHE[key] = ((synth.sphere_depth(inp["K1"], inp["E1"]), inp["K1"], inp["E1"]), (synth.sphere_depth(inp["K2"], inp["E2"]), inp["K2"], inp["E2"]))
    return _CACHE[key]


def _against_twin(got, want):
    assert got["keep"].dtype == np.uint8 and np.array_equal(got["keep"] != 0, want["keep"])
    for k in MAPS:
        assert got[k].dtype == np.float32
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), k
        err = np.abs(got[k].astype(np.float64) - want[k])
        print(f"{k}: largest |kernel - twin| {np.nanmax(err) if np.isfinite(err).any() else 0:.3e}")
        np.testing.assert_allclose(got[k], want[k], rtol=1e-6, atol=1e-7, equal_nan=True, err_msg=k)


# ------------------------------------------------------------------------------------------------------------------ 1. kernel against twin
@pytest.mark.parametrize("B,seed", [(2, 0), (3, 5)])
def test_depth_consistency_against_the_float64_twin_on_the_sphere_scene(B, seed):
    """Both directions, without and with conf_a (uniform from a fixed seed, conf_min 0.5) and mask_a (an ellipse).  No sampled pixel lies
    within 1e-3 px / 1e-5 of a threshold in float64 (asserted: a property of the inputs), so `keep` must be the twin's exactly."""
    v1, v2 = _sphere(B, seed)
    g = np.random.default_rng(23)
    conf = g.random((B, S, S), dtype=np.float32)
    yy, xx = np.mgrid[0:S, 0:S]
    mask = np.stack([(((yy - 110) / (70.0 + 9 * i)) ** 2 + ((xx - 118) / 95.0) ** 2 <= 1) for i in range(B)]).astype(np.uint8)
    for a, b in ((v1, v2), (v2, v1)):
        for kw in ({}, dict(conf_a=conf, mask_a=mask, conf_min=0.5)):
            want = depth_consistency_ref(*a, *b, **kw)
            s = want["sampled"]
            assert s.sum() > 4000 * B
            assert not (np.abs(want["reproj"][s] - 1.0) < 1e-3).any() and not (np.abs(want["rel"][s] - 0.01) < 1e-5).any()
            if kw:
                assert 0.2 < want["keep"].sum() / s.sum() < 0.6          # both filters bite
            _against_twin(_host(depth_consistency(*a, *b, **kw)), want)


def _exact_rig(n, size):
    """E = identity, power-of-two focal length: ((x - cx) d / f) f / d is x itself, so u and v land on the integers 0 .. size - 1."""
    K = np.tile(np.array([[256.0, 0, size / 2], [0, 256.0, size / 2], [0, 0, 1.0]])[None], (n, 1, 1))
    return K, np.tile(np.eye(4)[None], (n, 1, 1))


def test_depth_consistency_edges_of_a_small_map():
    """S = 8, n = 1, identical cameras on a rig whose round trip is exact: u, v are the integers 0 .. 7, and at 7 the second tap
    min(x0 + 1, S - 1) must stay inside the map (a read past the row would pick up the next row, past the map the NaN guard).  One NaN
    tap drops the four pixels that read it, whatever its weight.  Then view b's principal point moves by 2^-20 pixel: column 7 projects
    just outside [0, 7] and goes by rule 2, every other pixel reads two columns."""
    s = 8
    K, E = _exact_rig(1, s)
    y, x = np.mgrid[0:s, 0:s]
    d = (0.5 + 0.03 * x + 0.02 * y).astype(np.float32)[None]
    guard = torch.full((3, s, s), float("nan"), dtype=torch.float32, device="cuda")      # depth_b sits between NaN maps
    guard[1] = torch.from_numpy(d[0])
    got = _host(depth_consistency(d, K, E, guard[1:2], K, E))
    assert got["keep"].all() and (got["reproj"] == 0).all() and (got["rel"] == 0).all() and np.array_equal(got["fused"], d)
    db = d.copy()
    db[0, 3, 5] = np.nan
    guard[1] = torch.from_numpy(db[0])
    got = _host(depth_consistency(d, K, E, guard[1:2], K, E))
    want = depth_consistency_ref(d, K, E, db, K, E)
    gone = np.zeros((1, s, s), dtype=bool)
    gone[0, 2:4, 4:6] = True
    assert np.array_equal(want["keep"], ~gone)
    _against_twin(got, want)
    Kb = K.copy()
    Kb[:, 0, 2] += 2.0 ** -20
    guard[1] = torch.from_numpy(d[0])
    got = _host(depth_consistency(d, K, E, guard[1:2], Kb, E))
    want = depth_consistency_ref(d, K, E, d, Kb, E)
    assert not want["sampled"][0, :, 7].any() and want["sampled"][0, :, :7].all()
    _against_twin(got, want)
    assert np.isnan(got["fused"][0, :, 7]).all() and np.isnan(got["reproj"][0, :, 7]).all() and not got["keep"][0, :, 7].any()


def test_depth_consistency_invalid_pixels_and_singular_extrinsic():
    v1, v2 = _sphere(2, 0)
    da = v1[0].copy()
    ys, xs = np.nonzero(np.isfinite(da[0]))
    for j, val in enumerate((np.inf, -np.inf, 0.0, -0.4)):
        da[0, ys[100 + j], xs[100 + j]] = val
    Es = v2[2].copy()
    Es[1, 1] = 0.0                                          # pose 1: view b has no inverse
    want = depth_consistency_ref(da, v1[1], v1[2], v2[0], v2[1], Es)
    assert not want["keep"][1].any() and np.isnan(want["reproj"][1]).all() and want["keep"][0].sum() > 4000
    for j in range(4):
        assert np.isnan(want["rel"][0, ys[100 + j], xs[100 + j]])
    _against_twin(_host(depth_consistency(da, v1[1], v1[2], v2[0], v2[1], Es)), want)


def test_depth_consistency_without_the_diagnostic_maps():
    """reproj = rel = NULL: accepted, fused and keep bit for bit those of the full call."""
    v1, v2 = _sphere(2, 0)
    full = depth_consistency(*v1, *v2)
    lean = depth_consistency(*v1, *v2, want_diagnostics=False)
    assert lean["reproj"] is None and lean["rel"] is None
    full, lean = _host(full), _host(lean)
    assert np.array_equal(full["keep"], lean["keep"]) and np.array_equal(full["fused"].view(np.uint32), lean["fused"].view(np.uint32))
    assert full["keep"].sum() > 8000


# ------------------------------------------------------------------------------------------------------------------ 2. cloud_pack
def _pack_reference(f1, k1, K1, E1, f2=None, k2=None, K2=None, E2=None):
    """Per pose: depth_to_points(fused_v)[keep_v] in row-major order, view 1 then view 2; the flat indices; the counts."""
    n = f1.shape[0]
    views = [(f1, k1, K1, E1)] + ([(f2, k2, K2, E2)] if f2 is not None else [])
    pts = [depth_to_points(f, K, E).cpu().numpy().reshape(n, -1, 3) for f, _, K, E in views]
    torch.cuda.synchronize()
    out = []
    for i in range(n):
        idx = [np.flatnonzero(np.asarray(k[i]).reshape(-1) != 0) for _, k, _, _ in views]
        out.append((np.concatenate([p[i][j] for p, j in zip(pts, idx)]),
                    np.concatenate([j + v * S * S for v, j in enumerate(idx)]).astype(np.int32), [len(j) for j in idx] + [0] * (2 - len(idx))))
    return out


def _check_pack(args, cap=None):
    cloud, index, count = (t.cpu().numpy() for t in cloud_pack(*args, max_points=cap))
    torch.cuda.synchronize()
    n = len(args[0])
    full = (2 if len(args) == 8 else 1) * S * S
    cap = full if cap is None else cap
    assert cloud.shape == (n, cap, 3) and cloud.dtype == np.float32 and index.shape == (n, cap) and index.dtype == np.int32
    assert count.shape == (n, 2) and count.dtype == np.int32
    for i, (pts, idx, cnt) in enumerate(_pack_reference(*args)):
        m = min(len(idx), cap)
        assert count[i].tolist() == cnt, i                   # the full counts, whatever cap is
        assert np.array_equal(index[i, :m], idx[:m]), i
        assert np.array_equal(cloud[i, :m].view(np.uint32), pts[:m].view(np.uint32)), i
        assert (index[i, m:] == -1).all() and np.isnan(cloud[i, m:]).all(), i
    return cloud, index, count


def _patterns():
    g = np.random.default_rng(41)
    z = np.zeros(S * S, dtype=np.uint8)
    first, last, stride = z.copy(), z.copy(), z.copy()
    first[0], last[-1] = 1, 1
    stride[::1023] = 1
    return {"ones": np.ones(S * S, dtype=np.uint8), "zeros": z, "first": first, "last": last, "every 1023rd": stride,
            "bernoulli": (g.random(S * S) < 0.5).astype(np.uint8)}


@pytest.mark.parametrize("name", ["ones", "zeros", "first", "last", "every 1023rd", "bernoulli"])
def test_cloud_pack_synthetic_keep_patterns(name):
    """n = 3 with an all-zero pose in the middle; view 2 carries the pattern reversed (and 7 where view 1 has 1: any non-zero byte keeps).
    The patterns put kept pixels on both sides of every boundary of the scan: the 1024-pixel chunks, the eight pieces of a pose
    (12 544 pixels each at S = 224) and the seam between the views."""
    if "pack" not in _CACHE:
        g = np.random.default_rng(7)
        inp = synth.adapose_inputs(3, seed=5)
        _CACHE["pack"] = (g.uniform(0.2, 2.0, (3, S, S)).astype(np.float32), g.uniform(0.2, 2.0, (3, S, S)).astype(np.float32), inp)
    f1, f2, inp = _CACHE["pack"]
    p = _patterns()[name]
    k1 = np.stack([p, np.zeros_like(p), np.roll(p, 517)]).reshape(3, S, S)
    k2 = np.stack([p[::-1] * 7, np.zeros_like(p), p]).reshape(3, S, S)
    args = (f1, k1, inp["K1"], inp["E1"], f2, k2, inp["K2"], inp["E2"])
    a = _check_pack(args)
    b = _check_pack(args)
    for x, y in zip(a, b):                                   # two calls: identical bytes
        assert x.tobytes() == y.tobytes()
    total = int(p.sum()) * 2
    for cap in sorted({0, 1, total // 2, max(total - 1, 0), total + 5}):
        _check_pack(args, cap)
    _check_pack(args[:4])                                    # the one-view form
    _check_pack(args[:4], 3)


def test_cloud_pack_of_the_sphere_check():
    v1, v2 = _sphere(3, 5)
    r1, r2 = depth_consistency(*v1, *v2), depth_consistency(*v2, *v1)
    args = (r1["fused"], r1["keep"], v1[1], v1[2], r2["fused"], r2["keep"], v2[1], v2[2])
    host = tuple(a.cpu().numpy() if isinstance(a, torch.Tensor) else a for a in args)
    cloud, index, count = _check_pack(host)
    assert (count > 4000).all()
    _check_pack(host, 5000)
    _check_pack(host[:4])
    # every point of the cloud lies on the sphere the maps were rendered from
    for i in range(3):
        m = int(count[i].sum())
        r = np.linalg.norm(cloud[i, :m].astype(np.float64) - np.array([0, 0, 0.5]), axis=1)
        assert np.abs(r - 0.12).max() < 2e-3, i


# ------------------------------------------------------------------------------------------------------------------ 3. want_mask
def _scene():
    """The three poses of tests/test_gpu_dense_depth.py::_scene: float64 host frames with elliptical masks; pose 1's view-1 mask is empty."""
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


def test_want_mask_is_the_nearest_resize_of_the_mask_window():
    s = _scene()
    rgb, K = torch.from_numpy(s["u1"]).cuda(), torch.from_numpy(s["K"]).cuda()
    m8 = s["m1"].astype(np.uint8)
    plain = prepare_inputs(rgb, torch.from_numpy(m8).cuda(), K, seed=9)
    got = prepare_inputs(rgb, torch.from_numpy(m8).cuda(), K, seed=9, want_mask=True)
    assert sorted(plain) == ["Kcrop", "choose", "img", "valid", "window"] and sorted(got) == sorted(list(plain) + ["mask"])
    for k in plain:
        assert torch.equal(plain[k], got[k]), k
    mask = got["mask"].cpu().numpy()
    assert mask.shape == (3, S, S) and mask.dtype == np.uint8 and got["valid"].tolist() == [1, 0, 1]
    win, choose = got["window"].cpu().numpy(), got["choose"].cpu().numpy()
    for i in range(3):
        rmin, rmax, cmin, cmax = (int(v) for v in win[i])
        h, w = rmax - rmin, cmax - cmin
        ny = np.minimum(np.floor(np.arange(S) * (h / S)).astype(int), h - 1)      # nearest_tap of csrc/prepare.hip
        nx = np.minimum(np.floor(np.arange(S) * (w / S)).astype(int), w - 1)
        assert np.array_equal(mask[i], m8[i][rmin + ny][:, cmin + nx]), i
        if i != 1:
            assert mask[i].reshape(-1)[choose[i]].all() and 0 < mask[i].sum() < S * S
    assert not mask[1].any()
    # the packed-window form writes the same bytes
    window, valid = upload.mask_windows(m8)
    offset, total = upload.window_offsets(window)
    pix, mpix = np.zeros(3 * total, dtype=np.uint8), np.zeros(total, dtype=np.uint8)
    upload.pack_windows(pix, mpix, s["u1"], m8, 0, 3, window, offset)
    dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (pix, mpix, offset, window, valid)]
    wplain = prepare_inputs_windows(*dev, K, H, W, seed=9)
    wgot = prepare_inputs_windows(*dev, K, H, W, seed=9, want_mask=True)
    assert sorted(wplain) == sorted(plain) and sorted(wgot) == sorted(got)
    assert torch.equal(wgot["mask"], got["mask"]) and torch.equal(wgot["choose"], got["choose"])


# ------------------------------------------------------------------------------------------------------------------ 4. the estimator
def _net(**options):
    key = ("net", tuple(sorted(options.items())))
    if key not in _CACHE:
        _CACHE[key] = AdaPoseNet(synth.adapose_state_dict(seed=0, prefix="module."), dtype="bf16", options=options)
    return _CACHE[key]


def _estimator(net, **kw):
    from rgbmanip_amd.config import ADAPOSE_CFGS
    from rgbmanip_amd.estimator import AdaPoseEstimator_v5
    cfg = dict(ADAPOSE_CFGS["adapose_cabinet"], load=False, hip_dtype="bf16", hip_prepare="device", hip_prepare_seed=9, **kw)
    return AdaPoseEstimator_v5(None, cfg, None, net=net)


DEPTH_KEYS = ["Kcrop", "bbox", "conf", "depth", "points", "valid", "window"]
CLOUD_KEYS = sorted(DEPTH_KEYS + ["depth2", "conf2", "window2", "Kcrop2", "mask1", "mask2", "cloud", "cloud_index", "count"]
                    + [f"{k}{v}" for k in ("fused", "keep", "reproj", "rel") for v in (1, 2)])
# a synthetic net's two maps are unrelated, so the default thresholds keep next to nothing; these let a share of the pixels through
LOOSE = dict(px_max=60.0, rel_max=0.5, conf_min=0.05)


@pytest.mark.parametrize("mode,chunk", [("frames", 32), ("frames", 2), ("windows", 32), ("windows", 2)])
@pytest.mark.parametrize("frames", ["f", "u"])
def test_estimate_cloud(frames, mode, chunk):
    """estimate_cloud on three 480 x 640 host frames (float64 or uint8; pose 1 has an empty mask), whole-frame and window upload, one
    call and the chunk pipeline, on a bf16 net with the view-2 heads."""
    s = _scene()
    est = _estimator(_net(view2_heads=1), hip_view2_heads=True, hip_upload=mode, hip_upload_chunk=chunk)
    args = (s["K"], s[frames + "1"], s["m1"], s["E1"], s[frames + "2"], s["m2"], s["E2"])
    r = est.estimate_cloud(*args, **LOOSE)
    assert sorted(r) == CLOUD_KEYS and all(isinstance(v, np.ndarray) for v in r.values())
    maps32 = ["depth", "conf", "depth2", "conf2"] + [f"{k}{v}" for k in MAPS for v in (1, 2)]
    assert all(r[k].shape == (3, S, S) and r[k].dtype == np.float32 for k in maps32)
    assert all(r[k].shape == (3, S, S) and r[k].dtype == np.uint8 for k in ("mask1", "mask2", "keep1", "keep2"))
    assert r["cloud"].shape == (3, 2 * S * S, 3) and r["cloud"].dtype == np.float32
    assert r["cloud_index"].shape == (3, 2 * S * S) and r["cloud_index"].dtype == np.int32 and r["count"].shape == (3, 2) and r["count"].dtype == np.int32
    assert r["window2"].shape == (3, 4) and r["window2"].dtype == np.int32 and r["Kcrop2"].shape == (3, 3, 3) and r["Kcrop2"].dtype == np.float64
    assert r["valid"].tolist() == [1, 0, 1]
    # the pose with the empty mask
    assert all(np.isnan(r[k][1]).all() for k in maps32) and np.isnan(r["cloud"][1]).all() and (r["cloud_index"][1] == -1).all()
    assert r["count"][1].tolist() == [0, 0] and not r["keep1"][1].any() and not r["keep2"][1].any()
    assert (r["count"][[0, 2]] > 0).all(), r["count"]
    assert np.array_equal(r["window2"], upload.mask_windows(s["m2"])[0])
    # estimate_depth's keys: its own output, bit for bit
    d = est.estimate_depth(*args)
    assert sorted(d) == DEPTH_KEYS
    for k in d:
        assert np.array_equal(r[k], d[k], equal_nan=True), k
    # the checks and the cloud: the public functions on the returned tensors
    assert (r["keep1"] <= r["mask1"]).all() and (r["keep2"] <= r["mask2"]).all()
    c1 = _host(depth_consistency(r["depth"], r["Kcrop"], s["E1"], r["depth2"], r["Kcrop2"], s["E2"], conf_a=r["conf"], mask_a=r["mask1"], **LOOSE))
    c2 = _host(depth_consistency(r["depth2"], r["Kcrop2"], s["E2"], r["depth"], r["Kcrop"], s["E1"], conf_a=r["conf2"], mask_a=r["mask2"], **LOOSE))
    for v, c in ((1, c1), (2, c2)):
        for k in ("fused", "keep", "reproj", "rel"):
            assert np.array_equal(r[f"{k}{v}"], c[k], equal_nan=True), (k, v)
    cloud, index, count = (t.cpu().numpy() for t in cloud_pack(r["fused1"], r["keep1"], r["Kcrop"], s["E1"], r["fused2"], r["keep2"], r["Kcrop2"], s["E2"]))
    assert np.array_equal(r["cloud"], cloud, equal_nan=True) and np.array_equal(r["cloud_index"], index) and np.array_equal(r["count"], count)
    assert count.tolist() == [[int(r["keep1"][i].sum()), int(r["keep2"][i].sum())] for i in range(3)]
    # the device call, chunked as the host call's pipeline chunks
    u8 = frames == "u"
    dev = [torch.from_numpy(s["u1"] if u8 else s["f1"].astype(np.float32)).cuda(), torch.from_numpy(s["m1"]).cuda(),
           torch.from_numpy(s["u2"] if u8 else s["f2"].astype(np.float32)).cuda(), torch.from_numpy(s["m2"]).cuda()]
    parts = []
    for a in range(0, 3, chunk):
        b = min(a + chunk, 3)
        parts.append(est.estimate_cloud_device(s["K"][a:b], dev[0][a:b], dev[1][a:b], s["E1"][a:b], dev[2][a:b], dev[3][a:b], s["E2"][a:b], frame0=a, **LOOSE))
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for p in parts for v in p.values()) and sorted(parts[0]) == CLOUD_KEYS
    for k in r:
        assert np.array_equal(torch.cat([p[k] for p in parts]).cpu().numpy(), r[k], equal_nan=True), k


def test_estimate_cloud_options_and_what_it_leaves_alone():
    """masked=False and max_points; no view-2 heads: ValueError; estimate() and estimate_depth() before and after a cloud call; the
    feature cache is bypassed and counted; AdaPoseEstimator_v4 inherits the call."""
    from rgbmanip_amd.config import adapose_cfg
    from rgbmanip_amd.estimator import AdaPoseEstimator_v4
    s = _scene()
    args = (s["K"], s["u1"], s["m1"], s["E1"], s["u2"], s["m2"], s["E2"])
    net = _net(view2_heads=1)
    est = _estimator(net, hip_view2_heads=True, hip_feature_cache="content")
    box0, depth0 = est.estimate(*args), est.estimate_depth(*args)
    bypassed = est.feature_cache_bypassed
    r = est.estimate_cloud(*args, **LOOSE)
    assert est.feature_cache_bypassed == bypassed + 1
    free = est.estimate_cloud(*args, masked=False, max_points=1000, **LOOSE)
    assert free["cloud"].shape == (3, 1000, 3) and free["cloud_index"].shape == (3, 1000)
    assert (free["keep1"] >= r["keep1"]).all() and free["keep1"].sum() > r["keep1"].sum() and not (free["keep1"] <= free["mask1"]).all()
    assert (free["count"][[0, 2]].sum(1) > 1000).all() and np.isfinite(free["cloud"][[0, 2]]).all() and np.isnan(free["cloud"][1]).all()
    tight = est.estimate_cloud(*args)                       # the defaults: 1 px, 1 %, conf_min 0
    wide = est.estimate_cloud(*args, px_max=60.0, rel_max=0.5)
    assert (tight["keep1"] <= wide["keep1"]).all() and (r["keep1"] <= wide["keep1"]).all() and tight["keep1"].sum() < wide["keep1"].sum()
    assert tight["reproj1"][tight["keep1"] != 0].max() < 1.0 and tight["rel1"][tight["keep1"] != 0].max() < 0.01
    box1, depth1 = est.estimate(*args), est.estimate_depth(*args)
    assert np.array_equal(box0, box1)
    for k in depth0:
        assert np.array_equal(depth0[k], depth1[k], equal_nan=True), k
    with pytest.raises(ValueError, match="hip_view2_heads"):
        _estimator(_net(view2_heads=0)).estimate_cloud(*args)
    with pytest.raises(ValueError, match="hip_view2_heads"):
        _estimator(_net(view2_heads=0)).estimate_cloud_device(*args)
    v4 = AdaPoseEstimator_v4(None, dict(adapose_cfg("one_door_cabinet", load=False, name="adapose_v4"), hip_dtype="bf16", hip_prepare="device",
                                        hip_prepare_seed=9, hip_view2_heads=True), None, net=net)
    q = v4.estimate_cloud(*args, **LOOSE)
    assert sorted(q) == CLOUD_KEYS and q["valid"].tolist() == [1, 0, 1] and q["count"][1].tolist() == [0, 0]
