"""-m gpu: seeded Dropout2d of PSPNet (rgbm_adapose_set_dropout / _dropout_masks / _set_dropout_masks): parity with the reference's
own Dropout2d through recorded masks, drawn masks against the numpy restatement (tests/dropout_ref.py), independence of batching,
chunking and graph replay, the factors in the up_1 / up_2 taps, and the off switch."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dropout_ref  # noqa: E402
from rgbmanip_amd import synth  # noqa: E402

RTOL_FP32 = 1e-4
OUT_KEYS = ["view1_nocs", "view2_nocs", "view1_depth", "view2_depth", "view1_r", "view2_r", "view1_t", "view2_t",
            "view1_s", "view2_s"]


def _rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-12))


def _net(dtype, **kw):
    from rgbmanip_amd.adapose import AdaPoseNet
    return AdaPoseNet(synth.adapose_state_dict(seed=0, prefix="module."), dtype=dtype, **kw)


def _run(net, inp, **kw):
    out = net(inp["img1"], inp["choose1"], inp["img2"], inp["choose2"], inp["P1"], inp["P2"], inp["depths"], **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _repeat(inp, B):
    """pose 0 of `inp` repeated B times, on the device (masks are drawn per pose whatever the inputs)"""
    return {k: torch.from_numpy(np.ascontiguousarray(v[:1])).cuda().expand(B, *v.shape[1:]).contiguous() for k, v in inp.items()}


class _generic_kernels_only:
    """conv launches on the generic tiles while inside (rgbm_set_tuning ws_min_rows): batches of different sizes then sum in the same
    order, so their outputs can be compared bit for bit"""
    def __enter__(self):
        from rgbmanip_amd import _lib
        _lib.check(_lib.load().rgbm_set_tuning(b"ws_min_rows", 1 << 30))

    def __exit__(self, *a):
        from rgbmanip_amd import _lib
        _lib.check(_lib.load().rgbm_set_tuning(b"ws_min_rows", 0))


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
def test_as_shipped_matches_reference_dropout_golden(golden_dir, dtype):
    """norm_mode = 1 + the reference's own Dropout2d masks (recorded by tools/make_goldens.py::gen_adapose_dropout, the module in
    .train(), one pose per call) against its ten outputs: inside the fp32 gate in fp32, within 1e-4 in bf16x3."""
    g = np.load(os.path.join(golden_dir, "adapose_b2_dropout.npz"))
    inp = synth.adapose_inputs(2, seed=0)
    net = _net(dtype, norm_mode=1)
    net.set_dropout_masks(g["masks"])
    out = _run(net, inp)
    np.testing.assert_array_equal(net.dropout_masks(2).cpu().numpy(), g["masks"])
    errs = {k: _rel(out[k], g[k]) for k in OUT_KEYS}
    print(f"{dtype} norm_mode=1 + dropout masks vs reference:", errs)
    for k in OUT_KEYS:
        assert np.isfinite(out[k]).all(), k
        assert errs[k] < RTOL_FP32, (k, errs)
    # the masks matter: without them the same net is far from the golden
    off = _run(net, inp)
    assert max(_rel(off[k], g[k]) for k in OUT_KEYS) > 10 * RTOL_FP32


def test_drawn_masks_equal_numpy_restatement():
    """Forwards of B = 1, 8 and 256 after set_dropout: the masks read back are the numpy restatement's bit for bit, the pose counter
    running on across the three calls (first poses 0, 1, 9), for two seeds."""
    net = _net("bf16")
    base = synth.adapose_inputs(1, seed=3)
    for seed in (0, 0x1234_5678_9ABC_DEF0):
        net.set_dropout(0.15, seed)
        first = 0
        for B in (1, 8, 256):
            _run(net, _repeat(base, B), stop_after=1)
            got = net.dropout_masks(B).cpu().numpy()
            np.testing.assert_array_equal(got, dropout_ref.masks(0.15, seed, B, first_pose=first), err_msg=f"seed {seed} B {B}")
            first += B
    assert 0.8 < float((got != 0).mean()) < 0.9


def test_masks_and_outputs_do_not_depend_on_batching():
    """After a reset, 8 poses in one forward and 4 + 4 in two give the same masks and (kernel selection pinned) the same outputs bit
    for bit; the cost-volume chunk size changes nothing."""
    inp = synth.adapose_inputs(8, seed=4)
    net = _net("bf16", dropout=0.15, dropout_seed=11)
    with _generic_kernels_only():
        one = _run(net, inp)
        m8 = net.dropout_masks(8).cpu().numpy()
        net.set_dropout(0.15, 11)
        halves, mh = [], []
        for lo in (0, 4):
            halves.append(_run(net, {k: v[lo:lo + 4] for k, v in inp.items()}))
            mh.append(net.dropout_masks(4).cpu().numpy())
    for view in range(2):
        np.testing.assert_array_equal(m8[view * 8:(view + 1) * 8], np.concatenate([m[view * 4:(view + 1) * 4] for m in mh]))
    for k in OUT_KEYS:
        np.testing.assert_array_equal(one[k], np.concatenate([h[k] for h in halves]), err_msg=k)
    # max_chunk 512 and 32 views: the same masks (16 poses = 32 views: one chunk / two chunks of 16 poses' views each)
    got = []
    for chunk in (512, 16):
        n = _net("bf16", dropout=0.15, dropout_seed=11, max_chunk_views=chunk)
        _run(n, _repeat(inp, 16))
        got.append(n.dropout_masks(16).cpu().numpy())
    np.testing.assert_array_equal(got[0], got[1])
    np.testing.assert_array_equal(got[0], dropout_ref.masks(0.15, 11, 16))


def test_graph_replay_draws_the_eager_mask_sequence():
    """forward_graph (capture on the first call, replays after) and eager forwards draw the same masks over three calls — the
    warm-up forward in front of the capture does not advance the counter — the three calls differ, and so do the outputs."""
    inp = synth.adapose_inputs(2, seed=5)
    eager = _net("bf16x3", dropout=0.15, dropout_seed=3)
    graph = _net("bf16x3", dropout=0.15, dropout_seed=3, graph=True)
    seq = []
    for i in range(3):
        a = _run(eager, inp)
        b = _run(graph, inp)
        ma, mb = eager.dropout_masks(2).cpu().numpy(), graph.dropout_masks(2).cpu().numpy()
        np.testing.assert_array_equal(ma, mb, err_msg=f"call {i}")
        np.testing.assert_array_equal(ma, dropout_ref.masks(0.15, 3, 2, first_pose=2 * i))
        for k in OUT_KEYS:
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"call {i} {k}")
        seq.append((ma, a))
    assert graph.last_graph_nodes > 50
    for i in range(3):
        for j in range(i):
            assert not np.array_equal(seq[i][0], seq[j][0])
            assert not np.array_equal(seq[i][1]["view1_r"], seq[j][1]["view1_r"])


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "bf16x3"])
def test_taps_are_the_undropped_taps_times_the_factors(dtype):
    """fetch("u1") / fetch("u2") with masks set equal the dropout-off taps times each channel's factor, within one rounding of the
    storage type (the factor multiplies the fp32 value before it is rounded; split pairs: before the hi / lo split).  Each site is
    checked with the other site's factors at 1 (u2 is computed from the dropped u1)."""
    inp = synth.adapose_inputs(2, seed=6)
    B, V = 2, 4
    shapes = {"u1": (256, 56), "u2": (64, 112)}
    net = _net(dtype)

    def taps(masks=None):
        if masks is not None:
            net.set_dropout_masks(masks)
        _run(net, inp, stop_after=1)
        return {n: net.fetch(B, n, V * H * H * C).view(V, H, H, C).cpu().numpy() for n, (C, H) in shapes.items()}
    ref = taps()
    m = dropout_ref.masks(0.15, 21, B)
    ulp = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11, "bf16x3": 2.0 ** -15}[dtype]
    for n, cols in (("u1", slice(0, 256)), ("u2", slice(256, 320))):
        mm = np.ones_like(m)
        mm[:, cols] = m[:, cols]
        got = taps(mm)
        other = "u2" if n == "u1" else "u1"
        if n == "u2":
            np.testing.assert_array_equal(got[other], ref[other])        # factor 1.0 is exact
        f = m[:, None, None, cols]
        want = ref[n].astype(np.float64) * f
        assert (got[n][np.broadcast_to(f == 0, got[n].shape)] == 0).all(), n
        # both sides are one rounding of the same fp32 product: at most two units of the storage type's last place apart
        tol = 2 * ulp * np.abs(want) + (6e-8 if dtype == "fp16" else 0.0)
        bad = np.abs(got[n] - want) > tol
        assert not bad.any(), (n, int(bad.sum()), float(np.abs(got[n] - want).max()))
        assert float(np.abs(got[n]).max()) > 0


def test_dropout_off_is_bit_identical():
    """p = 0 (never set, or set and switched off again) computes what a handle that never heard of dropout computes, bit for bit."""
    inp = synth.adapose_inputs(2, seed=7)
    plain = _run(_net("bf16"), inp)
    n = _net("bf16", dropout=0.15, dropout_seed=5)
    on = _run(n, inp)
    n.set_dropout(0.0, 0)
    off = _run(n, inp)
    zero = _run(_net("bf16", dropout=0.0), inp)
    for k in OUT_KEYS:
        np.testing.assert_array_equal(off[k], plain[k], err_msg=k)
        np.testing.assert_array_equal(zero[k], plain[k], err_msg=k)
    assert not np.array_equal(on["view1_nocs"], plain["view1_nocs"])


def test_dropout_refuses_upconv_ab_paths():
    from rgbmanip_amd import _lib
    inp = synth.adapose_inputs(1, seed=8)
    net = _net("bf16", options={"upconv": 4}, dropout=0.15)
    with pytest.raises(_lib.RgbmError, match="upconv"):
        _run(net, inp)


def test_estimator_as_shipped_draws_fresh_masks_per_call():
    """hip_as_shipped: true (per-sample BatchNorm3d + Dropout2d 0.15): two estimate calls on the same frames give different boxes,
    re-seeding reproduces the first call exactly; a shared net with another dropout setting is refused."""
    from rgbmanip_amd.config import ADAPOSE_CFGS
    from rgbmanip_amd.estimator import AdaPoseEstimator_v5
    rng = np.random.default_rng(2)
    N, H, W = 2, 480, 640
    rgb = rng.random((N, H, W, 3), dtype=np.float32)
    yy, xx = np.mgrid[0:H, 0:W]
    mask = np.zeros((N, H, W), np.uint8)
    mask[0] = (((yy - 250) / 120.0) ** 2 + ((xx - 300) / 170.0) ** 2) < 1.0
    mask[1] = (((yy - 200) / 90.0) ** 2 + ((xx - 350) / 110.0) ** 2) < 1.0
    K = np.tile(np.array([[439.31, 0, 320.0], [0, 439.31, 240.0], [0, 0, 1.0]]), (N, 1, 1))
    inp = synth.adapose_inputs(N, seed=2)
    E1, E2 = inp["E1"].astype(np.float64), inp["E2"].astype(np.float64)
    cfg = dict(ADAPOSE_CFGS["adapose_cabinet"], load=False, hip_as_shipped=True, hip_dropout_seed=4)
    sd = synth.adapose_state_dict(seed=0, prefix="module.")
    est = AdaPoseEstimator_v5(None, cfg, None, state_dict=sd, dtype="bf16x3")
    assert est.estimator.norm_mode == 1 and est.estimator.dropout == 0.15
    b1 = est.estimate(K, rgb, mask, E1, rgb[:, :, ::-1].copy(), mask[:, :, ::-1].copy(), E2)
    b2 = est.estimate(K, rgb, mask, E1, rgb[:, :, ::-1].copy(), mask[:, :, ::-1].copy(), E2)
    assert np.isfinite(b1).all() and np.isfinite(b2).all()
    assert not np.array_equal(b1, b2)
    est.estimator.set_dropout(0.15, 4)
    b3 = est.estimate(K, rgb, mask, E1, rgb[:, :, ::-1].copy(), mask[:, :, ::-1].copy(), E2)
    np.testing.assert_array_equal(b3, b1)
    with pytest.raises(ValueError, match="dropout"):
        AdaPoseEstimator_v5(None, dict(cfg, hip_as_shipped=False), None, net=est.estimator)
    assert AdaPoseEstimator_v5(None, cfg, None, net=est.estimator).estimator is est.estimator
