"""-m gpu: the pose MLP's per-point layers of a bf16 net as two launches (pose_mlp.hip: pose_mlp1_kernel, pose_mlp2_kernel) against
the per-layer launches they replace (debug flag 524288: conversion, four 1x1 GEMMs in f16 storage, two mean kernels) and against a
float64 restatement of the four layers and the two means."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rgbmanip_amd import synth  # noqa: E402

FLAG = 524288               # rgbm_debug_flags: pose MLP as per-layer launches
OUT_KEYS = ["view1_nocs", "view2_nocs", "view1_depth", "view2_depth", "view1_r", "view2_r", "view1_t", "view2_t",
            "view1_s", "view2_s"]
P = 1024


def _net(dtype, **kw):
    from rgbmanip_amd.adapose import AdaPoseNet
    return AdaPoseNet(synth.adapose_state_dict(seed=0, prefix="module."), dtype=dtype, **kw)


@pytest.fixture(scope="module")
def bf16_net():
    return _net("bf16")


class _flags:
    def __init__(self, flags):
        self.flags = flags

    def __enter__(self):
        from rgbmanip_amd import _lib
        _lib.check(_lib.load().rgbm_debug_flags(self.flags))

    def __exit__(self, *a):
        from rgbmanip_amd import _lib
        _lib.check(_lib.load().rgbm_debug_flags(0))


def _run(net, inp, taps=(), views=None):
    """outputs (and the named taps' first `views` rows) of one forward as numpy arrays"""
    out = net(inp["img1"], inp["choose1"], inp["img2"], inp["choose2"], inp["P1"], inp["P2"], inp["depths"])
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    B = len(inp["img1"])
    V = 2 * B
    width = {"pf2": 256, "r6": 6, "pf96": P * 96}
    for t in taps:
        x = net.fetch(B, t, V * width[t]).view(V, width[t]).cpu().numpy()
        res[t] = x[: (views or V)]
    return res


def _rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-12))


@pytest.mark.parametrize("B,view2_heads", [(1, 1), (3, 1), (2, 0)])
def test_two_kernels_match_the_per_layer_launches(B, view2_heads):
    """B = 1: 16 slabs, fewer than CUs; B = 3: an odd view count; B = 2 with view2_heads = 0: the heads run on the view-1 crops only.
    nocs and depth do not depend on this branch: bit-equal.  r / t / s and the pf2 / r6 taps flow through four layers of f16 storage
    whose fp32 sums associate differently in the two paths: 2e-3 of the tensor's maximum, the bound
    test_point_mlp_matches_the_per_layer_launches holds the same quantities to."""
    inp = synth.adapose_inputs(B, seed=8)
    net = _net("bf16", options={"view2_heads": view2_heads})
    Vh = 2 * B if view2_heads else B
    new = _run(net, inp, taps=("pf2", "r6"), views=Vh)
    with _flags(FLAG):
        old = _run(net, inp, taps=("pf2", "r6"), views=Vh)
    errs = {}
    for k in OUT_KEYS + ["pf2", "r6"]:
        side, kind = (k.split("_") + [""])[:2]
        if view2_heads == 0 and side == "view2":
            np.testing.assert_array_equal(new[k], old[k], err_msg=k)      # no heads on the view-2 crops: the same fill in both paths
            continue
        assert np.isfinite(new[k]).all() and np.isfinite(old[k]).all(), k
        if kind in ("nocs", "depth"):
            np.testing.assert_array_equal(new[k], old[k], err_msg=k)
        else:
            errs[k] = _rel(new[k], old[k])
    print(f"B = {B}, view2_heads = {view2_heads}: two pose MLP kernels vs per-layer launches:", errs)
    for k, e in errs.items():
        assert e < 2e-3, (k, errs)


def _f16(x):
    return np.clip(x, -65504.0, 65504.0).astype(np.float16).astype(np.float64)


def _pose_mlp_f64(pf96):
    """pf96 [V][P][96] -> pf2 [V][256]: the four layers and the two means in float64, rounded to f16 where the kernels store (the
    input, the per-point layers' weights, every layer's output behind its ReLU); the global half of pose_mlp2.0 is applied in fp32
    weights to the mean, as view_linear_kernel does."""
    sd = synth.adapose_state_dict(seed=0)
    w = {n: np.asarray(sd[n + ".weight"], dtype=np.float64).reshape(np.asarray(sd[n + ".weight"]).shape[0], -1)
         for n in ("pose_mlp1.0", "pose_mlp1.2", "pose_mlp2.0", "pose_mlp2.2")}
    b = {n: np.asarray(sd[n + ".bias"], dtype=np.float64) for n in w}
    relu = lambda x: np.maximum(x, 0.0)
    x = _f16(pf96.astype(np.float64))
    h1 = _f16(relu(x @ _f16(w["pose_mlp1.0"]).T + b["pose_mlp1.0"]))
    h2 = _f16(relu(h1 @ _f16(w["pose_mlp1.2"]).T + b["pose_mlp1.2"]))
    glob = h2.mean(axis=1)                                                                  # [V][128]
    vbias = glob @ w["pose_mlp2.0"][:, 128:].T + b["pose_mlp2.0"]                           # [V][256]
    h3 = _f16(relu(h2 @ _f16(w["pose_mlp2.0"][:, :128]).T + vbias[:, None, :]))
    h4 = _f16(relu(h3 @ _f16(w["pose_mlp2.2"]).T + b["pose_mlp2.2"]))
    return h4.mean(axis=1)


def test_against_float64(bf16_net):
    """The pf2 tap of both paths against the float64 restatement on the pf96 tap of the same forward, B = 2.  The new path's worst
    error may exceed the old path's by no more than the old path's own spread between B = 2 run whole and run pose by pose (the
    accumulation-order noise the project accepts: the GEMM tiles, and with them the order of the fp32 sums, depend on the batch)."""
    B = 2
    inp = synth.adapose_inputs(B, seed=8)
    new = _run(bf16_net, inp, taps=("pf2", "pf96"))
    with _flags(FLAG):
        old = _run(bf16_net, inp, taps=("pf2", "pf96"))
        ones = [_run(bf16_net, {k: v[b:b + 1] for k, v in inp.items()}, taps=("pf2",))["pf2"] for b in range(B)]
    np.testing.assert_array_equal(new["pf96"], old["pf96"])      # what feeds the MLP does not depend on the path
    ref = _pose_mlp_f64(new["pf96"].reshape(2 * B, P, 96))
    err_new = float(np.abs(new["pf2"] - ref).max())
    err_old = float(np.abs(old["pf2"] - ref).max())
    whole = old["pf2"]                                            # views: pose 0 crop 1, pose 1 crop 1, pose 0 crop 2, pose 1 crop 2
    spread = max(float(np.abs(whole[[b, B + b]] - ones[b]).max()) for b in range(B))
    print(f"pf2 vs float64: new path {err_new:.3e}, per-layer launches {err_old:.3e}; old path whole vs pose by pose {spread:.3e}; "
          f"max |pf2| {np.abs(ref).max():.3e}")
    assert np.isfinite(new["pf2"]).all()
    assert err_new <= err_old + spread, (err_new, err_old, spread)


def test_deterministic_captured_and_poisoned(bf16_net):
    """Two forwards of the same B = 3 inputs are bit-identical (fixed-order sums, no atomics); a replayed hipGraph of the forward
    equals the eager one; a forward on a workspace filled with 0xFF bytes equals a clean one (nothing is read from the buffers the
    two kernels no longer write)."""
    inp = synth.adapose_inputs(3, seed=9)
    a = _run(bf16_net, inp, taps=("pf2",))
    b = _run(bf16_net, inp, taps=("pf2",))
    for k in a:
        assert np.isfinite(a[k]).all(), k
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    gnet = _net("bf16", graph=True)
    g1 = _run(gnet, inp)      # captures
    g2 = _run(gnet, inp)      # replays
    pnet = _net("bf16", poison_workspace=True)
    p = _run(pnet, inp)
    for k in OUT_KEYS:
        np.testing.assert_array_equal(g1[k], a[k], err_msg="capture " + k)
        np.testing.assert_array_equal(g2[k], a[k], err_msg="replay " + k)
        np.testing.assert_array_equal(p[k], a[k], err_msg="poisoned " + k)


@pytest.mark.parametrize("dtype", ["fp16", "fp32", "bf16x3"])
def test_other_storage_types_keep_the_per_layer_launches(dtype):
    """fp16, fp32 and split-pair nets never take the two kernels: the flag changes nothing, bit for bit."""
    inp = synth.adapose_inputs(1, seed=8)
    net = _net(dtype)
    a = _run(net, inp, taps=("pf2",))
    with _flags(FLAG):
        b = _run(net, inp, taps=("pf2",))
    for k in a:
        assert np.isfinite(a[k]).all(), k
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
