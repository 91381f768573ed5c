"""-m gpu: the feature cache (DESIGN.md "Feature cache") — `AdaPoseNet.features` / `forward_cached` against the plain forward and
the reference golden, and `AdaPoseEstimator_v5(cfg hip_feature_cache)` inside the controller loop against the uncached estimator.

Gates are the ones the project applies per storage type: RTOL_FP32 = 1e-4 for fp32 and bf16x3, GATE_BF16 / GATE_FP16 of
tests/test_gpu_at_batch.py (twice the errors of the 16-bit modes against the same golden at B = 2) for the 16-bit modes."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_at_batch import GATE_BF16, GATE_FP16, OUT_KEYS, RTOL_FP32, _rel  # noqa: E402

from rgbmanip_amd import synth  # noqa: E402

DTYPES = ["fp32", "bf16x3", "bf16", "fp16"]


def _gate(dtype, key):
    if dtype in ("fp32", "bf16x3"):
        return RTOL_FP32
    return (GATE_BF16 if dtype == "bf16" else GATE_FP16)[key.split("_")[1]]


def _net(dtype, **kw):
    from rgbmanip_amd.adapose import AdaPoseNet
    return AdaPoseNet(synth.adapose_state_dict(seed=0, prefix="module."), dtype=dtype, **kw)


@pytest.fixture(scope="module")
def inp():
    return {k: torch.from_numpy(v).cuda() for k, v in synth.adapose_inputs(2, seed=0).items()}


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "adapose_b2.npz"))
    return {k: g[k] for k in OUT_KEYS}


def _plain(net, inp):
    out = net(inp["img1"], inp["choose1"], inp["img2"], inp["choose2"], inp["P1"], inp["P2"], inp["depths"])
    torch.cuda.synchronize()
    return out


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


def _cached_identity(net, inp):
    pool = net.feature_pool(4)
    net.features(torch.cat((inp["img1"], inp["img2"])), _i32([0, 1, 2, 3]), pool)
    out = net.forward_cached(pool, _i32([0, 1]), _i32([2, 3]), inp["choose1"], inp["choose2"], inp["P1"], inp["P2"], inp["depths"])
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dtype,norm_mode", [(d, 0) for d in DTYPES] + [("bf16x3", 1)])
def test_cached_forward_is_bit_identical_at_equal_shapes(inp, dtype, norm_mode):
    """features() on the 2B views in [view1 ; view2] order in one call + forward_cached with identity slots == the plain forward, bit
    for bit, all ten outputs (view2_heads on).  bf16x3 with per-sample BatchNorm is the case whose record holds two maps."""
    net = _net(dtype, norm_mode=norm_mode)
    one = 224 * 224 * 32
    want = {"fp32": 4, "bf16": 2, "fp16": 2, "bf16x3": 8 if norm_mode else 4}[dtype] * one
    assert net.feature_bytes == want
    ref = _plain(net, inp)
    got = _cached_identity(net, inp)
    ref2 = _plain(net, inp)
    for k in OUT_KEYS:
        assert torch.isfinite(ref[k]).all(), k
        assert torch.equal(got[k], ref[k]), (dtype, norm_mode, k, _rel(got[k].cpu().numpy(), ref[k].cpu().numpy()))
        assert torch.equal(ref2[k], ref[k]), k          # and the plain forward is what it was after the cache used the workspace


def _poisoned_pool(net, records):
    pool = net.feature_pool(records)
    pool.fill_(0xFF)                                    # NaN in every storage type
    return pool


@pytest.mark.parametrize("dtype", DTYPES)
def test_split_calls_and_indirection(inp, golden, dtype):
    """The view-2 frames in one features() call, the view-1 frames (and a spare frame) in a later one of another V, scattered to
    permuted records of a larger pool full of NaN; pose 2 reads pose 0's frames the other way round, so one frame is view 2 of one pose
    and view 1 of another.  Poses 0 / 1 against the golden, pose 2 against the golden with the views exchanged."""
    net = _net(dtype)
    pool = _poisoned_pool(net, 9)
    net.features(inp["img2"], _i32([7, 2]), pool)
    net.features(torch.cat((inp["img1"], torch.zeros_like(inp["img1"][:1]))), _i32([5, 0, 8]), pool)
    pick = lambda a, b: torch.stack((inp[a][0], inp[a][1], inp[b][0]))      # noqa: E731
    out = net.forward_cached(pool, _i32([5, 0, 7]), _i32([7, 2, 5]), pick("choose1", "choose2"), pick("choose2", "choose1"),
                             pick("P1", "P2"), pick("P2", "P1"), pick("depths", "depths"))
    torch.cuda.synchronize()
    errs = {}
    for k in OUT_KEYS:
        got = out[k].cpu().numpy()
        assert np.isfinite(got).all(), k
        other = k.replace("view1", "viewX").replace("view2", "view1").replace("viewX", "view2")
        errs[k] = max(_rel(got[:2], golden[k]), _rel(got[2], golden[other][0]))
    print(f"{dtype} split calls + indirection vs golden:", errs)
    for k in OUT_KEYS:
        assert errs[k] < _gate(dtype, k), (k, errs)


@pytest.mark.parametrize("dtype", DTYPES)
def test_odd_and_small_view_counts(inp, golden, dtype):
    """features() with V = 1 and V = 3: the outputs computed from those records against the golden and against the outputs computed
    from the records of one even-V call, inside the storage type's gates."""
    net = _net(dtype)
    even = {k: v.cpu().numpy() for k, v in _cached_identity(net, inp).items()}
    frames = torch.cat((inp["img1"], inp["img2"]))
    pools = {}
    p1 = _poisoned_pool(net, 4)
    for v in range(4):
        net.features(frames[v:v + 1], _i32([v]), p1)                      # four calls of V = 1
    pools["V=1"] = p1
    p3 = _poisoned_pool(net, 4)
    net.features(frames[1:4], _i32([1, 2, 3]), p3)                        # V = 3, then the remaining frame alone
    net.features(frames[0:1], _i32([0]), p3)
    pools["V=3"] = p3
    for name, pool in pools.items():
        out = net.forward_cached(pool, _i32([0, 1]), _i32([2, 3]), inp["choose1"], inp["choose2"], inp["P1"], inp["P2"], inp["depths"])
        torch.cuda.synchronize()
        errs = {k: (_rel(out[k].cpu().numpy(), golden[k]), _rel(out[k].cpu().numpy(), even[k])) for k in OUT_KEYS}
        print(f"{dtype} {name} (vs golden, vs even-V records):", errs)
        for k in OUT_KEYS:
            assert np.isfinite(out[k].cpu().numpy()).all(), (name, k)
            assert errs[k][0] < _gate(dtype, k) and errs[k][1] < _gate(dtype, k), (name, k, errs)


def test_dropout_net_is_refused_and_launches_nothing(inp):
    from rgbmanip_amd._lib import RgbmError
    net = _net("bf16", dropout=0.15, dropout_seed=3)
    pool = net.feature_pool(4)
    pool.fill_(0x5A)
    with pytest.raises(RgbmError, match="Dropout2d"):
        net.features(torch.cat((inp["img1"], inp["img2"])), _i32([0, 1, 2, 3]), pool)
    with pytest.raises(RgbmError, match="Dropout2d"):
        net.forward_cached(pool, _i32([0, 1]), _i32([2, 3]), inp["choose1"], inp["choose2"], inp["P1"], inp["P2"], inp["depths"])
    torch.cuda.synchronize()
    assert bool((pool == 0x5A).all())                  # no record was written
    net.set_dropout(0.0)
    net.features(torch.cat((inp["img1"], inp["img2"])), _i32([0, 1, 2, 3]), pool)      # off again: accepted
    torch.cuda.synchronize()
    assert not bool((pool == 0x5A).all())


@pytest.mark.parametrize("dtype", ["bf16x3", "bf16"])
@pytest.mark.parametrize("bad", [4, 1 << 20, -1])
def test_out_of_range_slot_gives_nan_for_that_pose_only(inp, dtype, bad):
    net = _net(dtype)
    pool = net.feature_pool(4)
    frames = torch.cat((inp["img1"], inp["img2"]))
    net.features(frames, _i32([0, 1, 2, 3]), pool)
    args = (inp["choose1"], inp["choose2"], inp["P1"], inp["P2"], inp["depths"])
    clean = net.forward_cached(pool, _i32([0, 1]), _i32([2, 3]), *args)
    before = pool.clone()
    net.features(frames[:1], _i32([bad]), pool)                             # a store outside the pool writes nothing
    torch.cuda.synchronize()
    assert torch.equal(pool, before)
    for s1, s2, pose in (([0, bad], [2, 3], 1), ([0, 1], [bad, 3], 0)):
        out = net.forward_cached(pool, _i32(s1), _i32(s2), *args)
        torch.cuda.synchronize()
        for k in OUT_KEYS:
            assert bool(torch.isnan(out[k][pose]).all()), (k, pose)
            assert torch.equal(out[k][1 - pose], clean[k][1 - pose]), (k, pose)


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
def test_controller_rollout_with_and_without_the_cache(dtype):
    """SyntheticMultiVecEnv (8 envs, fixed seed) under ControlInterface: reset + one full episode with the estimator's cache on against
    off, identical actions.  Every step's pred_bbox agrees to the tensor-normalised 1e-4, the default-bbox entries are the same ones,
    and the PSPNet runs on exactly the rows written since the previous estimation — N views per estimation (and the reset row's N
    with the first one, which meets two new rows) — where the uncached path runs 2N."""
    from rgbmanip_amd import synthetic_env as se
    from rgbmanip_amd.config import ADAPOSE_CFGS
    from rgbmanip_amd.control_interface import ControlInterface
    from rgbmanip_amd.estimator import DEFAULT_BBOX, AdaPoseEstimator_v5
    N = 8
    sd = synth.adapose_state_dict(seed=0, prefix="module.")
    runs = {}
    for cache in (False, True):
        cfg = dict(ADAPOSE_CFGS["adapose_cabinet"], load=False, hip_prepare="device", hip_prepare_seed=1)
        if cache:
            cfg["hip_feature_cache"] = True
        est = AdaPoseEstimator_v5(None, cfg, None, state_dict=sd, dtype=dtype)
        env = se.SyntheticMultiVecEnv(N, "cuda", seed=3)
        ci = ControlInterface(env, est, se.SyntheticManipulation(env), synth.control_cfg("cabinet", 0.0))
        steps = ci.max_steps - 1
        boxes, counts = [], []
        for s in range(steps):
            before = est.feature_views_computed
            ci.step(torch.from_numpy(synth.control_actions(N, s, 9) * 0.3).cuda())
            counts.append(est.feature_views_computed - before)
            boxes.append(ci.pred_bbox[s + 1].cpu().numpy().copy())
        runs[cache] = (np.stack(boxes), counts)
    (off, n_off), (on, n_on) = runs[False], runs[True]
    assert n_off == [2 * N] * len(n_off)
    assert n_on == [2 * N] + [N] * (len(n_on) - 1), n_on
    dflt = lambda b: np.all(b == DEFAULT_BBOX[None, None], axis=(2, 3))      # noqa: E731  [steps, N]
    assert np.array_equal(dflt(off), dflt(on))
    assert not dflt(off).all()                                                # handles are seen: real boxes are compared
    errs = [_rel(on[s], off[s]) for s in range(len(off))]
    print(f"{dtype} rollout, cache on vs off, per step:", errs, "default entries per step:", dflt(off).sum(1))
    assert np.isfinite(on).all()
    assert max(errs) < 1e-4, errs
