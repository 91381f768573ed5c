"""-m gpu: the dense NOCS map (`dense_nocs_kernel`, `rgbm_nocs_map`, `AdaPoseNet.forward(..., dense_nocs=True)` /
`rgbm_adapose_forward_maps`) and `cloud_gather`."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rgbmanip_amd import synth  # noqa: E402
from rgbmanip_amd.adapose import AdaPoseNet, nocs_map  # noqa: E402
from rgbmanip_amd.cloud import cloud_gather  # noqa: E402

RTOL_FP32 = 1e-4            # the project's tensor-normalised gate (tests/test_gpu_adapose.py)
KERNEL_ATOL = 2e-6          # the fp32 entry of tests/test_gpu_adapose.py:781, on tanh-bounded values
OUT_KEYS = ["view1_nocs", "view2_nocs", "view1_depth", "view2_depth", "view1_r", "view2_r", "view1_t", "view2_t", "view1_s", "view2_s"]
S = 224
_CACHE = {}


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


def _branch64(feat):
    """The four layers in float64 torch from the state dict: feat [N, 32] -> [N, 3]."""
    sd = {k: torch.from_numpy(np.asarray(v)).double() for k, v in synth.adapose_state_dict(seed=0).items()
          if k.startswith(("instance_color.", "nocs_head."))}
    x = torch.as_tensor(feat).double()
    for name, act in (("instance_color.0", torch.relu), ("nocs_head.0", torch.relu), ("nocs_head.2", torch.relu), ("nocs_head.4", torch.tanh)):
        x = act(x @ sd[name + ".weight"].reshape(sd[name + ".weight"].shape[0], -1).T + sd[name + ".bias"])
    return x.numpy()


def _branch32(feat):
    """The same four layers in float32 torch on the CPU: what the number format itself resolves."""
    sd = {k: torch.from_numpy(np.asarray(v)).float() for k, v in synth.adapose_state_dict(seed=0).items()
          if k.startswith(("instance_color.", "nocs_head."))}
    x = torch.as_tensor(feat).float()
    for name, act in (("instance_color.0", torch.relu), ("nocs_head.0", torch.relu), ("nocs_head.2", torch.relu), ("nocs_head.4", torch.tanh)):
        x = act(x @ sd[name + ".weight"].reshape(sd[name + ".weight"].shape[0], -1).T + sd[name + ".bias"])
    return x.double().numpy()


def _features(V, HW, seed):
    """Random features with |x| up to 650: uniform values under a per-pixel amplitude of 1 or 25 (alternating), and eight pixels — the
    first, the last and six drawn ones — under an amplitude of 650 in all 32 channels.  Returns (feat [V, HW, 32] f32, the eight pixels)."""
    g = np.random.default_rng(seed)
    n = V * HW
    amp = np.array([1.0, 25.0])[np.arange(n) % 2]
    big = np.concatenate([[0, n - 1], g.choice(np.arange(1, n - 1), 6, replace=False)])
    amp[big] = 650.0
    return (g.uniform(-1, 1, (n, 32)) * amp[:, None]).astype(np.float32).reshape(V, HW, 32), big


# ------------------------------------------------------------------------------------------------------------------ 1. the kernel alone
# (V, HW, seed).  The seeds are the first of 0, 1, 2, ... for which float32 torch stays within 5e-7 of float64 (6, 6 and 8 seeds tried): half
# of what the condition below asserts, so that another BLAS's summation order does not decide it.
KERNEL_CASES = [(1, 64, 5), (3, 64, 5), (257, 64, 7)]
FP32_RESOLVES = 1e-6        # half the gate


@pytest.mark.parametrize("V,HW,seed", KERNEL_CASES)
def test_kernel_against_float64(V, HW, seed):
    """V * HW = 64 (one tile), 192 (three tiles: fewer than the workgroup count can share evenly), 64 * 257 (more tiles than CUs: the
    persistent walk); random features with |x| up to 650; the four layers in float64 torch; max |a - b| <= 2e-6 over every output.

    A condition on the inputs, asserted here like the threshold margin of tests/test_cloud_fit_host.py: a plain float32 evaluation of
    the four layers (torch on the CPU) agrees with the float64 reference to 1e-6, half the gate.  The pre-tanh sums grow with the
    feature amplitude (ReLU layers are homogeneous), an fp32 sum of terms of size M is good to about 2^-24 M, and tanh passes that
    on unreduced where the sum lands near zero; so whether fp32 can resolve an output of a 650-amplitude pixel to 2e-6 depends on where
    its three sums land.  Features at amplitude 650 in EVERY pixel are beyond fp32 (float32 torch and the kernel alike: 6.0e-06 /
    4.5e-06 / 1.3e-05 at the three shapes, profiles/dense_nocs_ab.txt); with eight such pixels per case most seeds leave one output
    1e-6 .. 5e-6 off in float32 torch.  The seeds used are those for which the number format resolves every output; the kernel then has
    the other half of the gate for summing in another order.  Several of the 24 outputs of the large pixels are unsaturated (asserted)."""
    feat, big = _features(V, HW, seed)
    flat = feat.reshape(-1, 32)
    want = _branch64(flat)
    assert 640 < np.abs(flat).max() <= 650 and (np.abs(want[big]) < 0.999).sum() >= 3
    fmt = float(np.abs(_branch32(flat) - want).max())
    assert fmt <= FP32_RESOLVES, ("inputs beyond what float32 resolves", fmt)
    got = nocs_map(_net("fp32"), feat).cpu().numpy()
    torch.cuda.synchronize()
    assert got.shape == (V, HW, 3) and got.dtype == np.float32
    err = float(np.abs(got.reshape(-1, 3) - want).max())
    print(f"V*HW = {V * HW}: max |kernel - float64| {err:.3e} (float32 torch - float64: {fmt:.3e})")
    assert np.isfinite(got).all() and err <= KERNEL_ATOL, err


def test_kernel_nan_stays_in_its_pixel():
    feat = _features(3, 64, 0)[0]
    clean = nocs_map(_net("fp32"), feat).cpu().numpy()
    for pix, ch in ((0, 0), (77, 31), (191, 13)):
        f = feat.copy().reshape(-1, 32)
        f[pix, ch] = np.nan
        got = nocs_map(_net("fp32"), f.reshape(3, 64, 32)).cpu().numpy().reshape(-1, 3)
        assert np.isnan(got[pix]).all(), pix
        rest = np.delete(np.arange(192), pix)
        assert np.array_equal(got[rest].view(np.uint32), clean.reshape(-1, 3)[rest].view(np.uint32)), pix


def test_kernel_refuses_a_pixel_count_that_is_no_multiple_of_64():
    with pytest.raises(ValueError, match="multiple of 64"):
        nocs_map(_net("fp32"), np.zeros((1, 100, 32), dtype=np.float32))


# ------------------------------------------------------------------------------------------------------------------ 2. in the forward
def _check_at_choose(out, inp, views=(1, 2)):
    for v in views:
        m = out[f"view{v}_nocs_map"]
        B = m.shape[0]
        assert m.shape == (B, S, S, 3) and m.dtype == torch.float32
        ch = torch.from_numpy(inp[f"choose{v}"]).cuda().long()
        at = m.reshape(B, S * S, 3).gather(1, ch.unsqueeze(2).expand(B, ch.shape[1], 3))
        assert torch.equal(at, out[f"view{v}_nocs"]), (v, float((at - out[f"view{v}_nocs"]).abs().max()))


@pytest.fixture(scope="module")
def oracle_nocs_maps():
    """The oracle's `pspnet` features of the golden batch through `_mlp1d` at every pixel, built once: {view: [2, S, S, 3] float64}."""
    from oracle import adapose_ref
    inp = _inputs(2, 0)
    sd = adapose_ref.to_torch_sd(synth.adapose_state_dict(seed=0))
    out = {}
    with torch.no_grad():
        for v in (1, 2):
            emb = adapose_ref.pspnet(torch.from_numpy(inp[f"img{v}"]), sd).reshape(2, 32, S * S)
            x = adapose_ref._mlp1d(emb, sd, "instance_color", (0,))
            x = torch.tanh(adapose_ref._mlp1d(x, sd, "nocs_head", (0, 2, 4), last_act=False))      # [B, 3, S*S]
            out[v] = x.permute(0, 2, 1).reshape(2, S, S, 3).double().numpy()
    return out


# measured on an MI355X against the oracle maps (profiles/dense_nocs_ab.txt): max |a - b| / max |b| over a view's map; the gates are
# twice these, the convention of tests/test_gpu_dense_depth.py::MEASURED_16BIT
# (bf16 1.06e-2 / 1.12e-2, fp16 1.17e-3 / 1.19e-3 for views 1 / 2)
MEASURED_16BIT = {"bf16": 1.13e-2, "fp16": 1.2e-3}


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3", "bf16", "fp16"])
def test_forward_maps_on_the_golden_batch(oracle_nocs_maps, dtype):
    """B = 2, the golden batch.  The map at `choose` is the point NOCS bit for bit; with dense_nocs alone the ten outputs are the plain
    forward's, with dense_depth as well those of forward(dense_depth=True), bit for bit; the whole map against the oracle."""
    inp = _inputs(2, 0)
    net = _net(dtype)
    plain = {k: v.clone() for k, v in _call(net, inp).items()}
    alone = _call(net, inp, dense_nocs=True)
    assert sorted(alone) == sorted(OUT_KEYS + ["view1_nocs_map", "view2_nocs_map"])
    for k in OUT_KEYS:
        assert torch.equal(alone[k], plain[k]), k
    _check_at_choose(alone, inp)
    dense = {k: v.clone() for k, v in _call(net, inp, dense_depth=True).items()}
    both = _call(net, inp, dense_depth=True, dense_nocs=True)
    assert sorted(both) == sorted(list(dense) + ["view1_nocs_map", "view2_nocs_map"])
    for k in dense:
        assert torch.equal(both[k], dense[k]), k
    _check_at_choose(both, inp)
    for v in (1, 2):
        assert torch.equal(both[f"view{v}_nocs_map"], alone[f"view{v}_nocs_map"]), v      # the PSPNet does not depend on the tail
        a, b = alone[f"view{v}_nocs_map"].cpu().numpy().astype(np.float64), oracle_nocs_maps[v]
        err = float(np.abs(a - b).max() / np.abs(b).max())
        print(f"{dtype} view{v}_nocs_map vs oracle: {err:.3e}")
        assert np.isfinite(a).all()
        if dtype in ("fp32", "bf16x3"):
            assert err < RTOL_FP32, (v, err)
        else:
            assert err < 2 * MEASURED_16BIT[dtype], (v, err)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_batch_one_and_view1_only(dtype):
    inp = _inputs(1, 5)
    _check_at_choose(_call(_net(dtype), inp, dense_nocs=True), inp)
    net = _net(dtype, options={"view2_heads": 0})
    inp = _inputs(2, 0)
    for kw in (dict(dense_nocs=True), dict(dense_nocs=True, dense_depth=True)):
        out = _call(net, inp, **kw)
        assert "view2_nocs_map" not in out and out["view1_nocs_map"].shape == (2, S, S, 3)
        _check_at_choose(out, inp, views=(1,))
        assert torch.equal(out["view1_nocs_map"], _call(_net(dtype), inp, dense_nocs=True)["view1_nocs_map"])


def test_per_sample_batchnorm_and_dropout():
    """norm_mode = 1 and Dropout2d on: the map still equals the point NOCS at `choose`."""
    inp = _inputs(2, 0)
    _check_at_choose(_call(_net("bf16x3", norm_mode=1), inp, dense_nocs=True), inp)
    net = AdaPoseNet(_sd(), dtype="bf16")
    net.set_dropout(0.3, seed=11)
    out = _call(net, inp, dense_nocs=True)
    _check_at_choose(out, inp)
    assert not torch.equal(out["view1_nocs_map"], _call(_net("bf16"), inp, dense_nocs=True)["view1_nocs_map"])      # the masks did act


# ------------------------------------------------------------------------------------------------------------------ 3. cloud_gather
@pytest.mark.parametrize("cap", [0, 7, 300])
@pytest.mark.parametrize("C_", [1, 3, 4])
def test_cloud_gather_against_numpy_indexing(cap, C_):
    S2, n = 100, 3
    g = np.random.default_rng(cap * 10 + C_)
    m1, m2 = g.normal(size=(n, S2, C_)).astype(np.float32), g.normal(size=(n, S2, C_)).astype(np.float32)
    index = g.integers(0, 2 * S2, (n, cap)).astype(np.int32)
    if cap >= 7:
        index[:, 0], index[:, 1], index[:, 2], index[:, 3] = 0, S2 - 1, S2, 2 * S2 - 1
        index[:, 4], index[:, 5], index[:, 6] = -1, 2 * S2, 2 ** 31 - 1

    def want(two):
        out = np.full((n, cap, C_), np.nan, dtype=np.float32)
        for i in range(n):
            for r in range(cap):
                ix = int(index[i, r])
                if 0 <= ix < S2:
                    out[i, r] = m1[i, ix]
                elif S2 <= ix < 2 * S2 and two:
                    out[i, r] = m2[i, ix - S2]
        return out
    for two in (True, False):
        got = cloud_gather(m1, m2 if two else None, index).cpu().numpy()
        ref = want(two)
        assert got.shape == ref.shape and got.dtype == np.float32
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        assert np.array_equal(got[~np.isnan(ref)].view(np.uint32), ref[~np.isnan(ref)].view(np.uint32))
    if cap:
        assert np.array_equal(cloud_gather(m1.reshape(n, 10, 10, C_), m2.reshape(n, 10, 10, C_), index).cpu().numpy(), want(True), equal_nan=True)
