"""GPU: the cross-view attention stack (rgbm_view_fusion) and depth_head (rgbm_depth_head) against their float64 twins.

Tolerance.  The kernels are fp32; so is the reference.  e = the reference's own float32-against-float64 error in the project's measure
max|a - b| / max|b|, taken on the CPU here: the reference ViewFusion's float32 outputs in tests/golden/view_fusion_small.npz against
the float64 twin at (B, P) = (3, 96) and (1, 32) (7.1e-7, 5.3e-7), and at (2, 1024), whose 0.5 MB of reference outputs are not stored,
the float32 restatement (tests/baseline_ref.py, bit-equal to the reference on the golden batch's fused rows) against the twin (9.95e-7).
e = 9.95e-7 .. 1.30e-6 (the (2, 1024) figure moves with the host BLAS's blocking, i.e. with the CPU the test runs on); the kernel
gets 8 e = 8.0e-6 .. 1.04e-5, the margin being for an accumulation order (online softmax over key tiles, MFMA K steps) that differs from
torch's.  Measured on the MI355X: 6.6e-7 at (1, 32), 9.1e-7 at (3, 96), 1.5e-6 at (2, 1024), 4.7e-6 with scores of -270 .. +234."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import baseline_ref as br  # noqa: E402

from rgbmanip_amd import _lib, adapose, synth  # noqa: E402

pytestmark = pytest.mark.gpu
SHAPES = [(1, 32), (3, 96), (2, 1024)]


@pytest.fixture(scope="module")
def sd():
    return synth.baseline_state_dict(seed=0)


@pytest.fixture(scope="module")
def net(sd):
    n = adapose.AdaPoseNet(sd, dtype="fp32", arch="baseline")
    yield n
    n.close()


@pytest.fixture(scope="module")
def cases(sd, golden_dir):
    """Per shape: inputs, the float64 twin's outputs, and the reference-side float32 error; E = their maximum."""
    small = np.load(os.path.join(golden_dir, "view_fusion_small.npz"))
    sd32 = br.to_sd(sd, torch.float32)
    out = {}
    for B, P in SHAPES:
        x1, x2 = synth.view_fusion_inputs(B, P, seed=0)
        y1, y2 = adapose.view_fusion_ref(sd, x1, x2)
        t = f"b{B}_p{P}_"
        if t + "y1" in small.files:
            r1, r2 = small[t + "y1"], small[t + "y2"]
        else:
            r1, r2 = (v.numpy() for v in br.view_fusion(torch.from_numpy(x1), torch.from_numpy(x2), sd32))
        out[(B, P)] = dict(x1=x1, x2=x2, y1=y1, y2=y2, e=max(br.rel_err(r1, y1), br.rel_err(r2, y2)))
    e = max(c["e"] for c in out.values())
    print("reference float32 vs float64 per shape:", {k: v["e"] for k, v in out.items()}, "-> e =", e, ", kernel bound 8 e =", 8 * e)
    assert 1e-7 < e < 3e-6, e            # float32 rounding of a conditioned fixture, not something else
    out["bound"] = 8 * e
    return out


def _run(net, x1, x2):
    y1, y2 = net.view_fusion(x1, x2)
    torch.cuda.synchronize()
    return y1.cpu().numpy(), y2.cpu().numpy()


@pytest.mark.parametrize("B,P", SHAPES)
def test_parity_and_repeatability(net, cases, B, P):
    c = cases[(B, P)]
    y1, y2 = _run(net, c["x1"], c["x2"])
    errs = br.rel_err(y1, c["y1"]), br.rel_err(y2, c["y2"])
    print(f"view_fusion ({B}, {P}) vs float64 twin:", errs, "bound", cases["bound"])
    assert np.isfinite(y1).all() and np.isfinite(y2).all()
    assert max(errs) <= cases["bound"], errs
    z1, z2 = _run(net, c["x1"], c["x2"])
    assert np.array_equal(y1, z1) and np.array_equal(y2, z2)


def test_a_pose_does_not_depend_on_the_batch(net, cases):
    c = cases[(3, 96)]
    y1, y2 = _run(net, c["x1"], c["x2"])
    for b in range(3):
        a1, a2 = _run(net, c["x1"][b:b + 1], c["x2"][b:b + 1])
        assert np.array_equal(a1[0], y1[b]) and np.array_equal(a2[0], y2[b]), b


def test_direction_and_ordering(net, cases, sd):
    c = cases[(3, 96)]
    # view 2 constant across points: every key of fusion1 is the same, so y1 - x1 is one vector per pose (and view 2 stays constant
    # through the blocks, because its queries are all equal)
    x2c = np.repeat(c["x2"][:, :1], 96, axis=1)
    y1, y2 = _run(net, c["x1"], x2c)
    t1, _ = adapose.view_fusion_ref(sd, c["x1"], x2c)
    assert br.rel_err(y1, t1) <= cases["bound"]
    d = y1.astype(np.float64) - c["x1"]
    spread = np.abs(d - d[:, :1]).max() / np.abs(y1).max()
    print("spread of y1 - x1 over the points:", spread)
    assert spread <= cases["bound"], spread
    assert np.abs(d).max() > 1e-2                               # and it is not zero
    # fusion1 != fusion2: swapping the inputs does not swap the outputs
    a1, a2 = _run(net, c["x1"], c["x2"])
    s1, s2 = _run(net, c["x2"], c["x1"])
    assert br.rel_err(s1, a2) > 1e-2 and br.rel_err(s2, a1) > 1e-2
    t1, t2 = adapose.view_fusion_ref(sd, c["x2"], c["x1"])
    assert br.rel_err(s1, t1) <= cases["bound"] and br.rel_err(s2, t2) <= cases["bound"]


def test_scores_of_plus_minus_200(net, cases, sd):
    """The softmax subtracts the running maximum: exp(200) is past float32.  Input: the (1, 32) fixture rows times 2.5, at which the
    twin's scores span -270 .. +234.  The case is chosen by the reference's own arithmetic: there torch's float32 stack is 3.2e-6 from
    float64, inside 8 e, so a float32 kernel can be held to the bound; at (3, 96) x 2.5 torch's float32 itself is 4.9e-5 from float64
    (near-tied scores of magnitude 200 carry 2e-5 in their probabilities, four blocks deep), which no float32 kernel can undercut."""
    c = cases[(1, 32)]
    x1, x2 = c["x1"] * np.float32(2.5), c["x2"] * np.float32(2.5)
    stats = {}
    t1, t2 = adapose.view_fusion_ref(sd, x1, x2, stats=stats)
    print("twin scores:", min(stats["score_min"]), max(stats["score_max"]))
    assert max(stats["score_max"]) >= 200 and min(stats["score_min"]) <= -200
    y1, y2 = _run(net, x1, x2)
    assert np.isfinite(y1).all() and np.isfinite(y2).all()
    errs = br.rel_err(y1, t1), br.rel_err(y2, t2)
    print("scores of +-200 vs twin:", errs, "bound", cases["bound"])
    assert max(errs) <= cases["bound"], errs


def test_poses_are_isolated(net, cases):
    c = cases[(3, 96)]
    y1, y2 = _run(net, c["x1"], c["x2"])
    x2 = c["x2"].copy()
    x2[1, 17, :] = np.nan
    n1, n2 = _run(net, c["x1"], x2)
    for b in (0, 2):
        assert np.array_equal(n1[b], y1[b]) and np.array_equal(n2[b], y2[b]), b
    assert np.isnan(n1[1]).any() and np.isnan(n2[1]).any()


def test_scratch_is_linear_in_the_rows():
    """A condition, not a measurement: the stack's state is 10 [B][P][32] buffers; one materialised score tensor per pose and direction
    would already be 8 times the cap."""
    import ctypes as C
    lib = _lib.load()
    n = C.c_size_t()
    _lib.check(lib.rgbm_view_fusion_scratch_bytes(256, 1024, C.byref(n)), "rgbm_view_fusion_scratch_bytes")
    assert 0 < n.value <= 16 * 256 * 1024 * 32 * 4


def test_bad_shapes_are_refused(net):
    with pytest.raises(ValueError):
        net.view_fusion(np.zeros((1, 48, 32), np.float32), np.zeros((1, 48, 32), np.float32))
    with pytest.raises(ValueError):
        net.view_fusion(np.zeros((1, 4128, 32), np.float32), np.zeros((1, 4128, 32), np.float32))


@pytest.mark.parametrize("n", [64, 2048])
def test_depth_head(net, sd, n):
    """depth_head against float64, rows of four magnitudes so that the final ReLU zeroes some (13 of 64, 479 of 2048).  Bound as above:
    8 times the float32 restatement's own error against float64 on these rows (3.6e-7 -> 2.9e-6)."""
    g = np.random.default_rng(7 + n)
    x = (g.normal(size=(n, 32)) * np.array([0.5, 2, 8, 16])[np.arange(n) % 4, None]).astype(np.float32)
    d64 = br.depth_head(torch.from_numpy(x).double(), br.to_sd(sd, torch.float64)).numpy()
    d32 = br.depth_head(torch.from_numpy(x), br.to_sd(sd, torch.float32)).numpy()
    assert (d64 == 0).sum() >= 8 and (d64 > 0).sum() >= 8
    e = br.rel_err(d32, d64)
    got = adapose.depth_head(net, x).cpu().numpy()
    err = br.rel_err(got, d64)
    print(f"depth_head {n} rows: kernel {err}, float32 restatement {e}")
    assert got.shape == (n,) and err <= 8 * e, (err, e)
    assert (got[d64 == 0] <= 8 * e * d64.max()).all() and (got >= 0).all()
