"""-m gpu: the content-keyed feature cache ("content keys") — `rgbm_crop_fingerprint` against its numpy
restatement, and `AdaPoseEstimator_v5(cfg hip_feature_cache: "content")` at the `estimate_device` and numpy `estimate` boundaries
against the uncached estimator: the PSPNet runs on exactly the crops not met before, the boxes agree to the tensor-normalised 1e-4
of tests/test_gpu_feature_cache.py::test_controller_rollout_with_and_without_the_cache.

Frames are seeded 480 x 640 noise over a smooth pattern with elliptical masks under look-at cameras (the geometry of the benchmark's
headline workload); weights are the seeded synthetic ones.  One network per storage type serves every estimator of this file."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rgbmanip_amd import _lib, synth  # noqa: E402
from rgbmanip_amd.feature_keys import crop_keys  # noqa: E402

GATE = 1e-4
_NETS, _REF = {}, {}


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-12))


# ------------------------------------------------------------------------------------------------------------------ the kernel
def _fingerprint(words_dev, V, n_words, out):
    _lib.check(_lib.load().rgbm_crop_fingerprint(C.c_void_p(words_dev.data_ptr()), V, n_words, C.c_void_p(out.data_ptr()), _lib.stream_ptr()),
               "rgbm_crop_fingerprint")


@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("n_words", [1, 63, 64, 65, 4099, 150528])
def test_kernel_matches_the_numpy_restatement(n_words, V):
    """All 2V key words equal.  Rows are dense, so with n_words = 4099 rows 1 and 2 start 12 and 8 bytes past a 16-byte boundary;
    the last row repeats row 0 (at another alignment where n_words % 4 != 0): identical rows, identical keys."""
    rng = np.random.default_rng(n_words * 7 + V)
    w = rng.integers(0, 2 ** 32, size=(V, n_words), dtype=np.uint32)
    special = np.array([0x7FC00000, 0x7F800000, 0xFF800000, 0x7F800001, 0xFFFFFFFF, 0x80000000, 0x00000000], dtype=np.uint32)
    for v in range(V):                                          # NaN (quiet, signalling, all ones), +-Inf, -0.0, +0.0 patterns
        at = rng.choice(n_words, size=min(n_words, len(special)), replace=False)
        w[v, at] = np.roll(special, -v)[: len(at)]              # another pattern first in every row: rows differ even at n_words = 1
    if V > 1:
        w[V - 1] = w[0]
    want = crop_keys(w)
    dev = torch.from_numpy(w.view(np.int32)).cuda()
    guard = 0x5A5A5A5A5A5A5A5A
    out = torch.full((V + 1, 2), guard, dtype=torch.int64, device="cuda")      # one row more than is written
    _fingerprint(dev, V, n_words, out)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint64)
    assert got[:V].tolist() == want.tolist()
    assert got[V].tolist() == [guard, guard]
    if V > 1:
        assert got[V - 1].tolist() == got[0].tolist() and got[1].tolist() != got[0].tolist()
    again = torch.full((V + 1, 2), 1, dtype=torch.int64, device="cuda")       # not zero on entry: the call clears what it sums into
    _fingerprint(dev, V, n_words, again)
    torch.cuda.synchronize()
    assert torch.equal(again[:V], out[:V])


# ------------------------------------------------------------------------------------------------------------------ the estimator
def _net(dtype):
    if dtype not in _NETS:
        from rgbmanip_amd.adapose import AdaPoseNet
        _NETS[dtype] = AdaPoseNet(synth.adapose_state_dict(seed=0, prefix="module."), dtype=dtype, options={"view2_heads": 0})
    return _NETS[dtype]


def _est(dtype, cache=False, **kw):
    from rgbmanip_amd.config import ADAPOSE_CFGS
    from rgbmanip_amd.estimator import AdaPoseEstimator_v5
    cfg = dict(ADAPOSE_CFGS["adapose_cabinet"], load=False, hip_prepare="device", hip_prepare_seed=1, **kw)
    if cache:
        cfg["hip_feature_cache"] = "content"
    return AdaPoseEstimator_v5(None, cfg, None, net=_net(dtype), dtype=dtype)


def _frames(n, seed):
    """n seeded frames with a mask each and the camera that looks at the object: dict(rgb [n,480,640,3] f32, mask [n,480,640] u8, E)."""
    g = np.random.default_rng(9000 + seed)
    yy, xx = np.meshgrid(np.arange(480, dtype=np.float32), np.arange(640, dtype=np.float32), indexing="ij")
    rgb = np.empty((n, 480, 640, 3), dtype=np.float32)
    mask = np.empty((n, 480, 640), dtype=np.uint8)
    E = np.empty((n, 4, 4))
    for i in range(n):
        ph = g.uniform(0, 6.2832, size=3)
        smooth = 0.5 + 0.125 * (np.cos(0.02 * xx + ph[0]) + np.cos(0.03 * yy + ph[1]) + np.cos(0.011 * (xx + yy) + ph[2]))
        rgb[i] = np.clip(0.5 * g.random((480, 640, 3), dtype=np.float32) + 0.5 * smooth[..., None], 0.0, 1.0)
        cy, cx, ry, rx = 240 + g.uniform(-50, 50), 320 + g.uniform(-80, 80), g.uniform(40, 120), g.uniform(40, 150)
        mask[i] = (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2) <= 1
        target = g.uniform(-0.05, 0.05, size=3) + np.array([0.0, 0.0, 0.5])
        d0 = g.normal(size=3)
        d0[2] = abs(d0[2]) * 0.3
        d0 /= np.linalg.norm(d0)
        E[i] = synth._lookat_extrinsic(target + d0 * g.uniform(0.55, 0.9), target)
    return {"rgb": rgb, "mask": mask, "E": E}


def _K(n):
    fx = 240.0 / np.tan(0.5)
    return np.tile(np.array([[fx, 0, 320.0], [0, fx, 240.0], [0, 0, 1.0]]), (n, 1, 1))


def _pick(f, idx):
    return {k: v[idx] for k, v in f.items()}


def _call_device(est, f1, f2):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    n = len(f1["rgb"])
    before = est.feature_views_computed
    box = est.estimate_device(_K(n), dev(f1["rgb"]), dev(f1["mask"]), f1["E"], dev(f2["rgb"]), dev(f2["mask"]), f2["E"])
    torch.cuda.synchronize()
    return box.cpu().numpy(), est.feature_views_computed - before


def _check_boxes(got, want, what):
    from rgbmanip_amd.estimator import DEFAULT_BBOX
    dflt = lambda b: np.all(b == DEFAULT_BBOX[None], axis=(1, 2))      # noqa: E731
    err = _rel(got, want)
    print(f"{what}: cached vs uncached {err:.3e}, default entries {dflt(want).tolist()}")
    assert np.isfinite(got).all()
    assert np.array_equal(dflt(got), dflt(want)), what
    assert not dflt(want).all(), what                                   # real boxes are compared
    assert err < GATE, (what, err)


def _sets(n):
    """Three frame sets of n frames, generated once per n."""
    key = ("frames", n)
    if key not in _REF:
        _REF[key] = [_frames(n, seed=10 * n + k) for k in range(3)]
    return _REF[key]


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
def test_estimate_device_computes_only_the_new_view(dtype):
    """n = 3.  Call A on (f0, f1): 2n crops.  Call B on (f2, f1): view 2 repeats, n crops.  Boxes of both against an uncached estimator."""
    n = 3
    f0, f1, f2 = _sets(n)
    off, on = _est(dtype), _est(dtype, cache=True)
    for name, (a, b), count in (("A", (f0, f1), 2 * n), ("B", (f2, f1), n)):
        want, c_off = _call_device(off, a, b)
        got, c_on = _call_device(on, a, b)
        assert c_off == 2 * n and c_on == count, (name, c_off, c_on)
        _check_boxes(got, want, f"{dtype} call {name}")
    assert on.feature_cache_bypassed == 0 and on._content.table.records == 2 * n


def test_numpy_estimate_through_the_chunk_pipeline():
    """float64 host frames, n = 5, hip_upload_chunk 2: three chunks, the last of one pose.  The second call shares view 2 with the first
    and computes n crops; boxes against the uncached estimator with the same chunking."""
    n = 5
    f0, f1, f2 = _sets(n)
    off, on = _est("bf16x3", hip_upload_chunk=2), _est("bf16x3", cache=True, hip_upload_chunk=2)
    K = _K(n)
    for name, (a, b), count in (("A", (f0, f1), 2 * n), ("B", (f2, f1), n)):
        args = (K, a["rgb"].astype(np.float64), a["mask"].astype(bool), a["E"], b["rgb"].astype(np.float64), b["mask"].astype(bool), b["E"])
        want = off.estimate(*args)
        before = on.feature_views_computed
        got = on.estimate(*args)
        assert isinstance(got, np.ndarray) and got.shape == (n, 8, 3)
        assert on.feature_views_computed - before == count, (name, on.feature_views_computed - before)
        _check_boxes(got, want, f"estimate() call {name}")
    assert on.feature_cache_bypassed == 0 and on._content.table.records == 2 * n      # sized by the call, not by its chunks


def test_duplicate_crops_are_computed_once():
    """Pose 0 has rgb1 is rgb2 with one mask; poses 1 and 2 share their view-1 frame and mask: 4 distinct crops in 6 views."""
    f0, f1, _ = _sets(3)
    v1 = _pick(f0, [0, 1, 1])
    v2 = {"rgb": np.stack((v1["rgb"][0], f1["rgb"][1], f1["rgb"][2])), "mask": np.stack((v1["mask"][0], f1["mask"][1], f1["mask"][2])),
          "E": np.stack((f1["E"][0], f1["E"][1], f1["E"][2]))}
    off, on = _est("bf16x3"), _est("bf16x3", cache=True)
    want, _ = _call_device(off, v1, v2)
    got, count = _call_device(on, v1, v2)
    assert count == 4
    _check_boxes(got, want, "duplicates")
    got, count = _call_device(on, v1, v2)
    assert count == 0                                                   # and all of them are hits the second time
    _check_boxes(got, want, "duplicates, second call")


def test_eviction_and_overflow():
    """hip_feature_cache_records 6 with n = 2 and four calls on new frames each (four records per call): every call computes 2n crops
    inside the gate, the latest call's records are still there, the first call's are not.  Three records cannot hold one call."""
    n = 2
    calls = [(_frames(n, seed=100 + 2 * i), _frames(n, seed=101 + 2 * i)) for i in range(4)]
    off, on = _est("bf16x3"), _est("bf16x3", cache=True, hip_feature_cache_records=6)
    wants = []
    for i, (a, b) in enumerate(calls):
        want, _ = _call_device(off, a, b)
        got, count = _call_device(on, a, b)
        wants.append(want)
        assert count == 2 * n, (i, count)
        _check_boxes(got, want, f"records 6, call {i}")
    assert on._content.table.records == 6 and on.feature_cache_bypassed == 0
    got, count = _call_device(on, *calls[3])
    assert count == 0                                                   # the latest call's four records are all there
    got, count = _call_device(on, *calls[0])
    assert count == 2 * n                                               # the first call's were evicted on the way: computed again
    _check_boxes(got, wants[0], "records 6, call 0 again")
    # three records cannot hold the four distinct crops of one call: the plain path, bit for bit, and counted
    small = _est("bf16x3", cache=True, hip_feature_cache_records=3)
    got, count = _call_device(small, *calls[0])
    assert small.feature_cache_bypassed == 1 and count == 2 * n
    assert np.array_equal(got, wants[0])
    assert len(small._content.table) == 0


def test_invalidate_features_forgets_the_keys():
    n = 3
    f0, f1, _ = _sets(n)
    on = _est("bf16x3", cache=True)
    assert _call_device(on, f0, f1)[1] == 2 * n
    assert _call_device(on, f0, f1)[1] == 0
    on.invalidate_features()
    box, count = _call_device(on, f0, f1)
    assert count == 2 * n
    want, _ = _call_device(_est("bf16x3"), f0, f1)
    _check_boxes(box, want, "after invalidate_features")
