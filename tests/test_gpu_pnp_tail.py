"""-m gpu: csrc/pnp.hip (`postprocess_pnp`, one workgroup per pose) against oracle/pnp_ref.py under the shared hash stream, on the
named cases of tests/pnp_cases.py.  tests/test_pnp_cases_host.py proves on the CPU that each case takes the branch it is named for
and that the compared cases are off the VVS stop rule and well conditioned; this file only compares."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pnp_cases as pc  # noqa: E402
from oracle.pnp_ref import DEFAULT_BBOX  # noqa: E402
from rgbmanip_amd import _lib  # noqa: E402
from rgbmanip_amd.adapose import postprocess_pnp  # noqa: E402

TAGS = {c[0]: c[5] for c in pc.CASES}
IDENTITY_SRT = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], dtype=np.float64)


def _stack(cases):
    st = lambda k, dt: torch.from_numpy(np.stack([c[k] for c in cases]).astype(dt)).cuda()  # noqa: E731
    return (st("nocs1", np.float32), st("pts1", np.float32), st("nocs2", np.float32), st("pts2", np.float32),
            st("K", np.float64), st("E1", np.float64), st("E2", np.float64))


def _run(cases):
    """(bbox, srt, info, valid) of one launch over `cases` (dicts of arrays), on the host."""
    out = postprocess_pnp(*_stack(cases), seed=pc.SEED)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _is_default(got, j):
    bbox, srt, info, valid = got
    return np.array_equal(bbox[j], DEFAULT_BBOX) and np.array_equal(srt[j, 1:], IDENTITY_SRT) and valid[j] == 0


def _against_restatement(got, j, name, pose):
    """Pose j of a launch against the restatement of case `name` run with `pose`: the integers exactly, the scale to 1e-12, the inlier
    count to 2 (the host test allows a case at most 2 points within 1e-6 px^2 of the threshold), R, t and box to the bounds of
    tests/test_pnp.py::test_device_pnp_branch_matches_the_restatement (5e-6, 5e-6, 1e-5)."""
    bbox, srt, info, valid = got
    want, wi = pc.oracle(name, pose)
    tag = (name, pose, info[j].tolist(), {k: wi.get(k) for k in ("n_matches", "ransac_ok", "n_examined", "n_inliers")})
    assert info[j, 0] == wi["n_matches"], tag
    ransac_ok = bool(wi.get("ransac_ok", False))                # RANSAC does not run without a scale
    assert info[j, 1] == int(ransac_ok), tag
    if "n_examined" in wi:
        assert info[j, 3] == wi["n_examined"], tag
    if np.isnan(wi["scale"]):
        assert np.isnan(srt[j, 0]), tag
    else:
        assert abs(srt[j, 0] - wi["scale"]) <= 1e-12 * abs(wi["scale"]), (tag, srt[j, 0], wi["scale"])
    if ransac_ok:
        assert abs(int(info[j, 2]) - wi["n_inliers"]) <= 2, tag
    else:
        assert info[j, 2] == 0, tag
    if np.array_equal(want, DEFAULT_BBOX):
        assert _is_default(got, j), (tag, bbox[j], srt[j], valid[j])
        return
    assert valid[j] == 1, tag
    eR, et, eb = np.abs(srt[j, 1:10].reshape(3, 3) - wi["R"]).max(), np.abs(srt[j, 10:13] - wi["t"]).max(), np.abs(bbox[j] - want).max()
    print(f"\n{name} pose {pose}: |dR| {eR:.2e} |dt| {et:.2e} |dbox| {eb:.2e} inliers {info[j, 2]} / {wi['n_inliers']}")
    assert eR < 5e-6 and et < 5e-6 and eb < 1e-5, (tag, eR, et, eb)


@pytest.mark.parametrize("P", pc.PS)
def test_cases_against_the_restatement(P):
    """Every case of one P in one launch, a case's pose index being its place in the batch.  Measured by
    tests/test_pnp_cases_host.py on the compared cases: a relative 1e-10 on the pose entering VVS moves the result by at most
    1.3e-10 (R), 9.4e-11 (t) and 4.4e-11 (box), four orders below the bounds of 5e-6, 5e-6 and 1e-5; no case has a point within
    1e-6 px^2 of the 9 px^2 inlier threshold (largest count: 0), so the allowance of 2 on the inlier count hides nothing; no VVS
    step of a case changes the residual by 0.9e-6 .. 1.1e-6; and every scan is the same under six other bases of the five-point
    null space.  With the restatement's control axes signed like the kernel's (pnp_ref.jacobi_eigh) the device was within 2e-15
    (R, t) and 1e-8 (box: the pose goes through float32 there) on every case; with LAPACK's signs p37_outliers was 1.7e-5 off in R.
    The all-zero E1 case is compared with nothing: `emit_bbox_world` guarantees the default box, whatever came before."""
    names = pc.groups()[P]
    got = _run([pc.inputs(n) for n in names])
    assert all(g.shape[0] == len(names) for g in got)
    for j, name in enumerate(names):
        if "singular_E1" in TAGS[name]:
            assert np.array_equal(got[0][j], DEFAULT_BBOX) and got[3][j] == 0 and np.isfinite(got[0][j]).all(), (name, got[0][j], got[3][j])
            continue
        _against_restatement(got, j, name, j)


def test_nan_follows_numpy_argmin():
    """One NaN in nocs2 / nocs1 / pts1 / pts2 (tests/test_pnp_cases_host.py says what each does in the reference's numpy): match count,
    validity and box as the restatement has them.  np.argmin takes the first NaN for the minimum, so a NaN in either NOCS cloud
    leaves no mutual match; a comparison `d < best` alone skips it and goes on matching the other points (with it the kernel
    returned 130 matches for both p200 NOCS cases, and for the NaN in nocs2 a finite box with valid = 1)."""
    for name in pc.NAN_CASES:
        P = pc.inputs(name)["P"]
        names = pc.groups()[P]
        j = names.index(name)
        got = _run([pc.inputs(n) for n in names])
        bbox, srt, info, valid = got
        want, wi = pc.oracle(name, j)
        dflt = np.array_equal(want, DEFAULT_BBOX)
        print(f"\n{name}: matches {info[j, 0]} (restatement {wi['n_matches']}), valid {valid[j]}, default box {np.array_equal(bbox[j], DEFAULT_BBOX)}")
        assert info[j, 0] == wi["n_matches"], (name, info[j], wi["n_matches"])
        assert valid[j] == (0 if dflt else 1), name
        if dflt:
            assert np.array_equal(bbox[j], DEFAULT_BBOX), (name, bbox[j])
        else:
            assert np.abs(bbox[j] - want).max() < 1e-5, name


def test_pose_depends_on_its_batch_index_only_through_the_hash():
    """One P = 37 case at b = 0, 5 and 47 of a batch of 48 whose other slots hold the other P = 37 cases: each of the three equals the
    restatement run with pose = b (whose scans differ: 38, 46 and 38 hypotheses), and the case alone in a batch is bit for bit
    slot 0."""
    others = [n for n in pc.groups()[37] if n != pc.MOVED_CASE]
    names = [pc.MOVED_CASE if b in pc.MOVED_TO else others[b % len(others)] for b in range(pc.MOVED_BATCH)]
    got = _run([pc.inputs(n) for n in names])
    for b in pc.MOVED_TO:
        _against_restatement(got, b, pc.MOVED_CASE, b)
    assert len({int(got[2][b, 3]) for b in pc.MOVED_TO}) > 1
    alone = _run([pc.inputs(pc.MOVED_CASE)])
    for a, g in zip(alone, got):
        assert _same_bits(a[0], g[0])


def test_poses_are_isolated_and_runs_repeat():
    """A NaN row in pose 1's nocs2 changes nothing in poses 0 and 2 (all four outputs bit for bit), and a second launch of either
    batch repeats the first bit for bit."""
    names = ["p37_outliers", "p37_ties", "p37_many_outliers"]
    cases = [pc.inputs(n) for n in names]
    poisoned = [dict(c) for c in cases]
    poisoned[1]["nocs2"] = np.array(cases[1]["nocs2"])
    poisoned[1]["nocs2"][11] = np.nan
    clean1, clean2 = _run(cases), _run(cases)
    bad1, bad2 = _run(poisoned), _run(poisoned)
    for a, b in zip(clean1, clean2):
        assert _same_bits(a, b)
    for a, b in zip(bad1, bad2):
        assert _same_bits(a, b)
    for c, p in zip(clean1, bad1):
        assert _same_bits(c[0], p[0]) and _same_bits(c[2], p[2])
    assert clean1[3].tolist() == [1, 1, 1] and bad1[3].tolist() == [1, 0, 1] and bad1[2][1, 0] == 0


def test_point_counts_outside_the_range_are_refused():
    """P = 7 and P = 1025 raise through the wrapper, and the C entry point returns its error before any launch: outputs it was handed
    keep their fill."""
    c = pc.inputs("p8_plain")
    for P in (7, 1025):
        big = {k: np.resize(c[k], (P,) + c[k].shape[1:]) for k in ("nocs1", "pts1", "nocs2", "pts2")}
        args = _stack([dict(c, **big)])
        with pytest.raises(_lib.RgbmError, match="8 <= P <= 1024"):
            postprocess_pnp(*args, seed=pc.SEED)
        bbox = torch.full((1, 8, 3), -7.0, dtype=torch.float64, device="cuda")
        srt = torch.full((1, 13), -7.0, dtype=torch.float64, device="cuda")
        info = torch.full((1, 4), -7, dtype=torch.int32, device="cuda")
        valid = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        rc = _lib.load().rgbm_adapose_postprocess_pnp(1, P, pc.SEED, *[_lib.ptr(a) for a in args], _lib.ptr(bbox), _lib.ptr(srt), _lib.ptr(info),
                                                     _lib.ptr(valid), _lib.stream_ptr(None))
        torch.cuda.synchronize()
        assert rc != 0
        assert (bbox == -7).all() and (srt == -7).all() and (info == -7).all() and (valid == -7).all()
