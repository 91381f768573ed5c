"""The fixtures of tests/pnp_cases.py, from oracle/pnp_ref.py alone (no GPU): every case takes the branch it is named for, and the
cases that tests/test_gpu_pnp_tail.py compares to rounding are (a) off the VVS stop rule and (b) conditioned well enough for the
bounds it uses.  Both are conditions on the INPUTS: a case that misses one is replaced by another seed, never given a wider bound.
Run with -s to see the measured figures."""
import numpy as np
import pytest

import pnp_cases as pc
from oracle import pnp_ref

NAMES = [c[0] for c in pc.CASES]
TAGS = {c[0]: c[5] for c in pc.CASES}
OK_NAMES = [n for n in NAMES if "ok" in TAGS[n]]
# the batch-position test of tests/test_gpu_pnp_tail.py runs one case at other pose indices too
POSITIONS = [(n, None) for n in OK_NAMES] + [(pc.MOVED_CASE, b) for b in pc.MOVED_TO if b != pc.pose_of(pc.MOVED_CASE)]
# the GPU test's bounds on R, t and the box (those of tests/test_pnp.py); a case may use up a tenth of each by its conditioning
BOUNDS = np.array([5e-6, 5e-6, 1e-5])


def _is_default(bbox):
    return np.array_equal(bbox, pnp_ref.DEFAULT_BBOX)


def test_every_loop_bound_has_a_case_and_every_branch_a_name():
    g = pc.groups()
    assert set(g) == {8, 37, 200, 256, 257, 1000, 1024} and all(len(v) >= 1 for v in g.values())
    assert all(any("ok" in TAGS[n] for n in v) for v in g.values())          # every P runs the whole tail at least once
    have = {t for tags in TAGS.values() for t in tags}
    assert have >= {"ok", "examined_1", "examined_mid", "examined_100", "ransac_fails", "failed_hyp", "pairs_odd", "pairs_even",
                    "one_pair", "one_match", "no_match", "ties", "nan_nocs1", "nan_nocs2", "nan_pts1", "nan_pts2", "singular_E1"}


@pytest.mark.parametrize("name", [n for n in NAMES if "singular_E1" not in TAGS[n]])
def test_case_takes_the_branch_it_is_named_for(name):
    bbox, info = pc.oracle(name)
    c, tags = pc.inputs(name), TAGS[name]
    print(f"\n{name}: P {c['P']} pose {pc.pose_of(name)} matches {info['n_matches']} pairs {info['n_pairs_kept']} scale {info['scale']:.6g} "
          f"ransac_ok {info.get('ransac_ok')} examined {info.get('n_examined')} failed {info.get('n_failed_hyp')} inliers {info.get('n_inliers')}")
    if "ok" in tags:
        assert np.isfinite(info["scale"]) and info["ransac_ok"] and np.isfinite(bbox).all() and not _is_default(bbox)
        assert 1 <= len(info["vvs_trace"]) <= 20
    if "examined_1" in tags:
        assert info["n_examined"] == 1
    if "examined_mid" in tags:
        assert 1 < info["n_examined"] < 100
    if "examined_100" in tags:
        assert info["n_examined"] == 100 and info["ransac_ok"]
    if "ransac_fails" in tags:
        assert np.isfinite(info["scale"]) and info["ransac_ok"] is False and info["n_examined"] == 100 and _is_default(bbox)
    if "failed_hyp" in tags:
        assert info["n_failed_hyp"] >= 1 and info["ransac_ok"]                # the scan steps over it and still ends with a model
    if "pairs_odd" in tags:
        assert info["n_pairs_kept"] % 2 == 1
    if "pairs_even" in tags:
        assert info["n_pairs_kept"] % 2 == 0 and info["n_pairs_kept"] > 0
    if "one_pair" in tags:
        assert info["n_matches"] == 2 and info["n_pairs_kept"] == 1 and np.isfinite(info["scale"])
    if "one_match" in tags:
        assert info["n_matches"] == 1 and info["n_pairs_kept"] == 0 and np.isnan(info["scale"]) and _is_default(bbox)
    if "no_match" in tags:
        assert info["n_matches"] == 0 and np.isnan(info["scale"]) and _is_default(bbox)


def test_ties_are_the_nearest_neighbours_and_the_first_wins():
    (name,) = [n for n in NAMES if "ties" in TAGS[n]]
    c = pc.inputs(name)
    tie = c["ties"]
    dis = np.linalg.norm(c["nocs1"][:, None, :] - c["nocs2"][None, :, :], axis=-1)
    lo2, hi2 = tie["dup2"]
    assert lo2 < hi2 and np.array_equal(c["nocs2"][lo2], c["nocs2"][hi2])
    p = tie["left_of_dup2"]
    assert dis[p, lo2] == dis[p, hi2] == dis[p].min() and np.argmin(dis[p]) == lo2
    lo1, hi1 = tie["dup1"]
    assert lo1 < hi1 and np.array_equal(c["nocs1"][lo1], c["nocs1"][hi1]) and {lo1, hi1}.isdisjoint({p})
    q = tie["right_of_dup1"]
    assert dis[lo1, q] == dis[hi1, q] == dis[:, q].min() and np.argmin(dis[:, q]) == lo1
    # what a LAST-wins argmin would have matched differs: the tie decides the match list
    ml, mr = pnp_ref.nocs_matches(c["pts1"], c["nocs1"], c["pts2"], c["nocs2"], c["E1"], c["E2"], c["K"])
    pairs = set(zip(ml.tolist(), mr.tolist()))
    assert (p, lo2) in pairs and (p, hi2) not in pairs and (lo1, q) in pairs and (hi1, q) not in pairs


@pytest.mark.parametrize("name", pc.NAN_CASES)
def test_nan_cases_follow_numpy_argmin(name):
    """np.argmin returns the first NaN, so one NaN in either NOCS cloud ends every mutual match (lib/utils.py:128-137); a NaN pixel
    only drops its own match at the epipolar gate, and one of view 1 then reaches the refined pose through the VVS residual."""
    bbox, info = pc.oracle(name)
    c = pc.inputs(name)
    (arr,) = [t[4:] for t in TAGS[name] if t.startswith("nan_")]
    assert np.isnan(c[arr]).sum() == 1 and all(np.isfinite(c[k]).all() for k in ("nocs1", "nocs2", "pts1", "pts2") if k != arr)
    cl = pc.clean(name)
    _, before = pnp_ref.pnp_bbox_world(cl["nocs1"], cl["pts1"], cl["nocs2"], cl["pts2"], cl["K"], cl["E1"], cl["E2"], seed=pc.SEED,
                                       pose=pc.pose_of(name))
    print(f"\n{name}: matches {before['n_matches']} -> {info['n_matches']}, default box {_is_default(bbox)}")
    assert before["n_matches"] > 20
    if arr in ("nocs1", "nocs2"):
        assert info["n_matches"] == 0 and _is_default(bbox)
    else:
        assert info["n_matches"] == before["n_matches"] - 1
        if arr == "pts1":
            assert info["ransac_ok"] and not np.isfinite(info["R"]).any() and _is_default(bbox)
        else:
            assert info["ransac_ok"] and np.isfinite(bbox).all() and not _is_default(bbox)


def test_moved_case_shows_its_batch_position():
    examined = [pc.oracle(pc.MOVED_CASE, b)[1]["n_examined"] for b in pc.MOVED_TO]
    print(f"\n{pc.MOVED_CASE} at poses {pc.MOVED_TO}: examined {examined}")
    assert len(set(examined)) > 1 and all(1 < e < 100 for e in examined) and max(pc.MOVED_TO) < pc.MOVED_BATCH


SCANNED = [n for n in NAMES if {"ok", "ransac_fails", "nan_pts1", "nan_pts2"} & set(TAGS[n])]      # RANSAC runs in these


@pytest.mark.parametrize("name,pose", [(n, None) for n in SCANNED] + POSITIONS[len(OK_NAMES):])
def test_scan_does_not_depend_on_the_null_space_basis(name, pose):
    """(c) Five points give EPnP a 10 x 12 system, whose null space is two-dimensional: its basis is the eigen-solver's accident
    (LAPACK here, cyclic Jacobi in the kernel), the beta approximations start from that basis, and on some subsets they end in
    another pose.  One inlier more or less in one hypothesis moves the budget of the scan, so a case is compared scan by scan only if
    success, hypotheses examined and the kept inlier set are the same under six other bases."""
    runs = pc.scan_under_turned_bases(name, pose)
    ok0, ex0, m0 = runs[0]
    print(f"\n{name} pose {pc.pose_of(name) if pose is None else pose}: examined {[r[1] for r in runs]} inliers {[None if r[2] is None else int(r[2].sum()) for r in runs]}")
    for ok, ex, m in runs[1:]:
        assert ok == ok0 and ex == ex0
        assert (m is None and m0 is None) or np.array_equal(m, m0)


def test_singular_extrinsic_case_is_what_it_says():
    (name,) = [n for n in NAMES if "singular_E1" in TAGS[n]]
    c = pc.inputs(name)
    assert not c["E1"].any() and np.isfinite(np.linalg.inv(c["E2"])).all()


@pytest.mark.parametrize("name,pose", POSITIONS)
def test_successful_case_is_off_the_stop_rule_and_well_conditioned(name, pose):
    """(a) no |err - prev| of the VVS trace within 10 % of the 1e-6 rule: the rule is a discontinuous decision, and a case on it would
    compare iteration counts, not arithmetic.  (b) a relative 1e-10 on the pose entering VVS (what two correct small dense solvers may
    differ by) moves the result by at most a tenth of the GPU test's bounds.  And at most 2 points of the kept hypothesis lie
    within 1e-6 px^2 of the inlier threshold: the GPU test's allowance of 2 on the inlier count cannot hide more than those."""
    bbox, info = pc.oracle(name, pose)
    assert info["ransac_ok"] and np.isfinite(info["R"]).all()
    trace = np.array(info["vvs_trace"])
    near = pc.near_threshold(info)
    cond = pc.conditioning(name, pose)
    print(f"\n{name} pose {pc.pose_of(name) if pose is None else pose}: VVS trace {' '.join('%.3g' % x for x in trace)}; conditioning "
          f"R {cond[0]:.2g} t {cond[1]:.2g} box {cond[2]:.2g}; points within 1e-6 px^2 of the threshold {near}")
    assert not ((trace >= 0.9e-6) & (trace <= 1.1e-6)).any(), trace
    assert (cond <= BOUNDS / 10).all(), cond
    assert near <= 2
