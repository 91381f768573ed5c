"""Named two-view cases for the PnP tail (tests/test_pnp_cases_host.py on the CPU, tests/test_gpu_pnp_tail.py on the device): each is
`synth.pnp_case(case, P)` plus a small edit and states the branch of csrc/pnp.hip it is there for.  A case's pose index is its
position among the cases of its P (`groups()`): the subset hash depends on it, so the branch a case takes holds at that position
only.  The host test proves from oracle/pnp_ref.py alone that every case takes the branch it is named for."""
import functools
import warnings

import numpy as np

from oracle import pnp_ref
from rgbmanip_amd import synth

SEED = 5           # the RANSAC seed in both test files
PS = (8, 37, 200, 256, 257, 1000, 1024)      # below one stride of 256, no multiple of it, the boundary on both sides, the LDS cap

# Branch tags (what tests/test_pnp_cases_host.py asserts for each):
#   ok            RANSAC succeeds, the pose is refined by VVS           examined_1    the scan stops after the first hypothesis
#   examined_mid  1 < n_examined < 100                                  examined_100  the budget never shrinks below 100, success
#   ransac_fails  finite scale, no hypothesis above 4 inliers           failed_hyp    a non-finite EPnP inside the scan
#   pairs_odd / pairs_even  arm of the scale median                     one_pair      two matches, one pair
#   one_match     one match, no pair: scale NaN, info[0] == 1           no_match      nothing in common (synth case 3)
#   ties          identical rows in nocs2 and in nocs1, first wins      nan_*         one NaN in that input
#   singular_E1   E1 all zeros: only the default box is defined
CASES = [
    # name, P, synth case, edit, argument of the edit, branch tags
    ("p8_plain", 8, 14, None, None, ("ok", "pairs_even")),
    ("p8_two_matches", 8, 0, "share", 2, ("one_pair", "pairs_odd")),
    ("p8_one_match", 8, 0, "share", 1, ("one_match",)),
    ("p8_no_match", 8, 3, None, None, ("no_match",)),
    ("p37_plain", 37, 15, None, None, ("ok",)),
    ("p37_outliers", 37, 1, None, None, ("ok",)),
    ("p37_ties", 37, 4, "ties", None, ("ok", "ties")),
    ("p37_nan_pts1_hyp", 37, 1, "nan", "pts1", ("nan_pts1", "failed_hyp")),
    ("p37_many_outliers", 37, 6, "outliers", 0.4, ("ok", "examined_mid")),
    ("p200_plain", 200, 0, None, None, ("ok",)),
    ("p200_ransac_fails", 200, 1, "outliers", 0.9, ("ransac_fails",)),
    ("p200_nan_nocs2", 200, 0, "nan", "nocs2", ("nan_nocs2",)),
    ("p200_nan_nocs1", 200, 0, "nan", "nocs1", ("nan_nocs1",)),
    ("p200_nan_pts1", 200, 0, "nan", "pts1", ("nan_pts1",)),
    ("p200_nan_pts2", 200, 0, "nan", "pts2", ("nan_pts2",)),
    ("p256_plain", 256, 0, None, None, ("ok", "pairs_odd")),
    ("p256_outliers", 256, 17, None, None, ("ok", "examined_mid")),
    ("p257_plain", 257, 0, None, None, ("ok",)),
    ("p257_outliers", 257, 2, None, None, ("ok", "examined_mid")),
    ("p1000_plain", 1000, 0, None, None, ("ok",)),
    ("p1000_outliers", 1000, 6, None, None, ("ok", "examined_mid")),
    ("p1024_first", 1024, 0, None, None, ("ok", "examined_1", "pairs_even")),
    ("p1024_mid", 1024, 2, None, None, ("ok", "examined_mid")),
    ("p1024_all_100", 1024, 1, "outliers", 0.5, ("ok", "examined_100")),
    ("p1024_ransac_fails", 1024, 1, "outliers", 0.9, ("ransac_fails",)),
    ("p1024_singular_E1", 1024, 0, "singular_E1", None, ("singular_E1",)),
]
NAN_CASES = [c[0] for c in CASES if c[3] == "nan"]
# the batch-position test: one case at three pose indices of a batch of 48.  With few outliers the first all-inlier subset ends the
# scan wherever it is drawn and the position would not show; with 40 % of them the scan examines 38 hypotheses at b = 0 and 47, 46 at 5
MOVED_CASE, MOVED_TO, MOVED_BATCH = "p37_many_outliers", (0, 5, 47), 48


def _matches(c):
    return pnp_ref.nocs_matches(c["pts1"], c["nocs1"], c["pts2"], c["nocs2"], c["E1"], c["E2"], c["K"])


def _edit(c, P, case, edit, arg):
    rng = np.random.default_rng(9100 + 16 * P + case)
    if edit == "share":
        # view 2 keeps its partner of the first `arg` matches; every other row moves out of reach, as in synth case 3
        ml, mr = _matches(c)
        assert len(ml) >= arg
        far = np.ones(P, dtype=bool)
        far[mr[:arg]] = False
        c["nocs2"][far] += np.float32(2.0)
    elif edit == "outliers":
        bad = rng.random(P) < arg
        c["pts1"][bad] = rng.uniform([100, 60], [540, 420], (int(bad.sum()), 2)).astype(np.float32)
    elif edit == "ties":
        # a second copy of a matched row of nocs2 at a LOWER index and of a matched row of nocs1 at a HIGHER one: the copy wins in
        # view 2, the original in view 1
        ml, mr = _matches(c)
        k2 = int(np.argmax(mr))                          # the match whose partner has the highest index in view 2
        free2 = [j for j in range(P) if j not in set(mr.tolist())]
        assert free2[0] < mr[k2]
        c["nocs2"][free2[0]] = c["nocs2"][mr[k2]]
        k1 = int(np.argmin(ml)) if int(np.argmin(ml)) != k2 else int(np.argsort(ml)[1])
        free1 = [i for i in range(P) if i not in set(ml.tolist())]
        assert free1[-1] > ml[k1]
        c["nocs1"][free1[-1]] = c["nocs1"][ml[k1]]
        c["ties"] = dict(left_of_dup2=int(ml[k2]), dup2=(free2[0], int(mr[k2])), right_of_dup1=int(mr[k1]), dup1=(int(ml[k1]), free1[-1]))
    elif edit == "nan":
        # the NaN sits on a matched point, so that the clean case says what it costs
        ml, mr = _matches(c)
        k = len(ml) // 2
        row = int(ml[k]) if arg in ("nocs1", "pts1") else int(mr[k])
        c[arg][row, 1] = np.nan
        c["nan_at"] = row
    elif edit == "singular_E1":
        c["E1"] = np.zeros((4, 4))
    else:
        assert edit is None, edit
    return c


@functools.lru_cache(maxsize=None)
def _built(name):
    (_, P, case, edit, arg, tags), = [c for c in CASES if c[0] == name]
    c = synth.pnp_case(case, P)
    c = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    c = _edit(c, P, case, edit, arg)
    c.update(name=name, P=P, tags=tags)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def inputs(name):
    """The case's arrays (read-only: they are shared by every test) with its name, P and branch tags."""
    return _built(name)


def clean(name):
    """`synth.pnp_case` of a case before its edit."""
    (_, P, case, _, _, _), = [c for c in CASES if c[0] == name]
    return synth.pnp_case(case, P)


def groups():
    """{P: [names in batch order]}: a case's pose index is its position in its list."""
    out = {P: [] for P in PS}
    for name, P, *_ in CASES:
        out[P].append(name)
    return out


def pose_of(name):
    (P,), = [[c[1]] for c in CASES if c[0] == name]
    return groups()[P].index(name)


@functools.lru_cache(maxsize=None)
def oracle(name, pose=None):
    """oracle.pnp_ref.pnp_bbox_world of a case at `pose` (default: its own position) -> (bbox, info), computed once and shared."""
    c = inputs(name)
    pose = pose_of(name) if pose is None else pose
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                       # np.median of the empty pair list of a single match
        bbox, info = pnp_ref.pnp_bbox_world(c["nocs1"], c["pts1"], c["nocs2"], c["pts2"], c["K"], c["E1"], c["E2"], seed=SEED, pose=pose)
    bbox.setflags(write=False)
    return bbox, info


def near_threshold(info, width=1e-6):
    """How many points of the kept hypothesis lie within `width` px^2 of the 9 px^2 inlier threshold."""
    return int((np.abs(info["kept_sq_err"] - pnp_ref.REPROJ_ERR ** 2) <= width).sum())


BASIS_ANGLES = (0.4, 0.9, 1.4, 1.9, 2.4, 2.9)      # a turn by pi only changes signs, which EPnP's betas absorb


def scan_under_turned_bases(name, pose=None):
    """What the RANSAC scan of a case gives when `epnp` gets another basis of the two-dimensional null space of its five-point
    systems (pnp_ref.NULL_BASIS_ANGLE): [(ok, n_examined, inlier mask)], the first entry being the unturned run.  LAPACK and the
    kernel's Jacobi return different bases there, so only a case whose entries are all equal can be compared scan by scan."""
    c = inputs(name)
    pose = pose_of(name) if pose is None else pose
    _, info = oracle(name, pose)
    out = [(bool(info["ransac_ok"]), info["n_examined"], info.get("inliers"))]
    try:
        for a in BASIS_ANGLES:
            pnp_ref.NULL_BASIS_ANGLE = a
            got = {}
            with np.errstate(all="ignore"):
                ok, _, _, mask = pnp_ref.solve_pnp_ransac(info["pw"], info["uv"], c["K"], SEED, pose, got)
            out.append((ok, got["n_examined"], mask))
    finally:
        pnp_ref.NULL_BASIS_ANGLE = 0.0
    return out


def conditioning(name, pose=None, draws=10, rel=1e-10):
    """Largest change of the refined (R, t, box) over `draws` seeded relative perturbations of size `rel` of the pose that enters
    refine_vvs: how far two correct solvers that start 1e-10 apart may end apart."""
    from oracle.align_ref import bbox_from_srt
    c = inputs(name)
    bbox, info = oracle(name, pose)
    rng = np.random.default_rng(77)
    worst = np.zeros(3)
    for _ in range(draws):
        R0 = info["R0"] * (1.0 + rel * rng.uniform(-1, 1, (3, 3)))
        t0 = info["t0"] * (1.0 + rel * rng.uniform(-1, 1, 3))
        R, t = pnp_ref.refine_vvs(info["pw"], info["uv"], c["K"], R0, t0)
        box = bbox_from_srt(c["nocs1"], info["scale"], R, t, c["E1"])
        worst = np.maximum(worst, [np.abs(R - info["R"]).max(), np.abs(t - info["t"]).max(), np.abs(box - bbox).max()])
    return worst
