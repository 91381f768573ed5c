"""Planted similarities for the cloud-fit tests (tests/test_cloud_fit_host.py on the CPU, tests/test_gpu_cloud_fit.py on the device):
the idea of tests/test_gpu_align.py::_case with world-frame targets, plus the oracle evaluation both test files compare against."""
import numpy as np

SEED = 23          # the fit's seed in both test files
CASES = [
    # name, rows m, cap, outlier share, mirrored, special
    ("m5", 5, 5, 0.0, False, None),
    ("m37", 37, 40, 0.2, False, None),
    ("m1024_clean", 1024, 1024, 0.0, False, None),
    ("m1024_o20", 1024, 1100, 0.2, False, None),
    ("m1024_o45", 1024, 1024, 0.45, False, None),
    ("m1024_none", 1024, 1024, 1.0, False, None),
    ("m1024_mirror", 1024, 1024, 0.05, True, None),
    ("m4099_o20", 4099, 4099, 0.2, False, None),
    ("m4099_o45", 4099, 4200, 0.45, False, None),
    ("m4", 4, 16, 0.0, False, None),
    ("nan_row", 200, 200, 0.1, False, "nan"),
    ("count_over_cap", 300, 300, 0.2, False, "over"),
]


def planted(k, m, cap, outliers, mirror, special=None, noise=0.002):
    """(nocs [cap,3] f32, cloud [cap,3] f32, count [2] i32): cloud = s R nocs + t (+ noise), a share of rows replaced by uniform
    object-space points, rows m .. cap - 1 NaN as cloud_pack leaves them."""
    rng = np.random.default_rng(4100 + k)
    nocs = rng.uniform(-0.45, 0.45, (m, 3))
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] *= -1
    s, t = rng.uniform(0.1, 0.4), rng.normal(0, 0.5, 3)
    cloud = s * nocs @ q.T + t + rng.normal(0, noise * s, (m, 3))
    bad = rng.random(m) < outliers
    nocs[bad] = rng.uniform(-0.5, 0.5, (int(bad.sum()), 3))
    if mirror:
        nocs[:, 0] = -nocs[:, 0]
    N = np.full((cap, 3), np.nan, dtype=np.float32)
    Cl = np.full((cap, 3), np.nan, dtype=np.float32)
    N[:m], Cl[:m] = nocs, cloud
    c1 = m // 3
    count = np.array([c1, m - c1], dtype=np.int32)
    if special == "nan":
        N[m // 2, 1] = np.nan
    if special == "over":
        count = np.array([m, 57], dtype=np.int32)      # the sum exceeds cap: the first cap rows are used
    return N, Cl, count


def oracle_fit(nocs, cloud, count, seed, pose):
    """oracle.align_ref.similarity_ransac + bbox_from_srt(E = I) on the first m rows -> (bbox, s, R, t) with s None for an invalid or
    no-consensus pose, the smallest relative distance of a residual to its threshold over every hypothesis the oracle evaluated (inf
    when there was none), and what the scan did: (kept hypothesis or -1, its inlier count, hypotheses examined)."""
    from oracle import align_ref as ar
    cap = nocs.shape[0]
    m = int(min(cap, int(count[0]) + int(count[1])))
    s, t = nocs[:m].astype(np.float64), cloud[:m].astype(np.float64)
    if m < 5 or np.isnan(s).any() or np.isnan(t).any():
        return ar.DEFAULT_BBOX.copy(), None, None, None, np.inf, (-1, 0, 0)
    drawn = []
    base = ar.hash_sampler(seed, pose)

    def sampler(i, n):
        idx = base(i, n)
        drawn.append(idx)
        return idx
    sc, R, tr, _ = ar.similarity_ransac(s, t, sampler)
    # the margin and the scan, from the hypotheses the oracle drew (the same arithmetic as similarity_ransac)
    n = m
    SH = np.transpose(np.hstack([s, np.ones([n, 1])]))
    TH = np.transpose(np.hstack([t, np.ones([n, 1])]))
    thr = 2 * np.amax(np.linalg.norm(SH[:3] - np.mean(SH[:3], axis=1)[:, None], axis=0)) / 10.0
    margin, best, kept, kept_n = np.inf, 0, -1, 0
    for i, idx in enumerate(drawn):
        Scale, _, _, T = ar.umeyama(SH[:, idx], TH[:, idx])
        res = np.linalg.norm((TH - T @ SH)[:3], axis=0)
        lim = Scale * thr
        if lim > 0:
            margin = min(margin, float(np.min(np.abs(res - lim)) / lim))
        c = int((res < lim).sum())
        if c / n > best:
            best, kept, kept_n = c / n, i, c
    if sc is None:
        return ar.DEFAULT_BBOX.copy(), None, None, None, margin, (-1, 0, len(drawn))
    return ar.bbox_from_srt(nocs[:m], sc, R, tr, np.eye(4)), sc, R, tr, margin, (kept, kept_n, len(drawn))
