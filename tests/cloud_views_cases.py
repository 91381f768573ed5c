"""Scenes shared by the multi-view fusion tests, computed once per process and handed out read-only."""
import functools

import numpy as np

from rgbmanip_amd import synth
from rgbmanip_amd.cloud import depth_fusion_ref

S = 224
SCENES = {4: (0, 5), 6: (0, 5, 11)}      # V -> the seeds whose camera pairs make up the views


def _frozen(x):
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def sphere_views(V):
    """The sphere of `synth.sphere_depth` seen by V cameras in each of 2 poses: views 2 s, 2 s + 1 = (K1, E1), (K2, E2) of
    synth.adapose_inputs(2, seed) for the seeds of SCENES[V].  Returns (depth [2,V,S,S] f32, K [2,V,3,3], E [2,V,4,4])."""
    Ks, Es = [], []
    for seed in SCENES[V]:
        inp = synth.adapose_inputs(2, seed=seed)
        Ks += [inp["K1"], inp["K2"]]
        Es += [inp["E1"], inp["E2"]]
    K, E = np.stack(Ks, axis=1).astype(np.float64), np.stack(Es, axis=1).astype(np.float64)
    depth = np.stack([synth.sphere_depth(K[:, v], E[:, v]) for v in range(V)], axis=1)
    return _frozen(depth), _frozen(K), _frozen(E)


@functools.lru_cache(maxsize=None)
def conf_and_mask(V):
    """Seeded uniform confidences [2,V,S,S] f32 and an elliptical mask [2,V,S,S] u8 (another ellipse per view)."""
    g = np.random.default_rng(77 + V)
    conf = g.random((2, V, S, S), dtype=np.float32)
    y, x = np.mgrid[0:S, 0:S]
    mask = np.empty((2, V, S, S), dtype=np.uint8)
    for i in range(2):
        for v in range(V):
            mask[i, v] = (((x - 105 - 3 * v) / (95.0 - 2 * v)) ** 2 + ((y - 118 + 2 * i) / (80.0 + v)) ** 2 <= 1.0)
    return _frozen(conf), _frozen(mask)


@functools.lru_cache(maxsize=None)
def sphere_ref(V, n_min, with_conf):
    """`depth_fusion_ref` of the scene at the default thresholds (with_conf: conf_min 0.5 and the mask)."""
    depth, K, E = sphere_views(V)
    kw = {}
    if with_conf:
        conf, mask = conf_and_mask(V)
        kw = dict(conf=conf, mask=mask, conf_min=0.5)
    r = depth_fusion_ref(depth, K, E, n_min=n_min, **kw)
    return {k: _frozen(v) for k, v in r.items()}


def assert_scene_preconditions(V):
    """What the kernel-against-twin comparison rests on: no sampled pixel / source pair within 1e-6 px or 1e-8 (relative) of its
    threshold, so float64 rounding differences between the twin and the kernel cannot flip a decision; and every count 0 .. V - 1 of
    agreeing sources occurs in every view of both poses."""
    r = sphere_ref(V, 1, False)
    m = r["margin"]
    with np.errstate(invalid="ignore"):
        assert not (m[..., 0] < 1e-6).any(), int((m[..., 0] < 1e-6).sum())
        assert not (m[..., 1] < 1e-8).any(), int((m[..., 1] < 1e-8).sum())
    rarest = min(int((r["nviews"][i, a] == c).sum()) for i in range(2) for a in range(V) for c in range(V))
    assert rarest >= 1, rarest
    return rarest
