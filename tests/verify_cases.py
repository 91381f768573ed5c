"""Inputs of the box verification tests (numpy only; shared by tests/test_verify_host.py and tests/test_gpu_verify.py).

Boxes are written in the frame of camera 0, which sits at the world origin and looks along +z (E = identity), so that what a case is
meant to hit (a frame border, the camera plane, the camera itself) can be read off its numbers.  Corner k of a box is
o + x_k ex + y_k ey + z_k ez with (x_k, y_k, z_k) the bits of k as in DEFAULT_BBOX: the model's edges are corner 2 (ey), 4 (ex), 1 (ez).
"""
import numpy as np

_BITS = np.asarray([[(k >> 2) & 1, (k >> 1) & 1, k & 1] for k in range(8)], dtype=np.float64)


def corners(o, ex, ey, ez):
    o, ex, ey, ez = (np.asarray(a, dtype=np.float64) for a in (o, ex, ey, ez))
    return o + _BITS[:, 0:1] * ex + _BITS[:, 1:2] * ey + _BITS[:, 2:3] * ez


def intrinsic(f, cx, cy):
    return np.asarray([[f, 0.0, cx], [0.0, f, cy], [0.0, 0.0, 1.0]])


def rotation(rng, angle):
    """A rotation by at most `angle` radians about a random axis."""
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    t = rng.uniform(-angle, angle)
    Kx = np.asarray([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * Kx + (1 - np.cos(t)) * (Kx @ Kx)


def extrinsic(rng, angle=0.25, shift=0.3):
    E = np.eye(4)
    E[:3, :3] = rotation(rng, angle)
    E[:3, 3] = rng.uniform(-shift, shift, 3)
    return E


# ---- the analytic case (a): 48 x 64, f = 32, integer principal point, an axis-aligned box whose near face z = 2 spans x in
# [-0.5, 0.25], y in [-0.25, 0.5]: its silhouette is the near face's, u = 32 x / 2 + 32 in [24, 36], v = 32 y / 2 + 24 in [20, 32]; every
# number is dyadic, so the boundary pixels are exact ties and the closed hit rule counts them.  dq is exactly 0 on column 32 and row 24.
ANALYTIC_HW = (48, 64)
ANALYTIC_K = intrinsic(32.0, 32.0, 24.0)
ANALYTIC_BOX = corners([-0.5, -0.25, 2.0], [0.75, 0, 0], [0, 0.75, 0], [0, 0, 1.0])
ANALYTIC_RECT = (20, 24, 32, 36)                   # row min, col min, row max, col max
ANALYTIC_AREA = 13 * 13


def special_boxes():
    """(boxes [12, 8, 3], ok [12], names): the cases (a) to (g) that need no camera of their own, in the frame of camera 0."""
    b, names = [], []

    def add(name, *a):
        names.append(name)
        b.append(corners(*a))

    add("axis_aligned", [-0.5, -0.25, 2.0], [0.75, 0, 0], [0, 0.75, 0], [0, 0, 1.0])
    add("sheared_negative_det", [-0.2, -0.3, 2.5], [0.4, 0.1, 0.0], [0.1, 0.3, 0.1], [0.05, -0.1, -0.5])
    add("border_left", [-2.4, -0.2, 2.0], [0.6, 0, 0.1], [0, 0.4, 0], [0, 0, 0.5])
    add("border_right", [1.8, -0.2, 2.0], [0.6, 0, 0.1], [0, 0.4, 0], [0, 0, 0.5])
    add("border_top", [-0.2, -1.8, 2.0], [0.4, 0, 0], [0, 0.6, 0.1], [0, 0, 0.5])
    add("border_bottom", [-0.2, 1.3, 2.0], [0.4, 0, 0], [0, 0.6, 0.1], [0, 0, 0.5])
    add("behind", [-0.3, -0.3, -3.0], [0.6, 0, 0], [0, 0.6, 0], [0, 0, 1.0])
    add("straddles_camera_plane", [0.3, -0.2, -0.5], [0.5, 0, 0], [0, 0.4, 0], [0, 0, 2.5])
    add("camera_inside", [-1.0, -1.0, -1.0], [2.0, 0, 0], [0, 2.0, 0], [0, 0, 2.0])
    add("zero_volume", [-0.2, -0.2, 2.0], [0.4, 0, 0], [0.8, 0, 0], [0, 0, 0.5])
    add("nan_corner", [-0.2, -0.2, 2.0], [0.4, 0, 0], [0, 0.4, 0], [0, 0, 0.5])
    b[-1][7, 1] = np.nan                            # a corner the model never reads still makes the box unusable
    add("not_ok", [-0.2, -0.2, 2.0], [0.4, 0, 0], [0, 0.4, 0], [0, 0, 0.5])
    ok = np.ones(len(b), dtype=np.uint8)
    ok[-1] = 0
    return np.stack(b), ok, names


def random_boxes(rng, count):
    """Rotated boxes scattered through and around the frustum of camera 0 (some partly or wholly out of view, some mirrored)."""
    out = []
    for _ in range(count):
        R = rotation(rng, np.pi)
        size = rng.uniform(0.1, 0.7, 3) * rng.choice([1.0, 1.0, 1.0, -1.0], 3)      # a negative edge mirrors the corner order
        centre = np.asarray([rng.uniform(-1.6, 1.6), rng.uniform(-1.2, 1.2), rng.uniform(0.9, 4.0)])
        ex, ey, ez = R[:, 0] * size[0], R[:, 1] * size[1], R[:, 2] * size[2]
        out.append(corners(centre - (ex + ey + ez) / 2, ex, ey, ez))
    return np.stack(out)


def random_mask(rng, H, W):
    """Bytes 0 / 1 / 255 in blocks, so that silhouettes meet foreground and background."""
    coarse = rng.choice(np.asarray([0, 0, 1, 255], dtype=np.uint8), ((H + 7) // 8, (W + 7) // 8))
    return np.repeat(np.repeat(coarse, 8, axis=0), 8, axis=1)[:H, :W].copy()


def _boxes(rng, n, S):
    sp, ok_sp, _ = special_boxes()
    boxes, ok = np.empty((n, S, 8, 3)), np.ones((n, S), dtype=np.uint8)
    for i in range(n):
        k = min(S, len(sp))
        order = rng.permutation(len(sp))[:k] if S < len(sp) else np.arange(len(sp))
        boxes[i, :k], ok[i, :k] = sp[order], ok_sp[order]
        if S > k:
            boxes[i, k:] = random_boxes(rng, S - k)
    return boxes, ok


def _views(rng, n, V, K):
    E = np.stack([np.stack([np.eye(4) if v == 0 else extrinsic(rng) for v in range(V)]) for _ in range(n)])
    return np.broadcast_to(K, (n, V, 3, 3)).copy(), E


def _masks(rng, n, V, H, W):
    m = np.stack([np.stack([random_mask(rng, H, W) for _ in range(V)]) for _ in range(n)])
    return m


def silhouette_cases():
    """-> list of dicts: name, boxes [n,S,8,3], ok [n,S] or None, K, E, masks, and `offset`: the byte offset of the mask's base address
    from 4-byte alignment the GPU test must give it (0: aligned)."""
    cases = []
    H, W = ANALYTIC_HW
    full = np.full((1, 1, H, W), 255, dtype=np.uint8)
    cases.append(dict(name="analytic", boxes=ANALYTIC_BOX[None, None], ok=None, K=ANALYTIC_K[None], E=np.eye(4)[None, None], masks=full, offset=0))

    # (a)-(h): every special box in every pose, V = 2; pose 0: random bytes / empty mask, pose 1: full mask / random bytes,
    # pose 2: view 1 has K00 = 0 (every box unusable there, the mask still counted)
    rng = np.random.default_rng(11)
    n, S, V = 3, 14, 2
    boxes, ok = _boxes(rng, n, S)
    K, E = _views(rng, n, V, ANALYTIC_K)
    K[2, 1, 0, 0] = 0.0
    masks = _masks(rng, n, V, H, W)
    masks[0, 1] = 0
    masks[1, 0] = 255
    cases.append(dict(name="special_48x64", boxes=boxes, ok=ok, K=K, E=E, masks=masks, offset=0))

    # (i): odd width, unaligned base: the byte path; the squeezed forms of the arguments (V = 1, K [n,3,3])
    rng = np.random.default_rng(12)
    Ho, Wo = 37, 63
    boxes, ok = _boxes(rng, 2, 5)
    cases.append(dict(name="odd_37x63_unaligned", boxes=boxes, ok=ok, K=np.broadcast_to(intrinsic(30.0, 31.25, 18.5), (2, 3, 3)).copy(),
                      E=np.stack([np.eye(4), extrinsic(rng)]), masks=_masks(rng, 2, 1, Ho, Wo)[:, 0], offset=1))
    # the same frame size with an aligned base still takes the byte path (H W is odd); and an even frame on an unaligned base
    boxes, ok = _boxes(rng, 1, 5)
    cases.append(dict(name="odd_37x63_aligned", boxes=boxes, ok=ok, K=intrinsic(30.0, 31.25, 18.5)[None], E=np.eye(4)[None, None],
                      masks=_masks(rng, 1, 1, Ho, Wo), offset=0))
    boxes, ok = _boxes(rng, 1, 5)
    cases.append(dict(name="even_48x64_unaligned", boxes=boxes, ok=ok, K=ANALYTIC_K[None], E=np.eye(4)[None, None],
                      masks=_masks(rng, 1, 1, H, W), offset=3))

    # (j): S = 64 with V = 16
    rng = np.random.default_rng(13)
    boxes, ok = _boxes(rng, 1, 64)
    K, E = _views(rng, 1, 16, ANALYTIC_K)
    cases.append(dict(name="s64_v16", boxes=boxes, ok=ok, K=K, E=E, masks=_masks(rng, 1, 16, H, W), offset=0))

    # (i): one 480 x 640 pose (300 tiles of 1.6 rows: the bounds cull most of them)
    rng = np.random.default_rng(14)
    boxes, ok = _boxes(rng, 1, 5)
    boxes[0, 4] = random_boxes(rng, 1)[0]
    K, E = _views(rng, 1, 2, intrinsic(439.3, 320.0, 240.0))
    cases.append(dict(name="frame_480x640", boxes=boxes, ok=ok, K=K, E=E, masks=_masks(rng, 1, 2, 480, 640), offset=0))

    # more tiles than the launch has workgroups (200 x 16 frames of 3 tiles > 8192): the grid-stride walk
    rng = np.random.default_rng(15)
    n, V = 200, 16
    boxes = random_boxes(rng, n)[:, None]
    K, E = _views(rng, n, V, intrinsic(30.0, 31.25, 18.5))
    masks = np.broadcast_to(_masks(rng, 4, V, Ho, Wo)[None], (n // 4, 4, V, Ho, Wo)).reshape(n, V, Ho, Wo).copy()
    cases.append(dict(name="grid_stride", boxes=boxes, ok=None, K=K, E=E, masks=masks, offset=0))
    return cases


def cloud_cases():
    """-> list of dicts: name, cloud [n,cap,3] f32, count, boxes [n,S,8,3], ok.  Case (k): counts 0, 1, cap, more than cap, a NaN row, and
    points exactly on a face of a dyadic box (inside with inflate 0: the test is closed) and 3 % of an edge outside it (inside with
    inflate 0.05 only)."""
    rng = np.random.default_rng(21)
    n, cap, S = 6, 2500, 4
    unit = corners([0.0, 0.0, 0.0], [1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0])
    boxes = np.empty((n, S, 8, 3))
    ok = np.ones((n, S), dtype=np.uint8)
    for i in range(n):
        sp = special_boxes()[0]
        boxes[i] = np.stack([unit, sp[1], sp[9], random_boxes(rng, 1)[0]])          # dyadic, sheared with det < 0, zero volume, rotated
    ok[1, 3] = 0
    cloud = rng.uniform(-0.5, 1.5, (n, cap, 3)).astype(np.float32)
    cloud[:, ::3] = (rng.uniform(-0.5, 0.5, (n, len(range(0, cap, 3)), 3)) + [0.0, 0.0, 2.4]).astype(np.float32)      # near the sheared box
    on_face = np.asarray([[1.0, 0.5, 0.5], [0.0, 0.25, 0.75], [0.5, 1.0, 0.5], [0.5, 0.0, 0.125], [0.25, 0.5, 1.0], [0.5, 0.5, 0.0],
                          [1.0, 1.0, 1.0], [0.0, 0.0, 0.0]], dtype=np.float32)
    outside = np.asarray([[1.03125, 0.5, 0.5], [-0.03125, 0.5, 0.5], [0.5, 1.03125, 0.5], [0.5, 0.5, -0.03125], [1.0625, 0.5, 0.5]], dtype=np.float32)
    cloud[:, 1:1 + len(on_face)] = on_face
    cloud[:, 20:20 + len(outside)] = outside
    cloud[4, 5] = np.nan
    cloud[4, 40, 1] = np.inf
    count = np.asarray([[0, 0], [1, 0], [cap // 2, cap - cap // 2], [cap, cap], [700, 300], [0, 1500]], dtype=np.int32)
    for i in range(n):
        cloud[i, min(int(count[i].sum()), cap):] = np.nan                           # what cloud_pack leaves past the kept rows
    cases = [dict(name="two_view_counts", cloud=cloud, count=count, boxes=boxes, ok=ok)]
    cases.append(dict(name="flat_count", cloud=cloud, count=np.minimum(count.sum(1), cap).astype(np.int32), boxes=boxes, ok=None))
    cases.append(dict(name="view_counts_one_box", cloud=cloud[:, :1024], count=np.stack([count[:, 0], count[:, 1] // 2, count[:, 1] // 3], 1),
                      boxes=boxes[:, 0], ok=None))
    cases.append(dict(name="s64", cloud=cloud[2:4], count=np.asarray([[1200, 800], [5, 5]], np.int32),
                      boxes=np.concatenate([boxes[2:4], random_boxes(rng, 120).reshape(2, 60, 8, 3)], 1), ok=None))
    return cases


INFLATES = (0.0, 0.05)


# ---- seeded scenes of the synthetic camera, for the twin against the renderer's own twin
def hand_camera_scenes(N, episode=0, seed=5):
    """N scenes of `synthetic_env.sample_scene` seen from seeded hand-camera poses that look at the handle, a few degrees off."""
    from oracle import control_ref as cr
    from rgbmanip_amd import synthetic_env as se
    robots, boxes = (np.stack(a) for a in zip(*[se.sample_scene(i, episode) for i in range(N)]))
    rng = np.random.default_rng(seed)
    cam = np.zeros((N, 7))
    cam[:, :3] = rng.uniform([-0.3, -0.3, 0.4], [0.3, 0.3, 1.0], (N, 3))
    heading = boxes[:, :3] - (robots[:, :3] + cam[:, :3])
    heading = heading / np.linalg.norm(heading, axis=1, keepdims=True) + rng.normal(0, 0.05, (N, 3))
    cam[:, 3:] = cr.canonical_quat(cr.lookat_quat(heading))
    return robots, boxes, cam
