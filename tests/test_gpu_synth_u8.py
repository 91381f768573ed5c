"""-m gpu: the synthetic camera delivering bytes — `rgbm_synth_render_u8` through the C ABI, `SyntheticMultiVecEnv(color_dtype="uint8")`,
`render_into` and the controller's `hip_render_to_queue` — bit for bit against the code paths that existed before it: the expected
values always come from `rgbm_synth_camera`, `rgbm_synth_render`, `rgbm_quantize_frames` and `rgbm_mask_extent` (or their numpy
restatements), never from the kernel under test."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rgbmanip_amd import _lib, synth  # noqa: E402

_CACHE = {}
GUARD = 0xA5


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------------------------ 1. the kernel
def _scene_arrays():
    """Four envs, camera 0.7 m up looking along +x (env 3: slightly rotated): a box fully inside the frame, a box cut by the top and
    the right border, a box behind the camera, and a second box inside the frame of another size."""
    X, Y, Z = [0, 0, 1.0], [0, 1.0, 0], [-1.0, 0, 0]
    box = np.array([[1.0, 0.05, 0.72] + X + Y + Z + [0.15, 0.10, 0.03],
                    [1.0, -0.70, 1.20] + X + Y + Z + [0.20, 0.20, 0.03],
                    [-1.0, 0.0, 0.70] + X + Y + Z + [0.15, 0.10, 0.03],
                    [0.9, 0.20, 0.55] + X + Y + Z + [0.08, 0.12, 0.05]])
    robot = np.zeros((4, 7))
    robot[:, 3] = 1
    robot[:, 0] = [0.0, 0.02, -0.01, 0.03]
    cam = np.zeros((4, 7))
    cam[:, 2], cam[:, 3] = 0.7, 1.0
    cam[3, 3:] = [0.99, 0.01, 0.05, -0.03]
    return robot, box, cam


def _expected(H, W, env0):
    """The parent's path on a hand-filled scene: camera -> float render -> quantise, mask extent.  Computed once per case and shared;
    holds the device inputs (scene record, rays) the kernel under test is then given."""
    key = (H, W, env0)
    if key in _CACHE:
        return _CACHE[key]
    from oracle import synth_env_ref as sr
    lib = _lib.load()
    N = 4
    robot, box, cam = _scene_arrays()
    hold = dict(cam=_cuda(cam), robot=_cuda(robot), box=_cuda(box))
    f = (H / 2) / math.tan(0.5)                                   # fovy = 1 rad, scaled to the frame
    sc = _lib.SynthScene()
    sc.cam_pose, sc.robot_pose, sc.box = hold["cam"].data_ptr(), hold["robot"].data_ptr(), hold["box"].data_ptr()
    sc.fx = sc.fy = f
    sc.cx, sc.cy = W / 2, H / 2
    sc.N, sc.H, sc.W, sc.env0 = N, H, W, env0
    K = torch.empty(N, 3, 3, dtype=torch.float64, device="cuda")
    E = torch.empty(N, 4, 4, dtype=torch.float64, device="cuda")
    rays = torch.empty(N, 12, dtype=torch.float64, device="cuda")
    colf = torch.empty(N, H, W, 3, dtype=torch.float32, device="cuda")
    mask = torch.empty(N, H, W, dtype=torch.uint8, device="cuda")
    col8 = torch.empty(N, H, W, 3, dtype=torch.uint8, device="cuda")
    ext = torch.empty(N, 4, dtype=torch.int32, device="cuda")
    cnt = torch.empty(N, dtype=torch.int32, device="cuda")
    s = _lib.stream_ptr()
    _lib.check(lib.rgbm_synth_camera(C.byref(sc), _lib.ptr(K), _lib.ptr(E), _lib.ptr(rays), s), "rgbm_synth_camera")
    _lib.check(lib.rgbm_synth_render(C.byref(sc), _lib.ptr(rays), _lib.ptr(colf), _lib.ptr(mask), s), "rgbm_synth_render")
    _lib.check(lib.rgbm_quantize_frames(_lib.ptr(colf), _lib.ptr(col8), colf.numel(), s), "rgbm_quantize_frames")
    _lib.check(lib.rgbm_mask_extent(_lib.ptr(mask), N, H, W, _lib.ptr(ext), _lib.ptr(cnt), s), "rgbm_mask_extent")
    torch.cuda.synchronize()
    exp = dict(sc=sc, hold=hold, rays=rays, color=col8.cpu().numpy(), mask=mask.cpu().numpy(), ext=ext.cpu().numpy(), cnt=cnt.cpu().numpy())
    # conditions on the INPUTS (from the float path's mask): three envs show their box and some background, one shows no box; the
    # cut box touches row 0 and the last column; the float path is the numpy twin's frame
    m = exp["mask"].reshape(N, -1)
    assert set(np.unique(m)) <= {0, 1}
    for e in (0, 1, 3):
        assert 0 < m[e].sum() < H * W, (e, m[e].sum())
    assert m[2].sum() == 0
    assert exp["ext"][1, 0] == 0 and exp["ext"][1, 3] == W - 1 and exp["ext"][2].tolist() == [2 * H, 2 * W, 0, 0] and exp["cnt"][2] == 0
    _, _, rays_ref = sr.camera_ref(cam, robot, box, f, f, W / 2, H / 2)
    color_ref, mask_ref = sr.render_ref(rays_ref, box, f, f, W / 2, H / 2, H, W, env0=env0)
    assert np.array_equal(rays.cpu().numpy(), rays_ref) and np.array_equal(exp["mask"], mask_ref)
    if env0 >= 0:                                                 # (a negative id: C's % and numpy's differ in the background)
        assert np.array_equal(colf.cpu().numpy(), color_ref)
        with np.errstate(all="ignore"):
            assert np.array_equal(exp["color"], np.clip(np.rint(color_ref * np.float32(255)), 0, 255).astype(np.uint8))
    ys, xs = np.nonzero(mask_ref[0])
    assert exp["ext"][0].tolist() == [ys.min(), xs.min(), ys.max(), xs.max()] and exp["cnt"][0] == len(ys)
    _CACHE[key] = exp
    return exp


def _render_u8(exp, offset, with_extent):
    """rgbm_synth_render_u8 into 0xA5-filled buffers, colour and mask `offset` bytes past an aligned address, with guard bytes on both
    sides of every output -> (color, mask, ext or None, cnt or None, guards intact)."""
    sc = exp["sc"]
    N, H, W = sc.N, sc.H, sc.W
    pad = 16
    cbuf = torch.full((pad + offset + N * H * W * 3 + pad,), GUARD, dtype=torch.uint8, device="cuda")
    mbuf = torch.full((pad + offset + N * H * W + pad,), GUARD, dtype=torch.uint8, device="cuda")
    ebuf = torch.full((4 + N * 4 + 4,), -0x5A5A5A5B, dtype=torch.int32, device="cuda")          # 0xA5A5A5A5
    nbuf = torch.full((4 + N + 4,), -0x5A5A5A5B, dtype=torch.int32, device="cuda")
    assert cbuf.data_ptr() % 4 == 0 and mbuf.data_ptr() % 4 == 0
    c0, m0 = pad + offset, pad + offset
    eptr = C.c_void_p(ebuf.data_ptr() + 16) if with_extent else None
    nptr = C.c_void_p(nbuf.data_ptr() + 16) if with_extent else None
    _lib.check(_lib.load().rgbm_synth_render_u8(C.byref(sc), _lib.ptr(exp["rays"]), C.c_void_p(cbuf.data_ptr() + c0),
                                                C.c_void_p(mbuf.data_ptr() + m0), eptr, nptr, _lib.stream_ptr()), "rgbm_synth_render_u8")
    torch.cuda.synchronize()
    c, m, e, n = cbuf.cpu().numpy(), mbuf.cpu().numpy(), ebuf.cpu().numpy(), nbuf.cpu().numpy()
    nc, nm = N * H * W * 3, N * H * W
    clean = bool((c[:c0] == GUARD).all() and (c[c0 + nc:] == GUARD).all() and (m[:m0] == GUARD).all() and (m[m0 + nm:] == GUARD).all()
                 and (e[:4] == -0x5A5A5A5B).all() and (e[4 + 4 * N:] == -0x5A5A5A5B).all() and (n[:4] == -0x5A5A5A5B).all()
                 and (n[4 + N:] == -0x5A5A5A5B).all())
    if not with_extent:
        clean = clean and bool((e == -0x5A5A5A5B).all() and (n == -0x5A5A5A5B).all())
    return (c[c0:c0 + nc].reshape(N, H, W, 3), m[m0:m0 + nm].reshape(N, H, W), e[4:4 + 4 * N].reshape(N, 4) if with_extent else None,
            n[4:4 + N] if with_extent else None, clean)


@pytest.mark.parametrize("env0", [0, 517, -3])
@pytest.mark.parametrize("H,W", [(8, 12), (7, 10), (40, 52)])
def test_render_u8_equals_render_quantise_extent(H, W, env0):
    """8x12: 32-bit stores; 7x10: H*W % 4 != 0, byte stores; 40x52: three workgroups per env whose 1024 pixels span rows and which share
    a box.  env0 is a field of the scene record (the partition's first global env id), so "an env with env0 != 0" is the same four envs
    in a partition that starts at 517; at -3 the background's pattern indices are negative for some pixels, which the kernel's background
    table cannot index: it evaluates the pattern per pixel there.  Colour, mask, extent and count equal the parent's render -> quantise / mask-extent bit for bit;
    the same with colour and mask one byte past alignment, and with extent = count = NULL; nothing outside the outputs is written."""
    exp = _expected(H, W, env0)
    for offset, with_extent in ((0, True), (1, True), (0, False), (1, False)):
        color, mask, ext, cnt, clean = _render_u8(exp, offset, with_extent)
        tag = (H, W, env0, offset, with_extent)
        assert np.array_equal(mask, exp["mask"]), tag
        assert np.array_equal(color, exp["color"]), (tag, np.argwhere(color != exp["color"])[:4])
        if with_extent:
            assert np.array_equal(ext, exp["ext"]), (tag, ext, exp["ext"])
            assert np.array_equal(cnt, exp["cnt"]), (tag, cnt, exp["cnt"])
        assert clean, tag


def test_render_u8_refuses_one_null_of_extent_and_count():
    exp = _expected(8, 12, 0)
    sc = exp["sc"]
    color = torch.empty(sc.N, sc.H, sc.W, 3, dtype=torch.uint8, device="cuda")
    mask = torch.empty(sc.N, sc.H, sc.W, dtype=torch.uint8, device="cuda")
    ext = torch.empty(sc.N, 4, dtype=torch.int32, device="cuda")
    cnt = torch.empty(sc.N, dtype=torch.int32, device="cuda")
    lib = _lib.load()
    for e, n in ((ext, None), (None, cnt)):
        assert lib.rgbm_synth_render_u8(C.byref(sc), _lib.ptr(exp["rays"]), _lib.ptr(color), _lib.ptr(mask), _lib.ptr(e), _lib.ptr(n),
                                        _lib.stream_ptr()) != 0
    assert lib.rgbm_synth_render_u8(C.byref(sc), _lib.ptr(exp["rays"]), None, _lib.ptr(mask), _lib.ptr(ext), _lib.ptr(cnt),
                                    _lib.stream_ptr()) != 0


# ------------------------------------------------------------------------------------------------------------------ 2. the env
def _synth_inputs(N, episode=0):
    from oracle import control_ref as cr
    from rgbmanip_amd import synthetic_env as se
    robots, boxes = (np.stack(a) for a in zip(*[se.sample_scene(i, episode) for i in range(N)]))
    rng = np.random.default_rng(5)
    cam = np.zeros((N, 7))
    cam[:, :3] = rng.uniform([-0.3, -0.3, 0.4], [0.3, 0.3, 1.0], (N, 3))
    heading = np.concatenate([np.ones((N, 1)), rng.normal(0, 0.15, (N, 2))], axis=1)
    heading[:, 2] -= 0.1
    cam[:, 3:] = cr.canonical_quat(cr.lookat_quat(heading)) * 1.7          # un-normalised on purpose: the kernel normalises
    return robots, boxes, cam


def _env_pair(N):
    from rgbmanip_amd import synthetic_env as se
    robots, boxes, cam = _synth_inputs(N)
    envs = []
    for dt in ("float32", "uint8"):
        env = se.SyntheticMultiVecEnv(N, "cuda", seed=0, color_dtype=dt)
        env._robot.copy_(torch.from_numpy(robots)); env._box.copy_(torch.from_numpy(boxes)); env._cam.copy_(torch.from_numpy(cam))
        envs.append(env)
    return envs


def test_env_uint8_color_is_the_quantised_float_color():
    """N = 2 at 480x640: get_image() of a color_dtype="uint8" env against an identically set-up float env — Color equals
    rgbm_quantize_frames of the float Color, Mask / Intrinsic / Extrinsic are identical; render_into writes the same view plus
    rgbm_mask_extent's extent and count, and refuses tensors of another dtype, shape or layout."""
    N = 2
    fenv, benv = _env_pair(N)
    want, got = fenv.get_image()["camera0"], benv.get_image()["camera0"]
    assert want["Color"].dtype == torch.float32 and got["Color"].dtype == torch.uint8 and got["Color"].shape == (N, 480, 640, 3)
    q = torch.empty(N, 480, 640, 3, dtype=torch.uint8, device="cuda")
    lib = _lib.load()
    _lib.check(lib.rgbm_quantize_frames(_lib.ptr(want["Color"]), _lib.ptr(q), q.numel(), _lib.stream_ptr()), "rgbm_quantize_frames")
    ext = torch.empty(N, 4, dtype=torch.int32, device="cuda")
    cnt = torch.empty(N, dtype=torch.int32, device="cuda")
    _lib.check(lib.rgbm_mask_extent(_lib.ptr(want["Mask"]), N, 480, 640, _lib.ptr(ext), _lib.ptr(cnt), _lib.stream_ptr()), "rgbm_mask_extent")
    assert torch.equal(got["Color"], q)
    for k in ("Mask", "Intrinsic", "Extrinsic"):
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k
    assert int(cnt.min()) > 0 and int(q.max()) > int(q.min())    # every handle is in view; the frames are not flat
    # render_into: the same view into caller-owned tensors
    out = dict(color=torch.full((N, 480, 640, 3), GUARD, dtype=torch.uint8, device="cuda"),
               mask=torch.full((N, 480, 640), GUARD, dtype=torch.uint8, device="cuda"),
               intrinsic=torch.zeros(N, 3, 3, dtype=torch.float64, device="cuda"), extrinsic=torch.zeros(N, 4, 4, dtype=torch.float64, device="cuda"),
               extent=torch.full((N, 4), -7, dtype=torch.int32, device="cuda"), count=torch.full((N,), -7, dtype=torch.int32, device="cuda"))
    assert benv.render_into(**out) is None
    assert torch.equal(out["color"], q) and torch.equal(out["mask"], want["Mask"])
    assert torch.equal(out["intrinsic"], want["Intrinsic"]) and torch.equal(out["extrinsic"], want["Extrinsic"])
    assert torch.equal(out["extent"], ext) and torch.equal(out["count"], cnt)
    bad = dict(color=out["color"].float(), mask=out["mask"][:, :, :639], intrinsic=out["intrinsic"].transpose(1, 2),
               extrinsic=out["extrinsic"].cpu(), extent=out["extent"].long(), count=out["count"][:1])
    for name, t in bad.items():
        with pytest.raises(ValueError, match=name):
            benv.render_into(**dict(out, **{name: t}))


# ------------------------------------------------------------------------------------------------------------------ 3. the controller
def _est(**kw):
    from rgbmanip_amd.adapose import AdaPoseNet
    from rgbmanip_amd.config import ADAPOSE_CFGS
    from rgbmanip_amd.estimator import AdaPoseEstimator_v5
    if "net" not in _CACHE:
        _CACHE["net"] = AdaPoseNet(synth.adapose_state_dict(seed=0, prefix="module."), dtype="fp32", options={"view2_heads": 0})
    cfg = dict(ADAPOSE_CFGS["adapose_cabinet"], load=False, hip_prepare="device", hip_prepare_seed=9, **kw)
    return AdaPoseEstimator_v5(None, cfg, None, net=_CACHE["net"], dtype="fp32")


@pytest.mark.parametrize("cache", [False, True])
def test_controller_render_to_queue_equals_add_view(cache):
    """Two ControlInterfaces on identically seeded synthetic envs (2 envs, max_steps 3, byte queue), reset + three steps with the same
    actions: hip_render_to_queue against get_image() -> add_view.  Observations, rewards, pred_bbox and every queue agree bit for bit,
    the estimator saw the same frames, and the direct side never calls get_image.  cache: with the per-slot feature cache."""
    from rgbmanip_amd import synthetic_env as se
    from rgbmanip_amd.control_interface import ControlInterface
    N = 2
    runs = {}
    for direct in (False, True):
        est = _est(hip_feature_cache=True) if cache else _est()
        env = se.SyntheticMultiVecEnv(N, "cuda", seed=3)
        cfg = synth.control_cfg("cabinet", 0.0)
        cfg["controller"]["max_steps"] = 3
        cfg["controller"]["hip_queue_dtype"] = "uint8"
        if direct:
            cfg["controller"]["hip_render_to_queue"] = True

            def no_get_image(*a, **k):
                raise AssertionError("get_image() called on the render-to-queue path")
            env.get_image = no_get_image
        views0, native0 = est.feature_views_computed, est.frames_u8_native
        ci = ControlInterface(env, est, se.SyntheticManipulation(env), cfg)
        assert ci.render_to_queue is direct
        obs, rew = [ci.get_observation().cpu().numpy()], []
        for s in range(3):
            o, r, done, _ = ci.step(_cuda(synth.control_actions(N, s, 9) * 0.3))
            obs.append(o.cpu().numpy())
            rew.append(r.cpu().numpy())
        runs[direct] = dict(ci=ci, obs=np.stack(obs), rew=np.stack(rew), views=est.feature_views_computed - views0,
                            native=est.frames_u8_native - native0)
    a, b = runs[True], runs[False]
    assert np.array_equal(a["obs"], b["obs"]) and np.array_equal(a["rew"], b["rew"])
    for name in ("pred_bbox", "image_queue", "mask_queue", "bbox_queue", "available", "intrinsic_queue", "extrinsic_queue", "pose_queue",
                 "available_num"):
        qa, qb = getattr(a["ci"], name), getattr(b["ci"], name)
        assert qa.dtype == qb.dtype and torch.equal(qa, qb), name
    assert a["ci"].image_queue.dtype == torch.uint8
    pred = a["ci"].pred_bbox.cpu().numpy()
    assert np.isfinite(pred).all() and np.abs(pred[1:]).max() > 0
    assert int(a["ci"].mask_queue.sum()) > 0 and float(a["ci"].available.sum()) > 0      # handles were seen
    assert a["native"] == b["native"] == 3 * 2 * N
    assert a["views"] == b["views"] == ((2 * N + N + N) if cache else 3 * 2 * N)
