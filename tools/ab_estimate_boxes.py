"""Boxes and feature-cache counters of a fixed list of estimator calls on seeded synthetic inputs, written to an .npz: run it in two
trees (each run its own process, both with RGBM_HIP_LIB at the same librgbm_hip.so) and compare bit for bit.

usage: ab_estimate_boxes.py out.npz            (in each tree)
       ab_estimate_boxes.py --dense out.npz    (the dense calls alone: `dense` below)
       ab_estimate_boxes.py --compare a.npz b.npz

Inputs: n = 5 poses of 480x640 with one empty mask (big ellipse, blob at the border, empty, two corner blobs, thin line) — three chunks
with a single-pose last chunk at hip_upload_chunk = 2; only names both trees have are used (public calls and `_CHUNK_BYTES`)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def compare(a, b):
    A, B = np.load(a), np.load(b)
    if sorted(A.files) != sorted(B.files):
        print("different call lists:", sorted(set(A.files) ^ set(B.files)))
        return 1
    for k in A.files:
        if A[k].shape != B[k].shape or A[k].dtype != B[k].dtype or A[k].tobytes() != B[k].tobytes():      # bytes: the dense maps hold NaN
            print(f"FIRST DIFFERENCE at {k}: shapes {A[k].shape} {B[k].shape}, dtypes {A[k].dtype} {B[k].dtype}")
            return 1
    print(f"all equal: {len(A.files)} arrays\n" + "\n".join(sorted(A.files)))
    return 0


def case(seed=5):
    rng = np.random.default_rng(seed)
    N, H, W = 5, 480, 640
    rgb = rng.random((N, H, W, 3), dtype=np.float32)
    yy, xx = np.mgrid[0:H, 0:W]
    mask = np.zeros((N, H, W), dtype=np.uint8)
    mask[0] = (((yy - 250) / 120.0) ** 2 + ((xx - 300) / 170.0) ** 2) < 1.0
    mask[1] = (((yy - 12) / 9.0) ** 2 + ((xx - 630) / 7.0) ** 2) < 1.0
    mask[3][440:480, 600:640] = 1
    mask[3][0:30, 0:25] = 1
    mask[4][200:203, 50:400] = 1
    K = np.tile(np.array([[439.31, 0, 320.0], [0, 439.31, 240.0], [0, 0, 1.0]]), (N, 1, 1))
    K[:, 0, 2] += np.arange(N) * 1.5
    return rgb, mask, K


def main(path):
    import torch
    from rgbmanip_amd import synth
    from rgbmanip_amd.adapose import AdaPoseNet
    from rgbmanip_amd.config import ADAPOSE_CFGS
    from rgbmanip_amd.control_interface import ControlInterface
    from rgbmanip_amd.estimator import AdaPoseEstimator_v5
    out = {}
    rgb, mask, K = case()
    rgb2, mask2 = np.ascontiguousarray(rgb[:, :, ::-1]), np.ascontiguousarray(mask[:, :, ::-1])
    rgb3 = np.ascontiguousarray(rgb[:, ::-1])                     # a third frame set with the first's masks flipped the same way
    mask3 = np.ascontiguousarray(mask[:, ::-1])
    N = len(rgb)
    inp = synth.adapose_inputs(N, seed=2)
    E1, E2 = inp["E1"].astype(np.float64), inp["E2"].astype(np.float64)
    base = dict(ADAPOSE_CFGS["adapose_cabinet"], load=False, hip_prepare="device", hip_prepare_seed=9)
    sd = synth.adapose_state_dict(seed=0, prefix="module.")
    frames = {"f64": lambda x: x.astype(np.float64), "f32": lambda x: x, "u8": lambda x: np.clip(np.rint(x * 255.0), 0, 255).astype(np.uint8)}
    masks = {"bool": lambda m: m.astype(bool), "u8": lambda m: m * np.uint8(255), "f64": lambda m: m.astype(np.float64) * 0.5}

    def put(name, est, box):
        out[name] = box.cpu().numpy() if isinstance(box, torch.Tensor) else np.asarray(box)
        out[name + "|counters"] = np.array([est.feature_views_computed, est.feature_cache_bypassed])

    for dt in ("bf16x3", "bf16"):
        net = AdaPoseNet(sd, dtype=dt, options={"view2_heads": 0})
        mk = lambda **kw: AdaPoseEstimator_v5(None, dict(base, **kw), None, dtype=dt, net=net)      # noqa: E731
        for chunk in (0, 2, 32):
            for small in (False, True):
                est = mk(hip_upload_chunk=chunk)
                if small:
                    est._CHUNK_BYTES = 480 * 640 * 3 * 4              # one float32 frame per staging chunk of the whole-array upload
                for fn, f in frames.items():
                    for mn, m in masks.items():
                        put(f"{dt} estimate chunk={chunk} small_staging={small} frames={fn} masks={mn}", est,
                            est.estimate(K, f(rgb), m(mask), E1, f(rgb2), m(mask2), E2))
        est = mk()
        cu = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()      # noqa: E731
        put(f"{dt} estimate_device cuda", est, est.estimate_device(cu(K), cu(rgb), cu(mask), cu(E1), cu(rgb2), cu(mask2), cu(E2)))
        put(f"{dt} estimate cuda tensors", est, est.estimate(K, cu(rgb), cu(mask), E1, cu(rgb2), cu(mask2), E2))
        est = mk(hip_prepare="host")
        est.rng = np.random.default_rng(11)
        put(f"{dt} hip_prepare=host generator 11", est, est.estimate(K, rgb, mask, E1, rgb2, mask2, E2))
        est = mk(hip_prepare="host")
        est.rng = ("hash", 3)
        put(f"{dt} hip_prepare=host hash", est, est.estimate(K, rgb, mask, E1, rgb2, mask2, E2))
        for mode in (False, True, "content"):
            for chunk in (32, 2):
                est = mk(hip_feature_cache=mode, hip_upload_chunk=chunk)
                put(f"{dt} cache={mode} chunk={chunk} call A", est, est.estimate(K, frames["f64"](rgb), mask.astype(bool), E1, frames["f64"](rgb2), mask2.astype(bool), E2))
                put(f"{dt} cache={mode} chunk={chunk} call B (view 2 repeats)", est,
                    est.estimate(K, frames["f64"](rgb3), mask3.astype(bool), E1, frames["f64"](rgb2), mask2.astype(bool), E2))
                put(f"{dt} cache={mode} chunk={chunk} estimate_device C", est, est.estimate_device(cu(K), cu(rgb3), cu(mask3), cu(E1), cu(rgb), cu(mask), cu(E2)))
                est.invalidate_features()
                put(f"{dt} cache={mode} chunk={chunk} after invalidate", est, est.estimate_device(cu(K), cu(rgb3), cu(mask3), cu(E1), cu(rgb), cu(mask), cu(E2)))
        for chunk in (32, 2):
            est = mk(hip_feature_cache="content", hip_feature_cache_records=2, hip_upload_chunk=chunk)
            put(f"{dt} cache=content records=2 chunk={chunk} (overflow)", est, est.estimate(K, frames["f64"](rgb), mask.astype(bool), E1, frames["f64"](rgb2), mask2.astype(bool), E2))
        # the controller's queue through the slot cache: three steps, an estimation after each
        est = mk(hip_feature_cache=True, hip_prepare_seed=1)
        ci = ControlInterface.queue_only(3, est, 5)
        for t in range(3):
            img, pose, _ = synth.control_view(3, t, seed=6)
            ci.add_view(img, pose)
            ci.accumulate_steps += 1
            put(f"{dt} ControlInterface.queue_only cache=True step {t}", est, ci.get_estimation())
        del net
    # the PnP tail (its own net: it reads the view-2 heads)
    est = AdaPoseEstimator_v5(None, dict(base, direct_regression=False, use_depth=False), None, state_dict=sd, dtype="bf16x3")
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        put("bf16x3 PnP branch", est, est.estimate(K, rgb, mask, E1, rgb2, mask2, E2))
    # AdaPoseNet variants, outputs of the network itself
    for name, B, kw in (("graph B=2", 2, dict(graph=True)), ("split_streams B=4", 4, dict(split_streams=True, split_min_batch=4)),
                        ("poison_workspace B=2", 2, dict(poison_workspace=True))):
        net = AdaPoseNet(sd, dtype="bf16x3", **kw)
        i = synth.adapose_inputs(B, seed=3)
        for rep in range(2):
            pred = net(i["img1"], i["choose1"], i["img2"], i["choose2"], i["P1"], i["P2"], i["depths"])
            for k, v in pred.items():
                out[f"AdaPoseNet {name} run {rep} {k}"] = v.cpu().numpy()
    net = AdaPoseNet(sd, dtype="bf16x3", poison_workspace=True, options={"view2_heads": 0})
    est = AdaPoseEstimator_v5(None, dict(base, hip_feature_cache="content"), None, dtype="bf16x3", net=net)
    put("bf16x3 poison_workspace cache=content", est, est.estimate(K, rgb, mask, E1, rgb2, mask2, E2))
    del net, est
    dense(out)
    torch.cuda.synchronize()
    np.savez(path, **out)
    print(f"{len(out)} arrays -> {path}")


def dense(out):
    """Every array of the four dense dicts — estimate_depth, estimate_cloud, estimate_cloud_pose(fit_seed) and estimate_cloud_views(fit=True,
    V = 3) — on the five poses, max_points 4096, at hip_upload frames / windows x hip_upload_chunk 32 / 2 (the views call: frames only),
    with hip_feature_cache: "content" set so that the bypass counter moves; the two counters after each call."""
    from rgbmanip_amd import synth
    from rgbmanip_amd.adapose import AdaPoseNet
    from rgbmanip_amd.config import ADAPOSE_CFGS
    from rgbmanip_amd.estimator import AdaPoseEstimator_v5
    rgb, mask, K = case()
    u8 = np.clip(np.rint(rgb * 255.0), 0, 255).astype(np.uint8)
    views = [(u8, mask), (np.ascontiguousarray(u8[:, :, ::-1]), np.ascontiguousarray(mask[:, :, ::-1])),
             (np.ascontiguousarray(u8[:, ::-1]), np.ascontiguousarray(mask[:, ::-1]))]
    i1, i2 = synth.adapose_inputs(len(rgb), seed=2), synth.adapose_inputs(len(rgb), seed=4)
    E = [i1["E1"].astype(np.float64), i1["E2"].astype(np.float64), i2["E2"].astype(np.float64)]
    net = AdaPoseNet(synth.adapose_state_dict(seed=0, prefix="module."), dtype="bf16x3", options={"view2_heads": 1})
    base = dict(ADAPOSE_CFGS["adapose_cabinet"], load=False, hip_prepare="device", hip_prepare_seed=9, hip_view2_heads=True,
                hip_feature_cache="content")
    pair = (K, views[0][0], views[0][1], E[0], views[1][0], views[1][1], E[1])
    for upload in ("frames", "windows"):
        for chunk in (32, 2):
            est = AdaPoseEstimator_v5(None, dict(base, hip_upload=upload, hip_upload_chunk=chunk), None, dtype="bf16x3", net=net)
            calls = [("estimate_depth", lambda: est.estimate_depth(*pair)), ("estimate_cloud", lambda: est.estimate_cloud(*pair, max_points=4096)),
                     ("estimate_cloud_pose", lambda: est.estimate_cloud_pose(*pair, max_points=4096, fit_seed=5))]
            if upload == "frames":
                calls.append(("estimate_cloud_views", lambda: est.estimate_cloud_views(
                    K, np.stack([v[0] for v in views], axis=1), np.stack([v[1] for v in views], axis=1), np.stack(E, axis=1), max_points=4096,
                    fit=True, fit_seed=5)))
            for name, call in calls:
                tag = f"dense {name} upload={upload} chunk={chunk}"
                for k, v in call().items():
                    out[f"{tag} {k}"] = np.asarray(v)
                out[tag + "|counters"] = np.array([est.feature_views_computed, est.feature_cache_bypassed])


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if sys.argv[1] == "--dense":                      # the dense calls alone
        arrays = {}
        dense(arrays)
        np.savez(sys.argv[2], **arrays)
        print(f"{len(arrays)} arrays -> {sys.argv[2]}")
    else:
        main(sys.argv[1])
