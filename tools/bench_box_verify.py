#!/usr/bin/env python3
"""Times the box verification kernels: `rgbm_box_silhouette` at 256 poses x V = 2 views of 480 x 640 with the
synthetic camera's masks for S = 1, 8 and 64 hypotheses per pose (the ground-truth box and copies of it moved by a few centimetres, like
the dropout draws of a pose), and `rgbm_cloud_in_box` at 256 poses x cap = 100 352 rows for S = 2 and 64.  The legs take turns in blocks
in one process (device events around the C call, outputs and scratch allocated beforehand; per leg the median of its blocks' medians
and their spread).  Beside them: `rgbm_microbench_copy` over the same bytes in the same run (the floor of the silhouette is its 157 MB
of masks read once, of the cloud its rows read once), and the numpy twins on a slice of the poses, extrapolated to 256 and labelled so.

    python tools/bench_box_verify.py [--poses 256] [--blocks 5] [--calls 5] [--out profiles/box_verify_ab.txt]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rgbmanip_amd import _lib, synthetic_env, verify  # noqa: E402

CAP = 100352                      # 2 x 224 x 224, the default cap of estimate_cloud


def scene(n):
    """K [n,3,3], E [n,2,4,4], masks [n,2,480,640] u8 of the synthetic hand camera from two poses, and the ground-truth corners [n,8,3]."""
    env = synthetic_env.SyntheticMultiVecEnv(n, "cuda", seed=0)
    views = []
    for dy in (-0.12, 0.12):
        env._cam[:, :3] = torch.tensor([0.25, dy, 0.75], dtype=torch.float64, device="cuda")
        head = env._box[:, :3] - (env._robot[:, :3] + env._cam[:, :3])
        # the camera's x axis along `head`: yaw and pitch as a quaternion (w, x, y, z)
        yaw, pitch = torch.atan2(head[:, 1], head[:, 0]), -torch.atan2(head[:, 2], head[:, :2].norm(dim=1))
        cy, sy, cp, sp = torch.cos(yaw / 2), torch.sin(yaw / 2), torch.cos(pitch / 2), torch.sin(pitch / 2)
        env._cam[:, 3:] = torch.stack([cy * cp, -sy * sp, cy * sp, sy * cp], 1)
        img = env.get_image()["camera0"]
        views.append((img["Intrinsic"], img["Extrinsic"], img["Mask"]))
    truth = env.get_observation(gt=True)["handle_bbox"]
    return views[0][0], torch.stack([v[1] for v in views], 1).contiguous(), torch.stack([v[2] for v in views], 1).contiguous(), truth


def hypotheses(truth, S, rng):
    """[n,S,8,3]: the ground truth at index 0, then copies moved by up to 4 cm"""
    n = truth.shape[0]
    shift = torch.from_numpy(rng.uniform(-0.04, 0.04, (n, S, 1, 3))).cuda()
    shift[:, 0] = 0
    return (truth[:, None] + shift).contiguous()


def block_ms(fn, calls):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(calls + 1)]
    ev[0].record()
    for i in range(calls):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return float(np.median([ev[i].elapsed_time(ev[i + 1]) for i in range(calls)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--twin-poses", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_verify_ab.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_box_verify needs a GPU: no timing is taken without one")
    lib = _lib.load()
    st = _lib.stream_ptr()
    rng = np.random.default_rng(0)
    n, V, H, W = args.poses, 2, synthetic_env.CAM_H, synthetic_env.CAM_W
    K, E, masks, truth = scene(n)
    Kv = K[:, None].expand(n, V, 3, 3).contiguous()
    mask_bytes = masks.numel()
    legs, info = {}, {}

    for S in (1, 8, 64):
        boxes = hypotheses(truth, S, rng)
        out = [torch.empty(*shp, dtype=torch.int32, device="cuda") for shp in ((n, S, V), (n, S, V), (n, V), (n, S, V, 4), (n, S, V))]
        need = C.c_size_t(0)
        _lib.check(lib.rgbm_box_silhouette_scratch_bytes(n, S, V, C.byref(need)), "scratch_bytes")
        scratch = torch.empty((need.value + 7) // 8, dtype=torch.float64, device="cuda")
        legs[f"box_silhouette S={S}"] = (lambda b=boxes, o=out, sc=scratch, S=S: _lib.check(lib.rgbm_box_silhouette(
            _lib.ptr(b), None, _lib.ptr(Kv), _lib.ptr(E), _lib.ptr(masks), n, S, V, H, W, *[_lib.ptr(x) for x in o], _lib.ptr(sc), sc.numel() * 8, st),
            "rgbm_box_silhouette"))
        info[f"box_silhouette S={S}"] = dict(bytes=mask_bytes, boxes=boxes, out=out)
    dst = torch.empty_like(masks)
    legs["microbench_copy masks"] = lambda: _lib.check(lib.rgbm_microbench_copy(_lib.ptr(masks), _lib.ptr(dst), mask_bytes, st), "copy")
    info["microbench_copy masks"] = dict(bytes=2 * mask_bytes)

    centre = truth.mean(dim=1)
    cloud = (centre[:, None] + torch.from_numpy(rng.normal(0, 0.05, (n, CAP, 3))).cuda()).to(torch.float32).contiguous()
    count = torch.full((n, 2), CAP // 2, dtype=torch.int32, device="cuda")
    cloud_bytes = cloud.numel() * 4
    for S in (2, 64):
        boxes = hypotheses(truth, S, rng)
        inside, total = torch.empty(n, S, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
        legs[f"cloud_in_box S={S}"] = (lambda b=boxes, i=inside, t=total, S=S: _lib.check(lib.rgbm_cloud_in_box(
            _lib.ptr(cloud), _lib.ptr(count), 2, _lib.ptr(b), None, n, S, CAP, 0.02, _lib.ptr(i), _lib.ptr(t), st), "rgbm_cloud_in_box"))
        info[f"cloud_in_box S={S}"] = dict(bytes=cloud_bytes, boxes=boxes, inside=inside)
    cdst = torch.empty_like(cloud)
    legs["microbench_copy cloud"] = lambda: _lib.check(lib.rgbm_microbench_copy(_lib.ptr(cloud), _lib.ptr(cdst), cloud_bytes, st), "copy")
    info["microbench_copy cloud"] = dict(bytes=2 * cloud_bytes)

    for fn in legs.values():                      # warm
        fn()
    torch.cuda.synchronize()
    meds = {k: [] for k in legs}
    for _ in range(args.blocks):                  # the legs take turns
        for k, fn in legs.items():
            meds[k].append(block_ms(fn, args.calls))
    lines = [f"# tools/bench_box_verify.py: {n} poses, V = {V}, {H} x {W} masks of the synthetic camera ({mask_bytes / 1e6:.1f} MB), cloud cap {CAP} "
             f"({cloud_bytes / 1e6:.1f} MB); device events around the C call, {args.blocks} alternating blocks of {args.calls} calls",
             f"{'leg':<26} {'ms: median of block medians (min .. max)':>44} {'GB/s':>9}   note"]
    res = {}
    for k, v in meds.items():
        med = float(np.median(v))
        res[k] = med
        note = "bytes read + written" if k.startswith("microbench") else "bytes of the floor (masks / rows read once)"
        lines.append(f"{k:<26} {med:>24.3f} ({min(v):.3f} .. {max(v):.3f}) {info[k]['bytes'] / med / 1e6:>9.1f}   {note}")
    s1, s8, s64 = (res[f"box_silhouette S={S}"] for S in (1, 8, 64))
    lines.append(f"# box_silhouette: S = 64 costs {s64 / s1:.2f} x S = 1 (64 launches of S = 1 would cost 64 x), S = 8 costs {s8 / s1:.2f} x; "
                 f"cloud_in_box: S = 64 costs {res['cloud_in_box S=64'] / res['cloud_in_box S=2']:.2f} x S = 2")
    sil = info["box_silhouette S=64"]["out"]
    lines.append(f"# mean silhouette pixels per box and view {float(sil[0].double().mean()):.0f}, mean mask pixels {float(sil[2].double().mean()):.0f}, "
                 f"ground-truth box: mean |silhouette - mask| {float((sil[0][:, 0] + sil[2] - 2 * sil[1][:, 0]).double().mean()):.2f} pixels; "
                 f"cloud rows inside the ground-truth box at inflate 0.02: {float(info['cloud_in_box S=64']['inside'][:, 0].double().mean()):.0f} of {CAP}")
    # the numpy twins on a slice of the poses, extrapolated
    m = min(args.twin_poses, n)
    hm, hK, hE = masks[:m].cpu().numpy(), K[:m].cpu().numpy(), E[:m].cpu().numpy()
    for S in (1, 8):
        hb = info[f"box_silhouette S={S}"]["boxes"][:m].cpu().numpy()
        t0 = time.perf_counter()
        ref = verify.box_silhouette_ref(hb, hK, hE, hm)
        dt = (time.perf_counter() - t0) * 1e3
        same = all(np.array_equal(ref[key], info[f"box_silhouette S={S}"]["out"][j][:m].cpu().numpy()) for j, key in enumerate(verify.INT_KEYS))
        lines.append(f"{'box_silhouette_ref S=' + str(S):<26} {dt * n / m:>24.1f} ms for {n} poses, EXTRAPOLATED from {dt:.1f} ms for {m} poses (numpy twin, host); "
                     f"integer outputs equal to the kernel's: {same}")
    hb = info["cloud_in_box S=2"]["boxes"][:m].cpu().numpy()
    t0 = time.perf_counter()
    ref = verify.cloud_in_box_ref(cloud[:m].cpu().numpy(), count[:m].cpu().numpy(), hb, inflate=0.02)
    dt = (time.perf_counter() - t0) * 1e3
    same = np.array_equal(ref["inside"], info["cloud_in_box S=2"]["inside"][:m].cpu().numpy())
    lines.append(f"{'cloud_in_box_ref S=2':<26} {dt * n / m:>24.1f} ms for {n} poses, EXTRAPOLATED from {dt:.1f} ms for {m} poses (numpy twin, host); "
                 f"counts equal to the kernel's: {same}")
    for ln in lines:
        print(ln, flush=True)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
