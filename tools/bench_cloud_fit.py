#!/usr/bin/env python3
"""The dense NOCS map and the fit over the two-view cloud at 8 and 256 poses: the three kernels on their own
(`nocs_map` on an fp32 feature array of 2 n crops, `cloud_gather` and `cloud_similarity` on a full-capacity cloud of planted
similarities with 20 % outliers), and `AdaPoseEstimator_v5.estimate_cloud_pose_device` against `estimate_cloud_device` on a bf16 net
with the view-2 heads and uint8 device frames, the two calls taking turns inside every step.  Device events; one JSON line per pose
count.

    python tools/bench_cloud_fit.py [--poses 8 256] [--steps 10] [--warmup 2]
    python tools/bench_cloud_fit.py --kernel-only    # the pose calls only, for `rocprofv3 --kernel-trace --stats -- python
                                                     # tools/bench_cloud_fit.py --kernel-only`
    python tools/bench_cloud_fit.py --trace-csv FILE # per-kernel, per-grid times of that run's kernel_trace.csv: dense_nocs_kernel beside
                                                     # point_mlp_kernel (the yardstick: time per pixel against time per point), the gather
                                                     # and the eight kernels of the fit

On a commit without `estimate_cloud_pose_device` only the `estimate_cloud_device` leg runs (the same-tool comparison with the parent).
"""
import argparse
import collections
import csv
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_cloud import S, frames, time_alternating  # noqa: E402

KERNELS = ("dense_nocs_kernel", "point_mlp_kernel", "cloud_gather_kernel", "cf_sum_kernel", "cf_far_kernel", "cf_hypotheses_kernel",
           "cf_count_kernel", "cf_scan_kernel", "cf_inlier_sum_kernel", "cf_inlier_cov_kernel", "cf_finish_kernel")
MAP_FLOP_PER_PIXEL = 2 * (32 * 64 + 64 * 128 + 128 * 64 + 64 * 16)      # the four layers as the kernel runs them (layer 3 on a 16-channel tile)


def summarize_trace(path):
    rows = list(csv.DictReader(open(path)))
    agg = collections.OrderedDict()
    for r in rows:
        name = r["Kernel_Name"]
        hit = [k for k in KERNELS if k in name]
        if not hit:
            continue
        key = (hit[0], r.get("Grid_Size_X", r.get("Grid_Size", "")), r.get("Grid_Size_Y", ""))
        agg.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for key, us in agg.items():
        print(key, f"n={len(us)} median_us={np.median(us):.1f} min_us={min(us):.1f} max_us={max(us):.1f}")


def planted_cloud(n, cap):
    """n poses of cap rows: cloud = s R nocs + t with noise, 20 % of the rows replaced (device tensors; eight seeded poses tiled)."""
    g = np.random.default_rng(11)
    m = min(n, 8)
    nocs = g.uniform(-0.45, 0.45, (m, cap, 3))
    cloud = np.empty_like(nocs)
    for i in range(m):
        q, _ = np.linalg.qr(g.normal(size=(3, 3)))
        q *= np.sign(np.linalg.det(q))
        s = g.uniform(0.1, 0.4)
        cloud[i] = s * nocs[i] @ q.T + g.normal(0, 0.5, 3) + g.normal(0, 0.002 * s, (cap, 3))
        bad = g.random(cap) < 0.2
        nocs[i][bad] = g.uniform(-0.5, 0.5, (int(bad.sum()), 3))
    reps = -(-n // m)
    tile = lambda a: torch.from_numpy(np.concatenate([a] * reps)[:n].astype(np.float32)).cuda()      # noqa: E731
    count = torch.tensor([[cap // 2, cap - cap // 2]] * n, dtype=torch.int32, device="cuda")
    return tile(nocs), tile(cloud), count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, nargs="+", default=[8, 256])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-only", action="store_true", help="pose calls only (for a kernel-trace run)")
    ap.add_argument("--trace-csv", help="summarise the kernels' dispatches of a rocprofv3 kernel_trace.csv and exit")
    args = ap.parse_args()
    if args.trace_csv:
        return summarize_trace(args.trace_csv)
    if not torch.cuda.is_available():
        sys.exit("bench_cloud_fit needs a GPU: no timing is taken without one")
    from rgbmanip_amd import adapose, synth
    from rgbmanip_amd.adapose import AdaPoseNet
    from rgbmanip_amd.config import ADAPOSE_CFGS
    from rgbmanip_amd.estimator import AdaPoseEstimator_v5
    net = AdaPoseNet(synth.adapose_state_dict(seed=0, prefix="module."), dtype="bf16", options={"view2_heads": 1})
    cfg = dict(ADAPOSE_CFGS["adapose_cabinet"], load=False, hip_dtype="bf16", hip_prepare="device", hip_prepare_seed=9, hip_view2_heads=True)
    est = AdaPoseEstimator_v5(None, cfg, None, net=net)
    has_pose = hasattr(est, "estimate_cloud_pose_device")
    loose = dict(px_max=60.0, rel_max=0.5, conf_min=0.05)      # seeded weights: the two maps are unrelated, the default thresholds keep nothing
    cap = 2 * S * S
    for n in args.poses:
        x = frames(n)
        cloud = lambda: est.estimate_cloud_device(*x, **loose)      # noqa: E731
        pose = (lambda: est.estimate_cloud_pose_device(*x, **loose)) if has_pose else None
        if args.kernel_only:
            time_alternating([pose or cloud], args.warmup, args.steps)
            continue
        ms, spread = time_alternating([cloud, pose] if has_pose else [cloud], args.warmup, args.steps)
        rec = {"poses": n, "steps": args.steps, "warmup": args.warmup, "ms_estimate_cloud_device": round(ms[0], 3),
               "ms_spread_max_minus_min": [round(s, 3) for s in spread]}
        if has_pose:
            r = pose()
            used = r["fit_info"][:, 0].double()
            rec.update(ms_estimate_cloud_pose_device=round(ms[1], 3), ms_pose_minus_cloud=round(ms[1] - ms[0], 3),
                       cloud_rows_share_of_pixels=round(float(used.sum()) / (2 * n * S * S), 4), valid_cloud=int(r["valid_cloud"].sum()))
            del r
            # the three kernels on their own
            feat = torch.randn(2 * n, S * S, 32, device="cuda")
            maps = net.nocs_map(feat)
            index = torch.randint(-1, 2 * S * S, (n, cap), dtype=torch.int32, device="cuda")
            nocs, cl, count = planted_cloud(n, cap)
            k_ms, k_sp = time_alternating([lambda: net.nocs_map(feat), lambda: adapose.cloud_gather(maps[:n], maps[n:], index),
                                           lambda: adapose.cloud_similarity(nocs, cl, count, seed=1)], args.warmup, args.steps)
            px = 2 * n * S * S
            rec.update(ms_nocs_map=round(k_ms[0], 3), ns_nocs_map_per_pixel=round(k_ms[0] * 1e6 / px, 3),
                       nocs_map_tflops=round(MAP_FLOP_PER_PIXEL * px / (k_ms[0] * 1e-3) / 1e12, 1), ms_cloud_gather=round(k_ms[1], 3),
                       ms_cloud_similarity=round(k_ms[2], 3), ms_kernel_spread=[round(s, 3) for s in k_sp])
            del feat, maps, index, nocs, cl, count
        print(json.dumps(rec), flush=True)
        del x
        net._ws = None
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
