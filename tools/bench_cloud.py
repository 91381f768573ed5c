#!/usr/bin/env python3
"""A/B of `AdaPoseEstimator_v5.estimate_cloud_device` against `estimate_depth_device` at 8 and 256 poses, bf16
net with the view-2 heads, uint8 frames that live on the device.  The two calls take turns inside every step and are timed with device
events; the difference is what the two consistency checks, the compaction and the handling of the view-2 maps cost on top of the dense
call.  Prints one JSON line per pose count.

    python tools/bench_cloud.py [--poses 8 256] [--steps 10] [--warmup 2]
    python tools/bench_cloud.py --kernel-only      # cloud calls only, for `rocprofv3 --kernel-trace --stats -- python tools/bench_cloud.py
                                                   # --kernel-only`: depth_consistency_kernel's and cloud_pack_kernel's own times
    python tools/bench_cloud.py --trace-csv FILE   # per-kernel, per-grid times of the two kernels from that run's kernel_trace.csv

On a commit without `estimate_cloud_device` only the `estimate_depth_device` leg runs (the same-tool comparison with the parent commit).
"""
import argparse
import collections
import csv
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

S, H, W = 224, 480, 640
COPY_PROBE_TBPS = 4.57      # profiles/README.md


def frames(n):
    """n poses of uint8 device frames with elliptical masks: eight seeded poses tiled (the kernels' time does not depend on the values)."""
    from rgbmanip_amd import synth
    g = np.random.default_rng(3)
    m = min(n, 8)
    yy, xx = np.mgrid[0:H, 0:W]
    base = synth.adapose_inputs(m, seed=0)
    K = np.tile(np.array([[439.31, 0, 320.0], [0, 439.31, 240.0], [0, 0, 1.0]])[None], (m, 1, 1))
    u1, u2 = (g.integers(0, 256, (m, H, W, 3), dtype=np.uint8) for _ in range(2))
    m1 = np.stack([((yy - 240) / 60.0) ** 2 + ((xx - 300 - 10 * i) / 90.0) ** 2 <= 1 for i in range(m)]).astype(np.uint8)
    m2 = np.stack([((yy - 250) / 70.0) ** 2 + ((xx - 340 + 10 * i) / 80.0) ** 2 <= 1 for i in range(m)]).astype(np.uint8)
    reps = -(-n // m)
    tile = lambda a: torch.from_numpy(np.concatenate([a] * reps)[:n]).cuda()      # noqa: E731
    return tuple(tile(a) for a in (K, u1, m1, base["E1"].astype(np.float64), u2, m2, base["E2"].astype(np.float64)))


def time_alternating(fns, warmup, steps):
    """median ms per call of each fn and its max - min, the fns taking turns inside every step"""
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(steps):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b))
    return [float(np.median(m)) for m in ms], [float(np.max(m) - np.min(m)) for m in ms]


def kernel_bytes(n):
    """Bytes the two kernels need at n poses (default capacity 2 S S, thresholds that keep a share k of the pixels: the cloud rows are
    written whatever k is — a kept row or a NaN row)."""
    px = n * S * S
    check = px * (4 + 4 + 1 + 4 + 4 * 3 + 1)      # depth_a, conf_a, mask_a, one pass over depth_b; fused, reproj, rel, keep
    pack = 2 * px * (1 + 12 + 4)                    # keep once (the eight counting passes hit L2); 12-byte row + 4-byte index per slot
    return check, pack


def summarize_trace(path):
    rows = list(csv.DictReader(open(path)))
    agg = collections.OrderedDict()
    for r in rows:
        name = r["Kernel_Name"]
        if "depth_consistency_kernel" not in name and "cloud_pack_kernel" not in name:
            continue
        key = (name.split("(")[0][-40:], r.get("Grid_Size_Y", r.get("Grid_Size", "")))
        agg.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for key, us in agg.items():
        print(key, f"n={len(us)} median_us={np.median(us):.1f} min_us={min(us):.1f} max_us={max(us):.1f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, nargs="+", default=[8, 256])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-only", action="store_true", help="cloud calls only (for a kernel-trace run)")
    ap.add_argument("--trace-csv", help="summarise the two kernels' dispatches of a rocprofv3 kernel_trace.csv and exit")
    args = ap.parse_args()
    if args.trace_csv:
        return summarize_trace(args.trace_csv)
    if not torch.cuda.is_available():
        sys.exit("bench_cloud needs a GPU: no timing is taken without one")
    from rgbmanip_amd import synth
    from rgbmanip_amd.adapose import AdaPoseNet
    from rgbmanip_amd.config import ADAPOSE_CFGS
    from rgbmanip_amd.estimator import AdaPoseEstimator_v5
    net = AdaPoseNet(synth.adapose_state_dict(seed=0, prefix="module."), dtype="bf16", options={"view2_heads": 1})
    cfg = dict(ADAPOSE_CFGS["adapose_cabinet"], load=False, hip_dtype="bf16", hip_prepare="device", hip_prepare_seed=9, hip_view2_heads=True)
    est = AdaPoseEstimator_v5(None, cfg, None, net=net)
    has_cloud = hasattr(est, "estimate_cloud_device")
    loose = dict(px_max=60.0, rel_max=0.5, conf_min=0.05)      # seeded weights: the two maps are unrelated, the default thresholds keep nothing
    for n in args.poses:
        x = frames(n)
        depth = lambda: est.estimate_depth_device(*x)      # noqa: E731
        cloud = (lambda: est.estimate_cloud_device(*x, **loose)) if has_cloud else None
        if args.kernel_only:
            time_alternating([cloud], args.warmup, args.steps)
            continue
        fns = [depth, cloud] if has_cloud else [depth]
        ms, spread = time_alternating(fns, args.warmup, args.steps)
        rec = {"poses": n, "steps": args.steps, "warmup": args.warmup, "ms_estimate_depth_device": round(ms[0], 3),
               "ms_spread_max_minus_min": [round(s, 3) for s in spread]}
        if has_cloud:
            r = cloud()
            check, pack = kernel_bytes(n)
            rec.update(ms_estimate_cloud_device=round(ms[1], 3), ms_cloud_minus_depth=round(ms[1] - ms[0], 3),
                       kept_share=round(float(r["count"].sum()) / (2 * n * S * S), 4),
                       check_MB_per_launch=round(check / 1e6, 2), check_us_at_copy_probe=round(check / COPY_PROBE_TBPS / 1e6, 1),
                       pack_MB=round(pack / 1e6, 2), pack_us_at_copy_probe=round(pack / COPY_PROBE_TBPS / 1e6, 1))
            del r
        print(json.dumps(rec), flush=True)
        del x
        net._ws = None
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
