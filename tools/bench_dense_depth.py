#!/usr/bin/env python3
"""A/B of `AdaPoseNet.forward` against `forward(dense_depth=True)` (DESIGN.md "Dense depth maps") at B = 8 and B = 256 in bf16 and
bf16x3, on seeded weights and inputs.  Three legs per (dtype, B), timed alternately with device events:

  default      forward() of a default net (sparse cost regularisation, sparse tail)
  dense_opts   forward() of a net built with sparse_dec = 0 and the dense tail: every 3-D layer and conv11 computed densely — the
               `value_dense` leg of bench.py plus the dense conv11.  This is the honest base of the dense call.
  dense_call   forward(dense_depth=True) of the default net = dense_opts + the dense head kernel

The dense head's own time is reported as dense_call - dense_opts (the two run the same launches but for that kernel) and its rate as
the bytes the algorithm needs (u11 read once + both maps written) over that time; `--kernel-only` runs just dense calls, for a
`rocprofv3 --kernel-trace --stats` run that reads dense_depth_kernel's time directly.  Prints one JSON line per (dtype, B).

    python tools/bench_dense_depth.py [--batches 8 256] [--dtypes bf16 bf16x3] [--steps 10] [--warmup 2]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rgbmanip_amd import synth  # noqa: E402
from rgbmanip_amd.adapose import AdaPoseNet  # noqa: E402

S, D, C = 224, 24, 8


def batch(B):
    """B poses: eight seeded pairs tiled (the kernels' time does not depend on the values)."""
    base = synth.adapose_inputs(min(B, 8), seed=0)
    reps = -(-B // min(B, 8))
    order = ("img1", "choose1", "img2", "choose2", "P1", "P2", "depths")
    dt = {"choose1": torch.int32, "choose2": torch.int32}
    return [torch.from_numpy(np.concatenate([base[k]] * reps)[:B]).cuda().to(dt.get(k, torch.float32)).contiguous() for k in order]


def time_alternating(fns, warmup, steps):
    """median ms per call of each fn, the fns taking turns inside every step"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 256])
    ap.add_argument("--dtypes", nargs="+", default=["bf16", "bf16x3"])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-only", action="store_true", help="dense calls only (for a kernel-trace run)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_dense_depth needs a GPU: no timing is taken without one")
    sd = synth.adapose_state_dict(seed=0, prefix="module.")
    for dtype in args.dtypes:
        es = 2 if dtype == "bf16" else 4
        default = AdaPoseNet(sd, dtype=dtype)
        dense_opts = None if args.kernel_only else AdaPoseNet(sd, dtype=dtype, sparse_tail=0, options={"sparse_dec": 0})
        for B in args.batches:
            x = batch(B)
            call = lambda: default(*x, dense_depth=True)      # noqa: E731
            if args.kernel_only:
                time_alternating([call], args.warmup, args.steps)
                continue
            (t_def, t_opts, t_call), spread = time_alternating([lambda: default(*x), lambda: dense_opts(*x), call], args.warmup, args.steps)
            out = call()
            at = out["view1_depth_map"].flatten(1).gather(1, x[1].long())
            V = 2 * B
            bytes_algo = V * D * S * S * C * es + 2 * V * S * S * 4
            k_ms = t_call - t_opts
            print(json.dumps({"dtype": dtype, "B": B, "steps": args.steps, "warmup": args.warmup,
                              "ms_default_forward": round(t_def, 3), "ms_dense_options_forward": round(t_opts, 3), "ms_dense_call": round(t_call, 3),
                              "ms_spread_max_minus_min": [round(s, 3) for s in spread],
                              "ms_dense_head_by_difference": round(k_ms, 3), "dense_head_algorithmic_GB": round(bytes_algo / 1e9, 3),
                              "dense_head_GBps_by_difference": round(bytes_algo / 1e6 / k_ms, 1) if k_ms > 0 else None,
                              "ms_dense_options_forward_plus_head": round(t_opts + k_ms, 3),
                              "map_at_choose_equals_point_depth": bool(torch.equal(at, out["view1_depth"]))}), flush=True)
            del x, out
            default._ws = dense_opts._ws = None
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
