#!/usr/bin/env python3
"""A/B of S Dropout2d samples per pose: S consecutive `AdaPoseNet.forward` calls of B poses (block A: what a
caller had to do before `forward_samples`, the forward's code unchanged) against one `forward_samples(.., samples=S)` (block B), on
seeded weights and inputs, in bf16x3 with `hip_dropout: 0.15` and with `hip_as_shipped` (per-sample BatchNorm3d + Dropout2d 0.15).
The two blocks take turns inside every step of one process and are timed with device events; the first step's inputs are uploaded
once, outside the timed window, for both.  Writes one table row per (mode, B, S) and prints one JSON line each.

    python tools/bench_dropout_samples.py [--shapes 1x8 1x16 8x8] [--modes dropout as_shipped] [--steps 20] [--warmup 3]
                                          [--out profiles/dropout_samples_ab.txt]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rgbmanip_amd import synth  # noqa: E402
from rgbmanip_amd.adapose import AdaPoseNet  # noqa: E402

MODES = {"dropout": dict(norm_mode=0), "as_shipped": dict(norm_mode=1)}
ORDER = ("img1", "choose1", "img2", "choose2", "P1", "P2", "depths")


def batch(B):
    base = synth.adapose_inputs(B, seed=0)
    dt = {"choose1": torch.int32, "choose2": torch.int32}
    return [torch.from_numpy(base[k]).cuda().to(dt.get(k, torch.float32)).contiguous() for k in ORDER]


def time_alternating(fns, warmup, steps):
    """per fn: (median, min, max) ms per call, the fns taking turns inside every step"""
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
    return [(float(np.median(m)), float(np.min(m)), float(np.max(m))) for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["1x8", "1x16", "8x8"], help="BxS: poses x samples")
    ap.add_argument("--modes", nargs="+", default=list(MODES), choices=list(MODES))
    ap.add_argument("--dtype", default="bf16x3")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dropout_samples_ab.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_dropout_samples needs a GPU: no timing is taken without one")
    sd = synth.adapose_state_dict(seed=0, prefix="module.")
    lines = [f"# tools/bench_dropout_samples.py: {args.dtype}, Dropout2d p = 0.15, view2_heads = 0 (what the estimator runs); steps {args.steps}, "
             f"warmup {args.warmup}; blocks alternate in one process, device events",
             "# A = S consecutive forward() calls of B poses; B = one forward_samples(samples = S); ms per block: median (min .. max)",
             f"{'mode':<11} {'B':>3} {'S':>3} {'A ms':>26} {'B ms':>26} {'A / B':>7} {'ms per sample A':>16} {'ms per sample B':>16}"]
    for mode in args.modes:
        net = AdaPoseNet(sd, dtype=args.dtype, dropout=0.15, dropout_seed=0, options={"view2_heads": 0}, **MODES[mode])
        for shape in args.shapes:
            B, S = (int(v) for v in shape.lower().split("x"))
            x = batch(B)

            def block_a():
                for _ in range(S):
                    net(*x)

            def block_b():
                net.forward_samples(*x, samples=S)
            (a, b) = time_alternating([block_a, block_b], args.warmup, args.steps)
            # the same masks give the same numbers (to the rounding between the GEMM tiles of 2B and 2SB views): sample 0 of a fresh sequence
            net.set_dropout(0.15, 0)
            one = net(*x)["view1_nocs"].clone()
            net.set_dropout(0.15, 0)
            many = net.forward_samples(*x, samples=S)["view1_nocs"][0]
            rel = float((one - many).abs().max() / one.abs().max())
            row = {"mode": mode, "dtype": args.dtype, "B": B, "S": S, "steps": args.steps, "warmup": args.warmup,
                   "ms_A_S_forwards": [round(v, 3) for v in a], "ms_B_forward_samples": [round(v, 3) for v in b],
                   "A_over_B_median": round(a[0] / b[0], 3), "sample0_rel_diff_A_vs_B": rel}
            print(json.dumps(row), flush=True)
            fmt = lambda t: f"{t[0]:8.3f} ({t[1]:.3f} .. {t[2]:.3f})"      # noqa: E731
            lines.append(f"{mode:<11} {B:>3} {S:>3} {fmt(a):>26} {fmt(b):>26} {a[0] / b[0]:>7.2f} {a[0] / S:>16.3f} {b[0] / S:>16.3f}")
            del x
            net._ws = None
            torch.cuda.empty_cache()
        net.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
