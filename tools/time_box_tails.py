#!/usr/bin/env python3
"""Time the two `direct_regression: True` box tails on the device: v5's pair-median tail (`rgbmanip_amd.adapose.postprocess`, with the
scratch that small batches slice the search over) and v4's regressed tail (`postprocess_regressed`), at B = 1 and B = 256.

The two are called alternately in one process, each call between two events on an otherwise idle stream, and the medians over the
rounds are printed, so clock and thermal state are shared.  Usage: python tools/time_box_tails.py [rounds]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rgbmanip_amd import synth  # noqa: E402
from rgbmanip_amd.adapose import postprocess, postprocess_regressed  # noqa: E402


def main(rounds=200):
    g = np.random.default_rng(0)
    for B in (1, 256):
        inp = synth.adapose_inputs(2, seed=0)
        rep = lambda x: torch.from_numpy(np.ascontiguousarray(np.resize(x, (B,) + x.shape[1:]))).cuda()      # noqa: E731
        nocs = torch.from_numpy(g.uniform(-0.45, 0.45, (B, 1024, 3)).astype(np.float32)).cuda()
        depth = torch.from_numpy(g.uniform(0.5, 0.8, (B, 1024)).astype(np.float32)).cuda()
        r = torch.from_numpy(np.stack([np.linalg.qr(g.normal(size=(3, 3)))[0] for _ in range(B)]).astype(np.float32)).cuda()
        t = torch.from_numpy(g.normal(0, 0.3, (B, 3)).astype(np.float32)).cuda()
        s = torch.from_numpy(g.normal(0, 0.3, (B, 3)).astype(np.float32)).cuda()
        choose, K, E = rep(inp["choose1"]).to(torch.int32), rep(inp["K1"]).double(), rep(inp["E1"]).double()
        calls = {"v5 median tail": lambda: postprocess(nocs, depth, r, choose, K, E),
                 "v4 regressed tail": lambda: postprocess_regressed(nocs, r, t, s, E)}
        times = {k: [] for k in calls}
        for i in range(rounds + 20):
            for name, fn in calls.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                if i >= 20:
                    times[name].append(a.elapsed_time(b))
        for name, v in times.items():
            v = np.sort(v)
            print(f"B = {B:3d}  {name:18s} median {np.median(v) * 1e3:8.1f} us   p10 {v[len(v) // 10] * 1e3:8.1f}   p90 {v[9 * len(v) // 10] * 1e3:8.1f}   ({len(v)} rounds)")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 200)
