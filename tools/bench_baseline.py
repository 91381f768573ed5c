#!/usr/bin/env python3
"""The baseline network's attention stack and forward against what they replace, on one MI355X, in one process.

  1. rgbm_view_fusion against the same four blocks composed from torch.matmul / torch.softmax on the GPU (which writes and re-reads a
     [B, 4, P, P] fp32 score tensor per attention), same weights, same rows; the two outputs are compared too.
  2. The baseline forward + the direct-regression box tail against the v5 forward + the same tail, per storage type (bf16, bf16x3),
     view2_heads = 0 (what `estimate` consumes), the two taking turns inside every step.
  3. Both at B = 256, 8 and 1.

Device events on the current stream; per leg the median of --steps steps after --warmup warm-up steps of every shape, "spread" = max - min.
The box's bare-MFMA probe (bench.achievable_peaks) is printed beside the numbers.  Prints one JSON line per measurement; with --out the
same lines go to that file (profiles/baseline_ab.txt is the recorded run).

usage: python tools/bench_baseline.py [--steps 10] [--warmup 3] [--batches 256,8,1] [--out FILE]"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rgbmanip_amd import _lib, synth  # noqa: E402
from rgbmanip_amd.adapose import AdaPoseNet, postprocess  # noqa: E402


def timed(legs, steps, warmup):
    """legs: list of callables taking turns inside every step -> per leg (median ms, max - min ms)."""
    for _ in range(warmup):
        for f in legs:
            f()
    torch.cuda.synchronize()
    ms = [[] for _ in legs]
    for _ in range(steps):
        for i, f in enumerate(legs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ms[i].append(e0.elapsed_time(e1))
    return [(float(np.median(m)), float(max(m) - min(m))) for m in ms]


def torch_stack(w, x1, x2):
    """The four blocks from matmuls and a softmax (lib/fusion.py's arithmetic), rows [B, P, 32]."""
    B, P, _ = x1.shape

    def attend(xq, xkv, p):
        lin = lambda i, x: torch.addmm(w[f"{p}.linears.{i}.bias"], x.reshape(-1, 32), w[f"{p}.linears.{i}.weight"].t()).view(B, P, 32)
        q, k, v = (lin(i, x).view(B, P, 4, 8).transpose(1, 2) for i, x in ((0, xq), (1, xkv), (2, xkv)))
        pr = torch.softmax(torch.matmul(q, k.transpose(-2, -1)) / math.sqrt(8.0), dim=-1)
        return lin(3, torch.matmul(pr, v).transpose(1, 2).reshape(B, P, 32))
    for blk in range(4):
        y1 = attend(x1, x2, f"view_fusion.blocks.{blk}.fusion1") + x1
        y2 = attend(x2, x1, f"view_fusion.blocks.{blk}.fusion2") + x2
        x1, x2 = y1, y2
    return x1, x2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="256,8,1")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_baseline.py measures on the GPU; there is none")
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    sys.path.insert(0, ROOT)
    import bench
    emit({"probe": bench.achievable_peaks(_lib.load(), torch.device("cuda", 0)), "device": torch.cuda.get_device_name(0)})
    batches = [int(b) for b in a.batches.split(",")]
    sd_b, sd_5 = synth.baseline_state_dict(seed=0), synth.adapose_state_dict(seed=0)
    wt = {k: torch.from_numpy(v).cuda() for k, v in sd_b.items() if k.startswith("view_fusion.")}

    # 1. the attention stack alone (fp32 in either case)
    net = AdaPoseNet(sd_b, dtype="bf16", arch="baseline")
    for B in batches:
        x1, x2 = (torch.from_numpy(x).cuda() for x in synth.view_fusion_inputs(B, 1024, seed=1))
        got, ref = net.view_fusion(x1, x2), torch_stack(wt, x1, x2)
        torch.cuda.synchronize()
        diff = max(float((g - r).abs().max() / r.abs().max()) for g, r in zip(got, ref))
        (k_ms, k_sp), (t_ms, t_sp) = timed([lambda: net.view_fusion(x1, x2), lambda: torch_stack(wt, x1, x2)], a.steps, a.warmup)
        flop = B * 2 * 4 * (4 * 2 * 1024 * 32 * 32 + 2 * 2 * 4 * 1024 * 1024 * 8)      # per direction and block: four linears, q k^T and p v
        emit({"leg": "view_fusion", "B": B, "P": 1024, "ms_kernel": round(k_ms, 3), "ms_torch_composed": round(t_ms, 3),
              "ms_spread_max_minus_min": [round(k_sp, 3), round(t_sp, 3)], "kernel_TFLOPs_algorithmic": round(flop / k_ms / 1e9, 1),
              "score_bytes_torch_writes_GB": round(B * 2 * 4 * 4 * 1024 * 1024 * 4 / 1e9, 2), "max_rel_diff_kernel_vs_torch": diff})
        del got, ref
    net.close()

    # 2. forward + box tail, baseline against v5
    for dt in ("bf16", "bf16x3"):
        nb = AdaPoseNet(sd_b, dtype=dt, arch="baseline", options={"view2_heads": 0})
        n5 = AdaPoseNet(sd_5, dtype=dt, options={"view2_heads": 0})
        for B in batches:
            i8 = synth.adapose_inputs(min(B, 8), seed=0)
            rep = (B + 7) // 8
            t = {k: torch.from_numpy(np.concatenate([v] * rep)[:B]).cuda() for k, v in i8.items()}
            t = {k: (v.int() if k.startswith("choose") else v.float() if k in ("img1", "img2", "P1", "P2", "depths") else v.double()) for k, v in t.items()}

            def step(n):
                o = n(t["img1"], t["choose1"], t["img2"], t["choose2"], t["P1"], t["P2"], t["depths"])
                return postprocess(o["view1_nocs"], o["view1_depth"], o["view1_r"], t["choose1"], t["K1"], t["E1"])
            (b_ms, b_sp), (v_ms, v_sp) = timed([lambda: step(nb), lambda: step(n5)], a.steps, a.warmup)
            emit({"leg": "forward+postprocess", "dtype": dt, "B": B, "view2_heads": 0, "ms_baseline": round(b_ms, 3), "ms_v5": round(v_ms, 3),
                  "ms_spread_max_minus_min": [round(b_sp, 3), round(v_sp, 3)]})
        nb.close()
        n5.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
