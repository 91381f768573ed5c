"""Stages A and B of the v1 network's heads alone, stage A against v2's point-rows kernel on the same inputs, and forward + box tail of the
v1 network beside v2's, in one process on one device.

usage: bench_v1.py [--batches 256 1] [--dtypes bf16 bf16x3] [--blocks 5] [--iters N]
Per (batch, dtype), on the v1 forward's own fp32 feature maps, all 2B views, device events, A / B blocks alternating (median, min .. max):
  stage_a     rgbm_v1_point_rows without stage B          (v1_fused_points_kernel + the homography launch)
  v2_rows     rgbm_v2_point_rows on the same maps, cameras and points, with a v2 net's weights (v2_point_rows_kernel + the homography launch)
  stage_ab    rgbm_v1_point_rows with stage B; stage B = stage_ab - stage_a (point_mlp_kernel's rows variant, or the per-layer launches
              where 2B x 1024 is no multiple of 64 - never at these batches)
  forward + tail of both networks (view2_heads = 0, postprocess_pnp_scaled), the same alternation; then the forwards alone, v5's beside
  them.  Under `rocprofv3 --kernel-trace --stats -- python tools/bench_v1.py --batches 256 --dtypes bf16 --blocks 1` the trace holds the
  16-bit-map kernels of the forwards (v1_fused_points_kernel<unsigned short>, v2_point_rows_kernel<unsigned short>) and, from v5's
  forward, point_mlp_kernel<unsigned short> beside stage B's point_mlp_kernel<float, 1>, all on 256 views x 1024 points.
One JSON line per measurement at the end.  The map storage type of the alone runs is fp32 (the entry points take fp32 maps); the 16-bit
gathers are inside the bf16 forward's figure."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rgbmanip_amd import synth  # noqa: E402
from rgbmanip_amd.adapose import AdaPoseNet, postprocess_pnp_scaled  # noqa: E402


def tiled(a, B):
    reps = -(-B // a.shape[0])
    return torch.from_numpy(np.concatenate([a] * reps, 0)[:B]).cuda()


def events_ms(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def alternate(arms, blocks, iters):
    for fn in arms.values():      # warm every shape of the timed window
        fn(); fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(blocks):      # A B A B ...: drift of the box lands on every arm
        for k, fn in arms.items():
            ms[k].append(events_ms(fn, iters))
    return {k: dict(median=round(float(np.median(v)), 4), min=round(min(v), 4), max=round(max(v), 4)) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 1])
    ap.add_argument("--dtypes", nargs="+", default=["bf16", "bf16x3"])
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=0, help="calls per block (0: 3 at batch >= 64, else 20)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_v1.py measures on the GPU; there is no CPU timing"
    base = synth.adapose_inputs(16, seed=0)
    g = np.random.default_rng(0)
    results = []
    for dtype in args.dtypes:
        nets = {"v5": AdaPoseNet(synth.adapose_state_dict(seed=0), dtype=dtype, options={"view2_heads": 0}),
                "v2": AdaPoseNet(synth.v2_state_dict(seed=0), dtype=dtype, arch="v2", options={"view2_heads": 0}),
                "v1": AdaPoseNet(synth.v1_state_dict(seed=0), dtype=dtype, arch="v1", options={"view2_heads": 0})}
        for B in args.batches:
            iters = args.iters or (3 if B >= 64 else 20)
            inp = {k: tiled(v, B) for k, v in base.items()}
            net_args = (inp["img1"], inp["choose1"], inp["img2"], inp["choose2"], inp["P1"], inp["P2"], inp["depths"])
            pts = torch.from_numpy(np.stack([g.integers(0, 640, size=(B, 1024)), g.integers(0, 480, size=(B, 1024))], -1).astype(np.float32)).cuda()
            K0 = torch.tensor([[439.31, 0, 320.0], [0, 439.31, 240.0], [0, 0, 1.0]], dtype=torch.float64, device="cuda").expand(B, 3, 3).contiguous()

            def arm(name):
                def fn():
                    o = nets[name](*net_args)
                    postprocess_pnp_scaled(o["view1_nocs"], pts, o["view1_s"], K0, inp["E1"], seed=5)
                return fn
            fwd = alternate({"v2": arm("v2"), "v1": arm("v1")}, args.blocks, iters)
            # the forwards without a tail (v5 for context: under a kernel trace its point_mlp_kernel stands beside stage B's variant)
            only = alternate({k: (lambda k=k: nets[k](*net_args)) for k in ("v5", "v2", "v1")}, args.blocks, iters)
            feat = nets["v1"].fetch(B, "feat", 2 * B * 224 * 224 * 32).view(2 * B, 224, 224, 32).clone()
            choose = torch.cat((inp["choose1"], inp["choose2"])).to(torch.int32)
            Pv = torch.cat((inp["P1"], inp["P2"]))
            alone = alternate({"stage_a": lambda: nets["v1"].v1_point_rows(feat, choose, Pv, inp["depths"], stage_b=False),
                               "v2_rows": lambda: nets["v2"].v2_point_rows(feat, choose, Pv, inp["depths"]),
                               "stage_ab": lambda: nets["v1"].v1_point_rows(feat, choose, Pv, inp["depths"])}, args.blocks, 10)
            del feat
            r = dict(batch=B, dtype=dtype, iters=iters, blocks=args.blocks, forward_tail_ms=fwd, forward_only_ms=only, alone_ms_2B_views_fp32_maps=alone,
                     stage_a_over_v2_rows=round(alone["stage_a"]["median"] / alone["v2_rows"]["median"], 4),
                     stage_b_ms=round(alone["stage_ab"]["median"] - alone["stage_a"]["median"], 4),
                     v1_over_v2=round(fwd["v1"]["median"] / fwd["v2"]["median"], 4))
            print(f"B={B:4d} {dtype:7s}  forward + tail: v2 {fwd['v2']}  v1 {fwd['v1']}  ratio {r['v1_over_v2']:.3f}\n"
                  f"      forward alone: v5 {only['v5']}  v2 {only['v2']}  v1 {only['v1']}\n"
                  f"      alone ({2 * B} views, fp32 maps): stage A {alone['stage_a']}  v2 rows {alone['v2_rows']}  A / v2 {r['stage_a_over_v2_rows']:.3f}  "
                  f"A + B {alone['stage_ab']}  stage B {r['stage_b_ms']:.4f} ms", flush=True)
            results.append(r)
        for n in nets.values():
            n.close()
        del nets
        torch.cuda.empty_cache()
    for r in results:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
