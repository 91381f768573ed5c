"""Forward + box tail of the v2 network, its per-point plane-sweep kernel alone, and its point selection against v5's, in one process on
one device.

usage: bench_v2.py [--batches 256 1] [--dtypes bf16 bf16x3] [--blocks 5] [--iters N]
  A = v5 (context): AdaPoseNet(adapose_state_dict), view2_heads = 0 -> postprocess          (the shipped direct-regression tail)
  B = v2:           AdaPoseNet(arch="v2"),          view2_heads = 0 -> postprocess_pnp_scaled
Per (batch, dtype): ms per call of both arms in alternating blocks (median over the blocks, min .. max); ms of the new kernel alone
(rgbm_v2_point_rows on the forward's own fp32 feature maps, all 2B views: device events) with the gather traffic it asks for - 4 taps x
24 planes x 128 bytes + the reference row per point - as GB/s; ms of both tails alone.  Then prepare_inputs on 480 x 640 8-bit frames with
elliptical masks, sample="native" (choose_native_kernel) against the default (choose_kernel), the whole call each (they share the window
and crop kernels).  One JSON line per measurement at the end."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rgbmanip_amd import synth  # noqa: E402
from rgbmanip_amd.adapose import AdaPoseNet, postprocess, postprocess_pnp_scaled, prepare_inputs  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 1])
    ap.add_argument("--dtypes", nargs="+", default=["bf16", "bf16x3"])
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=0, help="calls per block (0: 3 at batch >= 64, else 20)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_v2.py measures on the GPU; there is no CPU timing"
    base = synth.adapose_inputs(16, seed=0)
    g = np.random.default_rng(0)
    results = []
    for dtype in args.dtypes:
        nets = {"v5": AdaPoseNet(synth.adapose_state_dict(seed=0), dtype=dtype, options={"view2_heads": 0}),
                "v2": AdaPoseNet(synth.v2_state_dict(seed=0), dtype=dtype, arch="v2", options={"view2_heads": 0})}
        for B in args.batches:
            iters = args.iters or (3 if B >= 64 else 20)
            inp = {k: tiled(v, B) for k, v in base.items()}
            net_args = (inp["img1"], inp["choose1"], inp["img2"], inp["choose2"], inp["P1"], inp["P2"], inp["depths"])
            pts = torch.from_numpy(np.stack([g.integers(0, 640, size=(B, 1024)), g.integers(0, 480, size=(B, 1024))], -1).astype(np.float32)).cuda()
            K0 = torch.tensor([[439.31, 0, 320.0], [0, 439.31, 240.0], [0, 0, 1.0]], dtype=torch.float64, device="cuda").expand(B, 3, 3).contiguous()
            last = {}

            def arm_v5():
                o = last["v5"] = nets["v5"](*net_args)
                postprocess(o["view1_nocs"], o["view1_depth"], o["view1_r"], inp["choose1"], inp["K1"], inp["E1"])

            def arm_v2():
                o = last["v2"] = nets["v2"](*net_args)
                postprocess_pnp_scaled(o["view1_nocs"], pts, o["view1_s"], K0, inp["E1"], seed=5)
            arms = {"v5": arm_v5, "v2": arm_v2}
            for fn in arms.values():      # warm every shape of the timed window
                fn(); fn()
            torch.cuda.synchronize()
            ms = {k: [] for k in arms}
            for _ in range(args.blocks):      # A B A B ...: drift of the box lands on both arms
                for k, fn in arms.items():
                    ms[k].append(events_ms(fn, iters))
            med = {k: float(np.median(v)) for k, v in ms.items()}
            o5, o2 = last["v5"], last["v2"]
            tails = {"v5_postprocess": events_ms(lambda: postprocess(o5["view1_nocs"], o5["view1_depth"], o5["view1_r"], inp["choose1"], inp["K1"], inp["E1"]), 10),
                     "v2_pnp_scaled": events_ms(lambda: postprocess_pnp_scaled(o2["view1_nocs"], pts, o2["view1_s"], K0, inp["E1"], seed=5), 10)}
            feat = nets["v2"].fetch(B, "feat", 2 * B * 224 * 224 * 32).view(2 * B, 224, 224, 32).clone()
            choose = torch.cat((inp["choose1"], inp["choose2"])).to(torch.int32)
            Pv = torch.cat((inp["P1"], inp["P2"]))
            alone = lambda: nets["v2"].v2_point_rows(feat, choose, Pv, inp["depths"])      # noqa: E731
            alone()
            torch.cuda.synchronize()
            k_ms = events_ms(alone, 10)
            gather_gb = 2 * B * 1024 * (4 * 24 + 1) * 128 / 1e9      # fp32 maps: what the taps and the reference row ask for
            del feat
            r = dict(batch=B, dtype=dtype, iters=iters, blocks=args.blocks,
                     ms={k: dict(median=round(med[k], 4), min=round(min(v), 4), max=round(max(v), 4)) for k, v in ms.items()},
                     v2_over_v5=round(med["v2"] / med["v5"], 4), point_rows_ms_2B_views_fp32_maps=round(k_ms, 4),
                     point_rows_gather_gb=round(gather_gb, 4), point_rows_gather_gbps=round(gather_gb / (k_ms * 1e-3), 1),
                     tail_ms={k: round(v, 4) for k, v in tails.items()})
            print(f"B={B:4d} {dtype:7s}  v5 {med['v5']:9.3f} ms [{min(ms['v5']):.3f} .. {max(ms['v5']):.3f}]   v2 {med['v2']:9.3f} ms "
                  f"[{min(ms['v2']):.3f} .. {max(ms['v2']):.3f}]   ratio {r['v2_over_v5']:.3f}   point rows alone ({2 * B} views, fp32 maps) {k_ms:.4f} ms = "
                  f"{r['point_rows_gather_gbps']} GB/s of {gather_gb:.3f} GB requested   tails {r['tail_ms']}", flush=True)
            results.append(r)
        for n in nets.values():
            n.close()
        del nets
        torch.cuda.empty_cache()
    # point selection: the whole prepare call, native against the resized-mask sampling, on the same frames
    yy, xx = np.mgrid[0:480, 0:640]
    for N, (ry, rx) in ((16, (60.0, 90.0)), (16, (200.0, 260.0))):
        u8 = torch.from_numpy(g.integers(0, 256, size=(N, 480, 640, 3), dtype=np.uint8)).cuda()
        mask = torch.from_numpy(np.stack([((yy - 240) / ry) ** 2 + ((xx - 300 - i) / rx) ** 2 <= 1 for i in range(N)]).astype(np.uint8)).cuda()
        K = torch.tensor([[439.31, 0, 320.0], [0, 439.31, 240.0], [0, 0, 1.0]], dtype=torch.float64, device="cuda").expand(N, 3, 3).contiguous()
        t = {}
        for mode in ("resized", "native"):
            fn = lambda mode=mode: prepare_inputs(u8, mask, K, 224, 1024, 3, want_pts2d=True, sample=mode)      # noqa: E731
            w = fn()
            torch.cuda.synchronize()
            t[mode] = events_ms(fn, 20)
        win = w["window"][0].tolist()
        r = dict(frames=N, window=win[1] - win[0], candidates_native=int(mask[0].sum()), prepare_ms={k: round(v, 4) for k, v in t.items()})
        print(f"prepare_inputs, {N} frames, window {r['window']}, {r['candidates_native']} native candidates: resized {t['resized']:.4f} ms, "
              f"native {t['native']:.4f} ms", flush=True)
        results.append(r)
    for r in results:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
