#!/usr/bin/env python3
"""Timings of the multi-view depth fusion at n = 256 poses, S = 224, on one device in one process.  Every
comparison runs as alternating blocks A B A B ...: a block is `--calls` calls timed one by one with device events, its figure their
median; reported per leg are the median of its blocks' figures and their spread (max - min over the blocks), so that a difference between
two legs can be read against what the same leg does from block to block.

  fusion    depth_fusion at V = 2, 4, 8 on the sphere scene's cameras (maps: seeded, smooth, with a NaN surround; conf and mask given).
            At V = 2 leg A is what it replaces: the two depth_consistency launches (one per direction, diagnostics off).
  pack      cloud_pack_views against cloud_pack at V = 2 on the keep / fused maps of that fusion, default capacity.
  estimate  estimate_cloud_views_device at V = 2 and V = 4 against estimate_cloud_device (bf16 net with the view-2 heads, uint8 frames on
            the device, loose thresholds: seeded weights give unrelated maps).  V = 2 runs 2 n network poses (each frame is a view 1
            once), V = 4 runs 4 n; estimate_cloud_device runs n.

    python tools/bench_cloud_views.py [--poses 256] [--blocks 5] [--calls 5] [--warmup 2] [--skip-estimate]

Prints one JSON line per comparison.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

S, H, W = 224, 480, 640


def time_blocks(legs, blocks, calls, warmup):
    """legs: {name: fn}.  Returns {name: (median over blocks of the block medians, max - min of the block medians)} in ms."""
    for _ in range(warmup):
        for f in legs.values():
            f()
    torch.cuda.synchronize()
    fig = {k: [] for k in legs}
    for _ in range(blocks):
        for k, f in legs.items():
            ms = []
            for _ in range(calls):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                f()
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            fig[k].append(float(np.median(ms)))
    return {k: (round(float(np.median(v)), 4), round(float(np.max(v) - np.min(v)), 4)) for k, v in fig.items()}


def fusion_inputs(n, V):
    """n poses x V views: the cameras of the sphere scenes (eight seeded poses tiled), smooth positive maps inside a disc, NaN outside."""
    from rgbmanip_amd import synth
    m = min(n, 8)
    Ks, Es = [], []
    for s in range((V + 1) // 2):
        inp = synth.adapose_inputs(m, seed=(0, 5, 11, 17)[s])
        Ks += [inp["K1"], inp["K2"]]
        Es += [inp["E1"], inp["E2"]]
    K, E = np.stack(Ks[:V], 1).astype(np.float64), np.stack(Es[:V], 1).astype(np.float64)
    depth = np.stack([synth.sphere_depth(K[:, v], E[:, v]) for v in range(V)], 1)
    g = np.random.default_rng(1)
    conf = g.random(depth.shape, dtype=np.float32)
    yy, xx = np.mgrid[0:S, 0:S]
    mask = np.broadcast_to((((yy - 112) / 100.0) ** 2 + ((xx - 112) / 100.0) ** 2 <= 1).astype(np.uint8), depth.shape).copy()
    reps = -(-n // m)
    tile = lambda a: torch.from_numpy(np.concatenate([a] * reps)[:n]).cuda()      # noqa: E731
    return tuple(tile(a) for a in (depth, K, E, conf, mask))


def frames(n, V):
    from rgbmanip_amd import synth
    g = np.random.default_rng(3)
    m = min(n, 8)
    yy, xx = np.mgrid[0:H, 0:W]
    Es = []
    for s in range((V + 1) // 2):
        inp = synth.adapose_inputs(m, seed=(0, 5)[s])
        Es += [inp["E1"], inp["E2"]]
    E = np.stack(Es[:V], 1).astype(np.float64)
    K = np.tile(np.array([[439.31, 0, 320.0], [0, 439.31, 240.0], [0, 0, 1.0]])[None], (m, 1, 1))
    u = g.integers(0, 256, (m, V, H, W, 3), dtype=np.uint8)
    mk = np.stack([np.stack([((yy - 240 - 5 * v) / (60.0 + 5 * v)) ** 2 + ((xx - 300 - 10 * i - 15 * v) / 90.0) ** 2 <= 1 for v in range(V)])
                   for i in range(m)]).astype(np.uint8)
    reps = -(-n // m)
    tile = lambda a: torch.from_numpy(np.concatenate([a] * reps)[:n]).cuda()      # noqa: E731
    return tuple(tile(a) for a in (K, u, mk, E))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-estimate", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_cloud_views needs a GPU: no timing is taken without one")
    from rgbmanip_amd.adapose import cloud_pack, cloud_pack_views, depth_consistency, depth_fusion
    n = args.poses
    tb = lambda legs: time_blocks(legs, args.blocks, args.calls, args.warmup)      # noqa: E731
    for V in (2, 4, 8):
        depth, K, E, conf, mask = fusion_inputs(n, V)
        th = dict(conf_min=0.5)
        legs = {}
        if V == 2:
            v = [(depth[:, i].contiguous(), K[:, i].contiguous(), E[:, i].contiguous(), conf[:, i].contiguous(), mask[:, i].contiguous()) for i in (0, 1)]

            def two():
                for a, b in ((0, 1), (1, 0)):
                    depth_consistency(*v[a][:3], *v[b][:3], conf_a=v[a][3], mask_a=v[a][4], want_diagnostics=False, **th)
            legs["A_two_depth_consistency"] = two
        legs["B_depth_fusion"] = lambda: depth_fusion(depth, K, E, conf=conf, mask=mask, n_min=1, want_agree=True, **th)
        rec = {"what": "fusion", "poses": n, "V": V, "blocks": args.blocks, "calls": args.calls}
        rec.update({k: {"ms": ms, "spread": sp} for k, (ms, sp) in tb(legs).items()})
        r = depth_fusion(depth, K, E, conf=conf, mask=mask, n_min=1, **th)
        rec["kept_share"] = round(float(r["keep"].float().mean()), 4)
        rec["pairs_per_s"] = round(n * V * (V - 1) * S * S / (rec["B_depth_fusion"]["ms"] * 1e-3), 0)
        print(json.dumps(rec), flush=True)
        if V == 2:
            f, k = r["fused"], r["keep"]
            pv = [(f[:, i].contiguous(), k[:, i].contiguous(), K[:, i].contiguous(), E[:, i].contiguous()) for i in (0, 1)]
            legs = {"A_cloud_pack": lambda: cloud_pack(*pv[0], *pv[1]), "B_cloud_pack_views": lambda: cloud_pack_views(f, k, K, E)}
            rec = {"what": "pack", "poses": n, "V": 2, "blocks": args.blocks, "calls": args.calls}
            rec.update({k_: {"ms": ms, "spread": sp} for k_, (ms, sp) in tb(legs).items()})
            print(json.dumps(rec), flush=True)
        del depth, K, E, conf, mask, r
        torch.cuda.empty_cache()
    if args.skip_estimate:
        return
    from rgbmanip_amd import synth
    from rgbmanip_amd.adapose import AdaPoseNet
    from rgbmanip_amd.config import ADAPOSE_CFGS
    from rgbmanip_amd.estimator import AdaPoseEstimator_v5
    net = AdaPoseNet(synth.adapose_state_dict(seed=0, prefix="module."), dtype="bf16", options={"view2_heads": 1})
    cfg = dict(ADAPOSE_CFGS["adapose_cabinet"], load=False, hip_dtype="bf16", hip_prepare="device", hip_prepare_seed=9, hip_view2_heads=True)
    est = AdaPoseEstimator_v5(None, cfg, None, net=net)
    loose = dict(px_max=60.0, rel_max=0.5, conf_min=0.05)
    for V in (2, 4):
        Kf, u, mk, E = frames(n, V)
        pair = (Kf, u[:, 0].contiguous(), mk[:, 0].contiguous(), E[:, 0].contiguous(), u[:, 1].contiguous(), mk[:, 1].contiguous(), E[:, 1].contiguous())
        legs = {"A_estimate_cloud_device": lambda: est.estimate_cloud_device(*pair, **loose),
                "B_estimate_cloud_views_device": lambda: est.estimate_cloud_views_device(Kf, u, mk, E, **loose)}
        rec = {"what": "estimate", "poses": n, "V": V, "network_poses": {"A": n, "B": n * V}, "blocks": args.blocks, "calls": max(args.calls // 2, 2)}
        rec.update({k: {"ms": ms, "spread": sp} for k, (ms, sp) in time_blocks(legs, args.blocks, max(args.calls // 2, 2), 1).items()})
        print(json.dumps(rec), flush=True)
        del Kf, u, mk, E, pair
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
