"""Forward + box tail of the real-world network against v5 with view2_heads equal (0: what either estimator runs), in one process on one
device, alternating A / B blocks; and the kernels that differ, each alone.

usage: bench_realworld.py [--batches 256 8 1] [--dtypes bf16 bf16x3] [--blocks 5] [--iters N]
  A = v5:         AdaPoseNet(adapose_state_dict)   -> postprocess            (the shipped direct-regression tail)
  B = real-world: AdaPoseNet(arch="realworld")     -> postprocess_pnp_scaled
  bf16 also times A with option sweep_f16 = 0 (arm v5_bf16_sweep): the conv0 form the real-world network runs (bf16 feature map, fp32
  blend), the yardstick of its conv0; v5's default bf16 form is the packed-f16 persistent sweep, which a variance volume cannot use.
Per (batch, dtype): ms per call of both arms (median over the blocks, min .. max), B / A; ms per forward of conv0 in both arms (the
in-library profiler's rows), of the pose-rows kernel and of both tails alone (device events).  One JSON line per (batch, dtype) at the end.
Last, both PnP tails on the same points: case p1024_mid of tests/pnp_cases.py tiled to each batch, rgbm_adapose_postprocess_pnp (two
views: matching, triangulation, scale median, then the shared steps) against rgbm_adapose_postprocess_pnp_scaled (the shared steps)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rgbmanip_amd import _lib, synth  # noqa: E402
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from rgbmanip_amd.adapose import AdaPoseNet, postprocess, postprocess_pnp, postprocess_pnp_scaled  # noqa: E402


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


def prof_rows(lib, fn, iters, pat):
    """ms per call of the profiler rows whose name contains `pat`, summed"""
    _lib.check(lib.rgbm_prof_start())
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    st = (C.c_double * (4 * _lib.PROF_ROWS))()
    _lib.check(lib.rgbm_prof_stop(st))
    st = np.array(list(st)).reshape(_lib.PROF_ROWS, 4)
    rows = {_lib.PROF_KERNELS[v][0]: st[v][1] / iters for v in range(_lib.PROF_ROWS) if st[v][0] > 0}
    return {k: round(v, 4) for k, v in rows.items() if pat in k}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 8, 1])
    ap.add_argument("--dtypes", nargs="+", default=["bf16", "bf16x3"])
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=0, help="calls per block (0: 3 at batch >= 64, else 20)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_realworld.py measures on the GPU; there is no CPU timing"
    lib = _lib.load()
    base = synth.adapose_inputs(16, seed=0)
    pts1, pts2, coor1, coor2 = synth.realworld_coor(16, seed=0)
    results = []
    for dtype in args.dtypes:
        nets = {"v5": AdaPoseNet(synth.adapose_state_dict(seed=0), dtype=dtype, options={"view2_heads": 0}),
                "realworld": AdaPoseNet(synth.realworld_state_dict(seed=0), dtype=dtype, arch="realworld", options={"view2_heads": 0})}
        if dtype == "bf16":
            nets["v5_bf16_sweep"] = AdaPoseNet(synth.adapose_state_dict(seed=0), dtype=dtype, options={"view2_heads": 0, "sweep_f16": 0})
        for B in args.batches:
            iters = args.iters or (3 if B >= 64 else 20)
            inp = {k: tiled(v, B) for k, v in base.items()}
            c1, c2, p1 = tiled(coor1, B), tiled(coor2, B), tiled(pts1, B)
            net_args = (inp["img1"], inp["choose1"], inp["img2"], inp["choose2"], inp["P1"], inp["P2"], inp["depths"])
            K0 = torch.tensor([[439.31, 0, 320.0], [0, 439.31, 240.0], [0, 0, 1.0]], dtype=torch.float64, device="cuda").expand(B, 3, 3).contiguous()
            last = {}

            def arm_v5():
                o = last["v5"] = nets["v5"](*net_args)
                postprocess(o["view1_nocs"], o["view1_depth"], o["view1_r"], inp["choose1"], inp["K1"], inp["E1"])

            def arm_rw():
                o = last["realworld"] = nets["realworld"](*net_args, coor1=c1, coor2=c2)
                postprocess_pnp_scaled(o["view1_nocs"], p1, o["view1_s"], K0, inp["E1"], seed=5)
            arms = {"v5": arm_v5, "realworld": arm_rw}
            if "v5_bf16_sweep" in nets:
                def arm_v5s():
                    o = nets["v5_bf16_sweep"](*net_args)
                    postprocess(o["view1_nocs"], o["view1_depth"], o["view1_r"], inp["choose1"], inp["K1"], inp["E1"])
                arms["v5_bf16_sweep"] = arm_v5s
            for fn in arms.values():      # warm every shape of the timed window
                fn(); fn()
            torch.cuda.synchronize()
            ms = {k: [] for k in arms}
            for _ in range(args.blocks):      # A B A B ...: drift of the box lands on both arms
                for k, fn in arms.items():
                    ms[k].append(events_ms(fn, iters))
            med = {k: float(np.median(v)) for k, v in ms.items()}
            conv0 = {k: prof_rows(lib, (lambda k=k: arms[k]()), 3, "conv0") for k in arms}
            o5, orw = last["v5"], last["realworld"]
            tails = {"v5_postprocess": events_ms(lambda: postprocess(o5["view1_nocs"], o5["view1_depth"], o5["view1_r"], inp["choose1"], inp["K1"], inp["E1"]), 10),
                     "realworld_pnp_scaled": events_ms(lambda: postprocess_pnp_scaled(orw["view1_nocs"], p1, orw["view1_s"], K0, inp["E1"], seed=5), 10)}
            nocs4 = torch.zeros(B * 1024, 4, dtype=torch.float32, device="cuda")
            nocs4[:, :3] = orw["view1_nocs"].reshape(-1, 3)
            rows = torch.empty(B * 1024, 128, dtype=torch.float32, device="cuda")
            depth = orw["view1_depth"].contiguous()
            pose_rows = events_ms(lambda: _lib.check(lib.rgbm_pose_rows(nets["realworld"]._h, _lib.ptr(nocs4), _lib.ptr(c1), None, _lib.ptr(depth),
                                                                         _lib.ptr(rows), B, 1024, B, _lib.stream_ptr(None)), "rgbm_pose_rows"), 20)
            r = dict(batch=B, dtype=dtype, iters=iters, blocks=args.blocks,
                     ms={k: dict(median=round(med[k], 4), min=round(min(v), 4), max=round(max(v), 4)) for k, v in ms.items()},
                     realworld_over_v5=round(med["realworld"] / med["v5"], 4), conv0_ms=conv0, pose_rows_ms=round(pose_rows, 4),
                     tail_ms={k: round(v, 4) for k, v in tails.items()})
            print(f"B={B:4d} {dtype:7s}  v5 {med['v5']:9.3f} ms [{min(ms['v5']):.3f} .. {max(ms['v5']):.3f}]   real-world {med['realworld']:9.3f} ms "
                  f"[{min(ms['realworld']):.3f} .. {max(ms['realworld']):.3f}]   ratio {r['realworld_over_v5']:.3f}   conv0 {conv0}   "
                  f"pose rows {pose_rows:.4f} ms   tails {r['tail_ms']}", flush=True)
            results.append(r)
        for n in nets.values():
            n.close()
        del nets
        torch.cuda.empty_cache()
    import pnp_cases as pc
    c, scale = pc.inputs("p1024_mid"), pc.oracle("p1024_mid")[1]["scale"]
    for B in args.batches:
        t = {k: tiled(np.asarray(c[k])[None].astype(np.float32 if k in ("nocs1", "pts1", "nocs2", "pts2") else np.float64), B)
             for k in ("nocs1", "pts1", "nocs2", "pts2", "K", "E1", "E2")}
        s1 = torch.tensor([scale, 0.0, 0.0], dtype=torch.float32, device="cuda").expand(B, 3).contiguous()
        two = lambda: postprocess_pnp(t["nocs1"], t["pts1"], t["nocs2"], t["pts2"], t["K"], t["E1"], t["E2"], seed=5)      # noqa: E731
        one = lambda: postprocess_pnp_scaled(t["nocs1"], t["pts1"], s1, t["K"], t["E1"], seed=5)                            # noqa: E731
        two(); one()
        torch.cuda.synchronize()
        r = dict(batch=B, case="p1024_mid", pnp_two_view_ms=round(events_ms(two, 5), 4), pnp_scaled_ms=round(events_ms(one, 5), 4))
        print(f"B={B:4d} PnP tails on p1024_mid: two-view {r['pnp_two_view_ms']:.3f} ms, scaled {r['pnp_scaled_ms']:.3f} ms", flush=True)
        results.append(r)
    for r in results:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
