#!/usr/bin/env python3
"""A/B of the estimator's feature cache (cfg hip_feature_cache, DESIGN.md "Feature cache"): cache off (the plain path) against on,
in one process on one device, for the estimator in bf16 and bf16x3.

    python tools/bench_feature_cache.py [--envs 512] [--iters 3] [--dtypes bf16,bf16x3] [--out profiles/feature_cache_ab.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_feature_cache.py --trace [--cache 0|1]     # kernel counts, one mode
    python tools/bench_feature_cache.py --stats-csv DIR/.../*_kernel_stats.csv --envs 512 --dtypes bf16    # GB/s of the two copies
    python tools/bench_feature_cache.py --boundary [--poses 256] [--calls 10] [--out profiles/feature_cache_content_ab.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_feature_cache.py --fingerprint [--views 512]      # the key kernel alone

Per dtype and mode, after one warm-up PPO iteration: the median over iterations of the rollout's env-steps/s of the PPO loop as
bench.py's PPO leg builds it (PPO over ControlInterface over SyntheticMultiVecEnv), and the median estimator time per controller step
(device events around estimate_device_indexed), the first estimation of an episode (two new rows) apart from the others (one new row).

--boundary: the numpy `estimate()` boundary with hip_feature_cache "content" ("content keys") against off: float64
host frames, every call replaces one of the two views of each pose by a frame not met for two calls (what rl_pose.py's host
ControlInterface hands over); wall time per call, median of --calls after three warm-up calls, and the views the PSPNet ran on.
--fingerprint: rgbm_crop_fingerprint on --views crops against rgbm_microbench_copy over the same bytes, device events.
"""
import argparse
import csv
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(dtype, cache, envs, device=0):
    import torch
    from rgbmanip_amd import synth
    from rgbmanip_amd.config import ADAPOSE_CFGS, rl_cfg
    from rgbmanip_amd.control_interface import ControlInterface
    from rgbmanip_amd.estimator import AdaPoseEstimator_v5
    from rgbmanip_amd.ppo import PPO
    from rgbmanip_amd.synthetic_env import SyntheticManipulation, SyntheticMultiVecEnv
    dev = torch.device("cuda", device)
    cfg = rl_cfg(task="cabinet", device=str(dev), print_log=False, log_dir="/tmp/rgbm_bench_logs", save_dir="/tmp/rgbm_bench_saves")
    ecfg = dict(ADAPOSE_CFGS["adapose_cabinet"], load=False, hip_prepare="device")
    if cache:
        ecfg["hip_feature_cache"] = True
    est = AdaPoseEstimator_v5(None, ecfg, None, state_dict=synth.adapose_state_dict(seed=0, prefix="module."), dtype=dtype, device=device)
    venv = SyntheticMultiVecEnv(envs, dev, seed=0)
    ci = ControlInterface(venv, est, SyntheticManipulation(venv), cfg, device=dev)
    events = []
    inner = est.estimate_device_indexed

    def timed(*a, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = inner(*a, **kw)
        e1.record()
        events.append((e0, e1, len(kw["fresh"]) if kw.get("fresh") is not None else -1))
        return out
    est.estimate_device_indexed = timed
    return est, ci, PPO(ci, cfg), events


def run_mode(dtype, cache, envs, iters):
    import torch
    est, ci, ppo, events = build(dtype, cache, envs)
    ppo.run(1, log_interval=1, save_interval=10 ** 9)             # warm-up: allocations, code objects, the feature pool
    torch.cuda.synchronize()
    events.clear()
    v0 = est.feature_views_computed
    fps = []
    for _ in range(iters):
        ppo.run(1, log_interval=1, save_interval=10 ** 9)
        fps.append(float(ppo.last_fps))
    torch.cuda.synchronize()
    ms = [(e0.elapsed_time(e1), nf) for e0, e1, nf in events]
    later = [t for t, nf in ms if nf in (-1, envs)] if cache else [t for t, _ in ms]
    first = [t for t, nf in ms if nf == 2 * envs]
    res = {"dtype": dtype, "cache": int(cache), "envs": envs, "estimations": len(ms),
           "psp_views_per_estimation": round((est.feature_views_computed - v0) / max(len(ms), 1), 1),
           "estimator_ms_median": round(statistics.median(later), 3),
           "estimator_ms_first_of_episode_median": round(statistics.median(first), 3) if first else None,
           "env_steps_per_sec_median": round(statistics.median(fps), 1), "env_steps_per_sec_all": [round(f, 1) for f in fps],
           "feature_bytes": est.estimator.feature_bytes}
    del ppo, ci, est
    import gc
    gc.collect()
    torch.cuda.empty_cache()
    return res


def stats_csv(path, envs, dtype):
    """Achieved GB/s of the store and the gather from a rocprofv3 --kernel-trace --stats kernel_stats.csv of a --trace --cache 1 run."""
    per = {"bf16": 2, "fp16": 2, "fp32": 4, "bf16x3": 4}[dtype] * 224 * 224 * 32
    rows = list(csv.DictReader(open(path)))
    for r in rows:
        name = r.get("Name", "")
        for kern in ("feat_gather_kernel", "feat_store_kernel"):
            if kern not in name:
                continue
            avg_ns = float(r["AverageNs"])
            # the gather fills both views of every pose; a store holds one new row, two at the first estimation of a 4-step episode
            views = 2 * envs if "gather" in kern else envs * 1.25
            gb = 2.0 * views * per / 1e9                            # read + written
            print(f"{kern}: calls {r['Calls']}, average {avg_ns / 1e3:.1f} us, {views:.0f} views x {per} B read + written on average "
                  f"-> {gb / (avg_ns * 1e-9):.0f} GB/s")


def boundary_sets(poses, device=0):
    """Three sets of `poses` float64 host frames with masks and cameras (the headline workload's frames, bench.make_inputs_crop)."""
    import numpy as np
    import torch
    import bench
    sets = []
    for seed in (0, 1):
        fr = bench.make_inputs_crop(poses, torch.device("cuda", device), seed=seed, keep_frames=True)[2]
        for v in ((1, 2) if seed == 0 else (1,)):
            sets.append((fr[f"rgb{v}"].cpu().numpy().astype(np.float64), fr[f"mask{v}"].cpu().numpy().astype(bool), fr[f"E{v}"].cpu().numpy()))
        K = fr["K"].cpu().numpy()
        del fr
        torch.cuda.empty_cache()
    return K, sets


def run_boundary(dtype, mode, K, sets, calls, warmup=3):
    import time
    import torch
    from rgbmanip_amd import synth
    from rgbmanip_amd.config import ADAPOSE_CFGS
    from rgbmanip_amd.estimator import AdaPoseEstimator_v5
    ecfg = dict(ADAPOSE_CFGS["adapose_cabinet"], load=False, hip_prepare="device")
    if mode:
        ecfg["hip_feature_cache"] = mode
    est = AdaPoseEstimator_v5(None, ecfg, None, state_dict=synth.adapose_state_dict(seed=0, prefix="module."), dtype=dtype)
    cur, ms, views = [0, 1], [], []
    for k in range(warmup + calls):
        if k:
            cur[(k + 1) % 2] = 3 - cur[0] - cur[1]          # the slot the reference's queue refills, with the set not in use
        (r1, m1, e1), (r2, m2, e2) = sets[cur[0]], sets[cur[1]]
        v0 = est.feature_views_computed
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        est.estimate(K, r1, m1, e1, r2, m2, e2)
        ms.append((time.perf_counter() - t0) * 1e3)
        views.append(est.feature_views_computed - v0)
    res = {"boundary": "estimate() float64 host frames", "dtype": dtype, "cache": mode or "off", "poses": len(K), "calls": calls,
           "ms_per_call_median": round(statistics.median(ms[warmup:]), 2), "ms_per_call_min": round(min(ms[warmup:]), 2),
           "ms_per_call_all": [round(t, 1) for t in ms[warmup:]], "psp_views_per_call": views[warmup:],
           "bypassed": est.feature_cache_bypassed, "records": 0 if est._content.pool is None else int(est._content.pool.shape[0]),
           "feature_bytes": est.estimator.feature_bytes}
    del est
    import gc
    gc.collect()
    torch.cuda.empty_cache()
    return res


def run_fingerprint(views, iters=20):
    """Device-event time of the key kernel on `views` crops of 3 x 224 x 224 words, and of the 16-byte copy over the same bytes."""
    import torch
    from rgbmanip_amd import _lib
    lib = _lib.load()
    n_words = 3 * 224 * 224
    img = torch.randn(views, n_words, device="cuda")
    dst = torch.empty_like(img)
    keys = torch.empty(views, 2, dtype=torch.int64, device="cuda")
    nbytes = img.numel() * 4

    def timed(fn):
        for _ in range(3):
            fn()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
        ev[0].record()
        for i in range(iters):
            fn()
            ev[i + 1].record()
        torch.cuda.synchronize()
        return statistics.median(ev[i].elapsed_time(ev[i + 1]) for i in range(iters))
    t_key = timed(lambda: _lib.check(lib.rgbm_crop_fingerprint(_lib.ptr(img), views, n_words, _lib.ptr(keys), _lib.stream_ptr()), "rgbm_crop_fingerprint"))
    t_copy = timed(lambda: _lib.check(lib.rgbm_microbench_copy(_lib.ptr(img), _lib.ptr(dst), nbytes, _lib.stream_ptr()), "rgbm_microbench_copy"))
    return {"fingerprint": "rgbm_crop_fingerprint (memset + kernel, device events)", "views": views, "bytes_read": nbytes,
            "ms_median": round(t_key, 4), "GB_per_s_read": round(nbytes / t_key / 1e6, 1),
            "microbench_copy_ms_median": round(t_copy, 4), "microbench_copy_GB_per_s_read_plus_written": round(2 * nbytes / t_copy / 1e6, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=512)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--dtypes", default="bf16,bf16x3")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true", help="one PPO iteration after the warm-up in one mode (--cache), for rocprofv3")
    ap.add_argument("--cache", type=int, default=1)
    ap.add_argument("--stats-csv", default=None)
    ap.add_argument("--boundary", action="store_true", help='the numpy estimate() boundary, hip_feature_cache "content" against off')
    ap.add_argument("--poses", type=int, default=256)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--fingerprint", action="store_true", help="rgbm_crop_fingerprint alone against rgbm_microbench_copy")
    ap.add_argument("--views", type=int, default=512)
    args = ap.parse_args()
    dtypes = args.dtypes.split(",")
    if args.stats_csv:
        return stats_csv(args.stats_csv, args.envs, dtypes[0])
    import json
    lines = []
    if args.boundary or args.fingerprint:
        if args.fingerprint:
            lines.append(json.dumps(run_fingerprint(args.views)))
            print(lines[-1], flush=True)
        if args.boundary:
            K, sets = boundary_sets(args.poses)
            for dt in dtypes:
                for mode in (False, "content"):
                    lines.append(json.dumps(run_boundary(dt, mode, K, sets, args.calls)))
                    print(lines[-1], flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        return
    for dt in dtypes:
        for cache in ((args.cache,) if args.trace else (0, 1)):
            r = run_mode(dt, bool(cache), args.envs, 1 if args.trace else args.iters)
            lines.append(json.dumps(r))
            print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
