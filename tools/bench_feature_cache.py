#!/usr/bin/env python3
"""A/B of the estimator's feature cache (cfg hip_feature_cache, DESIGN.md "Feature cache"): cache off (the plain path) against on,
in one process on one device, for the estimator in bf16 and bf16x3.

    python tools/bench_feature_cache.py [--envs 512] [--iters 3] [--dtypes bf16,bf16x3] [--out profiles/feature_cache_ab.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_feature_cache.py --trace [--cache 0|1]     # kernel counts, one mode
    python tools/bench_feature_cache.py --stats-csv DIR/.../*_kernel_stats.csv --envs 512 --dtypes bf16    # GB/s of the two copies

Per dtype and mode, after one warm-up PPO iteration: the median over iterations of the rollout's env-steps/s of the PPO loop as
bench.py's PPO leg builds it (PPO over ControlInterface over SyntheticMultiVecEnv), and the median estimator time per controller step
(device events around estimate_device_indexed), the first estimation of an episode (two new rows) apart from the others (one new row).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=512)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--dtypes", default="bf16,bf16x3")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true", help="one PPO iteration after the warm-up in one mode (--cache), for rocprofv3")
    ap.add_argument("--cache", type=int, default=1)
    ap.add_argument("--stats-csv", default=None)
    args = ap.parse_args()
    dtypes = args.dtypes.split(",")
    if args.stats_csv:
        return stats_csv(args.stats_csv, args.envs, dtypes[0])
    import json
    lines = []
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
