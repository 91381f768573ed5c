#!/usr/bin/env python3
"""A/B of 8-bit frames consumed natively (rgbm_prepare_inputs_u8, cfg controller.hip_queue_dtype) against a checkout of the parent
commit, on one device in one run, legs alternating.

    git worktree add ../parent HEAD~1 && (cd ../parent && bash rgbmanip_amd/csrc/build.sh)
    python tools/bench_frames_u8.py --parent ../parent [--rounds 3] [--poses 256] [--envs 512] [--out profiles/frames_u8_ab.txt]

Every leg is a fresh child process (`--leg TREE`) that imports `rgbmanip_amd` from TREE and its own library, so the two trees never
share a process.  A leg measures, on the frames of the headline workload (bench.make_inputs_crop) quantised to bytes:

  (a) `estimate()` at --poses poses with uint8 HOST frames, bf16 and bf16x3: wall ms per call (the call returns host boxes);
  (b) `estimate()` at --poses poses with uint8 CUDA frames (it enters `estimate_device()`; the parent converts the bytes to a float32
      copy first, upload.frames_to_device), bf16 and bf16x3: wall ms per call;
  (c) one `ControlInterface.step` at --envs synthetic envs, bf16 estimator, float32 queue (both trees) and uint8 queue (this tree):
      wall ms per step over two episodes after one warm-up episode, the view queue's bytes and torch.cuda.max_memory_allocated().

Each figure is the median over the leg's calls; the table gives every round's figure per tree and the median over rounds.  The boxes of
legs (a) and (b) are hashed (sha1 of the bytes) so that the table also says whether both trees computed the same bits."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _median_ms(fn, calls, warmup):
    import torch
    out = None
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 3), [round(t, 2) for t in ts], out


def leg(tree, poses, envs, calls):
    sys.path.insert(0, os.path.abspath(tree))            # rgbmanip_amd of this tree ...
    sys.path.append(ROOT)                                # ... bench.py (the frames) of the tree the tool lives in
    import gc
    import numpy as np
    import torch
    import bench
    from rgbmanip_amd import _lib, synth
    from rgbmanip_amd.config import ADAPOSE_CFGS
    from rgbmanip_amd.control_interface import ControlInterface
    from rgbmanip_amd.estimator import AdaPoseEstimator_v5
    from rgbmanip_amd.synthetic_env import SyntheticManipulation, SyntheticMultiVecEnv
    assert os.path.abspath(_lib.__file__).startswith(os.path.abspath(tree)), _lib.__file__
    dev = torch.device("cuda", 0)
    native = "rgbm_prepare_inputs_u8" in _lib.SIGNATURES
    res = {"tree": tree, "native_u8": native, "poses": poses, "envs": envs}
    fr = bench.make_inputs_crop(poses, dev, seed=0, keep_frames=True)[2]
    q = lambda x: torch.clamp(torch.round(x * 255.0), 0, 255).to(torch.uint8)      # noqa: E731
    u1, u2 = q(fr["rgb1"]), q(fr["rgb2"])
    m1, m2 = fr["mask1"], fr["mask2"]
    K, E1, E2 = (fr[k].cpu().numpy() for k in ("K", "E1", "E2"))
    h1, h2, hm1, hm2 = (t.cpu().numpy() for t in (u1, u2, m1, m2))
    del fr
    sha = lambda b: hashlib.sha1(np.ascontiguousarray(b).tobytes()).hexdigest()[:12]      # noqa: E731
    sd = synth.adapose_state_dict(seed=0, prefix="module.")
    for dtype in ("bf16", "bf16x3"):
        est = AdaPoseEstimator_v5(None, dict(ADAPOSE_CFGS["adapose_cabinet"], load=False, hip_prepare="device"), None, state_dict=sd,
                                  dtype=dtype)
        med, all_, box = _median_ms(lambda: est.estimate(K, h1, hm1, E1, h2, hm2, E2), calls, 2)
        res[f"a_estimate_host_u8_{dtype}_ms"], res[f"a_{dtype}_all"], res[f"a_{dtype}_sha"] = med, all_, sha(box)
        med, all_, box = _median_ms(lambda: est.estimate(K, u1, m1, E1, u2, m2, E2), calls, 2)
        res[f"b_estimate_cuda_u8_{dtype}_ms"], res[f"b_{dtype}_all"], res[f"b_{dtype}_sha"] = med, all_, sha(box)
        res[f"frames_u8_native_{dtype}"] = getattr(est, "frames_u8_native", None)
        if dtype == "bf16":
            est_bf16 = est
    del est, u1, u2, m1, m2
    gc.collect()
    torch.cuda.empty_cache()
    # (c) the controller step, bf16 estimator
    for qd in (("float32", "uint8") if native else ("float32",)):
        gc.collect()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        cfg = synth.control_cfg("cabinet", 0.0)
        if qd != "float32":
            cfg["controller"]["hip_queue_dtype"] = qd
        venv = SyntheticMultiVecEnv(envs, dev, seed=0, episodes=8)
        ci = ControlInterface(venv, est_bf16, SyntheticManipulation(venv), cfg, device=dev)
        acts = [torch.from_numpy(synth.control_actions(envs, s, 9) * 0.3).to(dev) for s in range(ci.max_steps)]
        step = [0]

        def one():
            step[0] += 1
            return ci.step(acts[step[0] % len(acts)])[1]
        med, all_, _ = _median_ms(one, 2 * ci.max_steps, ci.max_steps)
        res[f"c_step_{qd}_queue_ms"], res[f"c_{qd}_all"] = med, all_
        res[f"c_{qd}_queue_bytes"] = ci.image_queue.numel() * ci.image_queue.element_size()
        res[f"c_{qd}_max_memory_allocated"] = int(torch.cuda.max_memory_allocated())
        del ci, venv
    print("LEG " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg")
    ap.add_argument("--parent")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--poses", type=int, default=256)
    ap.add_argument("--envs", type=int, default=512)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--leg-timeout", type=int, default=420)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_u8_ab.txt"))
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg, a.poses, a.envs, a.calls)
    if not a.parent:
        ap.error("--parent: a built checkout of the parent commit")
    legs = {"parent": [], "branch": []}
    for r in range(a.rounds):
        for name in (("parent", "branch") if r % 2 == 0 else ("branch", "parent")):
            tree = a.parent if name == "parent" else ROOT
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", tree, "--poses", str(a.poses), "--envs", str(a.envs),
                                "--calls", str(a.calls)], capture_output=True, text=True, timeout=a.leg_timeout)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("LEG ")]
            if p.returncode != 0 or not line:                    # nothing more is started on the device after a failed leg
                sys.stderr.write(p.stdout[-4000:] + p.stderr[-4000:])
                sys.exit(f"leg {name} of round {r} failed (exit code {p.returncode})")
            legs[name].append(json.loads(line[0][4:]))
            print(f"round {r} {name}: " + line[0][4:], flush=True)
    report(legs, a)


def report(legs, a):
    keys = [k for k in legs["branch"][0] if k.endswith("_ms") or k.endswith("_bytes") or k.endswith("_max_memory_allocated")]
    rows = [f"8-bit frames consumed natively: parent commit against this change, one device, {a.rounds} alternating rounds of fresh processes",
            f"(tools/bench_frames_u8.py --poses {a.poses} --envs {a.envs} --calls {a.calls}; each figure: median over a leg's calls, then per round | median)",
            "", f"{'measurement':46s} {'parent':>44s} {'this change':>44s}  change"]
    for k in keys:
        cols, meds = [], []
        for name in ("parent", "branch"):
            vals = [leg_[k] for leg_ in legs[name] if k in leg_]
            meds.append(statistics.median(vals) if vals else None)
            cols.append((" ".join(f"{v:g}" for v in vals) + f" | {meds[-1]:g}") if vals else "-")
        change = f"{(meds[1] / meds[0] - 1) * 100:+.1f} %" if meds[0] and meds[1] and k.endswith("_ms") else ""
        rows.append(f"{k:46s} {cols[0]:>44s} {cols[1]:>44s}  {change}")
    rows.append("")
    for k in [k for k in legs["branch"][0] if k.endswith("_sha")]:
        shas = {name: sorted({leg_[k] for leg_ in legs[name]}) for name in legs}
        rows.append(f"{k}: parent {shas['parent']} this change {shas['branch']} -> {'same bits' if shas['parent'] == shas['branch'] else 'DIFFERENT'}")
    rows.append("frames_u8_native after a leg (bf16 estimator): parent "
                f"{legs['parent'][0].get('frames_u8_native_bf16')}, this change {legs['branch'][0].get('frames_u8_native_bf16')}")
    text = "\n".join(rows) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
