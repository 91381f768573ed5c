#!/usr/bin/env python3
"""A/B of the crop-window upload (cfg hip_upload: "windows", rgbm_prepare_inputs_windows) against a checkout of the parent commit and
against this tree's own whole-frame upload, on one device in one run, legs alternating.

    git worktree add ../parent HEAD~1 && (cd ../parent && bash rgbmanip_amd/csrc/build.sh)
    python tools/bench_upload_windows.py --parent ../parent [--rounds 3] [--poses 256] [--out profiles/upload_windows_ab.txt]

Three legs per round, each a fresh child process (`--leg TREE --mode MODE`) that imports `rgbmanip_amd` from TREE and its own library:

  parent    the parent commit's `estimate()` as it is
  frames    this tree with hip_upload: "frames" — the control: the same upload as the parent through this tree's code
  windows   this tree with hip_upload: "windows"

A leg runs `estimate()` on the frames of the headline workload (bench.make_inputs_crop) at --poses poses, as float64 and as uint8 HOST
frames, on a bf16 and a bf16x3 net, with hip_upload_chunk 32 (the chunk pipeline) and 0 (one batch): wall ms per call (median of the
leg's calls after two warm-up calls; the call returns host boxes), `upload_bytes_last_call` and the sha1 of the boxes.  The table gives
every round's figure per leg and the median over rounds; the boxes of the three legs must be the same bits at equal chunking."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("parent", "frames", "windows")


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
    return round(statistics.median(ts), 3), out


def leg(tree, mode, poses, calls):
    sys.path.insert(0, os.path.abspath(tree))            # rgbmanip_amd of this tree ...
    sys.path.append(ROOT)                                # ... bench.py (the frames) of the tree the tool lives in
    import numpy as np
    import torch
    import bench
    from rgbmanip_amd import _lib, synth
    from rgbmanip_amd.adapose import AdaPoseNet
    from rgbmanip_amd.config import ADAPOSE_CFGS
    from rgbmanip_amd.estimator import AdaPoseEstimator_v5
    assert os.path.abspath(_lib.__file__).startswith(os.path.abspath(tree)), _lib.__file__
    dev = torch.device("cuda", 0)
    res = {"tree": tree, "mode": mode, "poses": poses}
    fr = bench.make_inputs_crop(poses, dev, seed=0, keep_frames=True)[2]
    K, E1, E2 = (fr[k].cpu().numpy() for k in ("K", "E1", "E2"))
    hm1, hm2 = fr["mask1"].cpu().numpy(), fr["mask2"].cpu().numpy()
    host = {"float64": tuple(fr[k].cpu().numpy().astype(np.float64) for k in ("rgb1", "rgb2")),
            "uint8": tuple(torch.clamp(torch.round(fr[k] * 255.0), 0, 255).to(torch.uint8).cpu().numpy() for k in ("rgb1", "rgb2"))}
    del fr
    torch.cuda.empty_cache()
    sha = lambda b: hashlib.sha1(np.ascontiguousarray(b).tobytes()).hexdigest()[:12]      # noqa: E731
    sd = synth.adapose_state_dict(seed=0, prefix="module.")
    for dtype in ("bf16", "bf16x3"):
        net = AdaPoseNet(sd, dtype=dtype, device=0, options={"view2_heads": 0})
        for chunk in (32, 0):
            cfg = dict(ADAPOSE_CFGS["adapose_cabinet"], load=False, hip_prepare="device", hip_upload_chunk=chunk, hip_dtype=dtype)
            if mode != "parent":
                cfg["hip_upload"] = mode
            est = AdaPoseEstimator_v5(None, cfg, None, net=net)
            for hd, (h1, h2) in host.items():
                key = f"{hd}_{dtype}_chunk{chunk}"
                med, box = _median_ms(lambda: est.estimate(K, h1, hm1, E1, h2, hm2, E2), calls, 2)
                res[key + "_ms"], res[key + "_sha"] = med, sha(box)
                res[key + "_upload_bytes"] = getattr(est, "upload_bytes_last_call", None)
            del est
        del net
        torch.cuda.empty_cache()
    print("LEG " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg")
    ap.add_argument("--mode", choices=LEGS)
    ap.add_argument("--parent")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--poses", type=int, default=256)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--leg-timeout", type=int, default=420)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upload_windows_ab.txt"))
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg, a.mode, a.poses, a.calls)
    if not a.parent:
        ap.error("--parent: a built checkout of the parent commit")
    legs = {name: [] for name in LEGS}
    for r in range(a.rounds):
        for name in LEGS[r % 3:] + LEGS[:r % 3]:                 # every leg takes every place in the order
            tree = a.parent if name == "parent" else ROOT
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", tree, "--mode", name, "--poses", str(a.poses),
                                "--calls", str(a.calls)], capture_output=True, text=True, timeout=a.leg_timeout)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("LEG ")]
            if p.returncode != 0 or not line:                    # nothing more is started on the device after a failed leg
                sys.stderr.write(p.stdout[-4000:] + p.stderr[-4000:])
                sys.exit(f"leg {name} of round {r} failed (exit code {p.returncode})")
            legs[name].append(json.loads(line[0][4:]))
            print(f"round {r} {name}: " + line[0][4:], flush=True)
    report(legs, a)


def report(legs, a):
    cases = [k[:-3] for k in legs["windows"][0] if k.endswith("_ms")]
    rows = [f"crop-window upload: parent commit | this tree, hip_upload: frames (control) | this tree, hip_upload: windows; one device, {a.rounds} "
            "rounds of fresh processes, legs rotating",
            f"(tools/bench_upload_windows.py --poses {a.poses} --calls {a.calls}; estimate() wall ms per call: median over a leg's calls, then per round | median)",
            "", f"{'host frames_net_chunk':30s} {'parent':>34s} {'frames (control)':>34s} {'windows':>34s}  control/parent  windows/parent"]
    slow = []
    for c in cases:
        cols, meds = [], []
        for name in LEGS:
            vals = [leg_[c + "_ms"] for leg_ in legs[name]]
            meds.append(statistics.median(vals))
            cols.append(" ".join(f"{v:g}" for v in vals) + f" | {meds[-1]:g}")
        rows.append(f"{c:30s} {cols[0]:>34s} {cols[1]:>34s} {cols[2]:>34s}  {(meds[1] / meds[0] - 1) * 100:+13.1f} %  {(meds[2] / meds[0] - 1) * 100:+13.1f} %")
        if meds[1] > 1.04 * meds[0]:
            slow.append(c)
    rows += ["", "upload_bytes_last_call (payload handed to the copy engine per call; the parent does not report it):"]
    for c in cases:
        b = [legs[name][0].get(c + "_upload_bytes") for name in LEGS]
        rows.append(f"{c:30s} frames {b[1]}  windows {b[2]}  ({100.0 * b[2] / b[1]:.1f} %)")
    rows.append("")
    same = True
    for c in cases:
        shas = {name: sorted({leg_[c + "_sha"] for leg_ in legs[name]}) for name in LEGS}
        ok = shas["parent"] == shas["frames"] == shas["windows"] and len(shas["parent"]) == 1
        same &= ok
        rows.append(f"{c + '_sha':34s} parent {shas['parent']} frames {shas['frames']} windows {shas['windows']} -> {'same bits' if ok else 'DIFFERENT'}")
    rows.append("boxes: " + ("the three legs agree bit for bit in every case" if same else "DIFFERENCES above"))
    rows.append("control slower than the parent by more than 4 % (the box-to-box spread the README records): " + (", ".join(slow) if slow else "no case"))
    text = "\n".join(rows) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
