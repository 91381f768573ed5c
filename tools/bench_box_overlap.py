#!/usr/bin/env python3
"""Times the box agreement kernels: `rgbm_box_iou_matrix` at n = 256 poses with P = Q = 64 boxes (1 048 576 pairs)
and `rgbm_box_agreement` at n = 256 and n = 65 535 pairs, on seeded boxes that overlap like the S dropout samples of a pose do; device
events around the C call with the outputs allocated beforehand, warm, median of `--steps`.  The kernels have no predecessor: for scale
the host time of the numpy twin for 1000 pairs stands beside them.  With hipcc on PATH the compiler's resource report of
csrc/box_overlap.hip (VGPRs, LDS, scratch) is put in front.

    python tools/bench_box_overlap.py [--steps 20] [--warmup 3] [--out profiles/box_overlap_ab.txt]
"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rgbmanip_amd import _lib, boxes  # noqa: E402

SIGNS = np.array([[1, 1, 1], [1, 1, -1], [-1, 1, 1], [-1, 1, -1], [1, -1, 1], [1, -1, -1], [-1, -1, 1], [-1, -1, -1]], dtype=np.float64)


def rotations(rng, shape, near=None, spread=0.12):
    """random rotations [*shape, 3, 3]; with `near` [.., 3, 3]: rotations a few degrees from it"""
    m = rng.normal(size=shape + (3, 3)) if near is None else near + spread * rng.normal(size=shape + (3, 3))
    q, r = np.linalg.qr(m)
    q = q * np.sign(np.diagonal(r, axis1=-2, axis2=-1))[..., None, :]
    return q * np.sign(np.linalg.det(q))[..., None, None]


def box_sets(rng, n, m):
    """[n, m, 8, 3]: per pose m boxes around one box (sizes +-10 %, a few degrees, offsets of a fifth of the size), metres from the origin"""
    size = rng.uniform(0.1, 1.0, size=(n, 1, 3))
    t = rng.uniform(-6.0, 6.0, size=(n, 1, 3))
    R = rotations(rng, (n, m), near=np.broadcast_to(rotations(rng, (n, 1)), (n, m, 3, 3)))
    half = SIGNS[None, None] * (size * rng.uniform(0.9, 1.1, size=(n, m, 3)))[:, :, None, :] / 2
    return np.einsum("nmkj,nmij->nmki", half, R) + (t + size * rng.uniform(-0.2, 0.2, size=(n, m, 3)))[:, :, None, :]


def event_ms(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def resource_report():
    """the kernel-resource-usage remarks of box_overlap.hip, compiled with build.sh's flags for this file: one line per kernel"""
    if shutil.which("hipcc") is None:
        return ["# resource report: hipcc not on PATH"]
    src = os.path.join(ROOT, "rgbmanip_amd", "csrc", "box_overlap.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops",
               "-ffp-contract=off", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(tmp, "bo.o")]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        return ["# resource report: hipcc failed", *("# " + ln for ln in r.stderr.splitlines()[-5:])]
    lines, cur = ["# hipcc -Rpass-analysis=kernel-resource-usage, csrc/box_overlap.hip with build.sh's flags (gfx950):"], None
    for ln in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?) \[-Rpass-analysis", ln)
        if not m:
            continue
        text = m.group(1).strip()
        if text.startswith("Function Name:"):
            name = text.split(":", 1)[1].strip()
            cur = {"kernel": "box_agreement_kernel" if "box_agreement" in name else "box_iou_matrix_kernel" if "box_iou_matrix" in name else name}
            lines.append(cur)
        elif cur is not None and ":" in text:
            k, v = text.split(":", 1)
            cur[k.strip()] = v.strip()
    keys = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")
    return [ln if isinstance(ln, str) else f"#   {ln['kernel']}: " + ", ".join(f"{k} {ln.get(k, '?')}" for k in keys) for ln in lines]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_overlap_ab.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_box_overlap needs a GPU: no timing is taken without one")
    lib = _lib.load()
    rng = np.random.default_rng(0)
    lines = [f"# tools/bench_box_overlap.py: device events around the C call, outputs allocated beforehand; warmup {args.warmup}, median of {args.steps}",
             *resource_report(),
             f"{'call':<20} {'n':>6} {'P':>3} {'Q':>3} {'pairs':>9} {'ms: median (min .. max)':>30} {'ns per pair':>12} {'mean IoU':>9}"]
    fmt = lambda t: f"{t[0]:8.3f} ({t[1]:.3f} .. {t[2]:.3f})"      # noqa: E731
    st = _lib.stream_ptr()
    # the matrix: every pair of the 64 samples of 256 poses
    n, P = 256, 64
    a = torch.from_numpy(box_sets(rng, n, P)).cuda()
    iou = torch.empty(n, P, P, dtype=torch.float64, device="cuda")
    t = event_ms(lambda: _lib.check(lib.rgbm_box_iou_matrix(_lib.ptr(a), _lib.ptr(a), None, None, n, P, P, _lib.ptr(iou), st)), args.warmup, args.steps)
    rows = [{"call": "rgbm_box_iou_matrix", "n": n, "P": P, "Q": P, "pairs": n * P * P, "ms": t, "mean_iou": float(iou.mean())}]
    # pairs: box 0 of a pose against its box 1
    for n in (256, 65535):
        s = torch.from_numpy(box_sets(rng, n, 2)).cuda()
        x, y = s[:, 0].contiguous(), s[:, 1].contiguous()
        out = {"valid": torch.empty(n, dtype=torch.int32, device="cuda")}
        out.update({k: torch.empty(n, *shp, dtype=torch.float64, device="cuda") for k, shp in boxes._SHAPES.items()})
        ptrs = [_lib.ptr(out[k]) for k in boxes.AGREEMENT_KEYS]
        t = event_ms(lambda: _lib.check(lib.rgbm_box_agreement(_lib.ptr(x), _lib.ptr(y), None, None, n, *ptrs, st)), args.warmup, args.steps)
        rows.append({"call": "rgbm_box_agreement", "n": n, "P": 1, "Q": 1, "pairs": n, "ms": t, "mean_iou": float(out["iou"].mean())})
    for r in rows:
        print(json.dumps(r), flush=True)
        lines.append(f"{r['call']:<20} {r['n']:>6} {r['P']:>3} {r['Q']:>3} {r['pairs']:>9} {fmt(r['ms']):>30} {r['ms'][0] * 1e6 / r['pairs']:>12.2f} "
                     f"{r['mean_iou']:>9.3f}")
    # for scale: the numpy twin on the host
    s = box_sets(rng, 1000, 2)
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        ref = boxes.box_agreement_ref(s[:, 0], s[:, 1])
        ts.append((time.perf_counter() - t0) * 1e3)
    got = boxes.box_agreement(s[:, 0], s[:, 1])["iou"].cpu().numpy()
    lines.append(f"{'box_agreement_ref':<20} {1000:>6} {1:>3} {1:>3} {1000:>9} {fmt((float(np.median(ts)), min(ts), max(ts))):>30} "
                 f"{float(np.median(ts)) * 1e6 / 1000:>12.2f} {float(ref['iou'].mean()):>9.3f}   (numpy twin, host, 5 runs; max |kernel - twin| iou "
                 f"{float(np.abs(got - ref['iou']).max()):.1e})")
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
