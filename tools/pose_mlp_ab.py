"""Same-process A/B of the pose MLP's two kernels (default) against the per-layer launches (rgbm_debug_flags 524288), bf16 forward.
usage: pose_mlp_ab.py [B] [alternations] [forwards per repetition]      default 256 8 5
  every repetition: median of the forwards' times (HIP events around one forward each); the two settings alternate.
       pose_mlp_ab.py trace [B]      three forwards per setting, for a rocprofv3 --kernel-trace --stats run (both kernel sets in one trace)"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from rgbmanip_amd import synth, _lib
from rgbmanip_amd.adapose import AdaPoseNet

FLAG = 524288
lib = _lib.load()
trace = len(sys.argv) > 1 and sys.argv[1] == "trace"
args = [int(a) for a in sys.argv[(2 if trace else 1):]]
B = args[0] if args else 256
alts = args[1] if len(args) > 1 else 8
per = args[2] if len(args) > 2 else 5
net = AdaPoseNet(synth.adapose_state_dict(seed=0), dtype="bf16")
d = {k: torch.from_numpy(v).cuda() for k, v in synth.adapose_inputs(B, seed=0).items()}
fwd = lambda: net(d["img1"], d["choose1"], d["img2"], d["choose2"], d["P1"], d["P2"], d["depths"])


def timed():
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fwd(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1)


if trace:
    for fl in (FLAG, 0):
        lib.rgbm_debug_flags(fl)
        for _ in range(3):
            fwd()
        torch.cuda.synchronize()
    lib.rgbm_debug_flags(0)
    sys.exit(0)
reps = {0: [], FLAG: []}
for fl in (0, FLAG):
    lib.rgbm_debug_flags(fl)
    for _ in range(2):
        fwd()
torch.cuda.synchronize()
for a in range(alts):
    for fl in ((0, FLAG) if a % 2 == 0 else (FLAG, 0)):
        lib.rgbm_debug_flags(fl)
        fwd()
        reps[fl].append(float(np.median([timed() for _ in range(per)])))
lib.rgbm_debug_flags(0)
for fl, name in ((0, "two kernels"), (FLAG, "per-layer launches")):
    r = reps[fl]
    print(f"bf16 B={B} {name}: median {np.median(r):.3f} ms, range {min(r):.3f} .. {max(r):.3f} ms, repetitions {[round(x, 3) for x in r]}", flush=True)
print("ranges disjoint (slowest two-kernel repetition faster than the fastest per-layer one):", max(reps[0]) < min(reps[FLAG]))
