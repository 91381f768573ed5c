#!/usr/bin/env python3
"""A/B of the synthetic camera delivering bytes (rgbm_synth_render_u8, cfg controller.hip_render_to_queue) on one device, in ONE
process, A and B blocks alternating.

    python tools/bench_synth_u8.py [--envs 512] [--rounds 5] [--out profiles/synth_render_u8_ab.txt]

A is always the path as it stood before this option existed, unchanged in this tree and never a variant of the new code:

  (1) the camera alone:   A  SyntheticMultiVecEnv.get_image() with the float32 `Color` (rgbm_synth_camera + rgbm_synth_render)
                          B  the same env built with color_dtype="uint8" (rgbm_synth_camera + rgbm_synth_render_u8, no extent)
  (2) a controller step:  A  ControlInterface.step on the byte queue (hip_queue_dtype "uint8"): get_image() -> rgbm_quantize_frames ->
                             mask pass and copies -> rgbm_mask_extent
                          B  the same with hip_render_to_queue: env.render_into() straight into the queue slot
      once with the bf16 estimator in the loop and once with the estimator stubbed out (a constant box per env), which leaves the
      camera, the queue and the reward.

A block is `--calls` get_image() calls or `--steps` controller steps (whole episodes) of one side; its figure is the median wall time per
call with a device synchronisation after every call.  Blocks run A B A B ... for `--rounds` rounds after one warm-up block per side.
The table gives every block's figure, the median over blocks per side and the spread (min .. max) of the A blocks: B "holds" when its
median is not above the slowest A block of the same run."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _block_ms(fn, calls):
    import torch
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 3)


def _alternate(sides, calls, rounds):
    """sides: {"A": fn, "B": fn} -> {"A": [block medians], "B": [...]}; one warm-up block per side, then A B A B ..."""
    out = {k: [] for k in sides}
    for k, fn in sides.items():
        _block_ms(fn, calls)
    for _ in range(rounds):
        for k, fn in sides.items():
            out[k].append(_block_ms(fn, calls))
    return out


class _StubEstimator:
    """The estimator taken out of the step: a constant box per env, no kernel."""

    def __init__(self, n, device):
        import torch
        self.cfg = {"task_name": "cabinet"}
        g = torch.Generator().manual_seed(0)
        self.boxes = (torch.rand(n, 8, 3, generator=g, dtype=torch.float64) + 0.5).to(device)

    def estimate_device_indexed(self, *a, **k):
        return self.boxes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10, help="get_image() calls per block")
    ap.add_argument("--steps", type=int, default=0, help="controller steps per block (default: two episodes)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "synth_render_u8_ab.txt"))
    a = ap.parse_args()
    import torch
    from rgbmanip_amd import synth
    from rgbmanip_amd.config import ADAPOSE_CFGS
    from rgbmanip_amd.control_interface import ControlInterface
    from rgbmanip_amd.estimator import AdaPoseEstimator_v5
    from rgbmanip_amd.synthetic_env import SyntheticManipulation, SyntheticMultiVecEnv
    dev = torch.device("cuda", 0)
    n = a.envs
    res = {}
    # (1) the camera alone
    envs = {"A": SyntheticMultiVecEnv(n, dev, seed=0, episodes=8), "B": SyntheticMultiVecEnv(n, dev, seed=0, episodes=8, color_dtype="uint8")}
    res["1_get_image"] = _alternate({k: e.get_image for k, e in envs.items()}, a.calls, a.rounds)
    del envs
    torch.cuda.empty_cache()
    # (2) the controller step
    est_bf16 = AdaPoseEstimator_v5(None, dict(ADAPOSE_CFGS["adapose_cabinet"], load=False, hip_prepare="device"), None,
                                   state_dict=synth.adapose_state_dict(seed=0, prefix="module."), dtype="bf16")
    for name, est in (("2_step_stub_estimator", _StubEstimator(n, dev)), ("3_step_bf16_estimator", est_bf16)):
        sides = {}
        hold = []
        for side in ("A", "B"):
            cfg = synth.control_cfg("cabinet", 0.0)
            cfg["controller"]["hip_queue_dtype"] = "uint8"
            if side == "B":
                cfg["controller"]["hip_render_to_queue"] = True
            venv = SyntheticMultiVecEnv(n, dev, seed=0, episodes=8)
            ci = ControlInterface(venv, est, SyntheticManipulation(venv), cfg, device=dev)
            acts = [torch.from_numpy(synth.control_actions(n, s, 9) * 0.3).to(dev) for s in range(ci.max_steps)]
            state = {"i": 0}

            def one(ci=ci, acts=acts, state=state):
                state["i"] += 1
                return ci.step(acts[state["i"] % len(acts)])
            sides[side] = one
            hold.append(ci)
        steps = a.steps or 2 * hold[0].max_steps
        res[name] = _alternate(sides, steps, a.rounds)
        res[name + "_steps_per_block"] = steps
        del sides, hold
        torch.cuda.empty_cache()
    report(res, a, torch.cuda.get_device_name(0))


def report(res, a, device_name):
    rows = [f"Synthetic camera delivering bytes: A (the path before the option) against B, one process on {device_name}, {a.envs} envs,",
            f"{a.rounds} alternating rounds (tools/bench_synth_u8.py --envs {a.envs} --rounds {a.rounds} --calls {a.calls}); figures: median wall ms per call of a block",
            "(device synchronised after every call), per block | median over blocks; A spread = fastest .. slowest A block", ""]
    label = {"1_get_image": "get_image(): float32 Color (A) / color_dtype uint8 (B)",
             "2_step_stub_estimator": "ControlInterface.step, byte queue, estimator stubbed out: add_view (A) / hip_render_to_queue (B)",
             "3_step_bf16_estimator": "ControlInterface.step, byte queue, bf16 estimator: add_view (A) / hip_render_to_queue (B)"}
    for k, text in label.items():
        A, B = res[k]["A"], res[k]["B"]
        ma, mb = statistics.median(A), statistics.median(B)
        rows.append(text + (f"  [{res[k + '_steps_per_block']} steps per block]" if k + "_steps_per_block" in res else f"  [{a.calls} calls per block]"))
        rows.append("  A  " + " ".join(f"{v:g}" for v in A) + f" | {ma:g}    spread {min(A):g} .. {max(A):g}")
        rows.append("  B  " + " ".join(f"{v:g}" for v in B) + f" | {mb:g}")
        verdict = "holds (B's median is not above the slowest A block)" if mb <= max(A) else "B IS SLOWER than every A block"
        rows.append(f"  B / A = {mb / ma:.3f} ({(mb / ma - 1) * 100:+.1f} %, A - B = {ma - mb:+.3f} ms per call): {verdict}")
        rows.append("")
    text = "\n".join(rows)
    print(text)
    print("RESULT " + json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
