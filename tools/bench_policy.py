"""Times `PPO.update` (8 epochs x 4 minibatches over 512 envs x 16 steps) with HIP events: median of the timed calls after warm-up.

usage: bench_policy.py [shipped|default|torch-default ...] [--calls 20] [--warmup 3] [--rounds 1]
  shipped        the shipped policy (60 -> 96-96-32 -> 12 / 1, ELU)
  default        the class default (model_cfg=None: 256-256-256 SELU)
  torch-default  the yardstick for `default`: the same update written in eager torch on the same GPU (nn.Sequential, the
                 Gaussian in closed form, torch.optim.Adam, clip_grad_norm_, the adaptive-LR rule with its two host reads)
Several names are interleaved round by round (--rounds) in one process; one JSON line per (round, name).  To time another build of the
package, put its directory first on PYTHONPATH: the tool imports `rgbmanip_amd` from wherever Python finds it first.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn as nn

try:
    import rgbmanip_amd  # noqa: F401
except ImportError:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rgbmanip_amd import synth  # noqa: E402
from rgbmanip_amd.ppo import PPO  # noqa: E402
from rgbmanip_amd.spaces import Box  # noqa: E402

T, N = 16, 512
LEARN = dict(exp_name="PPO", reset=True, num_transitions_per_env=T, num_transitions_eval=512, num_learning_epochs=8,
             num_mini_batches=4, clip_range=0.2, gamma=0.98, lam=0.98, init_noise_std=0.6, value_loss_coef=1.0, entropy_coef=0.0,
             learning_rate=0.00001, max_grad_norm=1.0, use_clipped_value_loss=True, schedule="adaptive", desired_kl=0.016,
             max_lr=0.005, min_lr=0.0002, device="cuda", sampler="sequential", log_dir="/tmp/rgbm_logs", save_dir="/tmp/rgbm_saves",
             testing=False, eval_interval=64, eval_round=16, eval=False, print_log=False, contrastive=False, contrastive_m=0.99,
             asymmetric=False)
SHAPES = {"shipped": ([96, 96, 32], "elu", nn.ELU), "default": ([256, 256, 256], "selu", nn.SELU)}


class FakeEnv:
    num_envs = N
    observation_space, state_space, action_space = Box(-1.5, 1.5, (60,)), Box(-1.5, 1.5, (75,)), Box(-1.5, 1.5, (12,))


def make_ppo(shape):
    hid, act, _ = SHAPES[shape]
    torch.manual_seed(0)
    ppo = PPO(FakeEnv(), {"learn": dict(LEARN), "policy": dict(actor_critic_class="ActorCritic", pi_hid_sizes=hid, vf_hid_sizes=hid,
                                                               activation=act), "load": ""})
    tr = {k: torch.from_numpy(v).cuda() for k, v in synth.ppo_rollout(T, N, seed=0).items()}
    for t in range(T):
        lp, _, _, mm, ss, _ = ppo.actor_critic.evaluate(tr["observations"][t], None, tr["actions"][t])
        ppo.storage.add_transitions(tr["observations"][t], tr["states"][t], tr["actions"][t], tr["rewards"][t].view(-1),
                                    tr["dones"][t].view(-1), tr["values"][t], lp - 0.01, mm + 0.02, ss - 0.005)
    ppo.storage.compute_returns(tr["last_values"], 0.98, 0.98)
    return ppo


class TorchUpdate:
    """The reference's update (ppo.py:449-534) in eager torch on the device, fed from the same storage."""

    def __init__(self, ppo, shape):
        hid, _, act = SHAPES[shape]

        def mlp(out):
            dims, mods = [60] + hid, []
            for a, b in zip(dims[:-1], dims[1:]):
                mods += [nn.Linear(a, b), act()]
            return nn.Sequential(*mods, nn.Linear(dims[-1], out)).cuda()
        self.actor, self.critic = mlp(12), mlp(1)
        self.log_std = nn.Parameter(torch.full((12,), float(np.log(0.6)), device="cuda"))
        self.params = [self.log_std] + list(self.actor.parameters()) + list(self.critic.parameters())
        self.opt = torch.optim.Adam(self.params, lr=LEARN["learning_rate"])
        self.lr = LEARN["learning_rate"]
        self.st = ppo.storage

    def update(self, it):
        st, clip = self.st, LEARN["clip_range"]
        f = {k: getattr(st, k).reshape(T * N, -1) for k in ("observations", "actions", "values", "returns", "actions_log_prob",
                                                             "advantages", "mu", "sigma")}
        mvl = msl = 0.0
        for _ in range(LEARN["num_learning_epochs"]):
            for idx in st.mini_batch_generator(LEARN["num_mini_batches"]):
                b = {k: v[idx.start:idx.stop] for k, v in f.items()}
                mu = self.actor(b["observations"])
                value = self.critic(b["observations"])
                ls = self.log_std
                logp = (-0.5 * (b["actions"] - mu) ** 2 * torch.exp(-4 * ls) - 2 * ls).sum(1) - 6 * float(np.log(2 * np.pi))
                ent = 6 * (1 + float(np.log(2 * np.pi))) + 2 * ls.sum()
                sig = ls.repeat(mu.shape[0], 1)
                kl = torch.sum(sig - b["sigma"] + (torch.square(b["sigma"].exp()) + torch.square(b["mu"] - mu)) /
                               (2.0 * torch.square(sig.exp())) - 0.5, axis=-1).mean()
                if kl > LEARN["desired_kl"] * 2.0:
                    self.lr = max(LEARN["min_lr"], self.lr / 1.5)
                elif kl < LEARN["desired_kl"] / 2.0 and kl > 0.0:
                    self.lr = min(LEARN["max_lr"], self.lr * 1.5)
                for gp in self.opt.param_groups:
                    gp["lr"] = self.lr
                ratio = torch.exp(logp - b["actions_log_prob"].squeeze(1))
                adv = b["advantages"].squeeze(1)
                surr = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1 - clip, 1 + clip)).mean()
                vclip = b["values"] + (value - b["values"]).clamp(-clip, clip)
                vloss = torch.max((value - b["returns"]).pow(2), (vclip - b["returns"]).pow(2)).mean()
                loss = surr + LEARN["value_loss_coef"] * vloss - LEARN["entropy_coef"] * ent
                self.opt.zero_grad()
                loss.backward()
                nn.utils.clip_grad_norm_(self.params, LEARN["max_grad_norm"])
                self.opt.step()
                mvl += vloss.item()
                msl += surr.item()
        return mvl / 32, msl / 32


def time_calls(fn, calls, warmup):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    ms = []
    for i in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(i)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("names", nargs="*", default=["shipped"])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    if a.calls < 20:
        ap.error("--calls must be at least 20")
    runners = {}
    for name in a.names:
        shape = name.replace("torch-", "")
        ppo = make_ppo(shape)
        runners[name] = TorchUpdate(ppo, shape).update if name.startswith("torch-") else ppo.update
    for rnd in range(a.rounds):
        for name, fn in runners.items():
            ms = time_calls(fn, a.calls, a.warmup)
            print(json.dumps(dict(tag=a.tag, name=name, round=rnd, calls=a.calls, median_ms=round(statistics.median(ms), 4),
                                  min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))), flush=True)


if __name__ == "__main__":
    main()
