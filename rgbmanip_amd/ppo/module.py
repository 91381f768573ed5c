"""ActorCritic on a flat fp32 parameter vector, evaluated by the HIP policy kernels.

Mirrors `/root/reference/algo/ppo/ppo/module.py:8-107`: same constructor arguments, `act`, `act_inference`,
`evaluate`, `state_dict` key names (`log_std`, `actor.{0,2,..}.{weight,bias}`, `critic.{0,2,..}.{weight,bias}`) for any depth,
every hidden-size list, activation name and the asymmetric critic the reference builds, orthogonal initialisation with the
reference's gains drawn in its order, and the reference's Gaussian (`scale_tril = diag(exp(log_std)**2)`, module.py:76-77).
Sampling noise is drawn from torch's generator (`torch.randn`) so RNG stays with the caller; everything else runs in
`rgbm_policy_forward_ex`.
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn

from .. import _lib


_ACTIVATIONS = {"elu": nn.ELU, "selu": nn.SELU, "relu": nn.ReLU, "crelu": nn.ReLU, "lrelu": nn.LeakyReLU, "tanh": nn.Tanh,
                "sigmoid": nn.Sigmoid}


def get_activation(act_name):
    """The reference's names (module.py:109-126); an unknown one is an error here, not a `None` inside `nn.Sequential`."""
    if act_name not in _ACTIVATIONS:
        raise ValueError(f"unknown activation {act_name!r}: expected one of {sorted(_ACTIVATIONS)}")
    return _ACTIVATIONS[act_name]()


class ActorCritic:
    def __init__(self, obs_shape, states_shape, actions_shape, initial_std, model_cfg, asymmetric=False):
        self.asymmetric = bool(asymmetric)
        if model_cfg is None:      # module.py:15-18
            a_h, c_h, act_name = [256, 256, 256], [256, 256, 256], "selu"
        else:
            a_h, c_h, act_name = list(model_cfg["pi_hid_sizes"]), list(model_cfg["vf_hid_sizes"]), model_cfg["activation"]
        get_activation(act_name)
        self.activation = act_name
        self.obs_dim, self.act_dim = int(obs_shape[0]), int(actions_shape[0])
        self.state_dim = int(states_shape[0]) if self.asymmetric else self.obs_dim
        a_h, c_h = [int(h) for h in a_h], [int(h) for h in c_h]
        for name, hid in (("pi_hid_sizes", a_h), ("vf_hid_sizes", c_h)):
            if not 1 <= len(hid) <= _lib.POLICY_MAX_HIDDEN or not all(1 <= h <= _lib.POLICY_MAX_WIDTH for h in hid):
                raise ValueError(f"{name}={hid}: the policy kernels take 1..{_lib.POLICY_MAX_HIDDEN} hidden layers of width "
                                 f"1..{_lib.POLICY_MAX_WIDTH}")
        if not (1 <= self.obs_dim <= _lib.POLICY_MAX_WIDTH and 1 <= self.state_dim <= _lib.POLICY_MAX_WIDTH
                and 1 <= self.act_dim <= _lib.POLICY_MAX_ACT):
            raise ValueError(f"observation / state dim must be in 1..{_lib.POLICY_MAX_WIDTH} and action dim in 1..{_lib.POLICY_MAX_ACT}")
        self.hidden = a_h
        self.critic_hidden = c_h
        a_dims = [self.obs_dim] + a_h + [self.act_dim]
        c_dims = [self.state_dim if self.asymmetric else self.obs_dim] + c_h + [1]
        # ---- layout of the flat vector = the reference's state_dict order ----
        self.keys = OrderedDict()
        off = 0
        self.keys["log_std"] = (off, (self.act_dim,))
        off += self.act_dim
        D = _lib.PolicyDesc()
        D.obs_dim, D.state_dim, D.act_dim = self.obs_dim, self.state_dim, self.act_dim
        D.activation, D.asymmetric, D.log_std = _lib.POLICY_ACTIVATIONS[act_name], int(self.asymmetric), 0
        for net, (name, dims) in enumerate((("actor", a_dims), ("critic", c_dims))):
            D.n_hidden[net] = len(dims) - 2
            for l in range(len(dims) - 1):
                i, o = dims[l], dims[l + 1]
                if l < len(dims) - 2:
                    D.hidden[net][l] = o
                self.keys[f"{name}.{2 * l}.weight"] = (off, (o, i))
                D.w[net][l] = off
                off += o * i
                self.keys[f"{name}.{2 * l}.bias"] = (off, (o,))
                D.b[net][l] = off
                off += o
        D.total = off
        self.desc = D
        self.total = off
        # the shipped shape's descriptor, for callers of the four original entry points
        self.layout = None
        if a_h == c_h and len(a_h) == 3 and not self.asymmetric:
            L = _lib.PolicyLayout()
            for k, d in enumerate(a_dims):
                L.dims[k] = d
            L.log_std = 0
            for net in range(2):
                for l in range(4):
                    L.w[net][l], L.b[net][l] = D.w[net][l], D.b[net][l]
            L.total = off
            self.layout = L
        # ---- initialisation exactly like the reference: nn.Linear defaults, then orthogonal_ with its gains ----
        actor = [nn.Linear(a_dims[l], a_dims[l + 1]) for l in range(len(a_dims) - 1)]
        critic = [nn.Linear(c_dims[l], c_dims[l + 1]) for l in range(len(c_dims) - 1)]
        log_std = np.log(initial_std) * torch.ones(self.act_dim)
        for mods, gains in ((actor, [np.sqrt(2)] * len(a_h) + [0.01]), (critic, [np.sqrt(2)] * len(c_h) + [1.0])):
            for m, gain in zip(mods, gains):
                torch.nn.init.orthogonal_(m.weight, gain=gain)
        flat = torch.zeros(off, dtype=torch.float32)
        flat[: self.act_dim] = log_std
        for name, mods in (("actor", actor), ("critic", critic)):
            for l, m in enumerate(mods):
                o, shp = self.keys[f"{name}.{2 * l}.weight"]
                flat[o:o + m.weight.numel()] = m.weight.detach().reshape(-1)
                o, shp = self.keys[f"{name}.{2 * l}.bias"]
                flat[o:o + m.bias.numel()] = m.bias.detach()
        self.flat = flat
        self.device = torch.device("cpu")
        self.training = True

    # ---- nn.Module-like plumbing used by PPO / RLPoseController ----
    def to(self, device):
        self.device = torch.device(device)
        self.flat = self.flat.to(self.device).contiguous()
        return self

    def train(self):
        self.training = True
        return self

    def eval(self):
        self.training = False
        return self

    def parameters(self):
        return [self.flat]

    @property
    def log_std(self):
        return self.flat[: self.act_dim]

    def state_dict(self):
        return OrderedDict((k, self.flat[o:o + int(np.prod(s))].view(*s).clone()) for k, (o, s) in self.keys.items())

    def load_state_dict(self, sd, strict=True):
        missing = [k for k in self.keys if k not in sd]
        extra = [k for k in sd if k not in self.keys]
        if strict and (missing or extra):
            raise RuntimeError(f"state_dict mismatch: missing {missing}, unexpected {extra}")
        for k, (o, s) in self.keys.items():
            if k in sd:
                v = torch.as_tensor(sd[k]).to(device=self.flat.device, dtype=torch.float32)
                if tuple(v.shape) != tuple(s):
                    raise RuntimeError(f"size mismatch for {k}: {tuple(v.shape)} vs {tuple(s)}")
                self.flat[o:o + v.numel()] = v.reshape(-1)

    def forward(self):
        raise NotImplementedError

    # ---- the three entry points of module.py:73-107 ----
    def _run(self, mode, observations, states=None, noise=None, actions=None):
        if self.flat.device.type != "cuda":
            raise _lib.RgbmError("ActorCritic runs on the HIP policy kernels only: move it to a cuda device (no CPU fallback)")
        lib = _lib.load()
        obs = observations.to(device=self.flat.device, dtype=torch.float32).contiguous()
        n = obs.shape[0]
        dev = self.flat.device
        st = None
        if self.asymmetric and mode != 1:
            if states is None:
                raise ValueError("an asymmetric ActorCritic needs `states` for act / evaluate")
            st = states.to(device=dev, dtype=torch.float32).contiguous()
            if st.shape != (n, self.state_dim):
                raise ValueError(f"states must be [{n}, {self.state_dim}], got {tuple(st.shape)}")
        mu = torch.empty(n, self.act_dim, device=dev)
        logp = torch.empty(n, device=dev)
        value = torch.empty(n, 1, device=dev)
        if mode == 0:
            actions = torch.empty(n, self.act_dim, device=dev)
        elif mode == 2:
            actions = actions.to(device=dev, dtype=torch.float32).contiguous()
        _lib.check(lib.rgbm_policy_forward_ex(_lib.ptr(self.flat), C.byref(self.desc), n, mode, _lib.ptr(obs), _lib.ptr(st),
                                              _lib.ptr(noise), _lib.ptr(actions), _lib.ptr(logp), _lib.ptr(value), _lib.ptr(mu),
                                              _lib.stream_ptr()), "rgbm_policy_forward_ex")
        return actions, logp, value, mu

    def act(self, observations, states, noise=None):
        n = observations.shape[0]
        if noise is None:
            noise = torch.randn(n, self.act_dim, device=self.flat.device)
        noise = noise.to(device=self.flat.device, dtype=torch.float32).contiguous()
        actions, logp, value, mu = self._run(0, observations, states=states, noise=noise)
        return actions, logp, value, mu, self.log_std.repeat(n, 1).detach()

    def act_inference(self, observations):
        return self._run(1, observations)[3]

    def evaluate(self, observations, states, actions, contrastive=False):
        n = observations.shape[0]
        _, logp, value, mu = self._run(2, observations, states=states, actions=actions)
        k = self.act_dim
        entropy = (0.5 * k * (1.0 + np.log(2 * np.pi)) + 2.0 * self.log_std.sum()).expand(n)
        return logp, entropy, value, mu, self.log_std.repeat(n, 1), 0
