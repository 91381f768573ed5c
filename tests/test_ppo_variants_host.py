"""CPU-only: layout arithmetic, initialisation and constructor paths of the general ActorCritic / PPO against what the reference
recorded for every variant of rgbmanip_amd.synth.PPO_VARIANTS (tests/golden/ppo_variants.npz, tools/make_goldens.py::gen_ppo_variants)."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

from rgbmanip_amd import _lib, synth
from rgbmanip_amd.ppo import PPO, ActorCritic
from rgbmanip_amd.spaces import Box

VARIANTS = list(synth.PPO_VARIANTS)
LEARN = dict(exp_name="PPO", reset=True, num_transitions_per_env=16, num_transitions_eval=512, num_learning_epochs=8,
             num_mini_batches=4, clip_range=0.2, gamma=0.98, lam=0.98, init_noise_std=0.6, value_loss_coef=1.0, entropy_coef=0.0,
             learning_rate=0.00001, max_grad_norm=1.0, use_clipped_value_loss=True, schedule="adaptive", desired_kl=0.016,
             max_lr=0.005, min_lr=0.0002, device="cpu", sampler="sequential", log_dir="/tmp/rgbm_logs", save_dir="/tmp/rgbm_saves",
             testing=False, eval_interval=64, eval_round=16, eval=False, print_log=False, contrastive=False, contrastive_m=0.99,
             asymmetric=False)


def _build(name):
    mcfg, asym, _ = synth.PPO_VARIANTS[name]
    return ActorCritic((60,), (75,), (12,), 0.6, mcfg, asymmetric=asym)


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "ppo_variants.npz"))


@pytest.mark.parametrize("name", VARIANTS)
def test_layout_matches_reference_state_dict(gold, name):
    ac = _build(name)
    keys = [str(k) for k in gold[name + "_keys"]]
    shapes = [tuple(int(d) for d in row if d > 0) for row in gold[name + "_shapes"]]
    assert list(ac.keys) == keys and keys[0] == "log_std"
    assert list(ac.state_dict().keys()) == keys
    off = 0
    for k, shp in zip(keys, shapes):          # contiguous, in the reference's order, with the reference's shapes
        assert ac.keys[k] == (off, shp), k
        off += int(np.prod(shp))
    assert ac.total == off == ac.desc.total == ac.flat.numel()
    # the descriptor the kernels read says the same
    D = ac.desc
    for net, prefix in enumerate(("actor", "critic")):
        n_lin = D.n_hidden[net] + 1
        assert n_lin == sum(1 for k in keys if k.startswith(prefix) and k.endswith("weight"))
        for l in range(n_lin):
            assert D.w[net][l] == ac.keys[f"{prefix}.{2 * l}.weight"][0] and D.b[net][l] == ac.keys[f"{prefix}.{2 * l}.bias"][0]
            if l < n_lin - 1:
                assert D.hidden[net][l] == ac.keys[f"{prefix}.{2 * l}.weight"][1][0]
    sd = synth.policy_variant_state_dict(name, seed=0)
    assert list(sd) == keys and [tuple(v.shape) for v in sd.values()] == shapes
    # the library accepts the descriptor (argument check on the host, nothing is launched)
    need = C.c_size_t()
    _lib.check(_lib.load().rgbm_ppo_scratch_floats_ex(C.byref(D), 512, 1, C.byref(need)))
    assert need.value >= 8 * (ac.total + 4)


@pytest.mark.parametrize("name", VARIANTS)
def test_same_seed_same_initial_parameters(gold, name):
    torch.manual_seed(1234)
    ac = _build(name)
    flat = ac.flat.numpy()
    step = max(1, flat.size // 256)
    assert np.array_equal(flat[::step][:256], gold[name + "_init_slice"])


def test_unknown_activation_is_a_value_error():
    with pytest.raises(ValueError, match="swish"):
        ActorCritic((60,), (75,), (12,), 0.6, dict(pi_hid_sizes=[8], vf_hid_sizes=[8], activation="swish"))


def test_crelu_is_relu():
    assert _lib.POLICY_ACTIVATIONS["crelu"] == _lib.POLICY_ACTIVATIONS["relu"]
    ac = ActorCritic((60,), (75,), (12,), 0.6, dict(pi_hid_sizes=[8], vf_hid_sizes=[8], activation="crelu"))
    assert ac.desc.activation == _lib.POLICY_ACTIVATIONS["relu"]


def test_shapes_outside_the_kernel_bounds_are_refused_at_construction():
    for pi, vf, act in (([513], [8], 12), ([8] * 7, [8], 12), ([8], [], 12), ([8], [8], 33)):
        with pytest.raises(ValueError):
            ActorCritic((60,), (75,), (act,), 0.6, dict(pi_hid_sizes=pi, vf_hid_sizes=vf, activation="elu"))


class _Env:
    num_envs = 8
    observation_space, state_space, action_space = Box(-1.5, 1.5, (60,)), Box(-1.5, 1.5, (75,)), Box(-1.5, 1.5, (12,))


@pytest.mark.parametrize("override", [dict(contrastive=True), dict(use_clipped_value_loss=False), dict(asymmetric=True)])
def test_ppo_constructor_accepts_the_reference_options(override, tmp_path):
    learn = copy.deepcopy(LEARN)
    learn.update(override, log_dir=str(tmp_path / "l"), save_dir=str(tmp_path / "s"))
    cfg = {"learn": learn, "policy": dict(actor_critic_class="ActorCritic", pi_hid_sizes=[16, 8], vf_hid_sizes=[24], activation="tanh"),
           "load": ""}
    ppo = PPO(_Env(), cfg)
    assert ppo.actor_critic.asymmetric == bool(override.get("asymmetric", False))
    assert ppo.actor_critic.keys["critic.0.weight"][1] == (24, 75 if override.get("asymmetric") else 60)
    assert ppo._grads.numel() == ppo.actor_critic.total + 4 and ppo._exp_avg.numel() == ppo.actor_critic.total


def test_other_policy_classes_stay_refused(tmp_path):
    learn = copy.deepcopy(LEARN)
    learn.update(log_dir=str(tmp_path / "l"), save_dir=str(tmp_path / "s"))
    with pytest.raises(NotImplementedError):
        PPO(_Env(), {"learn": learn, "policy": dict(actor_critic_class="Other", pi_hid_sizes=[8], vf_hid_sizes=[8], activation="elu"),
                     "load": ""})
