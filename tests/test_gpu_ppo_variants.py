"""-m gpu: the general ActorCritic / PPO (any hidden-size lists, every activation, asymmetric critic, plain-MSE value loss) against
the reference's own outputs (tests/golden/ppo_variants.npz, tools/make_goldens.py::gen_ppo_variants), float64 and torch autograd."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

from rgbmanip_amd import _lib, synth  # noqa: E402
from rgbmanip_amd.spaces import Box  # noqa: E402

VARIANTS = list(synth.PPO_VARIANTS)
LEARN = dict(exp_name="PPO", reset=True, num_transitions_per_env=16, num_transitions_eval=512, num_learning_epochs=8,
             num_mini_batches=4, clip_range=0.2, gamma=0.98, lam=0.98, init_noise_std=0.6, value_loss_coef=1.0, entropy_coef=0.0,
             learning_rate=0.00001, max_grad_norm=1.0, use_clipped_value_loss=True, schedule="adaptive", desired_kl=0.016,
             max_lr=0.005, min_lr=0.0002, device="cuda", sampler="sequential", log_dir="/tmp/rgbm_logs", save_dir="/tmp/rgbm_saves",
             testing=False, eval_interval=64, eval_round=16, eval=False, print_log=False, contrastive=False, contrastive_m=0.99,
             asymmetric=False)
_ACT = {"elu": nn.ELU, "selu": nn.SELU, "relu": nn.ReLU, "crelu": nn.ReLU, "lrelu": nn.LeakyReLU, "tanh": nn.Tanh, "sigmoid": nn.Sigmoid}
U32 = 2.0 ** -24


class FakeEnv:
    def __init__(self, n):
        self.num_envs = n
        self.observation_space, self.state_space, self.action_space = Box(-1.5, 1.5, (60,)), Box(-1.5, 1.5, (75,)), Box(-1.5, 1.5, (12,))


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-12))


def _cfg(name, **learn):
    mcfg, asym, clipped = synth.PPO_VARIANTS[name]
    lc = copy.deepcopy(LEARN)
    lc.update(asymmetric=asym, use_clipped_value_loss=clipped)
    lc.update(learn)
    pol = dict(actor_critic_class="ActorCritic", **(mcfg or dict(pi_hid_sizes=[256] * 3, vf_hid_sizes=[256] * 3, activation="selu")))
    return {"learn": lc, "policy": pol, "load": ""}


def _ppo(name, N, **learn):
    from rgbmanip_amd.ppo import PPO
    ppo = PPO(FakeEnv(N), _cfg(name, **learn))
    ppo.actor_critic.load_state_dict({k: torch.from_numpy(v) for k, v in synth.policy_variant_state_dict(name, seed=0).items()})
    return ppo


def _seq64(sd, prefix, act):
    """The reference's nn.Sequential of one net (module.py:24-49) in float64 from a state dict."""
    n_lin = sum(1 for k in sd if k.startswith(prefix) and k.endswith("weight"))
    mods = []
    for l in range(n_lin):
        w = torch.as_tensor(sd[f"{prefix}.{2 * l}.weight"]).double()
        lin = nn.Linear(w.shape[1], w.shape[0]).double()
        with torch.no_grad():
            lin.weight.copy_(w)
            lin.bias.copy_(torch.as_tensor(sd[f"{prefix}.{2 * l}.bias"]).double())
        mods.append(lin)
        if l < n_lin - 1:
            mods.append(_ACT[act]())
    return nn.Sequential(*mods)


def _evaluate64(actor, critic, log_std, obs, critic_in, actions):
    """module.py:93-107 in closed form: MultivariateNormal(mu, scale_tril=diag(exp(log_std)^2))."""
    mu = actor(obs.double())
    ls = log_std.double()
    k = mu.shape[1]
    logp = (-0.5 * ((actions.double() - mu) ** 2) * torch.exp(-4 * ls) - 2 * ls).sum(1) - 0.5 * k * np.log(2 * np.pi)
    ent = (0.5 * k * (1 + np.log(2 * np.pi)) + 2 * ls.sum()).expand(mu.shape[0])
    return logp, ent, critic(critic_in.double()), mu


def _variant_nets64(name):
    mcfg, asym, _ = synth.PPO_VARIANTS[name]
    sd = synth.policy_variant_state_dict(name, seed=0)
    act = "selu" if mcfg is None else mcfg["activation"]
    return _seq64(sd, "actor", act), _seq64(sd, "critic", act), torch.from_numpy(sd["log_std"]), asym


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "ppo_variants.npz"))


@pytest.mark.parametrize("name", VARIANTS)
def test_act_evaluate_match_reference_golden(gold, name):
    """Gate of tests/test_gpu_ppo.py: tensor-normalised max error < 1e-5 against the reference's float32 CPU outputs.  Printed next to
    each figure: the reference golden's own distance from the same forward in float64."""
    ppo = _ppo(name, 32)
    ac = ppo.actor_critic
    roll = synth.ppo_rollout(16, 32, seed=0)
    obs, st = torch.from_numpy(roll["observations"][0]).cuda(), torch.from_numpy(roll["states"][0]).cuda()
    act = torch.from_numpy(roll["actions"][0])
    g = lambda k: gold[f"{name}_{k}"]  # noqa: E731
    a, logp, v, mu, sig = ac.act(obs, st, noise=torch.from_numpy(g("act_eps")))
    lp, ent, vv, mu2, _, zero = ac.evaluate(obs, st, act.cuda())
    inf = ac.act_inference(obs)
    torch.cuda.synchronize()
    actor, critic, ls, asym = _variant_nets64(name)
    with torch.no_grad():
        lp64, _, v64, mu64 = _evaluate64(actor, critic, ls, obs.cpu(), (st if asym else obs).cpu(), act)
    print(f"{name}: golden vs float64: logp {_rel(g('eval_logp'), lp64):.2e} value {_rel(g('eval_v'), v64):.2e} mu {_rel(g('act_mu'), mu64):.2e}")
    print(f"{name}: device vs float64: logp {_rel(lp.cpu(), lp64):.2e} value {_rel(vv.cpu(), v64):.2e} mu {_rel(mu.cpu(), mu64):.2e}")
    figs = dict(a=_rel(a.cpu(), g("act_a")), logp=_rel(logp.cpu(), g("act_logp")), v=_rel(v.cpu(), g("act_v")), mu=_rel(mu.cpu(), g("act_mu")),
                eval_logp=_rel(lp.cpu(), g("eval_logp")), eval_ent=_rel(ent.cpu(), g("eval_ent")), eval_v=_rel(vv.cpu(), g("eval_v")),
                inference=_rel(inf.cpu(), g("act_mu")))
    print(f"{name}: device vs golden: {figs}")
    assert all(x < 1e-5 for x in figs.values()), figs
    assert sig.shape == (32, 12) and zero == 0 and torch.equal(mu, mu2) and torch.equal(inf, mu)


def _fill_and_update(ppo, N, T=16):
    """Same storage fill as tools/make_goldens.py::gen_ppo_variants."""
    roll = synth.ppo_rollout(T, N, seed=0)
    tr = {k: torch.from_numpy(v).cuda() for k, v in roll.items()}
    ac = ppo.actor_critic
    for t in range(T):
        lp, _, _, mm, ss, _ = ac.evaluate(tr["observations"][t], tr["states"][t], tr["actions"][t])
        mm = mm + 0.02 * torch.sin(torch.arange(12.0)).cuda()[None]
        ppo.storage.add_transitions(tr["observations"][t], tr["states"][t], tr["actions"][t], tr["rewards"][t].view(-1),
                                    tr["dones"][t].view(-1), tr["values"][t], lp - 0.01, mm, ss - 0.005)
    ppo.storage.compute_returns(tr["last_values"], 0.98, 0.98)
    return ppo.update(0)


@pytest.mark.parametrize("name", VARIANTS)
def test_update_matches_reference_golden(gold, name):
    """Recorded rollout -> compute_returns -> 32 optimiser steps at N = 32, at the tolerances of tests/test_gpu_ppo.py."""
    ppo = _ppo(name, 32)
    mvl, msl = _fill_and_update(ppo, 32)
    flat = ppo.actor_critic.flat.cpu().numpy()
    g = lambda k: gold[f"{name}_{k}"]  # noqa: E731
    step = max(1, flat.size // 2048)
    perr = _rel(flat[::step][:2048], g("params_after_slice"))
    print(f"{name}: value loss {mvl} vs {float(g('mvl'))}; surrogate {msl} vs {float(g('msl'))}; lr {ppo.step_size} vs {float(g('lr_after'))}; "
          f"parameters {perr:.2e}")
    assert abs(mvl - float(g("mvl"))) < 1e-3 * abs(float(g("mvl")))
    assert abs(msl - float(g("msl"))) < 2e-3 * abs(float(g("msl"))) + 1e-5
    assert abs(ppo.step_size - float(g("lr_after"))) < 1e-9 + 1e-6 * float(g("lr_after"))
    assert perr < 2e-3


def _desc(obs_dim, state_dim, act_dim, pi, vf, activation, asym):
    from rgbmanip_amd.ppo import ActorCritic
    return ActorCritic((obs_dim,), (state_dim,), (act_dim,), 0.6, dict(pi_hid_sizes=pi, vf_hid_sizes=vf, activation=activation),
                       asymmetric=asym)


def _grad_case(ac, n, clipped, seed=5, clip=0.2, vcoef=1.0, ecoef=0.01):
    """One minibatch through rgbm_ppo_minibatch_fwd_bwd_ex and through float64 autograd on the reference's loss (ppo.py:497-513).
    Returns (device gradient + statistics, float64 gradient, float64 surrogate, float64 value loss, device evaluate, float64 evaluate)."""
    lib = _lib.load()
    gen = torch.Generator().manual_seed(seed)
    A = ac.act_dim
    obs = torch.rand(n, ac.obs_dim, generator=gen) * 2 - 1
    st = torch.rand(n, ac.state_dim, generator=gen) * 2 - 1
    act = torch.randn(n, A, generator=gen) * 0.5
    sd = ac.state_dict()
    actor, critic = _seq64(sd, "actor", ac.activation), _seq64(sd, "critic", ac.activation)
    ls = sd["log_std"].double().requires_grad_(True)
    cin = st if ac.asymmetric else obs
    with torch.no_grad():
        lp0, _, v0, mu0 = _evaluate64(actor, critic, ls, obs, cin, act)
    f32 = lambda t: t.float()  # noqa: E731
    old_logp = f32(lp0 + 0.3 * torch.randn(n, generator=gen).double())         # large enough to hit both clip branches
    adv = torch.randn(n, generator=gen)
    ret = f32(v0.squeeze(1)) + torch.randn(n, generator=gen)
    old_v = f32(v0.squeeze(1)) + 0.3 * torch.randn(n, generator=gen)            # both sides of the value clip
    old_mu = f32(mu0) + 0.05 * torch.randn(n, A, generator=gen)
    old_ls = f32(ls.detach() - 0.01).repeat(n, 1)
    lp, ent, v, mu = _evaluate64(actor, critic, ls, obs, cin, act)
    ratio = torch.exp(lp - old_logp.double())
    surr = torch.max(-adv.double() * ratio, -adv.double() * torch.clamp(ratio, 1 - clip, 1 + clip)).mean()
    vs = v.squeeze(1)
    if clipped:
        vc = old_v.double() + (vs - old_v.double()).clamp(-clip, clip)
        vl = torch.max((vs - ret.double()) ** 2, (vc - ret.double()) ** 2).mean()
    else:
        vl = ((ret.double() - vs) ** 2).mean()
    loss = surr + vcoef * vl - ecoef * ent.mean()
    params = [ls] + list(actor.parameters()) + list(critic.parameters())          # = the flat vector's order
    gref = torch.cat([x.reshape(-1) for x in torch.autograd.grad(loss, params)]).numpy()
    ac.to("cuda")
    need = C.c_size_t()
    _lib.check(lib.rgbm_ppo_scratch_floats_ex(C.byref(ac.desc), n, int(clipped), C.byref(need)))
    scratch = torch.empty(need.value, device="cuda")
    gout = torch.zeros(ac.total + 4, device="cuda")
    d = lambda t: t.cuda().contiguous()  # noqa: E731
    args = [d(obs), d(st), d(act), d(old_logp), d(adv), d(ret), d(old_v), d(old_mu), d(old_ls)]
    _lib.check(lib.rgbm_ppo_minibatch_fwd_bwd_ex(_lib.ptr(ac.flat), C.byref(ac.desc), n, *[_lib.ptr(a) for a in args], clip, vcoef, ecoef,
                                                 int(clipped), _lib.ptr(scratch), _lib.ptr(gout), _lib.stream_ptr()))
    dlp, _, dv, dmu, _, _ = ac.evaluate(d(obs), d(st), d(act))
    torch.cuda.synchronize()
    return (gout.cpu().numpy(), gref, surr.item(), vl.item(), (dlp.cpu(), dv.cpu(), dmu.cpu()),
            (lp.detach(), v.detach(), mu.detach()))


def _check_grad_case(ac, n, clipped, label):
    got, gref, surr, vl, dev, ref = _grad_case(ac, n, clipped)
    depth = max(ac.desc.n_hidden[0], ac.desc.n_hidden[1]) + 1
    kmax = max([ac.obs_dim, ac.state_dim] + ac.hidden + ac.critic_hidden)
    # fp32 dot products of K terms carry a relative error of about sqrt(K) * 2^-24 each and a forward chains `depth` of them; four
    # times that, and never below the 1e-5 gate of the golden comparisons
    tol_f = max(1e-5, 4 * depth * np.sqrt(kmax) * U32)
    fw = [_rel(a, b) for a, b in zip(dev, ref)]
    gerr = _rel(got[:ac.total], gref)
    print(f"{label}: n={n} forward (logp, value, mu) vs float64 {fw} (bound {tol_f:.1e}); gradient {gerr:.2e}; "
          f"surrogate {got[ac.total] / n} vs {surr}; value loss {got[ac.total + 1] / n} vs {vl}")
    assert all(x < tol_f for x in fw), fw
    assert gerr < 1e-4                                    # the gate of test_gpu_ppo.py::test_gradients_match_autograd
    assert abs(got[ac.total] / n - surr) < 1e-5 and abs(got[ac.total + 1] / n - vl) < 1e-4 * vl
    assert got[ac.total + 3] == n


@pytest.mark.parametrize("activation", ["elu", "selu", "relu", "crelu", "lrelu", "tanh", "sigmoid"])
@pytest.mark.parametrize("asym", [False, True])
def test_gradients_match_autograd(activation, asym):
    """HIP analytic gradients against torch autograd in float64; 200 rows: a ragged last tile."""
    torch.manual_seed(3)
    ac = _desc(60, 75, 12, [40, 24], [48, 20, 12], activation, asym)
    _check_grad_case(ac, 200, clipped=True, label=f"{activation} asym={asym}")


def test_gradients_plain_mse_value_loss():
    torch.manual_seed(4)
    _check_grad_case(_desc(60, 75, 12, [40, 24], [48], "tanh", True), 130, clipped=False, label="mse")


@pytest.mark.parametrize("label,shape,n", [
    ("width512", (512, 512, 12, [512, 512], [512], "tanh", True), 70),
    ("six_layers", (60, 75, 12, [48] * 6, [64, 48, 32, 24, 16, 8], "selu", True), 100),
    ("action32", (60, 75, 32, [64], [64], "elu", False), 64),
    ("one_row", (60, 75, 12, [96, 96, 32], [96, 96, 32], "relu", False), 1),
    ("rows65", (60, 75, 12, [256, 256, 256], [256, 256, 256], "selu", False), 65),
    ("rows_not_multiple_of_tile", (60, 75, 12, [33, 7, 130], [5], "elu", False), 2 * 64 + 37),
])
def test_bounds_against_float64(label, shape, n):
    torch.manual_seed(6)
    _check_grad_case(_desc(*shape), n, clipped=True, label=label)


@pytest.mark.parametrize("what", ["width513", "seven_layers", "action33", "zero_layers", "activation"])
def test_out_of_bounds_descriptors_are_errors(what):
    """Argument checks on the host: an error code and a message, nothing is launched."""
    lib = _lib.load()
    ac = _desc(60, 75, 12, [32, 16], [32], "elu", False).to("cuda")
    D = copy.copy(ac.desc)
    if what == "width513":
        D.hidden[0][0] = 513
    elif what == "seven_layers":
        D.n_hidden[1] = 7
    elif what == "action33":
        D.act_dim = 33
    elif what == "zero_layers":
        D.n_hidden[0] = 0
    else:
        D.activation = 6
    word = {"width513": b"width", "seven_layers": b"hidden layers", "action33": b"action dim", "zero_layers": b"hidden layers",
            "activation": b"activation"}[what]
    need = C.c_size_t()
    assert lib.rgbm_ppo_scratch_floats_ex(C.byref(D), 64, 1, C.byref(need)) != 0
    assert word in lib.rgbm_last_error()
    obs = torch.zeros(4, 60, device="cuda")
    mu = torch.full((4, 12), 7.0, device="cuda")
    assert lib.rgbm_policy_forward_ex(_lib.ptr(ac.flat), C.byref(D), 4, 1, _lib.ptr(obs), None, None, None, None, None, _lib.ptr(mu),
                                      _lib.stream_ptr()) != 0
    assert word in lib.rgbm_last_error()
    buf = torch.zeros(1 << 16, device="cuda")
    z = torch.zeros(4 * 33, device="cuda")
    assert lib.rgbm_ppo_minibatch_fwd_bwd_ex(_lib.ptr(ac.flat), C.byref(D), 4, _lib.ptr(obs), None, *[_lib.ptr(z)] * 7, 0.2, 1.0, 0.0, 1,
                                             _lib.ptr(buf), _lib.ptr(buf), _lib.stream_ptr()) != 0
    assert word in lib.rgbm_last_error()
    torch.cuda.synchronize()
    assert bool((mu == 7.0).all()) and bool((buf == 0).all())


@pytest.mark.parametrize("name", ["default", "asym_tanh"])
def test_two_identical_updates_are_bit_identical(name):
    flats = []
    for _ in range(2):
        ppo = _ppo(name, 32)
        _fill_and_update(ppo, 32)
        flats.append(ppo.actor_critic.flat.clone())
    assert torch.equal(flats[0], flats[1])


def test_state_dict_round_trip(gold):
    from rgbmanip_amd.ppo import ActorCritic
    name = "asym_tanh"
    ac = _ppo(name, 32).actor_critic
    sd = ac.state_dict()
    assert list(sd.keys()) == [str(k) for k in gold[name + "_keys"]]
    mcfg, asym, _ = synth.PPO_VARIANTS[name]
    fresh = ActorCritic((60,), (75,), (12,), 0.6, mcfg, asymmetric=asym).to("cuda")
    fresh.load_state_dict({k: v.cpu() for k, v in sd.items()}, strict=True)
    obs = torch.from_numpy(synth.ppo_rollout(16, 32, seed=0)["observations"][3]).cuda()
    assert torch.equal(fresh.act_inference(obs), ac.act_inference(obs))
    with pytest.raises(RuntimeError):
        fresh.load_state_dict({k: v for k, v in list(sd.items())[:-1]}, strict=True)


def test_contrastive_flag_changes_nothing():
    out = []
    for flag in (False, True):
        ppo = _ppo("lrelu64_mse", 32, contrastive=flag)
        losses = _fill_and_update(ppo, 32)
        out.append((ppo.actor_critic.flat.clone(), losses, ppo.step_size))
    assert torch.equal(out[0][0], out[1][0]) and out[0][1] == out[1][1] and out[0][2] == out[1][2]


@pytest.mark.parametrize("sampler", ["sequential", "random"])
def test_run_two_iterations_asymmetric(tmp_path, sampler):
    from rgbmanip_amd.ppo import PPO
    cfg = _cfg("asym_tanh", log_dir=str(tmp_path / "logs"), save_dir=str(tmp_path / "saves"), sampler=sampler)
    torch.manual_seed(11)
    ppo = PPO(synth.StubVecEnv(32, Box, seed=0), cfg)
    before = ppo.actor_critic.flat.clone()
    ppo.run(2, log_interval=1, save_interval=1000)
    flat = ppo.actor_critic.flat
    assert bool(torch.isfinite(flat).all()) and not torch.equal(flat, before)
    assert os.path.exists(os.path.join(cfg["learn"]["save_dir"], "model_2.pt"))
    # the critic's first layer is the one that reads `states`: it moved
    o, shp = ppo.actor_critic.keys["critic.0.weight"]
    assert shp == (256, 75) and not torch.equal(flat[o:o + 256 * 75], before[o:o + 256 * 75])
