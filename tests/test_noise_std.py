"""The action-noise options without a GPU (rl/modules.py `noise_std_type` / `state_dependent_std`): parameters and
initialisation, the torch spelling of the loss against float64 autograd of rsl_rl's spelling (tests/noise_ref.py), sigma staying positive
under `log`, the default classes / keys / checkpoints being what they were, the flags and every refusal, and the checkpoint and export
round trip over the oracle-backed env of tests/test_env_plumbing.py."""
import copy
import json
import math
import os

import pytest
import torch

from tests import noise_ref as R
from tests.test_env_plumbing import oracle_backend  # noqa: F401  (the fixture)
from wiki_grx_gym_amd.envs import GR1T1Cfg, GR1T1CfgPPO, config
from wiki_grx_gym_amd.envs.config import class_to_dict
from wiki_grx_gym_amd.rl.modules import ActorCriticMLP, MeanHead
from wiki_grx_gym_amd.rl.ppo import PPO
from wiki_grx_gym_amd.rl.runner import OnPolicyRunner
from wiki_grx_gym_amd.utils import export_policy_as_jit, get_args, task_registry
from wiki_grx_gym_amd.utils.helpers import update_cfg_from_args

VARIANTS = {"log": dict(noise_std_type="log"), "sd_scalar": dict(state_dependent_std=True),
            "sd_log": dict(noise_std_type="log", state_dependent_std=True)}
MLP_KEYS = [f"{net}.model.{i}.{p}" for net in ("actor", "critic") for i in (0, 2, 4) for p in ("weight", "bias")]
FULL_BODY_STD = [0.2] * 12 + [0.05] * 20


def _ac(A=10, **kw):
    return ActorCriticMLP(39, 168, A, actor_hidden_dims=[32, 16], critic_hidden_dims=[32, 16], activation="elu", **kw)


# ---- parameters and initialisation --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("init,A", [(0.2, 10), (FULL_BODY_STD, 32)], ids=["scalar_init", "vector_init"])
def test_log_std_parameter(init, A):
    ac = _ac(A, init_noise_std=init, noise_std_type="log")
    want = torch.log(torch.as_tensor(init, dtype=torch.float32) * torch.ones(A))
    assert sorted(ac.state_dict()) == sorted(MLP_KEYS + ["log_std"]) and not hasattr(ac, "std")
    assert torch.equal(ac.log_std.detach(), want) and ac.log_std.requires_grad
    assert torch.equal(ac.noise_std(), torch.exp(ac.log_std)) and ac.noise_std().requires_grad
    assert ac.actor.model[-1].weight.shape == (A, 16)
    ac.act(torch.randn(4, 39))
    assert torch.allclose(ac.action_std[0], torch.as_tensor(init, dtype=torch.float32) * torch.ones(A), rtol=1e-6)
    fixed = _ac(A, init_noise_std=init, noise_std_type="log", fixed_std=True)   # fixed_std as today: init_noise_std, whatever the parameter holds
    with torch.no_grad():
        fixed.log_std.add_(1.0)
    fixed.act(torch.randn(4, 39))
    assert torch.equal(fixed.action_std[0], torch.as_tensor(init, dtype=torch.float32) * torch.ones(A))


@pytest.mark.parametrize("kind", ["scalar", "log"])
@pytest.mark.parametrize("init,A", [(0.2, 10), (FULL_BODY_STD, 32)], ids=["scalar_init", "vector_init"])
def test_state_dependent_output_layer(init, A, kind):
    torch.manual_seed(0)
    ac = _ac(A, init_noise_std=init, noise_std_type=kind, state_dependent_std=True)
    assert sorted(ac.state_dict()) == sorted(MLP_KEYS) and not hasattr(ac, "std") and not hasattr(ac, "log_std")
    last = ac.actor.model[-1]
    assert last.weight.shape == (2 * A, 16) and last.bias.shape == (2 * A,)
    init_t = torch.as_tensor(init, dtype=torch.float32) * torch.ones(A)
    assert not last.weight[A:].any() and last.weight[:A].abs().min() > 0
    assert torch.equal(last.bias[A:].detach(), torch.log(init_t + 1e-7) if kind == "log" else init_t)
    obs = torch.randn(6, 39)
    ac.act(obs)
    assert ac.action_mean.shape == (6, A) and ac.action_std.shape == (6, A)
    assert torch.allclose(ac.action_std, init_t.expand(6, A), rtol=1e-5)               # every state starts at init_noise_std (`log`: + 1e-7, 2e-6 of 0.05)
    assert torch.equal(ac.act_inference(obs), ac.actor(obs)[:, :A]) and ac.act_inference(obs).shape == (6, A)
    assert isinstance(ac.inference_actor(), MeanHead) and _ac(A).inference_actor() is not None
    with pytest.raises(RuntimeError, match="state_dependent_std"):
        ac.noise_std()


def test_actor_output_gain_scales_the_mean_rows_only():
    A = 10
    torch.manual_seed(4)
    ref = _ac(A, init_noise_std=0.3, state_dependent_std=True)
    torch.manual_seed(4)
    ac = _ac(A, init_noise_std=0.3, state_dependent_std=True, actor_output_gain=0.01)
    a, b = ac.actor.model[-1], ref.actor.model[-1]
    assert torch.allclose(a.weight[:A], b.weight[:A] * 0.01) and torch.allclose(a.bias[:A], b.bias[:A] * 0.01)
    assert torch.equal(a.weight[A:], b.weight[A:]) and torch.equal(a.bias[A:], b.bias[A:]) and torch.equal(a.bias[A:], torch.full((A,), 0.3))
    torch.manual_seed(4)                                                                # ... and the default's gain is what it was: all rows
    plain, gained = _ac(A), None
    torch.manual_seed(4)
    gained = _ac(A, actor_output_gain=0.01)
    assert torch.allclose(gained.actor.model[-1].weight, plain.actor.model[-1].weight * 0.01)


def test_constructor_refusals():
    with pytest.raises(ValueError, match="actor_output_activation"):
        _ac(state_dependent_std=True, actor_output_activation="tanh")
    with pytest.raises(ValueError, match="fixed_std"):
        _ac(state_dependent_std=True, fixed_std=True)
    with pytest.raises(ValueError, match="noise_std_type"):
        _ac(noise_std_type="softplus")


def test_load_state_dict_overwrite_belongs_to_std_only():
    src = _ac(noise_std_type="log", init_noise_std=0.3)
    with torch.no_grad():
        src.log_std.add_(0.25)
    dst = _ac(noise_std_type="log", init_noise_std=0.3)                                  # (set_std defaults to True, set_noise_std to 1.0)
    dst.load_state_dict(src.state_dict())
    assert torch.equal(dst.log_std, src.log_std)
    plain_src, plain = _ac(init_noise_std=0.3), _ac(init_noise_std=0.3)
    plain.load_state_dict(plain_src.state_dict())
    assert torch.equal(plain.std.detach(), torch.ones(10))                               # the reference's quirk, as ever


# ---- the loss against float64 -------------------------------------------------------------------------------------------------------------
CLIP, VCOEF, ECOEF = 0.2, 1.0, 0.01


def _minibatch(ac, B, seed):
    """a minibatch drawn like a rollout's from the policy itself (tests/test_ppo_kernels_gpu.py _e2e_setup, on the CPU)"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    A = ac.num_actor_output
    obs, cobs = r(B, 39), r(B, 168)
    with torch.no_grad():
        ac.update_distribution(obs)
        mu, sigma, v = ac.action_mean.clone(), ac.action_std.clone(), ac.evaluate(cobs)
        actions = mu + sigma * r(B, A)
        old_mu = mu + 0.1 * sigma * r(B, A)
        old_sigma = sigma * (1.0 + 0.1 * torch.rand(B, A, generator=g))
        tv, ret, adv = v + 0.3 * r(B, 1), v + r(B, 1), r(B, 1)
        logp = torch.distributions.Normal(mu, sigma).log_prob(actions).sum(-1, keepdim=True)
        old_logp = logp + 0.25 * r(B, 1)
    return [obs, cobs, actions, tv, adv, ret, old_logp, old_mu, old_sigma]


@pytest.mark.parametrize("use_clipped", [True, False], ids=["clipped", "unclipped"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_loss_and_parameter_gradients_match_float64(variant, use_clipped):
    """PPO._losses' torch spelling at B = 64, A = 10: the four scalars and every parameter gradient against float64 autograd of rsl_rl's
    spelling on a float64 copy of the policy, at tests/test_ppo_golden.py's bounds for the existing update on the CPU (scalars 1e-4
    relative, 1e-6 absolute; tensors rtol 1e-4, atol 2e-6).  The actor's s rows are given weight first: at initialisation they are zero
    and sigma would not depend on the state."""
    torch.manual_seed(7)
    ac = _ac(init_noise_std=0.3, **VARIANTS[variant])
    if ac.state_dependent_std:
        with torch.no_grad():
            ac.actor.model[-1].weight[10:].copy_(0.02 * torch.randn(10, 16))   # (small: `scalar`'s sigma = 0.3 + ... stays positive)
    ac64 = copy.deepcopy(ac).double()
    alg = PPO(ac, clip_param=CLIP, value_loss_coef=VCOEF, entropy_coef=ECOEF, use_clipped_value_loss=use_clipped, schedule="adaptive",
              desired_kl=0.01, device="cpu")
    batch = _minibatch(ac, 64, 5)
    if ac.state_dependent_std:
        assert float(batch[8].std(0).min()) > 0                                          # sigma does differ from row to row
    surrogate, value_loss, loss, kl = alg._losses(*batch)
    alg.optimizer.zero_grad()
    loss.backward()
    obs, cobs, actions, tv, adv, ret, old_logp, old_mu, old_sigma = (t.double() for t in batch)
    mean, sigma = R.policy_sigma(ac64, obs)
    t = R.loss_terms(mean, sigma, ac64.critic.model(cobs), actions, old_logp, old_mu, old_sigma, adv, ret, tv, CLIP, VCOEF, ECOEF, use_clipped)
    t["loss"].backward()
    for got, want in ((surrogate, t["surrogate"]), (value_loss, t["value_loss"]), (loss, t["loss"]), (kl, t["kl"])):
        assert float(got.detach()) == pytest.approx(float(want.detach()), rel=1e-4, abs=1e-6)
    names = [n for n, _ in ac.named_parameters()]
    assert ("log_std" in names) == (variant == "log") and "std" not in names
    for (n, p), q in zip(ac.named_parameters(), ac64.parameters()):
        assert p.grad is not None and q.grad is not None and float(q.grad.abs().max()) > 0, n
        torch.testing.assert_close(p.grad.double(), q.grad, rtol=1e-4, atol=2e-6, msg=lambda m: f"{variant} {n}: {m}")


# ---- sigma under `log` ----------------------------------------------------------------------------------------------------------------------
def _shrinking_step(ac, opt, alg, batch):
    surrogate, value_loss, loss, kl = alg._losses(*batch)
    opt.zero_grad()
    loss.backward()
    opt.step()
    return float(loss)


def test_sigma_stays_positive_under_log():
    """A hand-made minibatch whose gradient shrinks sigma (actions equal to the mean, positive advantages: the likelihood rises as sigma
    falls), 200 Adam steps at lr 1e-1 on the noise parameter.  Under `log` every loss is finite and sigma stays positive.  The default
    parametrisation on the same minibatch carries `std` through zero: from then on the loss is not finite (on the CPU, where
    torch.distributions validates, Normal refuses the scale instead) -- DESIGN.md 4.13 documents that and leaves it."""
    results = {}
    for kind in ("log", "scalar"):
        torch.manual_seed(1)
        ac = _ac(A=4, init_noise_std=0.5, noise_std_type=kind)
        alg = PPO(ac, clip_param=1e6, value_loss_coef=0.0, entropy_coef=0.0, use_clipped_value_loss=False, schedule="fixed", device="cpu")
        B, g = 16, torch.Generator().manual_seed(2)
        obs, cobs = torch.randn(B, 39, generator=g), torch.randn(B, 168, generator=g)
        with torch.no_grad():
            mu = ac.actor(obs)
        batch = [obs, cobs, mu.clone(), torch.zeros(B, 1), torch.ones(B, 1), torch.zeros(B, 1), torch.zeros(B, 1), mu.clone(),
                 torch.full((B, 4), 0.5)]
        noise = ac.log_std if kind == "log" else ac.std
        opt = torch.optim.Adam([noise], lr=1e-1)
        losses, sigmas, refused = [], [], False
        for _ in range(200):
            try:
                losses.append(_shrinking_step(ac, opt, alg, batch))
            except ValueError:                                                            # Normal's validation of a non-positive scale
                refused = True
                break
            sigmas.append(float(ac.noise_std().min()))
        results[kind] = (losses, sigmas, refused)
    losses, sigmas, refused = results["log"]
    assert len(losses) == 200 and not refused and all(math.isfinite(v) for v in losses) and all(s > 0 for s in sigmas)
    assert sigmas[-1] < 0.5 * sigmas[0]                                                   # ... and the minibatch did shrink it
    losses, sigmas, refused = results["scalar"]
    assert any(s <= 0 for s in sigmas) and (refused or not all(math.isfinite(v) for v in losses))   # the failure `log` closes


# ---- the default is what it was -----------------------------------------------------------------------------------------------------------
def _args(extra=()):
    return get_args(["--task", "GR1T1", "--headless", "--num_envs", "16", "--sim_device", "cpu", "--rl_device", "cpu", "--pipeline", "cpu",
                     "--seed", "3", *extra])


def _train_cfg(steps=6):
    tcfg = GR1T1CfgPPO()
    tcfg.runner.num_steps_per_env = steps
    tcfg.algorithm.num_mini_batches, tcfg.algorithm.num_learning_epochs = 3, 2
    tcfg.policy.actor_hidden_dims, tcfg.policy.critic_hidden_dims = [32, 16], [32, 16]
    return tcfg


def _make(tmp_path, flags=(), steps=6):
    args = _args(flags)
    env, _ = task_registry.make_env("GR1T1", args=args, env_cfg=GR1T1Cfg())
    runner, _ = task_registry.make_alg_runner(env, name=None, args=args, train_cfg=_train_cfg(steps), log_root=str(tmp_path) if tmp_path else None)
    return env, runner


def test_default_is_unchanged(oracle_backend, tmp_path):  # noqa: F811
    ac = _ac()
    assert type(ac) is ActorCriticMLP and sorted(ac.state_dict()) == sorted(MLP_KEYS + ["std"]) and not hasattr(ac, "log_std")
    assert ac.noise_std() is ac.std and ac.inference_actor() is ac.actor and ac.actor.model[-1].weight.shape == (10, 16)
    assert ac.noise_std_type == "scalar" and ac.state_dependent_std is False
    env, runner = _make(tmp_path)
    assert type(runner.alg.actor_critic) is ActorCriticMLP and runner.noise is None and not runner.alg._state_dependent
    assert "noise_std_type" not in runner.policy_cfg and "state_dependent_std" not in runner.policy_cfg
    runner.learn(num_learning_iterations=1)
    ck = torch.load(os.path.join(runner.log_dir, "model_1.pt"), weights_only=False)
    assert set(ck) == {"model_state_dict", "optimizer_state_dict", "iter", "infos"}
    assert sorted(ck["model_state_dict"]) == sorted(MLP_KEYS + ["std"])
    assert runner.get_inference_policy(device="cpu") == runner.alg.actor_critic.act_inference


# ---- flags and refusals ---------------------------------------------------------------------------------------------------------------------
def test_cli_flags_reach_the_configs():
    a = get_args([])
    assert a.noise_std_type is None and a.state_dependent_std is False
    d = class_to_dict(update_cfg_from_args(None, config.GR1T1CfgPPO(), a)[1])
    assert "noise_std_type" not in d["policy"] and "state_dependent_std" not in d["policy"]
    d = class_to_dict(update_cfg_from_args(None, config.GR1T1CfgPPO(), get_args(["--noise_std_type", "log"]))[1])
    assert d["policy"]["noise_std_type"] == "log" and "state_dependent_std" not in d["policy"]
    d = class_to_dict(update_cfg_from_args(None, config.GR1T1CfgPPO(), get_args(["--state_dependent_std"]))[1])
    assert d["policy"]["state_dependent_std"] is True and "noise_std_type" not in d["policy"]
    d = class_to_dict(update_cfg_from_args(None, config.GR1T1CfgPPO(), get_args(["--state_dependent_std", "--noise_std_type", "log"]))[1])
    assert d["policy"]["state_dependent_std"] is True and d["policy"]["noise_std_type"] == "log"
    with pytest.raises(SystemExit):
        get_args(["--noise_std_type", "softplus"])
    for cls in (config.GR1T1CfgPPO, config.GR1T2CfgPPO, config.GR1T1FullBodyCfgPPO):     # not config keys
        assert not hasattr(cls.policy, "noise_std_type") and not hasattr(cls.policy, "state_dependent_std")


class _NoEnv:
    num_envs, num_obs, num_pri_obs, num_actions = 8, 39, 168, 10

    def reset(self):
        return None


def _cfg_dict(flags, runner=(), algorithm=(), policy=()):
    d = class_to_dict(update_cfg_from_args(None, _train_cfg(), get_args(list(flags)))[1])
    d["runner"].update(runner); d["algorithm"].update(algorithm); d["policy"].update(policy)
    return d


SD = ("--state_dependent_std",)


def test_refused_combinations(monkeypatch, tmp_path):
    for flags in (("--noise_std_type", "log"), SD, SD + ("--noise_std_type", "log")):                 # the options alone are fine
        r = OnPolicyRunner(_NoEnv(), _cfg_dict(flags), None, "cpu")
        assert r.noise == {"std_type": "log" if "log" in flags else "scalar", "state_dependent": "--state_dependent_std" in flags}
    # ... and what `log` and state-dependent sigma compose with
    OnPolicyRunner(_NoEnv(), _cfg_dict(("--noise_std_type", "log", "--recurrent", "--rnn_hidden_size", "32")), None, "cpu")
    OnPolicyRunner(_NoEnv(), _cfg_dict(SD + ("--empirical_normalization", "--obs_history", "3")), None, "cpu")
    OnPolicyRunner(_NoEnv(), _cfg_dict(SD + ("--privileged_actor",)), None, "cpu")
    OnPolicyRunner(_NoEnv(), _cfg_dict(SD + ("--rnd",)), None, "cpu")
    teacher = str(tmp_path / "teacher.pt")
    for flags, other in ((SD + ("--recurrent", "--rnn_hidden_size", "32"), "--recurrent"),
                         (SD + ("--symmetry", "augment"), "--symmetry"),
                         (SD + ("--distill_from", teacher), "--distill_from")):
        with pytest.raises(ValueError, match=other) as info:
            OnPolicyRunner(_NoEnv(), _cfg_dict(flags), None, "cpu")
        assert "--state_dependent_std" in str(info.value), flags                                     # the message names both options
    with pytest.raises(ValueError, match="--distill_from") as info:                                  # either noise option: the student's noise is a buffer
        OnPolicyRunner(_NoEnv(), _cfg_dict(("--noise_std_type", "log", "--distill_from", teacher)), None, "cpu")
    assert "--noise_std_type" in str(info.value)
    with pytest.raises(ValueError, match="--noise_std_type"):
        OnPolicyRunner(_NoEnv(), _cfg_dict((), policy={"noise_std_type": "softplus"}), None, "cpu")
    # a teacher checkpoint with a state-dependent sigma
    src = OnPolicyRunner(_NoEnv(), _cfg_dict(SD), None, "cpu")
    src.save(teacher)
    assert torch.load(teacher, weights_only=False)["noise"] == {"std_type": "scalar", "state_dependent": True}
    with pytest.raises(ValueError, match="--distill_from") as info:
        OnPolicyRunner(_NoEnv(), _cfg_dict(("--distill_from", teacher)), None, "cpu")
    assert "--state_dependent_std" in str(info.value)
    # the algorithm itself refuses what the runner refuses
    with pytest.raises(ValueError, match="--symmetry") as info:
        PPO(actor_critic=_ac(state_dependent_std=True), device="cpu", symmetry="augment", symmetry_maps=object())
    assert "--state_dependent_std" in str(info.value)
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    monkeypatch.setattr(dist, "get_rank", lambda *a: 0)
    with pytest.raises(NotImplementedError, match="world size") as info:
        OnPolicyRunner(_NoEnv(), _cfg_dict(SD), None, "cpu")
    assert "--state_dependent_std" in str(info.value)
    with pytest.raises(NotImplementedError, match="world size") as info:
        PPO(actor_critic=_ac(state_dependent_std=True), device="cpu")
    assert "--state_dependent_std" in str(info.value)


# ---- checkpoints and the exported module ----------------------------------------------------------------------------------------------------
FLAGS = {"log": ("--noise_std_type", "log"), "sd_scalar": SD, "sd_log": SD + ("--noise_std_type", "log")}


@pytest.mark.parametrize("variant", list(FLAGS))
def test_runner_trains_saves_loads_and_exports(oracle_backend, tmp_path, variant):  # noqa: F811
    flags = FLAGS[variant]
    env, runner = _make(tmp_path, flags=flags)
    ac = runner.alg.actor_critic
    sd = "--state_dependent_std" in flags
    want = {"std_type": "log" if "log" in flags else "scalar", "state_dependent": sd}
    assert type(ac) is ActorCriticMLP and ac.state_dependent_std == sd and runner.noise == want
    before = {k: v.clone() for k, v in ac.state_dict().items()}
    runner.learn(num_learning_iterations=2)
    after = ac.state_dict()
    assert all(torch.isfinite(v).all() for v in after.values())
    assert not torch.equal(before["actor.model.4.weight"], after["actor.model.4.weight"])
    if sd:
        assert after["actor.model.4.weight"].shape == (20, 16) and after["actor.model.4.weight"][10:].abs().max() > 0    # the s rows train
        assert "std" not in after and "log_std" not in after
    else:
        assert not torch.equal(before["log_std"], after["log_std"]) and "std" not in after
    scalars = [json.loads(line) for line in open(os.path.join(runner.log_dir, "scalars.jsonl"))]
    logged = {s["tag"]: s["value"] for s in scalars if s["step"] == 1}
    assert all(f"Policy/noise_std_{i}" in logged for i in range(10)) and 0 < logged["Policy/mean_noise_std"] < 1
    if sd:   # the per-action mean of the last rollout's stored sigma rows
        assert logged["Policy/noise_std_3"] == pytest.approx(float(runner.alg.storage.sigma[:, :, 3].mean()), rel=1e-6)
    else:
        assert logged["Policy/noise_std_3"] == pytest.approx(float(torch.exp(after["log_std"][3])), rel=1e-6)
    ck_path = os.path.join(runner.log_dir, "model_2.pt")
    ck = torch.load(ck_path, weights_only=False)
    assert ck["noise"] == want and set(ck) == {"model_state_dict", "optimizer_state_dict", "iter", "infos", "noise"}
    _, again = _make(None, flags=flags)
    again.load(ck_path)
    assert all(torch.equal(v, again.alg.actor_critic.state_dict()[k]) for k, v in after.items())          # log_std included: loaded as saved
    _, plain = _make(None)
    with pytest.raises(ValueError, match="--noise_std_type") as info:
        plain.load(ck_path)
    assert ("--state_dependent_std" in str(info.value)) and f"--noise_std_type {want['std_type']}" in str(info.value)
    plain.save(str(tmp_path / "plain.pt"))
    with pytest.raises(ValueError, match="--noise_std_type scalar"):
        again.load(str(tmp_path / "plain.pt"))
    other = [f for name, f in FLAGS.items() if name != variant][0]
    _, third = _make(None, flags=other)
    with pytest.raises(ValueError, match="--noise_std_type"):
        third.load(ck_path)

    # the exported module returns [B, A] and equals act_inference within tests/test_obs_norm.py's export bound
    policy = runner.get_inference_policy(device="cpu")
    jit = torch.jit.load(export_policy_as_jit(ac, str(tmp_path / "exported")))
    obs = env.get_observations()
    with torch.no_grad():
        for _ in range(3):
            a = policy(obs)
            got = jit(obs)
            assert got.shape == (16, 10) and a.shape == (16, 10) and (got - a).abs().max() < 1e-6
            obs = env.step(a)[0]


def test_state_dependent_composes_with_normalisation_and_history(oracle_backend, tmp_path):  # noqa: F811
    flags = SD + ("--noise_std_type", "log", "--empirical_normalization", "--obs_history", "3")
    env, runner = _make(tmp_path, flags=flags)
    runner.learn(num_learning_iterations=1)
    ac = runner.alg.actor_critic
    assert ac.actor.model[0].in_features == 3 * 39 and ac.actor.model[-1].out_features == 20
    policy = runner.get_inference_policy(device="cpu")
    jit = torch.jit.load(export_policy_as_jit(ac, str(tmp_path / "exported"), normalizer=runner.obs_normalizer, history=3))
    jit.reset_memory()
    obs = env.get_observations()
    with torch.no_grad():
        for _ in range(4):
            a = policy(obs)
            got = jit(obs)
            assert got.shape == (16, 10) and (got - a).abs().max() < 1e-6
            obs, _, _, dones, _ = env.step(a)
            policy.reset(dones)
            jit.reset(dones)


def test_c_entries_check_their_arguments():
    """invalid sizes and NULL pointers: negative, nothing launched (no GPU needed; the pointers are never followed)"""
    from wiki_grx_gym_amd.rl.fused_loss import load_ppo_library
    lib = load_ppo_library()
    p = [0x10000000 * k for k in range(1, 16)]
    names = ("raw", "value", "actions", "old_logp", "old_mu", "old_sigma", "advantages", "returns", "target_values", "out", "d_raw", "d_value",
             "partials")

    def loss(B=8, A=10, clipped=1, **kw):
        a = {n: kw.get(n, v) for n, v in zip(names, p)}
        return lib.grx_ppo_loss_sd(B, A, a["raw"], 1, a["value"], a["actions"], a["old_logp"], a["old_mu"], a["old_sigma"], a["advantages"],
                                   a["returns"], a["target_values"], 0.2, 1.0, 0.01, clipped, a["out"], a["d_raw"], a["d_value"], a["partials"], None)
    assert loss(B=0) < 0 and loss(B=-3) < 0 and loss(A=0) < 0 and loss(A=33) < 0
    for n in names:
        assert loss(**{n: None}) < 0, n
    assert loss(partials=p[12] + 4) < 0                                                   # the partials hold doubles
    assert lib.grx_ppo_loss_sd_partials_size(0) == 0 and lib.grx_ppo_loss_sd_partials_size(257) == 2 * 4 * 2
    hnames = ("X", "W", "bias", "eps", "actions", "logp", "mu", "sigma")

    def head(M=8, K=16, A=10, **kw):
        a = {n: kw.get(n, v) for n, v in zip(hnames, p)}
        return lib.grx_mlp_policy_head_sd(M, K, A, a["X"], a["W"], a["bias"], 0, a["eps"], a["actions"], a["logp"], a["mu"], a["sigma"], None)
    assert head(M=0) < 0 and head(K=0) < 0 and head(A=0) < 0 and head(A=33) < 0
    for n in hnames:
        if n != "bias":
            assert head(**{n: None}) < 0, n
