"""The Beta action distribution without a GPU: the torch spelling against float64 torch.distributions, the initialisation,
the flags, the refusals, checkpoints and the exported module, the default path, and the NaN-skip."""
import json
import os

import numpy as np
import pytest
import torch
from torch.distributions import Beta, kl_divergence

from tests import beta_ref as R
from tests.test_env_plumbing import oracle_backend  # noqa: F401  (the fixture)
from wiki_grx_gym_amd.envs import GR1T1Cfg, GR1T1CfgPPO, config
from wiki_grx_gym_amd.envs.config import class_to_dict
from wiki_grx_gym_amd.rl import beta as B
from wiki_grx_gym_amd.rl.modules import ActorCriticMLP
from wiki_grx_gym_amd.rl.ppo import PPO
from wiki_grx_gym_amd.rl.runner import OnPolicyRunner
from wiki_grx_gym_amd.utils import export_policy_as_jit, get_args, task_registry
from wiki_grx_gym_amd.utils.helpers import update_cfg_from_args

MLP_KEYS = [f"{net}.model.{i}.{p}" for net in ("actor", "critic") for i in (0, 2, 4) for p in ("weight", "bias")]
BETA = ("--action_dist", "beta")
LL_LO = np.asarray(config.GR1T1LowerLimbCfg.normalization.clip_actions_min, dtype=np.float64)
LL_HI = np.asarray(config.GR1T1LowerLimbCfg.normalization.clip_actions_max, dtype=np.float64)
FB_LO = np.asarray(config.GR1T1FullBodyCfg.normalization.clip_actions_min, dtype=np.float64)
FB_HI = np.asarray(config.GR1T1FullBodyCfg.normalization.clip_actions_max, dtype=np.float64)


def _ac(A=10, **kw):
    kw.setdefault("action_bounds", (LL_LO[:A].tolist(), LL_HI[:A].tolist()) if A <= 10 else (-1.0, 2.0))
    return ActorCriticMLP(39, 168, A, actor_hidden_dims=[32, 16], critic_hidden_dims=[32, 16], init_noise_std=0.2, action_dist="beta", **kw)


# ---- the torch spelling against float64 torch.distributions ----------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [1, 10, 32])
@pytest.mark.parametrize("Bn", [1, 7])
@pytest.mark.parametrize("use_clipped", [True, False], ids=["clipped", "unclipped"])
def test_torch_spelling_matches_float64_distributions(Bn, A, use_clipped):
    raw, value, x, old_logp, a0, b0, adv, ret, tv = R.make_batch(Bn, A, "init", seed=100 * Bn + A)
    ref = R.loss64(raw, value, x, old_logp, a0, b0, adv, ret, tv, R.CLIP, R.VCOEF, R.ECOEF, use_clipped)
    raw64 = raw.double().requires_grad_(True)
    v64 = value.double().requires_grad_(True)
    alpha, beta = B.params_torch(raw64)
    tol = dict(rtol=1e-10, atol=1e-11)
    torch.testing.assert_close(B.logp_torch(alpha, beta, x.double()), ref["logp"], **tol)
    torch.testing.assert_close(B.entropy_torch(alpha, beta), ref["entropy"], **tol)
    torch.testing.assert_close(B.kl_torch(a0.double(), b0.double(), alpha, beta).detach(), ref["kl"], **tol)
    s, vl, loss, kl = B.loss_torch(raw64, v64, x.double(), old_logp.double(), a0.double(), b0.double(), adv.double(), ret.double(), tv.double(),
                                   R.CLIP, R.VCOEF, R.ECOEF, use_clipped)
    loss.backward()
    torch.testing.assert_close(torch.stack([s, vl, loss, kl]).detach(), ref["out"], **tol)
    torch.testing.assert_close(raw64.grad, ref["d_raw"], **tol)
    torch.testing.assert_close(v64.grad, ref["d_value"], **tol)
    # the entropy's own gradient (it enters the loss with a small weight only): the header's closed forms against autograd
    al = alpha.detach().clone().requires_grad_(True)
    be = beta.detach().clone().requires_grad_(True)
    Beta(al, be, validate_args=False).entropy().sum().backward()
    sm = al.detach() + be.detach()
    tri = lambda t: torch.polygamma(1, t)
    torch.testing.assert_close(-(al.detach() - 1) * tri(al.detach()) + (sm - 2) * tri(sm), al.grad, **tol)
    torch.testing.assert_close(-(be.detach() - 1) * tri(be.detach()) + (sm - 2) * tri(sm), be.grad, **tol)
    # the KL of a policy with itself is exactly zero, in fp32 too
    assert torch.equal(B.kl_torch(a0, b0, a0, b0), torch.zeros(Bn))
    assert torch.equal(kl_divergence(Beta(a0.double(), b0.double()), Beta(a0.double(), b0.double())).sum(-1), torch.zeros(Bn, dtype=torch.float64))


def test_sample_is_clamped_and_mapped():
    torch.manual_seed(0)
    alpha, beta = torch.full((64, 10), 1.0), torch.full((64, 10), 300.0)   # mass at the lower end
    lo, span = torch.tensor(LL_LO, dtype=torch.float32), torch.tensor(LL_HI - LL_LO, dtype=torch.float32)
    x, a, logp = B.sample_torch(alpha, beta, lo, span)
    assert x.min() >= B.X_MIN and x.max() <= B.X_MAX and torch.isfinite(logp).all()
    assert (a >= lo).all() and (a <= lo + span).all()
    torch.testing.assert_close(logp, B.logp_torch(alpha, beta, x))


# ---- the initialisation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi,sigma", [(LL_LO, LL_HI, 0.2), (FB_LO, FB_HI, np.asarray(config.GR1T1FullBodyCfgPPO.policy.init_noise_std))],
                         ids=["lower_limb", "full_body"])
def test_initial_policy_has_its_mode_at_zero_and_the_configured_spread(lo, hi, sigma):
    span = hi - lo
    a0, b0 = B.init_params(lo, span, sigma)
    assert (a0 > 1).all() and (b0 > 1).all()
    mode = (a0 - 1) / (a0 + b0 - 2)
    assert np.abs(lo + span * mode).max() <= 1e-6 * span.max() and np.all(np.abs(lo + span * mode) <= 1e-6 * span)
    s = a0 + b0
    std = span * np.sqrt(a0 * b0 / (s * s * (s + 1)))
    assert np.all(np.abs(std / np.broadcast_to(sigma, std.shape) - 1) < 0.05), std
    # ... and through the module: the biases are the inverse softplus, the weights carry the gain
    A = len(lo)
    torch.manual_seed(1)
    ac = ActorCriticMLP(39, 168, A, actor_hidden_dims=[32, 16], critic_hidden_dims=[32, 16], init_noise_std=np.broadcast_to(sigma, lo.shape).tolist(),
                        action_dist="beta", action_bounds=(lo.tolist(), hi.tolist()), actor_output_gain=0.0)
    ac.update_distribution(torch.randn(5, 39))   # (gain 0: the output is the bias in every state)
    al, be = ac.beta_params()
    np.testing.assert_allclose(al[0].detach().numpy(), a0, rtol=2e-6)
    np.testing.assert_allclose(be[0].detach().numpy(), b0, rtol=2e-6)
    np.testing.assert_allclose(ac.action_std[0].detach().numpy(), std, rtol=1e-5)
    assert sorted(ac.state_dict()) == sorted(MLP_KEYS + ["action_lo", "action_span"])
    assert ac.actor.model[-1].weight.shape == (2 * A, 16) and ac.actor.model[-1].weight.abs().max() == 0


def test_initialisation_clamps_a_box_that_excludes_zero():
    a0, b0 = B.init_params(np.array([0.5, -2.0]), np.array([1.0, 1.0]), 0.1)   # zero lies below the first box, above the second
    mode = (a0 - 1) / (a0 + b0 - 2)
    np.testing.assert_allclose(mode, [0.05, 0.95], rtol=1e-12)
    a0, b0 = B.init_params(np.array([-1.0]), np.array([2.0]), 5.0)   # a spread no Beta on the box has: the uniform density
    assert a0[0] == 1.0 and b0[0] == 1.0
    bias = B.init_biases(np.array([-1.0]), np.array([2.0]), 5.0)
    assert torch.isfinite(bias).all() and (bias < -60).all()   # softplus^-1 of a floored zero
    assert torch.equal(1.0 + torch.nn.functional.softplus(bias), torch.ones(2))


def test_constructor_refusals():
    for kw, other in (({"noise_std_type": "log"}, "--noise_std_type"), ({"state_dependent_std": True}, "--state_dependent_std"),
                      ({"fixed_std": True}, "fixed_std"), ({"actor_output_activation": "tanh"}, "actor_output_activation"),
                      ({"layer_norm": True}, "--layer_norm"), ({"num_critic_outputs": 2}, "--reward_groups")):
        with pytest.raises(ValueError, match=other) as info:
            _ac(**kw)
        assert "--action_dist" in str(info.value), kw
    with pytest.raises(ValueError, match="action_bounds"):
        ActorCriticMLP(39, 168, 10, action_dist="beta")
    with pytest.raises(ValueError, match="action_dist"):
        ActorCriticMLP(39, 168, 10, action_dist="squashed")
    for bounds in ((0.0, 0.0), (1.0, -1.0), (0.0, float("inf")), (float("nan"), 1.0)):
        with pytest.raises(ValueError, match="span"):
            _ac(action_bounds=bounds)


# ---- flags, configs, refusals ---------------------------------------------------------------------------------------------------------------
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


def test_cli_flags_reach_the_configs():
    a = get_args([])
    assert a.action_dist is None and a.action_bounds is None
    d = class_to_dict(update_cfg_from_args(None, config.GR1T1CfgPPO(), a)[1])
    assert "action_dist" not in d["policy"] and "action_bounds" not in d["policy"]
    d = class_to_dict(update_cfg_from_args(None, config.GR1T1CfgPPO(), get_args(list(BETA)))[1])
    assert d["policy"]["action_dist"] == "beta" and "action_bounds" not in d["policy"]
    d = class_to_dict(update_cfg_from_args(None, config.GR1T1CfgPPO(), get_args([*BETA, "--action_bounds", "-1.5", "2"]))[1])
    assert d["policy"]["action_dist"] == "beta" and d["policy"]["action_bounds"] == [-1.5, 2.0]
    with pytest.raises(SystemExit):
        get_args(["--action_dist", "squashed"])
    for cls in (config.GR1T1CfgPPO, config.GR1T2CfgPPO, config.GR1T1FullBodyCfgPPO):     # not config keys
        assert not hasattr(cls.policy, "action_dist") and not hasattr(cls.policy, "action_bounds")


class _NoEnv:
    num_envs, num_obs, num_pri_obs, num_actions = 8, 39, 168, 10
    cfg = GR1T1Cfg()

    def reset(self):
        return None


class _ScalarClipEnv(_NoEnv):
    cfg = config.LeggedRobotCfg()


def _cfg_dict(flags, runner=(), algorithm=(), policy=()):
    d = class_to_dict(update_cfg_from_args(None, _train_cfg(), get_args(list(flags)))[1])
    d["runner"].update(runner); d["algorithm"].update(algorithm); d["policy"].update(policy)
    return d


def test_refused_combinations(monkeypatch, tmp_path):
    r = OnPolicyRunner(_NoEnv(), _cfg_dict(BETA), None, "cpu")
    assert r.action_dist["kind"] == "beta" and r.alg._beta and not r.alg._use_act_graph
    np.testing.assert_allclose(r.action_dist["lo"], LL_LO); np.testing.assert_allclose(r.action_dist["hi"], LL_HI)
    ac = r.alg.actor_critic
    np.testing.assert_allclose(ac.action_lo.numpy(), LL_LO, rtol=1e-7); np.testing.assert_allclose(ac.action_span.numpy(), LL_HI - LL_LO, rtol=1e-7)
    # what it composes with builds
    for flags in (("--empirical_normalization",), ("--obs_history", "3", "--critic_obs_history", "2"), ("--privileged_actor",),
                  ("--value_norm", "running"), ("--value_norm", "popart")):
        OnPolicyRunner(_NoEnv(), _cfg_dict(BETA + flags), None, "cpu")
    teacher = str(tmp_path / "teacher.pt")
    OnPolicyRunner(_NoEnv(), _cfg_dict(()), None, "cpu").save(teacher)
    for flags, other in ((("--noise_std_type", "log"), "--noise_std_type"), (("--state_dependent_std",), "--state_dependent_std"),
                         (("--recurrent", "--rnn_hidden_size", "32"), "--recurrent"), (("--symmetry", "augment"), "--symmetry"),
                         (("--smooth", "both"), "--smooth"), (("--grad_penalty_coef", "0.002"), "--grad_penalty_coef"),
                         (("--reward_groups", "a=*"), "--reward_groups"), (("--distill_from", teacher), "--distill_from"),
                         (("--rnd",), "--rnd"), (("--estimator",), "--estimator"), (("--layer_norm",), "--layer_norm"),
                         (("--precision", "bf16"), "--precision bf16"), (("--exact_resume",), "--exact_resume")):
        with pytest.raises((ValueError, NotImplementedError), match=other) as info:
            OnPolicyRunner(_NoEnv(), _cfg_dict(BETA + flags), None, "cpu")
        assert "--action_dist" in str(info.value), flags                                           # the message names both options
    for policy, other in (({"fixed_std": True}, "fixed_std"), ({"actor_output_activation": "tanh"}, "actor_output_activation")):
        with pytest.raises(ValueError, match=other) as info:
            OnPolicyRunner(_NoEnv(), _cfg_dict(BETA, policy=policy), None, "cpu")
        assert "--action_dist" in str(info.value)
    with pytest.raises(ValueError, match="--action_dist"):
        OnPolicyRunner(_NoEnv(), _cfg_dict((), policy={"action_dist": "squashed"}), None, "cpu")
    # a config with only the scalar clip: refused without --action_bounds, accepted with them, a bad span refused
    with pytest.raises(ValueError, match="--action_bounds") as info:
        OnPolicyRunner(_ScalarClipEnv(), _cfg_dict(BETA), None, "cpu")
    assert "--action_dist" in str(info.value) and "clip_actions" in str(info.value)
    r = OnPolicyRunner(_ScalarClipEnv(), _cfg_dict(BETA + ("--action_bounds", "-1", "1.5")), None, "cpu")
    assert r.action_dist == {"kind": "beta", "lo": [-1.0] * 10, "hi": [1.5] * 10}
    for lo_hi in (("1", "1"), ("2", "-2"), ("0", "inf")):
        with pytest.raises(ValueError, match="span"):
            OnPolicyRunner(_ScalarClipEnv(), _cfg_dict(BETA + ("--action_bounds", *lo_hi)), None, "cpu")
    # the algorithm itself refuses what lives there
    for kw, other in (({"symmetry": "augment", "symmetry_maps": object()}, "--symmetry"), ({"smooth": "both"}, "--smooth"),
                      ({"grad_penalty_coef": 0.002}, "--grad_penalty_coef"), ({"reward_groups": object()}, "--reward_groups")):
        with pytest.raises(ValueError, match=other) as info:
            PPO(actor_critic=_ac(), device="cpu", **kw)
        assert "--action_dist" in str(info.value), kw
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    monkeypatch.setattr(dist, "get_rank", lambda *a: 0)
    with pytest.raises(NotImplementedError, match="world size") as info:
        OnPolicyRunner(_NoEnv(), _cfg_dict(BETA), None, "cpu")
    assert "--action_dist" in str(info.value)
    with pytest.raises(NotImplementedError, match="world size") as info:
        PPO(actor_critic=_ac(), device="cpu")
    assert "--action_dist" in str(info.value)


# ---- the default path is what it was --------------------------------------------------------------------------------------------------------
def test_default_path_never_touches_the_beta_code(oracle_backend, tmp_path, monkeypatch):  # noqa: F811
    ac = ActorCriticMLP(39, 168, 10, actor_hidden_dims=[32, 16], critic_hidden_dims=[32, 16], init_noise_std=0.2)
    assert sorted(ac.state_dict()) == sorted(MLP_KEYS + ["std"]) and ac.action_dist == "gaussian" and ac.inference_actor() is ac.actor

    def boom(*a, **k):
        raise AssertionError("the default path called into rl/beta.py")
    for name in ("fused_ppo_loss_beta", "beta_params", "beta_sample", "beta_functions", "rollout_sample", "loss_torch", "params_torch",
                 "sample_torch", "_lib", "resolve_bounds", "init_biases"):
        monkeypatch.setattr(B, name, boom)
    env, runner = _make(tmp_path)
    assert runner.action_dist is None and not runner.alg._beta
    assert "action_dist" not in runner.policy_cfg and "action_bounds" not in runner.policy_cfg
    runner.learn(num_learning_iterations=1)
    ck = torch.load(os.path.join(runner.log_dir, "model_1.pt"), weights_only=False)
    assert set(ck) == {"model_state_dict", "optimizer_state_dict", "iter", "infos"}
    assert sorted(ck["model_state_dict"]) == sorted(MLP_KEYS + ["std"])


# ---- training, checkpoints, the exported module ---------------------------------------------------------------------------------------------
def _watch_actions(env, seen):
    step = env.step

    def wrapped(actions):
        seen.append(actions.detach().clone())
        return step(actions)
    env.step = wrapped


def test_runner_trains_saves_loads_and_exports(oracle_backend, tmp_path):  # noqa: F811
    env, runner = _make(tmp_path, flags=BETA)
    ac, alg = runner.alg.actor_critic, runner.alg
    seen = []
    _watch_actions(env, seen)
    before = {k: v.clone() for k, v in ac.state_dict().items()}
    runner.learn(num_learning_iterations=2)
    after = ac.state_dict()
    assert all(torch.isfinite(v).all() for v in after.values()) and np.isfinite(alg.mean_kl)
    assert not torch.equal(before["actor.model.4.weight"], after["actor.model.4.weight"]) and after["actor.model.4.weight"].shape == (20, 16)
    assert torch.equal(before["action_lo"], after["action_lo"]) and "std" not in after
    lo, hi = torch.tensor(LL_LO, dtype=torch.float32), torch.tensor(LL_HI, dtype=torch.float32)
    acts = torch.stack(seen)
    assert len(seen) == 12 and (acts >= lo).all() and (acts <= hi + 1e-6).all()                    # every action handed to env.step
    st = alg.storage
    assert (st.actions > 0).all() and (st.actions < 1).all() and (st.mu >= 1).all() and (st.sigma >= 1).all()
    torch.testing.assert_close(st.actions_log_prob.squeeze(-1), B.logp_torch(st.mu, st.sigma, st.actions))   # the density at the stored x
    scalars = [json.loads(line) for line in open(os.path.join(runner.log_dir, "scalars.jsonl"))]
    logged = {s["tag"]: s["value"] for s in scalars if s["step"] == 1}
    assert all(f"Policy/noise_std_{i}" in logged for i in range(10)) and 0.1 < logged["Policy/mean_noise_std"] < 0.3
    want = float(B.std_torch(st.mu.flatten(0, 1), st.sigma.flatten(0, 1), ac.action_span).mean(0)[3])
    assert logged["Policy/noise_std_3"] == pytest.approx(want, rel=1e-6)
    ck_path = os.path.join(runner.log_dir, "model_2.pt")
    ck = torch.load(ck_path, weights_only=False)
    assert set(ck) == {"model_state_dict", "optimizer_state_dict", "iter", "infos", "action_dist"}
    assert ck["action_dist"] == runner.action_dist and ck["action_dist"]["kind"] == "beta"
    _, again = _make(None, flags=BETA)
    again.load(ck_path)
    assert all(torch.equal(v, again.alg.actor_critic.state_dict()[k]) for k, v in after.items())
    _, plain = _make(None)
    with pytest.raises(ValueError, match="--action_dist beta"):
        plain.load(ck_path)
    plain.save(str(tmp_path / "plain.pt"))
    with pytest.raises(ValueError, match="--action_dist gaussian"):
        again.load(str(tmp_path / "plain.pt"))
    other = dict(ck, action_dist=dict(ck["action_dist"], hi=[h + 0.5 for h in ck["action_dist"]["hi"]]))   # another box
    torch.save(other, str(tmp_path / "other.pt"))
    with pytest.raises(ValueError, match="--action_dist"):
        again.load(str(tmp_path / "other.pt"))

    # the exported module runs without libgrx_ppo.so, returns [B, A] inside the box and equals act_inference
    policy = runner.get_inference_policy(device="cpu")
    path = export_policy_as_jit(ac, str(tmp_path / "exported"))
    code = ("import sys, torch\nm = torch.jit.load(sys.argv[1])\ny = m(torch.zeros(4, 39))\nassert y.shape == (4, 10)\n"
            "assert not any(n.startswith('wiki_grx_gym_amd') for n in sys.modules)\nprint('ok')\n")   # (the package, and with it the library, never loads)
    import subprocess
    import sys
    done = subprocess.run([sys.executable, "-c", code, path], capture_output=True, text=True, env={**os.environ, "GRX_PPO_LIB": "/nonexistent"})
    assert done.returncode == 0 and "ok" in done.stdout, done.stderr
    jit = torch.jit.load(path)
    assert sorted(k for k in jit.state_dict() if "actor" not in k) == ["lo", "span"]
    obs = env.get_observations()
    with torch.no_grad():
        for _ in range(3):
            a = policy(obs)
            got = jit(obs)
            assert got.shape == (16, 10) and a.shape == (16, 10) and (got - a).abs().max() < 1e-6
            assert (got > lo).all() and (got < hi).all()
            obs = env.step(a)[0]


def test_composes_with_normalisation_history_privileged_actor_and_value_norm(oracle_backend, tmp_path):  # noqa: F811
    # (a privileged actor's history is the critic's: the runner refuses --obs_history beside --privileged_actor, with or without this option)
    flags = BETA + ("--empirical_normalization", "--critic_obs_history", "3", "--privileged_actor", "--value_norm", "running")
    env, runner = _make(tmp_path, flags=flags)
    seen = []
    _watch_actions(env, seen)
    runner.learn(num_learning_iterations=2)
    ac = runner.alg.actor_critic
    assert all(torch.isfinite(v).all() for v in ac.state_dict().values()) and ac.actor.model[-1].out_features == 20
    lo, hi = torch.tensor(LL_LO, dtype=torch.float32), torch.tensor(LL_HI, dtype=torch.float32)
    assert all(((a >= lo) & (a <= hi + 1e-6)).all() for a in seen)
    policy = runner.get_inference_policy(device="cpu")
    a = policy(env.get_privileged_observations())
    assert a.shape == (16, 10) and (a > lo).all() and (a < hi).all()


def test_obs_history_alone_exports_with_its_history(oracle_backend, tmp_path):  # noqa: F811
    flags = BETA + ("--empirical_normalization", "--obs_history", "3", "--critic_obs_history", "2", "--value_norm", "running")
    env, runner = _make(tmp_path, flags=flags)
    runner.learn(num_learning_iterations=1)
    ac = runner.alg.actor_critic
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


def test_non_finite_loss_skips_the_step(oracle_backend):  # noqa: F811
    env, runner = _make(None, flags=BETA)
    alg = runner.alg
    obs, pri = env.get_observations(), env.get_privileged_observations()
    with torch.inference_mode():
        for _ in range(runner.num_steps_per_env):
            obs, pri, rew, dones, infos = env.step(alg.act(obs, pri))
            alg.process_env_step(rew, dones, infos)
        alg.compute_returns(pri)
    alg.storage.returns[...] = float("nan")
    before = [p.detach().clone() for p in alg.actor_critic.parameters()]
    alg.update()
    assert all(torch.equal(b, p) for b, p in zip(before, alg.actor_critic.parameters()))
    assert not alg.optimizer.state or all(float(s.get("step", 0)) == 0 for s in alg.optimizer.state.values())


def test_c_entries_check_their_arguments():
    """invalid sizes and NULL pointers: negative, nothing launched (no GPU needed; the pointers are never followed)"""
    lib = B._lib()
    p = [0x10000000 * k for k in range(1, 16)]
    names = ("raw", "value", "x", "old_logp", "old_alpha", "old_beta", "advantages", "returns", "target_values", "out", "d_raw", "d_value",
             "partials")

    def loss(Bn=8, A=10, clipped=1, **kw):
        a = {n: kw.get(n, v) for n, v in zip(names, p)}
        return lib.grx_ppo_loss_beta(Bn, A, *[a[n] for n in names[:9]], 0.2, 1.0, 0.01, clipped, a["out"], a["d_raw"], a["d_value"],
                                     a["partials"], None)
    assert loss(Bn=0) < 0 and loss(Bn=-3) < 0 and loss(A=0) < 0 and loss(A=33) < 0
    for n in names:
        assert loss(**{n: None}) < 0, n
    assert loss(partials=p[12] + 4) < 0                                                   # the partials hold doubles
    assert lib.grx_ppo_loss_beta_partials_size(0) == 0 and lib.grx_ppo_loss_beta_partials_size(65) == 2 * 4 * 2
    assert lib.grx_beta_params(0, 10, p[0], p[1], p[2], None) < 0 and lib.grx_beta_params(8, 33, p[0], p[1], p[2], None) < 0
    assert lib.grx_beta_params(8, 10, None, p[1], p[2], None) < 0 and lib.grx_beta_params(8, 10, p[0], p[1], None, None) < 0
    for k in range(9):
        ptrs = [None if j == k else p[j] for j in range(9)]
        assert lib.grx_beta_sample(8, 10, *ptrs, None) < 0, k
    assert lib.grx_beta_sample(0, 10, *p[:9], None) < 0 and lib.grx_beta_sample(8, 0, *p[:9], None) < 0 and lib.grx_beta_sample(8, 33, *p[:9], None) < 0
    assert lib.grx_beta_functions(0, p[0], p[1], p[2], p[3], None) < 0 and lib.grx_beta_functions(4, p[0], None, p[2], p[3], None) < 0
