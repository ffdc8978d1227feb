"""Multi-critic PPO (rl/multi_critic.py) on the CPU: the group spec, the torch spelling of the three operations against the
float64 reference (tests/mc_ref.py) and -- with one group of weight 1 -- against RolloutStorage.compute_returns and PPO's own loss bit for
bit, the flags, the refusals, the checkpoint entry, the runner over the oracle-backed env, the default path, and the C entries' argument
checks."""
import os
import sys
import types

import numpy as np
import pytest
import torch

from tests import mc_ref as R
from tests.test_env_plumbing import oracle_backend  # noqa: F401  (the fixture)
from wiki_grx_gym_amd import _capi
from wiki_grx_gym_amd.envs import GR1T1Cfg, GR1T1CfgPPO, config
from wiki_grx_gym_amd.envs.config import class_to_dict
from wiki_grx_gym_amd.rl import multi_critic as M
from wiki_grx_gym_amd.rl.modules import ActorCriticMLP
from wiki_grx_gym_amd.rl.ppo import PPO
from wiki_grx_gym_amd.rl.runner import OnPolicyRunner
from wiki_grx_gym_amd.rl.storage import RolloutStorage
from wiki_grx_gym_amd.utils import get_args, task_registry
from wiki_grx_gym_amd.utils.helpers import update_cfg_from_args

SPEC = "track=cmd_diff_lin_vel_x,cmd_diff_lin_vel_y,cmd_diff_ang_vel_yaw;rest=*"
TRACK = ["cmd_diff_ang_vel_yaw", "cmd_diff_lin_vel_x", "cmd_diff_lin_vel_y"]   # (table order)


def _active(cfg_cls=GR1T1Cfg):
    return [n for n, v in class_to_dict(cfg_cls().rewards.scales).items() if v != 0]


def _parse(spec, active=None, base=_capi.BASE_REWARD_TERMS):
    return M.parse_reward_groups(spec, _active() if active is None else active, _capi.REWARD_TERMS, base)


# ---- the group spec ----------------------------------------------------------------------------------------------------------------------------
def test_star_takes_the_remaining_active_terms():
    active = _active()
    g = _parse(SPEC)
    assert g.names == ["track", "rest"] and g.K == 2 and g.terms["track"] == TRACK
    assert sorted(g.terms["track"] + g.terms["rest"]) == sorted(active) and not set(g.terms["track"]) & set(g.terms["rest"])
    assert len(g.term_group) == _capi.NUM_REWARD_TERMS + _capi.NUM_BASE_REWARD_TERMS and not g.uses_base
    for t, name in enumerate(_capi.REWARD_TERMS):                                   # the map: main-table rows
        assert g.term_group[t] == (0 if name in TRACK else 1 if name in active else -1), name
    assert all(x == -1 for x in g.term_group[_capi.NUM_REWARD_TERMS:])
    assert ("termination" in g.terms["rest"]) == ("termination" in active)
    one = _parse("all=*")
    assert one.K == 1 and one.terms["all"] == [n for n in _capi.REWARD_TERMS if n in active]
    assert g.entry([1.0, 2.0]) == {"groups": {"track": TRACK, "rest": g.terms["rest"]}, "weights": [1.0, 2.0]}


def test_map_of_a_task_with_base_terms():
    active = ["cmd_diff_lin_vel_x", "termination", "torques", "tracking_lin_vel", "action_rate", "dof_tor_new"]
    g = _parse("move=tracking_lin_vel,cmd_diff_lin_vel_x;eff=torques,dof_tor_new;rest=*", active)
    assert g.uses_base and g.K == 3
    assert g.terms == {"move": ["cmd_diff_lin_vel_x", "tracking_lin_vel"], "eff": ["dof_tor_new", "torques"], "rest": ["termination", "action_rate"]}
    want = {"cmd_diff_lin_vel_x": 0, "tracking_lin_vel": 0, "dof_tor_new": 1, "torques": 1, "termination": 2, "action_rate": 2}
    table = list(_capi.REWARD_TERMS) + list(_capi.BASE_REWARD_TERMS)
    assert g.term_group == [want.get(n, -1) for n in table]
    assert g.term_group[_capi.NUM_REWARD_TERMS + _capi.BASE_REWARD_TERMS.index("torques")] == 1


@pytest.mark.parametrize("spec, what", [
    ("a=no_such_term;b=*", "is not a reward term"),
    ("a=feet_stumble_nonexistent", "is not a reward term"),
    ("a=tracking_lin_vel;b=*", "not active"),                                       # a base term whose scale is 0 in GR1T1
    ("a=cmd_diff_lin_vel_x;b=cmd_diff_lin_vel_x,*", "two groups"),
    ("a=*;b=*", r"`\*` may appear in one group"),
    ("a=cmd_diff_lin_vel_x;b=cmd_diff_lin_vel_y", "are in no group"),
    ("", "needs a spec"),
    ("a", "is not `name="),
    ("a=cmd_diff_lin_vel_x;a=*", "appears twice"),
])
def test_refused_specs(spec, what):
    with pytest.raises(ValueError, match=what) as info:
        _parse(spec)
    assert "--reward_groups" in str(info.value)
    if "not a reward term" in what or "not active" in what:
        assert all(n in str(info.value) for n in _active())                         # the refusal lists the active terms


def test_group_count_and_weights():
    active = [n for n in _capi.REWARD_TERMS if n in _active()][:9]
    with pytest.raises(ValueError, match="1..8"):
        _parse(";".join(f"g{k}={n}" for k, n in enumerate(active)), active)          # nine groups
    assert _parse(";".join(f"g{k}={n}" for k, n in enumerate(active[:8])), active[:8]).K == 8
    assert M.parse_weights(None, 3) == [1.0, 1.0, 1.0] and M.parse_weights("0.5,2", 2) == [0.5, 2.0] and M.parse_weights([3, 1], 2) == [3.0, 1.0]
    for bad in ("1", "1,2,3", "1,0", "1,-2", "1,nan", "1,inf", "1,x", [1.0, float("inf")]):
        with pytest.raises(ValueError, match="--reward_group_weights"):
            M.parse_weights(bad, 2)


# ---- the torch spelling against the float64 reference ------------------------------------------------------------------------------------------
def _t(a, dtype=None):
    x = torch.from_numpy(np.array(a))
    return x.to(dtype) if dtype is not None else x


@pytest.mark.parametrize("N, NT, NB, K", [(1, 3, 0, 1), (65, 36, 15, 3), (130, 36, 0, 8), (7, 5, 4, 2)])
def test_store_torch_against_the_reference(N, NT, NB, K):
    terms, base, group, values, to = R.tables(N, NT, NB, K)
    for tos in (None, to):
        want_v, want_r, _, mag = R.store(terms, base, group, values, tos)
        for dt, tol in ((torch.float64, 1e-12), (torch.float32, (NT + NB + 2) * R.U)):
            sv, sr = torch.full((N, K), 7.0, dtype=dt), torch.full((N, K), 7.0, dtype=dt)
            M.mc_store_torch(_t(terms, dt), _t(base, dt) if base is not None else None, group.tolist(), _t(values, dt),
                             _t(tos) if tos is not None else None, R.f32(R.GAMMA) if dt == torch.float64 else R.GAMMA, sv, sr)
            assert np.array_equal(sv.double().numpy(), want_v)
            bound = tol * (mag[:, None] + np.abs(want_v) + 1e-30)
            assert bool((np.abs(sr.double().numpy() - want_r) <= bound).all())
    with pytest.raises(ValueError, match="group"):
        M.mc_store_torch(_t(terms), None, [K] * NT, _t(values), None, R.GAMMA, torch.zeros(N, K), torch.zeros(N, K))


@pytest.mark.parametrize("K", [1, 2, 3, 8])
@pytest.mark.parametrize("T, N", [(1, 1), (2, 7), (7, 65)])
def test_returns_torch_against_the_reference(T, N, K):
    r, v, d, last = R.rollout(T, N, K)
    w = R.weights(K)
    ref = R.returns(r, v, d, last, w)
    ret, adv, stats = torch.zeros(T, N, K, dtype=torch.float64), torch.zeros(T, N, dtype=torch.float64), torch.zeros(K, 2, dtype=torch.float64)
    M.mc_returns_torch(_t(r).double(), _t(v).double(), _t(d), _t(last).double(), w, R.f32(R.GAMMA), R.f32(R.LAM), ret, adv, stats)
    # (float64 data, but `alive` is the spelling's fp32 0 / 1: alive gamma lam is rounded to fp32 once per step -- T roundings of size u S)
    S = float(np.abs(r).max() + np.abs(v).max() + np.abs(last).max() + np.abs(ref["returns"]).max())
    b_ret = 2 * T * R.U * S
    assert float(np.abs(ret.numpy() - ref["returns"]).max()) <= b_ret
    if T * N == 1:
        assert bool(torch.isnan(adv).all()) and np.isnan(ref["advantages"]).all() and bool(torch.isnan(stats[:, 1]).all())
        return
    assert bool((np.abs(stats.numpy() - ref["stats"]) <= np.array([2 * b_ret, 4 * b_ret]) + 1e-12).all())
    b_adv = sum(w[k] * 2 * (2 * b_ret + np.abs(ref["normalised"][..., k]) * 4 * b_ret) / ref["stats"][k, 1] for k in range(K))
    assert bool((np.abs(adv.numpy() - ref["advantages"]) <= b_adv + 1e-12).all())
    # ... and in fp32, as it runs: within the forward error of 8 T + 16 rounded operations per column
    ret32, adv32 = torch.zeros(T, N, K), torch.zeros(T, N, 1)
    M.mc_returns_torch(_t(r), _t(v), _t(d).unsqueeze(-1), _t(last), w, R.GAMMA, R.LAM, ret32, adv32)
    assert float(np.abs(ret32.double().numpy() - ref["returns"]).max()) <= (8 * T + 16) * R.U * S


@pytest.mark.parametrize("use_clipped", [True, False])
@pytest.mark.parametrize("B, A, K", [(1, 1, 1), (255, 10, 2), (257, 32, 3), (64, 10, 8)])
def test_loss_torch_against_the_reference(B, A, K, use_clipped):
    b = R.minibatch(B, A, K)
    ref = R.loss(b, use_clipped=use_clipped)
    t = {k: _t(x).double().requires_grad_(k in ("mu", "std", "value")) for k, x in b.items()}
    s, vl, loss, kl, heads = M.mc_loss_torch(t["mu"], t["mu"] * 0.0 + t["std"], t["value"], t["actions"], t["old_logp"], t["old_mu"],
                                             t["old_sigma"], t["advantages"], t["returns"], t["target_values"], R.f32(0.2), 1.0,
                                             R.f32(0.01), use_clipped)
    loss.backward()
    got = np.array([s.item(), vl.item(), loss.item(), kl.item()] + heads.tolist())
    assert np.allclose(got, ref["out"], rtol=1e-9, atol=1e-9) and heads.shape == (K,)
    assert abs(vl.item() - float(np.sum(ref["out"][4:]))) <= 1e-12 * (1 + abs(vl.item()))   # the value loss is the sum over the heads
    for name, key in (("mu", "d_mu"), ("std", "d_std"), ("value", "d_value")):
        assert np.allclose(t[name].grad.numpy(), ref[key], rtol=1e-9, atol=1e-12), name


# ---- one group of weight 1 is the code that was there -------------------------------------------------------------------------------------------
def test_one_group_is_compute_returns_bit_for_bit():
    for T, N in ((1, 1), (2, 7), (7, 65), (7, 130)):
        r, v, d, last = R.rollout(T, N, 1)
        st = RolloutStorage(N, T, [3], [3], [2], "cpu")
        st.rewards.copy_(_t(r)); st.values.copy_(_t(v)); st.dones.copy_(_t(d).unsqueeze(-1))
        st.compute_returns(_t(last), R.GAMMA, R.LAM)
        ret, adv = torch.zeros(T, N, 1), torch.zeros(T, N, 1)
        M.mc_returns_torch(_t(r), _t(v), st.dones, _t(last), [1.0], R.GAMMA, R.LAM, ret, adv)
        assert torch.equal(ret, st.returns), (T, N)
        assert torch.equal(adv, st.advantages) or (T * N == 1 and bool(torch.isnan(adv).all() and torch.isnan(st.advantages).all()))


def _ppo(K=None, weights=None, seed=0, **kw):
    torch.manual_seed(seed)
    ac = ActorCriticMLP(5, 9, 3, actor_hidden_dims=[16, 8], critic_hidden_dims=[16, 8], **({} if K is None else {"num_critic_outputs": K}))
    extra = {}
    if K is not None:
        active = list(_capi.REWARD_TERMS[:K])
        extra = {"reward_groups": M.parse_reward_groups(";".join(f"g{k}={n}" for k, n in enumerate(active)), active, _capi.REWARD_TERMS),
                 "reward_group_weights": weights}
    return PPO(ac, num_learning_epochs=2, num_mini_batches=2, schedule="adaptive", entropy_coef=0.01, device="cpu", **extra, **kw)


@pytest.mark.parametrize("use_clipped", [True, False])
def test_one_group_is_ppos_torch_loss_bit_for_bit(use_clipped):
    b = {k: _t(x) for k, x in R.minibatch(257, 3, 1).items()}
    plain, mc = _ppo(use_clipped_value_loss=use_clipped), _ppo(1, use_clipped_value_loss=use_clipped)
    obs = torch.randn(257, 5)
    outs = []
    for alg in (plain, mc):
        alg.actor_critic.update_distribution(obs)
        mu = alg.actor_critic.action_mean
        value = b["value"].clone().requires_grad_(True)
        s, vl, loss, kl = alg._loss_terms(mu, value, b["actions"], b["target_values"], b["advantages"].unsqueeze(1), b["returns"],
                                          b["old_logp"].unsqueeze(1), b["old_mu"], b["old_sigma"])
        loss.backward()
        outs.append([s.detach(), vl.detach(), loss.detach(), kl.detach(), value.grad.clone()]
                    + [p.grad.clone() for p in alg.actor_critic.actor.parameters()] + [alg.actor_critic.std.grad.clone()])
    assert all(torch.equal(a, c) for a, c in zip(*outs))
    assert torch.equal(mc.multi_critic.head_sum, outs[1][1].reshape(1))


# ---- flags and configuration --------------------------------------------------------------------------------------------------------------------
def test_cli_flags_reach_the_config():
    a = get_args([])
    assert a.reward_groups is None and a.reward_group_weights is None
    d = class_to_dict(update_cfg_from_args(None, config.GR1T1CfgPPO(), a)[1])
    assert "reward_groups" not in d["algorithm"] and d == class_to_dict(config.GR1T1CfgPPO())       # the config dump is unchanged
    d = class_to_dict(update_cfg_from_args(None, config.GR1T1CfgPPO(), get_args(["--reward_groups", SPEC, "--reward_group_weights", "1,2"]))[1])
    assert d["algorithm"].pop("reward_groups") == SPEC and d["algorithm"].pop("reward_group_weights") == "1,2"
    assert d == class_to_dict(config.GR1T1CfgPPO())                                                 # ... but for the two keys
    d = class_to_dict(update_cfg_from_args(None, config.GR1T1CfgPPO(), get_args(["--reward_group_weights", "1,2"]))[1])
    assert d == class_to_dict(config.GR1T1CfgPPO())                                                 # the weights travel only with the spec
    for cls in (config.GR1T1CfgPPO, config.GR1T2CfgPPO, config.GR1T1FullBodyCfgPPO):                 # not config keys
        assert not any(k.startswith("reward_group") for k in vars(cls.algorithm))


def test_critic_keyword():
    torch.manual_seed(0)
    a = ActorCriticMLP(5, 9, 3, actor_hidden_dims=[16], critic_hidden_dims=[16])
    torch.manual_seed(0)
    b = ActorCriticMLP(5, 9, 3, actor_hidden_dims=[16], critic_hidden_dims=[16], num_critic_outputs=1)
    assert list(a.state_dict()) == list(b.state_dict()) and all(torch.equal(x, y) for x, y in zip(a.state_dict().values(), b.state_dict().values()))
    c = ActorCriticMLP(5, 9, 3, actor_hidden_dims=[16], critic_hidden_dims=[16], num_critic_outputs=3)
    assert c.num_critic_output == 3 and c.evaluate(torch.zeros(4, 9)).shape == (4, 3) and list(c.state_dict()) == list(a.state_dict())
    for bad in (0, 9, 1.5):
        with pytest.raises(ValueError, match="num_critic_outputs"):
            ActorCriticMLP(5, 9, 3, num_critic_outputs=bad)


class _Sim:
    def __init__(self, n):
        self.n = n

    def tensor(self, name):
        return torch.zeros({"REWARD_TERMS": _capi.NUM_REWARD_TERMS, "BASE_REWARD_TERMS": _capi.NUM_BASE_REWARD_TERMS}[name], self.n)


class _NoEnv:
    num_envs, num_obs, num_pri_obs, num_actions = 8, 39, 168, 10

    def __init__(self, publish=True, only_positive=False):
        self.cfg = types.SimpleNamespace(env=types.SimpleNamespace(publish_reward_terms=publish),
                                         rewards=types.SimpleNamespace(only_positive_rewards=only_positive))
        self.reward_scales = {n: 1.0 for n in _active()}
        self._sim = _Sim(self.num_envs)

    def reset(self):
        return None


def _train_cfg(steps=6):
    tcfg = GR1T1CfgPPO()
    tcfg.runner.num_steps_per_env = steps
    tcfg.algorithm.num_mini_batches, tcfg.algorithm.num_learning_epochs = 3, 2
    tcfg.policy.actor_hidden_dims, tcfg.policy.critic_hidden_dims = [32, 16], [32, 16]
    return tcfg


def _cfg_dict(runner=(), algorithm=(), policy=(), flags=("--reward_groups", SPEC)):
    d = class_to_dict(update_cfg_from_args(None, _train_cfg(), get_args(list(flags)))[1])
    d["runner"].update(runner); d["algorithm"].update(algorithm); d["policy"].update(policy)
    return d


def test_the_flag_alone_builds_a_critic_per_group():
    r = OnPolicyRunner(_NoEnv(), _cfg_dict(), None, "cpu")
    mc = r.alg.multi_critic
    assert isinstance(mc, M.MultiCritic) and mc.K == 2 and mc.weights == [1.0, 1.0] and mc.groups.names == ["track", "rest"]
    assert r.alg.actor_critic.num_critic_output == 2 and r.alg.actor_critic.critic.model[-1].out_features == 2
    assert mc.values.shape == mc.rewards.shape == mc.returns.shape == (6, 8, 2) and r.alg.storage.values.shape == (6, 8, 1)
    assert r.multi_critic == {"groups": {"track": TRACK, "rest": mc.groups.terms["rest"]}, "weights": [1.0, 1.0]}
    assert mc.terms.shape == (_capi.NUM_REWARD_TERMS, 8) and mc.base_terms is None
    r = OnPolicyRunner(_NoEnv(), _cfg_dict(flags=("--reward_groups", SPEC, "--reward_group_weights", "0.5,2")), None, "cpu")
    assert r.alg.multi_critic.weights == [0.5, 2.0]
    with pytest.raises(ValueError, match="--reward_group_weights"):
        OnPolicyRunner(_NoEnv(), _cfg_dict(flags=("--reward_groups", SPEC, "--reward_group_weights", "1,2,3")), None, "cpu")
    with pytest.raises(ValueError, match="active terms are"):
        OnPolicyRunner(_NoEnv(), _cfg_dict(flags=("--reward_groups", "a=tracking_lin_vel;b=*")), None, "cpu")
    with pytest.raises(ValueError, match="needs a spec"):                                          # an empty spec is not "no flag"
        OnPolicyRunner(_NoEnv(), _cfg_dict(flags=("--reward_groups", "")), None, "cpu")
    # composes with: empirical normalisation, both observation histories, a privileged actor, a log noise parameter
    r = OnPolicyRunner(_NoEnv(), _cfg_dict(flags=("--reward_groups", SPEC, "--empirical_normalization", "--obs_history", "2",
                                                  "--critic_obs_history", "3", "--noise_std_type", "log")), None, "cpu")
    assert r.alg.multi_critic.K == 2 and r.alg.actor_critic.num_critic_input == 3 * 168
    r = OnPolicyRunner(_NoEnv(), _cfg_dict(flags=("--reward_groups", SPEC, "--privileged_actor", "--empirical_normalization")), None, "cpu")
    assert r.alg.multi_critic.K == 2 and r.alg.actor_critic.num_actor_input == 168


def test_refused_combinations_in_the_runner(monkeypatch, tmp_path):
    g = ("--reward_groups", SPEC)
    cases = ((dict(flags=g + ("--recurrent", "--rnn_hidden_size", "32")), ValueError, "--recurrent"),
             (dict(flags=g + ("--value_norm", "running")), ValueError, "--value_norm"),
             (dict(flags=g + ("--symmetry", "loss")), ValueError, "--symmetry"),
             (dict(flags=g + ("--smooth", "spatial")), ValueError, "--smooth"),
             (dict(flags=g + ("--grad_penalty_coef", "0.002")), ValueError, "--grad_penalty_coef"),
             (dict(flags=g + ("--state_dependent_std",)), ValueError, "--state_dependent_std"),
             (dict(flags=g + ("--rnd",)), ValueError, "--rnd"),
             (dict(flags=g + ("--estimator",)), ValueError, "--estimator"),
             (dict(flags=g + ("--layer_norm",)), ValueError, "--layer_norm"),
             (dict(flags=g + ("--precision", "bf16")), ValueError, "--precision bf16"),
             (dict(runner={"distill_from": str(tmp_path / "teacher.pt")}), ValueError, "--distill_from"),
             (dict(runner={"exact_resume": True}), NotImplementedError, "--exact_resume"))
    for keys, exc, both in cases:
        with pytest.raises(exc, match=both) as info:
            OnPolicyRunner(_NoEnv(), _cfg_dict(**keys), None, "cpu")
        assert "--reward_groups" in str(info.value), keys                                          # the message names both options
    with pytest.raises(ValueError, match="publish_reward_terms") as info:
        OnPolicyRunner(_NoEnv(publish=False), _cfg_dict(), None, "cpu")
    assert "--reward_groups" in str(info.value)
    with pytest.raises(ValueError, match="only_positive_rewards") as info:
        OnPolicyRunner(_NoEnv(only_positive=True), _cfg_dict(), None, "cpu")
    assert "--reward_groups" in str(info.value)
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    monkeypatch.setattr(dist, "get_rank", lambda *a: 0)
    with pytest.raises(NotImplementedError, match="world size") as info:
        OnPolicyRunner(_NoEnv(), _cfg_dict(), None, "cpu")
    assert "--reward_groups" in str(info.value)


def test_refused_combinations_in_ppo(monkeypatch):
    assert _ppo(2, [1.0, 3.0]).multi_critic.weights == [1.0, 3.0]
    groups = _ppo(2).multi_critic.groups

    def build(ac_kw=(), reward_groups=groups, **kw):
        ac = ActorCriticMLP(5, 9, 3, actor_hidden_dims=[16, 8], critic_hidden_dims=[16, 8], num_critic_outputs=2, **dict(ac_kw))
        return PPO(ac, device="cpu", reward_groups=reward_groups, **kw)
    from wiki_grx_gym_amd.rl.recurrent import ActorCriticRecurrent
    with pytest.raises(ValueError, match="--recurrent") as info:
        PPO(ActorCriticRecurrent(5, 9, 3, rnn_hidden_size=32, actor_hidden_dims=[16], critic_hidden_dims=[16]), device="cpu", reward_groups=groups)
    assert "--reward_groups" in str(info.value)
    maps = types.SimpleNamespace(obs=types.SimpleNamespace(width=5), cobs=types.SimpleNamespace(width=9), actions=types.SimpleNamespace(width=3),
                                 sigma=None)
    cases = ((dict(value_norm="running"), "--value_norm"), (dict(symmetry="loss", symmetry_maps=maps), "--symmetry"),
             (dict(smooth="spatial"), "--smooth"), (dict(grad_penalty_coef=0.002), "--grad_penalty_coef"),
             (dict(ac_kw={"state_dependent_std": True}), "--state_dependent_std"), (dict(ac_kw={"layer_norm": True}), "--layer_norm"))
    for kw, both in cases:
        with pytest.raises(ValueError, match=both) as info:
            build(**kw)
        assert "--reward_groups" in str(info.value), kw
    with pytest.raises(ValueError, match="2 groups, the critic has 1 outputs"):
        PPO(ActorCriticMLP(5, 9, 3), device="cpu", reward_groups=groups)
    with pytest.raises(ValueError, match="RewardGroups"):
        PPO(ActorCriticMLP(5, 9, 3, num_critic_outputs=2), device="cpu", reward_groups=SPEC)
    with pytest.raises(ValueError, match="--reward_group_weights"):
        build(reward_group_weights=[1.0, float("nan")])
    with pytest.raises(ValueError, match="--rnd") as info:                                         # a caller that assigns `rnd` itself
        build().rnd_step(None, 0)
    assert "--reward_groups" in str(info.value)
    bad = M.RewardGroups(groups.names, groups.terms, [2] + groups.term_group[1:], groups.num_main, groups.num_base)
    with pytest.raises(ValueError, match="term_group"):                                            # the map is checked on the host, once
        build(reward_groups=bad)
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    with pytest.raises(NotImplementedError, match="world size") as info:
        build()
    assert "--reward_groups" in str(info.value)


def test_bf16_is_refused_in_ppo(monkeypatch):
    """(precision="bf16" is refused on the CPU before anything else: the multi-critic refusal is reached through the attribute)"""
    alg = _ppo(2)
    alg.precision, alg.multi_critic = "bf16", None
    with pytest.raises(ValueError, match="--precision bf16") as info:
        alg._init_multi_critic(_ppo(2).multi_critic.groups, None)
    assert "--reward_groups" in str(info.value)


def test_checkpoint_entry_round_trips_and_mismatches_are_refused(tmp_path):
    other = "vel=cmd_diff_lin_vel_x;rest=*"
    swapped = ";".join(reversed(SPEC.split(";")))                                                  # the same groups, the heads in the other order
    paths = {}
    for key, flags in ((None, ()), ("spec", ("--reward_groups", SPEC)), ("other", ("--reward_groups", other)),
                       ("swapped", ("--reward_groups", swapped)),
                       ("weights", ("--reward_groups", SPEC, "--reward_group_weights", "1,2"))):
        r = OnPolicyRunner(_NoEnv(), _cfg_dict(flags=flags), None, "cpu")
        paths[key] = str(tmp_path / f"{key}.pt")
        r.save(paths[key])
        ck = torch.load(paths[key], weights_only=False)
        assert ("multi_critic" in ck) == (key is not None)
        if key is None:
            assert set(ck) == {"model_state_dict", "optimizer_state_dict", "iter", "infos"}         # the reference's keys
        else:
            assert ck["multi_critic"] == r.multi_critic and set(ck["multi_critic"]) == {"groups", "weights"}
            assert ck["model_state_dict"]["critic.model.4.weight"].shape[0] == 2
    flags_of = {None: (), "spec": ("--reward_groups", SPEC), "other": ("--reward_groups", other)}
    for mine, theirs in ((None, "spec"), ("spec", None), ("spec", "other"), ("spec", "weights"), ("spec", "swapped")):
        r = OnPolicyRunner(_NoEnv(), _cfg_dict(flags=flags_of[mine]), None, "cpu")
        with pytest.raises(ValueError, match="--reward_groups") as info:
            r.load(paths[theirs])
        assert ("no --reward_groups" if theirs is None else "--reward_group_weights") in str(info.value)
        r.load(paths[mine])                                                                        # its own kind loads
        assert r.multi_critic == torch.load(paths[mine], weights_only=False).get("multi_critic")
    player = OnPolicyRunner(_NoEnv(), _cfg_dict(flags=(), runner={"inference_only": True}), None, "cpu")   # play.py: the actor alone
    assert player.alg.multi_critic is None
    critic = [p.detach().clone() for p in player.alg.actor_critic.critic.parameters()]
    player.load(paths["spec"])
    saved = torch.load(paths["spec"], weights_only=False)["model_state_dict"]
    assert all(torch.equal(p, saved["actor." + n]) for n, p in player.alg.actor_critic.actor.state_dict().items())
    assert all(torch.equal(a, b) for a, b in zip(critic, player.alg.actor_critic.critic.parameters()))


# ---- the runner over the oracle-backed env -------------------------------------------------------------------------------------------------------
def _args(extra=()):
    return get_args(["--task", "GR1T1", "--headless", "--num_envs", "16", "--sim_device", "cpu", "--rl_device", "cpu", "--pipeline", "cpu",
                     "--seed", "3", *extra])


def _make(tmp_path, flags=(), steps=6, publish=True):
    args = _args(flags)
    cfg = GR1T1Cfg()
    if publish is not None:
        cfg.env.publish_reward_terms = publish
    env, _ = task_registry.make_env("GR1T1", args=args, env_cfg=cfg)
    runner, _ = task_registry.make_alg_runner(env, name=None, args=args, train_cfg=_train_cfg(steps), log_root=str(tmp_path) if tmp_path else None)
    return env, runner


def _tags(runner):
    out = {}
    for line in open(os.path.join(runner.log_dir, "scalars.jsonl")):
        out.setdefault(line.split('"tag": "')[1].split('"')[0], []).append(float(line.split('"value": ')[1].split(",")[0]))
    return out


def test_runner_trains_logs_saves_and_resumes(oracle_backend, tmp_path):  # noqa: F811
    env, runner = _make(tmp_path, flags=("--reward_groups", SPEC, "--reward_group_weights", "1,2"))
    alg, mc = runner.alg, runner.alg.multi_critic
    seen = []
    store = mc.store

    def store_and_check(step, values, time_outs, gamma):
        out = store(step, values, time_outs, gamma)
        terms = env._sim.tensor("REWARD_TERMS")
        sums = torch.zeros_like(values)                                                            # the group sums before the bootstrap
        M.mc_store_torch(terms, None, mc.groups.term_group, values, None, gamma, torch.zeros_like(values), sums)
        boot = torch.where(time_outs.reshape(-1, 1) != 0, gamma * values, torch.zeros_like(values))
        assert torch.equal(mc.rewards[step], sums + boot)
        bound = terms.double().abs().sum(0) * _capi.NUM_REWARD_TERMS * 2.0 ** -24
        assert bool(((sums.sum(1).double() - env.rew_buf.double()).abs() <= bound).all())            # the groups add up to the env's reward
        assert torch.equal(out, values.sum(-1, keepdim=True)) and torch.equal(mc.values[step], values)
        seen.append(step)
        return out
    mc.store = store_and_check
    runner.learn(num_learning_iterations=2, init_at_random_ep_len=False)
    assert seen == list(range(6)) * 2
    st = alg.storage
    assert torch.equal(st.values, mc.values.sum(-1, keepdim=True))                                  # the scalar column: sum_k v_k, for logging
    assert torch.isfinite(st.advantages).all() and torch.isfinite(mc.returns).all()
    assert all(bool(torch.isfinite(p).all()) for p in alg.actor_critic.parameters())
    tags = _tags(runner)
    for name in ("track", "rest"):
        assert len(tags["Loss/value_function_" + name]) == 2 and len(tags["Train/adv_std_" + name]) == 2
        assert all(np.isfinite(v) and v > 0 for v in tags["Train/adv_std_" + name])
    for it in range(2):                                                                            # Loss/value_function is the sum over the heads
        assert tags["Loss/value_function"][it] == pytest.approx(tags["Loss/value_function_track"][it] + tags["Loss/value_function_rest"][it], rel=1e-4)
    assert tags["Train/adv_std_track"][1] == pytest.approx(float(mc.stats[0, 1]))
    ck = torch.load(os.path.join(runner.log_dir, "model_2.pt"), weights_only=False)
    assert set(ck) == {"model_state_dict", "optimizer_state_dict", "iter", "infos", "multi_critic"}
    assert ck["multi_critic"]["weights"] == [1.0, 2.0] and list(ck["multi_critic"]["groups"]) == ["track", "rest"]
    args = _args(("--reward_groups", SPEC, "--reward_group_weights", "1,2", "--resume"))
    cfg = GR1T1Cfg()
    cfg.env.publish_reward_terms = True
    env2, _ = task_registry.make_env("GR1T1", args=args, env_cfg=cfg)
    again, _ = task_registry.make_alg_runner(env2, name=None, args=args, train_cfg=_train_cfg(), log_root=str(tmp_path))
    assert again.current_learning_iteration == 2
    sd = again.alg.actor_critic.state_dict()
    assert sd["critic.model.4.weight"].shape[0] == 2
    assert all(torch.equal(sd[k], v) for k, v in ck["model_state_dict"].items() if k != "std")       # (load() resets std to set_noise_std)
    again.learn(num_learning_iterations=1)                                                          # ... and it trains on
    with pytest.raises(ValueError, match="--reward_groups"):                                        # a resume without the flag is refused
        a2 = _args(("--resume",))
        env3, _ = task_registry.make_env("GR1T1", args=a2, env_cfg=GR1T1Cfg())
        task_registry.make_alg_runner(env3, name=None, args=a2, train_cfg=_train_cfg(), log_root=str(tmp_path))


def test_an_env_without_the_tables_is_refused(oracle_backend):  # noqa: F811
    with pytest.raises(ValueError, match="publish_reward_terms"):
        _make(None, flags=("--reward_groups", SPEC), publish=None)                                  # make_env's default: off


def test_train_script_turns_the_tables_on(oracle_backend, monkeypatch):  # noqa: F811
    from wiki_grx_gym_amd.scripts import train as T
    seen = {}

    class Built(Exception):
        pass

    def stop(env, name, args):
        raise Built(env)
    monkeypatch.setattr(task_registry, "make_alg_runner", stop)
    for flags in (("--reward_groups", SPEC), ()):
        cfg, _ = task_registry.get_cfgs("GR1T1")
        if hasattr(cfg.env, "publish_reward_terms"):
            del cfg.env.publish_reward_terms
        try:
            T.train(_args(flags))
        except Built as built:
            seen[bool(flags)] = bool(built.args[0].cfg.env.publish_reward_terms)
    assert seen == {True: True, False: False}
    del task_registry.get_cfgs("GR1T1")[0].env.publish_reward_terms


def test_default_run_is_what_it_was(oracle_backend, tmp_path, monkeypatch):  # noqa: F811
    """without the flag nothing of rl/multi_critic.py is imported, the checkpoint has the reference's keys, and the parameters after the
    first iteration are those of a run whose PPO and policy are built with the new keywords passed at their defaults"""
    monkeypatch.setitem(sys.modules, M.__name__, None)                                              # any import of rl.multi_critic now raises
    _, runner = _make(tmp_path / "a", flags=(), publish=None)
    runner.learn(num_learning_iterations=1)
    assert runner.multi_critic is None and runner.alg.multi_critic is None
    ck = torch.load(os.path.join(runner.log_dir, "model_1.pt"), weights_only=False)
    assert set(ck) == {"model_state_dict", "optimizer_state_dict", "iter", "infos"}
    assert not any("value_function_" in t or "adv_std" in t for t in _tags(runner))
    import wiki_grx_gym_amd.rl.runner as RR
    plain_policy, plain_ppo = RR._POLICIES["ActorCriticMLP"], RR._ALGORITHMS["PPO"]
    monkeypatch.setitem(RR._POLICIES, "ActorCriticMLP", lambda *a, **k: plain_policy(*a, num_critic_outputs=1, **k))
    monkeypatch.setitem(RR._POLICIES, "ActorCritic", lambda *a, **k: plain_policy(*a, num_critic_outputs=1, **k))
    monkeypatch.setitem(RR._ALGORITHMS, "PPO", lambda **k: plain_ppo(reward_groups=None, reward_group_weights=None, **k))
    _, second = _make(tmp_path / "b", flags=(), publish=None)
    second.learn(num_learning_iterations=1)
    ck2 = torch.load(os.path.join(second.log_dir, "model_1.pt"), weights_only=False)
    assert set(ck2) == set(ck) and list(ck2["model_state_dict"]) == list(ck["model_state_dict"])
    assert all(torch.equal(a, b) for a, b in zip(ck["model_state_dict"].values(), ck2["model_state_dict"].values()))
    with pytest.raises(ImportError):
        _make(None, flags=("--reward_groups", SPEC))                                                # (the patch does bite with the flag)


# ---- the C entries ------------------------------------------------------------------------------------------------------------------------------
def test_c_entries_check_their_arguments():
    """invalid sizes, group counts, NULL pointers, misaligned partials, overlapping outputs: negative, nothing launched (no GPU needed; the
    pointers are never followed)"""
    import ctypes as C
    lib = M._lib()
    p = [0x10000000 * k for k in range(1, 16)]
    w = (C.c_float * 8)(*[1.0] * 8)
    assert lib.grx_mc_partials_size(7, 130, 3) == 3 * 3 * 6 and lib.grx_mc_partials_size(7, 64, 1) == 6
    assert lib.grx_mc_partials_size(0, 1, 1) == 0 and lib.grx_mc_partials_size(1, 0, 1) == 0 and lib.grx_mc_partials_size(1, 1, 0) == 0
    assert lib.grx_mc_partials_size(1, 1, 9) == 0 and lib.grx_mc_partials_size(1 << 13, 1 << 12, 1) == 0
    assert lib.grx_mc_loss_partials_size(0) == 0 and lib.grx_mc_loss_partials_size(257) == 2 * 42 * 2

    def store(N=8, K=2, NT=36, NB=15, **kw):
        a = dict(terms=p[0], base=p[1], group=p[2], values=p[3], to=p[4], sv=p[5], sr=p[6]); a.update(kw)
        return lib.grx_mc_store(N, K, NT, NB, a["terms"], a["base"], a["group"], a["values"], a["to"], 0.99, a["sv"], a["sr"], None)
    assert store(N=0) < 0 and store(K=0) < 0 and store(K=9) < 0 and store(NT=0) < 0 and store(NB=-1) < 0 and store(NB=0) < 0 and store(NT=250) < 0
    for name in ("terms", "group", "values", "sv", "sr"):
        assert store(**{name: None}) < 0, name
    assert store(sv=p[3]) < 0 and store(sr=p[5] + 8 * 2 * 4 - 4) < 0 and store(sr=p[0] + 4) < 0        # overlaps

    def rets(T=7, N=8, K=2, weights=w, **kw):
        a = dict(r=p[0], v=p[1], d=p[2], last=p[3], ret=p[4], adv=p[5], stats=p[6], part=p[7]); a.update(kw)
        return lib.grx_mc_returns(T, N, K, a["r"], a["v"], a["d"], a["last"], weights, 0.99, 0.95, a["ret"], a["adv"], a["stats"], a["part"], None)
    assert rets(T=0) < 0 and rets(N=0) < 0 and rets(K=0) < 0 and rets(K=9) < 0 and rets(T=1 << 13, N=1 << 12) < 0
    for name in ("r", "v", "d", "last", "ret", "adv", "stats", "part"):
        assert rets(**{name: None}) < 0, name
    assert rets(weights=None) < 0 and rets(part=p[7] + 4) < 0                                           # a misaligned partials
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert rets(weights=(C.c_float * 8)(1.0, bad)) < 0, bad
    assert rets(ret=p[1]) < 0 and rets(adv=p[4] + 16) < 0 and rets(stats=p[2]) < 0 and rets(part=p[0] + 8) < 0

    def loss(B=257, A=10, K=2, clipped=1, **kw):
        names = ("mu", "std", "value", "actions", "old_logp", "old_mu", "old_sigma", "adv", "ret", "tv", "out", "d_mu", "d_std", "d_value", "part")
        a = dict(zip(names, p)); a.update(kw)
        return lib.grx_mc_loss(B, A, K, *[a[n] for n in names[:10]], 0.2, 1.0, 0.01, clipped, *[a[n] for n in names[10:]], None)
    assert loss(B=0) < 0 and loss(A=0) < 0 and loss(A=33) < 0 and loss(K=0) < 0 and loss(K=9) < 0
    for name in ("mu", "std", "value", "actions", "old_logp", "old_mu", "old_sigma", "adv", "ret", "tv", "out", "d_mu", "d_std", "d_value", "part"):
        assert loss(**{name: None}) < 0, name
    assert loss(part=p[14] + 4) < 0 and loss(d_value=p[2]) < 0 and loss(d_mu=p[0] + 4) < 0 and loss(out=p[11] + 8) < 0
