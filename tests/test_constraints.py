"""Constraints as terminations on the CPU (rl/constraints.py): the spec parser and the ramp, the torch spelling against the
float64 restatement of tests/constraints_ref.py, the properties the definition promises, the flags, every refused combination, the checkpoint
entry, the runner over the oracle-backed env, the default path, and the C entries' argument checks (no GPU: the pointers are never followed)."""
import os
import sys
import types

import numpy as np
import pytest
import torch

from tests import constraints_ref as R
from tests import gae_ref as G
from tests.test_env_plumbing import oracle_backend  # noqa: F401  (the fixture)
from wiki_grx_gym_amd.envs import GR1T1Cfg, GR1T1CfgPPO, config
from wiki_grx_gym_amd.envs.config import class_to_dict
from wiki_grx_gym_amd.rl import constraints as K
from wiki_grx_gym_amd.rl.modules import ActorCriticMLP
from wiki_grx_gym_amd.rl.ppo import PPO
from wiki_grx_gym_amd.rl.runner import OnPolicyRunner
from wiki_grx_gym_amd.rl.storage import RolloutStorage
from wiki_grx_gym_amd.utils import get_args, task_registry
from wiki_grx_gym_amd.utils.helpers import update_cfg_from_args

SPEC = "torque:0.05..0.25,dof_vel:0.05..0.25,dof_pos:0.25,action_rate:0.25@1.5,upright:1.0@0.7"
U = R.U


# ---- the parser and the ramp -------------------------------------------------------------------------------------------------------------------
def test_the_issues_spec_parses():
    s = K.parse_constraints(SPEC)
    assert s.families == [("torque", 0.05, 0.25, None), ("dof_vel", 0.05, 0.25, None), ("dof_pos", 0.25, 0.25, None),
                          ("action_rate", 0.25, 0.25, 1.5), ("upright", 1.0, 1.0, 0.7)]
    assert K.parse_constraints(s) is s and K.parse_constraints(s.text()).key() == s.key()        # the text form round-trips
    assert K.ConstraintSpec(s.key()).key() == s.key()                                             # ... and so does a checkpoint's entry
    one = K.parse_constraints(" upright : 0.5 @ 0.3 ")
    assert one.families == [("upright", 0.5, 0.5, 0.3)]
    assert K.parse_constraints("dof_pos:0,torque:1").names == ["dof_pos", "torque"]               # the spec's order is kept


@pytest.mark.parametrize("spec, what", [
    ("", "needs a spec"), (None, "needs a spec"), (",", "needs a spec"), ("torque", "family:p"), ("torque:", "family:p"),
    ("knee:0.5", "known ones are torque, dof_vel, dof_pos, action_rate, upright"), ("torque:0.1,torque:0.2", "appears twice"),
    ("torque:1.5", r"\[0, 1\]"), ("torque:-0.1", r"\[0, 1\]"), ("torque:0.1..1.2", r"\[0, 1\]"), ("torque:nan", "finite"),
    ("torque:abc", "not a number"), ("torque:0.1@2", "takes no `@L`"), ("dof_vel:0.1@2", "takes no `@L`"), ("dof_pos:0.1@2", "takes no `@L`"),
    ("action_rate:0.1", "needs its limit"), ("upright:0.1", "needs its limit"), ("upright:0.1@", "needs its limit"),
    ("upright:0.1@x", "not a number"), ("action_rate:0.1@-1", ">= 0")])
def test_refused_specs(spec, what):
    with pytest.raises(ValueError, match=what) as info:
        K.parse_constraints(spec)
    assert "--constraints" in str(info.value)


def test_options_are_checked_by_name():
    assert K.check_options(0.95, 1000, "zero") == (0.95, 1000, "zero") and K.check_options(0, 1, "none") == (0.0, 1, "none")
    for tau in (1.0, -0.1, 1.5, float("nan"), "x"):
        with pytest.raises(ValueError, match="--constraint_tau"):
            K.check_options(tau, 1000, "zero")
    for ramp in (0, -5, 2.5, True, None):
        with pytest.raises(ValueError, match="--constraint_ramp_its"):
            K.check_options(0.95, ramp, "zero")
    with pytest.raises(ValueError, match="--constraint_reward_clip"):
        K.check_options(0.95, 1000, "positive")


def test_the_ramp():
    s = K.parse_constraints(SPEC)
    Rm = 1000
    assert s.probabilities(0, Rm) == [0.05, 0.05, 0.25, 0.25, 1.0]
    assert s.probabilities(Rm // 2, Rm) == pytest.approx([0.15, 0.15, 0.25, 0.25, 1.0], abs=1e-15)
    assert s.probabilities(Rm, Rm) == [0.05 + (0.25 - 0.05) * 1.0, 0.05 + (0.25 - 0.05) * 1.0, 0.25, 0.25, 1.0]
    assert s.probabilities(2 * Rm, Rm) == s.probabilities(Rm, Rm)                                # it stays at p_hi
    down = K.parse_constraints("torque:0.5..0.1")                                               # a ramp may go down
    assert down.probabilities(0, 10) == [0.5] and down.probabilities(5, 10) == pytest.approx([0.3]) and down.probabilities(99, 10) == pytest.approx([0.1])
    c = K.Constraints("torque:0.0..1.0,upright:0.5@0.2", ramp_its=4, device="cpu")
    c.bind(_Env(N=3, A=2))
    for it, p in ((0, 0.0), (2, 0.5), (4, 1.0), (8, 1.0)):                                       # the device tensor: one entry per column
        c.set_iteration(it)
        assert c.prob.tolist() == [p, p, 0.5]


# ---- the torch spelling against float64 ----------------------------------------------------------------------------------------------------------
def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if dtype is None else t.to(dtype)


def _table(families, D, A, lims, soft=(0.9, 0.95)):
    spec = K.ConstraintSpec([(n, 0.5, 0.5, lim) for n, lim in families])
    return K.ColumnTable(spec, D, A, lims[0], lims[1], lims[2], soft[0], soft[1], "cpu")


ALL = (("torque", None), ("dof_vel", None), ("dof_pos", None), ("action_rate", 0.4), ("upright", 0.35))


def _run_torch(table, prob, steps, N, A, clip_zero, tau=0.95):
    """`steps`: [(sources, dones, reward row)]; returns per step (delta, row, c_max, prev, counts) of the torch spelling"""
    tau32 = torch.tensor(tau, dtype=torch.float32)
    tau_f, omt_f = tau32.item(), (torch.tensor(1.0) - tau32).item()
    has_rate = 3 in table.kinds
    prev = torch.zeros(N, A) if has_rate else None
    c_max, counts = torch.zeros(table.C), torch.zeros(table.F, dtype=torch.int32)
    out = []
    for k, (src, dones, row) in enumerate(steps):
        delta, r = torch.zeros(N), _t(row).clone()
        K.cat_step_torch(table, prob, _t(src["torques"]), _t(src["dof_vel"]), _t(src["dof_pos"]), _t(src["actions"]), _t(src["gravity"]),
                         _t(dones), tau_f, omt_f, clip_zero, k == 0, prev, c_max, counts, delta, r)
        out.append((delta, r, c_max.clone(), None if prev is None else prev.clone(), counts.clone()))
    return out


@pytest.mark.parametrize("clip_zero", [True, False])
@pytest.mark.parametrize("N, D, A, families", [(1, 1, 1, ALL), (7, 3, 2, ALL), (65, 10, 10, ALL), (33, 12, 10, ALL[:3]), (9, 4, 4, ALL[3:]),
                                               (5, 2, 2, (("upright", 0.35),))])
def test_step_torch_against_the_reference(N, D, A, families, clip_zero):
    """three consecutive steps, so that the running maxima and the previous actions carry over.  The bounds, with u = 2^-24:
      c+, per column : |x| - hi, lo - x, x - hi and |a - prev| - hi are at most 2 rounded operations on numbers of magnitude S_c = max|x| +
                       max|limit|, the upright column 5 on numbers <= 1 + L: b_c = 4 u S_c (6 u (1 + L)); max(., 0) is 1-Lipschitz
      c_max          : the maximum is exact; one update adds 3 roundings of numbers <= M = max c_max and passes (1 - tau) b_c + tau e on:
                       e_k <= b_c + 4 u M k
      delta          : per live column p ((b_c + r e) / c_max + 2 u) with r = c+ / c_max <= 1 after the clip, the maximum 1-Lipschitz.  The
                       inputs keep every violation at least 1 % of its limit away from zero, so no column is live in one evaluation only
      reward row     : |r| (b_delta + 2 u)"""
    lims = R.limits(D)
    table = _table(families, D, A, lims)
    cols = R.columns(list(families), D, A, lims[0], lims[1], lims[2], 0.9, 0.95)
    assert [(int(a), int(b), int(c)) for a, b, c in zip(table.kind, table.src, table.family)] == [c[:3] for c in cols]
    assert table.lo.tolist() == [c[3] for c in cols] and table.hi.tolist() == [c[4] for c in cols]     # the table holds the reference's fp32 limits
    g = np.random.default_rng(N + D)
    prob = g.uniform(0.1, 1.0, len(cols)).astype(np.float32)
    steps = []
    for k in range(3):
        src, dones = R.sources(N, D, A, lims, 0.4, 0.35, k, quiet_column=0)
        steps.append((src, dones, g.uniform(-0.05, 0.1, N).astype(np.float32)))
    got = _run_torch(table, _t(prob), steps, N, A, clip_zero)
    state = {"c_max": np.zeros(len(cols)), "prev": np.zeros((N, A)) if any(n == "action_rate" for n, _ in families) else None,
             "counts": np.zeros(len(families), np.int64)}
    mags = {0: lims[0].max() * 2.5, 1: lims[1].max() * 2.5, 2: np.abs(lims[2]).max() * 2 + 1.0, 3: 0.4 * 8, 4: 1.35}
    b_c = np.array([(6 if c[0] == 4 else 4) * U * mags[c[0]] for c in cols])
    for k, (src, dones, row) in enumerate(steps):
        cplus, delta, new_row, state = R.step(cols, len(families), prob, src, dones, state, 0.95, row, clip_zero, k == 0)
        d32, r32, cm32, prev32, counts32 = got[k]
        M = float(state["c_max"].max())
        e = b_c + 4 * U * M * (k + 1)
        assert np.all(np.abs(cm32.double().numpy() - state["c_max"]) <= e), k
        live = state["c_max"] > 0
        assert np.array_equal(cm32.numpy() > 0, live)
        r = np.where(live, np.minimum(cplus / np.where(live, state["c_max"], 1.0), 1.0), 0.0)
        b_delta = (prob * np.where(live, (b_c + r * e) / np.where(live, state["c_max"], 1.0) + 2 * U, 0.0)).max(1)
        assert np.all(np.abs(d32.double().numpy() - delta) <= b_delta), k
        assert np.all(np.abs(r32.double().numpy() - new_row) <= np.abs(row) * (b_delta + 2 * U)), k
        assert np.array_equal(counts32.numpy(), state["counts"]), k
        if prev32 is not None:
            assert np.array_equal(prev32.double().numpy(), state["prev"]), k                       # copies and zeros: exact
        assert np.all(delta[dones != 0] == 0) and bool((d32[_t(dones) != 0] == 0).all())           # a done row: delta = 0
    assert state["counts"].sum() > 0 or N < 5                                                      # (the inputs do violate)


@pytest.mark.parametrize("T, N", [(1, 1), (2, 7), (5, 65), (7, 130)])
def test_returns_torch_against_the_reference(T, N):
    """the scan does at most 10 rounded operations per step where tests/gae_ref.py's counts 8 (1 - delta and its product with 1 - done are
    the two more): its bounds, every one a sum of terms at most linear in that count, times 10 / 8"""
    r, v, d, p, last = R.rollout(T, N)
    ret32, adv32, stats32 = torch.zeros(T, N), torch.zeros(T, N), torch.zeros(4)
    K.cat_returns_torch(_t(r), _t(v), _t(d), _t(p), _t(last), R.GAMMA, R.LAM, ret32, adv32, stats32)
    ret = R.returns(r, v, d, p, last)
    adv, stats = R.advantages(ret, v)
    ref = {"returns_raw": ret, "a": ret - v.astype(np.float64), "advantages": adv, "stats": stats}
    b = G.bounds(ref, r, v, last)
    assert np.all(np.abs(ret32.double().numpy() - ret) <= 1.25 * b["returns_raw"])
    if T * N > 1:
        assert np.all(np.abs(adv32.double().numpy() - adv) <= 1.25 * b["advantages"])
        assert np.all(np.abs(stats32.double().numpy() - stats) <= 1.25 * b["stats"])
    else:
        assert bool(torch.isnan(adv32).all())                                                      # torch.std of one element


# ---- properties ----------------------------------------------------------------------------------------------------------------------------------
def _storage(T, N, seed=0):
    r, v, d, p, last = R.rollout(T, N, seed)
    st = RolloutStorage(N, T, [3], [None], [2], "cpu")
    st.rewards.copy_(_t(r).unsqueeze(-1)); st.values.copy_(_t(v).unsqueeze(-1)); st.dones.copy_(_t(d).unsqueeze(-1))
    return st, _t(p), _t(last).unsqueeze(-1)


@pytest.mark.parametrize("T, N", [(1, 2), (5, 65), (24, 16)])
def test_zero_probabilities_are_compute_returns_bit_for_bit(T, N):
    st, _, last = _storage(T, N)
    ret, adv = torch.zeros(T, N, 1), torch.zeros(T, N, 1)
    K.cat_returns_torch(st.rewards, st.values, st.dones, torch.zeros(T, N), last, 0.994, 0.9, ret, adv)
    st.compute_returns(last, 0.994, 0.9)
    assert torch.equal(ret, st.returns) and torch.equal(adv, st.advantages)
    c = K.Constraints("upright:1.0@0.5", device="cpu")                                           # ... and through the object PPO holds
    c.init_storage(N, T)
    st2, _, _ = _storage(T, N)
    c.compute_returns(st2, last, 0.994, 0.9)
    assert torch.equal(st2.returns, st.returns) and torch.equal(st2.advantages, st.advantages)


def test_probability_one_at_the_maximum_is_a_done():
    """p = 1 on a violated column at its maximum: delta = 1 exactly (c+ / c_max = 1 with tau = 0), and that row's returns are those of a
    rollout with the done byte set there"""
    N, A = 6, 2
    table = _table((("upright", 0.2),), 1, A, R.limits(1))
    grav = torch.tensor([[0.1, 0.0, -1.0]] * N)
    grav[2] = torch.tensor([0.6, 0.3, -0.7])                                                     # the one violator: it is the column's maximum
    delta, row = torch.zeros(N), torch.full((N,), 0.5)
    K.cat_step_torch(table, torch.ones(1), None, None, None, None, grav, torch.zeros(N, dtype=torch.uint8), 0.0, 1.0, True, True, None,
                     torch.zeros(1), torch.zeros(1, dtype=torch.int32), delta, row)
    assert delta.tolist() == [0, 0, 1.0, 0, 0, 0] and row.tolist() == [0.5, 0.5, 0.0, 0.5, 0.5, 0.5]
    T = 5
    st, _, last = _storage(T, N)
    st.dones.zero_()
    p = torch.zeros(T, N); p[3, 2] = 1.0
    ret, adv = torch.zeros(T, N, 1), torch.zeros(T, N, 1)
    K.cat_returns_torch(st.rewards, st.values, st.dones, p, last, 0.994, 0.9, ret, adv)
    st.dones[3, 2] = 1
    st.compute_returns(last, 0.994, 0.9)
    assert torch.equal(ret, st.returns)


def test_returns_do_not_increase_with_the_probability():
    """non-negative rewards and values: the return of every (step, env) is non-increasing in every delta"""
    T, N = 6, 40
    g = np.random.default_rng(5)
    r, v, last = (_t(g.uniform(0, 1, s).astype(np.float32)) for s in ((T, N), (T, N), (N,)))
    d = _t((g.random((T, N)) < 0.1).astype(np.uint8))
    p_lo = _t(g.uniform(0, 0.6, (T, N)).astype(np.float32))
    p_hi = torch.clamp(p_lo + _t(g.uniform(0, 0.4, (T, N)).astype(np.float32)) * _t((g.random((T, N)) < 0.5).astype(np.float32)), max=1.0)
    out = []
    for p in (torch.zeros(T, N), p_lo, p_hi, torch.ones(T, N)):
        ret, adv = torch.zeros(T, N), torch.zeros(T, N)
        K.cat_returns_torch(r, v, d, p, last, 0.994, 0.9, ret, adv)
        out.append(ret)
    # (a return is a sum of products of non-negative fp32 numbers, each factor 1 - delta rounded monotonically: no tolerance is needed
    #  beyond the rounding of the sums, 10 T u times the magnitude)
    for a, b in zip(out, out[1:]):
        assert bool((b <= a + 10 * T * U * float(a.abs().max())).all())
    assert bool((out[-1] < out[0]).any())


def test_a_quiet_column_keeps_a_zero_maximum_and_yields_no_nan():
    N, D, A = 33, 4, 3
    lims = R.limits(D)
    table = _table(ALL, D, A, lims)
    steps = []
    for k in range(3):
        src, dones = R.sources(N, D, A, lims, 0.4, 0.35, k, quiet_column=1)
        steps.append((src, dones, np.full(N, 0.25, np.float32)))
    got = _run_torch(table, torch.full((table.C,), 0.5), steps, N, A, True)
    for delta, row, c_max, prev, counts in got:
        quiet = [c for c in range(table.C) if int(table.kind[c]) in (0, 1, 2) and int(table.src[c]) == 1]
        assert len(quiet) == 3 and all(float(c_max[c]) == 0.0 for c in quiet) and float(c_max.max()) > 0
        assert bool(torch.isfinite(delta).all()) and bool(torch.isfinite(row).all()) and bool(torch.isfinite(c_max).all())
        assert bool((delta >= 0).all()) and bool((delta <= 0.5).all())


def test_a_done_row_has_no_probability_and_restarts_its_previous_actions():
    N, A = 8, 3
    table = _table((("action_rate", 0.1),), 1, A, R.limits(1))
    actions = torch.arange(N * A, dtype=torch.float32).reshape(N, A) + 1.0                       # every row violates against prev = 0
    dones = torch.tensor([0, 1, 0, 0, 1, 0, 0, 0], dtype=torch.uint8)
    prev, delta, row = torch.zeros(N, A), torch.zeros(N), torch.ones(N)
    counts = torch.zeros(1, dtype=torch.int32)
    K.cat_step_torch(table, torch.ones(A), None, None, None, actions, None, dones, 0.95, 0.05, True, True, prev, torch.zeros(A), counts, delta, row)
    live = dones == 0
    assert bool((delta[~live] == 0).all()) and bool((delta[live] > 0).all()) and bool((row[~live] == 1).all())
    assert bool((prev[~live] == 0).all()) and torch.equal(prev[live], actions[live]) and int(counts[0]) == int(live.sum())
    delta2 = torch.zeros(N)                                                                      # the same actions again: only the restarted rows move
    K.cat_step_torch(table, torch.ones(A), None, None, None, actions, None, torch.zeros(N, dtype=torch.uint8), 0.95, 0.05, True, False, prev,
                     torch.zeros(A), counts, delta2, torch.ones(N))
    assert bool((delta2[live] == 0).all()) and bool((delta2[~live] > 0).all()) and int(counts[0]) == N


def test_the_reward_clip():
    table = _table((("upright", 0.2),), 1, 1, R.limits(1))
    grav = torch.tensor([[0.5, 0.0, -0.8], [0.25, 0.0, -0.9], [0.0, 0.0, -1.0]])
    for clip, want in ((True, [0.0, 0.0, 0.0]), (False, [-0.0, -0.5, -1.0])):
        delta, row = torch.zeros(3), torch.full((3,), -1.0)
        K.cat_step_torch(table, torch.ones(1), None, None, None, None, grav, torch.zeros(3, dtype=torch.uint8), 0.0, 1.0, clip, True, None,
                         torch.zeros(1), torch.zeros(1, dtype=torch.int32), delta, row)
        assert delta[0] == 1.0 and delta[2] == 0.0 and 0 < delta[1] < 1
        assert row.tolist() == pytest.approx(want if clip else [0.0, -(1.0 - float(delta[1])), -1.0])


# ---- flags and configuration --------------------------------------------------------------------------------------------------------------------
def test_cli_flags_reach_the_config():
    a = get_args([])
    assert a.constraints is None and a.constraint_tau == 0.95 and a.constraint_ramp_its == 1000 and a.constraint_reward_clip == "zero"
    d = class_to_dict(update_cfg_from_args(None, config.GR1T1CfgPPO(), a)[1])
    assert d == class_to_dict(config.GR1T1CfgPPO())                                               # the config dump is unchanged
    d = class_to_dict(update_cfg_from_args(None, config.GR1T1CfgPPO(), get_args(
        ["--constraints", SPEC, "--constraint_tau", "0.9", "--constraint_ramp_its", "50", "--constraint_reward_clip", "none"]))[1])
    alg = d["algorithm"]
    assert (alg.pop("constraints"), alg.pop("constraint_tau"), alg.pop("constraint_ramp_its"), alg.pop("constraint_reward_clip")) == \
        (SPEC, 0.9, 50, "none")
    assert d == class_to_dict(config.GR1T1CfgPPO())                                               # ... but for the four keys
    d = class_to_dict(update_cfg_from_args(None, config.GR1T1CfgPPO(), get_args(["--constraint_tau", "0.5"]))[1])
    assert d == class_to_dict(config.GR1T1CfgPPO())                                               # the options travel only with the spec
    for cls in (config.GR1T1CfgPPO, config.GR1T2CfgPPO, config.GR1T1FullBodyCfgPPO):               # not config keys
        assert not any(k.startswith("constraint") for k in vars(cls.algorithm))
    with pytest.raises(SystemExit):
        get_args(["--constraint_reward_clip", "positive"])


class _Env:
    """what the runner and Constraints.bind read of an env, with nothing behind it"""
    num_obs, num_pri_obs = 39, 168

    def __init__(self, N=8, A=10, D=None):
        D = A if D is None else D
        self.num_envs, self.num_actions = N, A
        self.cfg = types.SimpleNamespace(env=types.SimpleNamespace(), normalization=types.SimpleNamespace(clip_actions=100.0),
                                         rewards=types.SimpleNamespace(only_positive_rewards=False, soft_torque_limit=0.9, soft_dof_vel_limit=0.95))
        self.reward_scales = {}
        lims = R.limits(D)
        self.torque_limits, self.dof_vel_limits, self.dof_pos_limits = (_t(x) for x in lims)
        self.torques, self.dof_vel, self.dof_pos = torch.zeros(N, D), torch.zeros(N, D), torch.zeros(N, D)
        self.actions, self.base_projected_gravity = torch.zeros(N, A), torch.tensor([[0.0, 0.0, -1.0]] * N)

    def reset(self):
        return None


def _train_cfg(steps=6):
    tcfg = GR1T1CfgPPO()
    tcfg.runner.num_steps_per_env = steps
    tcfg.algorithm.num_mini_batches, tcfg.algorithm.num_learning_epochs = 3, 2
    tcfg.policy.actor_hidden_dims, tcfg.policy.critic_hidden_dims = [32, 16], [32, 16]
    return tcfg


def _cfg_dict(runner=(), algorithm=(), policy=(), flags=("--constraints", SPEC)):
    d = class_to_dict(update_cfg_from_args(None, _train_cfg(), get_args(list(flags)))[1])
    d["runner"].update(runner); d["algorithm"].update(algorithm); d["policy"].update(policy)
    return d


def test_the_flag_alone_builds_and_binds():
    r = OnPolicyRunner(_Env(), _cfg_dict(), None, "cpu")
    c = r.alg.constraints
    assert isinstance(c, K.Constraints) and c.spec.names == list(K.FAMILIES) and c.table.C == 41 and c.table.F == 5
    assert c.table.ranges == [(0, 10), (10, 20), (20, 30), (30, 40), (40, 41)] and c.table.kind_mask == 31
    assert c.term_prob.shape == (6, 8) and c.prev.shape == (8, 10) and c.c_max.shape == (41,) and float(c.c_max.abs().max()) == 0
    assert (c.tau_option, c.ramp_its, c.reward_clip) == (0.95, 1000, "zero") and c.one_minus_tau == float(np.float32(1) - np.float32(0.95))
    assert r.constraints == {"spec": c.spec.key(), "tau": 0.95, "ramp_its": 1000, "reward_clip": "zero"}
    env = _Env()
    assert torch.equal(c.table.hi[:10], env.torque_limits * 0.9) and torch.equal(c.table.hi[10:20], env.dof_vel_limits * 0.95)
    assert torch.equal(c.table.lo[20:30], env.dof_pos_limits[:, 0]) and torch.equal(c.table.hi[20:30], env.dof_pos_limits[:, 1])
    assert c.table.hi[30:].tolist() == [1.5] * 10 + [float(np.float32(0.7))]
    assert c.prob.tolist() == [float(np.float32(x)) for x in [0.05] * 20 + [0.25] * 20 + [1.0]]
    r = OnPolicyRunner(_Env(), _cfg_dict(flags=("--constraints", "upright:0.5@0.3", "--constraint_tau", "0.5", "--constraint_ramp_its", "7",
                                                "--constraint_reward_clip", "none")), None, "cpu")
    c = r.alg.constraints
    assert c.prev is None and c.table.C == 1 and (c.tau, c.one_minus_tau, c.ramp_its, c.reward_clip) == (0.5, 0.5, 7, "none")
    for flags, what in ((("--constraints", ""), "needs a spec"), (("--constraints", "knee:1"), "known ones"),
                        (("--constraints", SPEC, "--constraint_tau", "1.0"), "--constraint_tau"),
                        (("--constraints", SPEC, "--constraint_ramp_its", "0"), "--constraint_ramp_its")):
        with pytest.raises(ValueError, match=what):
            OnPolicyRunner(_Env(), _cfg_dict(flags=flags), None, "cpu")
    with pytest.raises(ValueError, match="1..256"):                                                # 3 x 86 columns
        OnPolicyRunner(_Env(A=86), _cfg_dict(flags=("--constraints", "torque:1,dof_vel:1,dof_pos:1")), None, "cpu")
    # composes with: empirical normalisation, both observation histories, a privileged actor, a log noise parameter
    r = OnPolicyRunner(_Env(), _cfg_dict(flags=("--constraints", SPEC, "--empirical_normalization", "--obs_history", "2", "--critic_obs_history",
                                                "3", "--noise_std_type", "log")), None, "cpu")
    assert r.alg.constraints.table.C == 41 and r.alg.actor_critic.num_critic_input == 3 * 168
    r = OnPolicyRunner(_Env(), _cfg_dict(flags=("--constraints", SPEC, "--privileged_actor", "--empirical_normalization")), None, "cpu")
    assert r.alg.constraints.table.C == 41 and r.alg.actor_critic.num_actor_input == 168


def test_refused_combinations_in_the_runner(monkeypatch, tmp_path):
    g = ("--constraints", SPEC)
    cases = ((dict(flags=g + ("--recurrent", "--rnn_hidden_size", "32")), ValueError, "--recurrent"),
             (dict(flags=g + ("--value_norm", "running")), ValueError, "--value_norm"),
             (dict(flags=g + ("--reward_groups", "all=*")), ValueError, "--reward_groups"),
             (dict(flags=g + ("--rnd",)), ValueError, "--rnd"),
             (dict(runner={"distill_from": str(tmp_path / "teacher.pt")}), ValueError, "--distill_from"),
             (dict(flags=g + ("--action_dist", "beta", "--action_bounds", "-1", "1")), ValueError, "--action_dist beta"),
             (dict(flags=g + ("--symmetry", "loss")), ValueError, "--symmetry"),
             (dict(flags=g + ("--smooth", "spatial")), ValueError, "--smooth"),
             (dict(flags=g + ("--grad_penalty_coef", "0.002")), ValueError, "--grad_penalty_coef"),
             (dict(flags=g + ("--state_dependent_std",)), ValueError, "--state_dependent_std"),
             (dict(flags=g + ("--layer_norm",)), ValueError, "--layer_norm"),
             (dict(flags=g + ("--estimator",)), ValueError, "--estimator"),
             (dict(flags=g + ("--cenet",)), ValueError, "--cenet"),
             (dict(flags=g + ("--precision", "bf16")), ValueError, "--precision bf16"),
             (dict(runner={"exact_resume": True}), NotImplementedError, "--exact_resume"))
    for keys, exc, both in cases:
        env = _Env()
        if "--reward_groups" in keys.get("flags", ()):                                             # (far enough for the multi-critic's own checks)
            from wiki_grx_gym_amd import _capi
            env.cfg.env.publish_reward_terms = True
            env.reward_scales = {_capi.REWARD_TERMS[0]: 1.0}
        with pytest.raises(exc, match=both) as info:
            OnPolicyRunner(env, _cfg_dict(**keys), None, "cpu")
        assert "--constraints" in str(info.value), keys                                            # the message names both options
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    monkeypatch.setattr(dist, "get_rank", lambda *a: 0)
    with pytest.raises(NotImplementedError, match="world size") as info:
        OnPolicyRunner(_Env(), _cfg_dict(), None, "cpu")
    assert "--constraints" in str(info.value)


def test_refused_combinations_in_ppo(monkeypatch):
    def build(ac_kw=(), constraints=SPEC, **kw):
        ac = ActorCriticMLP(5, 9, 3, actor_hidden_dims=[16, 8], critic_hidden_dims=[16, 8], **dict(ac_kw))
        return PPO(ac, device="cpu", constraints=constraints, **kw)
    alg = build(constraint_tau=0.5, constraint_ramp_its=3, constraint_reward_clip="none")
    assert (alg.constraints.tau_option, alg.constraints.ramp_its, alg.constraints.reward_clip) == (0.5, 3, "none")
    assert build(constraints=K.parse_constraints(SPEC)).constraints.spec.names == list(K.FAMILIES)   # a parsed spec is taken as it is
    assert PPO(ActorCriticMLP(5, 9, 3), device="cpu").constraints is None
    from wiki_grx_gym_amd.rl.recurrent import ActorCriticRecurrent
    with pytest.raises(ValueError, match="--recurrent") as info:
        PPO(ActorCriticRecurrent(5, 9, 3, rnn_hidden_size=32, actor_hidden_dims=[16], critic_hidden_dims=[16]), device="cpu", constraints=SPEC)
    assert "--constraints" in str(info.value)
    maps = types.SimpleNamespace(obs=types.SimpleNamespace(width=5), cobs=types.SimpleNamespace(width=9), actions=types.SimpleNamespace(width=3),
                                 sigma=None)
    cases = ((dict(value_norm="running"), "--value_norm"), (dict(symmetry="loss", symmetry_maps=maps), "--symmetry"),
             (dict(smooth="spatial"), "--smooth"), (dict(grad_penalty_coef=0.002), "--grad_penalty_coef"),
             (dict(ac_kw={"state_dependent_std": True}), "--state_dependent_std"), (dict(ac_kw={"layer_norm": True}), "--layer_norm"),
             (dict(ac_kw={"action_dist": "beta", "action_bounds": ([-1.0] * 3, [1.0] * 3)}), "--action_dist beta"))
    for kw, both in cases:
        with pytest.raises(ValueError, match=both) as info:
            build(**kw)
        assert "--constraints" in str(info.value), kw
    for kw, what in ((dict(constraints="knee:1"), "known ones"), (dict(constraint_tau=1.0), "--constraint_tau"),
                     (dict(constraint_ramp_its=0), "--constraint_ramp_its"), (dict(constraint_reward_clip="x"), "--constraint_reward_clip")):
        with pytest.raises(ValueError, match=what):
            build(**kw)
    with pytest.raises(ValueError, match="--rnd") as info:                                         # a caller that assigns `rnd` itself
        build().rnd_step(None, 0)
    assert "--constraints" in str(info.value)
    for attr, value, both in (("precision", "bf16", "--precision bf16"), ("multi_critic", object(), "--reward_groups")):
        alg = build()                                                                              # (neither is reachable on the CPU through the
        setattr(alg, attr, value)                                                                  #  constructor: through the attribute)
        with pytest.raises(ValueError, match=both) as info:
            alg._init_constraints(SPEC, 0.95, 1000, "zero")
        assert "--constraints" in str(info.value)
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    with pytest.raises(NotImplementedError, match="world size") as info:
        build()
    assert "--constraints" in str(info.value)


def test_checkpoint_entry_round_trips_and_mismatches_are_refused(tmp_path):
    other = "torque:0.1,upright:1.0@0.7"
    swapped = "dof_vel:0.05..0.25,torque:0.05..0.25,dof_pos:0.25,action_rate:0.25@1.5,upright:1.0@0.7"   # the same families, other columns
    flags_of = {None: (), "spec": ("--constraints", SPEC), "other": ("--constraints", other), "swapped": ("--constraints", swapped)}
    paths = {}
    for key, flags in flags_of.items():
        r = OnPolicyRunner(_Env(), _cfg_dict(flags=flags), None, "cpu")
        if key is not None:
            r.alg.constraints.c_max.copy_(torch.arange(r.alg.constraints.table.C, dtype=torch.float32) / 7)
        paths[key] = str(tmp_path / f"{key}.pt")
        r.save(paths[key])
        ck = torch.load(paths[key], weights_only=False)
        assert ("constraints" in ck) == (key is not None)
        if key is None:
            assert set(ck) == {"model_state_dict", "optimizer_state_dict", "iter", "infos"}         # the reference's keys
        else:
            assert set(ck["constraints"]) == {"spec", "tau", "ramp_its", "reward_clip", "c_max"}
            assert {k: v for k, v in ck["constraints"].items() if k != "c_max"} == r.constraints
            assert torch.equal(ck["constraints"]["c_max"], r.alg.constraints.c_max)
    for mine, theirs in ((None, "spec"), ("spec", None), ("spec", "other"), ("spec", "swapped")):
        r = OnPolicyRunner(_Env(), _cfg_dict(flags=flags_of[mine]), None, "cpu")
        with pytest.raises(ValueError, match="--constraints") as info:
            r.load(paths[theirs])
        assert ("no --constraints" if theirs is None else K.parse_constraints(flags_of[theirs][1]).text()) in str(info.value)
        r.load(paths[mine])                                                                        # its own kind loads
        if mine is not None:
            assert torch.equal(r.alg.constraints.c_max, torch.arange(41, dtype=torch.float32) / 7)   # ... and restores the running maxima
            assert float(r.alg.constraints.prev.abs().max()) == 0
    player = OnPolicyRunner(_Env(), _cfg_dict(flags=(), runner={"inference_only": True}), None, "cpu")   # play.py: the actor alone
    assert player.alg.constraints is None
    player.load(paths["spec"])
    saved = torch.load(paths["spec"], weights_only=False)["model_state_dict"]
    assert all(torch.equal(p, saved["actor." + n]) for n, p in player.alg.actor_critic.actor.state_dict().items())


# ---- the runner over the oracle-backed env -------------------------------------------------------------------------------------------------------
def _args(extra=()):
    return get_args(["--task", "GR1T1", "--headless", "--num_envs", "16", "--sim_device", "cpu", "--rl_device", "cpu", "--pipeline", "cpu",
                     "--seed", "3", *extra])


def _make(tmp_path, flags=(), steps=6):
    args = _args(flags)
    env, _ = task_registry.make_env("GR1T1", args=args, env_cfg=GR1T1Cfg())
    runner, _ = task_registry.make_alg_runner(env, name=None, args=args, train_cfg=_train_cfg(steps), log_root=str(tmp_path) if tmp_path else None)
    return env, runner


def _tags(runner):
    out = {}
    for line in open(os.path.join(runner.log_dir, "scalars.jsonl")):
        out.setdefault(line.split('"tag": "')[1].split('"')[0], []).append(float(line.split('"value": ')[1].split(",")[0]))
    return out


RUN_SPEC = "torque:0.05..0.25,dof_vel:0.05..0.25,dof_pos:0.25,action_rate:0.25@0.5,upright:1.0@0.7"


def test_runner_trains_logs_saves_and_resumes(oracle_backend, tmp_path):  # noqa: F811
    """two iterations with the flag: every step's row is the spelling's edit of the stored row, the scalars are logged, the checkpoint holds
    the entry, --resume restores c_max and continues the ramp, a resume with another spec or without the flag is refused.  (An untrained
    policy's actions are N(mu, 1) draws: |a_t - a_{t-1}| is N(0, 2) and exceeds the 0.5 of this spec in most rows)"""
    flags = ("--constraints", RUN_SPEC, "--constraint_ramp_its", "4")
    env, runner = _make(tmp_path, flags=flags)
    alg, c = runner.alg, runner.alg.constraints
    assert c.table.C == 3 * env.dof_pos.shape[1] + env.num_actions + 1
    seen = []
    step = alg.constraint_step

    def step_and_check(t):
        before, c_max = alg.storage.rewards[t].clone(), c.c_max.clone()
        prev = c.prev.clone()
        step(t)
        delta = c.term_prob[t]
        dones = alg.storage.dones[t].reshape(-1) != 0
        assert bool((delta >= 0).all()) and bool((delta <= 1).all()) and bool((delta[dones] == 0).all())
        want = (1.0 - delta) * torch.where(before.reshape(-1) < 0, torch.zeros_like(delta), before.reshape(-1))
        assert torch.equal(alg.storage.rewards[t].reshape(-1), want)
        assert torch.equal(c.prev, torch.where(dones.reshape(-1, 1), torch.zeros_like(env.actions), env.actions))
        rate = (env.actions - prev).abs() - 0.5                                                    # the action-rate columns, from the definition
        rate = torch.where(dones.reshape(-1, 1), torch.zeros_like(rate), torch.where(rate > 0, rate, torch.zeros_like(rate)))
        c0, c1 = c.table.ranges[3]
        assert torch.equal(c.c_max[c0:c1], c.tau * c_max[c0:c1] + c.one_minus_tau * rate.max(dim=0).values)
        seen.append((t, c.iteration, float(delta.max())))
    alg.constraint_step = step_and_check
    runner.learn(num_learning_iterations=2, init_at_random_ep_len=False)
    assert [s[:2] for s in seen] == [(t, it) for it in range(2) for t in range(6)]
    assert max(s[2] for s in seen) > 0 and float(c.c_max.max()) > 0
    assert c.prob[0].item() == float(np.float32(0.05 + 0.2 * 1 / 4))                               # iteration 1 of a ramp over 4
    assert torch.isfinite(alg.storage.advantages).all() and torch.isfinite(alg.storage.returns).all()
    assert all(bool(torch.isfinite(p).all()) for p in alg.actor_critic.parameters())
    tags = _tags(runner)
    names = ["mean_termination_prob"] + [f + s for f in K.FAMILIES for s in ("_violation_rate", "_max")]
    assert sorted(t for t in tags if t.startswith("Constraint/")) == sorted("Constraint/" + n for n in names)
    assert all(len(tags["Constraint/" + n]) == 2 and all(np.isfinite(v) and v >= 0 for v in tags["Constraint/" + n]) for n in names)
    assert tags["Constraint/action_rate_violation_rate"][1] > 0.3 and tags["Constraint/mean_termination_prob"][1] > 0
    assert tags["Constraint/mean_termination_prob"][1] == pytest.approx(float(c.term_prob.mean()))
    assert tags["Constraint/action_rate_max"][1] == pytest.approx(float(c.c_max[slice(*c.table.ranges[3])].max()))
    assert all(0 <= tags["Constraint/" + f + "_violation_rate"][1] <= 1 for f in K.FAMILIES)
    ck = torch.load(os.path.join(runner.log_dir, "model_2.pt"), weights_only=False)
    assert set(ck) == {"model_state_dict", "optimizer_state_dict", "iter", "infos", "constraints"}
    assert ck["constraints"]["spec"] == K.parse_constraints(RUN_SPEC).key() and ck["constraints"]["ramp_its"] == 4
    assert torch.equal(ck["constraints"]["c_max"], c.c_max)
    args = _args(flags + ("--resume",))
    env2, _ = task_registry.make_env("GR1T1", args=args, env_cfg=GR1T1Cfg())
    again, _ = task_registry.make_alg_runner(env2, name=None, args=args, train_cfg=_train_cfg(), log_root=str(tmp_path))
    assert again.current_learning_iteration == 2 and torch.equal(again.alg.constraints.c_max, c.c_max)
    assert float(again.alg.constraints.prev.abs().max()) == 0
    again.learn(num_learning_iterations=1)                                                          # ... and it trains on, the ramp continued
    assert again.alg.constraints.iteration == 2 and again.alg.constraints.prob[0].item() == float(np.float32(0.05 + 0.2 * 2 / 4))
    for other in (("--constraints", "upright:1.0@0.7", "--resume"), ("--resume",)):                 # another spec, no flag: refused
        with pytest.raises(ValueError, match="--constraints"):
            a2 = _args(other)
            env3, _ = task_registry.make_env("GR1T1", args=a2, env_cfg=GR1T1Cfg())
            task_registry.make_alg_runner(env3, name=None, args=a2, train_cfg=_train_cfg(), log_root=str(tmp_path))


def test_default_run_is_what_it_was(oracle_backend, tmp_path, monkeypatch):  # noqa: F811
    """without the flag nothing of rl/constraints.py is imported, the checkpoint has the reference's keys, no Constraint/* scalar is logged,
    and the parameters after the first iteration are those of a run whose PPO is built with the new keywords passed at their defaults"""
    monkeypatch.delitem(sys.modules, K.__name__)
    _, runner = _make(tmp_path / "a")
    runner.learn(num_learning_iterations=1)
    assert K.__name__ not in sys.modules                                                           # sys.modules does not hold rl.constraints
    monkeypatch.setitem(sys.modules, K.__name__, None)                                             # any import of rl.constraints now raises
    assert runner.constraints is None and runner.alg.constraints is None
    ck = torch.load(os.path.join(runner.log_dir, "model_1.pt"), weights_only=False)
    assert set(ck) == {"model_state_dict", "optimizer_state_dict", "iter", "infos"}
    assert not any(t.startswith("Constraint/") for t in _tags(runner))
    import wiki_grx_gym_amd.rl.runner as RR
    plain_ppo = RR._ALGORITHMS["PPO"]
    monkeypatch.setitem(RR._ALGORITHMS, "PPO", lambda **k: plain_ppo(constraints=None, constraint_tau=0.95, constraint_ramp_its=1000,
                                                                      constraint_reward_clip="zero", **k))
    _, second = _make(tmp_path / "b")
    second.learn(num_learning_iterations=1)
    ck2 = torch.load(os.path.join(second.log_dir, "model_1.pt"), weights_only=False)
    assert set(ck2) == set(ck) and list(ck2["model_state_dict"]) == list(ck["model_state_dict"])
    assert all(torch.equal(a, b) for a, b in zip(ck["model_state_dict"].values(), ck2["model_state_dict"].values()))
    with pytest.raises(ImportError):
        _make(None, flags=("--constraints", SPEC))                                                  # (the patch does bite with the flag)


# ---- the C entries ------------------------------------------------------------------------------------------------------------------------------
def test_the_header_is_part_of_grx_ppo_h():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "grx_ppo_cat.h")).read()
    assert '#include "grx_ppo_cat.h"' in open(os.path.join(root, "include", "grx_ppo.h")).read()
    import re
    assert set(re.findall(r"\b(grx_cat_[a-z_]+)\s*\(", hdr)) == {"grx_cat_step", "grx_cat_step_blocks", "grx_cat_returns", "grx_cat_partials_size"}
    assert K.MAX_COLUMNS == int(re.search(r"GRX_CAT_MAX_COLUMNS (\d+)", hdr).group(1))
    for k, name in enumerate(K.FAMILIES):                                                          # a family's position is its kind
        assert int(re.search(rf"GRX_CAT_{name.upper()} (\d+)", hdr).group(1)) == k


def test_c_entries_check_their_arguments():
    """invalid sizes, NULL pointers, a kind without its source, misaligned partials, overlapping outputs: negative, nothing launched (no GPU
    needed; the pointers are never followed)"""
    lib = K._lib()
    for name in ("grx_cat_step", "grx_cat_step_blocks", "grx_cat_returns", "grx_cat_partials_size"):
        assert hasattr(lib, name)
    assert lib.grx_cat_step_blocks(1) == 1 and lib.grx_cat_step_blocks(16) == 1 and lib.grx_cat_step_blocks(17) == 2 and lib.grx_cat_step_blocks(4096) == 256
    assert lib.grx_cat_step_blocks(0) == 0 and lib.grx_cat_step_blocks((1 << 24) + 1) == 0
    assert lib.grx_cat_partials_size(7, 130) == 3 * 12 and lib.grx_cat_partials_size(7, 64) == 12
    assert lib.grx_cat_partials_size(0, 1) == 0 and lib.grx_cat_partials_size(1, 0) == 0 and lib.grx_cat_partials_size(1 << 13, 1 << 12) == 0
    p = [0x10000000 * k for k in range(1, 32)]
    names = ("kind", "src", "family", "lo", "hi", "prob", "torques", "dof_vel", "dof_pos", "actions", "gravity", "dones", "prev", "c_max", "counts",
             "cplus", "part_max", "part_count", "delta", "row")

    def step(N=65, C=41, F=5, D=10, A=10, kinds=31, **kw):
        a = dict(zip(names, p), strides=None); a.update(kw)
        return lib.grx_cat_step(N, C, F, D, A, kinds, *[a[n] for n in names[:11]], a["strides"], a["dones"], 0.95, 0.05, 1, 0, *[a[n] for n in names[12:]], None)
    assert step(N=0) < 0 and step(N=(1 << 24) + 1) < 0 and step(C=0) < 0 and step(C=257) < 0 and step(F=0) < 0 and step(F=9) < 0
    assert step(kinds=0) < 0 and step(kinds=32) < 0 and step(D=0) < 0 and step(A=0) < 0
    for name in ("kind", "src", "family", "lo", "hi", "prob", "dones", "c_max", "counts", "cplus", "part_max", "part_count", "delta", "row"):
        assert step(**{name: None}) < 0, name
    for name in ("torques", "dof_vel", "dof_pos", "actions", "gravity", "prev"):                     # a family whose source is missing
        assert step(**{name: None}) < 0, name
    assert step(row=p[18]) < 0 and step(delta=p[11]) < 0 and step(c_max=p[5] + 4) < 0 and step(cplus=p[6] + 64) < 0 and step(prev=p[9]) < 0
    assert step(part_max=p[15] + 65 * 41 * 4 - 4) < 0 and step(counts=p[2]) < 0 and step(row=p[11] + 64) < 0
    import ctypes as C
    soa = (C.c_longlong * 10)(*[1, 65] * 5)                                                           # the env's views: strides (1, N)
    assert step(strides=(C.c_longlong * 10)(*[1, 65, 1, 65, -1, 65, 1, 65, 1, 65])) < 0               # a negative stride
    assert step(strides=soa, row=p[6] + 4 * (9 * 65 + 64)) < 0 and step(row=p[6] + 4 * (9 * 65 + 64)) < 0   # the spans follow the strides

    def rets(T=7, N=8, **kw):
        a = dict(r=p[0], v=p[1], d=p[2], prob=p[3], last=p[4], ret=p[5], adv=p[6], stats=p[7], part=p[8]); a.update(kw)
        return lib.grx_cat_returns(T, N, a["r"], a["v"], a["d"], a["prob"], a["last"], 0.99, 0.95, a["ret"], a["adv"], a["stats"], a["part"], None)
    assert rets(T=0) < 0 and rets(N=0) < 0 and rets(T=1 << 13, N=1 << 12) < 0
    for name in ("r", "v", "d", "prob", "last", "ret", "adv", "stats", "part"):
        assert rets(**{name: None}) < 0, name
    assert rets(part=p[8] + 4) < 0                                                                   # a misaligned partials
    assert rets(ret=p[1]) < 0 and rets(adv=p[5] + 16) < 0 and rets(stats=p[3]) < 0 and rets(part=p[0] + 8) < 0 and rets(ret=p[3] + 4) < 0
