"""Random network distillation (rl/rnd.py) on the CPU: the torch spelling of the reward against the float64 reference
(tests/rnd_ref.py), the weight schedules, the update, and the runner over the oracle-backed env."""
import os

import numpy as np
import pytest
import torch

from tests import rnd_ref as R
from tests.test_env_plumbing import oracle_backend  # noqa: F401  (the fixture)
from wiki_grx_gym_amd.envs import GR1T1Cfg, GR1T1CfgPPO, config
from wiki_grx_gym_amd.envs.config import class_to_dict
from wiki_grx_gym_amd.rl import rnd as M
from wiki_grx_gym_amd.rl.runner import OnPolicyRunner
from wiki_grx_gym_amd.utils import get_args, task_registry
from wiki_grx_gym_amd.utils.helpers import update_cfg_from_args


# ---- the reward ------------------------------------------------------------------------------------------------------------------------------
class TorchState:
    """ret and the statistics as rl/rnd.py keeps them, and one call of a reward function on them"""

    def __init__(self, N, fn, device="cpu"):
        z = lambda *s, **k: torch.zeros(*s, device=device, **k)
        self.fn, self.device = fn, device
        self.ret, self.count, self.mean = z(N), z(1, dtype=torch.long), z(1)
        self.var, self.std = torch.ones(1, device=device), torch.ones(1, device=device)
        self.intrinsic, self.raw = z(N), z(N)

    def __call__(self, pred, targ, rew, weight):
        t = lambda a: torch.from_numpy(np.array(a)).to(self.device)
        rewards = t(rew)
        self.fn(t(pred), t(targ), R.GAMMA, weight, R.EPS, self.ret, self.count, self.mean, self.var, self.std, rewards, self.intrinsic, self.raw)
        n = lambda x: x.detach().cpu().numpy().copy()
        return dict(raw=n(self.raw), ret=n(self.ret), intrinsic=n(self.intrinsic), rewards=n(rewards), mean=n(self.mean)[0], var=n(self.var)[0],
                    std=n(self.std)[0], count=n(self.count)[0])


@pytest.mark.parametrize("E", [1, 3, 32])
@pytest.mark.parametrize("N", [1, 5, 257])
def test_reward_torch_against_the_reference(N, E):
    R.check_sequence(N, E, TorchState(N, M.rnd_reward_torch), where="torch cpu")


def test_reference_without_raw_and_weight_zero():
    """raw is optional; weight 0 leaves the rewards alone and still advances the return"""
    N, E = 5, 3
    pred, targ, rew = R.inputs(N, E)[0]
    st = TorchState(N, M.rnd_reward_torch)
    rewards = torch.from_numpy(np.array(rew))
    M.rnd_reward_torch(torch.from_numpy(np.array(pred)), torch.from_numpy(np.array(targ)), R.GAMMA, 0.0, R.EPS, st.ret, st.count, st.mean, st.var,
                       st.std, rewards, st.intrinsic, None)
    assert torch.equal(rewards, torch.from_numpy(np.array(rew))) and float(st.intrinsic.abs().max()) == 0.0
    assert int(st.count) == N and bool((st.ret > 0).all())


# ---- the schedules ---------------------------------------------------------------------------------------------------------------------------
def test_weight_schedules_at_and_around_their_break_points():
    for it in (0, 1, 10 ** 6):
        assert M.weight_at(it, 0.1) == R.weight_at(it, 0.1) == 0.1
    lin = dict(weight=0.5, schedule="linear", final_weight=0.1, start_it=10, end_it=20)
    want = {0: 0.5, 9: 0.5, 10: 0.5, 11: 0.46, 15: 0.3, 19: 0.14, 20: 0.1, 21: 0.1, 1000: 0.1}
    for it, w in want.items():
        assert M.weight_at(it, **lin) == pytest.approx(w, abs=1e-12) and R.weight_at(it, **lin) == pytest.approx(w, abs=1e-12), it
    assert M.weight_at(10, **lin) == 0.5 and M.weight_at(20, **lin) == 0.1                      # exact at both ends
    up = dict(weight=0.0, schedule="linear", final_weight=1.0, start_it=0, end_it=4)
    assert [M.weight_at(i, **up) for i in range(6)] == [0.0, 0.25, 0.5, 0.75, 1.0, 1.0]
    stp = dict(weight=0.2, schedule="step", final_weight=0.0, at_it=7)
    assert [M.weight_at(i, **stp) for i in (0, 6, 7, 8)] == [0.2, 0.2, 0.0, 0.0] == [R.weight_at(i, **stp) for i in (0, 6, 7, 8)]
    assert M.weight_at(3, 0.3, "step", None, at_it=2) == 0.3                                      # no final weight: the weight itself
    with pytest.raises(ValueError, match="schedule"):
        M.weight_at(0, 0.1, "cosine")
    rnd = M.RandomNetworkDistillation(4, 2, 2, weight=0.5, weight_schedule="linear", final_weight=0.1, start_it=10, end_it=20)
    rnd.iteration = 15
    assert rnd.weight() == pytest.approx(0.3) and rnd.weight(20) == 0.1 and rnd.weight(0) == 0.5


# ---- the update ------------------------------------------------------------------------------------------------------------------------------
def _filled(seed=0, N=16, T=6, S=12, E=8, **kw):
    torch.manual_seed(seed)
    rnd = M.RandomNetworkDistillation(S, N, T, "cpu", num_outputs=E, predictor_hidden_dims=(32, 16), target_hidden_dims=(32, 16), **kw)
    rows = torch.zeros(T, N, 1)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.inference_mode():
        for t in range(T):
            rnd.rollout_step(3.0 + 2.0 * torch.randn(N, S, generator=g), rows[t], t)
    return rnd, rows


def test_rollout_step_stores_what_the_update_reads():
    rnd, rows = _filled()
    assert int(rnd.normalizer.count) == 6 * 16 and int(rnd.ret_count) == 6 * 16
    with torch.no_grad():
        assert torch.allclose(rnd.targets, rnd.target(rnd.states), atol=1e-6)
        r = (rnd.targets[5] - rnd.predictor(rnd.states[5])).norm(dim=1)
    assert torch.allclose(rnd.intrinsic[5], 0.1 * r / (rnd.ret_std + 1e-2), rtol=1e-5)
    assert torch.equal(rows.squeeze(-1), rnd.intrinsic) and bool((rnd.intrinsic > 0).all())
    assert not any(p.requires_grad for p in rnd.target.parameters()) and all(p.requires_grad for p in rnd.predictor.parameters())
    with pytest.raises(AssertionError, match="overflow"):
        rnd.rollout_step(torch.zeros(16, 12), rows[0], 6)
    with pytest.raises(ValueError, match="frame"):
        rnd.rollout_step(torch.zeros(16, 11), rows[0], 0)


def test_target_stays_frozen_and_the_predictor_moves():
    rnd, _ = _filled()
    targ = [p.detach().clone() for p in rnd.target.parameters()]
    pred = [p.detach().clone() for p in rnd.predictor.parameters()]
    loss = rnd.update(2, 3)
    assert np.isfinite(loss) and loss > 0
    assert all(torch.equal(a, b) for a, b in zip(targ, rnd.target.parameters()))                 # bitwise
    assert all(not torch.equal(a, b) for a, b in zip(pred, rnd.predictor.parameters()))          # every tensor has moved


def test_repeated_updates_on_one_rollout_lower_the_loss():
    rnd, _ = _filled(seed=4)
    torch.manual_seed(5)
    losses = [rnd.update(1, 1) for _ in range(20)]
    print("rnd losses over 20 steps:", [round(x, 5) for x in losses])
    assert losses[-1] < losses[0]


def test_a_poisoned_frame_skips_every_step():
    rnd, _ = _filled()
    rnd.states[2, 3, 1] = float("nan")
    before = [p.detach().clone() for p in rnd.predictor.parameters()]
    assert rnd.update(2, 1) == 0.0                                                                # every minibatch holds the row
    assert all(torch.equal(a, b) for a, b in zip(before, rnd.predictor.parameters()))


def test_constructor_refusals():
    for kw, word in ((dict(weight_schedule="cosine"), "schedule"), (dict(state="critic"), "state"), (dict(num_outputs=0), "num_outputs"),
                     (dict(num_outputs=257), "num_outputs")):
        with pytest.raises(ValueError, match=word):
            M.RandomNetworkDistillation(4, 2, 2, **kw)


# ---- the runner over the oracle-backed env ---------------------------------------------------------------------------------------------------
def _args(extra=()):
    return get_args(["--task", "GR1T1", "--headless", "--num_envs", "16", "--sim_device", "cpu", "--rl_device", "cpu", "--pipeline", "cpu",
                     "--seed", "3", *extra])


def _train_cfg(steps=6):
    tcfg = GR1T1CfgPPO()
    tcfg.runner.num_steps_per_env = steps
    tcfg.algorithm.num_mini_batches, tcfg.algorithm.num_learning_epochs = 3, 2
    tcfg.policy.actor_hidden_dims, tcfg.policy.critic_hidden_dims = [32, 16], [32, 16]
    return tcfg


def _make(tmp_path, flags=("--rnd",), env_cfg=None, steps=6):
    args = _args(flags)
    env, _ = task_registry.make_env("GR1T1", args=args, env_cfg=env_cfg if env_cfg is not None else GR1T1Cfg())
    runner, _ = task_registry.make_alg_runner(env, name=None, args=args, train_cfg=_train_cfg(steps), log_root=str(tmp_path) if tmp_path else None)
    return env, runner


def _tags(runner):
    out = {}
    for line in open(os.path.join(runner.log_dir, "scalars.jsonl")):
        out.setdefault(line.split('"tag": "')[1].split('"')[0], []).append(float(line.split('"value": ')[1].split(",")[0]))
    return out


def test_runner_adds_the_intrinsic_reward_saves_and_resumes(oracle_backend, tmp_path, capsys):  # noqa: F811
    cfg = GR1T1Cfg()
    cfg.env.episode_length_s = 0.1           # 5 steps: every env times out inside each rollout, so the bootstrap term is there
    env, runner = _make(tmp_path, env_cfg=cfg)
    alg, rnd = runner.alg, runner.rnd
    assert isinstance(rnd, M.RandomNetworkDistillation) and alg.rnd is rnd and rnd.num_states == env.num_pri_obs == 168 and rnd.num_outputs == 32
    assert rnd.config["weight"] == 0.1 and rnd.reward_gamma == 0.99 and rnd.eps == 1e-2 and rnd.learning_rate == 1e-3
    assert [m.out_features for m in rnd.predictor.model if hasattr(m, "out_features")] == [256, 128, 32]
    target0 = [p.detach().clone() for p in rnd.target.parameters()]
    ext_rows, snaps, totals = [], [], []
    cur = torch.zeros(16)
    process, returns = alg.process_env_step, alg.compute_returns

    def process_and_snap(rewards, dones, infos, log=None):
        nonlocal cur
        step, values = alg.storage.step, alg.transition.values.clone()
        want = rewards.clone()
        if "time_outs" in infos:
            want += alg.gamma * (values.squeeze(1) * infos["time_outs"])
        process(rewards, dones, infos, log=log)
        assert torch.equal(alg.storage.rewards[step].squeeze(1), want)                            # the env's reward plus the bootstrap, as ever
        ext_rows.append(want)
        cur = cur + rewards
        totals.extend(cur[dones > 0].tolist())
        cur = cur * (dones <= 0)

    def snap_and_returns(last):
        snaps.append((alg.storage.rewards.squeeze(-1).clone(), rnd.intrinsic.clone(), torch.stack(ext_rows[-6:])))
        return returns(last)
    alg.process_env_step, alg.compute_returns = process_and_snap, snap_and_returns
    runner.learn(num_learning_iterations=2, init_at_random_ep_len=False)
    assert len(snaps) == 2
    for total, intrinsic, ext in snaps:
        assert torch.equal(total, ext + intrinsic) and bool((intrinsic > 0).all())               # elementwise, before compute_returns
    assert any(bool((e != 0).any()) for _, _, e in snaps)
    rewbuffer = list(runner._log_buffers[2])
    assert len(totals) >= 16 and rewbuffer == totals[-100:]                                      # "Mean reward" is the extrinsic total
    assert all(torch.equal(a, b) for a, b in zip(target0, rnd.target.parameters()))
    tags = _tags(runner)
    assert len(tags["Loss/rnd"]) == 2 and all(np.isfinite(v) and v > 0 for v in tags["Loss/rnd"] + tags["Train/mean_intrinsic_reward"])
    assert tags["Train/rnd_weight"] == [0.1, 0.1]
    assert tags["Train/mean_intrinsic_reward"][1] == pytest.approx(float(snaps[1][1].mean()), rel=1e-6)

    ck_path = os.path.join(runner.log_dir, "model_2.pt")
    ck = torch.load(ck_path, weights_only=False)
    assert set(ck) == {"model_state_dict", "optimizer_state_dict", "iter", "infos", "rnd"}
    assert set(ck["rnd"]) == {"state_dict", "optimizer_state_dict", "config"} and ck["rnd"]["config"]["state"] == "privileged"
    for k in ("ret", "ret_count", "ret_mean", "ret_var", "ret_std", "normalizer._mean", "normalizer.count", "target.model.0.weight",
              "predictor.model.4.bias"):
        assert k in ck["rnd"]["state_dict"], k
    assert int(ck["rnd"]["state_dict"]["ret_count"]) == 2 * 6 * 16

    capsys.readouterr()
    args = _args(("--rnd", "--resume"))                                                          # --resume: the last run under the log root
    env2, _ = task_registry.make_env("GR1T1", args=args, env_cfg=GR1T1Cfg())
    again, _ = task_registry.make_alg_runner(env2, name=None, args=args, train_cfg=_train_cfg(), log_root=str(tmp_path))
    assert "rnd entry" not in capsys.readouterr().out
    sd, sd2 = rnd.state_dict(), again.rnd.state_dict()
    assert set(sd) == set(sd2) and all(torch.equal(sd[k], sd2[k]) for k in sd)                   # ret, statistics, target, predictor: bitwise
    assert again.current_learning_iteration == 2
    st, st2 = rnd.optimizer.state_dict()["state"], again.rnd.optimizer.state_dict()["state"]
    assert all(torch.equal(st[i]["exp_avg"], st2[i]["exp_avg"]) for i in st)
    again.learn(num_learning_iterations=1)                                                       # ... and it trains on

    _, plain = _make(None, flags=())
    assert plain.rnd is None and plain.alg.rnd is None
    plain.load(ck_path)                                                                          # play.py's case
    out = capsys.readouterr().out
    assert out.count("holds an rnd entry, this runner has no --rnd: ignored") == 1
    plain.save(str(tmp_path / "plain.pt"))
    assert "rnd" not in torch.load(tmp_path / "plain.pt", weights_only=False)
    _, fresh = _make(None)
    fresh.load(str(tmp_path / "plain.pt"))
    out = capsys.readouterr().out
    assert out.count("holds no rnd entry: random network distillation starts fresh") == 1 and int(fresh.rnd.ret_count) == 0
    _, other = _make(None, flags=("--rnd", "--rnd_num_outputs", "16"))
    with pytest.raises(ValueError, match="num_outputs"):
        other.load(ck_path)
    _, no_opt = _make(None)
    no_opt.load(ck_path, load_optimizer=False)                                                   # the flag holds for RND's Adam too
    assert len(no_opt.rnd.optimizer.state_dict()["state"]) == 0 and len(no_opt.alg.optimizer.state_dict()["state"]) == 0
    assert all(torch.equal(sd[k], v) for k, v in no_opt.rnd.state_dict().items())
    capsys.readouterr()
    args8 = get_args(["--task", "GR1T1", "--headless", "--num_envs", "8", "--sim_device", "cpu", "--rl_device", "cpu", "--pipeline", "cpu",
                      "--seed", "3", "--rnd"])
    env8, _ = task_registry.make_env("GR1T1", args=args8, env_cfg=GR1T1Cfg())
    fewer, _ = task_registry.make_alg_runner(env8, name=None, args=args8, train_cfg=_train_cfg(), log_root=None)
    fewer.load(ck_path)                                                                          # another --num_envs: ret restarts, the rest is kept
    assert capsys.readouterr().out.count("restart from zero") == 1
    sd8 = fewer.rnd.state_dict()
    assert sd8["ret"].shape == (8,) and float(sd8["ret"].abs().max()) == 0.0
    assert all(torch.equal(sd[k], sd8[k]) for k in sd if k != "ret")
    fewer.learn(num_learning_iterations=1)


class _NoEnv:
    num_envs, num_obs, num_pri_obs, num_actions = 8, 39, 168, 10

    def reset(self):
        return None


class _NoPriEnv(_NoEnv):
    num_pri_obs = None


def _cfg_dict(runner=(), algorithm=(), flags=("--rnd",)):
    d = class_to_dict(update_cfg_from_args(None, _train_cfg(), get_args(list(flags)))[1])
    d["runner"].update(runner); d["algorithm"].update(algorithm)
    return d


def test_refused_combinations(monkeypatch, tmp_path):
    r = OnPolicyRunner(_NoEnv(), _cfg_dict(), None, "cpu")                                        # the flag alone is fine
    assert r.rnd is not None and not any(k.startswith("rnd") for k in r.algorithm_cfg)
    for keys, exc, both in ((dict(runner={"distill_from": str(tmp_path / "teacher.pt")}), ValueError, "--distill_from"),
                            (dict(runner={"exact_resume": True}), NotImplementedError, "--exact_resume")):
        with pytest.raises(exc, match=both) as info:
            OnPolicyRunner(_NoEnv(), _cfg_dict(**keys), None, "cpu")
        assert "--rnd" in str(info.value), keys                                                  # the message names both options
    with pytest.raises(ValueError, match="privileged"):
        OnPolicyRunner(_NoPriEnv(), _cfg_dict(), None, "cpu")
    assert OnPolicyRunner(_NoPriEnv(), _cfg_dict(flags=("--rnd", "--rnd_state", "obs")), None, "cpu").rnd.num_states == 39
    with pytest.raises(ValueError, match="rnd_state"):
        OnPolicyRunner(_NoEnv(), _cfg_dict(algorithm={"rnd_state": "critic"}), None, "cpu")
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    monkeypatch.setattr(dist, "get_rank", lambda *a: 0)
    with pytest.raises(NotImplementedError, match="world size") as info:
        OnPolicyRunner(_NoEnv(), _cfg_dict(), None, "cpu")
    assert "--rnd" in str(info.value)


def test_cli_flags_reach_the_configs():
    a = get_args([])
    assert a.rnd is False and a.rnd_weight == 0.1 and a.rnd_weight_schedule == "constant" and a.rnd_state == "privileged"
    assert a.rnd_num_outputs == 32 and a.rnd_learning_rate == 1e-3
    d = class_to_dict(update_cfg_from_args(None, config.GR1T1CfgPPO(), a)[1])
    assert not any(k.startswith("rnd") for k in d["algorithm"])
    d = class_to_dict(update_cfg_from_args(None, config.GR1T1CfgPPO(), get_args(["--rnd_weight", "0.5"]))[1])
    assert not any(k.startswith("rnd") for k in d["algorithm"])                                  # without --rnd: nothing
    d = class_to_dict(update_cfg_from_args(None, config.GR1T1CfgPPO(), get_args(["--rnd"]))[1])["algorithm"]
    assert d["rnd"] is True and d["rnd_weight"] == 0.1 and d["rnd_weight_schedule"] == "constant" and d["rnd_final_weight"] is None
    assert d["rnd_state"] == "privileged" and d["rnd_num_outputs"] == 32 and d["rnd_learning_rate"] == 1e-3
    flags = ["--rnd", "--rnd_weight", "0.4", "--rnd_weight_schedule", "linear", "--rnd_final_weight", "0.05", "--rnd_start_it", "100",
             "--rnd_end_it", "500", "--rnd_state", "obs", "--rnd_num_outputs", "16", "--rnd_learning_rate", "3e-4"]
    d = class_to_dict(update_cfg_from_args(None, _train_cfg(), get_args(flags))[1])
    a = d["algorithm"]
    assert (a["rnd_weight"], a["rnd_weight_schedule"], a["rnd_final_weight"], a["rnd_start_it"], a["rnd_end_it"]) == (0.4, "linear", 0.05, 100, 500)
    rnd = OnPolicyRunner(_NoEnv(), d, None, "cpu").rnd
    assert rnd.state == "obs" and rnd.num_states == 39 and rnd.num_outputs == 16 and rnd.learning_rate == 3e-4
    assert rnd.weight(0) == 0.4 and rnd.weight(300) == pytest.approx(0.225) and rnd.weight(500) == 0.05
    d = class_to_dict(update_cfg_from_args(None, _train_cfg(), get_args(["--rnd", "--rnd_weight_schedule", "step", "--rnd_final_weight", "0",
                                                                         "--rnd_at_it", "3"]))[1])
    rnd = OnPolicyRunner(_NoEnv(), d, None, "cpu").rnd
    assert [rnd.weight(i) for i in (2, 3)] == [0.1, 0.0]
    with pytest.raises(SystemExit):
        get_args(["--rnd_weight_schedule", "cosine"])
    for cls in (config.GR1T1CfgPPO, config.GR1T2CfgPPO, config.GR1T1FullBodyCfgPPO):               # not config keys
        assert not any(k.startswith("rnd") for k in vars(cls.algorithm))


@pytest.mark.parametrize("flags", [("--recurrent", "--rnn_hidden_size", "32"), ("--symmetry", "augment"), ("--obs_history", "3"),
                                   ("--empirical_normalization",), ("--privileged_actor", "--critic_obs_history", "2")])
def test_compositions_train(oracle_backend, tmp_path, flags):  # noqa: F811
    env, runner = _make(tmp_path, flags=("--rnd", *flags))
    before = [p.detach().clone() for p in runner.rnd.predictor.parameters()]
    policy = [p.detach().clone() for p in runner.alg.actor_critic.parameters()]
    runner.learn(num_learning_iterations=2)
    assert all(not torch.equal(a, b) and bool(torch.isfinite(b).all()) for a, b in zip(before, runner.rnd.predictor.parameters()))
    assert all(bool(torch.isfinite(b).all()) for b in runner.alg.actor_critic.parameters())
    assert any(not torch.equal(a, b) for a, b in zip(policy, runner.alg.actor_critic.parameters()))
    assert int(runner.rnd.ret_count) == 2 * 6 * 16 and int(runner.rnd.normalizer.count) == 2 * 6 * 16 and runner.rnd.normalizer.dim == 168
    tags = _tags(runner)
    assert len(tags["Loss/rnd"]) == 2 and all(np.isfinite(v) for v in tags["Loss/rnd"] + tags["Train/mean_intrinsic_reward"])
    assert "rnd" in torch.load(os.path.join(runner.log_dir, "model_2.pt"), weights_only=False)


def test_default_path_constructs_nothing(oracle_backend, tmp_path, monkeypatch):  # noqa: F811
    def boom(self, *a, **k):
        raise AssertionError("RandomNetworkDistillation constructed without --rnd")
    monkeypatch.setattr(M.RandomNetworkDistillation, "__init__", boom)
    _, runner = _make(tmp_path, flags=())
    runner.learn(num_learning_iterations=1)
    assert runner.rnd is None and runner.alg.rnd is None
    ck = torch.load(os.path.join(runner.log_dir, "model_1.pt"), weights_only=False)
    assert set(ck) == {"model_state_dict", "optimizer_state_dict", "iter", "infos"}
    assert not any(t.startswith(("Loss/rnd", "Train/rnd", "Train/mean_intrinsic")) for t in _tags(runner))
    with pytest.raises(AssertionError, match="without --rnd"):
        _make(None)                                                                              # (the patch does bite with the flag)
