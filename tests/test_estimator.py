"""The concurrent state estimator (rl/estimator.py) on the CPU: the torch spelling of the forward against the float64
reference (tests/est_ref.py), flags and refusals, the alignment of stored rows and targets, learnability, the untouched PPO update, the
checkpoint, resume, inference and export, the compositions, and the C entry's argument checks."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import est_ref as R
from tests.test_env_plumbing import oracle_backend  # noqa: F401  (the fixture)
from wiki_grx_gym_amd.envs import GR1T1Cfg, GR1T1CfgPPO, config
from wiki_grx_gym_amd.envs.config import class_to_dict
from wiki_grx_gym_amd.rl import estimator as M
from wiki_grx_gym_amd.rl.history import ObsHistory
from wiki_grx_gym_amd.rl.modules import MLP
from wiki_grx_gym_amd.rl.runner import OnPolicyRunner
from wiki_grx_gym_amd.utils import export_policy_as_jit, get_args, task_registry
from wiki_grx_gym_amd.utils.helpers import update_cfg_from_args

ALL = "lin_vel,base_height,feet_contact,feet_height"


# ---- the forward -----------------------------------------------------------------------------------------------------------------------------
def _lin(net):
    mods = [m for m in net.model if isinstance(m, torch.nn.Linear)]
    return [m.weight.detach().numpy() for m in mods], [m.bias.detach().numpy() for m in mods]


@pytest.mark.parametrize("hidden", [(32,), (48, 33), (256, 128, 64)])
@pytest.mark.parametrize("N,D,E", [(1, 39, 1), (65, 40, 3), (130, 195, 8)])
def test_forward_torch_against_the_reference(N, D, E, hidden):
    torch.manual_seed(N + D + E)
    net = MLP(D, E, list(hidden), "elu").double()
    x, pri = 1.5 * torch.randn(N, D, dtype=torch.float64), torch.randn(N, D + 8 + 5, dtype=torch.float64)
    cols = [int(c) for c in torch.randperm(pri.shape[1])[:E]]
    with torch.no_grad():
        out, tg = M.est_forward_torch(net, x, pri, cols)
    ref_out, ref_tg = R.est_forward_ref(*_lin(net), x.numpy(), pri.numpy(), cols)
    assert out.shape == (N, D + E) and tg.shape == (N, E)
    assert torch.equal(out[:, :D], x) and np.array_equal(tg.numpy(), ref_tg)                    # the copies are exact
    assert np.abs(out.numpy() - ref_out).max() <= 1e-12 * max(1.0, np.abs(ref_out).max())       # float64 both: rounding of another order of sums
    with torch.no_grad():
        assert M.est_forward_torch(net, x)[1] is None


def test_one_minibatch_step_against_the_reference():
    """the loss and its gradient as StateEstimator._loss forms them (distill_loss, mse) against est_step_ref"""
    torch.manual_seed(5)
    est = M.StateEstimator(12, 12, 25, 4, 3, targets=ALL, hidden_dims=(16, 9))
    est.net.double()
    x, y = torch.randn(7, 12, dtype=torch.float64), torch.randn(7, 8, dtype=torch.float64)
    loss = est._loss(x, y)
    loss.backward()
    ref_loss, dws, dbs = R.est_step_ref(*_lin(est.net), x.numpy(), y.numpy())
    assert abs(float(loss.detach()) - ref_loss) <= 1e-12 * ref_loss
    mods = [m for m in est.net.model if isinstance(m, torch.nn.Linear)]
    for m, dw, db in zip(mods, dws, dbs):
        assert np.abs(m.weight.grad.numpy() - dw).max() <= 1e-12 and np.abs(m.bias.grad.numpy() - db).max() <= 1e-12


def test_targets_and_columns():
    assert M.parse_targets("lin_vel") == ["lin_vel"] and M.target_columns("lin_vel", 39) == [39, 40, 41]
    assert M.parse_targets("feet_height, lin_vel") == ["lin_vel", "feet_height"]                 # the canonical order, whatever was typed
    assert M.target_columns(ALL, 39) == list(range(39, 47)) and M.target_columns("base_height,feet_contact", 10) == [13, 14, 15]
    for bad, word in (("lin_vel,yaw", "unknown"), ("lin_vel,lin_vel", "twice"), ("", "empty"), (" , ", "empty")):
        with pytest.raises(ValueError, match=word):
            M.parse_targets(bad)
    for bad in ((), (1, 2, 3, 4), (0,), (257,), (128, 300)):
        with pytest.raises(ValueError, match="estimator_hidden_dims"):
            M.check_hidden_dims(bad)
    assert M.check_hidden_dims((256, 1, 7)) == [256, 1, 7]


# ---- flags and refusals --------------------------------------------------------------------------------------------------------------------
class _NoEnv:
    num_envs, num_obs, num_pri_obs, num_actions = 8, 39, 47, 10

    def reset(self):
        return None


def _train_cfg(steps=6):
    tcfg = GR1T1CfgPPO()
    tcfg.runner.num_steps_per_env = steps
    tcfg.algorithm.num_mini_batches, tcfg.algorithm.num_learning_epochs = 3, 2
    tcfg.policy.actor_hidden_dims, tcfg.policy.critic_hidden_dims = [32, 16], [32, 16]
    return tcfg


def _cfg_dict(runner=(), algorithm=(), policy=(), flags=("--estimator",), steps=6):
    d = class_to_dict(update_cfg_from_args(None, _train_cfg(steps), get_args(list(flags)))[1])
    d["runner"].update(runner); d["algorithm"].update(algorithm); d["policy"].update(policy)
    return d


def test_cli_flags_reach_the_runner():
    a = get_args([])
    assert a.estimator is False and a.estimator_targets == "lin_vel" and a.estimator_hidden_dims == [128, 64]
    assert a.estimator_learning_rate == 1e-3 and a.estimator_num_epochs == 1
    d = class_to_dict(update_cfg_from_args(None, config.GR1T1CfgPPO(), get_args(["--estimator_targets", ALL]))[1])
    assert not any(k.startswith("estimator") for k in d["runner"])                               # without --estimator: nothing
    d = class_to_dict(update_cfg_from_args(None, config.GR1T1CfgPPO(), get_args(["--estimator"]))[1])["runner"]
    assert d["estimator"] is True and d["estimator_targets"] == "lin_vel" and d["estimator_hidden_dims"] == [128, 64]
    r = OnPolicyRunner(_NoEnv(), _cfg_dict(), None, "cpu")
    est = r.estimator
    assert isinstance(est, M.StateEstimator) and est.cols == [39, 40, 41] and est.num_inputs == 39 and est.num_outputs == 3
    assert est.learning_rate == 1e-3 and est.num_epochs == 1 and est.config == {"targets": ["lin_vel"], "hidden_dims": [128, 64], "activation": "elu"}
    assert r.alg.actor_critic.actor.model[0].in_features == 42 and r.alg.actor_critic.critic.model[0].in_features == 47
    assert r.alg.storage.observations.shape == (6, 8, 42)
    flags = ["--estimator", "--estimator_targets", "feet_contact,base_height", "--estimator_hidden_dims", "48", "33", "7",
             "--estimator_learning_rate", "3e-4", "--estimator_num_epochs", "2", "--obs_history", "3", "--empirical_normalization"]
    r = OnPolicyRunner(_NoEnv(), _cfg_dict(flags=flags), None, "cpu")
    est = r.estimator
    assert est.cols == [42, 43, 44] and est.num_inputs == 117 and est.learning_rate == 3e-4 and est.num_epochs == 2
    assert [m.out_features for m in est.net.model if hasattr(m, "out_features")] == [48, 33, 7, 3]
    assert r.alg.actor_critic.actor.model[0].in_features == 120 and r.obs_normalizer.dim == 117   # the statistics stay actor_in wide
    for cls in (config.GR1T1CfgPPO, config.GR1T2CfgPPO, config.GR1T1FullBodyCfgPPO):               # not config keys
        assert not any(k.startswith("estimator") for k in vars(cls.runner))
    assert OnPolicyRunner(_NoEnv(), _cfg_dict(flags=()), None, "cpu").estimator is None


def test_refused_combinations(monkeypatch, tmp_path):
    cases = ((dict(runner={"policy_class_name": "ActorCriticRecurrent"}, policy={"rnn_hidden_size": 32}), ValueError, "--recurrent", "memory is the estimator"),
             (dict(runner={"privileged_actor": True}), ValueError, "--privileged_actor", "already reads the targets"),
             (dict(runner={"distill_from": str(tmp_path / "teacher.pt")}), ValueError, "--distill_from", "distillation"),
             (dict(algorithm={"symmetry": "augment"}), ValueError, "--symmetry", "mirror map of the appended columns"),
             (dict(runner={"exact_resume": True}), NotImplementedError, "--exact_resume", "train_state"))
    for keys, exc, both, why in cases:
        with pytest.raises(exc, match=both) as info:
            OnPolicyRunner(_NoEnv(), _cfg_dict(**keys), None, "cpu")
        assert "--estimator" in str(info.value) and why in str(info.value), keys
    for bad, word in (("lin_vel,yaw", "unknown"), ("lin_vel,lin_vel", "twice"), ("", "empty")):
        with pytest.raises(ValueError, match=word):
            OnPolicyRunner(_NoEnv(), _cfg_dict(runner={"estimator_targets": bad}), None, "cpu")
    with pytest.raises(ValueError, match="estimator_hidden_dims"):
        OnPolicyRunner(_NoEnv(), _cfg_dict(runner={"estimator_hidden_dims": [300]}), None, "cpu")

    class NoPri(_NoEnv):
        num_pri_obs = None

    class OtherLayout(_NoEnv):
        num_pri_obs = 48
    with pytest.raises(ValueError, match="no privileged observations"):
        OnPolicyRunner(NoPri(), _cfg_dict(), None, "cpu")
    with pytest.raises(ValueError, match=r"num_pri_obs=48 is not num_obs \+ 8 \+ 0 height points"):
        OnPolicyRunner(OtherLayout(), _cfg_dict(), None, "cpu")
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    monkeypatch.setattr(dist, "get_rank", lambda *a: 0)
    with pytest.raises(NotImplementedError, match="world size") as info:
        OnPolicyRunner(_NoEnv(), _cfg_dict(), None, "cpu")
    assert "--estimator" in str(info.value)


def test_the_real_env_has_the_layout(oracle_backend):  # noqa: F811
    args = _args(("--estimator",))
    env, _ = task_registry.make_env("GR1T1", args=args, env_cfg=GR1T1Cfg())
    M.check_layout(env)                                                                          # 168 = 39 + 8 + 121 height points
    assert env.num_pri_obs == 168 and env.num_obs == 39


# ---- alignment and learnability on fake envs --------------------------------------------------------------------------------------------------
class CounterEnv:
    """every env carries a counter that is in column 0 of its actor frame; the eight target columns of the privileged frame are a known
    function of that counter.  Env n ends every 3 + n steps and restarts its counter at 1000 (n + 1): no counter value occurs twice."""
    num_obs, num_actions, cfg = 6, 2, None

    def __init__(self, num_envs=5):
        self.num_envs, self.num_pri_obs = num_envs, self.num_obs + 8
        self.n = torch.arange(num_envs, dtype=torch.float32)
        self.max_episode_length = 100
        self.reset()

    @staticmethod
    def target(c):
        return torch.stack([(j + 1) * 0.5 * c + 7.0 * j for j in range(8)], dim=1)

    def reset(self):
        self.count, self.age, self.episode = 1000.0 * (self.n + 1), torch.zeros(self.num_envs), torch.ones(self.num_envs)
        self.episode_length_buf = torch.zeros(self.num_envs, dtype=torch.long)

    def get_observations(self):
        return torch.stack([self.count, self.n, self.age, torch.zeros_like(self.n), torch.ones_like(self.n), -self.n], dim=1)

    def get_privileged_observations(self):
        return torch.cat([self.get_observations(), self.target(self.count)], dim=1)

    def step(self, actions):
        self.count, self.age = self.count + 1.0, self.age + 1.0
        dones = self.age >= 3 + self.n
        self.episode = self.episode + dones
        self.count = torch.where(dones, 1000.0 * (self.n + 1) + 100.0 * (self.episode - 1), self.count)   # the frame returned is the reset frame
        self.age = torch.where(dones, torch.zeros_like(self.age), self.age)
        return self.get_observations(), self.get_privileged_observations(), torch.zeros(self.num_envs), dones.long(), {}


def test_every_stored_row_has_the_targets_of_its_own_frame():
    """the alignment rule: after each rollout, row (t, n) of the storage and targets[t, n] belong to one frame -- the rows after a done and
    the first row of the second rollout (which was built before the first update) included"""
    env = CounterEnv()
    d = _cfg_dict(flags=("--estimator", "--estimator_targets", ALL), steps=7)
    d["algorithm"]["num_mini_batches"] = 5
    runner = OnPolicyRunner(env, d, None, "cpu")
    est, seen, after_done = runner.estimator, set(), 0
    for it in range(2):
        runner.learn(num_learning_iterations=1)
        rows, dones = runner.alg.storage.observations, runner.alg.storage.dones.squeeze(-1)
        assert rows.shape == (7, 5, 6 + 8)
        for t in range(7):
            c = rows[t, :, 0]
            assert torch.equal(est.targets[t], CounterEnv.target(c)), (it, t)
            assert not seen & set(c.tolist())                                                    # a counter names one frame
            seen |= set(c.tolist())
            if t > 0:
                after_done += int(dones[t - 1].sum())
                assert bool((c[dones[t - 1] > 0] % 100 == 0).all())                              # the row after a done holds the reset frame
    assert after_done >= 5 and torch.equal(est.carry, CounterEnv.target(env.count))


class LinearEnv:
    """actor frames are noise; the target columns are a fixed linear map of the frame"""
    num_obs, num_actions, cfg = 6, 2, None

    def __init__(self, num_envs=64):
        self.num_envs, self.num_pri_obs, self.max_episode_length = num_envs, self.num_obs + 8, 100
        self.g = torch.Generator().manual_seed(3)
        self.A = torch.randn(self.num_obs, 8, generator=self.g)
        self.episode_length_buf = torch.zeros(num_envs, dtype=torch.long)
        self.reset()

    def reset(self):
        self.obs = torch.randn(self.num_envs, self.num_obs, generator=self.g)

    def get_observations(self):
        return self.obs

    def get_privileged_observations(self):
        return torch.cat([self.obs, self.obs @ self.A], dim=1)

    def step(self, actions):
        self.reset()
        return self.obs, self.get_privileged_observations(), torch.zeros(self.num_envs), torch.zeros(self.num_envs, dtype=torch.long), {}


def _tags(runner):
    out = {}
    for line in open(os.path.join(runner.log_dir, "scalars.jsonl")):
        out.setdefault(line.split('"tag": "')[1].split('"')[0], []).append(float(line.split('"value": ')[1].split(",")[0]))
    return out


def test_a_linear_target_is_learned(tmp_path):
    """20 iterations of 8 x 64 rows, 3 minibatches, 2 epochs, learning rate 1e-2: Loss/estimator falls below half its first value.  Measured
    on the CPU with the torch spelling: first 3.6881, last 0.0158 (a ratio of 0.0043); the bound is half the initial loss"""
    torch.manual_seed(0)
    d = _cfg_dict(flags=("--estimator", "--estimator_targets", ALL, "--estimator_hidden_dims", "32", "--estimator_learning_rate", "1e-2",
                         "--estimator_num_epochs", "2"), steps=8)
    runner = OnPolicyRunner(LinearEnv(), d, str(tmp_path), "cpu")
    before = [p.detach().clone() for p in runner.estimator.net.parameters()]
    runner.learn(num_learning_iterations=20)
    losses = _tags(runner)["Loss/estimator"]
    print(f"Loss/estimator: first {losses[0]:.4f}, last {losses[-1]:.4f}, ratio {losses[-1] / losses[0]:.4f}")
    assert len(losses) == 20 and all(np.isfinite(v) for v in losses) and losses[-1] < 0.5 * losses[0]
    assert all(not torch.equal(a, b) for a, b in zip(before, runner.estimator.net.parameters()))


def test_a_poisoned_row_skips_every_step():
    torch.manual_seed(1)
    est = M.StateEstimator(6, 6, 14, 4, 3, targets="lin_vel", hidden_dims=(8,))
    rows = torch.randn(3, 4, 9)
    assert est.update(rows, 1) > 0.0
    rows[1, 2, 3] = float("nan")
    before = [p.detach().clone() for p in est.net.parameters()]
    assert est.update(rows, 1) == 0.0 and all(torch.equal(a, b) for a, b in zip(before, est.net.parameters()))
    with pytest.raises(ValueError, match="expected rows"):
        est.update(rows[:, :, :8], 1)


# ---- the runner over the oracle-backed env ---------------------------------------------------------------------------------------------------
def _args(extra=()):
    return get_args(["--task", "GR1T1", "--headless", "--num_envs", "8", "--sim_device", "cpu", "--rl_device", "cpu", "--pipeline", "cpu",
                     "--seed", "3", *extra])


def _make(tmp_path, flags=("--estimator",), steps=6):
    args = _args(flags)
    env, _ = task_registry.make_env("GR1T1", args=args, env_cfg=GR1T1Cfg())
    runner, _ = task_registry.make_alg_runner(env, name=None, args=args, train_cfg=_train_cfg(steps), log_root=str(tmp_path) if tmp_path else None)
    return env, runner


def test_checkpoint_resume_and_the_untouched_update(oracle_backend, tmp_path):  # noqa: F811
    env, runner = _make(tmp_path / "est")
    est = runner.estimator
    policy = [p.detach().clone() for p in runner.alg.actor_critic.parameters()]
    runner.learn(num_learning_iterations=2)
    assert any(not torch.equal(a, b) for a, b in zip(policy, runner.alg.actor_critic.parameters()))
    tags = _tags(runner)
    assert len(tags["Loss/estimator"]) == 2 and all(np.isfinite(v) and v > 0 for v in tags["Loss/estimator"])
    rows = runner.alg.storage.observations
    assert rows.shape == (6, 8, 42)
    with torch.no_grad():                                                                        # (the estimate stored is the estimator's as it was during the rollout)
        assert not torch.equal(rows[0, :, 39:], est.net(rows[0, :, :39]))
    _, plain = _make(tmp_path / "plain", flags=())
    plain.learn(num_learning_iterations=1)
    assert plain.estimator is None
    ck_path = os.path.join(runner.log_dir, "model_2.pt")
    ck, ck_plain = torch.load(ck_path, weights_only=False), torch.load(os.path.join(plain.log_dir, "model_1.pt"), weights_only=False)
    assert set(ck_plain) == {"model_state_dict", "optimizer_state_dict", "iter", "infos"}       # without the flag: exactly today's keys
    assert set(ck) == set(ck_plain) | {"estimator"}
    assert set(ck["estimator"]) == {"state_dict", "optimizer_state_dict", "config"}
    assert ck["estimator"]["config"] == {"targets": ["lin_vel"], "hidden_dims": [128, 64], "activation": "elu"}
    assert set(ck["model_state_dict"]) == set(ck_plain["model_state_dict"])                       # the policy is the plain one, E columns wider
    shapes = {k: tuple(v.shape) for k, v in ck["model_state_dict"].items()}
    plain_shapes = {k: tuple(v.shape) for k, v in ck_plain["model_state_dict"].items()}
    assert shapes.pop("actor.model.0.weight") == (32, 42) and plain_shapes.pop("actor.model.0.weight") == (32, 39) and shapes == plain_shapes
    assert not any(t.startswith("Loss/estimator") for t in _tags(plain))

    args = _args(("--estimator", "--resume"))                                                    # --resume: the last run under the log root
    env2, _ = task_registry.make_env("GR1T1", args=args, env_cfg=GR1T1Cfg())
    again, _ = task_registry.make_alg_runner(env2, name=None, args=args, train_cfg=_train_cfg(), log_root=str(tmp_path / "est"))
    sd, sd2 = est.state_dict(), again.estimator.state_dict()
    assert set(sd) == set(sd2) and all(torch.equal(sd[k], sd2[k]) for k in sd) and again.current_learning_iteration == 2
    st, st2 = est.optimizer.state_dict()["state"], again.estimator.optimizer.state_dict()["state"]
    assert len(st) > 0 and all(torch.equal(st[i]["exp_avg"], st2[i]["exp_avg"]) for i in st)
    pa, pb = runner.alg.actor_critic.state_dict(), again.alg.actor_critic.state_dict()
    assert all(torch.equal(pa[k], pb[k]) for k in pa if k.startswith(("actor.", "critic.")))   # (load() resets std, as the reference does)
    again.learn(num_learning_iterations=1)                                                       # ... and it trains on
    _, no_opt = _make(None)
    no_opt.load(ck_path, load_optimizer=False)
    assert len(no_opt.estimator.optimizer.state_dict()["state"]) == 0

    with pytest.raises(ValueError, match=r"pass --estimator --estimator_targets lin_vel --estimator_hidden_dims 128 64"):
        plain.load(ck_path)                                                                      # a checkpoint with the entry, a runner without
    with pytest.raises(ValueError, match="pass no --estimator"):
        no_opt.load(os.path.join(plain.log_dir, "model_1.pt"))                                   # ... and the reverse
    _, other = _make(None, flags=("--estimator", "--estimator_targets", "lin_vel,base_height"))
    with pytest.raises(ValueError, match="estimator_targets lin_vel "):
        other.load(ck_path)
    _, other = _make(None, flags=("--estimator", "--estimator_hidden_dims", "64"))
    with pytest.raises(ValueError, match="estimator_hidden_dims 128 64"):
        other.load(ck_path)


def test_inference_and_export_take_raw_single_frames(oracle_backend, tmp_path):  # noqa: F811
    """history 3 and normalisation: the inference policy and the exported TorchScript module against the training-time pipeline's mean
    action, within tests/test_play_gpu.py's 1e-6 for the exported actor"""
    env, runner = _make(tmp_path, flags=("--estimator", "--estimator_targets", ALL, "--obs_history", "3", "--empirical_normalization"))
    runner.learn(num_learning_iterations=2)
    est, ac = runner.estimator, runner.alg.actor_critic
    assert est.num_inputs == 117 and ac.actor.model[0].in_features == 125 and runner.obs_normalizer.dim == 117
    policy = runner.get_inference_policy(device="cpu")
    path = export_policy_as_jit(ac, str(tmp_path / "exported"), normalizer=runner.obs_normalizer, history=3, estimator=est.net)
    exported = torch.jit.load(path)
    hist = ObsHistory(8, 39, 3)
    g = torch.Generator().manual_seed(4)
    runner.obs_normalizer.eval()
    for i in range(5):
        frame = torch.randn(8, 39, generator=g)
        dones = (torch.rand(8, generator=g) < 0.3).long() if i else None
        if dones is not None:
            policy.reset(dones); exported.reset(dones)
        with torch.no_grad():
            x = runner.obs_normalizer.normalize(hist.push(frame, dones) if i else hist.fill(frame))
            wide, _ = M.est_forward_torch(est.net, x)
            want = ac.act_inference(wide)
            got, got_jit = policy(frame), exported(frame)
        assert want.shape == got.shape == got_jit.shape == (8, env.num_actions)
        assert float((got - want).abs().max()) <= 1e-6 and float((got_jit - want).abs().max()) <= 1e-6, i


@pytest.mark.parametrize("flags", [("--empirical_normalization",), ("--obs_history", "3"), ("--critic_obs_history", "2"), ("--noise_std_type", "log"),
                                   ("--state_dependent_std", "--noise_std_type", "log"), ("--rnd",), ("--smooth", "both")],
                         ids=lambda f: f[0].lstrip("-"))
def test_compositions_train(oracle_backend, tmp_path, flags):  # noqa: F811
    """the rows are just wider: two iterations beside each option, and the widths are right (--precision bf16 has no CPU path, PPO refuses
    it there: tests/test_estimator_gpu.py runs that composition)"""
    env, runner = _make(tmp_path, flags=("--estimator", *flags))
    est, ac = runner.estimator, runner.alg.actor_critic
    before = [p.detach().clone() for p in est.net.parameters()]
    runner.learn(num_learning_iterations=2)
    D = 39 * runner.obs_history_length
    assert est.num_inputs == D and ac.actor.model[0].in_features == D + 3 and runner.alg.storage.observations.shape == (6, 8, D + 3)
    assert ac.critic.model[0].in_features == 168 * runner.critic_obs_history_length
    assert all(not torch.equal(a, b) and bool(torch.isfinite(b).all()) for a, b in zip(before, est.net.parameters()))
    assert all(bool(torch.isfinite(p).all()) for p in ac.parameters())
    assert len(_tags(runner)["Loss/estimator"]) == 2


def test_default_path_constructs_nothing(oracle_backend, tmp_path, monkeypatch):  # noqa: F811
    def boom(self, *a, **k):
        raise AssertionError("StateEstimator constructed without --estimator")
    monkeypatch.setattr(M.StateEstimator, "__init__", boom)
    _, runner = _make(tmp_path, flags=())
    runner.learn(num_learning_iterations=1)
    assert runner.estimator is None and runner.alg.actor_critic.actor.model[0].in_features == 39


# ---- the C entry -----------------------------------------------------------------------------------------------------------------------------
def test_entry_is_exported_and_refuses_bad_calls_without_a_gpu():
    """every call here is refused before anything is launched: no device is needed"""
    from wiki_grx_gym_amd.rl.fused_loss import load_ppo_library
    lib = load_ppo_library()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "grx_ppo_est.h")).read()
    assert "int grx_est_forward(" in hdr and hasattr(lib, "grx_est_forward")
    buf = (C.c_float * 4096)()
    base = C.addressof(buf)
    X, OUT, PRI, TG, W = base, base + 4096, base + 8192, base + 12288, base + 2048

    def net(n_layers=3, widths=(16, 9, 3, 0), w=(W, W, W, 0)):
        s = M._Net()
        s.n_layers = n_layers
        for i in range(4):
            s.widths[i], s.W[i], s.bias[i] = widths[i], w[i] or None, None
        return s

    def call(s=None, N=4, D=8, x=X, P=20, pri=PRI, cols=(8, 9, 10), out=OUT, tg=TG, null_net=False):
        s = s if s is not None else net()
        carr = (C.c_int * len(cols))(*cols) if cols is not None else None
        return lib.grx_est_forward(None if null_net else C.addressof(s), N, D, x, P, pri, carr, out, tg, None)
    assert call(null_net=True) < 0 and call(x=None) < 0 and call(out=None) < 0
    assert call(N=0) < 0 and call(N=-1) < 0 and call(D=0) < 0 and call(D=2049) < 0
    assert call(s=net(n_layers=1)) < 0 and call(s=net(n_layers=5)) < 0
    assert call(s=net(widths=(16, 9, 0, 0))) < 0 and call(s=net(widths=(16, 9, 9, 0))) < 0          # E < 1, E > 8
    assert call(s=net(widths=(257, 9, 3, 0))) < 0 and call(s=net(widths=(16, 0, 3, 0))) < 0         # a hidden width outside 1..256
    assert call(s=net(w=(W, 0, W, 0))) < 0                                                         # a NULL weight
    assert call(P=0) < 0 and call(cols=None) < 0 and call(cols=(8, 9, 20)) < 0 and call(cols=(-1, 9, 10)) < 0
    assert call(out=X) < 0 and call(out=X + 4 * 31) < 0 and call(x=OUT + 4 * 43, out=OUT) < 0       # out overlapping x
    assert call(N=1 << 27, D=16) < 0                                                               # N * (D + E) >= 2^31
    assert all(v == 0.0 for v in buf)
