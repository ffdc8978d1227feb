"""The recurrent actor-critic without a GPU (rl/recurrent.py): the torch spellings of the LSTM cell and its backward
against torch.nn.LSTMCell / nn.LSTM in float64 (tests/lstm_ref.py), the masked recurrence against the cut-trajectory reference, the
state-dict keys, the bootstrap evaluation, the env-range generator, the runner over the oracle-backed env of tests/test_env_plumbing.py
(training, checkpoints, the exported module, the refusals), the flags, and the C entries' argument checks."""
import os

import numpy as np
import pytest
import torch
from torch import nn

from tests import lstm_ref as R
from tests.test_env_plumbing import oracle_backend  # noqa: F401  (the fixture)
from wiki_grx_gym_amd.envs import GR1T1Cfg, GR1T1CfgPPO, config
from wiki_grx_gym_amd.envs.config import class_to_dict
from wiki_grx_gym_amd.rl import recurrent as L
from wiki_grx_gym_amd.rl.modules import ActorCriticMLP
from wiki_grx_gym_amd.rl.ppo import PPO
from wiki_grx_gym_amd.rl.runner import OnPolicyRunner
from wiki_grx_gym_amd.utils import export_policy_as_jit, get_args, task_registry
from wiki_grx_gym_amd.utils.helpers import update_cfg_from_args

KEYS = ["memory_a.rnn.weight_ih_l0", "memory_a.rnn.weight_hh_l0", "memory_a.rnn.bias_ih_l0", "memory_a.rnn.bias_hh_l0",
        "memory_c.rnn.weight_ih_l0", "memory_c.rnn.weight_hh_l0", "memory_c.rnn.bias_ih_l0", "memory_c.rnn.bias_hh_l0"]
T, N, D, H = 6, 5, 7, 32


def _policy(actor_in=D, critic_in=9, actions=3, **kw):
    return L.ActorCriticRecurrent(actor_in, critic_in, actions, rnn_hidden_size=H, actor_hidden_dims=[16, 8], critic_hidden_dims=[16, 8], **kw)


def _sequence_inputs(dtype, n=N, d=D, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, n, d, generator=g, dtype=torch.float64)
    h0 = torch.tanh(torch.randn(n, H, generator=g, dtype=torch.float64))
    c0 = torch.randn(n, H, generator=g, dtype=torch.float64)
    w = torch.randn(T, n, H, generator=g, dtype=torch.float64)       # the weights of the scalar whose gradient is taken
    return x.to(dtype), h0.to(dtype), c0.to(dtype), w.to(dtype)


# ---- the two operations against float64 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_reset", [False, True], ids=["plain", "reset"])
def test_cell_torch_against_lstmcell_float64(with_reset):
    """the torch spelling evaluated in float64 is nn.LSTMCell's float64 result to rounding (1e-12: ~40 terms of order one at 2^-53)"""
    torch.manual_seed(1)
    rnn = nn.LSTM(D, H, 1)
    p = R.params64(rnn)
    x, h, c, reset = R.cell_inputs(33, D, H)
    reset = reset if with_reset else None
    want_h, want_c = R.cell64(p, x, h, c, reset)
    got_h, got_c, acts = L.lstm_cell_torch(torch.tensor(x).double(), torch.tensor(h).double(), torch.tensor(c).double(),
                                           torch.tensor(reset) if with_reset else None, *[p[k] for k in R.NAMES])
    assert (got_h - want_h).abs().max() < 1e-12 and (got_c - want_c).abs().max() < 1e-12
    assert acts.shape == (33, 5 * H) and torch.equal(acts[:, 4 * H:], torch.tanh(got_c)) and torch.equal(got_h, acts[:, 3 * H:4 * H] * acts[:, 4 * H:])
    if with_reset:   # a reset row does not see its previous state at all
        h2, c2 = h.copy(), c.copy()
        h2[reset != 0] = 7.0
        c2[reset != 0] = np.nan
        again = L.lstm_cell_torch(torch.tensor(x).double(), torch.tensor(h2).double(), torch.tensor(c2).double(), torch.tensor(reset),
                                  *[p[k] for k in R.NAMES])
        assert torch.equal(again[0], got_h) and torch.equal(again[1], got_c)


def test_masked_recurrence_against_cut_trajectories():
    d = R.dones(N)
    assert d[0, 0] and d[T - 1, 1] and d[2, 2] and d[3, 2] and not d[:, 3].any() and d[:, 4].all()      # the five kinds of env
    torch.manual_seed(2)
    mem = L.Memory(D, H).double()
    x, h0, c0, _ = _sequence_inputs(torch.float64)
    want = R.sequence64(R.lstm64(R.params64(mem.rnn)), x, d, h0, c0)
    with torch.no_grad():
        got = mem.sequence(x, torch.tensor(R.resets_of(d)), h0, c0)
    assert got.shape == (T, N, H) and (got - want).abs().max() < 1e-12
    # ... and step mode, the rollout's spelling of the same thing: reset(dones) after every step, applied by the next
    step = L.Memory(D, H, rnn=mem.rnn)
    step._ensure_state(N, "cpu")
    step._state = (torch.stack([h0, h0]), torch.stack([c0, c0]))
    for t in range(T):
        assert (step.step(x[t]) - want[t]).abs().max() < 1e-12, t
        step.reset(torch.tensor(d[t]).bool())


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-10), (torch.float32, 1e-4)], ids=["float64", "float32"])
def test_sequence_gradients_against_float64_autograd(dtype, tol):
    """LSTMSequence's hand-written backward -- the element-wise half, the recurrent product per step, the stacked products -- against
    float64 autograd through nn.LSTM over the cut trajectories: all eight LSTM tensors of a policy and both inputs, each within
    tol * max|reference gradient| (1e-4 in float32: tests/test_ppo_gpu.py's bound for parameter gradients)"""
    d = R.dones(N)
    torch.manual_seed(3)
    ac = _policy().to(dtype)
    for mem, width, seed in ((ac.memory_a, D, 0), (ac.memory_c, 9, 1)):
        x, h0, c0, w = _sequence_inputs(dtype, d=width, seed=seed)
        x.requires_grad_(True)
        out = mem.sequence(x, torch.tensor(R.resets_of(d)), h0, c0)
        (out * w).sum().backward()
        ref = R.lstm64(R.params64(mem.rnn), requires_grad=True)
        x64 = x.detach().double().requires_grad_(True)
        (R.sequence64(ref, x64, d, h0.double(), c0.double()) * w.double()).sum().backward()
        for k in R.NAMES:
            got, want = getattr(mem.rnn, k).grad.double(), getattr(ref, k).grad
            assert (got - want).abs().max() <= tol * want.abs().max(), (k, float((got - want).abs().max()), float(want.abs().max()))
        assert (x.grad.double() - x64.grad).abs().max() <= tol * x64.grad.abs().max()
    assert sum(p.grad is not None for n, p in ac.named_parameters() if n.startswith("memory_")) == 8


def test_backward_torch_against_autograd_of_the_elementwise_map():
    g = torch.Generator().manual_seed(4)
    M = 33
    G = torch.randn(M, 4 * H, generator=g, dtype=torch.float64, requires_grad=True)
    c_prev = torch.randn(M, H, generator=g, dtype=torch.float64, requires_grad=True)
    dh, dc_in = torch.randn(M, H, generator=g, dtype=torch.float64), torch.randn(M, H, generator=g, dtype=torch.float64)
    reset = torch.tensor((np.arange(M) % 3 == 0).astype(np.uint8))
    keep = (reset == 0).double().view(-1, 1)
    gi, gf, gg, go = G.chunk(4, 1)
    i, f, gt, o = torch.sigmoid(gi), torch.sigmoid(gf), torch.tanh(gg), torch.sigmoid(go)
    c = f * (c_prev * keep) + i * gt
    h = o * torch.tanh(c)
    ((h * dh).sum() + (c * dc_in).sum()).backward()
    acts = torch.cat([i, f, gt, o, torch.tanh(c)], 1).detach()
    dG, dc_prev = L.lstm_cell_backward_torch(dh, dc_in, acts, c_prev.detach(), reset)
    assert (dG - G.grad).abs().max() < 1e-12 and (dc_prev - c_prev.grad).abs().max() < 1e-12
    assert not dc_prev[reset != 0].any()


# ---- the module ----------------------------------------------------------------------------------------------------------------------------
def test_state_dict_keys_are_rsl_rls():
    ac = _policy()
    assert ac.is_recurrent is True and ActorCriticMLP.is_recurrent is False
    keys = list(ac.state_dict())
    assert [k for k in keys if k.startswith("memory_")] == KEYS
    assert sorted(k for k in keys if not k.startswith("memory_")) == sorted(
        ["std"] + [f"{net}.model.{i}.{p}" for net in ("actor", "critic") for i in (0, 2, 4) for p in ("weight", "bias")])
    assert ac.actor.model[0].in_features == H and ac.critic.model[0].in_features == H           # the MLPs read h
    assert ac.num_actor_input == D and ac.num_critic_input == 9                                  # the storage keeps observations
    bare = nn.LSTM(D, H, 1)
    bare.load_state_dict({k[len("memory_a.rnn."):]: v for k, v in ac.state_dict().items() if k.startswith("memory_a.rnn.")})
    x = torch.randn(4, D)
    with torch.no_grad():
        want = bare(x.unsqueeze(0))[0].squeeze(0)
        assert (ac.memory_a.step(x) - want).abs().max() < 1e-6
    assert ac.get_hidden_states()[0][0].shape == (4, H) and ac.get_hidden_states()[1] is None


@pytest.mark.parametrize("kw", [dict(rnn_type="gru"), dict(rnn_num_layers=2), dict(rnn_hidden_size=48), dict(rnn_hidden_size=0),
                                dict(rnn_hidden_size=1056), dict(rnn_hidden_size=64.0)], ids=str)
def test_constructor_refusals(kw):
    with pytest.raises(ValueError, match="rnn_"):
        L.ActorCriticRecurrent(D, 9, 3, **{"rnn_hidden_size": 32, **kw})


def test_bootstrap_leaves_the_critics_memory_alone():
    torch.manual_seed(5)
    ac, twin = _policy(), _policy()
    twin.load_state_dict(ac.state_dict())
    xs = torch.randn(4, N, 9)
    done = torch.tensor([True, False, False, True, False])
    with torch.no_grad():
        for m in (ac, twin):
            m.evaluate(xs[0]); m.evaluate(xs[1])
            m.reset(done)
        before = [t.clone() for t in ac.memory_c.hidden_states()]
        boot = ac.evaluate_bootstrap(xs[2])
        after = ac.memory_c.hidden_states()
        assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
        assert torch.equal(boot, twin.evaluate(xs[2]))                       # ... it is the value the next step computes (the reset applied)
        assert torch.equal(ac.evaluate(xs[2]), boot)                         # ... and the pending reset is still pending
        assert torch.equal(ac.evaluate(xs[3]), twin.evaluate(xs[3]))


def test_env_range_generator():
    st = L.RecurrentRolloutStorage(11, 4, [3], [5], [2], H, "cpu")
    assert st.env_ranges(3) == [(0, 3), (3, 6), (6, 9)] and st.env_ranges(11)[-1] == (10, 11)      # in order, the tail dropped
    with pytest.raises(ValueError, match="num_mini_batches"):
        st.env_ranges(12)
    g = torch.Generator().manual_seed(6)
    for name in ("observations", "pri_observations", "actions", "values", "advantages", "returns", "actions_log_prob", "mu", "sigma"):
        getattr(st, name).copy_(torch.randn(getattr(st, name).shape, generator=g))
    st.dones[1, 4, 0] = 1
    st.dones[3, 0, 0] = 1
    st.set_start_states((torch.full((11, H), 1.0), torch.full((11, H), 2.0)), (torch.full((11, H), 3.0), torch.full((11, H), 4.0)))
    st.h0_a[7] = 9.0
    batches = list(st.recurrent_mini_batch_generator(3, num_epochs=2))
    assert len(batches) == 6
    for k, b in enumerate(batches):
        a, e = st.env_ranges(3)[k % 3]                                        # every epoch walks the same ranges in the same order
        obs, cobs, resets, start, actions, values, adv, ret, logp, mu, sigma = b
        assert torch.equal(obs, st.observations[:, a:e]) and torch.equal(cobs, st.pri_observations[:, a:e]) and obs.is_contiguous()
        assert resets.dtype == torch.uint8 and not resets[0].any() and torch.equal(resets[1:], st.dones[:-1, a:e, 0])
        assert [float(s[0, 0]) for s in start] == [1.0, 2.0, 3.0, 4.0] and torch.equal(start[0], st.h0_a[a:e])
        assert torch.equal(actions, st.actions[:, a:e].reshape(-1, 2)) and torch.equal(values.view(4, e - a), st.values[:, a:e, 0])
        assert torch.equal(mu.view(4, e - a, 2)[2, 1], st.mu[2, a + 1])       # step-major: row t * n + j is (step t, env a + j)
    assert int(batches[1][2][2, 1]) == 1 and int(batches[1][2].sum()) == 1    # env 4's done at t = 1 resets step 2; env 0's at T - 1 nothing


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


def _make(tmp_path, flags=("--recurrent", "--rnn_hidden_size", "32"), env_cfg=None, steps=6):
    args = _args(flags)
    env, _ = task_registry.make_env("GR1T1", args=args, env_cfg=env_cfg if env_cfg is not None else GR1T1Cfg())
    runner, _ = task_registry.make_alg_runner(env, name=None, args=args, train_cfg=_train_cfg(steps), log_root=str(tmp_path) if tmp_path else None)
    return env, runner


def test_runner_trains_saves_loads_and_exports(oracle_backend, tmp_path):  # noqa: F811
    cfg = GR1T1Cfg()
    cfg.env.episode_length_s = 0.1           # 5 steps: every env times out inside each rollout
    env, runner = _make(tmp_path, env_cfg=cfg)
    ac = runner.alg.actor_critic
    assert type(ac) is L.ActorCriticRecurrent and runner.recurrent and ac.rnn_hidden_size == 32
    assert isinstance(runner.alg.storage, L.RecurrentRolloutStorage) and runner.alg.storage.h0_a.shape == (16, 32)
    before = {k: v.clone() for k, v in ac.state_dict().items()}
    snaps, update = [], runner.alg.update

    def snap_then_update():
        snaps.append(runner.alg.storage.dones.clone())
        return update()
    runner.alg.update = snap_then_update
    runner.learn(num_learning_iterations=2, init_at_random_ep_len=False)
    assert len(snaps) == 2 and all(int(s.sum()) >= 16 for s in snaps)                       # resets did occur inside the rollouts
    after = ac.state_dict()
    assert all(torch.isfinite(v).all() for v in after.values())
    assert all(not torch.equal(before[k], after[k]) for k in KEYS + ["actor.model.0.weight", "critic.model.4.weight"])
    ck_path = os.path.join(runner.log_dir, "model_2.pt")
    ck = torch.load(ck_path, weights_only=False)
    assert ck["recurrent"] == {"hidden_size": 32} and set(ck) == {"model_state_dict", "optimizer_state_dict", "iter", "infos", "recurrent"}
    assert [k for k in ck["model_state_dict"] if k.startswith("memory_")] == KEYS
    _, again = _make(None)
    again.load(ck_path)
    assert all(torch.equal(v, again.alg.actor_critic.state_dict()[k]) for k, v in after.items() if k != "std")
    assert again.current_learning_iteration == 2
    _, other = _make(None, flags=("--recurrent", "--rnn_hidden_size", "64"))
    with pytest.raises(ValueError, match="--rnn_hidden_size"):
        other.load(ck_path)
    _, plain = _make(None, flags=())
    assert type(plain.alg.actor_critic) is ActorCriticMLP and not plain.recurrent
    with pytest.raises(ValueError, match="--recurrent"):
        plain.load(ck_path)
    plain.save(str(tmp_path / "plain.pt"))
    assert "recurrent" not in torch.load(tmp_path / "plain.pt", weights_only=False)
    with pytest.raises(ValueError, match="--recurrent"):
        again.load(str(tmp_path / "plain.pt"))

    # the exported module, fed env by env the frames the inference policy saw, reset_memory() where an episode ended
    policy = runner.get_inference_policy(device="cpu")
    assert isinstance(policy, L.RecurrentPolicy) and policy.memory.rnn is ac.memory_a.rnn and policy.memory is not ac.memory_a
    jit = torch.jit.load(export_policy_as_jit(ac, str(tmp_path / "exported")))
    frames, ended, acted = [], [], []
    obs = env.get_observations()
    training_state = [t.clone() for t in ac.memory_a.hidden_states()]
    with torch.no_grad():
        for _ in range(8):
            frames.append(obs.clone())
            acted.append(policy(obs).clone())
            obs, _, _, dones, _ = env.step(acted[-1])
            policy.reset(dones)
            ended.append(dones.clone())
        assert any(bool(d.any()) for d in ended[:-1])
        assert all(torch.equal(a, b) for a, b in zip(training_state, ac.memory_a.hidden_states()))   # the training memory was not touched
        for e in (0, 7, 15):
            jit.reset_memory()
            for t in range(8):
                got = jit(frames[t][e:e + 1])
                assert (got - acted[t][e:e + 1]).abs().max() < 1e-6, (e, t)
                if ended[t][e]:
                    jit.reset_memory()
        jit.reset_memory()                                                                     # ... and all envs at once, through reset(dones)
        for t in range(8):
            assert (jit(frames[t]) - acted[t]).abs().max() < 1e-6, t
            jit.reset(ended[t])


def test_normalisation_composes(oracle_backend, tmp_path):  # noqa: F811
    env, runner = _make(tmp_path, flags=("--recurrent", "--rnn_hidden_size", "32", "--empirical_normalization"))
    runner.learn(num_learning_iterations=1)
    assert int(runner.obs_normalizer.count) == 16 * 6 and runner.obs_normalizer.dim == 39 and runner.critic_obs_normalizer.dim == 168
    policy = runner.get_inference_policy(device="cpu")
    jit = torch.jit.load(export_policy_as_jit(runner.alg.actor_critic, str(tmp_path / "exported"), normalizer=runner.obs_normalizer))
    obs = env.get_observations()
    with torch.no_grad():
        for _ in range(3):
            a = policy(obs)
            assert (jit(obs) - a).abs().max() < 1e-6
            obs = env.step(a)[0]
    assert int(runner.obs_normalizer.count) == 16 * 6                                             # eval mode: inference left the statistics alone


class _NoEnv:
    num_envs, num_obs, num_pri_obs, num_actions = 8, 39, 168, 10

    def reset(self):
        return None


def _cfg_dict(runner=(), algorithm=(), policy=()):
    d = class_to_dict(update_cfg_from_args(None, _train_cfg(), get_args(["--recurrent", "--rnn_hidden_size", "32"]))[1])
    d["runner"].update(runner); d["algorithm"].update(algorithm); d["policy"].update(policy)
    return d


def test_refused_combinations(monkeypatch, tmp_path):
    OnPolicyRunner(_NoEnv(), _cfg_dict(), None, "cpu")                                             # the flag alone is fine
    OnPolicyRunner(_NoEnv(), _cfg_dict(runner={"empirical_normalization": True}), None, "cpu")    # ... and with normalisation
    for keys, exc, both in ((dict(runner={"obs_history_length": 3}), ValueError, "--obs_history"),
                            (dict(runner={"critic_obs_history_length": 2}), ValueError, "--critic_obs_history"),
                            (dict(runner={"privileged_actor": True}), ValueError, "--privileged_actor"),
                            (dict(runner={"distill_from": str(tmp_path / "teacher.pt")}), NotImplementedError, "--distill_from"),
                            (dict(algorithm={"precision": "bf16"}), ValueError, "bf16"),
                            (dict(runner={"exact_resume": True}), NotImplementedError, "--exact_resume")):
        with pytest.raises(exc, match=both) as info:
            OnPolicyRunner(_NoEnv(), _cfg_dict(**keys), None, "cpu")
        assert "--recurrent" in str(info.value), keys                                             # the message names both options
    for bad in (dict(rnn_type="gru"), dict(rnn_num_layers=2), dict(rnn_hidden_size=40)):
        with pytest.raises(ValueError, match="rnn_"):
            OnPolicyRunner(_NoEnv(), _cfg_dict(policy=bad), None, "cpu")
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    monkeypatch.setattr(dist, "get_rank", lambda *a: 0)
    with pytest.raises(NotImplementedError, match="world size") as info:
        OnPolicyRunner(_NoEnv(), _cfg_dict(), None, "cpu")
    assert "--recurrent" in str(info.value)
    with pytest.raises(NotImplementedError, match="one process"):
        PPO(actor_critic=_policy(), device="cpu")


def test_non_finite_loss_skips_the_step(oracle_backend):  # noqa: F811
    _, runner = _make(None)
    alg = runner.alg
    with torch.inference_mode():
        obs, pri = runner.env.get_observations(), runner.env.get_privileged_observations()
        for _ in range(6):
            obs, pri, rew, dones, infos = runner.env.step(alg.act(obs, pri))
            alg.process_env_step(rew, dones, infos)
        alg.compute_returns(pri)
    before = {k: v.clone() for k, v in alg.actor_critic.state_dict().items()}
    alg.storage.returns[:, :, 0] = float("nan")                       # every minibatch has a NaN value loss
    assert alg.update() == (0.0, 0.0)
    assert all(torch.equal(v, alg.actor_critic.state_dict()[k]) for k, v in before.items())


# ---- flags and configs -------------------------------------------------------------------------------------------------------------------
def test_cli_flags_reach_the_configs():
    a = get_args([])
    assert a.recurrent is False and a.rnn_hidden_size == 256
    d = class_to_dict(update_cfg_from_args(None, config.GR1T1CfgPPO(), a)[1])
    assert d["runner"]["policy_class_name"] == "ActorCriticMLP" and "rnn_hidden_size" not in d["policy"]
    d = class_to_dict(update_cfg_from_args(None, config.GR1T1CfgPPO(), get_args(["--rnn_hidden_size", "64"]))[1])
    assert d["runner"]["policy_class_name"] == "ActorCriticMLP" and "rnn_hidden_size" not in d["policy"]      # without --recurrent: nothing
    d = class_to_dict(update_cfg_from_args(None, config.GR1T1CfgPPO(), get_args(["--recurrent"]))[1])
    assert d["runner"]["policy_class_name"] == "ActorCriticRecurrent" and d["policy"]["rnn_hidden_size"] == 256
    d = class_to_dict(update_cfg_from_args(None, config.GR1T1CfgPPO(), get_args(["--recurrent", "--rnn_hidden_size", "64"]))[1])
    assert d["policy"]["rnn_hidden_size"] == 64
    for cls in (config.GR1T1CfgPPO, config.GR1T2CfgPPO, config.GR1T1FullBodyCfgPPO):                         # not config keys
        assert not hasattr(cls.policy, "rnn_hidden_size") and cls.runner.policy_class_name != "ActorCriticRecurrent"


# ---- the C entries -------------------------------------------------------------------------------------------------------------------------
def test_c_entries_check_their_arguments():
    """invalid sizes, NULL pointers, aliasing: negative, nothing launched (no GPU needed; the pointers are never followed)"""
    lib = L._lib()
    x, hp, cp, rs, wi, wh, bi, bh, h, c, acts = (0x10000000 * k for k in range(1, 12))
    cell = lambda M=8, Dm=5, Hh=32, **kw: lib.grx_lstm_cell(M, Dm, Hh, *[kw.get(n, v) for n, v in (
        ("x", x), ("hp", hp), ("cp", cp), ("rs", rs), ("wi", wi), ("wh", wh), ("bi", bi), ("bh", bh), ("h", h), ("c", c), ("acts", acts))], None)
    assert cell(M=0) < 0 and cell(Dm=0) < 0 and cell(Hh=0) < 0 and cell(Hh=48) < 0 and cell(Hh=1056) < 0 and cell(Hh=-32) < 0
    assert cell(M=2 ** 22, Hh=1024) < 0
    for name in ("x", "hp", "cp", "wi", "wh", "bi", "bh", "h", "c"):
        assert cell(**{name: None}) < 0, name
    assert cell(h=hp) < 0 and cell(c=cp) < 0 and cell(h=hp + 8 * 32 * 4 - 4) < 0 and cell(c=cp - 4) < 0                # aliasing, overlap
    pre = lib.grx_lstm_cell_preact
    assert pre(0, 5, 32, x, hp, rs, wi, wh, bi, bh, h, None) < 0 and pre(8, 5, 40, x, hp, rs, wi, wh, bi, bh, h, None) < 0
    assert pre(8, 5, 32, x, hp, rs, wi, wh, bi, bh, None, None) < 0 and pre(8, 5, 32, None, hp, rs, wi, wh, bi, bh, h, None) < 0
    bwd = lambda M=8, Hh=32, **kw: lib.grx_lstm_cell_backward(M, Hh, *[kw.get(n, v) for n, v in (
        ("dh", x), ("dc", hp), ("acts", acts), ("cp", cp), ("rs", rs), ("dG", h), ("dcp", c))], None)
    assert bwd(M=0) < 0 and bwd(Hh=0) < 0 and bwd(Hh=33) < 0 and bwd(Hh=2048) < 0
    for name in ("dh", "acts", "cp", "dG", "dcp"):
        assert bwd(**{name: None}) < 0, name
