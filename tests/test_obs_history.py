"""Observation history without a GPU (rl/history.py): the torch spelling against the numpy reference of
tests/obs_history_ref.py, the two alternating buffers, the runner's wiring over a stub env with scripted dones (what the storage
keeps), a second learn() call, the order with normalisation, checkpoints, the CLI flags, HistoryPolicy eager / scripted / exported,
and the C entry's argument checks.  Every comparison of stacked rows is exact: the operation only copies."""
import copy

import numpy as np
import pytest
import torch

from tests import obs_history_ref as R
from tests import obs_norm_ref as NR
from tests.test_obs_norm import StubEnv
from wiki_grx_gym_amd.envs import config
from wiki_grx_gym_amd.envs.config import class_to_dict
from wiki_grx_gym_amd.rl.history import HistoryPolicy, ObsHistory
from wiki_grx_gym_amd.rl.runner import OnPolicyRunner
from wiki_grx_gym_amd.utils.helpers import export_policy_as_jit, get_args, update_cfg_from_args

CFGS = [config.GR1T1CfgPPO, config.GR1T2CfgPPO, config.GR1T1FullBodyCfgPPO]
REFERENCE_KEYS = {"model_state_dict", "optimizer_state_dict", "iter", "infos"}
STEPS = 8


# ---- the definition ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", R.PATTERNS)
@pytest.mark.parametrize("N,D,H", [(1, 1, 2), (3, 5, 1), (8, 39, 3), (8, 168, 6)])
def test_torch_path_against_reference(N, D, H, pattern):
    h = ObsHistory(N, D, H, "cpu")
    assert not h.primed and h.current.shape == (N, H * D) and h.current.dtype == torch.float32
    x, want = R.frames(N, D, STEPS + 1), R.reference(N, D, H, pattern, STEPS)
    got = h.fill(torch.tensor(x[0]))
    assert h.primed and got is h.current and np.array_equal(got.numpy(), want[0])       # the first step's fill
    for t in range(STEPS):
        got = h.push(torch.tensor(x[t + 1]), torch.tensor(R.dones(pattern, N, t)))
        assert got is h.current and np.array_equal(got.numpy(), want[t + 1]), (pattern, t)


def test_the_reference_is_the_definition():
    """(the reference itself, on a case small enough to write down: N = 1, D = 2, H = 3)"""
    ref = R.RefHistory(1, 2, 3)
    assert ref.push([[1, 2]], [False]).tolist() == [[1, 2, 1, 2, 1, 2]]                 # not primed: a fill, whatever dones says
    assert ref.push([[3, 4]], [False]).tolist() == [[1, 2, 1, 2, 3, 4]]                 # oldest first, newest last
    assert ref.push([[5, 6]], [False]).tolist() == [[1, 2, 3, 4, 5, 6]]
    assert ref.push([[7, 8]], [True]).tolist() == [[7, 8, 7, 8, 7, 8]]                  # done: the new episode's first frame, H times
    assert ref.push([[9, 0]], [False]).tolist() == [[7, 8, 7, 8, 9, 0]]


def test_a_push_before_any_fill_fills():
    h = ObsHistory(3, 5, 4, "cpu")
    x = torch.tensor(R.frames(3, 5, 2)[0])
    assert torch.equal(h.push(x, torch.zeros(3, dtype=torch.bool)), x.repeat(1, 4)) and h.primed


@pytest.mark.parametrize("dtype", [torch.bool, torch.uint8, torch.int64, torch.float32])
def test_dones_of_any_dtype(dtype):
    N, D, H = 8, 39, 3
    x, want = R.frames(N, D, 3), R.reference(N, D, H, "every_other", 2)
    h = ObsHistory(N, D, H, "cpu")
    h.fill(torch.tensor(x[0]))
    for t in range(2):
        got = h.push(torch.tensor(x[t + 1]), torch.tensor(R.dones("every_other", N, t)).to(dtype))
    assert np.array_equal(got.numpy(), want[2])


def test_wrong_shapes_raise():
    h = ObsHistory(8, 39, 3, "cpu")
    with pytest.raises(ValueError):
        h.fill(torch.zeros(8, 40))
    with pytest.raises(ValueError):
        h.fill(torch.zeros(7, 39))
    h.fill(torch.zeros(8, 39))
    with pytest.raises(ValueError):
        h.push(torch.zeros(8, 39), torch.zeros(7, dtype=torch.bool))
    with pytest.raises(ValueError):
        ObsHistory(8, 39, 0, "cpu")


# ---- the buffers -------------------------------------------------------------------------------------------------------------------
def test_pushes_alternate_between_two_buffers():
    N, D, H = 8, 39, 3
    h = ObsHistory(N, D, H, "cpu")
    x = [torch.tensor(f) for f in R.frames(N, D, 4)]
    d = torch.zeros(N, dtype=torch.bool)
    h.fill(x[0])
    y0 = h.push(x[1], d); keep = y0.clone()
    y1 = h.push(x[2], d)
    assert y1.data_ptr() != y0.data_ptr() and torch.equal(y0, keep)      # push t's rows survive push t+1
    assert h.push(x[3], d).data_ptr() == y0.data_ptr()                   # ... and push t+2 reuses their storage


def test_state_dict_round_trip():
    N, D, H = 8, 39, 3
    a, b = ObsHistory(N, D, H, "cpu"), ObsHistory(N, D, H, "cpu")
    x = [torch.tensor(f) for f in R.frames(N, D, 4)]
    d = torch.tensor(R.dones("single", N, 0))
    a.fill(x[0]); a.push(x[1], d)
    state = a.state_dict()
    assert set(state) == {"rows", "primed"} and state["primed"] is True and state["rows"].data_ptr() != a.current.data_ptr()
    b.load_state_dict(state)
    assert b.primed and torch.equal(b.current, a.current)
    assert torch.equal(a.push(x[2], d), b.push(x[2], d))
    with pytest.raises(ValueError):
        ObsHistory(N, D, H + 1, "cpu").load_state_dict(state)


# ---- the runner ----------------------------------------------------------------------------------------------------------------------
DONE_STEPS = {2: (1, 5), 4: (0,), 5: (3,), 7: (0, 1, 2, 3, 4, 5, 6, 7)}   # env.step number -> the envs that end there (4: the iteration boundary)


class DoneStubEnv(StubEnv):
    """tests/test_obs_norm.py's stub (ONE output buffer per tensor, overwritten by every step) with scripted dones"""

    def step(self, actions):
        obs, pri, rew, done, infos = super().step(actions)
        done[list(DONE_STEPS.get(self.t, ()))] = True
        return obs, pri, rew, done, infos


def _env_on(env, device):
    if device != "cpu":
        for k in ("obs_buf", "pri_buf", "episode_length_buf"):
            if getattr(env, k) is not None:
                setattr(env, k, getattr(env, k).to(device))
        step0 = env.step

        def step(actions):
            o, p, r, d, i = step0(actions.cpu())
            return o, p, r.to(device), d.to(device), i
        env.obs_table = env.obs_table.to(device)
        env.pri_table = env.pri_table.to(device) if env.pri_table is not None else None
        env.step = step
    return env


def _runner(env=None, H=3, Hc=2, norm=False, steps=4, device="cpu"):
    cfg = config.GR1T1CfgPPO()
    if H != 1:
        cfg.runner.obs_history_length = H
    if Hc != 1:
        cfg.runner.critic_obs_history_length = Hc
    if norm:
        cfg.runner.empirical_normalization = True
    d = class_to_dict(cfg)
    d["policy"].update(actor_hidden_dims=[32, 16], critic_hidden_dims=[32, 16])
    d["runner"]["num_steps_per_env"] = steps
    d["algorithm"].update(num_learning_epochs=1, num_mini_batches=2)
    return OnPolicyRunner(env if env is not None else DoneStubEnv(), d, None, device=device)


def _snapshots(r):
    """(observations, privileged observations) of the storage as every update() finds them"""
    snaps, update = [], r.alg.update

    def snap_then_update():
        snaps.append((r.alg.storage.observations.detach().cpu().clone(), r.alg.storage.privileged_observations.detach().cpu().clone()))
        return update()
    r.alg.update = snap_then_update
    return snaps


def run_history_check(device):
    """row t of the storage = the reference stack of the RAW table at step t, for both tensors, across dones and across the iteration
    boundary (shared with tests/test_obs_history_gpu.py); H = 3, Hc = 2, two iterations of four steps"""
    env = _env_on(DoneStubEnv(), device)
    r = _runner(env, device=device)
    assert r.obs_history.length == 3 and r.critic_obs_history.length == 2
    assert r.alg.actor_critic.actor.model[0].in_features == 3 * 39 and r.alg.actor_critic.critic.model[0].in_features == 2 * 168
    snaps = _snapshots(r)
    r.learn(2)
    assert r.alg.storage.observations.shape == (4, 8, 117) and r.alg.storage.privileged_observations.shape == (4, 8, 336)
    for table, which, H in ((env.obs_table, 0, 3), (env.pri_table, 1, 2)):
        want = R.stack_table(table.cpu().numpy(), DONE_STEPS, H)
        for it in range(2):
            for row in range(4):
                t = it * 4 + row
                assert np.array_equal(snaps[it][which][row].numpy(), want[t]), (which, it, row)
        hist = r.obs_history if which == 0 else r.critic_obs_history
        assert np.array_equal(hist.current.cpu().numpy(), want[8])      # compute_returns' input: the rows after the last step
    return r


def test_storage_keeps_each_steps_own_stack():
    run_history_check("cpu")


def test_the_scripted_dones_are_seen():
    """(the check above crosses dones: rows that are three copies of one frame appear exactly where the script says)"""
    want = R.stack_table(DoneStubEnv().obs_table.numpy(), DONE_STEPS, 3)
    for t in range(1, 9):
        refilled = {n for n in range(8) if np.array_equal(want[t][n, :39], want[t][n, 78:])}
        assert refilled == set(DONE_STEPS.get(t, ())), t


def test_learn_twice_equals_one_longer_learn():
    a, b = _runner(), _runner()
    sa, sb = _snapshots(a), _snapshots(b)
    a.learn(1); a.learn(1)
    b.learn(2)
    assert len(sa) == len(sb) == 2
    for x, y in zip(sa, sb):
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
    assert torch.equal(a.obs_history.current, b.obs_history.current)


def test_critic_history_alone():
    r = _runner(H=1, Hc=2)
    assert r.obs_history is None and r.critic_obs_history.length == 2
    snaps = _snapshots(r)
    r.learn(1)
    assert snaps[0][0].shape == (4, 8, 39)      # (single raw frames: the stub's one output buffer is the actor's input itself)
    assert np.array_equal(snaps[0][1].numpy(), R.stack_table(r.env.pri_table.numpy(), DONE_STEPS, 2)[:4])


def test_without_privileged_observations_the_critic_gets_the_actor_stack():
    r = _runner(DoneStubEnv(pri=False), H=3, Hc=1)
    assert r.critic_obs_history is None and r.alg.actor_critic.critic.model[0].in_features == 3 * 39
    r.learn(1)
    with pytest.raises(ValueError, match="critic_obs_history_length"):
        _runner(DoneStubEnv(pri=False), H=3, Hc=2)


def test_history_first_then_normalisation():
    r = _runner(norm=True)
    assert r.obs_normalizer.dim == 3 * 39 and r.critic_obs_normalizer.dim == 2 * 168
    snaps = _snapshots(r)
    r.learn(2)
    for table, which, H, norm in ((r.env.obs_table, 0, 3, r.obs_normalizer), (r.env.pri_table, 1, 2, r.critic_obs_normalizer)):
        stack = R.stack_table(table.numpy(), DONE_STEPS, H)          # exact, float32
        ref = NR.RefNormalizer(stack.shape[2])
        want = [(ref.normalize(stack[0]), ref.mean, ref.std)]         # learn()'s first rows: the statistics as they are
        for t in range(1, 8):
            want.append((ref.forward(stack[t]), ref.mean, ref.std))
        for it in range(2):
            for row in range(4):
                y, m, sd = want[it * 4 + row]
                got = snaps[it][which][row].numpy().astype(np.float64)
                x = stack[it * 4 + row].astype(np.float64)
                bound = np.maximum(16 * NR.EPS * (np.abs(m) + np.abs(x - m) + sd) / (sd + NR.EPS_NORM), NR.EPS)   # obs_norm_ref.check's y bound
                assert (np.abs(got - y) <= bound).all(), (which, it, row, float((np.abs(got - y) / bound).max()))
        assert int(norm.count) == 8 * 8


# ---- checkpoints ---------------------------------------------------------------------------------------------------------------------
def test_checkpoint_enabled(tmp_path):
    r = _runner()
    r.learn(1)
    r.save(str(tmp_path / "model_1.pt"))
    ck = torch.load(tmp_path / "model_1.pt", weights_only=False)
    assert set(ck) == REFERENCE_KEYS | {"obs_history"} and ck["obs_history"] == {"actor": 3, "critic": 2}
    r2 = _runner()
    r2.load(str(tmp_path / "model_1.pt"))
    assert torch.equal(r.alg.actor_critic.actor.model[0].weight, r2.alg.actor_critic.actor.model[0].weight)
    assert r2.alg.actor_critic.actor.model[0].weight.shape[1] == 117


def test_checkpoint_disabled_keeps_the_reference_keys(tmp_path):
    r = _runner(H=1, Hc=1)
    assert r.obs_history is None and r.critic_obs_history is None and r.obs_history_length == 1 and r.critic_obs_history_length == 1
    assert r.alg.actor_critic.actor.model[0].in_features == 39 and r.alg.actor_critic.critic.model[0].in_features == 168
    r.learn(1)
    r.save(str(tmp_path / "model_1.pt"))
    assert set(torch.load(tmp_path / "model_1.pt", weights_only=False)) == REFERENCE_KEYS


def test_checkpoint_mismatch_raises(tmp_path):
    on, off, other = _runner(), _runner(H=1, Hc=1), _runner(H=3, Hc=1)
    on.save(str(tmp_path / "model_on.pt"))
    off.save(str(tmp_path / "model_off.pt"))
    for runner, name in ((off, "model_on.pt"), (on, "model_off.pt"), (other, "model_on.pt")):
        with pytest.raises(ValueError, match="--obs_history") as e:
            runner.load(str(tmp_path / name))
        assert "--critic_obs_history" in str(e.value)


def test_train_state_carries_the_rows(tmp_path):
    r = _runner()
    r.env.get_state = lambda: {}
    r.learn(1)
    state = r._train_state()
    assert torch.equal(state["obs_history"]["actor"]["rows"], r.obs_history.current) and state["obs_history"]["actor"]["primed"]
    assert torch.equal(state["obs_history"]["critic"]["rows"], r.critic_obs_history.current)
    assert "obs_history" not in _train_state_of_default()


def test_train_state_mismatch_raises(tmp_path):
    on, off = _runner(), _runner(H=1, Hc=1)
    for r in (on, off):
        r.env.get_state = lambda: {}
    torch.save(on._train_state(), tmp_path / "train_state_1.pt")
    torch.save(off._train_state(), tmp_path / "train_state_2.pt")
    with pytest.raises(ValueError, match="--obs_history"):
        off.load_train_state(str(tmp_path / "model_1.pt"))
    with pytest.raises(ValueError, match="--obs_history"):
        on.load_train_state(str(tmp_path / "model_2.pt"))


def _train_state_of_default():
    r = _runner(H=1, Hc=1)
    r.env.get_state = lambda: {}
    return r._train_state()


# ---- flags ---------------------------------------------------------------------------------------------------------------------------
def test_cli_flags_reach_the_runner_config():
    a = get_args([])
    assert a.obs_history == 1 and a.critic_obs_history == 1
    _, cfg = update_cfg_from_args(None, config.GR1T1CfgPPO(), a)
    assert "obs_history_length" not in class_to_dict(cfg)["runner"] and "critic_obs_history_length" not in class_to_dict(cfg)["runner"]
    _, cfg = update_cfg_from_args(None, config.GR1T1CfgPPO(), get_args(["--obs_history", "3", "--critic_obs_history", "2"]))
    assert class_to_dict(cfg)["runner"]["obs_history_length"] == 3 and class_to_dict(cfg)["runner"]["critic_obs_history_length"] == 2
    _, cfg = update_cfg_from_args(None, config.GR1T1CfgPPO(), get_args(["--obs_history", "5"]))
    assert class_to_dict(cfg)["runner"]["obs_history_length"] == 5 and "critic_obs_history_length" not in class_to_dict(cfg)["runner"]


@pytest.mark.parametrize("cls", CFGS)
def test_config_classes_have_no_new_attribute(cls):
    for key in ("obs_history_length", "critic_obs_history_length"):
        assert not hasattr(cls.runner, key) and key not in class_to_dict(cls())["runner"]
    update_cfg_from_args(None, cls(), get_args(["--obs_history", "3", "--critic_obs_history", "2"]))
    for key in ("obs_history_length", "critic_obs_history_length"):
        assert not hasattr(cls.runner, key) and key not in class_to_dict(cls())["runner"]


@pytest.mark.parametrize("argv", [["--obs_history", "0"], ["--critic_obs_history", "0"], ["--obs_history", "-2"]])
def test_lengths_below_one_raise(argv):
    with pytest.raises(ValueError, match="obs_history"):
        get_args(argv)


def test_runner_refuses_lengths_below_one():
    with pytest.raises(ValueError, match="obs_history_length"):
        _runner(H=0)
    with pytest.raises(ValueError, match="obs_history_length"):
        _runner(Hc=0)


# ---- HistoryPolicy and the export ----------------------------------------------------------------------------------------------------
def _script_round_trip(module, tmp_path):
    path = str(tmp_path / "scripted.pt")
    torch.jit.script(module).save(path)
    return torch.jit.load(path)


def test_history_policy_eager_and_scripted(tmp_path):
    N, D, H = 8, 39, 3
    actor = _runner().alg.actor_critic.actor.eval()
    eager = HistoryPolicy(copy.deepcopy(actor), D, H)
    jit = _script_round_trip(HistoryPolicy(copy.deepcopy(actor), D, H), tmp_path)
    x = R.frames(N, D, 9)
    d3 = R.dones("every_other", N, 0)
    ref = R.RefHistory(N, D, H)
    no = np.zeros(N, dtype=bool)
    with torch.no_grad():
        for t in range(8):
            if t == 3:      # what play.py does after an env.step that ended episodes
                eager.reset(torch.tensor(d3)); jit.reset(torch.tensor(d3))
            if t == 5:
                eager.reset_memory(); jit.reset_memory()
                ref = R.RefHistory(N, D, H)
            want_rows = ref.push(x[t], d3 if t == 3 else no)
            want = actor(torch.tensor(want_rows))
            xt = torch.tensor(x[t])
            assert torch.equal(eager(xt), want), t
            assert torch.equal(jit(xt), want), t
            assert np.array_equal(eager.rows.numpy(), want_rows)
        small = torch.tensor(x[8][:4])     # another batch size: a fill
        want = actor(small.repeat(1, H))
        assert torch.equal(eager(small), want) and torch.equal(jit(small), want)
        assert eager.rows.shape == (4, H * D)


def test_history_policy_reset_takes_any_dtype():
    p = HistoryPolicy(torch.nn.Identity(), 2, 2)
    x = torch.tensor([[1.0, 2.0], [3.0, 4.0]])
    p.reset(torch.tensor([1, 0]))                 # before the first call: nothing to mark
    assert p(x).tolist() == [[1, 2, 1, 2], [3, 4, 3, 4]]
    p.reset(torch.tensor([0, 1]))                 # (a reference-style long reset_buf)
    assert p(10 * x).tolist() == [[1, 2, 10, 20], [30, 40, 30, 40]]
    assert p(100 * x).tolist() == [[10, 20, 100, 200], [30, 40, 300, 400]]     # the mark is spent


def test_exported_module_takes_raw_single_frames(tmp_path):
    r = _runner(norm=True)
    r.learn(2)
    ac, norm = r.alg.actor_critic, r.obs_normalizer
    policy = r.get_inference_policy()
    assert isinstance(policy, HistoryPolicy) and not norm.training
    plain = torch.jit.load(export_policy_as_jit(ac, str(tmp_path / "plain"), history=3))
    normed = torch.jit.load(export_policy_as_jit(ac, str(tmp_path / "normed"), normalizer=norm, history=3))
    N, D, H = 8, 39, 3
    x, ref, no = R.frames(N, D, 5), R.RefHistory(N, D, H), np.zeros(N, dtype=bool)
    d2 = R.dones("single", N, 0)
    plain.reset_memory(); normed.reset_memory()
    with torch.no_grad():
        for t in range(5):
            if t == 2:
                for p in (plain, normed, policy):
                    p.reset(torch.tensor(d2))
            rows = torch.tensor(ref.push(x[t], d2 if t == 2 else no))
            xt = torch.tensor(x[t])
            assert torch.equal(plain(xt), ac.actor(rows)), t
            want = ac.actor((rows - norm._mean) / (norm._std + norm.eps))
            assert (normed(xt) - want).abs().max() < 1e-6, t          # (tests/test_obs_norm.py's bound for the exported normaliser)
            assert torch.equal(policy(xt), want), t
            assert (want - ac.actor(rows)).abs().max() > 1e-3         # the normaliser is in there
    assert int(norm.count) == 64                                       # eval mode: the calls above left the statistics alone


def test_inference_policy_without_history_is_what_it_was():
    r = _runner(H=1, Hc=1)
    assert r.get_inference_policy() == r.alg.actor_critic.act_inference


# ---- the C entry ---------------------------------------------------------------------------------------------------------------------
def test_c_entry_checks_its_arguments():
    """invalid sizes, NULL pointers, aliasing buffers: negative, nothing launched (no GPU needed; the pointers are never followed)"""
    from wiki_grx_gym_amd.rl.fused_loss import load_ppo_library
    push = load_ppo_library().grx_obs_history_push
    obs, src, dst, dones = 0x10000000, 0x20000000, 0x30000000, 0x40000000      # far apart: N * H * D * 4 = 960 bytes
    assert push(0, 5, 3, obs, dones, 0, src, dst, None) < 0                    # N = 0
    assert push(16, 0, 3, obs, dones, 0, src, dst, None) < 0                   # D = 0
    assert push(16, 5, 0, obs, dones, 0, src, dst, None) < 0                   # H = 0
    assert push(16, 5, 3, None, dones, 0, src, dst, None) < 0                  # NULL obs
    assert push(16, 5, 3, obs, dones, 0, src, None, None) < 0                  # NULL dst
    assert push(16, 5, 3, obs, dones, 0, dst, dst, None) < 0                   # src == dst
    assert push(16, 5, 3, obs, dones, 1, dst, dst, None) < 0                   # ... also when every row is filled
    assert push(16, 5, 3, obs, dones, 0, dst - 8, dst, None) < 0               # overlapping ranges
    assert push(16, 5, 3, obs, dones, 0, dst + 956, dst, None) < 0
    assert push(16, 5, 3, dst + 100, dones, 0, src, dst, None) < 0             # the frame inside dst
    assert push(16, 5, 3, obs, dones, 0, None, dst, None) < 0                  # NULL src when a row may shift
    assert push(4096, 4096, 128, obs, dones, 0, src, dst, None) < 0            # N * H * D = 2^31
