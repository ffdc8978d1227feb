"""Observation history on the GPU (include/grx_ppo.h grx_obs_history_push, rl/history.py): the HIP push against the numpy reference
of tests/obs_history_ref.py (exact: the operation only copies), the two buffers, determinism, dones dtypes, the torch spelling on the
device, stream order, the runner over the stub env, train / save / play / export with the option, exact resume, the default path."""
import os

import numpy as np
import pytest
import torch

from tests import obs_history_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PUSHES = 6
SHAPES = [(1, 1, 2), (3, 5, 1), (257, 39, 3), (5, 300, 4), (64, 168, 6), (4096, 39, 15)]   # one element per frame; H = 1; an odd width and
                                                          # rows no multiple of a block; a row wider than a block; the critic's width;
                                                          # the training shape at its longest


def _hist(N, D, H):
    from wiki_grx_gym_amd.rl.history import ObsHistory
    return ObsHistory(N, D, H, DEV)


@pytest.mark.parametrize("N,D,H", SHAPES, ids=[f"{n}x{d}x{h}" for n, d, h in SHAPES])
def test_hip_push_against_reference(N, D, H):
    xs = [torch.tensor(f).to(DEV) for f in R.frames(N, D, PUSHES + 1)]
    for pattern in R.PATTERNS:
        want = R.reference(N, D, H, pattern, PUSHES)
        h = _hist(N, D, H)
        assert h._hip(xs[0])
        got = h.fill(xs[0])
        assert np.array_equal(got.cpu().numpy(), want[0]), (pattern, "fill")
        for t in range(PUSHES):
            got = h.push(xs[t + 1], torch.tensor(R.dones(pattern, N, t)).to(DEV))
            assert got is h.current and np.array_equal(got.cpu().numpy(), want[t + 1]), (pattern, t)


def test_previous_rows_survive_the_next_push():
    N, D, H = 257, 39, 3
    h = _hist(N, D, H)
    xs = [torch.tensor(f).to(DEV) for f in R.frames(N, D, 4)]
    d = torch.tensor(R.dones("every_other", N, 0)).to(DEV)
    h.fill(xs[0])
    y0 = h.push(xs[1], d); keep = y0.clone()
    y1 = h.push(xs[2], d)
    assert y1.data_ptr() != y0.data_ptr() and torch.equal(y0, keep)
    assert h.push(xs[3], d).data_ptr() == y0.data_ptr()


def test_same_input_twice_gives_the_same_bytes():
    N, D, H = 4096, 39, 15
    xs = [torch.tensor(f).to(DEV) for f in R.frames(N, D, 3)]
    outs = []
    for _ in range(2):
        h = _hist(N, D, H)
        h.fill(xs[0])
        for t in range(2):
            y = h.push(xs[t + 1], torch.tensor(R.dones("single", N, t)).to(DEV))
        outs.append(y.cpu().numpy().tobytes())
    assert outs[0] == outs[1]


def test_dones_dtypes_and_the_torch_spelling_on_the_device():
    N, D, H = 257, 39, 3
    x = R.frames(N, D, 3)
    want = R.reference(N, D, H, "every_other", 2)[2]
    for dtype in (torch.bool, torch.uint8, torch.int64):
        h = _hist(N, D, H)
        h.fill(torch.tensor(x[0]).to(DEV))
        for t in range(2):
            got = h.push(torch.tensor(x[t + 1]).to(DEV), torch.tensor(R.dones("every_other", N, t)).to(DEV).to(dtype))
        assert np.array_equal(got.cpu().numpy(), want), dtype
    h = _hist(N, D, H)                                                        # the same frames, strided: the torch spelling
    strided = [torch.tensor(np.ascontiguousarray(f.T)).to(DEV).t() for f in x]
    assert not h._hip(strided[0])
    h.fill(strided[0])
    for t in range(2):
        got = h.push(strided[t + 1], torch.tensor(R.dones("every_other", N, t)).to(DEV))
    assert np.array_equal(got.cpu().numpy(), want)


def test_push_on_the_current_stream():
    """the frame is produced on a side stream behind a long matrix product; the push issued there reads the finished frame"""
    N, D, H = 257, 39, 3
    x = R.frames(N, D, 2)
    h = _hist(N, D, H)
    x0, x1 = torch.tensor(x[0]).to(DEV), torch.tensor(x[1]).to(DEV)
    big = torch.ones(2048, 2048, device=DEV)
    frame = torch.zeros(N, D, device=DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        h.fill(x0)
        for _ in range(4):
            big = (big @ big) * (1.0 / 2048)          # stays all ones
        frame.copy_(x1 * big[:N, :D])                  # = x1, after the products
        got = h.push(frame, torch.zeros(N, dtype=torch.bool, device=DEV))
    side.synchronize()
    assert np.array_equal(got.cpu().numpy(), R.reference(N, D, H, "none", 1)[1])


def test_storage_keeps_each_steps_own_stack():
    """the runner on the device over the stub env of tests/test_obs_history.py: the captured act graph takes the wider input, the
    fused store and the row gather carry H * D columns"""
    from tests.test_obs_history import run_history_check
    r = run_history_check(DEV)
    assert r.obs_history.current.is_cuda and r.alg.storage.observations.is_cuda


@pytest.mark.parametrize("norm", [False, True], ids=["plain", "empirical_normalization"])
def test_train_save_play_export(tmp_path, monkeypatch, norm):
    from wiki_grx_gym_amd.envs import GR1T1CfgPPO
    from wiki_grx_gym_amd.rl.history import HistoryPolicy
    from wiki_grx_gym_amd.scripts.play import play
    from wiki_grx_gym_amd.utils import get_args, task_registry
    # (play() takes the registered config instance, which the flags write to: undone when the test ends)
    reg = task_registry.train_cfgs["GR1T1"].runner
    monkeypatch.setattr(reg, "obs_history_length", 1, raising=False)
    monkeypatch.setattr(reg, "empirical_normalization", False, raising=False)
    flags = ["--obs_history", "3"] + (["--empirical_normalization"] if norm else [])
    args = get_args(["--task", "GR1T1", "--headless", "--num_envs", "256", "--seed", "3"] + flags)
    env, _ = task_registry.make_env("GR1T1", args=args)
    tcfg = GR1T1CfgPPO()
    tcfg.runner.num_steps_per_env = 16
    runner, _ = task_registry.make_alg_runner(env, name="GR1T1", args=args, train_cfg=tcfg, log_root=str(tmp_path))
    assert runner.obs_history_length == 3 and runner.critic_obs_history is None
    snaps, losses, update = [], [], runner.alg.update

    def snap_then_update():
        st = runner.alg.storage
        snaps.append((st.observations.detach().cpu().clone(), st.dones.detach().cpu().clone()))
        losses.append(update())
        return losses[-1]
    runner.alg.update = snap_then_update
    runner.learn(num_learning_iterations=3, init_at_random_ep_len=True)
    assert len(losses) == 3 and all(np.isfinite(float(v)) for pair in losses for v in pair), losses
    assert runner.alg.storage.observations.shape[-1] == 117 and runner.alg.actor_critic.actor.model[0].in_features == 117
    if norm:
        assert runner.obs_normalizer.dim == 117 and int(runner.obs_normalizer.count) == 256 * 16 * 3
    else:
        shifted = refilled = 0
        for obs, dones in snaps:
            done = dones.squeeze(-1).bool()[:-1]                 # [T - 1, N]: dones[t] came with the frame of row t + 1
            old, new = obs[:-1], obs[1:]
            assert torch.equal(new[~done][:, :78], old[~done][:, 39:])
            assert torch.equal(new[done], new[done][:, 78:].repeat(1, 3))
            shifted += int((~done).sum()); refilled += int(done.sum())
        print(f"obs history: {shifted} shifted rows, {refilled} refilled rows")
        assert shifted > 0 and refilled > 0, (shifted, refilled)
    ck = torch.load(os.path.join(runner.log_dir, "model_3.pt"), weights_only=False)
    assert ck["obs_history"] == {"actor": 3, "critic": 1}

    with pytest.raises(ValueError, match="--obs_history"):              # play without the flag refuses the checkpoint
        play(get_args(["--task", "GR1T1", "--headless", "--seed", "3"] + flags[2:]), steps=1, log_root=str(tmp_path))
    out = play(get_args(["--task", "GR1T1", "--headless", "--seed", "3"] + flags), steps=30, log_root=str(tmp_path))
    assert len(open(out["states"]).readlines()) == 30
    penv, prunner = out["env"], out["runner"]
    policy = prunner.get_inference_policy(device=penv.device)
    assert isinstance(policy, HistoryPolicy)
    jit = torch.jit.load(out["exported"])                                # on the CPU, fed env 0's raw frames
    jit.reset_memory()
    obs, worst = penv.get_observations(), 0.0
    with torch.no_grad():
        for _ in range(30):
            assert obs.shape == (50, 39)
            actions = policy(obs.detach())
            a0 = jit(obs[0:1].detach().cpu())
            worst = max(worst, float((a0[0] - actions[0].cpu()).abs().max()))
            obs, _, _, dones, _ = penv.step(actions.detach())
            policy.reset(dones)
            jit.reset(dones[0:1].cpu())
    print(f"obs history: exported policy against the device policy over 30 steps, env 0: max |difference| {worst:.3g}")
    assert worst < 1e-6                                                  # (tests/test_play_gpu.py's tolerance for the exported actor)


def test_training_resume_is_exact(tmp_path):
    """6 uninterrupted iterations against 3 + a resume from checkpoint 2 that trains iterations 3-5, with --obs_history 3: equal
    parameters, Adam state, learning rate, env state and logged scalars (train_state_<it>.pt carries the stacked rows)"""
    from tests.test_exact_resume_gpu import _assert_runs_equal, _scalars, _train
    argv = ["--exact_resume", "--obs_history", "3"]
    a = _train(tmp_path, "A", ["--max_iterations", "6"] + argv)
    run_a = a["log_dir"]
    state = torch.load(os.path.join(run_a, "train_state_2.pt"), weights_only=False)
    assert state["obs_history"]["actor"]["rows"].shape == (1024, 117) and state["obs_history"]["critic"] is None
    b = _train(tmp_path, "B", ["--max_iterations", "3", "--resume", "--load_run", run_a, "--checkpoint", "2"] + argv)
    _assert_runs_equal(a, b)
    ra, rb = _scalars(run_a, 2), _scalars(b["log_dir"], 2)
    assert ra.keys() == rb.keys() and any(t == "Train/mean_reward" for t, _ in ra)
    for k in ra:
        assert ra[k] == rb[k], (k, ra[k], rb[k])


def test_default_path_builds_nothing(tmp_path):
    """without the flags: no history object, the checkpoint keeps exactly the reference's keys, the policy takes single frames"""
    from wiki_grx_gym_amd.envs import GR1T1CfgPPO
    from wiki_grx_gym_amd.utils import get_args, task_registry
    args = get_args(["--task", "GR1T1", "--headless", "--num_envs", "256", "--seed", "3"])
    env, _ = task_registry.make_env("GR1T1", args=args)
    tcfg = GR1T1CfgPPO()
    tcfg.runner.num_steps_per_env = 8
    runner, _ = task_registry.make_alg_runner(env, name="GR1T1", args=args, train_cfg=tcfg, log_root=str(tmp_path))
    assert runner.obs_history is None and runner.critic_obs_history is None
    runner.learn(num_learning_iterations=1)
    for name in ("model_0.pt", "model_1.pt"):
        ck = torch.load(os.path.join(runner.log_dir, name), weights_only=False)
        assert set(ck) == {"model_state_dict", "optimizer_state_dict", "iter", "infos"}
    assert runner.alg.storage.observations.shape[-1] == 39 and runner.alg.actor_critic.actor.model[0].in_features == 39
    assert runner.get_inference_policy(device=env.device) == runner.alg.actor_critic.act_inference
