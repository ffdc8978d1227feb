"""Exact resume on the GPU: a handle's snapshot (include/grx.h grx_save_state / grx_load_state) continues a run bit for bit on every
layout, a mismatching handle refuses it and stays as it was, and a training run resumed from train_state_<it>.pt with --exact_resume
ends where the uninterrupted run ends (parameters, Adam, learning rate, env state, logged scalars)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.helpers import make_cfg, random_actions
from wiki_grx_gym_amd import _capi
from wiki_grx_gym_amd.sim import GrxError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 256


def _cfg(task="GR1T1", terrain="heightfield", base=False):
    cfg = make_cfg(task, noise=True, dr=True, push=True, terrain=terrain, curriculum=True)
    cfg.env.num_envs = N
    cfg.env.episode_length_s = 0.5            # resets, time-outs and curriculum moves within a few dozen steps
    cfg.domain_rand.push_interval_s = 0.2
    cfg.commands.resampling_command_interval_s = 0.3
    cfg.terrain.max_init_terrain_level = 4
    if base:   # legged_gym's base reward terms and the command curriculum (the *_base entries)
        cfg.rewards.scales.tracking_lin_vel = 1.0
        cfg.rewards.scales.torques = -1e-5
        cfg.rewards.scales.orientation = -0.5
        cfg.commands.curriculum = True
    return cfg


def _env(cfg):
    from wiki_grx_gym_amd.envs.grx_env import GRxEnv
    return GRxEnv(cfg, sim_device="cuda:0")


def _record(env, out):
    """every GRX_T_* tensor the handle publishes, what step() returned, extras["episode"], the command ranges and the on-refresh tensors"""
    obs, pri, rew, reset, extras = out
    rec = {"obs": obs.clone(), "pri": pri.clone() if pri is not None else None, "rew": rew.clone(), "reset": reset.clone(),
           "episode": {k: float(v) for k, v in extras["episode"].items()}, "ranges": env.command_ranges,
           "rbs": env.rigid_body_states.clone(), "heights": env.measured_heights.clone()}
    for name in _capi.TENSOR_IDS:
        try:
            rec["T_" + name] = env._sim.tensor(name).clone()
        except GrxError:   # (not published by this handle)
            pass
    return rec


def _assert_same(a, b, where):
    assert a.keys() == b.keys(), where
    for k in a:
        x, y = a[k], b[k]
        if torch.is_tensor(x):
            assert torch.equal(x, y), f"{where}: {k} differs"
        else:
            assert x == y, f"{where}: {k}: {x} != {y}"


LAYOUTS = [
    ("GR1T1", "heightfield", False, {}, "grx_step_kernel_quad<true, 8, false>"),
    ("GR1T1", "heightfield", False, {"GRX_LANES_PER_ENV": "2", "GRX_WAVES_PER_BLOCK": "8"}, "grx_step_kernel<true, 8, false>"),
    ("GR1T1", "heightfield", False, {"GRX_WAVES_PER_BLOCK": "1"}, "grx_step_kernel<true, 1, false>"),
    ("GR1T1Full", "heightfield", False, {"GRX_TREE_G": "16"}, "grx_step_tree16<true, false>"),
    ("GR1T1Full", "heightfield", False, {"GRX_TREE_G": "8"}, "grx_step_tree<true, false>"),
    ("GR1T1", "trimesh", False, {}, "grx_step_kernel_quad_trimesh<8, false>"),
    ("GR1T1", "heightfield", True, {}, "grx_step_kernel_base<true, false>"),
]


@pytest.mark.parametrize("task,terrain,base,envvars,kernel", LAYOUTS, ids=[l[4] for l in LAYOUTS])
def test_handle_round_trip(task, terrain, base, envvars, kernel, monkeypatch):
    """Run A: 60 steps of seeded random actions, get_state() right after step 30 (whose statistics the next launch would reduce).
    Run B: a fresh env of the same config, set_state(), steps 31-60: every tensor, output and statistic equal at every step."""
    for k, v in envvars.items():
        monkeypatch.setenv(k, v)
    cfg = _cfg(task, terrain, base)
    gen = torch.Generator().manual_seed(7)
    np.random.seed(3)
    a = _env(cfg)
    assert a._sim.layout()["kernel"] == kernel
    a.reset()
    actions = [random_actions(cfg, N, gen).cuda() for _ in range(60)]
    recs, resets = [], 0
    for t in range(60):
        out = a.step(actions[t])
        if t + 1 == 30:
            snap = a.get_state()
            levels30 = a.terrain_levels.clone()
        if t + 1 > 30:
            recs.append(_record(a, out))
            resets += int(out[3].sum())
    assert resets > 0 and not torch.equal(levels30, a.terrain_levels)   # resets and curriculum moves happened after the snapshot
    if base:
        assert "max_command_x" in recs[-1]["episode"]
    a.close()
    np.random.seed(11)   # (set_state restores numpy's generator: the action-delay draw)
    b = _env(cfg)
    b.reset()
    b.step(actions[5])   # a different history before the restore
    b.set_state(snap)
    assert b.common_step_counter == snap["common_step_counter"]
    for t in range(30, 60):
        _assert_same(recs[t - 30], _record(b, b.step(actions[t])), f"step {t + 1}")
    b.close()


def _handle_tensors(env):
    out = {}
    for name in _capi.TENSOR_IDS:
        try:
            out[name] = env._sim.tensor(name).clone()
        except GrxError:
            pass
    return out


@pytest.mark.parametrize("what", ["num_envs", "model", "terrain", "layout", "base_terms", "seed"])
def test_restore_into_a_different_handle_is_refused(what, monkeypatch):
    """A snapshot restores only into a handle created from the same inputs; the refused handle's tensors are unchanged."""
    cfg = _cfg()
    src = _env(cfg)
    src.reset()
    for _ in range(3):
        src.step(torch.zeros(N, src.num_actions, device="cuda"))
    snap = src.get_state()
    src.close()
    task, terrain, base = "GR1T1", "heightfield", False
    if what == "model":
        task = "GR1T2"
    elif what == "terrain":
        terrain = "trimesh"
    elif what == "base_terms":
        base = True
    elif what == "layout":
        monkeypatch.setenv("GRX_WAVES_PER_BLOCK", "1")
    cfg2 = _cfg(task, terrain, base)
    if what == "num_envs":
        cfg2.env.num_envs = N // 2
    if what == "seed":
        cfg2.seed = 2
    dst = _env(cfg2)
    dst.reset()
    dst.step(torch.zeros(dst.num_envs, dst.num_actions, device="cuda"))
    before = _handle_tensors(dst)
    counter = dst.common_step_counter
    with pytest.raises(GrxError, match="grx load_state"):
        dst._sim.load_state(snap["sim"])
    with pytest.raises((GrxError, ValueError)):
        dst.set_state(snap)
    after = _handle_tensors(dst)
    assert before.keys() == after.keys()
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert dst.common_step_counter == counter
    dst.close()


# ---- training resume ---------------------------------------------------------------------------------------------------------------
DRIVER = r'''
import sys
import torch
sys.path.insert(0, {root!r})
from wiki_grx_gym_amd.envs import *  # noqa: F401,F403
from wiki_grx_gym_amd.utils import get_args, task_registry
argv = sys.argv[1:]
log_root, out = argv.pop(0), argv.pop(0)
args = get_args(argv)
env_cfg, train_cfg = task_registry.get_cfgs("GR1T1")
env_cfg.terrain.mesh_type = "heightfield"
env_cfg.terrain.curriculum = True
env, _ = task_registry.make_env("GR1T1", args=args, env_cfg=env_cfg)
train_cfg.runner.save_interval = 2
runner, train_cfg = task_registry.make_alg_runner(env, args=args, train_cfg=train_cfg, log_root=log_root)
runner.learn(num_learning_iterations=train_cfg.runner.max_iterations, init_at_random_ep_len=True)
alg = runner.alg
torch.save({{"params": {{k: v.cpu() for k, v in alg.actor_critic.state_dict().items()}}, "opt": alg.optimizer.state_dict(),
            "learning_rate": alg.learning_rate, "lr_t": float(alg._lr_t), "root": env.root_states.cpu(), "dof_pos": env.dof_pos.cpu(),
            "dof_vel": env.dof_vel.cpu(), "levels": env.terrain_levels.cpu(), "log_dir": runner.log_dir,
            "iteration": runner.current_learning_iteration}}, out)
'''


def _train(tmp_path, name, argv, extra_env=None, timeout=600):
    """one training process (its own time limit); its runs go to tmp_path / "runs", where a resume finds them"""
    driver = tmp_path / "driver.py"
    driver.write_text(DRIVER.format(root=ROOT))
    out = tmp_path / f"{name}.pt"
    env = dict(os.environ, **(extra_env or {}))
    cmd = [sys.executable, str(driver), str(tmp_path / "runs"), str(out), "--task", "GR1T1", "--headless", "--num_envs", "1024", "--seed", "1"] + argv
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, f"{name}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
    return torch.load(out, weights_only=False)


def _scalars(log_dir, after):
    rows = {}
    for line in open(os.path.join(log_dir, "scalars.jsonl")):
        r = json.loads(line)
        if r["tag"].startswith("Perf/") or r["tag"].endswith("/time") or r["step"] <= after:
            continue
        rows[(r["tag"], r["step"])] = r["value"]
    return rows


def _assert_runs_equal(a, b):
    for k in a["params"]:
        assert torch.equal(a["params"][k], b["params"][k]), k
    sa, sb = a["opt"]["state"], b["opt"]["state"]
    assert sa.keys() == sb.keys()
    for i in sa:
        for k in sa[i]:
            assert torch.equal(sa[i][k].cpu(), sb[i][k].cpu()), (i, k)
    assert a["learning_rate"] == b["learning_rate"] and a["lr_t"] == b["lr_t"]
    for k in ("root", "dof_pos", "dof_vel", "levels"):
        assert torch.equal(a[k], b[k]), k
    assert a["iteration"] == b["iteration"] == 6


VARIANTS = [("graphs", [], {}), ("bf16", ["--precision", "bf16"], {}), ("eager_update", [], {"GRX_PPO_GRAPH": "0"})]


def test_training_resume_is_exact(tmp_path):
    """GR1T1, 1024 envs, rough curriculum, save_interval 2: 6 uninterrupted iterations against 3 + a resume from checkpoint 2 that trains
    iterations 3-5.  Final parameters, Adam state, learning rate, env root / dof state and terrain levels, and every logged scalar after
    the resume point (but Perf/* and */time) are equal -- for captured graphs, bf16 and the eager update.  Stops at the first failure."""
    for name, argv, extra in VARIANTS:
        d = tmp_path / name
        d.mkdir()
        a = _train(d, "A", ["--max_iterations", "6", "--exact_resume"] + argv, extra)
        run_a = a["log_dir"]
        assert os.path.exists(os.path.join(run_a, "train_state_2.pt")) and os.path.exists(os.path.join(run_a, "model_2.pt"))
        b = _train(d, "B", ["--max_iterations", "3", "--exact_resume", "--resume", "--load_run", run_a, "--checkpoint", "2"] + argv, extra)
        _assert_runs_equal(a, b)
        ra, rb = _scalars(run_a, 2), _scalars(b["log_dir"], 2)
        assert ra.keys() == rb.keys() and any(t == "Train/mean_reward" for t, _ in ra), name
        for k in ra:
            assert ra[k] == rb[k], (name, k, ra[k], rb[k])


def test_default_path_writes_no_training_state(tmp_path):
    """Without --exact_resume model_<it>.pt keeps exactly its keys (iter: the iteration learn() started at) and no train_state_* appears."""
    a = _train(tmp_path, "A", ["--max_iterations", "3"])
    files = sorted(os.listdir(a["log_dir"]))
    assert not [f for f in files if f.startswith("train_state_")]
    assert {"model_0.pt", "model_2.pt", "model_3.pt"} <= set(files)
    ck = torch.load(os.path.join(a["log_dir"], "model_2.pt"), weights_only=False)
    assert set(ck) == {"model_state_dict", "optimizer_state_dict", "iter", "infos"} and ck["iter"] == 0 and ck["infos"] is None
