"""The concurrent state estimator on the MI355X (rl/estimator.py, csrc/grx_ppo_est.hip): grx_est_forward bit for bit
against the per-layer path (fused_loss.mlp_forward + torch.cat + the column select), against the float64 reference (tests/est_ref.py), its
row independence, repeatability and argument checks, the fused launch against GRX_EST_FUSED=0 through the runner, and the runner end to
end through the HIP env, play and the exported module."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import est_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HIDDEN = [(32,), (48, 33), (256, 128, 64)]


def _M():
    from wiki_grx_gym_amd.rl import estimator
    return estimator


def _case(N, D, hidden, E, P=None, seed=0):
    """the net, x [N, D], pri [N, P] and E target columns; weights and inputs scaled so that every ELU sees both signs"""
    from wiki_grx_gym_amd.rl.modules import MLP
    g = torch.Generator().manual_seed(1000 * seed + 7 * N + 3 * D + E + len(hidden))
    net = MLP(D, E, list(hidden), "elu")
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (1.0 / np.sqrt(p.shape[-1]) if p.dim() == 2 else 0.5))
    P = P if P is not None else D + 8 + 5
    x = 1.5 * torch.randn(N, D, generator=g)
    pri = torch.randn(N, P, generator=g)
    cols = [int(c) for c in torch.randperm(P, generator=g)[:E]]
    return net.to(DEV), x.to(DEV), pri.to(DEV), cols


def _per_layer(net, x, pri, cols):
    from wiki_grx_gym_amd.rl.fused_loss import mlp_forward
    with torch.no_grad():
        e = mlp_forward(net, x)
    return torch.cat([x, e], 1), pri[:, cols].contiguous(), e


@pytest.mark.parametrize("E", [1, 3, 8])
@pytest.mark.parametrize("hidden", HIDDEN, ids=lambda h: "x".join(map(str, h)))
@pytest.mark.parametrize("D", [39, 40, 195])
def test_one_launch_equals_the_per_layer_path_bit_for_bit(D, hidden, E):
    """N = 1, one short of, at and one past a slab of 64 rows, and three slabs with a short last one; D = 39 and 195 take grx_mlp_layer's
    dword loads, 40 its float4 loads; hidden widths below, at no multiple of and at the 256-column buffer; an odd K (33, 39, 195)"""
    M = _M()
    for N in (1, 63, 64, 65, 130):
        net, x, pri, cols = _case(N, D, hidden, E)
        out, tg = M.est_forward_hip(net, x, pri, cols)
        want_out, want_tg, e = _per_layer(net, x, pri, cols)
        assert out.shape == (N, D + E) and tg.shape == (N, E)
        assert torch.equal(out[:, :D], x), (N, "copy")
        assert torch.equal(out[:, D:], e), (N, "estimate", float((out[:, D:] - e).abs().max()))
        assert torch.equal(out, want_out) and torch.equal(tg, want_tg), (N, "targets")
        with torch.no_grad():   # (inputs scaled so that ELU sees both signs)
            h = torch.nn.functional.linear(x, net.model[0].weight, net.model[0].bias)
        assert bool((h > 0).any()) and bool((h < 0).any())


@pytest.mark.parametrize("hidden", HIDDEN, ids=lambda h: "x".join(map(str, h)))
@pytest.mark.parametrize("D", [39, 40, 195])
def test_against_the_float64_reference(D, hidden):
    """the bound is 4 x the error mlp_forward itself shows against the same reference on the same inputs: the same arithmetic, the margin
    only covers the bound being taken from one draw.  Measured on the MI355X: see DESIGN.md 4.15"""
    M = _M()
    N, E = 130, 8
    net, x, pri, cols = _case(N, D, hidden, E, seed=1)
    lin = [(m.weight.detach().double().cpu().numpy(), m.bias.detach().double().cpu().numpy()) for m in net.model if isinstance(m, torch.nn.Linear)]
    ref_out, ref_tg = R.est_forward_ref([w for w, _ in lin], [b for _, b in lin], x.double().cpu().numpy(), pri.double().cpu().numpy(), cols)
    out, tg = M.est_forward_hip(net, x, pri, cols)
    _, _, e = _per_layer(net, x, pri, cols)
    err = np.abs(out.double().cpu().numpy()[:, D:] - ref_out[:, D:]).max()
    base = np.abs(e.double().cpu().numpy() - ref_out[:, D:]).max()
    print(f"est float64 error D={D} hidden={hidden}: fused {err:.3e}, per-layer {base:.3e}, scale {np.abs(ref_out[:, D:]).max():.3f}")
    assert err <= 4.0 * base
    assert np.array_equal(out.double().cpu().numpy()[:, :D], ref_out[:, :D]) and np.array_equal(tg.double().cpu().numpy(), ref_tg)


@pytest.mark.parametrize("hidden", HIDDEN, ids=lambda h: "x".join(map(str, h)))
def test_a_row_does_not_depend_on_the_batch(hidden):
    M = _M()
    net, x, pri, cols = _case(130, 195, hidden, 3, seed=2)
    full, ftg = M.est_forward_hip(net, x, pri, cols)
    for r in (0, 1, 31, 32, 63, 64, 65, 127, 128, 129):
        one, otg = M.est_forward_hip(net, x[r:r + 1].contiguous(), pri[r:r + 1].contiguous(), cols)
        assert torch.equal(one[0], full[r]) and torch.equal(otg[0], ftg[r]), r


def test_the_same_call_gives_the_same_bytes_and_targets_are_optional():
    M = _M()
    net, x, pri, cols = _case(130, 40, (256, 128, 64), 8, seed=3)
    a, at = M.est_forward_hip(net, x, pri, cols)
    b, bt = M.est_forward_hip(net, x, pri, cols)
    assert torch.equal(a, b) and torch.equal(at, bt)
    c, ct = M.est_forward_hip(net, x)
    assert ct is None and torch.equal(a, c)


def test_rejected_calls_write_nothing():
    from wiki_grx_gym_amd.rl.fused_loss import load_ppo_library
    M, lib = _M(), load_ppo_library()
    N, D, E = 65, 40, 3
    net, x, pri, cols = _case(N, D, (48, 33), E)
    out = torch.full((N, D + E), 777.0, device=DEV)
    tg = torch.full((N, E), 777.0, device=DEV)
    carr = (C.c_int * E)(*cols)

    def call(s=None, N=N, D=D, x=x.data_ptr(), P=pri.shape[1], pri=pri.data_ptr(), cols=carr, out=out.data_ptr(), tg=tg.data_ptr()):
        s = s if s is not None else M.net_struct(net)
        return lib.grx_est_forward(C.addressof(s) if s != 0 else None, N, D, x, P, pri, cols, out, tg, None)
    assert call(s=0) < 0 and call(N=0) < 0 and call(D=0) < 0 and call(D=2049) < 0 and call(x=None) < 0 and call(out=None) < 0
    assert call(P=0) < 0 and call(cols=None) < 0 and call(cols=(C.c_int * E)(0, 1, pri.shape[1])) < 0 and call(cols=(C.c_int * E)(-1, 1, 2)) < 0
    for field, value in (("n_layers", 1), ("n_layers", 5)):
        s = M.net_struct(net)
        setattr(s, field, value)
        assert call(s=s) < 0
    s = M.net_struct(net); s.widths[0] = 257
    assert call(s=s) < 0
    s = M.net_struct(net); s.widths[2] = 9
    assert call(s=s) < 0
    s = M.net_struct(net); s.W[1] = None
    assert call(s=s) < 0
    assert call(out=x.data_ptr()) < 0 and call(out=x.data_ptr() + 4 * (N * D - 1)) < 0                     # out overlapping x
    torch.cuda.synchronize()
    assert bool((out == 777).all()) and bool((tg == 777).all())
    assert call(pri=None) == 0                                                                     # no privileged frame: no targets
    torch.cuda.synchronize()
    assert bool((tg == 777).all()) and not bool((out == 777).any())
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(tg, pri[:, cols])


# ---- the runner through the HIP env ------------------------------------------------------------------------------------------------------------
def _make(tmp_path, flags=(), steps=8, num_envs=64):
    from wiki_grx_gym_amd.envs import GR1T1Cfg, GR1T1CfgPPO
    from wiki_grx_gym_amd.utils import get_args, task_registry
    args = get_args(["--task", "GR1T1", "--headless", "--num_envs", str(num_envs), "--seed", "3", *flags])
    env, _ = task_registry.make_env("GR1T1", args=args, env_cfg=GR1T1Cfg())   # (the registered GR1T1 task: flat terrain)
    tcfg = GR1T1CfgPPO()
    tcfg.runner.num_steps_per_env = steps
    tcfg.algorithm.num_mini_batches = 4
    runner, _ = task_registry.make_alg_runner(env, name=None, args=args, train_cfg=tcfg, log_root=str(tmp_path) if tmp_path else None)
    return env, runner


def _tags(runner):
    out = {}
    for line in open(os.path.join(runner.log_dir, "scalars.jsonl")):
        out.setdefault(line.split('"tag": "')[1].split('"')[0], []).append(float(line.split('"value": ')[1].split(",")[0]))
    return out


def _three_iterations(monkeypatch, fused):
    monkeypatch.setenv("GRX_EST_FUSED", fused)
    M = _M()
    calls = {"hip": 0, "torch": 0}
    hip, tch = M.est_forward_hip, M.est_forward_torch
    monkeypatch.setattr(M, "est_forward_hip", lambda *a, **k: (calls.__setitem__("hip", calls["hip"] + 1), hip(*a, **k))[1])
    monkeypatch.setattr(M, "est_forward_torch", lambda *a, **k: (calls.__setitem__("torch", calls["torch"] + 1), tch(*a, **k))[1])
    env, runner = _make(None, ("--estimator", "--estimator_targets", "lin_vel,base_height,feet_contact,feet_height"))
    runner.learn(num_learning_iterations=1)
    first = (runner.alg.storage.observations.clone(), runner.estimator.targets.clone())
    runner.learn(num_learning_iterations=2)
    params = [p.detach().clone() for p in list(runner.alg.actor_critic.parameters()) + list(runner.estimator.net.parameters())]
    return first, params, dict(calls), runner   # (a copy: a later call's wrappers sit on top of these and count here too)


def test_the_fused_launch_and_the_per_layer_path_train_the_same_bits(monkeypatch):
    """GRX_EST_FUSED=0 against the fused launch over a real GR1T1 env at 64 envs: bit-equal storage rows and targets after one rollout, and
    torch.equal parameters of policy and estimator after three iterations; one forward call per rollout step and one per learn()"""
    (rows_a, tg_a), params_a, calls_a, runner = _three_iterations(monkeypatch, "1")
    (rows_b, tg_b), params_b, calls_b, _ = _three_iterations(monkeypatch, "0")
    assert calls_a == {"hip": 3 * 8 + 2, "torch": 0} and calls_b == {"hip": 0, "torch": 3 * 8 + 2}
    assert rows_a.shape == (8, 64, 39 + 8) and tg_a.shape == (8, 64, 8)
    assert torch.equal(rows_a, rows_b) and torch.equal(tg_a, tg_b)
    assert bool((rows_a[:, :, 39:] != 0).any()) and bool((tg_a != 0).any())
    assert all(torch.equal(a, b) and bool(torch.isfinite(a).all()) for a, b in zip(params_a, params_b))
    assert isinstance(runner.alg._graph, torch.cuda.CUDAGraph) and type(runner.alg._gather).__name__ == "RowGather"   # PPO's captured step is what it was


def test_runner_trains_saves_plays_and_exports(tmp_path, monkeypatch):
    from wiki_grx_gym_amd.scripts.play import play
    from wiki_grx_gym_amd.utils import get_args, task_registry
    # (play() takes the registered config instance, which the flags write to: undone when the test ends)
    reg = task_registry.train_cfgs["GR1T1"].runner
    for name, value in (("obs_history_length", 1), ("empirical_normalization", False), ("estimator", False), ("estimator_targets", "lin_vel"),
                        ("estimator_hidden_dims", [128, 64]), ("estimator_learning_rate", 1e-3), ("estimator_num_epochs", 1)):
        monkeypatch.setattr(reg, name, value, raising=False)
    flags = ("--estimator", "--obs_history", "3", "--empirical_normalization")
    env, runner = _make(tmp_path, flags)
    est = runner.estimator
    before = [p.detach().clone() for p in est.net.parameters()]
    runner.learn(num_learning_iterations=3)
    losses = _tags(runner)["Loss/estimator"]
    assert len(losses) == 3 and all(np.isfinite(v) and v > 0 for v in losses)
    assert all(not torch.equal(a, b) and bool(torch.isfinite(b).all()) for a, b in zip(before, est.net.parameters()))
    assert runner.alg.storage.observations.shape == (8, 64, 117 + 3) and runner.obs_normalizer.dim == 117
    ck = torch.load(os.path.join(runner.log_dir, "model_3.pt"), weights_only=False)
    assert set(ck) == {"model_state_dict", "optimizer_state_dict", "iter", "infos", "obs_norm_state_dict", "critic_obs_norm_state_dict", "obs_history",
                       "estimator"}
    with pytest.raises(ValueError, match="pass --estimator --estimator_targets lin_vel --estimator_hidden_dims 128 64"):
        play(get_args(["--task", "GR1T1", "--headless", "--seed", "3", "--obs_history", "3", "--empirical_normalization"]), steps=2, log_root=str(tmp_path))
    out = play(get_args(["--task", "GR1T1", "--headless", "--seed", "3", *flags]), steps=10, log_root=str(tmp_path))
    prunner, penv = out["runner"], out["env"]
    assert len(open(out["states"]).readlines()) == 10 and prunner.current_learning_iteration == 3
    sd, sd2 = est.state_dict(), prunner.estimator.state_dict()
    assert all(torch.equal(sd[k], sd2[k]) for k in sd)
    jit = torch.jit.load(out["exported"])
    policy = prunner.get_inference_policy(device=penv.device)
    g = torch.Generator().manual_seed(5)
    for i in range(4):                                                                           # raw single frames, the rows of ended envs refilled
        frame = torch.randn(50, 39, generator=g)
        if i:
            dones = (torch.rand(50, generator=g) < 0.3).long()
            policy.reset(dones.to(penv.device)); jit.reset(dones)
        with torch.no_grad():
            want, got = policy(frame.to(penv.device)).cpu(), jit(frame)
        assert want.shape == got.shape == (50, penv.num_actions) and float((got - want).abs().max()) < 1e-6, i


@pytest.mark.parametrize("flags", [("--precision", "bf16"), ("--rnd",), ("--smooth", "both"), ("--state_dependent_std", "--noise_std_type", "log"),
                                   ("--critic_obs_history", "2")], ids=lambda f: f[0].lstrip("-"))
def test_compositions_train_on_the_device(tmp_path, flags):
    """one iteration each beside --estimator: the rows are E columns wider and nothing else changes; the estimator stays fp32 under bf16"""
    env, runner = _make(tmp_path, ("--estimator", *flags))
    est = runner.estimator
    before = [p.detach().clone() for p in est.net.parameters()]
    runner.learn(num_learning_iterations=1)
    assert runner.alg.storage.observations.shape == (8, 64, 42) and est.net.precision == "fp32"
    assert all(not torch.equal(a, b) and bool(torch.isfinite(b).all()) for a, b in zip(before, est.net.parameters()))
    assert all(bool(torch.isfinite(p).all()) for p in runner.alg.actor_critic.parameters())
    assert np.isfinite(_tags(runner)["Loss/estimator"][0])


def test_default_path_runs_nothing_of_it(monkeypatch):
    M = _M()

    def boom(*a, **k):
        raise AssertionError("the estimator ran without --estimator")
    monkeypatch.setattr(M.StateEstimator, "__init__", boom)
    monkeypatch.setattr(M, "est_forward_hip", boom)
    _, plain = _make(None)
    plain.learn(num_learning_iterations=1)
    assert plain.estimator is None and isinstance(plain.alg._graph, torch.cuda.CUDAGraph)
