"""LayerNorm hidden layers (rl/modules.py MLP(layer_norm=True), include/grx_ppo_ln.h) on the MI355X: grx_ln_elu_forward and
grx_ln_elu_backward against the float64 reference (tests/ln_ref.py) and, for the three batch sums, against grx_ppo_colsum bit for bit; a whole
network against its float64 copy; the captured minibatch step and policy step against the eager ones; the compositions; three iterations
through the runner with checkpoint, play and export.

Tolerances of the comparisons with float64: the rule of tests/ln_ref.py (four times the fp32 torch spelling's deviation, which counts as at
least half an fp32 ulp of the reference; column sums relative to the sum of their terms' magnitudes, at every shape).  The arrays with one
row per batch row (y, mean, rstd, dz) are judged twice per shape: the two special rows (the constant one and the one of mean 1e4, whose
deviations are a thousand times the others') and the ordinary rows on their own.  Both deviations are measured here and printed;
GRX_LN_PARITY_OUT=<path> writes their maxima as JSON (profiles/layer_norm_parity.json)."""
import copy
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import ln_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_PARITY = {}


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def _np(t):
    return t.detach().cpu().double().numpy()


def _hold(failures, case, name, got, spelling, ref, scale=None):
    """the tolerance rule for one quantity of one case: records both deviations, notes a failure"""
    ok, dh, dt = R.within(_np(got) if torch.is_tensor(got) else got, _np(spelling) if torch.is_tensor(spelling) else spelling, ref, scale)
    w = _PARITY.setdefault(name, {"torch": 0.0, "hip": 0.0, "ratio": 0.0})
    w["torch"], w["hip"], w["ratio"] = max(w["torch"], dt), max(w["hip"], dh), max(w["ratio"], dh / dt if dt > 0 else (0.0 if dh == 0 else float("inf")))
    print(f"{case} {name}: hip {dh:.3e} torch {dt:.3e}")
    if not ok:
        failures.append((case, name, dh, dt))


def _hold_rows(failures, case, name, got, spelling, ref):
    """_hold for an array with one row per batch row: the special rows 0 and 1 (tests/ln_ref.py inputs) and the ordinary rows apart, so
    that the special rows' large deviations do not set the ordinary rows' bound"""
    got, spelling, ref = _np(got), _np(spelling), np.asarray(ref)
    _hold(failures, case, name, got[:2], spelling[:2], ref[:2])
    if ref.shape[0] > 2:
        _hold(failures, case, name + "_ordinary_rows", got[2:], spelling[2:], ref[2:])


def _write_parity(failures):
    out = os.environ.get("GRX_LN_PARITY_OUT")
    if out:
        with open(out, "w") as f:
            json.dump({"rows": list(R.ROWS), "cols": list(R.COLS), "bound": "hip <= 4 x max(torch, half an fp32 ulp), per shape; column sums "
                       "relative to the sum of the terms' magnitudes", "max_deviation_from_float64": _PARITY,
                       "failures": [list(map(str, c)) for c in failures]}, f, indent=1)


def _torch_stats(z):
    """the torch fp32 spelling of the rows' mean and 1 / std"""
    m = z.mean(-1, keepdim=True)
    return m[:, 0], (1.0 / torch.sqrt(((z - m) * (z - m)).mean(-1, keepdim=True) + R.EPS))[:, 0]


@pytest.mark.parametrize("cols", R.COLS)
def test_forward_against_float64(cols):
    from wiki_grx_gym_amd.rl.fused_loss import ln_elu_forward
    failures = []
    for rows in R.ROWS:
        z, gamma, beta, _ = R.inputs(rows, cols)
        ref_y, ref_m, ref_s, _ = R.forward(z, gamma, beta)
        if cols > 1 and rows > 2:
            assert (ref_y > 0.1).any() and (ref_y < -0.1).any()                              # both of ELU's branches
        dz, dg, db = _dev(z, gamma, beta)
        y, mean, rstd = ln_elu_forward(dz, dg, db, R.EPS)
        y_inf, none_m, none_s = ln_elu_forward(dz, dg, db, R.EPS, stats=False)
        assert none_m is None and none_s is None and torch.equal(y, y_inf), (rows, cols)     # the same bits without mean / rstd
        y2, mean2, rstd2 = ln_elu_forward(dz, dg, db, R.EPS)
        assert torch.equal(y, y2) and torch.equal(mean, mean2) and torch.equal(rstd, rstd2)  # ... and between two calls
        assert bool(torch.isfinite(y).all()) and float(rstd[0]) > 300.0                      # the constant row: 1 / sqrt(eps)
        t_y = F.elu(F.layer_norm(dz, (cols,), dg, db, R.EPS))
        t_m, t_s = _torch_stats(dz)
        case = f"fwd {rows}x{cols}"
        _hold_rows(failures, case, "y", y, t_y, ref_y)
        _hold_rows(failures, case, "mean", mean, t_m, ref_m)
        _hold_rows(failures, case, "rstd", rstd, t_s, ref_s)
    _write_parity(failures)
    assert not failures, failures


@pytest.mark.parametrize("cols", R.COLS)
def test_backward_against_colsum_and_float64(cols):
    from wiki_grx_gym_amd.rl.fused_loss import colsum, ln_elu_backward, ln_elu_forward
    from wiki_grx_gym_amd.rl.modules import ln_elu_backward_torch
    failures = []
    for rows in R.ROWS:
        z, gamma, beta, dy = R.inputs(rows, cols)
        ref = R.backward(dy, z, gamma, beta)
        dz_, dg, db, ddy = _dev(z, gamma, beta, dy)
        y, mean, rstd = ln_elu_forward(dz_, dg, db, R.EPS)
        dz, dgamma, dbeta, dbias = ln_elu_backward(ddy, y, dz_, mean, rstd, dg)
        again = ln_elu_backward(ddy, y, dz_, mean, rstd, dg)
        assert all(torch.equal(a, b) for a, b in zip((dz, dgamma, dbeta, dbias), again)), (rows, cols)          # no atomics: the same bits
        # the three batch sums are grx_ppo_colsum's of g, g * xhat (from the kernel's own mean / rstd) and the returned dz, bit for bit
        g = ddy * torch.where(y > 0, torch.ones_like(y), y + 1.0)
        xh = (dz_ - mean[:, None]) * rstd[:, None]
        assert torch.equal(dbeta, colsum(g)), (rows, cols, "dbeta")
        assert torch.equal(dgamma, colsum(g * xh)), (rows, cols, "dgamma")
        assert torch.equal(dbias, colsum(dz)), (rows, cols, "dbias")
        if cols == 1:
            assert float(dz.abs().max()) == 0.0 and float(dbias.abs().max()) == 0.0 and float(dgamma.abs().max()) == 0.0
        t_y = F.elu(F.layer_norm(dz_, (cols,), dg, db, R.EPS))
        t_dz, t_dgamma, t_dbeta, t_dbias = ln_elu_backward_torch(ddy, t_y, dz_, dg, R.EPS)
        case = f"bwd {rows}x{cols}"
        _hold_rows(failures, case, "dz", dz, t_dz, ref["dz"])
        for name, got, spelling in (("dbeta", dbeta, t_dbeta), ("dgamma", dgamma, t_dgamma), ("dbias", dbias, t_dbias)):
            _hold(failures, case, name, got, spelling, ref[name], ref["scale"][name])
        if rows == 1 and cols > 1:
            # a figure, not a check: the header's formulas evaluated in float64 on the fp32 tensors the entry point is given (dy, y, z, mean,
            # rstd, gamma), i.e. what NO rounding inside the kernel would leave of dbias' deviation -- the share of the inputs' own rounding
            y64, g64 = _np(y), np.asarray(gamma, dtype=np.float64)
            q64 = _np(ddy) * np.where(y64 > 0, 1.0, y64 + 1.0) * g64
            xh64 = (_np(dz_) - _np(mean)[:, None]) * _np(rstd)[:, None]
            ideal = _np(rstd)[:, None] * ((q64 - q64.mean(1, keepdims=True)) - xh64 * (q64 * xh64).mean(1, keepdims=True))
            d = R.deviation(ideal.sum(0), ref["dbias"], ref["scale"]["dbias"])
            w = _PARITY.setdefault("dbias_rows1_float64_on_the_fp32_inputs", {})
            w[f"1x{cols}"] = d
            print(f"{case} dbias, float64 arithmetic on the entry point's fp32 inputs: {d:.3e}")
    _write_parity(failures)
    assert not failures, failures


def test_a_row_does_not_depend_on_the_batch():
    from wiki_grx_gym_amd.rl.fused_loss import ln_elu_backward, ln_elu_forward
    z, gamma, beta, dy = _dev(*R.inputs(513, 130))
    y, mean, rstd = ln_elu_forward(z, gamma, beta, R.EPS)
    dz = ln_elu_backward(dy, y, z, mean, rstd, gamma)[0]
    sl = slice(250, 263)
    y1, m1, s1 = ln_elu_forward(z[sl].contiguous(), gamma, beta, R.EPS)
    assert torch.equal(y1, y[sl]) and torch.equal(m1, mean[sl]) and torch.equal(s1, rstd[sl])
    assert torch.equal(ln_elu_backward(dy[sl].contiguous(), y1, z[sl].contiguous(), m1, s1, gamma)[0], dz[sl])


class _rocblas:
    """the update's BLAS preference (PPO._blas_for_update)"""

    def __enter__(self):
        self.prev = torch.backends.cuda.preferred_blas_library()
        torch.backends.cuda.preferred_blas_library("cublas")

    def __exit__(self, *exc):
        torch.backends.cuda.preferred_blas_library(self.prev)


@pytest.mark.parametrize("fused", ["1", "0"])
def test_network_against_its_float64_copy(fused, monkeypatch):
    """MLP(layer_norm=True) [24, 130, 64, 10] at 257 rows on the training path: output and every parameter gradient.  The torch spelling
    the rule measures against is the plain nn.Sequential of the same modules under torch's autograd, on the device in fp32."""
    from wiki_grx_gym_amd.rl.modules import MLP
    monkeypatch.setenv("GRX_LN_FUSED", fused)
    torch.manual_seed(2)
    net = MLP(24, 10, [130, 64], "elu", layer_norm=True)
    with torch.no_grad():
        for m in net.model:
            if isinstance(m, nn.LayerNorm):
                m.weight.uniform_(0.5, 1.5); m.bias.normal_(0.0, 0.3)
    ref = copy.deepcopy(net.model).double()
    x, w = torch.randn(257, 24), torch.randn(257, 10)
    out64 = ref(x.double())
    (out64 * w.double()).sum().backward()
    net = net.to(DEV)
    xd, wd = x.to(DEV), w.to(DEV)
    failures = []
    with _rocblas():
        assert torch.is_grad_enabled()
        out = net(xd)                                                                        # (MLP.forward -> _forward_train -> _TrainLinearLNELU)
        assert type(out.grad_fn.next_functions[0][0]).__name__ == "_TrainLinearLNELUBackward"         # (behind the output layer's _TrainLinear)
        (out * wd).sum().backward()
        got = [p.grad.clone() for p in net.parameters()]
        net.zero_grad(set_to_none=True)
        plain = net.model(xd)
        (plain * wd).sum().backward()
        spelled = [p.grad.clone() for p in net.parameters()]
    case = f"net GRX_LN_FUSED={fused}"
    _hold(failures, case, "net_output", out, plain, out64.detach().numpy())
    for (name, _), g, s, p64 in zip(net.named_parameters(), got, spelled, ref.parameters()):
        _hold(failures, case, "net_d_" + name, g, s, p64.grad.numpy())
    _write_parity(failures)
    assert not failures, failures


# ---- PPO -------------------------------------------------------------------------------------------------------------------------------
def _policy(**kw):
    from wiki_grx_gym_amd.rl.modules import ActorCriticMLP
    return ActorCriticMLP(39, 168, 10, actor_hidden_dims=[130, 64], critic_hidden_dims=[64, 32], activation="elu", init_noise_std=0.4,
                          layer_norm=True, **kw)


def _synthetic_rollout(alg, N, T, g):
    with torch.inference_mode():
        for _ in range(T):
            o = torch.randn(N, 39, device=DEV, generator=g); c = torch.randn(N, 168, device=DEV, generator=g)
            alg.act(o, c)
            r = torch.randn(N, device=DEV, generator=g) * 0.1
            d = torch.rand(N, device=DEV, generator=g) < 0.05
            alg.process_env_step(r, d, {"time_outs": torch.zeros(N, device=DEV, dtype=torch.bool)})
        alg.compute_returns(c)


def test_captured_step_equals_eager_step_with_rollouts_in_between(monkeypatch):
    """tests/test_ppo_gpu.py's pattern: updates (2 epochs x 4 minibatches, 64 envs x 8 steps) with synthetic rollouts -- eager GPU work, the
    captured policy step, fresh storage contents -- between them, under GRX_PPO_GRAPH=1 and 0: parameters and Adam state bit for bit"""
    from wiki_grx_gym_amd.rl.ppo import PPO
    N, T = 64, 8
    res = {}
    for graph in ("1", "0"):
        monkeypatch.setenv("GRX_PPO_GRAPH", graph)
        torch.manual_seed(0)
        alg = PPO(_policy(), num_learning_epochs=2, num_mini_batches=4, clip_param=0.2, entropy_coef=0.01, learning_rate=1e-3,
                  schedule="adaptive", desired_kl=0.01, device=DEV)
        assert alg._use_graph == (graph == "1") and alg._layer_norm
        alg.init_storage(N, T)
        g = torch.Generator(device=DEV).manual_seed(1)
        snaps = []
        for u in range(3):
            torch.manual_seed(50 + u)
            _synthetic_rollout(alg, N, T, g)
            out = alg.update()
            alg.clear_storage()
            assert all(np.isfinite(v) and abs(v) > 1e-7 for v in out)
            state = [t.detach().clone() for p in alg.actor_critic.parameters() for t in
                     (p, alg.optimizer.state[p]["exp_avg"], alg.optimizer.state[p]["exp_avg_sq"], alg.optimizer.state[p]["step"])]
            snaps.append((state, out, alg.learning_rate))
        if graph == "1":
            assert isinstance(alg._graph, torch.cuda.CUDAGraph) and alg._act_graph is not None and alg._act_fused    # both hold the LayerNorm network
        res[graph] = snaps
    for u in range(3):
        (a, oa, la), (b, ob, lb) = res["1"][u], res["0"][u]
        assert len(a) == len(b) == 4 * 21 and all(torch.equal(s, t) for s, t in zip(a, b)), u
        assert oa == ob and la == lb


def test_captured_policy_step_against_the_eager_module():
    """mu and the value of PPO.act's captured policy step (grx_mlp_layer without ELU, grx_ln_elu_forward without mean / rstd, the fused
    head) and the eager torch modules, both against a float64 copy on the same input"""
    from wiki_grx_gym_amd.rl.ppo import PPO
    torch.manual_seed(0)
    ac = _policy()
    with torch.no_grad():
        for m in ac.modules():
            if isinstance(m, nn.LayerNorm):
                m.weight.uniform_(0.5, 1.5); m.bias.normal_(0.0, 0.3)
    alg = PPO(ac, device=DEV)
    alg.init_storage(257, 2)
    ref = copy.deepcopy(ac).double().cpu()
    g = torch.Generator(device=DEV).manual_seed(1)
    o, c = torch.randn(257, 39, device=DEV, generator=g), torch.randn(257, 168, device=DEV, generator=g)
    with torch.inference_mode():
        alg.act(o, c)
        t = alg.transition
        mu, v = t.action_mean.clone(), t.values.clone()
        mu_e, v_e = ac.actor(o), ac.critic(c)
        mu64, v64 = ref.actor(o.cpu().double()), ref.critic(c.cpu().double())
    assert alg._act_graph is not None and alg._act_fused
    failures = []
    _hold(failures, "act 257", "act_mu", mu, mu_e, mu64.numpy())
    _hold(failures, "act 257", "act_value", v.reshape(-1), v_e.reshape(-1), v64.reshape(-1).numpy())
    _write_parity(failures)
    assert not failures, failures


def test_bf16_is_refused():
    from wiki_grx_gym_amd.rl.ppo import PPO
    with pytest.raises(ValueError, match="--precision bf16") as info:
        PPO(_policy(), device=DEV, precision="bf16")
    assert "--layer_norm" in str(info.value)


# ---- the runner ------------------------------------------------------------------------------------------------------------------------
def _make(tmp_path, flags=(), steps=8, num_envs=64, epochs=2):
    from wiki_grx_gym_amd.envs import GR1T1Cfg, GR1T1CfgPPO
    from wiki_grx_gym_amd.utils import get_args, task_registry
    args = get_args(["--task", "GR1T1", "--headless", "--num_envs", str(num_envs), "--seed", "3", *flags])
    env, _ = task_registry.make_env("GR1T1", args=args, env_cfg=GR1T1Cfg())
    tcfg = GR1T1CfgPPO()
    tcfg.runner.num_steps_per_env = steps
    tcfg.algorithm.num_mini_batches, tcfg.algorithm.num_learning_epochs = 4, epochs
    runner, _ = task_registry.make_alg_runner(env, name=None, args=args, train_cfg=tcfg, log_root=str(tmp_path) if tmp_path else None)
    return env, runner


def _tags(runner):
    return {line.split('"tag": "')[1].split('"')[0]: float(line.split('"value": ')[1].split(",")[0]) for line in open(os.path.join(runner.log_dir, "scalars.jsonl"))}


# every flag the runner accepts together with --layer_norm appears in at least one case (README)
COMPOSITIONS = [
    ("--empirical_normalization", "--obs_history", "3", "--value_norm", "popart", "--noise_std_type", "log"),
    ("--symmetry", "both"),
    ("--smooth", "both"),
    ("--state_dependent_std",),
    ("--privileged_actor", "--critic_obs_history", "2", "--value_norm", "running"),
    ("--rnd", "--estimator"),
]


@pytest.mark.parametrize("flags", COMPOSITIONS, ids=lambda f: "_".join(x.strip("-") for x in f))
def test_compositions_captured_against_eager(tmp_path, flags, monkeypatch):
    """one iteration through the runner (64 envs x 8 steps, 2 epochs x 4 minibatches) under GRX_PPO_GRAPH=1 and 0 from the same seed:
    parameters and Adam state bit for bit, finite losses"""
    got = {}
    for graph in ("1", "0"):
        monkeypatch.setenv("GRX_PPO_GRAPH", graph)
        _, runner = _make(tmp_path / graph, ("--layer_norm",) + flags)
        alg = runner.alg
        assert alg._layer_norm and alg._use_graph == (graph == "1")
        before = [p.detach().clone() for p in alg.actor_critic.parameters()]
        runner.learn(num_learning_iterations=1)
        torch.cuda.synchronize()
        if graph == "1":
            assert isinstance(alg._graph, torch.cuda.CUDAGraph) and alg._act_fused
        assert all(not torch.equal(a, b) and bool(torch.isfinite(b).all()) for a, b in zip(before, alg.actor_critic.parameters()))
        tags = _tags(runner)
        assert all(np.isfinite(tags[k]) for k in ("Loss/value_function", "Loss/surrogate", "Loss/kl"))
        got[graph] = [t.detach().clone() for p in alg.actor_critic.parameters() for t in
                      (p, alg.optimizer.state[p]["exp_avg"], alg.optimizer.state[p]["exp_avg_sq"])]
    assert len(got["1"]) == len(got["0"]) and all(torch.equal(a, b) for a, b in zip(got["1"], got["0"]))


def test_end_to_end_train_checkpoint_play_export(tmp_path, monkeypatch):
    """three iterations at 256 envs with --layer_norm, a checkpoint, play for 20 steps; the exported module on the CPU and the device
    policy (the fused inference forward) against a float64 evaluation of the same weights on the same frames"""
    from wiki_grx_gym_amd.rl.fused_loss import mlp_forward
    from wiki_grx_gym_amd.scripts.play import play
    from wiki_grx_gym_amd.utils import get_args, task_registry
    # (play() takes the registered config instance, which the flag writes to: undone when the test ends)
    monkeypatch.setattr(task_registry.train_cfgs["GR1T1"].policy, "layer_norm", False, raising=False)
    _, runner = _make(tmp_path, ("--layer_norm",), steps=8, num_envs=256)
    runner.learn(num_learning_iterations=3)
    ck = torch.load(os.path.join(runner.log_dir, "model_3.pt"), weights_only=False)
    assert ck["layer_norm"] == {"enabled": True, "eps": 1e-5}
    with pytest.raises(ValueError, match="--layer_norm"):                                                # play needs the same flag
        play(get_args(["--task", "GR1T1", "--headless", "--seed", "3"]), steps=1, log_root=str(tmp_path))
    out = play(get_args(["--task", "GR1T1", "--headless", "--seed", "3", "--layer_norm"]), steps=20, log_root=str(tmp_path))
    prunner, penv = out["runner"], out["env"]
    assert len(open(out["states"]).readlines()) == 20
    trained, loaded = runner.alg.actor_critic.state_dict(), prunner.alg.actor_critic.state_dict()
    assert all(torch.equal(v, loaded[k]) for k, v in trained.items() if k != "std")
    frames = penv.get_observations().detach().clone()                                                    # the frames play ended on
    actor = prunner.alg.actor_critic.actor
    ref = copy.deepcopy(actor).double().cpu()
    jit = torch.jit.load(out["exported"])
    with torch.no_grad():
        want = ref(frames.cpu().double()).numpy()
        spelled = actor.model(frames)                                                                    # torch's fp32 modules on the device
        device_policy = mlp_forward(actor, frames)
        exported = jit(frames.cpu())
        assert torch.equal(prunner.get_inference_policy(device=penv.device)(frames), spelled)
    failures = []
    _hold(failures, "play", "play_device_policy", device_policy, spelled, want)
    _hold(failures, "play", "play_exported_cpu", exported, spelled, want)
    _write_parity(failures)
    assert not failures, failures
