"""Action-smoothness regularisation on the MI355X (rl/smooth.py, csrc/grx_ppo_smooth.hip): grx_smooth_gather_rows against
numpy, grx_smooth_loss against float64, their argument checks, one minibatch step of every mode against float64 autograd and against the
torch spelling, the captured update against the eager one, and the runner."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import distill_ref as DR
from tests import smooth_ref as R
from tests.test_smooth import _fill, _policy, gather_case, minibatch_check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = list(R.MODES)


def _lib():
    from wiki_grx_gym_amd.rl.fused_loss import load_ppo_library
    return load_ppo_library()


def _P(t):
    return t.data_ptr() if t is not None else None


def _gather(srcs, dsts, idx, mb, N, T, dones, succ, pert, eps, sigma, valid, n=None, widths=None):
    k = len(srcs)
    n = k if n is None else n
    arr = lambda vals: (C.c_void_p * k)(*vals)
    w = (C.c_int * k)(*(widths if widths is not None else [(s if s is not None else d).shape[1] for s, d in zip(srcs, dsts)]))
    return _lib().grx_smooth_gather_rows(n, arr([_P(s) for s in srcs]), arr([_P(d) for d in dsts]), w, _P(idx), mb, N, T, _P(dones), int(succ),
                                         int(pert), _P(eps), sigma, _P(valid), None)


def _bufs(mb, widths, mode, fill=777.0):
    rows = 1 + sum(R.MODES[mode])
    return [torch.full((mb * (rows if t == 0 else 1), w), fill, device=DEV) for t, w in enumerate(widths)], torch.full((mb,), 7, dtype=torch.uint8, device=DEV)


# ---- the gather ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("widths", [(1, 10, 39), (168, 117, 32)])
@pytest.mark.parametrize("mb", [1, 63, 65, 300])
def test_gather_against_numpy(mb, widths):
    """three tensors, T = 4, N = mb, a random idx with a repeat, dones at rate 0.3, every mode: the own and the successor block, valid and
    the plain tensors equal the numpy gather BY VALUE; the perturbed block within 2^-23 (|sigma eps| + |x|), the rounding of a separate
    multiply and add, which bounds the fmaf too; a second call reproduces the first bit for bit.  mb > 1: the case holds a valid row, a row
    masked by a done and a row masked by t = T - 1 (asserted in gather_case); mb = 1: one valid and one invalid index.  Width 168 runs the
    dwordx4 path, and once more from a source that starts 4 bytes off a 16-byte boundary (the dword path)."""
    srcs_np, dones_np, idx_np, eps_np, N, T = gather_case(mb, widths)
    sigma = float(np.float32(0.05))
    if mb == 1:
        dones_np[:] = 0
    offset = torch.zeros(T * N * widths[0] + 1, device=DEV)
    offset[1:].copy_(torch.tensor(srcs_np[0]).reshape(-1))
    variants = [[torch.tensor(s).to(DEV) for s in srcs_np]]
    if widths[0] % 4 == 0:
        variants.append([offset[1:].view(T * N, widths[0])] + variants[0][1:])
        assert variants[1][0].data_ptr() % 16 == 4
    dones, eps = torch.tensor(dones_np).to(DEV), torch.tensor(eps_np).to(DEV)
    for srcs in variants:
        for one_idx in ([idx_np] if mb > 1 else [np.array([0]), np.array([3])]):
            idx = torch.tensor(one_idx).to(DEV)
            for mode in MODES:
                succ, pert = R.MODES[mode]
                dsts, valid = _bufs(mb, widths, mode)
                assert _gather(srcs, dsts, idx, mb, N, T, dones, succ, pert, eps, sigma, valid) == 0
                again, valid2 = _bufs(mb, widths, mode, -1.0)
                assert _gather(srcs, again, idx, mb, N, T, dones, succ, pert, eps, sigma, valid2) == 0
                torch.cuda.synchronize()
                want, v = R.gather_np(srcs_np, one_idx, N, T, dones_np, mode, eps_np, sigma)
                if mb == 1:
                    assert bool(v[0]) == (int(one_idx[0]) == 0)
                if succ:
                    assert np.array_equal(valid.cpu().numpy(), v.astype(np.uint8)) and torch.equal(valid, valid2)
                else:
                    assert bool((valid == 7).all())
                for t, (d, a, wnt) in enumerate(zip(dsts, again, want)):
                    assert torch.equal(d, a)
                    got = d.double().cpu().numpy()
                    keep = mb * (1 + int(succ)) if t == 0 else mb
                    np.testing.assert_array_equal(got[:keep], wnt[:keep])
                    if t == 0 and pert:
                        lim = 2.0 ** -23 * (np.abs(sigma * eps_np.astype(np.float64)) + np.abs(wnt[:mb]))
                        assert (np.abs(got[keep:] - wnt[keep:]) <= lim).all(), (mb, widths, mode, np.abs(got[keep:] - wnt[keep:]).max())


def test_rows_do_not_depend_on_the_minibatch():
    """row r of an mb = 300 call equals an mb = 1 call on that row (its idx, its eps), bit for bit"""
    widths, mb = (168, 117, 32), 300
    srcs_np, dones_np, idx_np, eps_np, N, T = gather_case(mb, widths, seed=9)
    srcs = [torch.tensor(s).to(DEV) for s in srcs_np]
    dones, eps, idx = torch.tensor(dones_np).to(DEV), torch.tensor(eps_np).to(DEV), torch.tensor(idx_np).to(DEV)
    dsts, valid = _bufs(mb, widths, "both", 0.0)
    assert _gather(srcs, dsts, idx, mb, N, T, dones, True, True, eps, 0.05, valid) == 0
    for r in (0, 3, 64, 255, 299):
        one, v1 = _bufs(1, widths, "both", 0.0)
        assert _gather(srcs, one, idx[r:r + 1].contiguous(), 1, N, T, dones, True, True, eps[r:r + 1].contiguous(), 0.05, v1) == 0
        torch.cuda.synchronize()
        assert int(v1[0]) == int(valid[r])
        assert all(torch.equal(dsts[0][k * mb + r], one[0][k]) for k in range(3))
        assert all(torch.equal(d[r], o[0]) for d, o in zip(dsts[1:], one[1:]))


# ---- the loss ------------------------------------------------------------------------------------------------------------------------
def _loss_hip(mu, mode, valid, ct, cs):
    lib = _lib()
    succ, pert = R.MODES[mode]
    mb, A = mu.shape[0] // (1 + succ + pert), mu.shape[1]
    out, d_mu = torch.full((4,), 777.0, device=DEV), torch.full_like(mu, 777.0)
    part = torch.empty(lib.grx_smooth_loss_partials_size(mb, A), device=DEV)
    rc = lib.grx_smooth_loss(mb, A, _P(mu), int(succ), int(pert), _P(valid) if succ else None, ct, cs, _P(out), _P(d_mu), _P(part), None)
    assert rc == 0
    return out, d_mu


@pytest.mark.parametrize("A", [1, 10, 32])
@pytest.mark.parametrize("mb", [1, 33, 257, 1000])
def test_hip_loss_against_float64(mb, A):
    """every mode and mask per case: out[0..2] within max(4 x the error of the torch float32 spelling on the CPU, 8 ulp); the gradient
    within tests/distill_ref.grad_bound; out[3] exact; the temporal gradient of masked rows exactly zero; the NaN rules; twice the same
    bytes (tests/test_distill_gpu.py::test_hip_loss_against_reference's criteria)"""
    from wiki_grx_gym_amd.rl import smooth as S
    ct, cs = float(np.float32(0.7)), float(np.float32(0.3))
    worst = [0.0, 0.0]
    for mode in MODES:
        succ, pert = R.MODES[mode]
        for mask in ("all", "none", "mixed"):
            mu_np, valid_np = R.loss_inputs(mb, A, mode, mask)
            want, want_grad = R.loss_and_grad(mu_np, mode, valid_np, ct, cs)
            mu, valid = torch.tensor(mu_np).to(DEV), torch.tensor(valid_np).to(DEV)
            out, d_mu = _loss_hip(mu, mode, valid, ct, cs)
            again = _loss_hip(mu, mode, valid, ct, cs)
            assert out.cpu().numpy().tobytes() == again[0].cpu().numpy().tobytes() and d_mu.cpu().numpy().tobytes() == again[1].cpu().numpy().tobytes()
            got = out.double().cpu().numpy()
            assert got[3] == want[3]
            total, terms = S.smooth_loss_torch(torch.tensor(mu_np), succ, pert, torch.tensor(valid_np), ct, cs)   # the fp32 spelling on the CPU
            torch32 = np.array([float(terms[0]), float(terms[1]), float(total)])
            for k in range(3):
                ulp = float(np.spacing(np.float32(want[k])))
                err, torch_err = abs(got[k] - want[k]), abs(torch32[k] - want[k])
                worst[0] = max(worst[0], err / max(4 * torch_err, 8 * ulp))
                assert err <= max(4 * torch_err, 8 * ulp), (mode, mask, k, err, torch_err, ulp)
            grad_err = np.abs(d_mu.double().cpu().numpy() - want_grad)
            worst[1] = max(worst[1], float((grad_err / DR.grad_bound(want_grad)).max()))
            assert (grad_err <= DR.grad_bound(want_grad)).all(), (mode, mask, float((grad_err / DR.grad_bound(want_grad)).max()))
            if succ:
                masked = torch.tensor(valid_np == 0).to(DEV)
                assert not d_mu[mb:2 * mb][masked].any()
                if not pert:
                    assert not d_mu[:mb][masked].any()
            if succ and mask == "none":
                assert got[0] == 0.0 and bool(torch.isfinite(out).all()) and bool(torch.isfinite(d_mu).all())
            if succ and mask == "mixed" and mb > 1:
                poisoned = mu.clone()
                poisoned[mb + int(np.flatnonzero(valid_np == 0)[0])] = float("nan")            # a masked pair's successor
                p_out, p_grad = _loss_hip(poisoned, mode, valid, ct, cs)
                assert torch.equal(p_out, out) and torch.equal(p_grad, d_mu)
                poisoned = mu.clone()
                poisoned[mb + int(np.flatnonzero(valid_np != 0)[0]), A - 1] = float("nan")     # a pair that counts
                p_out, _ = _loss_hip(poisoned, mode, valid, ct, cs)
                assert bool(torch.isnan(p_out[0])) and bool(torch.isnan(p_out[2])) and float(p_out[3]) == want[3]
            # ... and through autograd, as the update uses it
            mg = mu.clone().requires_grad_(True)
            loss, lts = S.smooth_loss(mg, succ, pert, valid, ct, cs)
            assert loss.shape == () and isinstance(loss.grad_fn, torch.autograd.function.BackwardCFunction) and not lts.requires_grad
            (2.0 * loss).backward()
            assert torch.equal(loss.detach(), out[2]) and torch.equal(lts, out[:2]) and torch.equal(mg.grad, 2.0 * d_mu)
    print(f"grx_smooth_loss {mb} x {A}: worst error / allowance {worst[0]:.3f}, worst gradient error / grad_bound {worst[1]:.3f}")


def test_invalid_arguments_leave_the_outputs_untouched():
    mb, widths, N, T = 8, (8, 39), 8, 4
    srcs_np, dones_np, idx_np, eps_np, _, _ = gather_case(mb, widths)
    srcs = [torch.tensor(s).to(DEV) for s in srcs_np]
    dones, eps, idx = torch.tensor(dones_np).to(DEV), torch.tensor(eps_np).to(DEV), torch.tensor(idx_np).to(DEV)
    dsts, valid = _bufs(mb, widths, "both")
    base = dict(srcs=srcs, dsts=dsts, idx=idx, mb=mb, N=N, T=T, dones=dones, succ=True, pert=True, eps=eps, sigma=0.05, valid=valid)
    call = lambda **kw: _gather(**{**base, **kw})
    assert call(mb=0) < 0 and call(mb=-3) < 0 and call(N=0) < 0 and call(T=0) < 0
    assert call(n=0) < 0
    assert _gather(**{**base, **dict(srcs=[srcs[1]] * 13, dsts=[dsts[1]] * 13)}) < 0                    # above GRX_PPO_GATHER_MAX
    assert call(widths=[0, 39]) < 0 and call(widths=[8, -1]) < 0
    assert call(srcs=[None, srcs[1]]) < 0 and call(dsts=[dsts[0], None]) < 0 and call(idx=None) < 0
    assert call(eps=None) < 0 and call(dones=None) < 0 and call(valid=None) < 0
    assert call(sigma=-0.1) < 0 and call(sigma=float("nan")) < 0 and call(sigma=float("inf")) < 0
    whole = torch.full((T * N + 3 * mb, 8), 777.0, device=DEV)                                            # dst[0] inside / behind src[0]
    assert call(srcs=[whole[:T * N], srcs[1]], dsts=[whole[mb:4 * mb], dsts[1]]) < 0
    assert call(srcs=[whole[:T * N], srcs[1]], dsts=[whole[T * N - 1:T * N - 1 + 3 * mb], dsts[1]]) < 0
    lib = _lib()
    one = (C.c_void_p * 1)(srcs[0].data_ptr())
    w1 = (C.c_int * 1)(8)
    tail = (_P(idx), mb, N, T, _P(dones), 1, 1, _P(eps), 0.05, _P(valid), None)
    assert lib.grx_smooth_gather_rows(1, None, one, w1, *tail) < 0 and lib.grx_smooth_gather_rows(1, one, None, w1, *tail) < 0
    assert lib.grx_smooth_gather_rows(1, one, one, None, *tail) < 0

    mu = torch.randn(3 * mb, 10, device=DEV)
    out, d_mu, part = torch.full((4,), 777.0, device=DEV), torch.full((3 * mb, 10), 777.0, device=DEV), torch.full((9,), 777.0, device=DEV)
    assert lib.grx_smooth_loss_partials_size(mb, 10) == 6 and lib.grx_smooth_loss_partials_size(0, 10) == 0
    assert lib.grx_smooth_loss_partials_size(mb, 257) == 0 and lib.grx_smooth_loss_partials_size(2 ** 24, 1) == 0
    good = (mb, 10, _P(mu), 1, 1, _P(valid), 0.5, 0.5, _P(out), _P(d_mu), _P(part), None)
    for pos, bad in ((0, 0), (0, 2 ** 24), (1, 0), (1, 257), (2, None), (5, None), (8, None), (9, None), (10, None), (10, _P(part) + 4), (3, 0)):
        args = list(good)
        args[pos] = bad
        if pos == 3:
            args[4] = 0                                                                                   # neither block: no loss
        assert lib.grx_smooth_loss(*args) < 0, (pos, bad)
    assert lib.grx_smooth_loss(2 ** 23, 200, *good[2:]) < 0                                                # R mb A >= 2^31
    torch.cuda.synchronize()
    assert all(bool((d == 777.0).all()) for d in dsts + [out, d_mu, part, whole]) and bool((valid == 7).all())
    assert call() == 0 and lib.grx_smooth_loss(*good) == 0                                                # ... and the valid calls do write
    torch.cuda.synchronize()
    assert not any(bool((d == 777.0).any()) for d in dsts + [out, d_mu]) and not bool((valid == 7).any())


# ---- one minibatch step through PPO ------------------------------------------------------------------------------------------------------
def _setup(mode, monkeypatch, graph="1", seed=5, **kw):
    from wiki_grx_gym_amd.rl.ppo import PPO
    monkeypatch.setenv("GRX_PPO_GRAPH", graph)
    torch.manual_seed(seed)
    alg = PPO(_policy(), num_learning_epochs=2, num_mini_batches=4, clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.01, schedule="adaptive",
              desired_kl=0.01, learning_rate=1e-3, device=DEV, smooth=mode, smooth_temporal_coef=0.7, smooth_spatial_coef=0.9, smooth_sigma=0.1, **kw)
    alg.init_storage(64, 8)
    _fill(alg, 8, 64, torch.Generator().manual_seed(seed + 1))
    return alg


@pytest.mark.parametrize("mode", MODES)
def test_minibatch_gradients_match_float64_and_the_torch_spelling(mode, monkeypatch):
    """One minibatch (64 of 512 rows): all parameter gradients against float64 autograd of tests/smooth_ref within 1e-4 max |g_ref| per
    tensor (the bound of test_minibatch_parameter_gradients_match_float64), the same eps fed to both, with the HIP gather and loss and with
    GRX_SMOOTH_FUSED=0; the two against each other within the same bound."""
    alg = _setup(mode, monkeypatch, graph="0")
    with alg._blas_for_update():
        results, ref = minibatch_check(alg, mode, DEV, fused_values=("1", "0"), monkeypatch=monkeypatch)
    for a, b, want in zip(results["1"], results["0"], ref["grads"]):
        assert float((a - b).abs().max()) <= 1e-4 * float(want.abs().max())


def test_captured_update_equals_the_eager_one(monkeypatch):
    """--smooth both: two updates under GRX_PPO_GRAPH=1 and GRX_PPO_GRAPH=0 from the same state, the device generator re-seeded before
    each, give bit-identical parameters, the same learning rate and the same mean smoothness losses"""
    got = {}
    for graph in ("1", "0"):
        alg = _setup("both", monkeypatch, graph=graph)
        assert alg._use_graph == (graph == "1")
        torch.manual_seed(77)
        stats = [alg.update(), alg.update()]
        torch.cuda.synchronize()
        if graph == "1":
            assert isinstance(alg._graph, torch.cuda.CUDAGraph) and type(alg._gather.gather).__name__ == "SmoothGather"
            assert alg._static[0].shape[0] == 3 * 128 and alg._static[1].shape[0] == 128 and alg._smooth_valid.shape == (128,)
        got[graph] = ([p.detach().clone() for p in alg.actor_critic.parameters()], stats, alg.learning_rate, alg.mean_smooth_temporal,
                      alg.mean_smooth_spatial)
    for a, b in zip(got["1"][0], got["0"][0]):
        assert torch.equal(a, b)
    assert got["1"][1:] == got["0"][1:] and got["1"][3] > 0 and got["1"][4] > 0


# ---- the runner ------------------------------------------------------------------------------------------------------------------------
def _make(tmp_path, flags=(), steps=8, num_envs=64):
    from wiki_grx_gym_amd.envs import GR1T1Cfg, GR1T1CfgPPO
    from wiki_grx_gym_amd.utils import get_args, task_registry
    args = get_args(["--task", "GR1T1", "--headless", "--num_envs", str(num_envs), "--seed", "3", *flags])
    env, _ = task_registry.make_env("GR1T1", args=args, env_cfg=GR1T1Cfg())
    tcfg = GR1T1CfgPPO()
    tcfg.runner.num_steps_per_env = steps
    tcfg.algorithm.num_mini_batches = 4
    runner, _ = task_registry.make_alg_runner(env, name=None, args=args, train_cfg=tcfg, log_root=str(tmp_path) if tmp_path else None)
    return env, runner


def _tags(runner):
    return {line.split('"tag": "')[1].split('"')[0]: float(line.split('"value": ')[1].split(",")[0]) for line in open(os.path.join(runner.log_dir, "scalars.jsonl"))}


DEFAULT_KEYS = {"model_state_dict", "optimizer_state_dict", "iter", "infos"}


@pytest.mark.parametrize("flags", [("--smooth", "temporal"), ("--smooth", "spatial"), ("--smooth", "both"),
                                   ("--smooth", "both", "--empirical_normalization", "--obs_history", "3"),
                                   ("--smooth", "both", "--precision", "bf16")], ids=lambda f: "_".join(x.strip("-") for x in f))
def test_runner_trains_with_smoothness(tmp_path, flags):
    env, runner = _make(tmp_path, flags)
    alg = runner.alg
    before = [p.detach().clone() for p in alg.actor_critic.parameters()]
    runner.learn(num_learning_iterations=2)
    assert type(alg._gather.gather).__name__ == "SmoothGather" and isinstance(alg._graph, torch.cuda.CUDAGraph)
    rows = {"temporal": 2, "spatial": 2, "both": 3}[flags[1]]
    assert alg._static[0].shape == (rows * 128, 39 * (3 if "--obs_history" in flags else 1)) and alg._static[2].shape[0] == 128
    assert all(not torch.equal(a, b) and bool(torch.isfinite(b).all()) for a, b in zip(before, alg.actor_critic.parameters()))
    tags = _tags(runner)
    assert all(np.isfinite(tags[k]) for k in ("Loss/smooth_temporal", "Loss/smooth_spatial", "Loss/value_function", "Loss/surrogate", "Loss/kl"))
    assert (tags["Loss/smooth_temporal"] > 0) == (flags[1] != "spatial") and (tags["Loss/smooth_spatial"] > 0) == (flags[1] != "temporal")
    want = DEFAULT_KEYS | ({"obs_norm_state_dict", "critic_obs_norm_state_dict"} if "--empirical_normalization" in flags else set()) \
        | ({"obs_history"} if "--obs_history" in flags else set())
    assert set(torch.load(os.path.join(runner.log_dir, "model_2.pt"), weights_only=False)) == want        # the key set of a run without the flag


def test_play_on_a_smooth_run_and_the_default_path(tmp_path):
    from wiki_grx_gym_amd.scripts.play import play
    from wiki_grx_gym_amd.utils import get_args
    _, runner = _make(tmp_path, ("--smooth", "both"))
    runner.learn(num_learning_iterations=1)
    out = play(get_args(["--task", "GR1T1", "--headless", "--seed", "3"]), steps=20, log_root=str(tmp_path))     # play.py knows nothing of it
    prunner, penv = out["runner"], out["env"]
    assert len(open(out["states"]).readlines()) == 20 and prunner.alg.smooth is None
    jit = torch.jit.load(out["exported"])
    x = torch.randn(64, 39)
    want = prunner.algorithm.actor_critic.actor(x.to(penv.device)).cpu()
    assert (jit(x) - want).abs().max() < 1e-6                                                                # tests/test_play_gpu.py's tolerance
    trained = runner.alg.actor_critic.state_dict()
    assert all(torch.equal(v, prunner.alg.actor_critic.state_dict()[k]) for k, v in trained.items() if k != "std")
    _, plain = _make(tmp_path / "plain")
    plain.learn(num_learning_iterations=1)
    alg = plain.alg
    assert type(alg._gather).__name__ == "RowGather" and alg.smooth is None and alg._static[0].shape[0] == 64 * 8 // 4
    assert not [k for k, v in vars(alg).items() if "smooth" in k and v is not None and not isinstance(v, float)]
    assert set(torch.load(os.path.join(plain.log_dir, "model_1.pt"), weights_only=False)) == DEFAULT_KEYS
    assert "Loss/smooth_temporal" not in _tags(plain)
