"""The Lipschitz gradient penalty (rl/grad_penalty.py, include/grx_ppo_gp.h) on the MI355X: every entry point against its
torch spelling, the autograd function against torch's float64 double backward, the captured minibatch step against the eager one, and two
iterations through the runner with play and export."""
import os

import numpy as np
import pytest
import torch

from tests import grad_penalty_ref as R
from tests.test_grad_penalty import TOL, _fill, _policy, assert_against_ref, minibatch_check, run_function

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BATCHES = [1, 63, 64, 65, 257, 513]       # around a wave, and around the 256-row slabs of the column sums (one, two and three slabs)
WIDTHS = [1, 10, 16, 39, 128]             # below, at no multiple of and above a wave of columns; odd counts take the dword path


def _inputs(B, n, seed=0):
    """fp32 CPU tensors of one [B, n] case; y holds positive, negative and exactly zero outputs (ELU's range: above -1)"""
    g = torch.Generator().manual_seed(100 * B + n + seed)
    r = lambda *s: torch.randn(*s, generator=g)
    y = torch.where(r(B, n) > 0, r(B, n).abs(), -torch.rand(B, n, generator=g) * 0.999)
    y.view(-1)[::3] = 0.0
    return {"y": y, "g": r(B, n), "hbar": r(B, n), "dY": r(B, n), "a": r(B, n), "mu": r(B, n), "ubar": r(B, n), "dmu": r(B, n),
            "sigma": 0.3 + torch.rand(n, generator=g)}


@pytest.mark.parametrize("n", WIDTHS)
def test_entry_points_against_their_torch_spelling(n):
    """Element-wise outputs equal the torch spelling bit for bit -- the spelling evaluated on the CPU, where every operation is one IEEE
    rounding, which is what the header promises of the kernels.  Column sums and P are within 1e-6 of float64, relative to the same sum with
    every term replaced by its magnitude (tests/ppo_ref.py's `scale`: what the rounding of a sum is proportional to -- the terms of a column
    have both signs and may cancel, at n = 1 there is no other column to lend a magnitude), and equal between two calls."""
    from wiki_grx_gym_amd.rl import grad_penalty as G
    for B in BATCHES:
        t = _inputs(B, n)
        d = {k: v.to(DEV) for k, v in t.items()}
        u = G.seed_fused(d["a"], d["mu"], d["sigma"])
        assert torch.equal(u.cpu(), G.seed_torch(t["a"], t["mu"], t["sigma"])), (B, n, "seed")
        h = G.gate_fused(d["g"], d["y"])
        assert torch.equal(h.cpu(), G.gate_torch(t["g"], t["y"])), (B, n, "gate")
        gbar, dz, db = G.gate_backward_fused(d["hbar"], d["g"], d["y"], d["dY"], want_gbar=True)
        dz2, db2 = G.gate_backward_fused(d["hbar"], d["g"], d["y"], d["dY"])
        want_dz, _ = G.gate_backward_torch(t["hbar"], t["g"], t["y"], t["dY"])
        assert torch.equal(gbar.cpu(), G.gate_torch(t["hbar"], t["y"])) and torch.equal(dz.cpu(), want_dz), (B, n, "gate_backward")
        assert torch.equal(dz, dz2) and torch.equal(db, db2), (B, n, "gate_backward twice")
        y64, e1, = t["y"].double(), G.e1(t["y"].double())
        terms = t["dY"].double() * e1 + t["hbar"].double() * t["g"].double() * G.e2(y64)
        err, lim = (db.double().cpu() - terms.sum(0)).abs(), 1e-6 * terms.abs().sum(0)
        print(f"B {B} n {n} db: worst err / bound {float((err / lim).max()):.3e}")
        assert bool((err <= lim).all()), (B, n, "db", err, lim)
        out, dsig = G.seed_backward_fused(d["ubar"], d["a"], d["mu"], d["sigma"], d["dmu"])
        out2, dsig2 = G.seed_backward_fused(d["ubar"], d["a"], d["mu"], d["sigma"], d["dmu"])
        want_out, _ = G.seed_backward_torch(t["ubar"], t["a"], t["mu"], t["sigma"], t["dmu"])
        assert torch.equal(out.cpu(), want_out) and torch.equal(out, out2) and torch.equal(dsig, dsig2), (B, n, "seed_backward")
        s64 = t["sigma"].double()
        terms = t["ubar"].double() * (-2.0 * (t["a"].double() - t["mu"].double()) / s64 ** 3)
        err, lim = (dsig.double().cpu() - terms.sum(0)).abs(), 1e-6 * terms.abs().sum(0)
        print(f"B {B} n {n} dsigma: worst err / bound {float((err / lim).max()):.3e}")
        assert bool((err <= lim).all()), (B, n, "dsigma", err, lim)
        P, P2 = G.sqnorm_fused(d["g"]), G.sqnorm_fused(d["g"])
        want_P = float(t["g"].double().square().sum() / B)
        print(f"B {B} n {n} P: {float(P):.9g} want {want_P:.9g}")
        assert abs(float(P) - want_P) <= 1e-6 * want_P and torch.equal(P, P2), (B, n, "sqnorm")
        # in place: dmu_out may be dmu
        dmu = d["dmu"].clone()
        lib = G._lib()
        partials = torch.empty(lib.grx_ppo_colsum_partials_size(B, n), device=DEV)
        ds = torch.empty(n, device=DEV)
        assert lib.grx_gp_seed_backward(B, n, d["ubar"].data_ptr(), d["a"].data_ptr(), d["mu"].data_ptr(), d["sigma"].data_ptr(), dmu.data_ptr(),
                                        dmu.data_ptr(), ds.data_ptr(), partials.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert torch.equal(dmu, out) and torch.equal(ds, dsig)


def test_rows_do_not_depend_on_the_batch():
    from wiki_grx_gym_amd.rl import grad_penalty as G
    t = {k: v.to(DEV) for k, v in _inputs(513, 39).items()}
    full = G.gate_backward_fused(t["hbar"], t["g"], t["y"], t["dY"])[0]
    part = G.gate_backward_fused(t["hbar"][100:165].contiguous(), t["g"][100:165].contiguous(), t["y"][100:165].contiguous(),
                                 t["dY"][100:165].contiguous())[0]
    assert torch.equal(full[100:165], part)
    assert torch.equal(G.seed_fused(t["a"], t["mu"], t["sigma"])[100:165], G.seed_fused(t["a"][100:165].contiguous(), t["mu"][100:165].contiguous(), t["sigma"]))


class _rocblas:
    """the update's BLAS preference (PPO._blas_for_update)"""

    def __enter__(self):
        self.prev = torch.backends.cuda.preferred_blas_library()
        torch.backends.cuda.preferred_blas_library("cublas")

    def __exit__(self, *exc):
        torch.backends.cuda.preferred_blas_library(self.prev)


@pytest.mark.parametrize("B,D,hidden,A", [(65, 39, [32, 16], 10), (130, 45, [512, 256, 128], 10)])
def test_function_on_the_device_against_float64(B, D, hidden, A, monkeypatch):
    """mu is the actor's own output on the training path, bit for bit; P and every gradient hold the CPU tier's bound (1e-4 max |want| per
    tensor) against torch's float64 double backward, with the HIP entry points and with GRX_GP_FUSED=0, and the two agree within it."""
    from wiki_grx_gym_amd.rl import grad_penalty as G
    from wiki_grx_gym_amd.rl.modules import MLP
    x, a, sigma, W, b, dmu = R.case(B, D, hidden, A, zero_row=True)
    ref = R.penalty_and_grads(x, a, sigma, W, b, dmu, 0.5)
    dev = lambda ts: [t.to(DEV) for t in ts]
    got = {}
    with _rocblas():
        for fused in ("1", "0"):
            monkeypatch.setenv("GRX_GP_FUSED", fused)
            got[fused] = run_function(x.to(DEV), a.to(DEV), sigma.to(DEV), dev(W), dev(b), dmu.to(DEV), 0.5)
            assert_against_ref(got[fused], ref, f"{(B, D, hidden, A)} GRX_GP_FUSED={fused}")
        actor = MLP(D, A, hidden, "elu").to(DEV)
        with torch.no_grad():
            for m, w, bb in zip([m for m in actor.model if isinstance(m, torch.nn.Linear)], W, b):
                m.weight.copy_(w); m.bias.copy_(bb)
        assert torch.is_grad_enabled() and torch.equal(got["1"][0], actor(x.to(DEV)).detach()) and torch.equal(got["0"][0], got["1"][0])
    flat = lambda r: [r[2]] + r[3] + r[4]
    wants = [ref["d_sigma"]] + ref["d_weights"] + ref["d_biases"]
    for g1, g0, want in zip(flat(got["1"]), flat(got["0"]), wants):
        assert float((g1 - g0).abs().max()) <= TOL * float(want.abs().max())


def _setup(monkeypatch, graph="1", seed=5, noise="scalar", **kw):
    from wiki_grx_gym_amd.rl.ppo import PPO
    monkeypatch.setenv("GRX_PPO_GRAPH", graph)
    torch.manual_seed(seed)
    alg = PPO(_policy(noise_std_type=noise), num_learning_epochs=2, num_mini_batches=4, clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.01,
              schedule="adaptive", desired_kl=0.01, learning_rate=1e-3, device=DEV, grad_penalty_coef=0.5, **kw)
    alg.init_storage(64, 8)
    _fill(alg, 8, 64, torch.Generator().manual_seed(seed + 1))
    return alg


@pytest.mark.parametrize("noise", ["scalar", "log"])
def test_minibatch_gradients_match_float64_and_the_torch_spelling(noise, monkeypatch):
    alg = _setup(monkeypatch, graph="0", noise=noise)
    with alg._blas_for_update():
        results, ref = minibatch_check(alg, DEV, fused_values=("1", "0"), monkeypatch=monkeypatch)
    for a, b, want in zip(results["1"], results["0"], ref["grads"]):
        assert float((a - b).abs().max()) <= TOL * float(want.abs().max())


def test_captured_update_equals_the_eager_one(monkeypatch):
    """two updates under GRX_PPO_GRAPH=1 and GRX_PPO_GRAPH=0 from the same state (64 envs, 8 steps, 4 minibatches), the device generator
    re-seeded before each, give bit-identical parameters, the same learning rate and the same mean penalty"""
    got = {}
    for graph in ("1", "0"):
        alg = _setup(monkeypatch, graph=graph)
        assert alg._use_graph == (graph == "1")
        torch.manual_seed(77)
        stats = [alg.update(), alg.update()]
        torch.cuda.synchronize()
        if graph == "1":
            assert isinstance(alg._graph, torch.cuda.CUDAGraph) and type(alg._gather).__name__ == "RowGather"
        got[graph] = ([p.detach().clone() for p in alg.actor_critic.parameters()], stats, alg.learning_rate, alg.mean_grad_penalty)
    for a, b in zip(got["1"][0], got["0"][0]):
        assert torch.equal(a, b)
    assert got["1"][1:] == got["0"][1:] and got["1"][3] > 0 and np.isfinite(got["1"][3])


def test_bf16_is_refused():
    from wiki_grx_gym_amd.rl.ppo import PPO
    with pytest.raises(ValueError, match="--precision bf16") as info:
        PPO(_policy(), device=DEV, precision="bf16", grad_penalty_coef=0.1)
    assert "--grad_penalty_coef" in str(info.value)


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
GP = ("--grad_penalty_coef", "0.002")


@pytest.mark.parametrize("flags", [(), ("--empirical_normalization", "--obs_history", "3", "--noise_std_type", "log"),
                                   ("--estimator", "--value_norm", "running", "--rnd")], ids=lambda f: "_".join(x.strip("-") for x in f) or "plain")
def test_runner_trains_with_the_penalty(tmp_path, flags):
    env, runner = _make(tmp_path, GP + flags)
    alg = runner.alg
    before = [p.detach().clone() for p in alg.actor_critic.parameters()]
    runner.learn(num_learning_iterations=2)
    assert isinstance(alg._graph, torch.cuda.CUDAGraph) and alg._static[0].shape[0] == 128
    assert all(not torch.equal(a, b) and bool(torch.isfinite(b).all()) for a, b in zip(before, alg.actor_critic.parameters()))
    tags = _tags(runner)
    assert all(np.isfinite(tags[k]) for k in ("Loss/grad_penalty", "Loss/value_function", "Loss/surrogate", "Loss/kl"))
    assert tags["Loss/grad_penalty"] > 0
    saved = set(torch.load(os.path.join(runner.log_dir, "model_2.pt"), weights_only=False))
    if not flags:
        assert saved == DEFAULT_KEYS                                                                 # nothing of it is saved
    assert not [k for k in saved if "grad_penalty" in k or k.startswith("gp")]


def test_play_on_a_penalty_run_and_the_default_path(tmp_path):
    from wiki_grx_gym_amd.scripts.play import play
    from wiki_grx_gym_amd.utils import get_args
    _, runner = _make(tmp_path, GP)
    runner.learn(num_learning_iterations=2)
    assert _tags(runner)["Loss/grad_penalty"] > 0
    out = play(get_args(["--task", "GR1T1", "--headless", "--seed", "3"]), steps=20, log_root=str(tmp_path))     # play.py knows nothing of it
    prunner, penv = out["runner"], out["env"]
    assert len(open(out["states"]).readlines()) == 20 and prunner.alg.grad_penalty_coef is None
    jit = torch.jit.load(out["exported"])
    x = torch.randn(64, 39)
    want = prunner.algorithm.actor_critic.actor(x.to(penv.device)).cpu()
    assert (jit(x) - want).abs().max() < 1e-6                                                                # tests/test_play_gpu.py's tolerance
    trained = runner.alg.actor_critic.state_dict()
    assert all(torch.equal(v, prunner.alg.actor_critic.state_dict()[k]) for k, v in trained.items() if k != "std")
    _, plain = _make(tmp_path / "plain")
    plain.learn(num_learning_iterations=1)
    alg = plain.alg
    assert type(alg._gather).__name__ == "RowGather" and alg.grad_penalty_coef is None and not [k for k in vars(alg) if k.startswith("_gp_")]
    assert set(torch.load(os.path.join(plain.log_dir, "model_1.pt"), weights_only=False)) == DEFAULT_KEYS
    assert "Loss/grad_penalty" not in _tags(plain)
