"""The Lipschitz gradient penalty (rl/grad_penalty.py) on the CPU: the torch spelling of the hand-written second-order pass
against torch's own float64 double backward (tests/grad_penalty_ref.py), a minibatch step of PPO, the refusals, the flag, one update through
the runner over the oracle-backed env, and the C entry points' argument checks.

The bound of every gradient comparison is 1e-4 max |want| per tensor, the bound tests/test_smooth.py uses for the same kind of comparison
(fp32 formulas against float64 autograd measured 2e-7 to 5e-7 here)."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import grad_penalty_ref as R
from tests.test_env_plumbing import oracle_backend  # noqa: F401  (the fixture)
from tests.test_smooth import _NoEnv, _make, _tags, _train_cfg
from wiki_grx_gym_amd.envs import GR1T1Cfg, config
from wiki_grx_gym_amd.envs.config import class_to_dict
from wiki_grx_gym_amd.rl import grad_penalty as G
from wiki_grx_gym_amd.rl.modules import MLP, ActorCriticMLP
from wiki_grx_gym_amd.rl.ppo import PPO
from wiki_grx_gym_amd.rl.runner import OnPolicyRunner
from wiki_grx_gym_amd.utils import get_args
from wiki_grx_gym_amd.utils.helpers import update_cfg_from_args

TOL = 1e-4
SHAPES = [(1, 5, [8], 1), (65, 39, [32, 16], 10), (257, 45, [512, 256, 128], 10)]


def run_function(x, a, sigma, weights, biases, dmu, c, needs_dx=False):
    """GradPenalty on fp32 leaves, backward of c P + sum(dmu mu): (mu, P, d_sigma, d_weights, d_biases, dx)"""
    x = x.clone().requires_grad_(needs_dx)
    sigma = sigma.clone().requires_grad_()
    weights, biases = [w.clone().requires_grad_() for w in weights], [b.clone().requires_grad_() for b in biases]
    mu, P = G.GradPenalty.apply(x, a, sigma, *[p for wb in zip(weights, biases) for p in wb])
    (c * P + (dmu * mu).sum()).backward()
    return mu.detach(), P.detach(), sigma.grad, [w.grad for w in weights], [b.grad for b in biases], x.grad


def assert_against_ref(got, ref, label=""):
    mu, P, d_sigma, d_w, d_b, _ = got
    print(f"{label} P {float(P):.9g} want {ref['P']:.9g}")
    assert abs(float(P) - ref["P"]) <= TOL * abs(ref["P"])
    assert float((mu.double().cpu() - ref["mu"]).abs().max()) <= TOL * float(ref["mu"].abs().max())
    named = [("sigma", d_sigma, ref["d_sigma"])] + [(f"W{l + 1}", g, w) for l, (g, w) in enumerate(zip(d_w, ref["d_weights"]))] \
        + [(f"b{l + 1}", g, w) for l, (g, w) in enumerate(zip(d_b, ref["d_biases"]))]
    for name, g, want in named:
        err, lim = float((g.double().cpu() - want).abs().max()), TOL * float(want.abs().max())
        print(f"{label} {name}: max err {err:.3e}, bound {lim:.3e}")
        assert err <= lim, (label, name, err, lim)


@pytest.mark.parametrize("B,D,hidden,A", SHAPES)
def test_torch_spelling_against_float64_double_backward(B, D, hidden, A):
    x, a, sigma, W, b, dmu = R.case(B, D, hidden, A)
    for c, seed_mu in ((1.0, None), (0.37, dmu)):                           # the penalty alone, and sharing the backward with a gradient at mu
        ref = R.penalty_and_grads(x, a, sigma, W, b, seed_mu, c)
        got = run_function(x, a, sigma, W, b, seed_mu if seed_mu is not None else torch.zeros_like(dmu), c)
        assert_against_ref(got, ref, f"{(B, D, hidden, A)} c={c}")
    actor = MLP(D, A, hidden, "elu")
    with torch.no_grad():
        for m, w, bb in zip([m for m in actor.model if isinstance(m, torch.nn.Linear)], W, b):
            m.weight.copy_(w); m.bias.copy_(bb)
    mu, _ = G.grad_penalty(actor, x, a, sigma)
    assert torch.equal(mu, actor(x))                                         # the actor's own output, bit for bit


def test_a_hidden_output_exactly_at_zero_and_rows_on_both_sides():
    B, D, hidden, A = 65, 39, [32, 16], 10
    x, a, sigma, W, b, dmu = R.case(B, D, hidden, A, zero_row=True)
    y1 = torch.nn.functional.elu(torch.nn.functional.linear(x, W[0], b[0]))
    assert float(y1[0, 0]) == 0.0 and float(y1[1, 0]) > 0.1 and float(y1[2, 0]) < -0.1
    ref = R.penalty_and_grads(x, a, sigma, W, b, dmu, 0.5)
    got = run_function(x, a, sigma, W, b, dmu, 0.5)
    assert_against_ref(got, ref, "zero row")
    # the row at zero alone (B = 1 makes its terms the whole gradient: a wrong side of ELU'' at 0 would show in b1[0] undiluted)
    one = lambda t: t[:1].clone()
    ref = R.penalty_and_grads(one(x), one(a), sigma, W, b, one(dmu), 0.5)
    got = run_function(one(x), one(a), sigma, W, b, one(dmu), 0.5)
    assert_against_ref(got, ref, "zero row alone")


def test_input_gradient_and_rows_do_not_mix():
    x, a, sigma, W, b, dmu = R.case(7, 6, [8, 4], 3)
    got = run_function(x, a, sigma, W, b, dmu, 0.5, needs_dx=True)
    x64 = R._d(x).requires_grad_()
    mu, P = R.penalty(x64, R._d(a), R._d(sigma), [R._d(w) for w in W], [R._d(v) for v in b])
    want, = torch.autograd.grad(0.5 * P + (R._d(dmu) * mu).sum(), x64)
    assert float((got[5].double() - want).abs().max()) <= TOL * float(want.abs().max())
    # a row's share of B P is its own: the penalty of rows 0..2 alone, rescaled, is what those rows add
    _, P3 = G.GradPenalty.apply(x[:3], a[:3], sigma, *[p for wb in zip(W, b) for p in wb])
    _, P4 = G.GradPenalty.apply(x[3:], a[3:], sigma, *[p for wb in zip(W, b) for p in wb])
    assert abs(float(3 * P3 + 4 * P4) - 7 * float(got[1])) <= 1e-5 * 7 * float(got[1])


# ---- PPO and the runner --------------------------------------------------------------------------------------------------------------------
def _policy(**kw):
    return ActorCriticMLP(39, 168, 10, actor_hidden_dims=[32, 16], critic_hidden_dims=[32, 16], activation="elu", init_noise_std=0.4, **kw)


def _fill(alg, T, N, g):
    """tests/test_smooth.py's filled storage, with sigma from noise_std() (either noise type)"""
    st, ac = alg.storage, alg.actor_critic
    r = lambda *s: torch.randn(*s, generator=g).to(st.observations.device)
    with torch.no_grad():
        st.observations.copy_(r(T, N, 39)); st.pri_observations.copy_(r(T, N, 168))
        mu, value = ac.actor(st.observations.flatten(0, 1)), ac.critic(st.pri_observations.flatten(0, 1))
        std = ac.noise_std().detach()
        st.mu.copy_((mu + 0.1 * std * r(T * N, 10)).view(T, N, 10))
        st.sigma.copy_((std * (1.0 + 0.1 * torch.rand(T * N, 10, generator=g).to(mu.device))).view(T, N, 10))
        st.actions.copy_((mu + std * r(T * N, 10)).view(T, N, 10))
        logp = torch.distributions.Normal(mu, std).log_prob(st.actions.flatten(0, 1)).sum(-1, keepdim=True)
        st.actions_log_prob.copy_((logp + 0.2 * r(T * N, 1)).view(T, N, 1))
        st.values.copy_((value + 0.2 * r(T * N, 1)).view(T, N, 1))
        st.returns.copy_((value + r(T * N, 1)).view(T, N, 1))
        st.advantages.copy_(r(T, N, 1))
        st.dones.copy_((torch.rand(T, N, 1, generator=g) < 0.3).to(torch.uint8))
    st.step = T


def minibatch_check(alg, device, fused_values=("1",), monkeypatch=None):
    """one minibatch step of `alg` (64 of T N rows) against tests/grad_penalty_ref's float64 autograd; returns the gradients per value of
    GRX_GP_FUSED, and the reference"""
    st = alg.storage
    T, N = st.num_transitions_per_env, st.num_envs
    idx = torch.randperm(T * N, generator=torch.Generator().manual_seed(3))[:64].to(device)
    batch = [s[idx].contiguous() for s in alg._sym_sources()]
    ac64 = copy.deepcopy(alg.actor_critic).double().cpu()
    ref = R.gp_minibatch_ref(ac64, batch, alg.grad_penalty_coef, alg.clip_param, alg.value_loss_coef, alg.entropy_coef, alg.use_clipped_value_loss)
    assert ref["P"] > 1e-3
    results = {}
    for fused in fused_values:
        if monkeypatch is not None:
            monkeypatch.setenv("GRX_GP_FUSED", fused)
        alg._gp_sum.zero_()
        s, vl, loss, kl = alg._losses_gp(*batch)
        alg.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        out = torch.stack([s, vl, loss, kl]).detach().double().cpu()
        grads = [p.grad.detach().clone() for p in alg.actor_critic.parameters()]
        P = float(alg._gp_sum.item())
        print(f"GRX_GP_FUSED={fused} P {P:.9g} want {ref['P']:.9g}")
        assert abs(P - ref["P"]) <= TOL * ref["P"], (fused, P, ref["P"])
        assert (out - ref["out"]).abs().max() <= TOL * ref["out"].abs().max(), (fused, out, ref["out"])
        for (n, _), got, want in zip(alg.actor_critic.named_parameters(), grads, ref["grads"]):
            err, lim = float((got.double().cpu() - want).abs().max()), TOL * float(want.abs().max())
            print(f"GRX_GP_FUSED={fused} {n}: max err {err:.3e}, bound {lim:.3e}")
            assert err <= lim, (fused, n, err, lim)
        results[fused] = grads
    return results, ref


@pytest.mark.parametrize("noise", ["scalar", "log"])
def test_minibatch_parameter_gradients_match_float64(noise):
    torch.manual_seed(5)
    alg = PPO(_policy(noise_std_type=noise), num_learning_epochs=2, num_mini_batches=4, entropy_coef=0.01, schedule="adaptive", device="cpu",
              grad_penalty_coef=0.5)
    alg.init_storage(32, 8)
    _fill(alg, 8, 32, torch.Generator().manual_seed(6))
    minibatch_check(alg, "cpu")
    before = [p.detach().clone() for p in alg.actor_critic.parameters()]
    alg.update()                                                              # ... and the CPU update runs on it
    assert alg.mean_grad_penalty > 0 and np.isfinite(alg.mean_grad_penalty)
    assert all(not torch.equal(a, b) and bool(torch.isfinite(b).all()) for a, b in zip(before, alg.actor_critic.parameters()))


def test_a_non_finite_penalty_skips_the_step():
    torch.manual_seed(5)
    alg = PPO(_policy(), num_learning_epochs=1, num_mini_batches=2, device="cpu", grad_penalty_coef=0.5)
    alg.init_storage(16, 4)
    _fill(alg, 4, 16, torch.Generator().manual_seed(6))
    alg.storage.actions[0, 0, 0] = float("inf")                               # reaches P through u, not the clipped surrogate alone
    before = [p.detach().clone() for p in alg.actor_critic.parameters()]
    alg.update()
    after = list(alg.actor_critic.parameters())
    assert all(bool(torch.isfinite(p).all()) for p in after) and any(not torch.equal(a, b) for a, b in zip(before, after))
    assert np.isfinite(alg.mean_grad_penalty)                                 # (the dropped step adds nothing to the statistic)


def test_default_path_builds_no_grad_penalty_state():
    alg = PPO(_policy(), device="cpu")
    assert alg.grad_penalty_coef is None and alg.mean_grad_penalty == 0.0
    assert not [k for k in vars(alg) if k.startswith("_gp_")]
    assert not [k for k, v in vars(alg).items() if "grad_penalty" in k and v is not None and not isinstance(v, float)]


def test_ppo_refusals(monkeypatch):
    from wiki_grx_gym_amd.rl import symmetry as Y
    from wiki_grx_gym_amd.rl.recurrent import ActorCriticRecurrent
    with pytest.raises(ValueError, match="--recurrent") as info:
        PPO(ActorCriticRecurrent(39, 168, 10, rnn_hidden_size=32, actor_hidden_dims=[16], critic_hidden_dims=[16]), device="cpu", grad_penalty_coef=0.1)
    assert "--grad_penalty_coef" in str(info.value)
    with pytest.raises(ValueError, match="--state_dependent_std") as info:
        PPO(_policy(state_dependent_std=True, noise_std_type="log"), device="cpu", grad_penalty_coef=0.1)
    assert "--grad_penalty_coef" in str(info.value)
    lower = [f"{s}_{j}_joint" for s in ("left", "right") for j in ("hip_roll", "hip_yaw", "hip_pitch", "knee_pitch", "ankle_pitch")]
    pts = [round(-0.5 + 0.1 * i, 1) for i in range(11)]
    maps = Y.SymmetryMaps(Y.MirrorMap(*Y.frame_map(lower), "cpu"), Y.MirrorMap(*Y.privileged_map(lower, pts, pts), "cpu"),
                          Y.MirrorMap(*Y.joint_map(lower), "cpu"))
    with pytest.raises(ValueError, match="--symmetry") as info:
        PPO(_policy(), device="cpu", symmetry="loss", symmetry_maps=maps, grad_penalty_coef=0.1)
    assert "--grad_penalty_coef" in str(info.value)
    with pytest.raises(ValueError, match="--smooth") as info:
        PPO(_policy(), device="cpu", smooth="spatial", grad_penalty_coef=0.1)
    assert "--grad_penalty_coef" in str(info.value)
    for bad in (0.0, -0.1, float("nan"), float("inf"), "0.1", True):
        with pytest.raises(ValueError, match="--grad_penalty_coef"):
            PPO(_policy(), device="cpu", grad_penalty_coef=bad)
    with pytest.raises(ValueError, match="Linear -> ELU") as info:               # an actor the pass does not cover
        PPO(ActorCriticMLP(39, 168, 10, actor_hidden_dims=[32, 16], critic_hidden_dims=[32, 16], activation="tanh"), device="cpu", grad_penalty_coef=0.1)
    assert "--grad_penalty_coef" in str(info.value)
    # (precision="bf16" needs a HIP device: tests/test_grad_penalty_gpu.py)
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    monkeypatch.setattr(dist, "get_rank", lambda *a: 0)
    with pytest.raises(NotImplementedError, match="world size") as info:
        PPO(_policy(), device="cpu", grad_penalty_coef=0.1)
    assert "--grad_penalty_coef" in str(info.value)


def _cfg_dict(flags=("--grad_penalty_coef", "0.002"), runner=(), algorithm=(), policy=()):
    d = class_to_dict(update_cfg_from_args(None, _train_cfg(), get_args(list(flags)))[1])
    d["runner"].update(runner); d["algorithm"].update(algorithm); d["policy"].update(policy)
    return d


def test_runner_refusals(monkeypatch, tmp_path):
    r = OnPolicyRunner(_NoEnv(), _cfg_dict(), None, "cpu")                                          # the flag alone is fine
    assert r.grad_penalty_coef == 0.002 and r.alg.grad_penalty_coef == 0.002
    for keys in (dict(runner={"empirical_normalization": True}), dict(runner={"obs_history_length": 3, "critic_obs_history_length": 2}),
                 dict(runner={"privileged_actor": True}), dict(algorithm={"rnd": True}),
                 dict(algorithm={"value_norm": "popart"}), dict(policy={"noise_std_type": "log"})):
        assert OnPolicyRunner(_NoEnv(), _cfg_dict(**keys), None, "cpu").alg.grad_penalty_coef == 0.002   # ... and with what it composes with
    for keys, exc, other in ((dict(runner={"policy_class_name": "ActorCriticRecurrent"}, policy={"rnn_hidden_size": 32}), ValueError, "--recurrent"),
                             (dict(algorithm={"symmetry": "loss"}), ValueError, "--symmetry"),
                             (dict(algorithm={"smooth": "spatial"}), ValueError, "--smooth"),
                             (dict(policy={"state_dependent_std": True, "noise_std_type": "log"}), ValueError, "--state_dependent_std"),
                             (dict(runner={"distill_from": str(tmp_path / "teacher.pt")}), ValueError, "--distill_from"),
                             (dict(algorithm={"precision": "bf16"}), ValueError, "--precision bf16"),
                             (dict(runner={"exact_resume": True}), NotImplementedError, "--exact_resume"),
                             (dict(algorithm={"grad_penalty_coef": -1.0}), ValueError, "above 0"),
                             (dict(algorithm={"grad_penalty_coef": float("nan")}), ValueError, "above 0")):
        with pytest.raises(exc, match=other) as info:
            OnPolicyRunner(_NoEnv(), _cfg_dict(**keys), None, "cpu")
        assert "--grad_penalty_coef" in str(info.value), keys                                       # the message names both options
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    monkeypatch.setattr(dist, "get_rank", lambda *a: 0)
    with pytest.raises(NotImplementedError, match="world size") as info:
        OnPolicyRunner(_NoEnv(), _cfg_dict(), None, "cpu")
    assert "--grad_penalty_coef" in str(info.value)


def test_cli_flag_reaches_the_config_and_is_no_config_key(tmp_path):
    assert get_args([]).grad_penalty_coef is None
    plain = class_to_dict(update_cfg_from_args(None, config.GR1T1CfgPPO(), get_args([]))[1])
    assert "grad_penalty_coef" not in plain["algorithm"]
    d = class_to_dict(update_cfg_from_args(None, config.GR1T1CfgPPO(), get_args(["--grad_penalty_coef", "0.002"]))[1])
    assert d["algorithm"]["grad_penalty_coef"] == 0.002
    del d["algorithm"]["grad_penalty_coef"]
    assert d == plain                                                                             # the one key, nothing else
    for cls in (config.GR1T1CfgPPO, config.GR1T2CfgPPO, config.GR1T1FullBodyCfgPPO):               # not a config key
        assert not [k for k in vars(cls.algorithm) if k.startswith("grad_penalty")]
    from wiki_grx_gym_amd.utils.helpers import get_args as ga
    import io, contextlib
    buf = io.StringIO()
    with pytest.raises(SystemExit), contextlib.redirect_stdout(buf):
        ga(["--help"])
    assert "--grad_penalty_coef" in buf.getvalue() and "0.002" in buf.getvalue() and "not tuned" in buf.getvalue()


@pytest.mark.parametrize("flags", [("--grad_penalty_coef", "0.002"), ("--grad_penalty_coef", "0.002", "--empirical_normalization", "--obs_history", "3")])
def test_one_update_through_the_runner(oracle_backend, tmp_path, flags):  # noqa: F811
    _, runner = _make(tmp_path / "gp", flags, env_cfg=GR1T1Cfg())
    alg = runner.alg
    assert alg.grad_penalty_coef == 0.002
    before = [p.detach().clone() for p in alg.actor_critic.parameters()]
    runner.learn(num_learning_iterations=1)
    assert all(not torch.equal(a, b) and bool(torch.isfinite(b).all()) for a, b in zip(before, alg.actor_critic.parameters()))
    tags = _tags(runner)
    assert np.isfinite(tags["Loss/grad_penalty"]) and tags["Loss/grad_penalty"] > 0 and tags["Loss/grad_penalty"] == alg.mean_grad_penalty
    plain_flags = tuple(f for f in flags if f not in ("--grad_penalty_coef", "0.002"))
    _, plain = _make(tmp_path / "plain", plain_flags)
    plain.learn(num_learning_iterations=1)
    assert plain.alg.grad_penalty_coef is None and "Loss/grad_penalty" not in _tags(plain)
    ck = torch.load(os.path.join(runner.log_dir, "model_1.pt"), weights_only=False)
    ck_plain = torch.load(os.path.join(plain.log_dir, "model_1.pt"), weights_only=False)
    assert set(ck) == set(ck_plain) and set(ck["model_state_dict"]) == set(ck_plain["model_state_dict"])
    if len(flags) == 2:
        assert set(ck) == {"model_state_dict", "optimizer_state_dict", "iter", "infos"}              # exactly today's four
    plain.load(os.path.join(runner.log_dir, "model_1.pt"))                                         # a policy trained with it loads like any other
    loaded = plain.alg.actor_critic.state_dict()
    assert all(torch.equal(v, loaded[k]) for k, v in alg.actor_critic.state_dict().items() if k != "std")


def test_default_path_imports_nothing_of_it(oracle_backend, tmp_path, monkeypatch):  # noqa: F811
    import sys
    monkeypatch.setitem(sys.modules, G.__name__, None)                                            # any import of rl.grad_penalty now raises
    _, runner = _make(tmp_path, flags=())
    runner.learn(num_learning_iterations=1)
    assert runner.grad_penalty_coef is None and runner.alg.grad_penalty_coef is None
    ck = torch.load(os.path.join(runner.log_dir, "model_1.pt"), weights_only=False)
    assert set(ck) == {"model_state_dict", "optimizer_state_dict", "iter", "infos"}
    assert "Loss/grad_penalty" not in _tags(runner)
    with pytest.raises(ImportError):
        _make(None, flags=("--grad_penalty_coef", "0.002"))                                       # (the patch does bite with the flag)


# ---- the C entry points, without a GPU --------------------------------------------------------------------------------------------------
def test_entry_points_are_exported_and_refuse_bad_arguments():
    from wiki_grx_gym_amd.rl.fused_loss import load_ppo_library
    lib = load_ppo_library()
    for name in ("grx_gp_seed", "grx_gp_gate", "grx_gp_sqnorm_partials_size", "grx_gp_sqnorm", "grx_gp_gate_backward", "grx_gp_seed_backward"):
        assert hasattr(lib, name), name
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "grx_ppo_gp.h")).read()
    assert all(f"int {n}(" in hdr for n in ("grx_gp_seed", "grx_gp_gate", "grx_gp_sqnorm", "grx_gp_gate_backward", "grx_gp_seed_backward"))
    assert lib.grx_gp_sqnorm_partials_size(65, 39) == 2 * 2 and lib.grx_gp_sqnorm_partials_size(1, 1) == 2
    assert lib.grx_gp_sqnorm_partials_size(0, 5) == 0 and lib.grx_gp_sqnorm_partials_size(5, 0) == 0
    assert lib.grx_gp_sqnorm_partials_size(1 << 20, 1 << 11) == 0                                   # B n = 2^31
    p = C.c_void_p(0x1000)    # (never dereferenced: every call below is refused before a launch)
    big = (1 << 20, 1 << 11)
    for B, n in ((0, 4), (4, 0), (-1, 4), big):
        assert lib.grx_gp_seed(B, n, p, p, p, p, None) < 0
        assert lib.grx_gp_gate(B, n, p, p, p, None) < 0
        assert lib.grx_gp_sqnorm(B, n, p, p, p, None) < 0
        assert lib.grx_gp_gate_backward(B, n, p, p, p, p, None, p, p, p, None) < 0
        assert lib.grx_gp_seed_backward(B, n, p, p, p, p, p, p, p, p, None) < 0
    for k in range(4):
        args = [p] * 4; args[k] = None
        assert lib.grx_gp_seed(4, 4, *args, None) < 0
    for k in range(3):
        args = [p] * 3; args[k] = None
        assert lib.grx_gp_gate(4, 4, *args, None) < 0
        assert lib.grx_gp_sqnorm(4, 4, *args, None) < 0
    assert lib.grx_gp_sqnorm(4, 4, p, p, C.c_void_p(0x1004), None) < 0                              # a misaligned partials
    for k in (0, 1, 2, 3, 5, 6, 7):                                                                 # (4, gbar, is optional)
        args = [p] * 8; args[4] = None; args[k] = None
        assert lib.grx_gp_gate_backward(4, 4, *args, None) < 0
    for k in range(8):
        args = [p] * 8; args[k] = None
        assert lib.grx_gp_seed_backward(4, 4, *args, None) < 0
    assert lib.grx_gp_gate_backward(65536 * 256, 1, p, p, p, p, None, p, p, p, None) < 0              # more slabs than a grid has rows
