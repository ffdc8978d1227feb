"""Action-smoothness regularisation (rl/smooth.py) on the CPU: the torch spellings of the gather and the loss against the
float64 reference of tests/smooth_ref.py, the masking rules, the refusals, the flags, and one update through the runner over the
oracle-backed env."""
import copy
import os

import numpy as np
import pytest
import torch

from tests import smooth_ref as R
from tests.test_env_plumbing import oracle_backend  # noqa: F401  (the fixture)
from wiki_grx_gym_amd.envs import GR1T1Cfg, GR1T1CfgPPO, config
from wiki_grx_gym_amd.envs.config import class_to_dict
from wiki_grx_gym_amd.rl import smooth as S
from wiki_grx_gym_amd.rl.modules import ActorCriticMLP
from wiki_grx_gym_amd.rl.ppo import PPO
from wiki_grx_gym_amd.rl.runner import OnPolicyRunner
from wiki_grx_gym_amd.utils import get_args, task_registry
from wiki_grx_gym_amd.utils.helpers import update_cfg_from_args

EPS32 = 2.0 ** -23


def gather_case(mb, widths, seed=0, T=4):
    """sources of T x N rows (N = mb), idx with a repeat, dones at rate 0.3; for mb > 1 the case holds a valid row, a row masked by a done
    and a row masked by t = T - 1 (asserted)"""
    g = np.random.default_rng(100 * mb + widths[0] + seed)
    N = mb
    srcs = [g.standard_normal((T * N, w)).astype(np.float32) for w in widths]
    dones = (g.random(T * N) < 0.3).astype(np.uint8)
    idx = g.integers(0, T * N, mb).astype(np.int64)
    if mb > 1:
        idx[0], idx[1], idx[2] = 0, N, (T - 1) * N + 1          # t = 0 (not done), t = 1 (done), the last step
        dones[0], dones[N], dones[(T - 1) * N + 1] = 0, 1, 0
        idx[-1] = idx[0]                                        # a repeat for certain
        v = R.valid_np(idx, N, T, dones)
        t = idx // N
        assert v.any() and ((t < T - 1) & (dones[idx] != 0)).any() and ((t == T - 1) & (dones[idx] == 0)).any()
    eps = g.standard_normal((mb, widths[0])).astype(np.float32)
    return srcs, dones, idx, eps, N, T


@pytest.mark.parametrize("mode", list(R.MODES))
@pytest.mark.parametrize("mb", [1, 7, 65])
def test_torch_gather_against_float64(mb, mode):
    succ, pert = R.MODES[mode]
    widths, sigma = (39, 10, 1), 0.05
    srcs, dones, idx, eps, N, T = gather_case(mb, widths)
    for one_idx in ([idx] if mb > 1 else [np.array([0]), np.array([3])]):      # (mb = 1: N = 1, T = 4: t = 0 and t = T - 1)
        if mb == 1:
            dones[:] = 0
        rows = 1 + int(succ) + int(pert)
        dsts = [torch.full((mb * (rows if t == 0 else 1), w), 777.0) for t, w in enumerate(widths)]
        valid = torch.full((mb,), 7, dtype=torch.uint8)
        S.smooth_gather_torch([torch.tensor(s) for s in srcs], dsts, torch.tensor(one_idx), N, T, torch.tensor(dones), succ, pert, torch.tensor(eps),
                              sigma, valid)
        want, v = R.gather_np(srcs, one_idx, N, T, dones, mode, eps, np.float32(sigma))
        if succ:
            assert np.array_equal(valid.numpy() != 0, v)
        else:
            assert bool((valid == 7).all())
        for t, (d, wnt) in enumerate(zip(dsts, want)):
            got = d.double().numpy()
            keep = mb * (1 + int(succ)) if t == 0 else mb
            np.testing.assert_array_equal(got[:keep], wnt[:keep])
            if t == 0 and pert:
                lim = EPS32 * (np.abs(np.float32(sigma) * eps.astype(np.float64)) + np.abs(wnt[:mb]))
                assert (np.abs(got[keep:] - wnt[keep:]) <= lim).all()


@pytest.mark.parametrize("mask", ["all", "none", "mixed"])
@pytest.mark.parametrize("mode", list(R.MODES))
@pytest.mark.parametrize("mb,A", [(1, 1), (33, 10), (257, 32)])
def test_torch_loss_and_gradient_against_float64(mb, A, mode, mask):
    succ, pert = R.MODES[mode]
    mu_np, valid_np = R.loss_inputs(mb, A, mode, mask)
    ct, cs = float(np.float32(0.7)), float(np.float32(0.3))
    want, want_grad = R.loss_and_grad(mu_np, mode, valid_np, ct, cs)
    mu = torch.tensor(mu_np, requires_grad=True)
    total, terms = S.smooth_loss(mu, succ, pert, torch.tensor(valid_np), ct, cs)
    total.backward()
    got = np.array([float(terms[0]), float(terms[1]), float(total.detach())])
    # a float32 sum of n squares, each within 3 roundings: relative error below (n + 4) 2^-24 of the sum of magnitudes (all terms >= 0)
    lim = (mb * A + 8) * 2.0 ** -24 * np.abs(want[:3]) + 1e-30
    assert (np.abs(got - want[:3]) <= lim).all(), (got, want)
    assert want[3] == int((valid_np != 0).sum()) if succ else want[3] == 0
    scale = np.abs(want_grad) * 2.0 ** -20 + 2.0 ** -24 * np.abs(want_grad).max() + 1e-30
    assert (np.abs(mu.grad.double().numpy() - want_grad) <= scale).all()
    if succ:
        masked = valid_np == 0
        assert not mu.grad[mb:2 * mb][torch.tensor(masked)].any()                     # exact zeros
        if not pert:
            assert not mu.grad[:mb][torch.tensor(masked)].any()
    if mask == "none" and succ:
        assert float(terms[0]) == 0.0 and np.isfinite(float(total.detach())) and bool(torch.isfinite(mu.grad).all())


def test_masked_pairs_ignore_a_nan_and_counted_rows_do_not():
    mb, A = 33, 10
    for mode in ("temporal", "both"):
        mu_np, valid_np = R.loss_inputs(mb, A, mode, "mixed")
        clean, clean_grad = R.loss_and_grad(mu_np, mode, valid_np, 0.5, 0.25)
        masked_row = int(np.flatnonzero(valid_np == 0)[0])
        poisoned = mu_np.copy()
        poisoned[mb + masked_row] = np.nan                                            # the successor of a masked pair
        mu = torch.tensor(poisoned, requires_grad=True)
        total, terms = S.smooth_loss(mu, True, mode == "both", torch.tensor(valid_np), 0.5, 0.25)
        total.backward()
        assert bool(torch.isfinite(total)) and bool(torch.isfinite(mu.grad).all()) and not mu.grad[mb + masked_row].any()
        assert abs(float(total.detach()) - clean[2]) <= 1e-5 * abs(clean[2])
        ref, ref_grad = R.loss_and_grad(poisoned, mode, valid_np, 0.5, 0.25)           # the reference never reads it either
        assert np.array_equal(ref, clean) and np.array_equal(ref_grad, clean_grad)
        counted = mu_np.copy()
        counted[mb + int(np.flatnonzero(valid_np != 0)[0])] = np.nan
        total, _ = S.smooth_loss(torch.tensor(counted), True, mode == "both", torch.tensor(valid_np), 0.5, 0.25)
        assert bool(torch.isnan(total))


# ---- PPO and the runner --------------------------------------------------------------------------------------------------------------------
def _policy(**kw):
    return ActorCriticMLP(39, 168, 10, actor_hidden_dims=[32, 16], critic_hidden_dims=[32, 16], activation="elu", init_noise_std=0.4, **kw)


def _fill(alg, T, N, g):
    st, ac = alg.storage, alg.actor_critic
    r = lambda *s: torch.randn(*s, generator=g).to(st.observations.device)
    with torch.no_grad():
        st.observations.copy_(r(T, N, 39)); st.pri_observations.copy_(r(T, N, 168))
        mu, value = ac.actor(st.observations.flatten(0, 1)), ac.critic(st.pri_observations.flatten(0, 1))
        std = ac.std.detach()
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


def minibatch_check(alg, mode, device, fused_values=("1",), monkeypatch=None, tol=1e-4):
    """one minibatch step of `alg` (64 of T N rows) against tests/smooth_ref's float64 autograd, with the same eps fed to both; returns
    the gradients per value of GRX_SMOOTH_FUSED"""
    st = alg.storage
    T, N = st.num_transitions_per_env, st.num_envs
    mb = 64
    succ, pert = R.MODES[mode]
    idx = torch.randperm(T * N, generator=torch.Generator().manual_seed(3))[:mb].to(device)
    srcs = alg._smooth_sources()
    rows = alg._smooth_rows()
    bufs = [torch.zeros(mb * (rows if t == 0 else 1), s.shape[1], device=device) for t, s in enumerate(srcs)]
    alg._smooth_alloc(mb, 39)
    eps = torch.randn(mb, 39, generator=torch.Generator().manual_seed(4))
    if pert:
        alg._smooth_eps.copy_(eps)
    dones = st.dones.reshape(-1).cpu().numpy()
    v = R.valid_np(idx.cpu().numpy(), N, T, dones)
    assert not succ or (v.any() and not v.all())
    succ_rows = srcs[0].cpu().double().numpy()[np.minimum(idx.cpu().numpy() + N, T * N - 1)]
    ac64 = copy.deepcopy(alg.actor_critic).double().cpu()
    ref = R.smooth_minibatch_ref(ac64, [s[idx] for s in srcs], succ_rows, v, eps.numpy(), mode, float(np.float32(alg.smooth_temporal_coef)),
                                 float(np.float32(alg.smooth_spatial_coef)), float(np.float32(alg.smooth_sigma)), alg.clip_param,
                                 alg.value_loss_coef, alg.entropy_coef, alg.use_clipped_value_loss)
    assert (ref["terms"][0] > 1e-4 or not succ) and (ref["terms"][1] > 1e-6 or not pert)
    results = {}
    for fused in fused_values:
        if monkeypatch is not None:
            monkeypatch.setenv("GRX_SMOOTH_FUSED", fused)
        alg._smooth_sum.zero_()
        alg._smooth_gatherer(srcs, bufs, draw=False)(idx)
        if succ:
            assert np.array_equal(alg._smooth_valid.cpu().numpy() != 0, v)
        s, vl, loss, kl = alg._losses_smooth(*bufs)
        alg.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        out = torch.stack([s, vl, loss, kl]).detach().double().cpu()
        grads = [p.grad.detach().clone() for p in alg.actor_critic.parameters()]
        terms = alg._smooth_sum.double().cpu().numpy()
        assert (np.abs(terms - ref["terms"]) <= tol * ref["terms"] + 1e-12).all(), (fused, terms, ref["terms"])
        assert (out - ref["out"]).abs().max() <= tol * ref["out"].abs().max(), (fused, out, ref["out"])
        for (n, _), got, want in zip(alg.actor_critic.named_parameters(), grads, ref["grads"]):
            err, lim = float((got.double().cpu() - want).abs().max()), tol * float(want.abs().max())
            print(f"{mode} GRX_SMOOTH_FUSED={fused} {n}: max err {err:.3e}, bound {lim:.3e}")
            assert err <= lim, (mode, fused, n, err, lim)
        results[fused] = grads
    return results, ref


@pytest.mark.parametrize("mode", list(R.MODES))
def test_minibatch_parameter_gradients_match_float64(mode):
    torch.manual_seed(5)
    alg = PPO(_policy(), num_learning_epochs=2, num_mini_batches=4, entropy_coef=0.01, schedule="adaptive", device="cpu", smooth=mode,
              smooth_temporal_coef=0.7, smooth_spatial_coef=0.9, smooth_sigma=0.1)
    alg.init_storage(32, 8)
    _fill(alg, 8, 32, torch.Generator().manual_seed(6))
    minibatch_check(alg, mode, "cpu")


def test_default_path_builds_no_smooth_state():
    alg = PPO(_policy(), device="cpu")
    assert alg.smooth is None and (alg.mean_smooth_temporal, alg.mean_smooth_spatial) == (0.0, 0.0)
    assert not [k for k, v in vars(alg).items() if "smooth" in k and v is not None and not isinstance(v, float)]


def test_ppo_refusals(monkeypatch):
    from wiki_grx_gym_amd.rl import symmetry as Y
    from wiki_grx_gym_amd.rl.recurrent import ActorCriticRecurrent
    with pytest.raises(ValueError, match="--recurrent") as info:
        PPO(ActorCriticRecurrent(39, 168, 10, rnn_hidden_size=32, actor_hidden_dims=[16], critic_hidden_dims=[16]), device="cpu", smooth="both")
    assert "--smooth" in str(info.value)
    with pytest.raises(ValueError, match="--state_dependent_std") as info:
        PPO(_policy(state_dependent_std=True, noise_std_type="log"), device="cpu", smooth="spatial")
    assert "--smooth" in str(info.value)
    lower = [f"{s}_{j}_joint" for s in ("left", "right") for j in ("hip_roll", "hip_yaw", "hip_pitch", "knee_pitch", "ankle_pitch")]
    pts = [round(-0.5 + 0.1 * i, 1) for i in range(11)]
    maps = Y.SymmetryMaps(Y.MirrorMap(*Y.frame_map(lower), "cpu"), Y.MirrorMap(*Y.privileged_map(lower, pts, pts), "cpu"),
                          Y.MirrorMap(*Y.joint_map(lower), "cpu"))
    with pytest.raises(ValueError, match="--symmetry") as info:
        PPO(_policy(), device="cpu", symmetry="loss", symmetry_maps=maps, smooth="temporal")
    assert "--smooth" in str(info.value) and "both extend the minibatch" in str(info.value)
    with pytest.raises(ValueError, match="smooth must be one of"):
        PPO(_policy(), device="cpu", smooth="sideways")
    for kw in (dict(smooth_temporal_coef=-0.1), dict(smooth_spatial_coef=float("nan")), dict(smooth_sigma=float("inf")), dict(smooth_sigma=-1.0)):
        with pytest.raises(ValueError, match="--smooth") as info:
            PPO(_policy(), device="cpu", smooth="both", **kw)
        assert "--" + list(kw)[0] in str(info.value)
    for mode, ok in (("temporal", False), ("both", False), ("spatial", True)):
        alg = PPO(_policy(), device="cpu", smooth=mode)
        if ok:
            alg.init_storage(8, 1)
        else:
            with pytest.raises(ValueError, match="num_transitions_per_env") as info:
                alg.init_storage(8, 1)
            assert "--smooth" in str(info.value)
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    monkeypatch.setattr(dist, "get_rank", lambda *a: 0)
    with pytest.raises(NotImplementedError, match="world size") as info:
        PPO(_policy(), device="cpu", smooth="both")
    assert "--smooth" in str(info.value)


class _NoEnv:
    num_envs, num_obs, num_pri_obs, num_actions = 8, 39, 168, 10
    dof_names = []

    def reset(self):
        return None


def _train_cfg(steps=6):
    tcfg = GR1T1CfgPPO()
    tcfg.runner.num_steps_per_env = steps
    tcfg.algorithm.num_mini_batches, tcfg.algorithm.num_learning_epochs = 3, 2
    tcfg.policy.actor_hidden_dims, tcfg.policy.critic_hidden_dims = [32, 16], [32, 16]
    return tcfg


def _cfg_dict(flags=("--smooth", "both"), runner=(), algorithm=(), policy=(), steps=6):
    d = class_to_dict(update_cfg_from_args(None, _train_cfg(steps), get_args(list(flags)))[1])
    d["runner"].update(runner); d["algorithm"].update(algorithm); d["policy"].update(policy)
    return d


def test_runner_refusals(monkeypatch, tmp_path):
    r = OnPolicyRunner(_NoEnv(), _cfg_dict(), None, "cpu")                                          # the flag alone is fine
    assert r.smooth == "both" and r.alg.smooth == "both" and (r.alg.smooth_temporal_coef, r.alg.smooth_spatial_coef, r.alg.smooth_sigma) == (0.1, 0.1, 0.05)
    for keys in (dict(runner={"empirical_normalization": True}), dict(runner={"obs_history_length": 3, "critic_obs_history_length": 2}),
                 dict(runner={"privileged_actor": True}), dict(algorithm={"rnd": True}), dict(policy={"noise_std_type": "log"})):
        OnPolicyRunner(_NoEnv(), _cfg_dict(**keys), None, "cpu")                                    # ... and with what it composes with
    for keys, exc, other in ((dict(runner={"policy_class_name": "ActorCriticRecurrent"}, policy={"rnn_hidden_size": 32}), ValueError, "--recurrent"),
                             (dict(algorithm={"symmetry": "loss"}), ValueError, "--symmetry"),
                             (dict(policy={"state_dependent_std": True, "noise_std_type": "log"}), ValueError, "--state_dependent_std"),
                             (dict(runner={"distill_from": str(tmp_path / "teacher.pt")}), ValueError, "--distill_from"),
                             (dict(runner={"exact_resume": True}), NotImplementedError, "--exact_resume"),
                             (dict(algorithm={"smooth_temporal_coef": -1.0}), ValueError, "--smooth_temporal_coef"),
                             (dict(algorithm={"smooth_spatial_coef": float("inf")}), ValueError, "--smooth_spatial_coef"),
                             (dict(algorithm={"smooth_sigma": float("nan")}), ValueError, "--smooth_sigma"),
                             (dict(steps=1), ValueError, "num_steps_per_env")):
        with pytest.raises(exc, match=other) as info:
            OnPolicyRunner(_NoEnv(), _cfg_dict(**keys), None, "cpu")
        assert "--smooth" in str(info.value), keys                                                  # the message names both options
    OnPolicyRunner(_NoEnv(), _cfg_dict(flags=("--smooth", "spatial"), steps=1), None, "cpu")        # (no successor rows needed)
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    monkeypatch.setattr(dist, "get_rank", lambda *a: 0)
    with pytest.raises(NotImplementedError, match="world size") as info:
        OnPolicyRunner(_NoEnv(), _cfg_dict(), None, "cpu")
    assert "--smooth" in str(info.value)


def test_cli_flags_reach_the_configs():
    a = get_args([])
    assert a.smooth is None and (a.smooth_temporal_coef, a.smooth_spatial_coef, a.smooth_sigma) == (0.1, 0.1, 0.05)
    d = class_to_dict(update_cfg_from_args(None, config.GR1T1CfgPPO(), get_args(["--smooth_sigma", "0.2"]))[1])
    assert not [k for k in d["algorithm"] if k.startswith("smooth")]                              # without --smooth: nothing
    d = class_to_dict(update_cfg_from_args(None, config.GR1T1CfgPPO(), get_args(["--smooth", "temporal", "--smooth_temporal_coef", "0.3"]))[1])
    assert {k: v for k, v in d["algorithm"].items() if k.startswith("smooth")} == {"smooth": "temporal", "smooth_temporal_coef": 0.3,
                                                                                   "smooth_spatial_coef": 0.1, "smooth_sigma": 0.05}
    for cls in (config.GR1T1CfgPPO, config.GR1T2CfgPPO, config.GR1T1FullBodyCfgPPO):               # not config keys
        assert not [k for k in vars(cls.algorithm) if k.startswith("smooth")]
    with pytest.raises(SystemExit):
        get_args(["--smooth", "sideways"])


def _make(tmp_path, flags=(), env_cfg=None, steps=6):
    args = get_args(["--task", "GR1T1", "--headless", "--num_envs", "16", "--sim_device", "cpu", "--rl_device", "cpu", "--pipeline", "cpu",
                     "--seed", "3", *flags])
    env, _ = task_registry.make_env("GR1T1", args=args, env_cfg=env_cfg if env_cfg is not None else GR1T1Cfg())
    runner, _ = task_registry.make_alg_runner(env, name=None, args=args, train_cfg=_train_cfg(steps), log_root=str(tmp_path) if tmp_path else None)
    return env, runner


def _tags(runner):
    return {line.split('"tag": "')[1].split('"')[0]: float(line.split('"value": ')[1].split(",")[0]) for line in open(os.path.join(runner.log_dir, "scalars.jsonl"))}


@pytest.mark.parametrize("flags", [("--smooth", "both"), ("--smooth", "temporal", "--empirical_normalization", "--obs_history", "3")])
def test_one_update_through_the_runner(oracle_backend, tmp_path, flags):  # noqa: F811
    cfg = GR1T1Cfg()
    cfg.env.episode_length_s = 0.1           # 5 steps: every env times out inside the rollout, so some pairs are masked by a done
    _, runner = _make(tmp_path / "smooth", flags, env_cfg=cfg)
    alg = runner.alg
    before = [p.detach().clone() for p in alg.actor_critic.parameters()]
    seen, update = [], alg.update

    def snap_then_update():
        seen.append(int(alg.storage.dones.sum()))
        return update()
    alg.update = snap_then_update
    runner.learn(num_learning_iterations=1)
    assert seen and seen[0] >= 16
    assert all(not torch.equal(a, b) and bool(torch.isfinite(b).all()) for a, b in zip(before, alg.actor_critic.parameters()))
    tags = _tags(runner)
    temporal, spatial = tags["Loss/smooth_temporal"], tags["Loss/smooth_spatial"]
    assert np.isfinite(temporal) and temporal > 0 and temporal == alg.mean_smooth_temporal
    if "both" in flags:
        assert np.isfinite(spatial) and spatial > 0 and spatial == alg.mean_smooth_spatial
        assert alg._smooth_bufs[0].shape == (3 * 32, 39)
    else:
        assert spatial == 0.0 and alg._smooth_bufs[0].shape == (2 * 32, 3 * 39)
    plain_flags = tuple(f for f in flags if not f.startswith("--smooth") and f not in R.MODES)
    _, plain = _make(tmp_path / "plain", plain_flags)
    plain.learn(num_learning_iterations=1)
    assert plain.alg.smooth is None and "Loss/smooth_temporal" not in _tags(plain)
    ck = torch.load(os.path.join(runner.log_dir, "model_1.pt"), weights_only=False)
    ck_plain = torch.load(os.path.join(plain.log_dir, "model_1.pt"), weights_only=False)
    assert set(ck) == set(ck_plain) and set(ck["model_state_dict"]) == set(ck_plain["model_state_dict"])
    plain.load(os.path.join(runner.log_dir, "model_1.pt"))                                       # a policy trained with it loads like any other
    loaded = plain.alg.actor_critic.state_dict()
    assert all(torch.equal(v, loaded[k]) for k, v in alg.actor_critic.state_dict().items() if k != "std")
