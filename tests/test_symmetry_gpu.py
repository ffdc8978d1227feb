"""Left-right symmetry on the MI355X (rl/symmetry.py, csrc/grx_ppo_sym.hip): grx_sym_gather_rows against numpy and its
argument checks, the observation map on the HIP step kernels' post-physics half (physically mirrored records), one minibatch step of every
mode against float64 and against the torch gather, the captured step against the eager one, and the runner."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import symmetry_ref as R
from tests.helpers import make_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PTS = [round(-0.5 + 0.1 * i, 1) for i in range(11)]
LOWER = ['left_hip_roll_joint', 'left_hip_yaw_joint', 'left_hip_pitch_joint', 'left_knee_pitch_joint', 'left_ankle_pitch_joint',
         'right_hip_roll_joint', 'right_hip_yaw_joint', 'right_hip_pitch_joint', 'right_knee_pitch_joint', 'right_ankle_pitch_joint']


def _S():
    from wiki_grx_gym_amd.rl import symmetry
    return symmetry


def _lib():
    from wiki_grx_gym_amd.rl.fused_loss import load_ppo_library
    return load_ppo_library()


def _random_map(w, g, affine):
    """(perm int32, scale, offset or None) on the device: any permutation; scale +-1, or an affine map"""
    perm = torch.randperm(w, generator=g).to(torch.int32)
    if affine:
        return perm.to(DEV), torch.randn(w, generator=g).to(DEV), torch.randn(w, generator=g).to(DEV)
    return perm.to(DEV), (torch.randint(0, 2, (w,), generator=g).float() * 2 - 1).to(DEV), None


def _call(srcs, dsts, modes, maps, idx, mb, n=None, widths=None):
    n = len(srcs) if n is None else n
    k = len(srcs)
    P = lambda t: t.data_ptr() if t is not None else None
    arr = lambda vals: (C.c_void_p * k)(*vals)
    w = (C.c_int * k)(*(widths if widths is not None else [(s if s is not None else d).shape[1] for s, d in zip(srcs, dsts)]))
    return _lib().grx_sym_gather_rows(n, arr([P(s) for s in srcs]), arr([P(d) for d in dsts]), w, (C.c_int * k)(*modes),
                                      arr([P(m[0]) if m else None for m in maps]), arr([P(m[1]) if m else None for m in maps]),
                                      arr([P(m[2]) if m else None for m in maps]), P(idx), mb, None)


def _np_maps(maps):
    return [(m[0].cpu().numpy().astype(np.int64), m[1].double().cpu().numpy(), m[2].double().cpu().numpy() if m[2] is not None else None) if m else None
            for m in maps]


@pytest.mark.parametrize("widths", [(1, 10, 39), (168, 117, 32)])
@pytest.mark.parametrize("mb", [1, 63, 65, 300])
def test_gather_against_numpy(mb, widths):
    """three tensors at once, modes 0 / 1 / 2 mixed (rotated so that every width meets every mode), a random idx with repeats into 4 mb
    source rows; scale = +-1 without an offset: both halves equal the numpy gather BY VALUE; an affine map: within
    2^-23 (|scale x| + |offset|), the rounding of a separate multiply and add, which bounds the fmaf too; idx == NULL; a second call
    reproduces the first bit for bit."""
    g = torch.Generator().manual_seed(100 * mb + widths[0])
    srcs = [torch.randn(4 * mb, w, generator=g).to(DEV) for w in widths]
    idx = torch.randint(0, 4 * mb, (mb,), generator=g).to(DEV)
    if mb > 1:
        idx[-1] = idx[0]                                                                          # (a repeat for certain)
    for rot in range(3):
        modes = [(t + rot) % 3 for t in range(3)]
        for affine in (False, True):
            maps = [_random_map(w, g, affine) if m == 2 else None for w, m in zip(widths, modes)]
            for use_idx in (idx, None):
                dsts = [torch.full((mb * (2 if m else 1), w), 777.0, device=DEV) for w, m in zip(widths, modes)]
                assert _call(srcs, dsts, modes, maps, use_idx, mb) == 0
                again = [torch.full_like(d, -1.0) for d in dsts]
                assert _call(srcs, again, modes, maps, use_idx, mb) == 0
                torch.cuda.synchronize()
                want = R.gather_np([s.cpu().numpy() for s in srcs], modes, _np_maps(maps), None if use_idx is None else use_idx.cpu().numpy(), mb)
                for t, (d, a, wnt, m) in enumerate(zip(dsts, again, want, modes)):
                    got = d.double().cpu().numpy()
                    assert torch.equal(d, a)
                    np.testing.assert_array_equal(got[:mb], wnt[:mb])
                    if m == 1 or (m == 2 and not affine):
                        np.testing.assert_array_equal(got[mb:], wnt[mb:])
                    elif m == 2:
                        perm, scale, offset = _np_maps(maps)[t]
                        lim = 2.0 ** -23 * (np.abs(scale * wnt[:mb][:, perm]) + np.abs(offset))
                        assert (np.abs(got[mb:] - wnt[mb:]) <= lim).all(), (mb, widths, t, np.abs(got[mb:] - wnt[mb:]).max())


def test_rows_do_not_depend_on_the_minibatch():
    """row r of an mb = 300 call equals an mb = 1 call on that row, bit for bit (affine map, three tensors)"""
    g = torch.Generator().manual_seed(9)
    widths, mb, modes = (168, 117, 32), 300, [2, 2, 1]
    srcs = [torch.randn(4 * mb, w, generator=g).to(DEV) for w in widths]
    maps = [_random_map(168, g, True), _random_map(117, g, True), None]
    idx = torch.randint(0, 4 * mb, (mb,), generator=g).to(DEV)
    dsts = [torch.zeros(2 * mb, w, device=DEV) for w in widths]
    assert _call(srcs, dsts, modes, maps, idx, mb) == 0
    for r in (0, 3, 64, 255, 299):
        one = [torch.zeros(2, w, device=DEV) for w in widths]
        assert _call(srcs, one, modes, maps, idx[r:r + 1].contiguous(), 1) == 0
        torch.cuda.synchronize()
        for d, o in zip(dsts, one):
            assert torch.equal(d[r], o[0]) and torch.equal(d[mb + r], o[1])


def test_invalid_arguments_leave_the_outputs_untouched():
    g = torch.Generator().manual_seed(1)
    mb, widths, modes = 8, (5, 39), [2, 1]
    srcs = [torch.randn(16, w, generator=g).to(DEV) for w in widths]
    maps = [_random_map(5, g, True), None]
    idx = torch.randint(0, 16, (mb,), generator=g).to(DEV)
    dsts = [torch.full((2 * mb, w), 777.0, device=DEV) for w in widths]
    call = lambda **kw: _call(**{**dict(srcs=srcs, dsts=dsts, modes=modes, maps=maps, idx=idx, mb=mb), **kw})
    assert call(mb=0) < 0 and call(mb=-3) < 0
    assert call(n=0) < 0
    thirteen = dict(srcs=[srcs[1]] * 13, dsts=[dsts[1]] * 13, modes=[1] * 13, maps=[None] * 13)
    assert call(**thirteen) < 0                                                               # above GRX_PPO_GATHER_MAX
    assert call(widths=[0, 39]) < 0 and call(widths=[5, -1]) < 0 and call(widths=[5, 2049]) < 0   # above GRX_SYM_MAX_WIDTH
    assert call(modes=[3, 1]) < 0 and call(modes=[2, -1]) < 0
    assert call(maps=[None, None]) < 0                                                        # mode 2 without perm / scale
    assert call(maps=[(maps[0][0], None, None), None]) < 0 and call(maps=[(None, maps[0][1], None), None]) < 0
    assert call(srcs=[None, srcs[1]]) < 0 and call(dsts=[dsts[0], None]) < 0
    lib = _lib()
    one = (C.c_void_p * 1)(srcs[0].data_ptr())
    assert lib.grx_sym_gather_rows(1, None, one, (C.c_int * 1)(5), (C.c_int * 1)(1), None, None, None, None, mb, None) < 0
    assert lib.grx_sym_gather_rows(1, one, None, (C.c_int * 1)(5), (C.c_int * 1)(1), None, None, None, None, mb, None) < 0
    torch.cuda.synchronize()
    assert all(bool((d == 777.0).all()) for d in dsts)
    assert call() == 0 and call(maps=[(maps[0][0], maps[0][1], None), None]) == 0 and call(idx=None) == 0    # ... and the valid calls do write
    torch.cuda.synchronize()
    assert not any(bool((d == 777.0).any()) for d in dsts)


# ---- the observation map on the HIP kernels' post-physics half ---------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [1, 4, "quad", "tree", "tree16", "full_body", "full_body16"])
def test_observation_map_on_mirrored_states_through_the_hip_kernels(layout, monkeypatch):
    """tests/test_symmetry.py's mirrored-record check through grx_debug_post_physics: one layout per kernel family tests/test_hip_golden.py
    covers (one wave, the lane-pair pipeline, the lane-quad pipeline, the tree kernel with 8 and -- a kernel of its own, grx_step_tree16 --
    with 16 lanes per env) and both tree kernels on the 32-DOF full body, at 1e-4"""
    from tests import test_oracle_golden as og
    from tests.test_hip_golden import make_hip
    from tests.test_symmetry import check_mirrored_records
    from wiki_grx_gym_amd.sim import HipSim
    from wiki_grx_gym_amd.envs import build_config
    from wiki_grx_gym_amd import model as grx_model
    if layout in ("full_body", "full_body16"):
        from tests.test_hip_golden import KERNEL_OF
        name, lanes, _ = KERNEL_OF["tree16" if layout == "full_body16" else "tree"]
        monkeypatch.delenv("GRX_FORCE_GENERIC", raising=False)
        monkeypatch.setenv("GRX_TREE", "1")
        monkeypatch.setenv("GRX_TREE_G", str(lanes))

        def make(N):
            cfg, c, keep, _ = og.make_other_robot("full_body", N, noise=False)
            sim = HipSim(c, DEV, keep)
            assert sim.layout()["kernel"].startswith(name) and sim.layout()["lanes_per_env"] == lanes, sim.layout()   # ("grx_step_tree<" / "grx_step_tree16<")
            return sim
        worst = check_mirrored_records(make, "pipeline_full_body.npz", "in_", list(grx_model.RobotModel("gr1t1").dof_names), 1e-4, True)
    else:
        make = lambda N: make_hip(make_cfg(noise=False, dr=False), N, layout=layout, monkeypatch=monkeypatch)[0]
        worst = check_mirrored_records(make, "pipeline.npz", "s0_in_", LOWER, 1e-4, True)
    print("mirrored records, worst error / tolerance:", layout, worst)


# ---- one minibatch step with symmetry ------------------------------------------------------------------------------------------------------
def _setup(mode, monkeypatch, graph="1", seed=5, hidden=(512, 256, 128)):
    """PPO with symmetry on 64 envs x 8 steps, 4 minibatches, a storage of consistent random data and normalisers whose statistics are
    deliberately asymmetric (a dropped offset, a scale without the std ratio would show)"""
    from wiki_grx_gym_amd.rl.modules import ActorCriticMLP
    from wiki_grx_gym_amd.rl.normalizer import EmpiricalNormalization
    from wiki_grx_gym_amd.rl.ppo import PPO
    S = _S()
    monkeypatch.setenv("GRX_PPO_GRAPH", graph)
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed + 1)
    norms = []
    for w in (39, 168):
        n = EmpiricalNormalization(w).to(DEV)
        n.update((torch.randn(600, w, generator=g) * torch.linspace(0.3, 2.5, w) + torch.linspace(-1.5, 2.0, w)).to(DEV))
        norms.append(n)
    maps = S.SymmetryMaps(S.MirrorMap(*S.frame_map(LOWER), DEV), S.MirrorMap(*S.privileged_map(LOWER, PTS, PTS), DEV),
                          S.MirrorMap(*S.joint_map(LOWER), DEV), *norms)
    ac = ActorCriticMLP(39, 168, 10, actor_hidden_dims=list(hidden), critic_hidden_dims=list(hidden), activation="elu", init_noise_std=0.4)
    alg = PPO(ac, num_learning_epochs=2, num_mini_batches=4, clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.01, schedule="adaptive",
              desired_kl=0.01, learning_rate=1e-3, device=DEV, symmetry=mode, symmetry_coef=0.8, symmetry_maps=maps)
    alg.init_storage(64, 8)
    _fill(alg, g)
    return alg, maps, norms


def _fill(alg, g):
    st, ac = alg.storage, alg.actor_critic
    T, N = 8, 64
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)
    with torch.no_grad():
        st.observations.copy_(r(T, N, 39)); st.pri_observations.copy_(r(T, N, 168))
        mu, value = ac.actor(st.observations.flatten(0, 1)), ac.critic(st.pri_observations.flatten(0, 1))
        std = ac.std.detach()
        st.mu.copy_((mu + 0.1 * std * r(T * N, 10)).view(T, N, 10))
        st.sigma.copy_((std * (1.0 + 0.1 * torch.rand(T * N, 10, generator=g).to(DEV))).view(T, N, 10))
        st.actions.copy_((mu + std * r(T * N, 10)).view(T, N, 10))
        logp = torch.distributions.Normal(mu, std).log_prob(st.actions.flatten(0, 1)).sum(-1, keepdim=True)
        st.actions_log_prob.copy_((logp + 0.2 * r(T * N, 1)).view(T, N, 1))
        st.values.copy_((value + 0.2 * r(T * N, 1)).view(T, N, 1))
        st.returns.copy_((value + r(T * N, 1)).view(T, N, 1))
        st.advantages.copy_(r(T, N, 1))
    st.step = T


def _ref_maps(maps, norms):
    """the float64 maps, from the normalisers' statistics by tests/symmetry_ref.normalized_ref"""
    S = _S()
    out = {}
    for key, pm, n in (("obs", S.frame_map(LOWER), norms[0]), ("cobs", S.privileged_map(LOWER, PTS, PTS), norms[1])):
        perm, sign = np.array(pm[0]), np.array(pm[1])
        out[key] = (perm,) + R.normalized_ref(perm, sign, n._mean[0].double().cpu().numpy(), n._std[0].double().cpu().numpy(), n.eps)
    jp, js = R.joint_map_ref(LOWER)
    out["actions"] = (jp, js, None)
    return out


def _step_grads(alg, idx):
    srcs = alg._sym_sources()
    mb = idx.numel()
    bufs = [torch.zeros(mb * (2 if m else 1), s.shape[1], device=DEV) for m, s in zip(alg._sym_modes, srcs)]
    alg._sym_gatherer(srcs, bufs)(idx)
    with alg._blas_for_update():
        s, v, loss, kl = alg._losses_sym(*bufs)
        alg.optimizer.zero_grad(set_to_none=True)
        loss.backward()
    torch.cuda.synchronize()
    return bufs, torch.stack([s, v, loss, kl]).detach().double().cpu(), [p.grad.detach().clone() for p in alg.actor_critic.parameters()]


@pytest.mark.parametrize("mode", ["augment", "loss", "both"])
def test_minibatch_gradients_match_float64_and_the_torch_gather(mode, monkeypatch):
    """One minibatch (128 of 512 rows) of every mode: all parameter gradients against float64 autograd of tests/symmetry_ref within
    1e-4 max |g_ref| per tensor (the bound of test_minibatch_parameter_gradients_match_float64), with grx_sym_gather_rows and with
    GRX_SYM_FUSED=0; the two gathers' buffers agree (first halves and sign-only maps by value, the normalised maps within the rounding of a
    separate multiply and add)."""
    alg, maps, norms = _setup(mode, monkeypatch, graph="0")
    idx = torch.randperm(512, generator=torch.Generator().manual_seed(3))[:128].to(DEV)
    srcs = alg._sym_sources()
    batch = [s[idx] for s in srcs]
    ac64 = copy.deepcopy(alg.actor_critic).double().cpu()
    ref = R.augmented_loss_ref(ac64, batch, _ref_maps(maps, norms), mode, 0.8, 0.2, 1.0, 0.01, True)
    assert ref["sym"] > 1e-3
    results = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("GRX_SYM_FUSED", fused)
        alg._sym_sum.zero_()
        bufs, out, grads = _step_grads(alg, idx)
        results[fused] = bufs
        assert abs(float(alg._sym_sum) - ref["sym"]) <= 1e-4 * ref["sym"], (fused, float(alg._sym_sum), ref["sym"])
        assert (out - ref["out"]).abs().max() <= 1e-4 * ref["out"].abs().max(), (fused, out, ref["out"])
        for (n, _), got, want in zip(alg.actor_critic.named_parameters(), grads, ref["grads"]):
            err, lim = float((got.double().cpu() - want).abs().max()), 1e-4 * float(want.abs().max())
            print(f"{mode} GRX_SYM_FUSED={fused} {n}: max err {err:.3e}, bound {lim:.3e}")
            assert err <= lim, (mode, fused, n, err, lim)
    rm = _ref_maps(maps, norms)
    which = {0: rm["obs"], 1: rm["cobs"], 2: rm["actions"], 7: rm["actions"], 8: (rm["actions"][0], np.abs(rm["actions"][1]), None)}
    for t, (a, b, full) in enumerate(zip(results["1"], results["0"], ref["full"])):
        mb = 128
        assert torch.equal(a[:mb], b[:mb]) and torch.equal(a[:mb].double().cpu(), full[:mb].reshape(a[:mb].shape))
        if a.shape[0] > mb and alg._sym_modes[t] == 1:
            assert torch.equal(a[mb:], a[:mb]) and torch.equal(b[mb:], a[:mb])
        elif a.shape[0] > mb:
            # fp32 scale and offset (three roundings each from the statistics) and the product-sum: 2^-22 (|scale x| + |offset|) covers them
            perm, scale, offset = which[t]
            lim = 2.0 ** -22 * (np.abs(scale * full[:mb].numpy()[:, perm]) + (np.abs(offset) if offset is not None else 0.0))
            for got in (a, b):
                assert (np.abs(got[mb:].double().cpu().numpy() - full[mb:].numpy()) <= lim).all(), (t, fused)


def test_captured_update_equals_the_eager_one(monkeypatch):
    """--symmetry both: two updates under GRX_PPO_GRAPH=1 and GRX_PPO_GRAPH=0 from the same state give bit-identical parameters (the
    property the default path is held to), the same learning rate and the same mean mirror loss"""
    got = {}
    for graph in ("1", "0"):
        alg, _, _ = _setup("both", monkeypatch, graph=graph, hidden=(64, 32))
        assert alg._use_graph == (graph == "1")
        torch.manual_seed(77)
        stats = [alg.update(), alg.update()]
        torch.cuda.synchronize()
        if graph == "1":
            assert isinstance(alg._graph, torch.cuda.CUDAGraph) and type(alg._gather).__name__ == "SymGather" and alg._static[0].shape[0] == 256
        got[graph] = ([p.detach().clone() for p in alg.actor_critic.parameters()], stats, alg.learning_rate, alg.mean_symmetry_loss)
    for a, b in zip(got["1"][0], got["0"][0]):
        assert torch.equal(a, b)
    assert got["1"][1:] == got["0"][1:] and got["1"][3] > 0


# ---- the runner ------------------------------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("flags", [("--symmetry", "augment"), ("--symmetry", "loss"), ("--symmetry", "both", "--empirical_normalization"),
                                   ("--symmetry", "both", "--precision", "bf16")])
def test_runner_trains_with_symmetry(tmp_path, flags):
    env, runner = _make(tmp_path, flags)
    alg = runner.alg
    before = [p.detach().clone() for p in alg.actor_critic.parameters()]
    runner.learn(num_learning_iterations=1 if "bf16" in flags else 2)
    assert type(alg._gather).__name__ == "SymGather" and isinstance(alg._graph, torch.cuda.CUDAGraph)
    assert all(not torch.equal(a, b) and bool(torch.isfinite(b).all()) for a, b in zip(before, alg.actor_critic.parameters()))
    tags = _tags(runner)
    assert all(np.isfinite(tags[k]) for k in ("Loss/symmetry", "Loss/value_function", "Loss/surrogate", "Loss/kl")) and tags["Loss/symmetry"] > 0
    it = 1 if "bf16" in flags else 2
    want = {"model_state_dict", "optimizer_state_dict", "iter", "infos"} | ({"obs_norm_state_dict", "critic_obs_norm_state_dict"} if "--empirical_normalization" in flags else set())
    assert set(torch.load(os.path.join(runner.log_dir, f"model_{it}.pt"), weights_only=False)) == want      # the key set of a run without the flag


def test_play_on_a_symmetric_run_and_the_default_path(tmp_path):
    from wiki_grx_gym_amd.scripts.play import play
    from wiki_grx_gym_amd.utils import get_args
    _, runner = _make(tmp_path, ("--symmetry", "both"))
    runner.learn(num_learning_iterations=1)
    out = play(get_args(["--task", "GR1T1", "--headless", "--seed", "3"]), steps=10, log_root=str(tmp_path))     # play.py knows nothing of it
    assert len(open(out["states"]).readlines()) == 10 and out["runner"].alg.symmetry is None
    _, plain = _make(None)
    plain.learn(num_learning_iterations=1)
    assert type(plain.alg._gather).__name__ == "RowGather" and plain.alg.symmetry_coef == 0 and plain.alg.symmetry is None
    assert plain.alg._static[0].shape[0] == 64 * 8 // 4


def test_height_permutation_on_two_ramps_through_the_hip_kernel(monkeypatch):
    """tests/test_symmetry.py's ramp-raster check on the lane-quad pipeline (what 4096 envs run): B's measured heights are A's under the
    map's permutation EXACTLY -- no scan point is within 1e-3 cells of a cell edge, so the allowance tests/test_hip_golden.py grants points
    on an edge is not used (the fp32 oracle needs none on these poses either: tests/test_symmetry.py) --, the height block of pri_obs at 1e-4"""
    from tests.test_hip_golden import pick_layout, KERNEL_OF
    from tests.test_symmetry import check_height_permutation
    from wiki_grx_gym_amd.envs import build_config
    from wiki_grx_gym_amd.sim import HipSim
    pick_layout(monkeypatch, "quad")

    def make(cfg, N, ter):
        c, keep, _ = build_config.build(cfg, cfg.sim.dt, N, terrain=ter)
        sim = HipSim(c, DEV, keep)
        assert sim.layout()["kernel"].startswith(KERNEL_OF["quad"][0]), sim.layout()
        return sim
    check_height_permutation(make, 1e-4)
