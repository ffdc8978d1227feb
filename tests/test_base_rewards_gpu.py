"""legged_gym's base reward terms on the MI355X (`-m gpu`): the grx_step_kernel_base* entries (include/grx.h ABI 7).

tests/golden/base_reward_terms.npz holds the 15 terms and compute_reward's total from the reference's own post_physics_step
(tools/gen_golden.py, every base term at a non-zero scale next to the registered GR1T1 scales); grx_debug_post_physics runs the base
entry's post-physics half on the same injected state.  The product step (no injection) is checked against a numpy restatement of
legged_robot.py:1277-1376 on the tensors it publishes.  The registered tasks keep their kernels (routing test)."""
import numpy as np
import pytest
import torch

from tests import test_oracle_golden as og
from tests.helpers import make_cfg
from tests.test_base_rewards import FIXTURE, base_cfg
from wiki_grx_gym_amd import _capi
from wiki_grx_gym_amd.envs import build_config

pytestmark = pytest.mark.gpu

NB = _capi.NUM_BASE_REWARD_TERMS
ENTRY = {"plane": "grx_step_kernel_base<false, false>", "heightfield": "grx_step_kernel_base<true, false>",
         "trimesh": "grx_step_kernel_base_trimesh<false>"}


TREE_ENTRY = {"plane": "_base<false, false>", "heightfield": "_base<true, false>", "trimesh": "_base_trimesh<false>"}


def make_base_hip(terrain, N=64, task="GR1T1", tree=None, monkeypatch=None):
    """tree = 8 / 16: the lower-limb robot forced through the tree kernel (GRX_FORCE_GENERIC) -- its base entry, the code the full body runs."""
    from wiki_grx_gym_amd.sim import HipSim
    if tree:
        monkeypatch.setenv("GRX_FORCE_GENERIC", "1"); monkeypatch.setenv("GRX_TREE", "1"); monkeypatch.setenv("GRX_TREE_G", str(tree))
    cfg = base_cfg(task=task, terrain="heightfield" if terrain != "plane" else "plane")
    ter = None
    if terrain != "plane":
        ter, _ = og.reference_raster_terrain()
        cfg.terrain.mesh_type = terrain
    c, keep, meta = build_config.build(cfg, cfg.sim.dt, N, terrain=ter)
    sim = HipSim(c, "cuda:0", keep)
    lay = sim.layout()
    if tree:
        assert lay["kernel"] == ("grx_step_tree16" if tree == 16 else "grx_step_tree") + TREE_ENTRY[terrain] and lay["lanes_per_env"] == tree, lay
    else:
        assert lay["kernel"] == ENTRY[terrain] and lay["lanes_per_env"] == 2 and lay["waves_per_block"] == 1, lay
    return sim, cfg, meta


@pytest.mark.parametrize("tree", [None, 8, 16])
@pytest.mark.parametrize("terrain", ["plane", "heightfield", "trimesh"])
def test_every_base_term_on_the_base_entry(terrain, tree, monkeypatch):
    """Each of the 15 terms (GRX_T_BASE_REWARD_TERMS, scaled) and the total (GRX_T_REW: both tables, termination after the clip) equal
    the reference's at 1e-4.  Plane: the fixture's plane case; heightfield / trimesh: its case on the reference raster (base_height reads
    the kernel's own scan of this step)."""
    d = np.load(FIXTURE)
    case = "plane" if terrain == "plane" else "rough"
    sim, cfg, meta = make_base_hip(terrain, tree=tree, monkeypatch=monkeypatch)
    assert [n for n in meta["active_terms"] if n != "termination"] == list(map(str, d[case + "_reward_names"]))   # (the reference's list leaves termination out)
    N = d[case + "_in_root"].shape[0]
    og.inject(sim, og.states_from(d, case + "_in_", N), common_step_counter=1, noise_uniform=torch.tensor(d[case + "_noise_u"]).contiguous())
    dt = cfg.control.decimation * cfg.sim.dt
    # the fixture evaluates the terms on the injected commands; the step first redraws those of rows whose episode length hits the
    # resampling interval (legged_robot.py:315-317)
    rows = (d[case + "_in_episode_length"] + 1) % int(cfg.commands.resampling_command_interval_s / dt) != 0
    assert rows.sum() >= N - 4
    got = sim.tensor("BASE_REWARD_TERMS").cpu().numpy()
    names = list(map(str, d["names"]))
    tol = 1e-4
    for t, n in enumerate(_capi.BASE_REWARD_TERMS):
        want = d[case + "_values"][names.index(n)][rows] * d["scales"][names.index(n)] * dt
        err = np.abs(got[t][rows] - want)
        assert (err <= tol + tol * np.abs(want)).all(), f"{n}: max err {err.max():.3e}"
    rew = sim.tensor("REW").cpu().numpy()[rows]
    want = d[case + "_rew"][rows]
    err = np.abs(rew - want)
    assert (err <= tol + tol * np.abs(want)).all(), f"total: max err {err.max():.3e}"


@pytest.mark.parametrize("task,kernel", [("GR1T1", "grx_step_kernel_base<true, false>"), ("GR1T1_full_body", "grx_step_tree16_base<true, false>"),
                                         ("GR1T1_full_body", "grx_step_tree_base<true, false>"), ("GR1T1_full_body", "grx_step_generic_base<true>")])
def test_product_step_matches_a_numpy_restatement(task, kernel, monkeypatch):
    """Each product entry (no injection) on the rough raster: after every step of a rollout with random actions, the 15 terms of the rows
    that did not reset, restated in numpy from the tensors the step publishes (legged_robot.py:1277-1376).  The full body on the tree
    kernel with 16 and 8 lanes per env and on the one-lane generic kernel (GRX_TREE=0)."""
    from wiki_grx_gym_amd.envs import GR1T1Cfg, GR1T1FullBodyCfg
    from wiki_grx_gym_amd.utils import get_args, task_registry
    if "generic" in kernel:
        monkeypatch.setenv("GRX_TREE", "0")
    elif "tree" in kernel:
        monkeypatch.setenv("GRX_TREE", "1"); monkeypatch.setenv("GRX_TREE_G", "16" if "tree16" in kernel else "8")
    N = 512 if task == "GR1T1" else 256
    args = get_args(["--task", task, "--headless", "--num_envs", str(N), "--seed", "3"])
    cfg = GR1T1Cfg() if task == "GR1T1" else GR1T1FullBodyCfg()
    cfg.terrain.mesh_type = "heightfield"
    d = np.load(FIXTURE)
    scales = dict(zip(map(str, d["names"]), map(float, d["scales"])))
    for n, v in scales.items():
        setattr(cfg.rewards.scales, n, v)
    cfg.env.publish_reward_terms = True
    env, _ = task_registry.make_env(task, args=args, env_cfg=cfg)
    assert env._sim.layout()["kernel"] == kernel
    env.reset()
    g = torch.Generator(device="cuda").manual_seed(0)
    rw = env.cfg.rewards
    lo, hi = env.dof_pos_limits[:, 0].cpu().numpy(), env.dof_pos_limits[:, 1].cpu().numpy()
    vlim, tlim = env.dof_vel_limits.cpu().numpy(), env.torque_limits.cpu().numpy()
    checked = 0
    for step in range(12):
        a_last = env.actions.detach().cpu().numpy().copy()
        qd_last = env.dof_vel.detach().cpu().numpy().copy()
        act = torch.randn(N, env.num_actions, device="cuda", generator=g) * 0.8
        _, _, _, done, _ = env.step(act)
        torch.cuda.synchronize()
        live = ~done.cpu().numpy()
        q, qd = env.dof_pos.cpu().numpy(), env.dof_vel.cpu().numpy()
        a, tau = env.actions.cpu().numpy(), env.torques.cpu().numpy()
        F = env._sim.tensor("FEET_CONTACT_FORCE").cpu().numpy()
        blv, bav, pg = env.base_lin_vel.cpu().numpy(), env.base_ang_vel.cpu().numpy(), env.base_projected_gravity.cpu().numpy()
        cmd = env.commands.cpu().numpy()
        z = env.root_states[:, 2].cpu().numpy()
        mh = env.measured_heights.cpu().numpy()
        r = {
            "action_rate": ((a_last - a) ** 2).sum(1),
            "ang_vel_xy": (bav[:, :2] ** 2).sum(1),
            "base_height": ((z[:, None] - mh).mean(1) - rw.base_height_target) ** 2,
            "dof_acc": (((qd - qd_last) / env.dt) ** 2).sum(1),
            "dof_pos_limits": (-np.minimum(q - lo, 0) + np.maximum(q - hi, 0)).sum(1),
            "dof_vel": (qd ** 2).sum(1),
            "dof_vel_limits": np.clip(np.abs(qd) - vlim * rw.soft_dof_vel_limit, 0, 1).sum(1),
            "feet_contact_forces": np.maximum(np.linalg.norm(F, axis=-1) - rw.max_contact_force, 0).sum(1),
            "lin_vel_z": blv[:, 2] ** 2,
            "orientation": (pg[:, :2] ** 2).sum(1),
            "stumble": (np.linalg.norm(F[..., :2], axis=-1) > 5 * np.abs(F[..., 2])).any(1).astype(np.float64),
            "torque_limits": np.maximum(np.abs(tau) - tlim * rw.soft_torque_limit, 0).sum(1),
            "torques": (tau ** 2).sum(1),
            "tracking_ang_vel": np.exp(-(cmd[:, 2] - bav[:, 2]) ** 2 / rw.tracking_sigma),
            "tracking_lin_vel": np.exp(-((cmd[:, :2] - blv[:, :2]) ** 2).sum(1) / rw.tracking_sigma),
        }
        got = env._sim.tensor("BASE_REWARD_TERMS").cpu().numpy()
        # (stumble is a comparison: rows within fp32 rounding of |F_xy| = 5 |F_z| may go either way)
        fxy, fz5 = np.linalg.norm(F[..., :2], axis=-1), 5 * np.abs(F[..., 2])
        sharp = live & ~(np.abs(fxy - fz5) <= 1e-4 * (fxy + fz5) + 1e-6).any(1)
        for t, n in enumerate(_capi.BASE_REWARD_TERMS):
            rows = sharp if n == "stumble" else live
            want = r[n][rows] * scales[n] * env.dt
            err = np.abs(got[t][rows] - want)
            assert (err <= 2e-4 + 1e-4 * np.abs(want)).all(), (step, n, float(err.max()))
            checked += 1
    assert checked == 12 * NB


def test_registered_tasks_keep_their_kernels():
    """A handle with a base term (or the command curriculum) runs the base entry of its layout; the registered GR1T1 config keeps the layout
    the parent picks (4096 envs: the lane-quad pipeline with eight waves; 32768 envs: the one-wave kernel), the full body at 4096 envs the
    16-lane tree kernel with the same lanes and waves with and without base terms."""
    from wiki_grx_gym_amd.sim import GrxError, HipSim
    for N, want in ((4096, ("grx_step_kernel_quad<false, 8, false>", 4, 8)), (32768, ("grx_step_kernel<false, 1, false>", 2, 1))):
        cfg = make_cfg()
        c, keep, _ = build_config.build(cfg, cfg.sim.dt, N)
        lay = HipSim(c, "cuda:0", keep).layout()
        assert (lay["kernel"], lay["lanes_per_env"], lay["waves_per_block"]) == want, lay
        cfg = make_cfg()
        cfg.rewards.scales.lin_vel_z = -2.0
        c, keep, _ = build_config.build(cfg, cfg.sim.dt, N)
        lay = HipSim(c, "cuda:0", keep).layout()
        assert (lay["kernel"], lay["lanes_per_env"], lay["waves_per_block"]) == (ENTRY["plane"], 2, 1), lay
    cfg = make_cfg()
    c, keep, _ = build_config.build(cfg, cfg.sim.dt, 64)
    with pytest.raises(GrxError, match="base reward term tensors"):
        HipSim(c, "cuda:0", keep).tensor("BASE_EPISODE_SUMS")
    lays = []
    for base in (False, True):
        cfg = base_cfg(task="GR1T1Full", terrain="heightfield") if base else make_cfg("GR1T1Full", terrain="heightfield")
        if base:
            cfg.commands.curriculum = True
        ter, _ = og.reference_raster_terrain()
        c, keep, _ = build_config.build(cfg, cfg.sim.dt, 4096, terrain=ter)
        lays.append(HipSim(c, "cuda:0", keep).layout())
    assert lays[0]["kernel"] == "grx_step_tree16<true, false>" and lays[1]["kernel"] == "grx_step_tree16_base<true, false>", lays
    assert [(l["lanes_per_env"], l["waves_per_block"], l["num_blocks"]) for l in lays] == [(16, lays[0]["waves_per_block"], lays[0]["num_blocks"])] * 2


@pytest.mark.parametrize("tree", [None, 16])
@pytest.mark.parametrize("N", [64, 50])
def test_episode_sums_and_statistics(N, tree, monkeypatch):
    """GRX_T_BASE_EPISODE_SUMS is caller-writable; a reset outside a step (grx_reset_idx) and a step that resets fold the finished episodes'
    sums into GRX_T_BASE_EPISODE_STATS (mean / max_episode_length_s, legged_robot.py:420-424) and zero them; other rows keep theirs."""
    sim, cfg, _ = make_base_hip("plane", N=N, tree=tree, monkeypatch=monkeypatch)
    sim.reset_all()
    sums = sim.tensor("BASE_EPISODE_SUMS")
    assert tuple(sums.shape) == (NB, N)
    g = torch.Generator(device="cuda").manual_seed(5)
    inj = torch.rand(NB, N, device="cuda", generator=g) - 0.5
    sums.copy_(inj)
    ids = [3, 17, 40]
    sim.reset_idx(torch.tensor(ids, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    stats = sim.tensor("BASE_EPISODE_STATS").cpu()
    T = cfg.env.episode_length_s
    assert torch.allclose(stats, inj[:, ids].mean(1).cpu() / T, rtol=1e-5, atol=1e-7)
    keep = [i for i in range(N) if i not in ids]
    assert (sums[:, ids] == 0).all() and torch.equal(sums[:, keep], inj[:, keep])
    # a step that resets (the fixture's termination / time-out rows, applied): sums + this step's terms of the reset rows
    d = np.load(FIXTURE)
    sums.copy_(inj)
    sim.debug_post_physics(og.states_from(d, "plane_in_", N), apply_reset=True, common_step_counter=1,
                           noise_uniform=torch.tensor(d["plane_noise_u"]).contiguous().cuda())
    torch.cuda.synchronize()
    reset = sim.tensor("RESET").cpu().numpy().astype(bool)
    assert 2 <= reset.sum() < N
    r = sim.tensor("BASE_REWARD_TERMS").cpu()
    total = inj.cpu() + r
    stats = sim.tensor("BASE_EPISODE_STATS").cpu()
    assert torch.allclose(stats, total[:, reset].mean(1) / T, rtol=1e-5, atol=1e-7)
    got = sums.cpu()
    assert (got[:, reset] == 0).all() and torch.allclose(got[:, ~reset], total[:, ~reset], rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("task,N", [("GR1T1", 512), ("GR1T1_full_body", 256)])
def test_short_training_with_base_terms(task, N, tmp_path):
    """A few PPO iterations through make_env / make_alg_runner with every base term and the command curriculum on: finite rewards,
    extras["episode"] carries rew_<name> of both tables and the curriculum's keys, env.command_ranges reads the device ranges."""
    from wiki_grx_gym_amd.envs import GR1T1Cfg, GR1T1CfgPPO, GR1T1FullBodyCfg, GR1T1FullBodyCfgPPO
    from wiki_grx_gym_amd.utils import get_args, task_registry
    args = get_args(["--task", task, "--headless", "--num_envs", str(N), "--seed", "1"])
    cfg = GR1T1Cfg() if task == "GR1T1" else GR1T1FullBodyCfg()
    cfg.terrain.mesh_type = "heightfield"
    d = np.load(FIXTURE)
    for n, v in zip(map(str, d["names"]), map(float, d["scales"])):
        setattr(cfg.rewards.scales, n, v)
    cfg.commands.curriculum = True
    env, _ = task_registry.make_env(task, args=args, env_cfg=cfg)
    kernel = env._sim.layout()["kernel"]
    assert kernel == ENTRY["heightfield"] if task == "GR1T1" else kernel.startswith("grx_step_tree") and "_base<true" in kernel, kernel
    assert env.reward_names == sorted(env.reward_names) and set(_capi.BASE_REWARD_TERMS) <= set(env.reward_names)
    assert set(env.episode_sums) == set(env.reward_scales)
    env.reset()
    for _ in range(3):
        _, _, r, _, ex = env.step(torch.zeros(N, env.num_actions, device="cuda"))
        assert torch.isfinite(r).all()
        for n in ("tracking_lin_vel", "torques", "stumble"):
            assert "rew_" + n in ex["episode"] and torch.isfinite(ex["episode"]["rew_" + n])
        assert "min_command_x" not in ex["episode"]
        assert float(ex["episode"]["max_command_x"]) == env.command_ranges["lin_vel_x"][1] and "max_command_yaw" in ex["episode"]
    assert env.command_ranges["lin_vel_x"] == pytest.approx(list(cfg.commands.ranges.lin_vel_x))
    tcfg = GR1T1CfgPPO() if task == "GR1T1" else GR1T1FullBodyCfgPPO()
    tcfg.runner.num_steps_per_env = 16
    runner, _ = task_registry.make_alg_runner(env, name=task, args=args, train_cfg=tcfg, log_root=str(tmp_path))
    runner.learn(num_learning_iterations=3, init_at_random_ep_len=True)
    assert runner.current_learning_iteration == 3
    assert all(torch.isfinite(p).all() for p in runner.algorithm.actor_critic.parameters())


# ---- cfg.commands.curriculum (legged_robot.py:395-396, 828-838) -----------------------------------------------------------------------
CUR = "command_curriculum.npz"


def curriculum_sim(curriculum=True, lin_vel_x=None, N=64, seed=1, tree=None, monkeypatch=None):
    """A plane handle with only tracking_lin_vel active, its sigma so large that the term is exactly scale x dt every step (the injected
    episode sums then decide the curriculum exactly); the fixture's start range and max_curriculum."""
    from wiki_grx_gym_amd.sim import HipSim
    if tree:
        monkeypatch.setenv("GRX_FORCE_GENERIC", "1"); monkeypatch.setenv("GRX_TREE", "1"); monkeypatch.setenv("GRX_TREE_G", str(tree))
    d = np.load(og.os.path.join(og.G, CUR))
    cfg = make_cfg()
    cfg.rewards.scales.tracking_lin_vel = 1.0
    cfg.rewards.tracking_sigma = 1e9
    cfg.commands.curriculum = curriculum
    cfg.commands.max_curriculum = float(d["max_curriculum"])
    cfg.commands.ranges.lin_vel_x = list(map(float, d["start"] if lin_vel_x is None else lin_vel_x))
    c, keep, _ = build_config.build(cfg, cfg.sim.dt, N, seed=seed)
    sim = HipSim(c, "cuda:0", keep)
    assert sim.layout()["kernel"] == (("grx_step_tree16" if tree == 16 else "grx_step_tree") + TREE_ENTRY["plane"] if tree else ENTRY["plane"])
    return sim, cfg, d


def force_resets(sim, rows, sums=None, scale_dt=None, cfg=None):
    """Make `rows` time out on the next step (EPISODE_LENGTH is caller-writable) with tracking_lin_vel episode sums that reach `sums` once
    the step has added its own term."""
    N = sim.num_envs
    ep = sim.tensor("EPISODE_LENGTH")
    ep.zero_()
    ep[torch.as_tensor(np.flatnonzero(rows), device="cuda")] = max_episode_length(cfg or make_cfg())
    if sums is not None:
        bs = sim.tensor("BASE_EPISODE_SUMS")
        bs[_capi.BASE_REWARD_TERMS.index("tracking_lin_vel")] = torch.as_tensor(sums - scale_dt, dtype=torch.float32, device="cuda")
    assert N == len(rows)


def max_episode_length(cfg):
    """ceil(episode_length_s / dt) (legged_robot.py:91-93): an episode of this many steps times out at the next one."""
    return int(np.ceil(cfg.env.episode_length_s / (cfg.control.decimation * cfg.sim.dt)))


@pytest.mark.parametrize("tree", [None, 16])
def test_curriculum_ranges_follow_the_reference(tree, monkeypatch):
    """A sequence of steps whose resets carry the fixture's tracking_lin_vel episode sums: the device ranges after each equal the
    reference's update_command_curriculum (asymmetric start, max_curriculum 1.7, means 0.1 % either side of the threshold)."""
    sim, cfg, d = curriculum_sim(tree=tree, monkeypatch=monkeypatch)
    N = sim.num_envs
    sim.reset_all()
    rng = sim.tensor("COMMAND_RANGES")
    assert tuple(rng.shape) == (3, 2) and np.allclose(rng[0].cpu().numpy(), d["start"])
    zero = torch.zeros(N, sim.num_dofs, device="cuda")
    counter = 1
    for k in range(len(d["reset"])):
        force_resets(sim, d["reset"][k], d["sums"][k], float(d["scale_dt"]), cfg)
        sim.step(zero, 0.0, counter); counter += 1
        torch.cuda.synchronize()
        assert np.array_equal(sim.tensor("RESET").cpu().numpy().astype(bool), d["reset"][k]), k
        assert np.allclose(rng[0].cpu().numpy(), d["lin_vel_x"][k], rtol=0, atol=1e-6), (k, rng[0].cpu().numpy(), d["lin_vel_x"][k])
        assert np.allclose(rng[1:].cpu().numpy(), [cfg.commands.ranges.lin_vel_y, cfg.commands.ranges.ang_vel_yaw])
    before = rng.clone()
    force_resets(sim, np.zeros(N, bool))   # a step without resets: the ranges stay
    sim.step(zero, 0.0, counter)
    torch.cuda.synchronize()
    assert not sim.tensor("RESET").cpu().numpy().any() and torch.equal(rng, before)


def test_curriculum_step_resets_draw_from_the_new_range():
    """Handle A (curriculum on) widens on a step; handle B (same entry, curriculum off, its config range = A's widened range), same seed, same
    state, same reset rows: the reset rows' commands, obs and pri_obs are bit-identical -- the resets of the widening step draw from the new
    range.  (Only reset rows: that step's time-based resamples use A's old range.)"""
    a, cfg, d = curriculum_sim()
    scale_dt = float(d["scale_dt"])
    lo, hi = d["start"]
    widened = [max(lo - 0.5, -float(d["max_curriculum"])), min(hi + 0.5, float(d["max_curriculum"]))]
    b, _, _ = curriculum_sim(curriculum=False, lin_vel_x=widened)
    N = a.num_envs
    zero = torch.zeros(N, 10, device="cuda")
    for s in (a, b):
        s.reset_all()
        for c in range(1, 4):
            s.step(zero, 0.0, c)
    torch.cuda.synchronize()
    assert torch.equal(a.tensor("ROOT_STATES"), b.tensor("ROOT_STATES"))   # zero actions: the commands do not move the robots
    rows = np.zeros(N, bool); rows[[2, 9, 30, 31, 50]] = True
    sums = np.full(N, 2.0 * 0.8 * scale_dt * max_episode_length(cfg), np.float32)   # mean well above the threshold: A widens
    force_resets(a, rows, sums, scale_dt)
    force_resets(b, rows, sums, scale_dt)
    oa, pa = torch.zeros(N, 39, device="cuda"), torch.zeros(N, 168, device="cuda")
    ob, pb = torch.zeros_like(oa), torch.zeros_like(pa)
    a.step(zero, 0.0, 4, obs_out=oa, pri_obs_out=pa)
    b.step(zero, 0.0, 4, obs_out=ob, pri_obs_out=pb)
    torch.cuda.synchronize()
    assert np.allclose(a.tensor("COMMAND_RANGES")[0].cpu().numpy(), widened, atol=1e-6)
    r = torch.as_tensor(rows, device="cuda")
    assert torch.equal(a.tensor("RESET").bool(), r) and torch.equal(b.tensor("RESET").bool(), r)
    ca, cb = a.tensor("COMMANDS")[r], b.tensor("COMMANDS")[r]
    assert torch.equal(ca, cb), (ca, cb)
    assert torch.equal(oa[r], ob[r]) and torch.equal(pa[r], pb[r])
    assert (ca[:, 0] != 0).any()   # (not every reset row's command was zeroed by |cmd_xy| <= 0.1)
    # the next step's kernels draw from A's widened range too: the same rows reset again, below the threshold (no further widening)
    low = np.zeros(N, np.float32)
    force_resets(a, rows, low, scale_dt)
    force_resets(b, rows, low, scale_dt)
    a.step(zero, 0.0, 5, obs_out=oa, pri_obs_out=pa)
    b.step(zero, 0.0, 5, obs_out=ob, pri_obs_out=pb)
    torch.cuda.synchronize()
    assert np.allclose(a.tensor("COMMAND_RANGES")[0].cpu().numpy(), widened, atol=1e-6)
    assert torch.equal(a.tensor("COMMANDS")[r], b.tensor("COMMANDS")[r]) and torch.equal(oa[r], ob[r])


def test_curriculum_steps_replayed_from_a_graph():
    """Curriculum steps recorded into a graph (the forced resets and their sums recorded with them) and replayed: after every replay the
    ranges and commands equal those of the same steps issued eagerly on a twin handle -- the widening accumulates over replays up to the
    clip."""
    g_sim, cfg, d = curriculum_sim()
    e_sim, _, _ = curriculum_sim()
    N = g_sim.num_envs
    scale_dt = float(d["scale_dt"])
    zero = torch.zeros(N, 10, device="cuda")
    for s in (g_sim, e_sim):
        s.reset_all(); s.step(zero, 0.0, 1)
    torch.cuda.synchronize()
    rows = torch.zeros(N, dtype=torch.bool, device="cuda"); rows[[4, 11, 27, 60]] = True
    T = max_episode_length(cfg)
    ep_src = torch.where(rows, torch.tensor(T, device="cuda"), torch.tensor(0, device="cuda")).to(torch.int64)
    sums_src = torch.full((N,), 2.0 * 0.8 * scale_dt * T - scale_dt, device="cuda")
    t = _capi.BASE_REWARD_TERMS.index("tracking_lin_vel")

    def one_step(s):
        s.tensor("EPISODE_LENGTH").copy_(ep_src)
        s.tensor("BASE_EPISODE_SUMS")[t].copy_(sums_src)
        s.step(zero, 0.0, 2)
    import gc
    gc.collect(); gc.disable()
    g_sim.flush_stats()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        one_step(g_sim)
    gc.enable()
    seen = []
    for rep in range(4):
        graph.replay()
        one_step(e_sim)
        torch.cuda.synchronize()
        rg, re = g_sim.tensor("COMMAND_RANGES").cpu(), e_sim.tensor("COMMAND_RANGES").cpu()
        assert torch.equal(rg, re), (rep, rg, re)
        assert torch.equal(g_sim.tensor("COMMANDS"), e_sim.tensor("COMMANDS")), rep
        assert torch.equal(g_sim.tensor("RESET").bool(), rows)
        seen.append(rg[0].tolist())
    m = float(d["max_curriculum"])
    assert np.allclose(seen, [[-0.8, 1.2], [-1.3, m], [-m, m], [-m, m]], atol=1e-6), seen
