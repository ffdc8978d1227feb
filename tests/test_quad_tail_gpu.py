"""The tail of the lane-quad eight-wave step kernel (`-m gpu`): behind reset_idx wave 0 hands ONE post-reset record to the idle waves --
wave 2 writes the observation rows from it, waves 4..7 store the state columns (csrc/grx_step_kernel_body.inc, GRX_TAIL_SPLIT;
DESIGN.md 4.1).  The lane-pair eight-wave kernel keeps observations and stores on wave 0, so it is the reference here: both layouts
get the same injected post-physics records (grx_debug_post_physics), then one plain step, and every tensor the handle publishes and
every state column readable through it is compared after each of the two launches -- what only the NEXT launch reads (anchors,
last_actions, last_dof_vel, the feet timers, the episode length, levels, origins) shows in the second comparison at the latest.

Sizes: 5 envs (one partial 16-env block), 16 (one full block), 37 (two full blocks and a partial one of 5)."""
import numpy as np
import pytest
import torch

from tests.helpers import make_cfg, make_terrain, random_actions
from tests.test_hip_parity import PHYS, set_layout
from wiki_grx_gym_amd import _capi
from wiki_grx_gym_amd.envs import build_config

pytestmark = pytest.mark.gpu

SIZES = [5, 16, 37]
PIPE_TOL = (1e-4, 1e-4)   # tests/test_hip_parity.py: "env pipeline (obs / reward / termination on identical state): 1e-4 abs + 1e-4 rel"

# After the INJECTED launch the two kernels run the same arithmetic on the same inputs everywhere but here, where the layouts sum in another order:
#   * the height scan's mean over 121 points (2 lanes x 4 waves per env with lane pairs, 4 lanes x 6 waves with lane quads) -> FEET_HEIGHT, and
#     through it PRI_OBS columns num_obs + 6, 7, REW and the sums / terms of the rewards that read it;
#   * the mean of the observation height block -> BASE_HEIGHTS_OFFSET and PRI_OBS column num_obs + 3;
#   * REW itself: the reward terms are summed over the two legs' lanes and the two reward waves, 2 lanes per env against 4;
#   * EPISODE_STATS (+ history): sums over the envs of a block, 32 against 16 per block.
# Everything else must be EXACTLY equal.
NON_EXACT = {"FEET_HEIGHT": PHYS["FEET_HEIGHT"][:2], "BASE_HEIGHTS_OFFSET": PHYS["BASE_HEIGHTS_OFFSET"][:2], "REW": PHYS["REW"][:2],
             "EPISODE_SUMS": PIPE_TOL, "REWARD_TERMS": PIPE_TOL, "EPISODE_STATS": PIPE_TOL, "EPISODE_STATS_HISTORY": PIPE_TOL}
SKIP = {"MOTOR_STRENGTH", "FRICTION", "BASE_MASS_COM", "COMMAND_RANGES",       # per-handle constants (compared once, below) / not published by these handles
        "BASE_EPISODE_SUMS", "BASE_REWARD_TERMS", "BASE_EPISODE_STATS", "BASE_EPISODE_STATS_HISTORY",
        "CONTACT_FORCES"}                                                    # (the injected launch runs no sub-steps: not written)
# After the PLAIN step the physics of the two layouts differs in rounding (another cut of the recursion over the lanes): the physics budgets of
# tests/test_hip_parity.py for one policy step from identical state, with NO outlier allowed at these sizes (every fraction there is below 1 / elements).
PLAIN_EXACT = ("RESET", "TIME_OUT", "EPISODE_LENGTH", "FEET_CONTACT", "TERRAIN_LEVELS", "TERRAIN_TYPES", "ACTIONS", "LAST_ACTIONS", "ENV_ORIGINS", "TERM_CONTACT")


def published(sim):
    out = {}
    for name in _capi.TENSOR_IDS:
        if name in SKIP:
            continue
        try:
            out[name] = sim.tensor(name).detach().cpu().clone()
        except Exception:
            continue
    return out


def make_pair(monkeypatch, cfg, N, seed=3):
    from wiki_grx_gym_amd.sim import HipSim
    ter = make_terrain(cfg, N, seed=seed)
    sims = {}
    for layout in ("quad", 8):
        set_layout(monkeypatch, layout)
        c, keep, _ = build_config.build(cfg, cfg.sim.dt, N, 0, N, seed, ter)
        sims[layout] = HipSim(c, "cuda:0", keep)
        lay = sims[layout].layout()
        want = ("grx_step_kernel_quad<", 4, 8) if layout == "quad" else ("grx_step_kernel<", 2, 8)
        assert lay["kernel"].startswith(want[0]) and (lay["lanes_per_env"], lay["waves_per_block"]) == want[1:], lay
        sims[layout].reset_all()
    return sims["quad"], sims[8], c


def records(sim, c, N, seed, reset_envs, resample_envs):
    """Plausible post-physics records, airborne (no contact in the plain step that follows); `reset_envs` are tilted past the termination
    angle, timed out or carry a terminating contact, `resample_envs` reach a command-resampling step."""
    rng = np.random.default_rng(seed)
    org = sim.tensor("ENV_ORIGINS").cpu().numpy()
    nd = sim.num_dofs
    arr = (_capi.PipelineState * N)()
    u = lambda lo, hi: float(rng.uniform(lo, hi))
    for i in range(N):
        ps = arr[i]
        for j in range(nd):
            ps.q[j] = c.default_dof_pos[j] + u(-0.2, 0.2); ps.qd[j] = u(-2, 2); ps.actions[j] = u(-1.5, 1.5)
            ps.last_actions[j] = u(-1, 1); ps.last_last_actions[j] = u(-1, 1); ps.last_dof_vel[j] = u(-2, 2); ps.torques[j] = u(-40, 40)
        ps.root[0], ps.root[1], ps.root[2] = org[i, 0] + u(-0.5, 0.5), org[i, 1] + u(-0.5, 0.5), org[i, 2] + 1.6
        q = np.array([u(-0.1, 0.1), u(-0.1, 0.1), u(-1, 1), 1.0])
        for k in range(3):
            ps.root[7 + k] = u(-0.5, 0.5); ps.root[10 + k] = u(-0.5, 0.5); ps.commands[k] = u(-0.5, 0.5)
        for f in range(2):
            ps.air_time[f] = u(0, 0.4) * (rng.random() < 0.7); ps.land_time[f] = u(0, 0.4) * (rng.random() < 0.5); ps.contact_last[f] = int(rng.random() < 0.5)
            ps.avg_force[f] = u(0, 300)
            for k in range(3):
                ps.feet_force[f][k] = u(0, 300) if k == 2 and rng.random() < 0.5 else u(-5, 5)
                ps.feet_pos[f][k] = ps.root[k] + (u(-0.2, 0.2) if k < 2 else -0.9)
                ps.avg_speed[f][k] = u(0, 1)
        for k in range(9):
            ps.torso_R[k] = float(k % 4 == 0)
        ps.base_heights_offset = u(0.8, 1.0); ps.episode_length = int(rng.integers(1, 50)); ps.term_contact = 0
        if i in resample_envs:
            ps.episode_length = int(c.resample_command_interval) - 1
        if i in reset_envs:
            kind = reset_envs.index(i) % 3
            if kind == 0: q = np.array([0.7, 0.1, 0.0, 0.7])          # tilted: |projected gravity z| below the threshold
            elif kind == 1: ps.episode_length = int(c.max_episode_length) + 1
            else: ps.term_contact = 1
        q = q / np.linalg.norm(q)
        for k in range(4):
            ps.root[3 + k] = float(q[k])
    return arr


def compare(a, b, exact_but, what, plain=False):
    assert set(a) == set(b) and len(a) >= 30, (sorted(a), sorted(b))
    for name in sorted(a):
        x, y = a[name], b[name]
        assert x.shape == y.shape and x.dtype == y.dtype, (what, name)
        if plain and name not in PLAIN_EXACT:
            atol, rtol = PHYS[name][:2] if name in PHYS else PIPE_TOL
            if name == "ANCHORS": atol, rtol = PHYS["FEET_POS"][:2]          # positions of the feet's contact spheres
            if name == "RIGID_BODY_STATES": atol, rtol = PHYS["DOF_VEL"][:2]  # link frames and their velocities
            # the rows hold the state above times an observation scale (GR1T1: 1, the heights 5): the joint velocities' budget is the widest of
            # budget x scale (DOF_VEL and BASE_ANG_VEL 5e-3; base_lin_vel 2e-3, heights 1e-4 x 5 lie below it), so it bounds every column
            if name in ("OBS", "PRI_OBS"): atol, rtol = PHYS["DOF_VEL"][:2]
        elif name in exact_but:
            atol, rtol = exact_but[name]
        else:
            assert torch.equal(x, y), f"{what}: {name} differs, max |d| = {(x.double() - y.double()).abs().max().item():.3e} at {int((x != y).sum())} elements"
            continue
        d = (x.double() - y.double()).abs()
        print(f"{what}: {name} max |d| = {d.max().item():.3e} (atol {atol:g}, rtol {rtol:g})")
        assert (d <= atol + rtol * y.double().abs()).all(), f"{what}: {name} max |d| = {d.max().item():.3e}"


def pri_obs_split(t, nobs):
    """PRI_OBS: its columns behind the height scan's means (num_obs + 3, 6, 7), and the rest -- exact."""
    cols = [nobs + 3, nobs + 6, nobs + 7]
    keep = [k for k in range(t.shape[1]) if k not in cols]
    return t[:, keep], t[:, cols]


CASES = {
    "noise_off": dict(noise=False), "noise_on": dict(noise=True), "caller_noise": dict(noise=True, caller=True),
    "publish_every_step": dict(noise=True, publish="every_step"), "publish_on_refresh": dict(noise=True, publish="on_refresh"),
}


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("case", list(CASES))
def test_injected_launch_then_plain_step_equal_the_lane_pair_kernel(case, N, monkeypatch):
    k = CASES[case]
    cfg = make_cfg(noise=k["noise"], dr=True, push=True, terrain="heightfield")
    cfg.env.publish_rigid_body_states = cfg.env.publish_measured_heights = k.get("publish", "every_step")
    quad, pair, c = make_pair(monkeypatch, cfg, N)
    nobs, npri = int(c.num_obs), int(c.num_pri_obs)
    for name in ("MOTOR_STRENGTH", "FRICTION", "BASE_MASS_COM", "ENV_ORIGINS", "TERRAIN_LEVELS"):
        assert torch.equal(quad.tensor(name), pair.tensor(name)), name   # the same handle constants behind both
    # resets in env 0, in the partial last block and (37 envs) in the middle; most envs are not reset.  A command-resampling step in two envs.
    reset_envs = sorted({0, N - 1, N - 3, N // 2})
    resample_envs = sorted({1, N - 2})
    arr = records(quad, c, N, seed=N, reset_envs=reset_envs, resample_envs=resample_envs)
    step0 = int(c.push_interval) * 3   # a PUSH step (legged_robot.py:786-797)
    assert c.push_robots and step0 > 0 and int(c.resample_command_interval) > 1
    gen = torch.Generator().manual_seed(N)
    noise = torch.rand(N, nobs, generator=gen).cuda().contiguous() if k.get("caller") else None
    for sim in (quad, pair):
        sim.debug_post_physics(arr, apply_reset=True, common_step_counter=step0, noise_uniform=noise)
    torch.cuda.synchronize()
    a, b = published(quad), published(pair)
    assert a["RESET"].bool().nonzero().flatten().tolist() == reset_envs
    assert (a["COMMANDS"][resample_envs] != torch.tensor([[arr[i].commands[j] for j in range(3)] for i in resample_envs])).any()
    assert (a["ROOT_STATES"][1, 7:9] != torch.tensor([arr[1].root[7], arr[1].root[8]])).all()   # pushed
    assert k["noise"] == bool((a["OBS"] != a["PRI_OBS"][:, :nobs]).any())
    for t in (a, b):
        t["PRI_OBS"], t["PRI_OBS[:, scan means]"] = pri_obs_split(t["PRI_OBS"], nobs)
    compare(a, b, dict(NON_EXACT, **{"PRI_OBS[:, scan means]": PIPE_TOL}), f"{case} N={N} injected")

    # ---- one plain step (no push, no reset expected: the robots are airborne), into caller-owned rows allocated larger than N
    actions = random_actions(cfg, N, gen, 0.5).cuda()
    noise2 = torch.rand(N, nobs, generator=gen).cuda().contiguous() if k.get("caller") else None
    outs = {}
    for key, sim in (("quad", quad), ("pair", pair)):
        obs = torch.full((N + 3, nobs), -7.0, device="cuda"); pri = torch.full((N + 3, npri), -7.0, device="cuda")
        sim.step(actions, 5.0, step0 + 1, noise_uniform=noise2, obs_out=obs[:N], pri_obs_out=pri[:N])
        outs[key] = (obs, pri)
    torch.cuda.synchronize()
    for obs, pri in outs.values():
        assert (obs[N:] == -7.0).all() and (pri[N:] == -7.0).all(), "rows e >= N of a caller's buffer were written"
        assert (obs[:N] != -7.0).all()
    a, b = published(quad), published(pair)
    for t, key in ((a, "quad"), (b, "pair")):
        t["OBS"], t["PRI_OBS"] = outs[key][0][:N].cpu(), outs[key][1][:N].cpu()   # (the step wrote the caller's rows, not the library's)
    assert torch.equal(a["LAST_ACTIONS"], a["ACTIONS"]) and torch.equal(a["LAST_DOF_VEL"], a["DOF_VEL"])   # legged_robot.py:299-300
    assert torch.equal(a["EPISODE_LENGTH"][reset_envs], torch.ones(len(reset_envs), dtype=a["EPISODE_LENGTH"].dtype))
    compare(a, b, {}, f"{case} N={N} plain step", plain=True)
    quad.close(); pair.close()


@pytest.mark.parametrize("N", SIZES)
def test_two_plain_steps_store_every_column_of_a_partial_block(N, monkeypatch):
    """Two plain steps from reset on the lane-quad kernel alone: what the first launch's helper waves stored is what the second one loads.  The state
    columns are [rows][N] with nothing behind row N - 1 but the next row, so a store of a lane e >= N would land in a neighbour's value: every column
    equals the lane-pair kernel's within the physics budgets after both steps."""
    cfg = make_cfg(noise=True, dr=True, push=True, terrain="heightfield")
    quad, pair, c = make_pair(monkeypatch, cfg, N)
    gen = torch.Generator().manual_seed(100 + N)
    for s in range(2):
        actions = random_actions(cfg, N, gen, 0.5).cuda()
        for sim in (quad, pair):
            sim.step(actions, 5.0, s + 1)
        torch.cuda.synchronize()
        compare(published(quad), published(pair), {}, f"N={N} step {s}", plain=True)
    quad.close(); pair.close()
