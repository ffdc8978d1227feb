"""Pin the reset family -- reset_idx and what it calls, the terrain curriculum, command resampling, pushes, _get_env_origins -- against
the REFERENCE's live code (tests/golden/reset_family.npz, tools/gen_golden.py gen_reset_family).

Every other pipeline fixture was recorded with the reference's reset_idx stubbed out, because its draws come from torch's global
generators.  This one turns the injection round: the BUILD's draws -- gro_rand(seed, env, step, stream, item), oracle/philox.h -- were
served to the reference's torch_rand_float / randint_like calls from a scripted queue while one post_physics_step() ran per case, so
legged_robot.py:377-440, 650-677, 717-826, 1163-1195 and legged_robot_fftai.py:137-146 produced the recorded outputs themselves.  The
generator asserts the margins (no row within 1e-3 of a threshold, every scan point 5e-4 cells from a cell edge, three rows per branch),
so every row of every tensor is compared here.  The checkers take a sim: tests/test_reset_golden_gpu.py runs them on the HIP kernels."""
import os
import re

import numpy as np
import pytest
import torch

from tests import test_oracle_golden as og
from tests.helpers import make_cfg
from wiki_grx_gym_amd import _capi
from wiki_grx_gym_amd.envs import build_config

G = og.G
STEP_CASES = ("curr", "push", "nodr", "plane", "shard", "full_body")      # one post_physics_step() each; "init": check_init_case
STREAMS = ("RESET_DOF", "RESET_ROOT", "CMD_TIME", "CMD_RESET", "PUSH", "CURRICULUM")
_CASES = STEP_CASES + ("init",)


def fixture():
    return np.load(os.path.join(G, "reset_family.npz"))


def load_case(d, case):
    """The arrays of one case by name (in_*, out_*, u_*, ...): undoes the storage layout of gen_reset_family's store() -- per-row arrays
    packed as the rows of <case>_f32 / <case>_i32, arrays equal to another one stored as its name in <case>_same."""
    out = {}
    for k in d.files:
        if k.startswith(case + "_") and not k.endswith(("_f32", "_i32", "_f32_names", "_i32_names", "_same")):
            out[k[len(case) + 1:]] = d[k]
    for tag in ("_f32", "_i32"):
        if case + tag not in d.files:
            continue
        M, r = d[case + tag], 0
        for spec in d[case + tag + "_names"]:
            name, shape, *dt = str(spec).split(":")
            if shape.startswith("T"):
                n = int(shape[1:])
                out[name] = M[r:r + n]
            else:
                dims = [int(x) for x in shape.split("x") if x]
                n = int(np.prod(dims)) if dims else 1
                out[name] = M[r:r + n].T.reshape([M.shape[1]] + dims)
            if dt:
                out[name] = out[name].astype(np.dtype(dt[0]))
            r += n
        assert r == M.shape[0]
    for a in d[case + "_same"]:
        name, ref = str(a).split("=@")
        m = re.fullmatch(r"(\w+?)(?:\[:(\d+)\])?", ref)
        src = next(c for c in _CASES if m.group(1).startswith(c + "_"))
        v = (out if src == case else load_case(d, src))[m.group(1)[len(src) + 1:]]
        out[name] = v if m.group(2) is None else v[:, :int(m.group(2))]
    return out


def case_cfg(case):
    """The build's task configuration of a case: the registered task with the reference's reset randomisation and pushes on."""
    cfg = make_cfg("GR1T1Full" if case == "full_body" else "GR1T1", noise=False, dr=False, push=True,
                   terrain="plane" if case == "plane" else "heightfield", curriculum=True)
    cfg.domain_rand.randomize_init_dof_pos = cfg.domain_rand.randomize_init_base_velocity = case != "nodr"
    return cfg


def case_config(case, k):
    """(cfg, grx_config, keepalive, meta) of the handle a case runs on: seed, env_offset and the batch size from the fixture."""
    cfg = case_cfg(case)
    step, seed, off = (int(x) for x in k["step_seed_offset"])
    N = k["in_root"].shape[0]
    ter = None if case == "plane" else og.reference_raster_terrain()[0]
    c, keep, meta = build_config.build(cfg, cfg.sim.dt, N, off, N + off, seed, ter)
    return cfg, c, keep, meta


def put(sim, name, value):
    t = sim.tensor(name)
    t.copy_(torch.as_tensor(np.ascontiguousarray(value)).to(t.dtype).to(t.device))


def seed_handle(sim, k, meta, heightfield):
    """Levels, origins and episode sums of the fixture go in through the handle's zero-copy views (the oracle takes them over with
    gro_debug_import_state); what creation derived -- terrain types, the plane's grid of origins -- is compared first."""
    term_idx = [_capi.REWARD_TERMS.index(n) for n in k["reward_names"]]
    assert list(k["reward_names"]) == meta["active_terms"]
    if heightfield:
        np.testing.assert_array_equal(og.T_(sim, "TERRAIN_TYPES").numpy(), k["in_terrain_types"])     # legged_robot.py:1177-1180
        put(sim, "TERRAIN_LEVELS", k["in_terrain_levels"])
        put(sim, "ENV_ORIGINS", k["in_env_origins"])
    else:
        np.testing.assert_array_equal(og.T_(sim, "ENV_ORIGINS").numpy(), k["in_env_origins"])          # legged_robot.py:1188-1195
    sums = np.zeros(tuple(sim.tensor("EPISODE_SUMS").shape), np.float32)
    sums[term_idx] = k["in_episode_sums"]
    put(sim, "EPISODE_SUMS", sums)
    if hasattr(sim, "import_state"):
        sim.import_state()
    return term_idx


class Worst:
    """Largest |got - want| per tensor of one run, for the record (printed; pytest -s)."""

    def __init__(self):
        self.err = {}

    def close(self, name, got, want, tol):
        got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
        assert got.shape == want.shape, (name, got.shape, want.shape)
        err = np.abs(got - want)
        self.err[name] = max(self.err.get(name, 0.0), float(err.max()) if err.size else 0.0)
        bad = err > tol + tol * np.abs(want)
        assert not bad.any(), f"{name}: max err {err.max():.3e} at {np.unravel_index(err.argmax(), err.shape)}, {int(bad.sum())} entries off"

    def __str__(self):
        return ", ".join(f"{n} {e:.2e}" for n, e in self.err.items())


def check_reset_case(sim, case, k, meta, tol, worst=None):
    """One reference post_physics_step() with a live reset_idx against `sim` (oracle or HIP) through the debug entry, apply_reset = 1,
    on the recorded inputs, seed, env_offset and common_step_counter: EVERY row of every recorded output."""
    w = worst or Worst()
    heightfield = case != "plane"
    N = k["in_root"].shape[0]
    step = int(k["step_seed_offset"][0])
    term_idx = seed_handle(sim, k, meta, heightfield)
    sim.debug_post_physics(og.states_from(k, "in_", N), apply_reset=True, common_step_counter=step)
    if sim.device.type == "cuda":
        torch.cuda.synchronize()
    T = lambda name: og.T_(sim, name).numpy()
    reset = k["out_reset"].astype(bool)
    np.testing.assert_array_equal(T("RESET").astype(bool), reset)
    np.testing.assert_array_equal(T("TIME_OUT").astype(bool), k["out_time_out"].astype(bool))
    np.testing.assert_array_equal(T("EPISODE_LENGTH"), k["out_episode_length"])
    np.testing.assert_array_equal(T("FEET_CONTACT").astype(bool), k["out_feet_contact"].astype(bool))
    if heightfield:
        np.testing.assert_array_equal(T("TERRAIN_LEVELS"), k["out_terrain_levels"])
    for name, key in (("DOF_POS", "dof_pos"), ("DOF_VEL", "dof_vel"), ("ROOT_STATES", "root"), ("COMMANDS", "commands"), ("ENV_ORIGINS", "env_origins"),
                      ("OBS", "obs"), ("PRI_OBS", "pri_obs"), ("REW", "rew"), ("LAST_ACTIONS", "last_actions"), ("LAST_DOF_VEL", "last_dof_vel"),
                      ("FEET_AIR_TIME", "feet_air_time"), ("FEET_LAND_TIME", "feet_land_time")):
        w.close(name, T(name), k["out_" + key], tol)
    # last_last_actions is last_actions after every step (legged_robot_fftai.py:94 follows legged_robot.py:299): the build keeps one buffer
    np.testing.assert_array_equal(k["out_last_last_actions"], k["out_last_actions"])
    w.close("EPISODE_SUMS", T("EPISODE_SUMS")[term_idx], k["out_episode_sums"], tol)
    assert np.abs(T("EPISODE_SUMS")).sum(0)[reset].max() == 0.0 and np.abs(k["in_episode_sums"]).sum(0)[reset].min() > 0.0
    np.testing.assert_array_equal(k["out_extras_time_outs"].astype(bool), T("TIME_OUT").astype(bool))       # extras["time_outs"]
    stats = sim.episode_stats()
    NT = len(stats) - 2
    assert stats[NT] == reset.sum()
    if "out_extras_rew" in k:      # extras["episode"] (legged_robot.py:420-428); the shard's reference means run over all 128 envs
        w.close("extras rew_*", stats[term_idx], k["out_extras_rew"], tol)
        if "out_extras_terrain_level" in k:
            assert abs(float(stats[NT + 1]) - float(k["out_extras_terrain_level"])) <= 1e-5
    elif heightfield:
        assert abs(float(stats[NT + 1]) - k["out_terrain_levels"].astype(np.float64).mean()) <= 1e-5
    # the case is what it was built to be
    cnt = dict(zip((str(n) for n in k["branch_names"]), k["branch_counts"]))
    assert all(cnt[n] >= 3 for n in cnt if n.startswith(("reset by", "no reset", "time resample", "reset and")))
    if case == "curr":
        assert min(cnt.values()) >= 3 and len(cnt) == 19, cnt
        assert (k["out_terrain_levels"] != k["in_terrain_levels"]).sum() >= 20
    if case == "push":
        assert step % 500 == 0 and np.abs(k["out_root"][~reset, 7:9] - k["in_root"][~reset, 7:9]).min() > 0
    if case == "nodr":
        assert np.abs(k["out_root"][reset, 7:13]).max() == 0.0
    return w


def make_oracle(case, k, precision):
    from oracle.binding import OracleSim
    cfg, c, keep, meta = case_config(case, k)
    return OracleSim(c, precision, keep), meta


@pytest.mark.parametrize("precision,tol", [("f64", 2e-6), ("f32", 1e-4)])
@pytest.mark.parametrize("case", STEP_CASES)
def test_reset_family_on_the_oracle(case, precision, tol):
    k = load_case(fixture(), case)
    sim, meta = make_oracle(case, k, precision)
    print(case, precision, "worst:", check_reset_case(sim, case, k, meta, tol))


def check_init_case(sim, k, meta, tol, worst=None):
    """init_done = False (legged_robot.py:806-808): the build's only such reset is reset_all, whose draws are keyed by step
    0x80000000 + the number of resets so far -- the fixture's `init` case ran the reference on those of the FIRST one.  The rows the
    reference reset are compared (reset_all resets every row); the levels and origins of ALL rows must stay, although the positions
    going in are the curriculum case's, where most rows would move."""
    w = worst or Worst()
    assert int(k["step_seed_offset"][0]) == 0x80000000
    seed_handle(sim, k, meta, True)
    to = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(sim.device)
    sim.set_state(to(k["in_root"]), to(k["in_dof_pos"]), to(k["in_dof_vel"]))
    sim.reset_all()
    if sim.device.type == "cuda":
        torch.cuda.synchronize()
    T = lambda name: og.T_(sim, name).numpy()
    reset = k["out_reset"].astype(bool)
    np.testing.assert_array_equal(k["out_terrain_levels"], k["in_terrain_levels"])
    np.testing.assert_array_equal(T("TERRAIN_LEVELS"), k["in_terrain_levels"])
    w.close("ENV_ORIGINS", T("ENV_ORIGINS"), k["out_env_origins"], tol)
    for name, key in (("DOF_POS", "dof_pos"), ("DOF_VEL", "dof_vel"), ("ROOT_STATES", "root"), ("COMMANDS", "commands")):
        w.close(name, T(name)[reset], k["out_" + key][reset], tol)
    d = np.linalg.norm(k["in_root"][:, :2].astype(np.float64) - k["in_env_origins"][:, :2], axis=1)
    assert (d[reset] > 4.0).sum() >= 10       # rows that would have moved up
    return w


@pytest.mark.parametrize("precision,tol", [("f64", 2e-6), ("f32", 1e-4)])
def test_init_done_false_leaves_the_levels(precision, tol):
    k = load_case(fixture(), "init")
    sim, meta = make_oracle("init", k, precision)
    print("init", precision, "worst:", check_init_case(sim, k, meta, tol))


def push_every_step(cfg):
    cfg.domain_rand.push_interval_s = cfg.control.decimation * cfg.sim.dt


def check_product_step(sim, c, cfg, k, meta, case):
    """The step itself (no debug entry), push_interval = 1, at the fixture's common_step_counter: what the draws decide whatever the
    physics does.  Rows whose episode_length_buf is written to 1000 time out; after the step their DOF_POS, DOF_VEL, ROOT_STATES, COMMANDS,
    TERRAIN_LEVELS and ENV_ORIGINS are the reference's recorded ones.  The curriculum compares the PRE-reset position, which one policy
    step cannot carry across a threshold: the rows are those the fixture puts more than 0.5 m from both.  `push`: the velocity of the
    rows that do not reset is the reference's recorded push."""
    step = int(k["step_seed_offset"][0])
    N = k["in_root"].shape[0]
    ref_reset = k["out_reset"].astype(bool)
    by_time = (k["in_episode_length"] + 1) % 500 == 0
    d = np.linalg.norm(k["in_root"][:, :2].astype(np.float64) - k["in_env_origins"][:, :2], axis=1)
    cn = np.linalg.norm(k["in_commands"][:, :2].astype(np.float64), axis=1)
    chosen = ref_reset & ~by_time & (np.abs(d - cfg.terrain.terrain_length / 2) > 0.5) & (np.abs(d - cn * cfg.env.episode_length_s * 0.5) > 0.5)
    assert chosen.sum() >= 30 and (k["out_terrain_levels"][chosen] > k["in_terrain_levels"][chosen]).sum() >= 5 \
        and (k["out_terrain_levels"][chosen] < k["in_terrain_levels"][chosen]).sum() >= 5
    sim.reset_all()
    root = torch.zeros(N, 13)
    root[:, 0:2] = torch.tensor(k["in_root"][:, 0:2])
    root[:, 2] = torch.tensor(k["in_root"][:, 2]).clamp(min=0.0) + 3.0      # in free fall over the terrain: no contact decides anything
    root[:, 6] = 1.0
    q0 = torch.tensor(np.array(c.default_dof_pos[:sim.num_dofs], dtype=np.float32)).repeat(N, 1)
    sim.set_state(root.to(sim.device).contiguous(), q0.to(sim.device).contiguous(), torch.zeros(N, sim.num_dofs).to(sim.device))
    put(sim, "COMMANDS", k["in_commands"])
    put(sim, "EPISODE_LENGTH", np.where(chosen, 1000, 0))
    seed_handle(sim, k, meta, True)      # (last: the oracle takes what the views hold over here)
    sim.step(torch.zeros(N, sim.num_dofs).to(sim.device), 0.0, step)
    if sim.device.type == "cuda":
        torch.cuda.synchronize()
    T = lambda name: og.T_(sim, name).numpy()
    np.testing.assert_array_equal(T("RESET").astype(bool), chosen)
    np.testing.assert_array_equal(T("TIME_OUT").astype(bool), chosen)
    w = Worst()
    for name, key in (("DOF_POS", "dof_pos"), ("DOF_VEL", "dof_vel"), ("ROOT_STATES", "root"), ("COMMANDS", "commands"), ("ENV_ORIGINS", "env_origins")):
        w.close(name, T(name)[chosen], k["out_" + key][chosen], 1e-4)
    np.testing.assert_array_equal(T("TERRAIN_LEVELS")[chosen], k["out_terrain_levels"][chosen])
    np.testing.assert_array_equal(T("TERRAIN_LEVELS")[~chosen], k["in_terrain_levels"][~chosen])
    if case == "push":
        assert step % 500 == 0 and (~ref_reset).sum() >= 10
        w.close("push", T("ROOT_STATES")[~ref_reset, 7:9], k["out_root"][~ref_reset, 7:9], 1e-4)
    return w


@pytest.mark.parametrize("case", ["curr", "push"])
def test_product_step_of_the_oracle_resets_and_pushes_like_the_reference(case):
    from oracle.binding import OracleSim
    k = load_case(fixture(), case)
    cfg = case_cfg(case)
    push_every_step(cfg)
    step, seed, off = (int(x) for x in k["step_seed_offset"])
    c, keep, meta = build_config.build(cfg, cfg.sim.dt, 64, off, 64 + off, seed, og.reference_raster_terrain()[0])
    print(case, "worst:", check_product_step(OracleSim(c, "f32", keep), c, cfg, k, meta, case))


def test_stored_uniforms_are_todays_draws():
    """The uniforms the reference was fed are gro_rand(seed, env_offset + row, step = common_step_counter, stream, item) of today's
    oracle/philox.h: a renumbered stream or item fails here, not as an unexplained mismatch on the GPU."""
    from oracle.binding import uniforms
    d = fixture()
    for case in _CASES:
        k = load_case(d, case)
        step, seed, off = (int(x) for x in k["step_seed_offset"])
        N = k["in_root"].shape[0]
        for stream in STREAMS:
            want = k["u_" + stream]
            assert want.shape == (N, {"RESET_DOF": k["in_dof_pos"].shape[1], "RESET_ROOT": 9, "CMD_TIME": 3, "CMD_RESET": 3, "PUSH": 2, "CURRICULUM": 1}[stream])
            np.testing.assert_array_equal(uniforms(seed, range(off, off + N), step, stream, want.shape[1]), want, err_msg=f"{case} {stream}")


def origins_cfg(curriculum, mesh="heightfield"):
    cfg = make_cfg(noise=False, dr=False, terrain=mesh, curriculum=curriculum)
    cfg.terrain.max_init_terrain_level = 4
    return cfg


def check_origins(make_sim, sizes):
    """_get_env_origins (legged_robot.py:1163-1195): terrain_types = floor(arange(N) / (N / num_cols)) in float32 and the plane's grid,
    equal to the reference's; the initial levels (the reference's own torch.randint: not reproducible) within [0, max_init_terrain_level]
    with the curriculum and [0, num_rows - 1] without it."""
    d = fixture()
    ter = og.reference_raster_terrain()[0]
    for N in sizes:
        for curriculum in (True, False):
            cfg = origins_cfg(curriculum)
            sim = make_sim(build_config.build(cfg, cfg.sim.dt, N, terrain=ter))
            np.testing.assert_array_equal(og.T_(sim, "TERRAIN_TYPES").numpy(), d[f"origins_types_{N}"])
            lv = og.T_(sim, "TERRAIN_LEVELS").numpy()
            top = 4 if curriculum else cfg.terrain.num_rows - 1
            assert lv.min() >= 0 and lv.max() <= top and (N < 4095 or (lv.max() == top and lv.min() == 0))
            np.testing.assert_array_equal(og.T_(sim, "ENV_ORIGINS").numpy(), ter.env_origins[lv, d[f"origins_types_{N}"]])
        if f"origins_grid_{N}" in d.files:
            cfg = origins_cfg(True, "plane")
            sim = make_sim(build_config.build(cfg, cfg.sim.dt, N))
            np.testing.assert_array_equal(og.T_(sim, "ENV_ORIGINS").numpy(), d[f"origins_grid_{N}"].T)
    assert int(d["origins_num_cols"]) == cfg.terrain.num_cols


def test_env_origins_on_the_oracle():
    from oracle.binding import OracleSim
    check_origins(lambda b: OracleSim(b[0], "f32", b[1]), (64, 100, 4095, 4096))


def test_shard_types_are_rows_64_to_127_of_the_128_env_assignment():
    """A handle with env_offset 64 of 128 envs carries the terrain types of the reference's rows 64-127 (the global env index, not the local
    one, enters legged_robot.py:1177-1180)."""
    d = fixture()
    k = load_case(d, "shard")
    sim, _ = make_oracle("shard", k, "f32")
    np.testing.assert_array_equal(sim.tensor("TERRAIN_TYPES").numpy(), k["in_terrain_types"])
    assert k["in_terrain_types"].min() >= 9 and not np.array_equal(k["in_terrain_types"], d["origins_types_64"])
