"""The zoo's own footing, on the CPU (tests/robot_zoo.py, tests/substep.ZOO_SCENES): is the reference right on trees other than the GR1's?
The fp64 oracle's dynamics (ABA against RNEA), its link frames (against tests/kinematics_ref.py) and its conservation laws -- momentum,
angular momentum and kinetic energy evaluated here, in fp64, from the published state and the model's masses, not by the oracle -- on
every zoo model and both shipped full bodies; the builders' exits; and, as tests/test_substep_parity.py does for SUBSTEP_BAND, that ZOO_BAND
is SENS_K x what the fp32 oracle shows against the fp64 one on exactly the trajectories tests/test_robot_zoo_gpu.py replays, that every
scene reaches the regimes it is there for and that the fp32 oracle meets the conditions the kernels are held to."""
import json
import os

import numpy as np
import pytest
import torch

from tests import robot_zoo, substep
from tests.helpers import make_cfg
from tests.kinematics_ref import BodyKinematics
from tests.substep import MIN_REGIME, SENS_K, ZOO_SCENES
from tests.test_kinematics import rbs_close
from tests.test_substep_parity import ALLOW
from wiki_grx_gym_amd.envs import build_config, config

ALL = robot_zoo.MODELS + ("gr1t1",)          # every zoo model and both shipped full bodies


def cfg_of(key, **kw):
    return make_cfg(config.GR1T1FullBodyCfg if key == "gr1t1" else robot_zoo.cfg_class(key), **kw)


def make(key, N=4, precision="f64", gravity=True, **grx):
    from oracle.binding import OracleSim
    cfg = cfg_of(key)
    if not gravity:
        cfg.sim.gravity = [0.0, 0.0, 0.0]
    for k, v in grx.items():
        setattr(cfg.sim.grx, k, v)
    c, keep, meta = build_config.build(cfg, cfg.sim.dt, N)
    return OracleSim(c, precision, keep), cfg, meta


def random_state(sim, rm, seed, vel=1.0, spread=0.5, z=50.0):
    """Free-floating, any orientation, the joints over `spread` of their ranges."""
    g = torch.Generator().manual_seed(seed)
    N, nd = sim.num_envs, sim.num_dofs
    root = torch.zeros(N, 13)
    root[:, 2] = z
    q = torch.randn(N, 4, generator=g)
    root[:, 3:7] = q / q.norm(dim=1, keepdim=True)
    root[:, 7:13] = torch.randn(N, 6, generator=g) * vel
    lo, hi = torch.tensor(rm.dof_lower, dtype=torch.float32), torch.tensor(rm.dof_upper, dtype=torch.float32)
    dq = (lo + hi) / 2 + (2 * torch.rand(N, nd, generator=g) - 1) * spread * (hi - lo) / 2
    dqd = torch.randn(N, nd, generator=g) * 3 * vel
    sim.set_state(root.contiguous(), dq.contiguous(), dqd.contiguous())


@pytest.fixture(autouse=True)
def zoo(monkeypatch):
    return robot_zoo.install(monkeypatch)


# ---------------------------------------------------------------------------------------------------------------- the oracle on these trees
@pytest.mark.parametrize("key", ALL)
def test_aba_matches_rnea(key):
    """ID(FD(tau)) == tau and the free-floating base carries no residual wrench (fp64; the bounds of tests/test_oracle_physics.py)."""
    sim, _, meta = make(key)
    random_state(sim, meta["model"], 0)
    rng = np.random.RandomState(0)
    for e in range(sim.num_envs):
        tau = rng.randn(sim.num_dofs) * 30
        qdd, acc = sim.forward_dynamics(e, tau)
        tau2, wrench = sim.inverse_dynamics(e, qdd, acc)
        np.testing.assert_allclose(tau2, tau, atol=1e-9, rtol=1e-10)
        assert np.abs(wrench).max() < 1e-8
    sim.close()


@pytest.mark.parametrize("key", ALL)
def test_oracle_rigid_body_states_match_the_torch_restatement(key):
    """GRX_T_RIGID_BODY_STATES of the oracle after a policy step from a random state against tests/kinematics_ref.py on the state it
    publishes (the tolerances of tests/test_kinematics.py)."""
    from tests.helpers import random_actions
    N = 24
    sim, cfg, meta = make(key, N=N, precision="f32")
    rm = meta["model"]
    sim.reset_all()
    random_state(sim, rm, 1, vel=0.3)
    g = torch.Generator().manual_seed(1)
    for s in range(3):
        sim.step(random_actions(cfg, N, g, 0.5), 5.0, s + 1)
    alive = ~sim.tensor("RESET").bool()
    assert alive.sum() >= N // 2
    want = BodyKinematics(rm, "cpu").rigid_body_states(sim.tensor("ROOT_STATES"), sim.tensor("DOF_POS"), sim.tensor("DOF_VEL"))
    got = sim.tensor("RIGID_BODY_STATES")[:, :rm.num_links]
    assert got.shape == (N, rm.num_links, 13) and rbs_close(got[alive], want[alive], 2e-5, 2e-5)
    assert float(sim.tensor("RIGID_BODY_STATES")[:, rm.num_links:].abs().max()) == 0
    sim.close()


def mechanics(rm, kin, root, q, qd, armature=None):
    """(P (N, 3), L about the world origin (N, 3), KE (N,)) in fp64 from the published state: link frames through tests/kinematics_ref.py,
    masses, centres of mass and inertias from the model; `armature` (nd,): the joint-space rotor inertias, which hold 1/2 arm qd^2 each (the
    full bodies' arm and head joints carry one) and, being joint-space terms, no momentum."""
    R, p, v, w = kin.body_frames(root.double(), q.double(), qd.double())
    m = torch.as_tensor(rm.mass, dtype=torch.float64)
    com = torch.as_tensor(rm.com, dtype=torch.float64)
    Ic = torch.as_tensor(rm.inertia, dtype=torch.float64)
    r = (R @ com[None, :, :, None]).squeeze(-1)                    # body origin -> centre of mass, world
    c, vc = p + r, v + torch.cross(w, r, dim=-1)
    Iw = R @ Ic[None] @ R.transpose(-1, -2)
    h = (Iw @ w[..., None]).squeeze(-1)
    P = (m[None, :, None] * vc).sum(1)
    L = (torch.cross(c, m[None, :, None] * vc, dim=-1) + h).sum(1)
    KE = 0.5 * (m[None] * (vc * vc).sum(-1) + (w * h).sum(-1)).sum(1)
    if armature is not None:
        KE = KE + 0.5 * (torch.as_tensor(armature, dtype=torch.float64)[None] * qd.double() ** 2).sum(1)
    return P, L, KE


def kin64(rm):
    kin = BodyKinematics(rm, "cpu")
    for t in ("axis", "rot0", "jpos", "link_rot", "link_pos"):
        setattr(kin, t, getattr(kin, t).double())
    return kin


def free_flight(key, dt):
    """Zero gravity, zero gains, no joint-limit springs, no contact, no self-collision: 1 s of zero torque, then 0.5 s of a constant torque on every joint --
    a quarter of the joint's velocity limit x its own body's inertia about the axis / 0.5 s, random sign, so that the joints gain some
    3 rad/s and none comes near its velocity limit (the clamp there is no conservative force: at three times these velocities the
    10-link chains of deep9 / deep10 whip into it and lose 3 % of their momentum whatever the time step).  Returns the changes of
    (P, L, KE) over either phase as tensors, the applied angular impulse sum_j |tau_j| t per env and what the torques would have added to L
    had they acted from outside, J = sum_j tau_j a_j t (a_j: the joint axis in the world, mean of both ends of the phase)."""
    from oracle.binding import OracleSim
    cfg = cfg_of(key)
    cfg.sim.gravity, cfg.sim.grx.k_limit, cfg.sim.dt = [0.0, 0.0, 0.0], 0.0, dt
    cfg.asset.self_collisions = 1      # (the reference's flag is a filter: 1 = off.  A self-collision is internal too, but its damping takes kinetic energy)
    c, keep, meta = build_config.build(cfg, cfg.sim.dt, 4)
    sim = OracleSim(c, "f64", keep)
    rm = meta["model"]
    kin = kin64(rm)
    lim = torch.tensor(rm.dof_vel_limit)
    snap = lambda: (sim.tensor("ROOT_STATES").clone().double(), sim.tensor("DOF_POS").clone().double(), sim.tensor("DOF_VEL").clone().double())
    world_axes = lambda s: (kin.body_frames(*s)[0][:, 1:] @ kin.axis[1:][None, :, :, None]).squeeze(-1)

    def run(tau, seconds):
        for _ in range(10):
            for i in range(sim.num_envs):
                sim.substeps(i, tau[i], int(round(seconds / 10 / dt)), contact=False)
            assert (sim.tensor("DOF_VEL").abs() < 0.9 * lim).all()
    random_state(sim, rm, 2, vel=0.2, spread=0.3, z=1.0)
    s0 = snap()
    run(np.zeros((sim.num_envs, sim.num_dofs)), 1.0)
    s1 = snap()
    own = np.array([rm.joint_axis[b] @ (rm.inertia[b] + rm.mass[b] * (rm.com[b] @ rm.com[b] * np.eye(3) - np.outer(rm.com[b], rm.com[b]))) @ rm.joint_axis[b]
                    for b in range(1, rm.num_bodies)])
    tau = np.sign(np.random.RandomState(3).randn(sim.num_envs, sim.num_dofs)) * 0.25 * np.asarray(rm.dof_vel_limit) * own / 0.5
    run(tau, 0.5)
    s2 = snap()
    sim.close()
    arm = [c.model.dof_armature[j] for j in range(rm.num_dofs)]
    m0, m1, m2 = (mechanics(rm, kin, *s, armature=arm) for s in (s0, s1, s2))
    J = ((world_axes(s1) + world_axes(s2)) / 2 * torch.as_tensor(tau)[..., None]).sum(1) * 0.5
    return {"free": [b - a for a, b in zip(m0, m1)], "torque": [b - a for a, b in zip(m1, m2)], "KE0": m0[2], "L0": m0[1], "impulse": torch.as_tensor(np.abs(tau).sum(1) * 0.5),
            "J": J, "M": float(rm.mass.sum())}


@pytest.mark.parametrize("key", ALL)
def test_momentum_and_energy_are_conserved_without_gravity(key):
    """Total momentum P, angular momentum L about the origin and kinetic energy, evaluated here from the published state (mechanics()),
    at the oracle's time step (2 ms) and at a quarter of it.
    (1) Zero torque, 1 s: KE stays to the 2e-2 of test_energy_without_gravity_is_conserved, P to the 0.02 m/s x M of
    test_free_fall_and_momentum, L to 2e-2 |L| + M x 0.02 m/s x 1 m; and what is left is the generalised-coordinate Euler step's
    first-order error: a quarter of the step leaves less than half of it (test_free_fall_and_momentum's rule; observed: a quarter).
    (2) A constant joint torque, 0.5 s: a joint torque is internal.  P and L change by no more than 5 % of the applied angular impulse
    sum |tau_j| t (x 1 m^-1 for P) plus phase 1's drift; that change is first-order error too (halves with a quarter of the step), and
    its Richardson extrapolation to dt = 0, (4 fine - coarse) / 3, is below 1 % of the impulse: a leak of the impulse would not shrink with
    the step.  The check has power: torques acting from OUTSIDE -- no reaction on the parent -- would add J = sum tau_j a_j t to L, and |J| is
    at least 5 x that last bound in at least three of the four envs (the torques' signs are random: in one env they may cancel)."""
    a, b = free_flight(key, 0.002), free_flight(key, 0.0005)
    amax = lambda t: float(t.abs().max())
    print("zoo conservation:", key, {ph: {dt: [float(f"{amax(x):.2e}") for x in r[ph]] for dt, r in (("2ms", a), ("0.5ms", b))} for ph in ("free", "torque")},
          "impulse", float(a["impulse"].min()), "|J|", float(a["J"].norm(dim=1).min()))
    dP, dL, dE = a["free"]
    assert (dE.abs() / a["KE0"] < 2e-2).all() and amax(dP) < 0.02 * a["M"]
    assert (dL.abs() < 2e-2 * a["L0"].norm(dim=1, keepdim=True) + 0.02 * a["M"]).all()
    for coarse, fine in zip(a["free"], b["free"]):
        assert amax(fine) < 0.5 * amax(coarse) + 1e-9
    imp = a["impulse"][:, None]
    for k in (0, 1):     # P, L
        coarse, fine = a["torque"][k], b["torque"][k]
        assert (fine.abs() <= 0.05 * imp + amax(b["free"][k])).all(), (key, "PL"[k], amax(fine), float(imp.min()))
        assert amax(fine) < 0.5 * amax(coarse) + 1e-9
        assert (((4 * fine - coarse) / 3).abs() <= 0.01 * imp).all(), (key, "PL"[k], amax((4 * fine - coarse) / 3), float(imp.min()))
    assert (a["J"].norm(dim=1) >= 5 * 0.01 * a["impulse"]).sum() >= 3, (key, a["J"].norm(dim=1), a["impulse"])


# ---------------------------------------------------------------------------------------------------------------- the models, the builders' exits
def topology(raw):
    """(chains, depth levels, most side chains on one body) of a model file, as DESIGN 4.3 deals chains: a body's first child continues
    its chain, every further child -- and every child of the base -- starts one."""
    links = raw["links"]
    body_of, parent, n = {}, [-1], 1
    for i, L in enumerate(links):
        if L["joint_type"] == "floating":
            body_of[i] = 0
        elif L["joint_type"] == "fixed":
            body_of[i] = body_of[L["parent"]]
        else:
            body_of[i] = n
            parent.append(body_of[L["parent"]])
            n += 1
    depth, kids, chains = [0] * n, [0] * n, 0
    for b in range(1, n):
        p = parent[b]
        depth[b] = 0 if p == 0 else depth[p] + 1
        if p == 0 or kids[p] > 0:
            chains += 1
        kids[p] += 1
    return chains, max(depth[1:]) + 1, max([k - 1 for k in kids[1:]] + [0])


def test_the_expected_kernels_follow_from_the_limits():
    """EXPECTED_KERNEL against the documented limits of the tree kernel (8 chains whatever the group size, 10 depth levels,
    4 side chains per body), counted from the model files alone; and the zoo holds a model on either side of each."""
    got = {}
    for key in robot_zoo.MODELS:
        with open(os.path.join(robot_zoo.asset_dir(), key + ".model.json")) as f:
            chains, levels, side = topology(json.load(f))
        got[key] = (chains, levels, side)
        fits = chains <= 8 and levels <= 10 and side <= 4
        assert robot_zoo.EXPECTED_KERNEL[key] == {8: "tree" if fits else "generic", 16: "tree" if fits else "generic"}, (key, chains, levels, side)
    assert got["deep9"][1] == 10 and got["deep10"][1] == 11 and got["bushy4"][2] == 4 and got["bushy5"][2] == 5
    assert [got[f"wide{n}"][0] for n in (8, 9, 16, 17)] == [8, 9, 16, 17] and got["comb"] == (11, 4, 3) and got["gr1t2"][:2] == (5, 10)


def test_every_model_builds_and_is_what_it_is_there_for():
    """RobotModel / build_config.build accept every zoo model within the hard limits of include/grx.h; the properties each model is in the
    zoo for; the explicit damper's stability ratio kd dt / I <= 0.5 about every joint axis (I: the joint's own body about the axis through
    the joint origin -- a lower bound of its subtree's)."""
    from wiki_grx_gym_amd import _capi
    ident = np.eye(3)
    for key in robot_zoo.ZOO:
        cfg = cfg_of(key)
        c, _, meta = build_config.build(cfg, cfg.sim.dt, 2)
        rm, m = meta["model"], c.model
        nd = rm.num_dofs
        assert nd <= 32 and m.num_spheres <= 48 and m.num_pairs <= 192 and len(rm.self_collision_link_pairs) <= 48 and rm.num_links <= _capi.MAX_LINKS
        assert len({m.sph_link[i] for i in range(m.num_spheres)}) <= 24
        assert all(0 <= rm.parent[b] < b for b in range(1, rm.num_bodies))
        per_foot = [sum(1 for i in range(m.num_spheres) if m.sph_flags[i] & f) for f in (_capi.SPH_FOOT_LEFT, _capi.SPH_FOOT_RIGHT)]
        assert m.foot_body[0] >= 1 and m.foot_body[1] >= 1 and all(1 <= n <= 4 for n in per_foot), (key, per_foot)
        assert cfg.env.num_obs == 9 + 3 * nd and cfg.env.num_pri_obs == cfg.env.num_obs + 8 + 121
        assert (0.5 <= rm.mass).all() and (rm.mass <= 5.5).all(), (key, rm.mass)
        for b in range(1, rm.num_bodies):
            a, r = rm.joint_axis[b], rm.com[b]
            I = a @ (rm.inertia[b] + rm.mass[b] * (r @ r * ident - np.outer(r, r))) @ a
            assert abs(np.linalg.norm(a) - 1) < 1e-12 and c.kd[b - 1] * cfg.sim.dt / I <= 0.5, (key, b, c.kd[b - 1] * cfg.sim.dt / I)
        if key == "skew":
            assert all(np.abs(rm.joint_axis[b]).max() < 0.9 and np.abs(rm.joint_axis[b]).min() > 0.1 and np.abs(rm.joint_rot0[b] - ident).max() > 0.1 for b in range(1, rm.num_bodies))
            assert sum(bool((rm.joint_axis[b] < 0).any()) for b in range(1, rm.num_bodies)) >= 4
        if key == "shapes":
            nsph = lambda b: sum(1 for i in range(m.num_spheres) if m.sph_body[i] == b)
            depth = lambda b: 0 if rm.parent[b] == 0 else 1 + depth(rm.parent[b])
            assert nsph(0) == 5 and nsph(1) == 5 and len({m.sph_link[i] for i in range(m.num_spheres) if m.sph_body[i] == 1}) == 2
            assert sorted(per_foot) == [1, 4] and m.foot_body[0] in rm.parent and m.forehead_body == -1
            assert m.torso_body >= 1 and depth(m.torso_body) > max(depth(m.foot_body[0]), depth(m.foot_body[1]))
            assert not any(m.sph_flags[i] & _capi.SPH_TERMINATE for i in range(m.num_spheres) if m.sph_body[i] == 0) and any(m.sph_flags[i] & _capi.SPH_TERMINATE for i in range(m.num_spheres))
        if key.startswith("pairs"):
            assert m.num_pairs == int(key[5:])
            assert any(m.sph_body[m.pair_a[k]] == 0 for k in range(m.num_pairs))                                          # base x limb
            if m.num_pairs % 2:   # the odd pair: its lower URDF link rides on the higher body, and it is the 33rd pair of pairs33
                odd = [k for k in range(m.num_pairs) if m.sph_link[m.pair_a[k]] > m.sph_link[m.pair_b[k]]]
                assert len(odd) == 1 and (key != "pairs33" or odd == [32])
    cfg = cfg_of("gr1t2")
    c, _, meta = build_config.build(cfg, cfg.sim.dt, 2)
    assert meta["model"].key == "gr1t2" and c.model.num_bodies == 33 and c.model.num_pairs > 64


@pytest.mark.parametrize("kind,message", [("dofs", "too many DOFs"), ("spheres", "too many collision spheres")])
def test_a_model_over_a_hard_limit_is_refused(kind, message, zoo):
    """33 DOFs (GRX_MAX_DOFS = 32), 49 collision spheres (GRX_MAX_SPHERES = 48): RobotModel's ValueError, not an index error further on."""
    from wiki_grx_gym_amd.model import RobotModel
    robot_zoo.write(zoo, "over_" + kind, robot_zoo.over_limit(kind))
    try:
        with pytest.raises(ValueError, match=message):
            RobotModel("over_" + kind)
    finally:
        os.remove(os.path.join(zoo, "over_" + kind + ".model.json"))


# ---------------------------------------------------------------------------------------------------------------- the bands
CLASSES = tuple(dict.fromkeys(s.cls for s in ZOO_SCENES.values()))


@pytest.mark.parametrize("cls", CLASSES)
def test_the_band_is_the_fp32_oracles_own_error(cls):
    """tests/test_substep_parity.py's conditions, per scene of the class: the fp32 oracle inside ZOO_BAND / SENS_K x 1.25, every regime
    counter the scene is there for >= 100 env-sub-steps, no row of the fp32 oracle out of band or with a differing discrete output (stairs:
    at most one of the three), contact thresholds the other way in at most three quarters of the allowed rows; over the class the table is
    not looser than its measurement either."""
    band = robot_zoo.ZOO_BAND[cls]
    top = {n: 0.0 for n in band}
    problems = []
    for name, scene in ZOO_SCENES.items():
        if scene.cls != cls:
            continue
        mx, cmp, traj = substep.measure_fp32(name)
        counters = substep.regime_counters(traj)
        print("zoo fp32:", json.dumps({"scene": name, "max": {n: float(f"{v:.3e}") for n, v in mx.items()}, "counters": counters,
                                       "flag_rows": int(cmp["flags"].sum()), "threshold_rows": int(cmp["thresholds"].sum())}))
        for n in scene.banded:
            top[n] = max(top[n], mx[n])
            if mx[n] > band[n] / SENS_K * ALLOW:
                problems.append(f"{name}: fp32 oracle {n} {mx[n]:.3e} beyond band / SENS_K x {ALLOW} = {band[n] / SENS_K * ALLOW:.3e}")
        for c in scene.reach:
            if counters[c] < MIN_REGIME:
                problems.append(f"{name}: regime {c} reached in {counters[c]} env-sub-steps only")
        out = cmp["flags"].clone()
        for n in scene.banded:
            out |= cmp["err"][n] > band[n]
        bad_cap, threshold_cap = substep.scene_caps(scene, traj.rows)
        if int(out.sum()) > bad_cap // 3:
            problems.append(f"{name}: {int(out.sum())} rows of the fp32 oracle out of band or with a differing discrete output")
        if int(cmp["thresholds"].sum()) > 3 * threshold_cap // 4:
            problems.append(f"{name}: {int(cmp['thresholds'].sum())} rows of the fp32 oracle with a contact threshold the other way (3 / 4 of the cap: {3 * threshold_cap // 4})")
    for n, v in top.items():
        if v * SENS_K * ALLOW < band[n]:
            problems.append(f"{cls}: ZOO_BAND[{n}] = {band[n]:.3e} is looser than SENS_K x the measured {v:.3e}")
    assert not problems, "\n".join(problems)


def test_the_recorded_maxima_give_the_committed_band():
    """profiles/zoo_bands.json (python -m tests.robot_zoo) is what ZOO_BAND was taken from."""
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "zoo_bands.json")) as f:
        rec = json.load(f)
    assert rec["sens_k"] == SENS_K and set(rec["maxima"]) == set(ZOO_SCENES)
    assert substep.band_from(rec["maxima"]) == robot_zoo.ZOO_BAND == rec["band"]


def test_scenes_are_what_the_tier_was_designed_for():
    """One sub-step per step, 64 envs; a drop scene per model, a flight scene per model with self-collision pairs (pairs65 a second time
    with every second sphere pair listed higher body first), stairs for skew only."""
    for scene in ZOO_SCENES.values():
        cfg, ter = substep.scene_cfg(scene)
        assert cfg.control.decimation == 1 and not cfg.domain_rand.push_robots and scene.N == 64 and cfg.asset.model == scene.model
        assert cfg.domain_rand.randomize_friction and cfg.domain_rand.randomize_base_mass
    c = substep.build_struct(ZOO_SCENES["pairs65_swapped"])[1]
    higher_first = [k for k in range(c.model.num_pairs) if c.model.sph_body[c.model.pair_a[k]] > c.model.sph_body[c.model.pair_b[k]]]
    assert len(higher_first) == 33 and [s.name for s in ZOO_SCENES.values() if s.swap_pairs] == ["pairs65_swapped"]
    assert {s.model for s in ZOO_SCENES.values() if s.script == "drop"} == set(robot_zoo.MODELS)
    assert {s.model for s in ZOO_SCENES.values() if s.script == "spread"} == set(robot_zoo.WITH_PAIRS)
    assert [s.model for s in ZOO_SCENES.values() if s.ground != "plane"] == ["skew"] and not set(ZOO_SCENES) & set(substep.SCENES)
