"""The sub-step tier: every step kernel against the fp64 oracle ONE physics sub-step at a time.

A policy step is ten stiff-contact sub-steps, which amplify rounding 1e2-1e4 x (tests/test_hip_parity.py lives with that through outlier
fractions, twins and hard caps).  `control.decimation` is a run-time field, so the same kernels run with ONE sub-step per step, and from
an identical fp32 state nothing is amplified: a tensor's band is then SENS_K x the error of the fp32 oracle against the fp64 oracle on
the same trajectories, and a row is either inside it or counted against a small, fixed cap (scene_caps).

  * Scene / SCENES            what is simulated: robot, terrain head, domain randomisation, actions, (re)placement of the robots;
  * oracle_trajectory(name)   the fp64 oracle owns the state.  Before every sub-step its published (fp32) state is recorded and imported
                              back, so that every side starts from the same fp32 values; the record is cached per scene;
  * replay(traj, sim)         any other simulator (the fp32 oracle, a HIP handle in any layout) from the recorded pre-states;
  * compare / check           per env row against the fp64 results; regime_counters says what the trajectory exercised.

What this tier does not see is left to the policy-step tests: anything between sub-steps (the self_near margin over a step, noise_seq, the
averaged feet tensors over more than one sub-step) and, at the coordinates of a curriculum grid's far side, stairs: the *_far scenes below
hold the plane and the smooth raster at 128-256 m from the origin (the last 64 envs of a 4096-env plane grid, the far tile of the default
10 x 20 grid with its 25 m border) to bands measured there; a riser within rounding of a contact sphere is 16-32 x as frequent there, and the
maxima it gives bound nothing (profiles/substep_bands.json records them, unasserted)."""
import dataclasses
import json
import os
import types
from dataclasses import dataclass

import numpy as np
import torch

from tests import robot_zoo
from tests.helpers import STATE_TENSORS, make_cfg, random_actions
from wiki_grx_gym_amd.envs import build_config

SENS_K = 10.0             # how far a kernel may sit beyond the oracle's own fp32 response (tests/test_hip_parity.SENS_K)
SUBSTEPS = 600
REPLACE_EVERY = 300       # raster scenes: the robots are placed again
THRESHOLD_FRAC = 2e-4     # rows in which a contact THRESHOLD falls the other way within rounding, of a test's env-sub-steps: an anchor's active flag
                          # (first touch / lift-off: penetration > 0), an anchor that sticks on one side and slips on the other (|ft| > mu fn: the
                          # slipping side drags it by ct u / kt, millimetres -- seen as a position beyond ANCHOR_EVENT) or FEET_CONTACT (foot force
                          # > 1 N; the oracles differ by 0.2 N there).  The fp32 oracle alone: at most 5 rows in 38 400
ANCHOR_EVENT = 1e-4       # [m] an anchor further out than this was captured or dragged by another branch, not by rounding
FAR_ULP_RATIO = 8         # far scenes: the fp32 ulp at 128-256 m (2^-16) over that at 16-32 m (2^-19), where THRESHOLD_FRAC was set -- a threshold falls the
                          # other way in proportion to the rounding of the positions that decide it.  The fp32 oracle alone: at most 30 rows in 38 400
STAIRS_BAD_ROWS = 3       # stairs scenes: rows out of band or with a differing flag (a contact sphere within rounding of a riser / cell edge)

COMPARED = ("DOF_POS", "DOF_VEL", "ROOT_STATES", "TORQUES", "BASE_LIN_VEL", "BASE_ANG_VEL", "PROJECTED_GRAVITY", "FEET_POS",
            "FEET_CONTACT_FORCE", "CONTACT_FORCES", "AVG_FEET_FORCE", "AVG_FEET_SPEED", "REW")
EXACT = ("RESET", "TIME_OUT", "EPISODE_LENGTH")
RECORDED = COMPARED + ("ANCHORS", "FEET_CONTACT") + EXACT
BANDED = COMPARED + ("ANCHORS", "ANCHOR_SPEED")   # ANCHORS: the anchors' xy [m]; ANCHOR_SPEED: their third column, the approach speed at first touch [m/s]

# SENS_K x the largest |fp32 oracle - fp64 oracle| over the class's scenes below (profiles/substep_bands.json holds the maxima per scene;
# tests/test_substep_parity.py measures them again and holds this table to them).
SUBSTEP_BAND = {
    "plane": {"DOF_POS": 7.8e-05, "DOF_VEL": 0.039, "ROOT_STATES": 0.0004, "TORQUES": 0.00084, "BASE_LIN_VEL": 0.00017, "BASE_ANG_VEL": 0.00041, "PROJECTED_GRAVITY": 4.8e-06, "FEET_POS": 3.9e-05, "FEET_CONTACT_FORCE": 2.6, "CONTACT_FORCES": 2.6, "AVG_FEET_FORCE": 1.2, "AVG_FEET_SPEED": 0.0024, "REW": 0.00077, "ANCHORS": 5.8e-05, "ANCHOR_SPEED": 1.5e-05},
    "raster": {"DOF_POS": 9.8e-05, "DOF_VEL": 0.05, "ROOT_STATES": 0.00035, "TORQUES": 0.00077, "BASE_LIN_VEL": 9.1e-05, "BASE_ANG_VEL": 0.00055, "PROJECTED_GRAVITY": 4.2e-06, "FEET_POS": 9.6e-06, "FEET_CONTACT_FORCE": 3.7, "CONTACT_FORCES": 3.7, "AVG_FEET_FORCE": 2.6, "AVG_FEET_SPEED": 0.0029, "REW": 0.00024, "ANCHORS": 2.7e-05, "ANCHOR_SPEED": 0.00012},
    "full": {"DOF_POS": 0.00034, "DOF_VEL": 0.17, "ROOT_STATES": 0.0018, "TORQUES": 0.00039, "BASE_LIN_VEL": 9.9e-05, "BASE_ANG_VEL": 0.0017, "PROJECTED_GRAVITY": 4.2e-06, "FEET_POS": 3.9e-05, "FEET_CONTACT_FORCE": 2.3, "CONTACT_FORCES": 3.9, "AVG_FEET_FORCE": 1.5, "AVG_FEET_SPEED": 0.0025, "REW": 0.00022, "ANCHORS": 5.8e-05, "ANCHOR_SPEED": 1.5e-05},
    # the same at 128-256 m from the origin (the *_far scenes), over the rows that are no threshold rows (banded_rows)
    "plane_far": {"DOF_POS": 0.00079, "DOF_VEL": 0.4, "ROOT_STATES": 0.0032, "TORQUES": 0.00073, "BASE_LIN_VEL": 0.0013, "BASE_ANG_VEL": 0.0034, "PROJECTED_GRAVITY": 6.6e-06, "FEET_POS": 0.00046, "FEET_CONTACT_FORCE": 21.0, "CONTACT_FORCES": 21.0, "AVG_FEET_FORCE": 9.1, "AVG_FEET_SPEED": 0.019, "REW": 0.012, "ANCHORS": 0.00077, "ANCHOR_SPEED": 1.5e-05},
    "raster_far": {"DOF_POS": 0.00043, "DOF_VEL": 0.22, "ROOT_STATES": 0.0034, "TORQUES": 0.00069, "BASE_LIN_VEL": 0.0013, "BASE_ANG_VEL": 0.0035, "PROJECTED_GRAVITY": 6.6e-06, "FEET_POS": 0.00031, "FEET_CONTACT_FORCE": 17.0, "CONTACT_FORCES": 17.0, "AVG_FEET_FORCE": 6.8, "AVG_FEET_SPEED": 0.016, "REW": 0.0045, "ANCHORS": 0.00046, "ANCHOR_SPEED": 1.5e-05},
    "full_far": {"DOF_POS": 0.0027, "DOF_VEL": 1.4, "ROOT_STATES": 0.03, "TORQUES": 0.00062, "BASE_LIN_VEL": 0.0042, "BASE_ANG_VEL": 0.031, "PROJECTED_GRAVITY": 4.2e-05, "FEET_POS": 0.00031, "FEET_CONTACT_FORCE": 18.0, "CONTACT_FORCES": 47.0, "AVG_FEET_FORCE": 7.7, "AVG_FEET_SPEED": 0.02, "REW": 0.0041, "ANCHORS": 0.00046, "ANCHOR_SPEED": 1.8e-05},
}


@dataclass(frozen=True)
class Scene:
    name: str
    cls: str                      # band class: "plane" / "raster" (lower limb), "full" (32-DOF body); "*_far": the same at 128-256 m from the origin
    task: str = "GR1T1"
    model: str = None             # a model of tests/robot_zoo.py instead of a task (the test points model.ASSET_DIR at the zoo: robot_zoo.install)
    ground: str = "plane"         # "plane" / "slope" / "stairs"
    mesh: str = "plane"           # terrain head: "plane" / "heightfield" / "trimesh"
    N: int = 64
    friction: tuple = None        # domain_rand.friction_range override
    scales: tuple = (0.5, 0.5)    # action scale of the first / second half of the run
    script: str = None            # "legs": the leg-crossing poses of test_self_collision_matches_the_oracle, in flight; zoo models: "drop" (from
                                  # 0.1-0.3 m onto the ground, joints near the default pose), "spread" (in flight, joints over 90 % of their ranges)
    base: bool = False            # legged_gym's base reward terms on (the *_base kernel entries)
    seed: int = 1
    episode_s: float = None       # env.episode_length_s: 0.5 s = 250 sub-steps, so that every env also times out within the run
    slip_dominates: bool = False  # low friction: the anchors of most rows in foot contact are dragged
    swap_pairs: bool = False      # every second self-collision sphere pair handed over as (b, a): the higher body first, which model.fill_model never emits
                                  # (build_gen_tables' `ba > bb` swap; the pairs of one link pair then arrive in both orders)
    reach: tuple = ()             # regime counters this scene is meant to reach (>= MIN_REGIME env-sub-steps)
    env_offset: int = 0           # plane scenes: these N envs are [env_offset, env_offset + N) of a grid of total_envs (None: of N) -- the far scenes are
    total_envs: int = None        # the last 64 of 4096: x = 189 m, y = 0-189 m
    tile: tuple = None            # raster scenes: the 80 x 80 raster is tile (row, col) of a `grid` = (rows, cols) curriculum raster that is zero elsewhere,
    grid: tuple = None            # inside FAR_BORDER m of border (None: the raster is the whole terrain, without border)

    @property
    def stairs(self):
        return self.ground == "stairs"

    @property
    def far(self):
        """128-256 m from the origin: threshold rows (compare) make no band and are held by their own cap alone, FAR_ULP_RATIO x as wide."""
        return self.cls.endswith("_far")

    @property
    def tile_corner(self):
        """World xy [m] of the raster's low corner."""
        return (self.tile[0] * TILE_M, self.tile[1] * TILE_M) if self.tile else (0.0, 0.0)

    @property
    def banded(self):
        """The tensors held to the band.  The oracle has no base reward terms (tests/test_base_rewards_gpu.py pins them to the reference's
        fixture): a *_base entry is compared for its physics -- a separate instantiation of the same body -- and not for REW."""
        return tuple(n for n in BANDED if not (self.base and n == "REW"))


MIN_REGIME = 100
_CONTACT = ("foot_contact", "first_touch", "slip", "bounce")
_FALLS = ("non_foot_load", "joint_limit", "velocity_clamp", "reset")
SCENES = {s.name: s for s in (
    Scene("plane", "plane", scales=(1.0, 0.5), episode_s=0.5, reach=_CONTACT + _FALLS),
    Scene("plane_t2", "plane", task="GR1T2", scales=(1.0, 0.5), episode_s=0.5, reach=_CONTACT + _FALLS),
    Scene("plane_n50", "plane", N=50, scales=(0.5, 1.0), seed=3, episode_s=0.5, reach=_CONTACT + _FALLS),
    Scene("plane_lowmu", "plane", friction=(0.05, 0.2), slip_dominates=True, reach=_CONTACT),
    Scene("legs", "plane", script="legs", scales=(1.0, 1.0), seed=5, reach=("self_collision", "non_foot_load")),
    Scene("slope_hf", "raster", ground="slope", mesh="heightfield", reach=_CONTACT),
    Scene("slope_tm", "raster", ground="slope", mesh="trimesh", reach=_CONTACT),
    Scene("stairs_hf", "raster", ground="stairs", mesh="heightfield", friction=(0.05, 0.05), seed=2, reach=_CONTACT + ("face_contact", "non_foot_load")),
    Scene("stairs_tm", "raster", ground="stairs", mesh="trimesh", friction=(0.05, 0.05), seed=2, reach=_CONTACT + ("face_contact", "non_foot_load")),
    Scene("full_plane", "full", task="GR1T1Full", reach=_CONTACT + ("non_foot_load", "joint_limit", "velocity_clamp")),
    Scene("full_stairs", "full", task="GR1T1Full", ground="stairs", mesh="trimesh", friction=(0.05, 0.05), seed=2,
          reach=_CONTACT + ("face_contact", "non_foot_load", "self_collision", "joint_limit", "velocity_clamp", "reset")),
    Scene("base_plane", "plane", base=True, scales=(0.5, 1.0), reach=_CONTACT),
    Scene("base_full_plane", "full", task="GR1T1Full", base=True, reach=_CONTACT),
)}

# The far side of a real run: each scene is its near twin -- seed, scales, episode, reach -- at 128-256 m, in a band class of its own (fp32 is
# 5-30 x less accurate per sub-step there: profiles/substep_bands.json, "far": "over_near").
TILE_M = 8.0              # an 80 x 80 raster at 0.1 m per cell
FAR_BORDER = 25.0         # [m] terrain.border_size of the curriculum grid
FAR_GRID = (10, 20)       # terrain.num_rows x num_cols: with the border a 1300 x 2100 raster
FAR_TILE = (9, 19)        # its far tile: world (72..80, 152..160) m
FAR_TOTAL = 4096


def _far(near, cls, **kw):
    s = SCENES[near]
    where = dict(tile=FAR_TILE, grid=FAR_GRID) if s.ground != "plane" else dict(env_offset=FAR_TOTAL - s.N, total_envs=FAR_TOTAL)
    return dataclasses.replace(s, name=near + "_far", cls=cls, **where, **kw)


SCENES.update({s.name: s for s in (
    _far("plane", "plane_far"),
    _far("plane_t2", "plane_far"),
    _far("base_plane", "plane_far"),
    _far("slope_hf", "raster_far"),
    _far("slope_tm", "raster_far"),
    # The 32-DOF body under half-scale actions mostly stands, its feet near the edge of the friction cone: at 189 m the fp32 oracle ALONE lets
    # stick / slip fall the other way in 40-60 rows (seeds 1-8; the cap is 61, and a scene's reference may use half of it), and under quarter-scale
    # actions in 54-102.  Full-scale actions and friction 1.0-1.25 leave 16-23 rows on the plane and 22-37 on the slope (seeds 1-4), and every
    # regime of the near twin is still reached.
    _far("full_plane", "full_far", scales=(1.0, 1.0), friction=(1.0, 1.25)),
    dataclasses.replace(_far("slope_tm", "full_far", scales=(1.0, 1.0), friction=(1.0, 1.25), seed=4), name="full_slope_tm_far", task="GR1T1Full",
                        reach=SCENES["full_plane"].reach),      # (the tree and generic kernels' terrain path at far coordinates)
)})

# Recorded by python -m tests.substep, asserted nowhere: the last 64 envs of a 32768-env plane grid (543 m: the fp32 oracle alone breaks the
# threshold cap) and stairs on the far tile (the maxima are riser- and cell-side events).
INFO_SCENES = {s.name: s for s in (
    dataclasses.replace(SCENES["plane"], name="plane_32768", cls="info", env_offset=32768 - 64, total_envs=32768),
    _far("stairs_hf", "info"),
    _far("stairs_tm", "info"),
)}


# The zoo (tests/robot_zoo.py), one band class per model (stairs: one of its own); python -m tests.robot_zoo measures ZOO_BAND.
_DROP = _CONTACT + ("reset", "joint_limit")   # (reset: termination contacts and the 0.3 s time-outs)
ZOO_SCENES = {s.name: s for s in (
    [Scene(f"{m}_drop", m, model=m, script="drop", scales=(1.0, 0.5), seed=1, episode_s=0.3,
           reach=_CONTACT + ("reset",) if m.startswith("wide") else _DROP)   # (wide*: the spokes carry the base, their joints stay inside the limits)
     for m in robot_zoo.MODELS]
    + [Scene(f"{m}_spread", m, model=m, script="spread", scales=(1.0, 1.0), seed=5, reach=("self_collision",)) for m in robot_zoo.WITH_PAIRS]
    + [Scene("pairs65_swapped", "pairs65", model="pairs65", script="spread", scales=(1.0, 1.0), seed=6, swap_pairs=True, reach=("self_collision",))]
    + [Scene("skew_stairs", "skew_stairs", model="skew", ground="stairs", mesh="trimesh", friction=(0.05, 0.05), seed=2, reach=_CONTACT + ("face_contact",))])}


def scene_of(name):
    return SCENES[name] if name in SCENES else INFO_SCENES[name] if name in INFO_SCENES else ZOO_SCENES[name]


def band_of(scene):
    return SUBSTEP_BAND[scene.cls] if scene.cls in SUBSTEP_BAND else robot_zoo.ZOO_BAND[scene.cls]


def substep_cfg(task="GR1T1", terrain="plane", **kw):
    """tests.helpers.make_cfg with ONE physics sub-step per step."""
    cfg = make_cfg(task=task, terrain=terrain, **kw)
    cfg.control.decimation = 1
    return cfg


def one_tile_scene(kind, tile=None, grid=None):
    """A 1 x 1 terrain without border from an 80 x 80 raster (8 m at 0.1 m per cell; what tests/test_terrain_golden._trimesh_tile hands to
    build_config).  "stairs": the golden pyramid-stairs raster.  "slope": 2 raster units (0.01 m) up per cell along x -- every cell and
    both of its triangle halves lie in one plane, so a cell edge is no event on either terrain head.
    With `tile` and `grid`: the same raster as tile (row, col) of a grid of rows x cols tiles inside FAR_BORDER m of border, zero everywhere
    else; every env origin is that tile's low corner, so that a reset lands where the one-tile scene's does, shifted."""
    if kind == "stairs":
        from tests.test_terrain_golden import _trimesh_tile
        blk = _trimesh_tile("stairs")[2]
    elif kind == "slope":
        blk = (2 * np.arange(80, dtype=np.int16)[:, None] * np.ones((1, 80), np.int16)).astype(np.int16)
    else:
        raise KeyError(kind)
    if tile is None:
        return types.SimpleNamespace(heightsamples=np.ascontiguousarray(blk), env_origins=np.zeros((1, 1, 3), np.float32))
    border = int(round(FAR_BORDER * 80 / TILE_M))
    hs = np.zeros((grid[0] * 80 + 2 * border, grid[1] * 80 + 2 * border), np.int16)
    r0, c0 = border + tile[0] * 80, border + tile[1] * 80
    hs[r0:r0 + 80, c0:c0 + 80] = blk
    org = np.zeros(tuple(grid) + (3,), np.float32)
    org[..., 0], org[..., 1] = tile[0] * TILE_M, tile[1] * TILE_M
    return types.SimpleNamespace(heightsamples=hs, env_origins=org)


def scene_cfg(scene):
    """(cfg, terrain or None) of a scene."""
    cfg = substep_cfg(robot_zoo.cfg_class(scene.model) if scene.model else scene.task, scene.mesh, curriculum=False, dr=True, push=False)
    ter = None
    if scene.ground != "plane":
        ter = one_tile_scene(scene.ground, scene.tile, scene.grid)
        cfg.terrain.border_size = FAR_BORDER if scene.tile else 0.0
        cfg.terrain.num_rows, cfg.terrain.num_cols = scene.grid if scene.tile else (1, 1)
    if scene.friction is not None:
        cfg.domain_rand.randomize_friction = True
        cfg.domain_rand.friction_range = list(scene.friction)
        if scene.friction[0] == scene.friction[1]:
            cfg.terrain.static_friction = cfg.terrain.dynamic_friction = scene.friction[0]
    if scene.episode_s is not None:
        cfg.env.episode_length_s = scene.episode_s
    if scene.base:
        from tests.test_base_rewards import FIXTURE
        d = np.load(FIXTURE)
        for n, v in zip(d["names"], d["scales"]):
            setattr(cfg.rewards.scales, str(n), float(v))
    return cfg, ter


def build_struct(scene):
    cfg, ter = scene_cfg(scene)
    c, keep, meta = build_config.build(cfg, cfg.sim.dt, scene.N, scene.env_offset, scene.total_envs, scene.seed, ter)
    if scene.swap_pairs:
        for k in range(0, c.model.num_pairs, 2):
            c.model.pair_a[k], c.model.pair_b[k] = c.model.pair_b[k], c.model.pair_a[k]
    return cfg, c, keep, meta


def make_oracle(scene, precision):
    from oracle.binding import OracleSim
    cfg, c, keep, meta = build_struct(scene)
    return OracleSim(c, precision, keep), cfg, meta


def make_hip(scene):
    from wiki_grx_gym_amd.sim import HipSim
    cfg, c, keep, _ = build_struct(scene)
    return HipSim(c, "cuda:0", keep)


def _place_on_tile(ora, q0, gen, height=0.93, corner=(0.0, 0.0)):
    """tests/test_hip_parity.stairs_tile_scene's placement: spread over the tile (whose low corner is at `corner`), 0.93 m (the GR1's standing
    height; `height`) above the ground under them, moving at 0.8-1.2 m/s in a random direction."""
    N = ora.num_envs
    root = torch.zeros(N, 13)
    root[:, 6] = 1.0
    xy = 1.0 + 5.9 * torch.rand(N, 2, generator=gen) + torch.tensor(corner)
    root[:, 0:2] = xy
    for i in range(N):
        root[i, 2] = float(ora.terrain(float(xy[i, 0]), float(xy[i, 1]))[0]) + height
    ang = 6.2832 * torch.rand(N, generator=gen)
    speed = 0.8 + 0.4 * torch.rand(N, generator=gen)
    root[:, 7] = speed * torch.cos(ang)
    root[:, 8] = speed * torch.sin(ang)
    ora.set_state(root.contiguous(), q0.contiguous(), torch.zeros_like(q0))


def _place_legs_crossed(ora, gen):
    """Robots in flight with both hips adducted, knees and feet crossing, joints moving: the legs collide with each other and nothing
    touches the ground."""
    N = ora.num_envs
    root = torch.zeros(N, 13)
    root[:, 2] = 3.0
    root[:, 6] = 1.0
    root[:, 7:13] = torch.randn(N, 6, generator=gen) * 0.3
    q = torch.tensor([[-0.35, 0.0, -0.3, 0.6, -0.3, 0.35, 0.0, -0.3, 0.6, -0.3]]).repeat(N, 1)
    q += (torch.rand(N, 10, generator=gen) - 0.5) * torch.tensor([0.5, 0.8, 0.8, 0.6, 0.4] * 2)
    qd = torch.randn(N, 10, generator=gen) * 2.0
    ora.set_state(root.contiguous(), q.contiguous(), qd.contiguous())


def _place_drop(ora, rm, q0, gen):
    """Zoo models: the base tilted by up to ~0.2 rad, the joints within 0.2 rad of the default pose (inside their limits), the lowest collision
    sphere 0.1-0.3 m above the plane, at rest."""
    from tests.kinematics_ref import BodyKinematics
    N = ora.num_envs
    lo, hi = torch.tensor(rm.dof_lower, dtype=torch.float32), torch.tensor(rm.dof_upper, dtype=torch.float32)
    q = torch.minimum(torch.maximum(q0 + 0.4 * (torch.rand(N, rm.num_dofs, generator=gen) - 0.5), lo), hi)
    root = torch.zeros(N, 13)
    quat = torch.cat([0.1 * torch.randn(N, 3, generator=gen), torch.ones(N, 1)], 1)
    root[:, 3:7] = quat / quat.norm(dim=1, keepdim=True)
    root[:, 2] = 0.1 + 0.2 * torch.rand(N, generator=gen) - robot_zoo.lowest_point(rm, BodyKinematics(rm, "cpu"), root, q)
    ora.set_state(root.contiguous(), q.contiguous(), torch.zeros_like(q))


def _place_spread(ora, rm, gen):
    """Zoo models in flight (3 m up), every joint anywhere in 90 % of its range and moving: the poses in which the model's self-collision
    pairs carry load."""
    N = ora.num_envs
    lo, hi = torch.tensor(rm.dof_lower, dtype=torch.float32), torch.tensor(rm.dof_upper, dtype=torch.float32)
    root = torch.zeros(N, 13)
    root[:, 2] = 3.0
    root[:, 6] = 1.0
    root[:, 7:13] = torch.randn(N, 6, generator=gen) * 0.3
    q = (lo + hi) / 2 + (2 * torch.rand(N, rm.num_dofs, generator=gen) - 1) * 0.9 * (hi - lo) / 2
    qd = torch.randn(N, rm.num_dofs, generator=gen)
    ora.set_state(root.contiguous(), q.contiguous(), qd.contiguous())


LEGS_REPLACE_EVERY = 60   # (the original script runs six policy steps = 60 sub-steps; at 3 m the ground stays out of reach)


@dataclass
class Trajectory:
    scene: Scene
    pre: dict          # STATE_TENSORS -> (T, N, ...) as the fp64 oracle published them (fp32 / integer views)
    actions: torch.Tensor
    delays: list
    ref: dict          # RECORDED -> (T, N, ...) fp64 oracle results, as published (fp32)
    info: dict         # feet links, joint limits, thresholds: what regime_counters needs

    @property
    def rows(self):
        return self.actions.shape[0] * self.actions.shape[1]


def _snapshot(sim, names):
    return {n: sim.tensor(n).detach().clone() for n in names}


def run_oracle(scene, steps=SUBSTEPS):
    """The fp64 oracle's trajectory of a scene.  Every sub-step starts from the state the oracle PUBLISHED (fp32), imported back into it."""
    ora, cfg, meta = make_oracle(scene, "f64")
    N = scene.N
    ora.reset_all()
    q0 = ora.tensor("DOF_POS").clone()
    gen = torch.Generator().manual_seed(100 + scene.seed)
    pgen = torch.Generator().manual_seed(200 + scene.seed)
    pre, ref, acts, delays = [], [], [], []
    for t in range(steps):
        if scene.ground != "plane" and t % REPLACE_EVERY == 0:
            _place_on_tile(ora, q0, pgen, *([robot_zoo.rest_height(scene.model) + 0.1] if scene.model else []), corner=scene.tile_corner)
        if scene.script == "drop" and t % REPLACE_EVERY == 0:
            _place_drop(ora, meta["model"], q0, pgen)
        if scene.script == "spread" and t % LEGS_REPLACE_EVERY == 0:
            _place_spread(ora, meta["model"], pgen)
        if scene.script == "legs" and t % LEGS_REPLACE_EVERY == 0:
            _place_legs_crossed(ora, pgen)
        pre.append(_snapshot(ora, STATE_TENSORS))
        ora.import_state()
        a = random_actions(cfg, N, gen, scene.scales[0] if t < steps // 2 else scene.scales[1])
        delay = 0.0 if t % 2 == 0 else 5.0      # (one sub-step: 0.0 drives the torque from `actions`, 5.0 from `last_actions`)
        ora.step(a, delay, t + 1)
        acts.append(a)
        delays.append(delay)
        ref.append(_snapshot(ora, RECORDED))
    m = ora._keep[-1].model
    nd = ora.num_dofs
    info = {"feet_links": list(meta["feet_links"]),
            "dof_lower": torch.tensor([m.dof_lower[j] for j in range(nd)], dtype=torch.float32),
            "dof_upper": torch.tensor([m.dof_upper[j] for j in range(nd)], dtype=torch.float32),
            "dof_vel_limit": torch.tensor([m.dof_vel_limit[j] for j in range(nd)], dtype=torch.float32),
            "bounce_threshold_velocity": float(ora._keep[-1].bounce_threshold_velocity)}
    ora.close()
    stack = lambda rows: {n: torch.stack([r[n] for r in rows]) for n in rows[0]}
    return Trajectory(scene, stack(pre), torch.stack(acts), delays, stack(ref), info)


_cache = {}


def oracle_trajectory(name):
    """run_oracle(SCENES[name]), computed once.  One scene is kept at a time (some 50-80 MB): tests that share a scene sit next to each
    other in their parametrisation."""
    if name not in _cache:
        _cache.clear()
        _cache[name] = run_oracle(scene_of(name))
    return _cache[name]


def replay(traj, sim):
    """Another simulator -- the fp32 oracle or a HIP handle -- through the recorded trajectory: before every sub-step its complete state
    (tests.helpers.STATE_TENSORS, ANCHORS included) is overwritten with the recorded one.  Returns RECORDED -> (T, N, ...) on the host."""
    dev = sim.device
    T = traj.actions.shape[0]
    pre = {n: v.to(dev) for n, v in traj.pre.items()}
    acts = traj.actions.to(dev)
    views = {n: sim.tensor(n) for n in STATE_TENSORS + RECORDED}
    out = {n: torch.empty((T,) + tuple(views[n].shape), dtype=views[n].dtype, device=dev) for n in RECORDED}
    sim.reset_all()
    for t in range(T):
        for n in STATE_TENSORS:
            views[n].copy_(pre[n][t])
        if hasattr(sim, "import_state"):
            sim.import_state()
        sim.step(acts[t], traj.delays[t], t + 1)
        for n in RECORDED:
            out[n][t].copy_(views[n])
    if dev.type == "cuda":
        torch.cuda.synchronize()
    return {n: v.cpu() for n, v in out.items()}


def regime_counters(traj):
    """Env-sub-steps of the fp64 trajectory in each contact / limit regime, from the exposed tensors alone."""
    pre, ref, info = traj.pre, traj.ref, traj.info
    on0, on1 = pre["ANCHORS"][..., 2] > 0, ref["ANCHORS"][..., 2] > 0                     # (T, N, 8)
    moved = (pre["ANCHORS"][..., :2] != ref["ANCHORS"][..., :2]).any(-1)
    cf = ref["CONTACT_FORCES"].double()                                                    # (T, N, links, 3)
    load = cf.norm(dim=-1)
    other = torch.ones(load.shape[2], dtype=torch.bool)
    other[info["feet_links"]] = False
    loaded = load > 1.0
    net = cf.sum(2).norm(dim=-1)                                                           # an internal force pair sums to zero
    q, qd = ref["DOF_POS"], ref["DOF_VEL"]
    return {
        "foot_contact": int(ref["FEET_CONTACT"].bool().any(-1).sum()),
        "first_touch": int((~on0 & on1).any(-1).sum()),
        "slip": int((on0 & on1 & moved).any(-1).sum()),
        "bounce": int((ref["ANCHORS"][..., 2] > info["bounce_threshold_velocity"]).any(-1).sum()),
        "non_foot_load": int(loaded[..., other].any(-1).sum()),
        # (beyond the friction cone of mu <= 0.2: a vertical face pushes -- tests/test_hip_parity.count_wall_contacts)
        "face_contact": int((cf[..., :2].norm(dim=-1) > 0.3 * cf[..., 2].abs() + 5.0).any(-1).sum()),
        "self_collision": int((loaded.any(-1) & (net < 1e-3 * load.amax(-1).clamp_min(1.0))).sum()),
        "joint_limit": int(((q < info["dof_lower"]) | (q > info["dof_upper"])).any(-1).sum()),
        "velocity_clamp": int((qd.abs() >= info["dof_vel_limit"]).any(-1).sum()),
        "reset": int(ref["RESET"].bool().sum()),
    }


def compare(traj, got):
    """Per env row against the fp64 results.  Returns
         err     BANDED -> (T, N) largest absolute error of the row (ANCHORS, ANCHOR_SPEED: over the anchors both sides hold active),
         flags   (T, N) bool: a discrete output (EXACT) differs,
         thresholds (T, N) bool: an anchor's active flag or FEET_CONTACT differs, or an anchor is further out than ANCHOR_EVENT."""
    ref = traj.ref
    T, N = traj.actions.shape[:2]
    err = {n: (got[n].double() - ref[n].double()).abs().reshape(T, N, -1).amax(-1) for n in COMPARED}
    on_g, on_r = got["ANCHORS"][..., 2] > 0, ref["ANCHORS"][..., 2] > 0
    d = (got["ANCHORS"].double() - ref["ANCHORS"].double()).abs()
    both = on_g & on_r
    dxy = torch.where(both, d[..., :2].amax(-1), torch.zeros_like(d[..., 0]))
    dragged = dxy > ANCHOR_EVENT
    err["ANCHORS"] = torch.where(dragged, torch.zeros_like(dxy), dxy).amax(-1)
    err["ANCHOR_SPEED"] = torch.where(both, d[..., 2], torch.zeros_like(d[..., 2])).amax(-1)
    flags = torch.zeros(T, N, dtype=torch.bool)
    for n in EXACT:
        flags |= (got[n].to(torch.int64) != ref[n].to(torch.int64)).reshape(T, N, -1).any(-1)
    feet = (got["FEET_CONTACT"].to(torch.int64) != ref["FEET_CONTACT"].to(torch.int64)).any(-1)
    return {"err": err, "flags": flags, "thresholds": (on_g != on_r).any(-1) | dragged.any(-1) | feet}


def banded_rows(scene, cmp):
    """(T, N) bool: the rows held to the band.  Far scenes: not the threshold rows -- two rows in which FEET_CONTACT fell the other way put the
    far slope's REW maximum at 0.02, against a 99.9 % quantile of 6.9e-5, and a band from them would bound nothing; their cap holds them."""
    return ~cmp["thresholds"] if scene.far else torch.ones_like(cmp["thresholds"])


def maxima(cmp, scene=None):
    """Largest error per tensor over the rows whose discrete outputs agree (a row that reset on one side only holds another episode); for a
    far `scene`, of those, over banded_rows."""
    keep = ~cmp["flags"] & (banded_rows(scene, cmp) if scene is not None else True)
    return {n: float(e[keep].max()) if keep.any() else 0.0 for n, e in cmp["err"].items()}


def scene_caps(scene, rows):
    """(rows that may be out of band or differ in a discrete output, rows in which a contact threshold may fall the other way) --
    conditions, not measurements."""
    return (STAIRS_BAD_ROWS if scene.stairs else 0), int(THRESHOLD_FRAC * rows * (FAR_ULP_RATIO if scene.far else 1))


def check(traj, got, label, log=None):
    """The sub-step conditions on `got` (a replay of traj): every row in band and every discrete output identical, but for the scene's
    caps.  Returns the report (also appended to `log`, a jsonl path, with every counted row)."""
    scene = traj.scene
    band = band_of(scene)
    cmp = compare(traj, got)
    out = torch.zeros_like(cmp["flags"])
    held = banded_rows(scene, cmp)
    rows = []
    for n in scene.banded:
        over = (cmp["err"][n] > band[n]) & held
        out |= over
        for t, i in torch.nonzero(over).tolist()[:20]:
            rows.append({"tensor": n, "substep": t, "env": i, "err": float(cmp["err"][n][t, i]), "band": band[n]})
    for t, i in torch.nonzero(cmp["flags"]).tolist()[:20]:
        rows.append({"tensor": "flags", "substep": t, "env": i,
                     "differ": [n for n in EXACT if not torch.equal(got[n][t, i].to(torch.int64), traj.ref[n][t, i].to(torch.int64))]})
    bad = int((out | cmp["flags"]).sum())
    thresholds = int(cmp["thresholds"].sum())
    mx = {n: float(cmp["err"][n][held].max()) for n in scene.banded}
    rec = {"scene": scene.name, "layout": label, "env_substeps": traj.rows, "max": {n: float(f"{v:.3e}") for n, v in mx.items()},
           "ratio_to_fp32_oracle": {n: round(mx[n] * SENS_K / band[n], 2) for n in scene.banded}, "bad_rows": bad, "threshold_rows": thresholds, "rows": rows}
    print("substep:", json.dumps(rec))
    if log:
        try:
            os.makedirs(os.path.dirname(os.path.abspath(log)), exist_ok=True)
            with open(log, "a") as f:
                f.write(json.dumps(rec) + "\n")
        except OSError:
            pass
    bad_cap, threshold_cap = scene_caps(scene, traj.rows)
    assert bad <= bad_cap, f"{scene.name} / {label}: {bad} rows out of band or with a differing discrete output (allowed: {bad_cap}): {rows[:8]}"
    assert thresholds <= threshold_cap, f"{scene.name} / {label}: {thresholds} rows in which a contact threshold fell the other way (anchor flags, stick / slip, FEET_CONTACT; allowed: {threshold_cap})"
    return rec


def measure_fp32(name):
    """(largest |fp32 oracle - fp64 oracle| per tensor, the comparison, the trajectory) of a scene."""
    traj = oracle_trajectory(name)
    o32 = make_oracle(traj.scene, "f32")[0]
    try:
        cmp = compare(traj, replay(traj, o32))
    finally:
        o32.close()
    return maxima(cmp, traj.scene), cmp, traj


def max_xy(traj):
    """Largest |x|, |y| [m] of a base over the recorded pre-states."""
    return float(traj.pre["ROOT_STATES"][..., :2].abs().max())


def band_from(per_scene):
    """SUBSTEP_BAND of measured maxima {scene: {tensor: max}}: SENS_K x the largest of the class, rounded up to two digits."""
    band = {}
    for name, mx in per_scene.items():
        b = band.setdefault(scene_of(name).cls, {})
        for n in scene_of(name).banded:
            b[n] = max(b.get(n, 0.0), SENS_K * mx[n])
    up = lambda v: float(np.format_float_scientific(v * (1 + 1e-9) + 0.5 * 10.0 ** (np.floor(np.log10(v)) - 1), precision=1)) if v > 0 else 0.0
    return {c: {n: up(v) for n, v in b.items()} for c, b in band.items()}


def write_zoo_bands():
    """python -m tests.robot_zoo: measure the zoo's bands inside robot_zoo.installed() (needs robot_zoo.ZOO_BAND only to exist), write profiles/zoo_bands.json, print ZOO_BAND."""
    per_scene, counters, rows = {}, {}, {}
    for name in ZOO_SCENES:
        per_scene[name], cmp, traj = measure_fp32(name)
        counters[name] = regime_counters(traj)
        rows[name] = {"flag_rows": int(cmp["flags"].sum()), "threshold_rows": int(cmp["thresholds"].sum())}
        print(name, counters[name], rows[name], flush=True)
    band = band_from(per_scene)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "profiles", "zoo_bands.json"), "w") as f:
        json.dump({"what": "largest |fp32 oracle - fp64 oracle| per zoo scene (tests/substep.ZOO_SCENES over tests/robot_zoo.py's models) and tensor: one "
                           "sub-step from identical fp32 state, 600 sub-steps, 64 envs; band = SENS_K x the largest of a class",
                   "sens_k": SENS_K, "maxima": per_scene, "regime_counters": counters, "fp32_rows": rows, "band": band}, f, indent=1)
    print("ZOO_BAND = {\n" + "\n".join(f"    {json.dumps(c)}: {json.dumps(b)}," for c, b in band.items()) + "\n}")


if __name__ == "__main__":      # python -m tests.substep: measure the bands again, write profiles/substep_bands.json, print SUBSTEP_BAND
    per_scene, counters, far_rows, info = {}, {}, {}, {}
    for name in SCENES:
        per_scene[name], cmp, traj = measure_fp32(name)
        counters[name] = regime_counters(traj)
        if traj.scene.far:
            far_rows[name] = {"max_xy_m": max_xy(traj), "flag_rows": int(cmp["flags"].sum()), "threshold_rows": int(cmp["thresholds"].sum()),
                              "threshold_cap": scene_caps(traj.scene, traj.rows)[1]}
        print(name, per_scene[name], far_rows.get(name, ""), flush=True)
    for name in INFO_SCENES:
        mx, cmp, traj = measure_fp32(name)
        info[name] = {"max_xy_m": max_xy(traj), "maxima": mx, "flag_rows": int(cmp["flags"].sum()), "threshold_rows": int(cmp["thresholds"].sum())}
        print(name, info[name], flush=True)
    band = band_from(per_scene)
    far_over_near = {c: {n: round(v / band[c[:-4]][n], 2) for n, v in b.items()} for c, b in band.items() if c.endswith("_far")}
    near = lambda d, far=False: {k: v for k, v in d.items() if k.endswith("_far") == far}      # (scene and class names alike)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "profiles", "substep_bands.json"), "w") as f:
        json.dump({"what": "largest |fp32 oracle - fp64 oracle| per scene and tensor over tests/substep.py's trajectories (one sub-step from identical "
                           "fp32 state, 600 sub-steps); band = SENS_K x the largest of a class.  maxima / regime_counters / band: the scenes near the "
                           "origin; far: the same for the *_far scenes (128-256 m from the origin), over the rows that are no threshold rows -- "
                           "fp32_rows holds the fp32 oracle's own flag and threshold rows against the cap the kernels are held to, over_near the far "
                           "band over its near class's.  info_only is asserted nowhere: the last 64 envs of a 32768-env plane grid and stairs on "
                           "the far tile, maxima over all rows",
                   "sens_k": SENS_K, "maxima": near(per_scene), "regime_counters": near(counters), "band": near(band),
                   "far": {"maxima": near(per_scene, True), "regime_counters": near(counters, True), "band": near(band, True), "fp32_rows": far_rows,
                           "over_near": far_over_near},
                   "info_only": info}, f, indent=1)
    print("SUBSTEP_BAND = " + json.dumps(band, indent=4))
