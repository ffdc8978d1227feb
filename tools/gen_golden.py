#!/usr/bin/env python3
"""Generate golden input/output vectors by IMPORTING THE REFERENCE PYTHON in the build container.

    python tools/gen_golden.py        # writes tests/golden/*.npz  (+ config dump json)

The reference (/root/reference) never travels to the GPU box; only the vectors produced here are
committed.  Physics (Isaac Gym / PhysX) is a closed, absent binary, so ``isaacgym``
is replaced by a stub: ``gymapi/gymtorch/gymutil`` are MagicMocks, ``torch_utils`` and
``terrain_utils`` are the real files.  The reference's own functions are then called on synthetic
state tensors: quaternion helpers, clip_actions/_compute_torques, the whole
``post_physics_step`` (state update, timers, termination, the 24 active reward terms,
observations incl. injected noise), ``_get_heights``, ``Terrain`` and the rsl_rl PPO pieces.
Those fixtures stub ``reset_idx`` out; ``gen_reset_family`` runs it live, fed with the build's own
random draws (which it takes from the oracle library: ``make -C oracle`` first).
"""
import importlib.util
import json
import os
import sys
import types
from unittest.mock import MagicMock

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


def install_stub():
    np.float = float  # torch_utils.py:135 default argument
    pkg = types.ModuleType("isaacgym")
    pkg.__path__ = []
    sys.modules["isaacgym"] = pkg
    for name in ("gymapi", "gymtorch", "gymutil"):
        m = MagicMock(name=name)
        sys.modules["isaacgym." + name] = m
        setattr(pkg, name, m)
    base = os.path.join(REF, "IsaacGym_Preview_4_Package/isaacgym/python/isaacgym")
    for name in ("torch_utils", "terrain_utils"):
        spec = importlib.util.spec_from_file_location("isaacgym." + name, os.path.join(base, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["isaacgym." + name] = mod
        spec.loader.exec_module(mod)
        setattr(pkg, name, mod)
    tb = types.ModuleType("torch.utils.tensorboard")
    tb.SummaryWriter = MagicMock()
    sys.modules["torch.utils.tensorboard"] = tb
    # scipy.interpolate.interp2d was removed (scipy >= 1.14): bilinear shim with the same call shape
    from scipy import interpolate

    class interp2d:  # noqa: N801
        def __init__(self, x, y, z, kind="linear"):
            self.f = interpolate.RegularGridInterpolator((np.asarray(y), np.asarray(x)), np.asarray(z, dtype=float))

        def __call__(self, xn, yn):
            yy, xx = np.meshgrid(yn, xn, indexing="ij")
            return self.f(np.stack([yy, xx], -1))
    interpolate.interp2d = interp2d
    sys.path.insert(0, os.path.join(REF, "legged_gym"))
    sys.path.insert(0, os.path.join(REF, "rsl_rl"))
    import legged_gym.envs  # noqa: F401  -- must precede legged_gym.utils (circular import, task_registry.py:42)


def build_full_body_cfg():
    """The BUILD's 32-DOF task configuration (wiki-grx-gym_amd/envs/config.py GR1T1FullBodyCfg: the reference ships no runnable full-body
    task) laid over the REFERENCE's own full-body config object (gr1t1_config.py GR1T1Cfg): every value the reference's
    post_physics_step reads -- reward scales and sigmas, thresholds, observation scales, noise, commands, default joint angles -- is the
    build's; every formula, index set and column layout that consumes it is the reference's."""
    from legged_gym.envs.gr1t1.gr1t1_config import GR1T1Cfg
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if repo not in sys.path:
        sys.path.insert(0, repo)
    from wiki_grx_gym_amd.envs.config import GR1T1FullBodyCfg as B
    cfg = GR1T1Cfg()

    def values(sec):
        return {k: getattr(sec, k) for k in dir(sec) if not k.startswith("_") and not isinstance(getattr(sec, k), type) and not callable(getattr(sec, k))}
    for name in ("env", "rewards", "normalization", "noise", "commands", "init_state", "control", "terrain", "domain_rand"):
        ref_sec, my_sec = getattr(cfg, name), getattr(B, name)
        for k, v in values(my_sec).items():
            setattr(ref_sec, k, v)
        for sub in [k for k in dir(my_sec) if not k.startswith("_") and isinstance(getattr(my_sec, k), type)]:
            ref_sub = getattr(ref_sec, sub)
            if sub == "scales" and name == "rewards":   # a scale the build does not list is off
                for k in values(ref_sub):
                    setattr(ref_sub, k, 0.0)
            for k, v in values(getattr(my_sec, sub)).items():
                setattr(ref_sub, k, v)
    cfg.asset.terminate_after_contacts_on = list(B.asset.terminate_after_contacts_on)
    cfg.asset.penalize_contacts_on = list(B.asset.penalize_contacts_on)
    return cfg


ROBOTS = {   # model table, reference class, reference config, dofs
    "gr1t1_lower_limb": ("gr1t1_lower_limb", "GR1T1", "legged_gym.envs.gr1t1.gr1t1_lower_limb_config:GR1T1LowerLimbCfg", 10),
    "gr1t2_lower_limb": ("gr1t2_lower_limb", "GR1T2", "legged_gym.envs.gr1t2.gr1t2_lower_limb_config:GR1T2LowerLimbCfg", 10),
    "gr1t1": ("gr1t1", "GR1T1", None, 32),
}


def make_ref_env(N, seed, terrain_obj=None, robot="gr1t1_lower_limb"):
    """A reference GR1T1 / GR1T2 instance without Isaac Gym: attributes set by hand on a bare object.  robot = "gr1t1": the reference's
    GR1T1 class -- it is DOF-count agnostic (gr1t1.py:281-313 emits 3 + 3 + 3 + 3 nd columns, the reward sums run over num_dof) -- on the
    32-DOF full body: body / dof names of GR1T1.urdf, the index sets of gr1t1.py:18-113 / 137-279 drawn from them by the reference's own code."""
    import legged_gym.envs as E  # noqa: F401  (must be imported before legged_gym.utils)
    import legged_gym.envs as envs_mod
    from isaacgym.torch_utils import quat_rotate_inverse
    model_key, cls_name, cfg_path, nd = ROBOTS[robot]
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed)
    if cfg_path is None:
        cfg = build_full_body_cfg()
    else:
        mod, cname = cfg_path.split(":")
        cfg = getattr(importlib.import_module(mod), cname)()
    nobs, npri = 9 + 3 * nd, 9 + 3 * nd + 3 + 1 + 2 + 2 + 121
    assert (cfg.env.num_obs, cfg.env.num_pri_obs, cfg.env.num_actions) == (nobs, npri, nd), (cfg.env.num_obs, cfg.env.num_pri_obs, cfg.env.num_actions)
    env = object.__new__(getattr(envs_mod, cls_name))
    env.cfg = cfg
    env.device = "cpu"
    env.num_envs, env.num_obs, env.num_pri_obs, env.num_actions = N, nobs, npri, nd
    env.num_dof = env.num_dofs = nd
    env.gym = MagicMock()
    env.sim = MagicMock()
    env.viewer = None
    env.sim_params = types.SimpleNamespace(dt=cfg.sim.dt)
    env.headless = True
    env.init_done = True
    env.up_axis_idx = 2
    env.height_samples = None
    env.debug_viz = False
    env._parse_cfg()
    names = json.load(open(os.path.join(os.path.dirname(OUT), "..", "wiki-grx-gym_amd", "assets", model_key + ".model.json")))
    nb = len(names["body_names"])
    body_names, dof_names = names["body_names"], names["dof_names"]
    env.dof_names = dof_names
    idx = lambda sub: torch.tensor([i for i, n in enumerate(body_names) if sub in n], dtype=torch.long)
    env.feet_indices = idx("foot_roll")
    env.torso_indices = idx("torso")
    env.forehead_indices = idx("head_pitch")
    term = []
    for n in cfg.asset.terminate_after_contacts_on:
        term.extend([i for i, b in enumerate(body_names) if n in b])
    env.termination_contact_indices = torch.tensor(term, dtype=torch.long)
    env.penalised_contact_indices = torch.zeros(0, dtype=torch.long)
    # buffers (BaseTask.__init__ / _init_buffers)
    env.obs_buf = torch.zeros(N, nobs)
    env.pri_obs_buf = torch.zeros(N, npri)
    env.rew_buf = torch.zeros(N)
    env.reset_buf = torch.ones(N, dtype=torch.long)
    env.episode_length_buf = torch.zeros(N, dtype=torch.long)
    env.time_out_buf = torch.zeros(N, dtype=torch.bool)
    env.extras = {}
    env.common_step_counter = 0
    env.root_states = torch.zeros(N, 13)
    env.root_states[:, 6] = 1
    env.dof_state = torch.zeros(N * nd, 2)
    env.dof_pos = env.dof_state.view(N, nd, 2)[..., 0]
    env.dof_vel = env.dof_state.view(N, nd, 2)[..., 1]
    env.dof_acc = torch.zeros(N, nd)
    env.dof_pos_offset = torch.zeros(N, nd)
    env.base_pos = env.root_states[:, 0:3]
    env.base_quat = env.root_states[:, 3:7]
    env.contact_forces = torch.zeros(N, nb, 3)
    env.rigid_body_states = torch.zeros(N, nb, 13)
    env.rigid_body_states[:, :, 6] = 1
    env.gravity_vec = torch.tensor([0., 0., -1.]).repeat(N, 1)
    env.forward_vec = torch.tensor([1., 0., 0.]).repeat(N, 1)
    env.torques = torch.zeros(N, nd)
    env.p_gains = torch.zeros(nd)
    env.d_gains = torch.zeros(nd)
    env.default_dof_pos = torch.zeros(nd)
    for i, name in enumerate(dof_names):
        env.default_dof_pos[i] = cfg.init_state.default_joint_angles[name]
        for k in cfg.control.stiffness:
            if k in name:
                env.p_gains[i] = cfg.control.stiffness[k]
                env.d_gains[i] = cfg.control.damping[k]
    env.default_dof_pos = env.default_dof_pos.unsqueeze(0)
    env.default_dof_pos_tenors = torch.ones(N, nd) * env.default_dof_pos
    env.last_dof_vel = torch.zeros(N, nd)
    env.actions = torch.zeros(N, nd)
    env.last_actions = torch.zeros(N, nd)
    env.last_last_actions = torch.zeros(N, nd)
    env.commands = torch.zeros(N, 3)
    env.commands_heading = torch.zeros(N)
    env.commands_scale = torch.ones(N, 3)
    env.base_lin_vel = torch.zeros(N, 3)
    env.base_ang_vel = torch.zeros(N, 3)
    env.base_projected_gravity = torch.zeros(N, 3)
    env.base_heights_offset = torch.zeros(N)
    env.surround_heights_offset = torch.zeros(N, 121)
    for nm in ("feet_air_time", "last_feet_air_time", "feet_land_time", "last_feet_land_time", "avg_feet_contact_force", "feet_height"):
        setattr(env, nm, torch.zeros(N, 2))
    env.avg_feet_speed_xyz = torch.zeros(N, 2, 3)
    env.avg_feet_speed_rpy = torch.zeros(N, 2, 3)
    for nm in ("feet_contact", "feet_contact_last", "feet_contact_filt"):
        setattr(env, nm, torch.zeros(N, 2, dtype=torch.bool))
    env.motor_strength_scales = torch.ones(N, nd)
    # URDF limits (legged_robot.py:582-616)
    links = {l["joint_name"]: l for l in names["links"] if l["joint_name"]}
    env.dof_pos_limits = torch.zeros(nd, 2)
    env.dof_vel_limits = torch.zeros(nd)
    env.torque_limits = torch.zeros(nd)
    for i, dn in enumerate(dof_names):
        lim = links[dn]["limit"]
        env.dof_pos_limits[i, 0], env.dof_pos_limits[i, 1] = lim["lower"], lim["upper"]
        env.dof_vel_limits[i], env.torque_limits[i] = lim["velocity"], lim["effort"]
        m = (env.dof_pos_limits[i, 0] + env.dof_pos_limits[i, 1]) / 2
        r = env.dof_pos_limits[i, 1] - env.dof_pos_limits[i, 0]
        env.dof_pos_limits[i, 0] = m - 0.5 * r * cfg.rewards.soft_dof_pos_limit
        env.dof_pos_limits[i, 1] = m + 0.5 * r * cfg.rewards.soft_dof_pos_limit
    env.swing_feet_height_target = torch.ones(N, 1) * cfg.rewards.swing_feet_height_target
    env._init_buffers_joint_indices()
    env.height_points = env._init_height_points()
    env.measured_heights = 0
    env.noise_scale_vec = env.compute_noise_scale_vec()
    env._prepare_reward_function()
    env.env_origins = torch.zeros(N, 3)
    env.custom_origins = False
    env.base_init_state = torch.tensor(cfg.init_state.pos + cfg.init_state.rot + cfg.init_state.lin_vel + cfg.init_state.ang_vel)
    if terrain_obj is not None:
        env.cfg.terrain.mesh_type = "heightfield"
        env.terrain = terrain_obj
        env.height_samples = torch.tensor(terrain_obj.heightsamples).view(terrain_obj.tot_rows, terrain_obj.tot_cols)
    return env, g, body_names


def rand_quat(n, g, tilt=0.6):
    e = (torch.rand(n, 3, generator=g) * 2 - 1) * torch.tensor([tilt, tilt, 3.14])
    from isaacgym.torch_utils import quat_from_euler_xyz
    return quat_from_euler_xyz(e[:, 0], e[:, 1], e[:, 2])


def gen_quat(out):
    from isaacgym.torch_utils import quat_rotate_inverse, quat_apply, quat_from_euler_xyz, quat_rotate
    from legged_gym.utils.math import quat_apply_yaw, wrap_to_pi
    g = torch.Generator().manual_seed(11)
    q = rand_quat(256, g, tilt=3.0)
    v = torch.randn(256, 3, generator=g)
    e = (torch.rand(256, 3, generator=g) * 2 - 1) * 6.28
    ang = (torch.rand(256, generator=g) * 2 - 1) * 20
    np.savez(os.path.join(out, "quat.npz"), q=q.numpy(), v=v.numpy(), rotate_inverse=quat_rotate_inverse(q, v).numpy(),
             rotate=quat_rotate(q, v).numpy(), apply=quat_apply(q, v).numpy(), apply_yaw=quat_apply_yaw(q.clone(), v.clone()).numpy(),
             euler=e.numpy(), from_euler=quat_from_euler_xyz(e[:, 0], e[:, 1], e[:, 2]).numpy(),
             ang=ang.numpy(), wrap_to_pi=wrap_to_pi(ang.clone()).numpy())


def gen_torques(out):
    env, g, _ = make_ref_env(64, 3)
    env.dof_pos[:] = env.default_dof_pos + (torch.rand(64, 10, generator=g) - 0.5)
    env.dof_vel[:] = (torch.rand(64, 10, generator=g) - 0.5) * 20
    env.motor_strength_scales = 0.9 + 0.2 * torch.rand(64, 10, generator=g)
    a = (torch.rand(64, 10, generator=g) - 0.5) * 6
    clipped = env.clip_actions(a)
    tq = env._compute_torques(clipped)
    np.savez(os.path.join(out, "torques.npz"), dof_pos=env.dof_pos.numpy().copy(), dof_vel=env.dof_vel.numpy().copy(),
             strength=env.motor_strength_scales.numpy(), actions=a.numpy(), clipped=clipped.numpy(), torques=tq.numpy(),
             p_gains=env.p_gains.numpy(), d_gains=env.d_gains.numpy(), default_dof_pos=env.default_dof_pos.numpy(),
             torque_limits=env.torque_limits.numpy(), dof_pos_limits=env.dof_pos_limits.numpy(),
             dof_vel_limits=env.dof_vel_limits.numpy(), noise_vec=env.noise_scale_vec.numpy(),
             reward_names=np.array(env.reward_names), reward_scales=np.array([env.reward_scales[n] for n in env.reward_names]),
             clip_min=np.asarray(env.cfg.normalization.clip_actions_min), clip_max=np.asarray(env.cfg.normalization.clip_actions_max))


def gen_control_modes(out):
    """The reference options the GRx tasks leave off (missing #4): _compute_torques with control_type 'V' and 'T'
    (legged_robot.py:699-704) on the G-2 inputs plus a last_dof_vel, and the heading command (legged_robot.py:320-326) through one
    post_physics_step() with cfg.commands.heading_command = True (num_commands = 4, as that mode needs)."""
    env, g, body_names = make_ref_env(64, 13)
    env.dof_pos[:] = env.default_dof_pos + (torch.rand(64, 10, generator=g) - 0.5)
    env.dof_vel[:] = (torch.rand(64, 10, generator=g) - 0.5) * 0.8
    env.last_dof_vel = env.dof_vel + (torch.rand(64, 10, generator=g) - 0.5) * 0.03   # (a velocity difference through d_gains / sim_dt: small, or every row saturates)
    env.motor_strength_scales = 0.9 + 0.2 * torch.rand(64, 10, generator=g)
    a = (torch.rand(64, 10, generator=g) - 0.5) * 1.2
    a[::7] *= 5                                            # some rows beyond the action clip
    clipped = env.clip_actions(a)
    data = dict(dof_pos=env.dof_pos.numpy().copy(), dof_vel=env.dof_vel.numpy().copy(), last_dof_vel=env.last_dof_vel.numpy().copy(),
                strength=env.motor_strength_scales.numpy(), actions=a.numpy(), clipped=clipped.numpy(), torque_limits=env.torque_limits.numpy())
    for ct in ("P", "V", "T"):
        env.cfg.control.control_type = ct
        data["torques_" + ct] = env._compute_torques(clipped.clone()).numpy().copy()
    env.cfg.control.control_type = "P"
    # heading command
    N = 64
    env, g, body_names = make_ref_env(N, 17)
    env.cfg.domain_rand.push_robots = False
    randomize_state(env, g, body_names, N, 0)
    env.cfg.commands.heading_command = True
    env.cfg.commands.num_commands = 4
    env.commands = torch.cat([env.commands, torch.zeros(N, 1)], 1)
    inp = snapshot_inputs(env)
    env.reset_idx = lambda ids: None
    noise_u = torch.rand(N, 39, generator=g)
    orig_rand_like = torch.rand_like
    torch.rand_like = lambda t, _u=noise_u: _u.clone()
    try:
        env.post_physics_step()
    finally:
        torch.rand_like = orig_rand_like
    for k, v in inp.items():
        data["h_in_" + k] = v
    data["h_in_commands"] = inp["commands"][:, :3] if inp["commands"].shape[1] > 3 else inp["commands"]
    data["h_out_commands"] = env.commands.numpy().copy()
    data["h_out_obs"] = torch.clip(env.obs_buf, -100, 100).numpy().copy()
    data["h_noise_u"] = noise_u.numpy()
    data["h_yaw_range"] = np.asarray(env.command_ranges["ang_vel_yaw"], dtype=np.float32)
    np.savez(os.path.join(out, "control_modes.npz"), **data)


def randomize_state(env, g, body_names, N, step):
    """Synthetic post-physics state incl. edge rows (thresholds, timers at zero, near limits)."""
    feet = env.feet_indices
    torso = int(env.torso_indices[0])
    nd = env.num_dof
    env.root_states[:, 0:2] = (torch.rand(N, 2, generator=g) - 0.5) * 4
    env.root_states[:, 2] = 0.6 + 0.5 * torch.rand(N, generator=g)
    env.root_states[:, 3:7] = rand_quat(N, g, tilt=0.5)
    env.root_states[:, 7:13] = torch.randn(N, 6, generator=g)
    env.dof_pos[:] = env.default_dof_pos + (torch.rand(N, nd, generator=g) - 0.5) * 1.5
    env.dof_vel[:] = torch.randn(N, nd, generator=g) * 8
    env.dof_vel[::7] *= 4                                   # some rows beyond the soft velocity limit
    env.torques = torch.randn(N, nd, generator=g) * 40
    env.torques[::5] *= 3                                   # some rows beyond the soft torque limit
    env.actions = env.clip_actions(torch.randn(N, nd, generator=g))
    env.commands[:] = (torch.rand(N, 3, generator=g) * 2 - 1) * torch.tensor([1.0, 0.5, 1.0])
    env.commands[::4, :2] = 0.0                             # standing commands
    env.contact_forces[:] = 0
    fz = torch.rand(N, 2, generator=g) * 400 * (torch.rand(N, 2, generator=g) > 0.4)
    env.contact_forces[:, feet, 2] = fz
    env.contact_forces[:, feet, 0:2] = torch.randn(N, 2, 2, generator=g) * 30 * (fz > 0).unsqueeze(-1)
    env.contact_forces[3, feet[0], 2] = 1.0                 # exactly at the contact threshold (not > 1)
    env.contact_forces[4, feet[1], 2] = 1.0 + 1e-3
    env.rigid_body_states[:, :, 0:3] = env.root_states[:, None, 0:3]
    env.rigid_body_states[:, feet, 2] = torch.rand(N, 2, generator=g) * 0.25
    env.rigid_body_states[:, feet, 7:10] = torch.randn(N, 2, 3, generator=g)
    env.rigid_body_states[:, torso, 3:7] = env.root_states[:, 3:7]
    env.avg_feet_contact_force = torch.rand(N, 2, generator=g) * 300
    env.avg_feet_speed_xyz = torch.rand(N, 2, 3, generator=g) * 2
    if step == 0:
        env.feet_air_time = torch.rand(N, 2, generator=g) * 0.8 * (torch.rand(N, 2, generator=g) > 0.3)
        env.feet_land_time = torch.rand(N, 2, generator=g) * 2.0
        env.feet_contact_last = torch.rand(N, 2, generator=g) > 0.5
        env.episode_length_buf[:] = torch.randint(0, 990, (N,), generator=g)
        env.episode_length_buf[5] = 499                     # resample-by-time row
        env.episode_length_buf[6] = 999                     # becomes 1000: not yet a time-out
        env.episode_length_buf[7] = 1000                    # becomes 1001: time-out
        env.last_actions = torch.randn(N, nd, generator=g) * 0.5
        env.last_last_actions = torch.randn(N, nd, generator=g) * 0.5
        env.last_dof_vel = torch.randn(N, nd, generator=g) * 8
        env.base_heights_offset = (torch.rand(N, generator=g) - 0.5) * 2   # stale value used by the reward (Q4)
    # termination rows
    tilt = rand_quat(N, g, tilt=0.0)
    env.root_states[8, 3:7] = torch.tensor([0.0, 0.62, 0.0, 0.7846])   # |g_z| just below 0.33 -> reset
    env.root_states[9, 3:7] = torch.tensor([0.0, 0.575, 0.0, 0.8182])  # |g_z| just above 0.33
    env.contact_forces[10, torso, 2] = 5.0                             # terminating body contact


def snapshot_inputs(env):
    feet = env.feet_indices
    torso = int(env.torso_indices[0])
    return dict(root=env.root_states.numpy().copy(), dof_pos=env.dof_pos.numpy().copy(), dof_vel=env.dof_vel.numpy().copy(),
                torques=env.torques.numpy().copy(), actions=env.actions.numpy().copy(), commands=env.commands.numpy().copy(),
                feet_force=env.contact_forces[:, feet].numpy().copy(), feet_pos=env.rigid_body_states[:, feet, 0:3].numpy().copy(),
                torso_quat=env.rigid_body_states[:, torso, 3:7].numpy().copy(),
                term_contact=(torch.norm(env.contact_forces[:, env.termination_contact_indices], dim=-1) > 1.0).any(1).numpy().copy(),
                avg_force=env.avg_feet_contact_force.numpy().copy(), avg_speed=env.avg_feet_speed_xyz.numpy().copy(),
                air_time=env.feet_air_time.numpy().copy(), land_time=env.feet_land_time.numpy().copy(),
                contact_last=env.feet_contact_last.numpy().copy(), episode_length=env.episode_length_buf.numpy().copy(),
                last_actions=env.last_actions.numpy().copy(), last_last_actions=env.last_last_actions.numpy().copy(),
                last_dof_vel=env.last_dof_vel.numpy().copy(), base_heights_offset=env.base_heights_offset.numpy().copy())


def gen_pipeline(out):
    """Two consecutive reference post_physics_step() calls on synthetic state, resets disabled
    (reset_idx is replaced by a recorder: its RNG stream cannot be reproduced)."""
    N = 64
    env, g, body_names = make_ref_env(N, 5)
    env.cfg.domain_rand.push_robots = False
    noise_u = torch.rand(2, N, 39, generator=g)
    data = {}
    for step in range(2):
        randomize_state(env, g, body_names, N, step)
        inp = snapshot_inputs(env)
        env.reset_idx = lambda ids: None          # keep rows un-reset; reset_buf/time_out still recorded
        # the time-based command resample draws from torch's RNG: record commands after the step instead
        orig_rand_like = torch.rand_like
        torch.rand_like = lambda t, _u=noise_u[step]: _u.clone()   # inject the observation-noise uniforms
        try:
            env.post_physics_step()
        finally:
            torch.rand_like = orig_rand_like
        obs = torch.clip(env.obs_buf, -100, 100)
        pri = torch.clip(env.pri_obs_buf, -100, 100)
        terms = {}
        for name, fn in zip(env.reward_names, env.reward_functions):
            terms[name] = None
        outd = dict(obs=obs.numpy().copy(), pri_obs=pri.numpy().copy(), rew=env.rew_buf.numpy().copy(),
                    reset=env.reset_buf.numpy().copy(), time_out=env.time_out_buf.numpy().copy(),
                    base_lin_vel=env.base_lin_vel.numpy().copy(), base_ang_vel=env.base_ang_vel.numpy().copy(),
                    projected_gravity=env.base_projected_gravity.numpy().copy(), commands_after=env.commands.numpy().copy(),
                    feet_contact=env.feet_contact.numpy().copy(), air_time_after=env.feet_air_time.numpy().copy(),
                    land_time_after=env.feet_land_time.numpy().copy(), feet_height=env.feet_height.numpy().copy(),
                    first_contact=env.feet_first_contact.numpy().copy(), base_heights_offset_after=env.base_heights_offset.numpy().copy(),
                    episode_sums=np.stack([env.episode_sums[n].numpy().copy() for n in env.reward_names]),
                    episode_length_after=env.episode_length_buf.numpy().copy(),
                    last_actions_after=env.last_actions.numpy().copy(), last_last_actions_after=env.last_last_actions.numpy().copy())
        for k, v in inp.items():
            data[f"s{step}_in_{k}"] = v
        for k, v in outd.items():
            data[f"s{step}_out_{k}"] = v
        data[f"s{step}_noise_u"] = noise_u[step].numpy()
    # per-term unscaled rewards of the second state (recomputed; read-only functions)
    data["reward_names"] = np.array(env.reward_names)
    data["reward_scales_dt"] = np.array([env.reward_scales[n] for n in env.reward_names])
    np.savez(os.path.join(out, "pipeline.npz"), **data)


def scan_edge_margin(env, tcfg, i):
    """Distance (in cells, fp64) of env i's nearest height-scan point to a cell edge of the raster."""
    from legged_gym.utils.math import quat_apply_yaw
    pts = quat_apply_yaw(env.base_quat[i:i + 1].repeat(1, 121), env.height_points[i:i + 1]).double() + env.root_states[i:i + 1, :3].double().unsqueeze(1)
    f = (pts[0, :, :2] + tcfg.border_size) / tcfg.horizontal_scale
    return float((f - torch.round(f)).abs().min())


def stand_on_terrain(env, g, tcfg, ter, N):
    """Heights under the base: put the base and the feet at plausible heights ABOVE the local terrain."""
    hs = torch.tensor(ter.heightsamples.astype(np.int64))
    feet = env.feet_indices
    torso = int(env.torso_indices[0])
    px = ((env.root_states[:, 0] + tcfg.border_size) / tcfg.horizontal_scale).long().clip(0, hs.shape[0] - 2)
    py = ((env.root_states[:, 1] + tcfg.border_size) / tcfg.horizontal_scale).long().clip(0, hs.shape[1] - 2)
    ground = hs[px, py].float() * tcfg.vertical_scale
    env.root_states[:, 2] = ground + 0.6 + 0.5 * torch.rand(N, generator=g)
    env.root_states[11, 2] = ground[11] + 2.5        # clip(z - target - h_k, -1, 1) saturates at +1 -> +25 in pri_obs (Q5) ...
    env.root_states[12, 2] = ground[12] - 0.5        # ... and at -1 -> -25
    env.rigid_body_states[:, :, 0:3] = env.root_states[:, None, 0:3]
    env.rigid_body_states[:, feet, 2] = ground[:, None] + torch.rand(N, 2, generator=g) * 0.25
    env.rigid_body_states[:, torso, 3:7] = env.root_states[:, 3:7]


def rough_poses(env, g, tcfg, ter, N):
    """Poses of gen_pipeline_rough over the reference raster: every scan point at least 5e-4 cells from a cell edge (fp64), base and feet
    above the local terrain.  Returns the number of redraws."""
    redraws = 0
    for i in range(N):
        while True:
            # over the tiles (10 rows x 8 m, 20 columns x 8 m), yaw anywhere, modest tilt; rows 0 / 1 keep randomize_state's poses near
            # the map corner: the border flat and the first tile
            if i >= 2:
                env.root_states[i, 0] = torch.rand((), generator=g) * 78 + 1
                env.root_states[i, 1] = torch.rand((), generator=g) * 158 + 1
            env.root_states[i, 3:7] = rand_quat(1, g, tilt=0.4)[0] if i not in (8, 9) else env.root_states[i, 3:7]
            if scan_edge_margin(env, tcfg, i) >= 5e-4:
                break
            if i < 2:
                env.root_states[i, 0:2] += 0.013
            redraws += 1
    stand_on_terrain(env, g, tcfg, ter, N)
    return redraws


def gen_pipeline_rough(out):
    """One reference post_physics_step() ON THE ROUGH-TERRAIN RASTER: the raster of terrain.npz (seed 1,
    10 x 20 curriculum tiles), the reference's own _get_heights (legged_robot.py:1235-1274) inside the step, so that the 121-entry
    height block of pri_obs with NON-UNIFORM heights, feet_height = mean(z_foot - h_k) (legged_robot_fftai.py:118-124), the x25
    scaling (gr1t1.py:281-313, Q5) and base_heights_offset come from the reference on a real raster.  A scan point within fp32
    rounding of a cell edge may legitimately read the neighbouring cell; poses are redrawn until every point of the env sits at
    least 5e-4 cells (5e-5 m) from an edge in fp64, so the fixture compares without an allowance."""
    from legged_gym.utils.terrain import Terrain
    from legged_gym.envs.base.legged_robot_config import LeggedRobotCfg
    tcfg = LeggedRobotCfg.terrain()
    tcfg.mesh_type = "heightfield"
    np.random.seed(1)
    ter = Terrain(tcfg, 64)          # the raster of terrain.npz (same seed, same call): the tests load it from there
    N = 64
    env, g, body_names = make_ref_env(N, 31, terrain_obj=ter)
    env.cfg.domain_rand.push_robots = False
    assert env.cfg.terrain.measure_heights
    noise_u = torch.rand(N, 39, generator=g)
    randomize_state(env, g, body_names, N, 0)
    redraws = rough_poses(env, g, tcfg, ter, N)
    inp = snapshot_inputs(env)
    env.reset_idx = lambda ids: None
    orig_rand_like = torch.rand_like
    torch.rand_like = lambda t, _u=noise_u: _u.clone()
    try:
        env.post_physics_step()
    finally:
        torch.rand_like = orig_rand_like
    mh = env.measured_heights.numpy().copy()
    assert mh.std(axis=1).max() > 0.05 and (mh.std(axis=1) > 1e-3).sum() > N // 2, "the scans must see non-uniform terrain"
    outd = dict(obs=torch.clip(env.obs_buf, -100, 100).numpy().copy(), pri_obs=torch.clip(env.pri_obs_buf, -100, 100).numpy().copy(),
                rew=env.rew_buf.numpy().copy(), reset=env.reset_buf.numpy().copy(), time_out=env.time_out_buf.numpy().copy(),
                measured_heights=mh, feet_height=env.feet_height.numpy().copy(), feet_contact=env.feet_contact.numpy().copy(),
                base_heights_offset_after=env.base_heights_offset.numpy().copy(), commands_after=env.commands.numpy().copy(),
                episode_sums=np.stack([env.episode_sums[n].numpy().copy() for n in env.reward_names]))
    data = {"in_" + k: v for k, v in inp.items()}
    data.update({"out_" + k: v for k, v in outd.items()})
    data["noise_u"] = noise_u.numpy()
    data["reward_names"] = np.array(env.reward_names)
    data["redraws"] = redraws
    np.savez_compressed(os.path.join(out, "pipeline_rough.npz"), **data)


def full_body_link_orientations(env):
    """The 32-DOF body's torso and forehead orientations in rigid_body_states: the forward kinematics of (root, dof_pos) in fp64 from the
    model table (tests/kinematics_ref.py), as PhysX would report them."""
    from wiki_grx_gym_amd.model import RobotModel
    from tests.kinematics_ref import BodyKinematics
    rm = RobotModel("gr1t1")
    kin = BodyKinematics(rm, "cpu")
    for attr in ("axis", "rot0", "jpos", "link_rot", "link_pos"):
        setattr(kin, attr, getattr(kin, attr).double())
    rbs = kin.rigid_body_states(env.root_states.double(), env.dof_pos.double(), env.dof_vel.double())
    torso = int(env.torso_indices[0])
    env.rigid_body_states[:, torso, 3:7] = rbs[:, torso, 3:7].float()
    for fi in env.forehead_indices:
        env.rigid_body_states[:, int(fi), 3:7] = rbs[:, int(fi), 3:7].float()


def gen_pipeline_other_robots(out):
    """One reference post_physics_step() for the robots the round 1-5 fixtures did not cover (VERDICT r5 #4b):
      pipeline_gr1t2.npz      the reference's GR1T2 class with GR1T2LowerLimbCfg and the body names of GR1T2_lower_limb.urdf: its 20-body
                              termination set (terminate_after_contacts_on, 'imu' matches imu_link) decides the injected contact rows;
      pipeline_full_body.npz  the reference's GR1T1 class on the 32-DOF GR1T1.urdf (build_full_body_cfg): obs 105 / pri_obs 234 columns,
                              32-joint reward sums, the joint index sets the reference draws from the full-body dof names (gr1t1.py:137-279:
                              hip_roll, hip_yaw, knee, ankle ...).  The torso link's orientation in rigid_body_states is the forward
                              kinematics of (root, dof_pos) -- in the full body the torso hangs from the three waist joints -- computed in
                              fp64 from the model table (tests/kinematics_ref.py), as PhysX would report it.
    Same record layout as pipeline_rough.npz (in_* / out_*), resets recorded but not applied."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if repo not in sys.path:
        sys.path.insert(0, repo)
    for robot, fname, seed in (("gr1t2_lower_limb", "pipeline_gr1t2.npz", 41), ("gr1t1", "pipeline_full_body.npz", 43)):
        N = 64
        env, g, body_names = make_ref_env(N, seed, robot=robot)
        nd = env.num_dof
        env.cfg.domain_rand.push_robots = False
        noise_u = torch.rand(N, env.num_obs, generator=g)
        randomize_state(env, g, body_names, N, 0)
        # contact rows over the robot's own termination set: a force above the threshold on a DIFFERENT terminating body per row, and one on
        # a body outside the set (no reset); GR1T2: imu_link is one of them
        term = [int(i) for i in env.termination_contact_indices]
        non_term = [i for i in range(len(body_names)) if i not in term and i not in [int(f) for f in env.feet_indices]]
        env.contact_forces[10] = 0
        for r, bidx in enumerate(term[:8]):
            env.contact_forces[16 + r, bidx, r % 3] = 2.0 + r
        if non_term:
            env.contact_forces[24, non_term[0], 2] = 50.0
        if robot == "gr1t2_lower_limb":
            imu = body_names.index("imu_link")
            assert imu in term, "GR1T2: 'imu' of terminate_after_contacts_on matches imu_link"
            env.contact_forces[25, imu, 0] = 3.0
        if robot == "gr1t1":
            full_body_link_orientations(env)
        inp = snapshot_inputs(env)
        env.reset_idx = lambda ids: None
        seen = {}   # every active term on its own (unscaled) AS compute_reward evaluates it inside the step (legged_robot.py:355-375)

        def recorder(name, fn):
            def wrapped():
                v = fn()
                seen[name] = v.float().numpy().copy()
                return v
            return wrapped
        env.reward_functions = [recorder(n, f) for n, f in zip(env.reward_names, env.reward_functions)]
        orig_rand_like = torch.rand_like
        torch.rand_like = lambda t, _u=noise_u: _u.clone()
        try:
            env.post_physics_step()
        finally:
            torch.rand_like = orig_rand_like
        outd = dict(obs=torch.clip(env.obs_buf, -100, 100).numpy().copy(), pri_obs=torch.clip(env.pri_obs_buf, -100, 100).numpy().copy(),
                    rew=env.rew_buf.numpy().copy(), reset=env.reset_buf.numpy().copy(), time_out=env.time_out_buf.numpy().copy(),
                    base_lin_vel=env.base_lin_vel.numpy().copy(), base_ang_vel=env.base_ang_vel.numpy().copy(),
                    projected_gravity=env.base_projected_gravity.numpy().copy(), commands_after=env.commands.numpy().copy(),
                    feet_contact=env.feet_contact.numpy().copy(), air_time_after=env.feet_air_time.numpy().copy(),
                    land_time_after=env.feet_land_time.numpy().copy(), feet_height=env.feet_height.numpy().copy(),
                    base_heights_offset_after=env.base_heights_offset.numpy().copy(),
                    episode_sums=np.stack([env.episode_sums[n].numpy().copy() for n in env.reward_names]),
                    episode_length_after=env.episode_length_buf.numpy().copy(), last_actions_after=env.last_actions.numpy().copy())
        outd["term_values"] = np.stack([seen[n] for n in env.reward_names])
        data = {"in_" + k: v for k, v in inp.items()}
        data.update({"out_" + k: v for k, v in outd.items()})
        data["noise_u"] = noise_u.numpy()
        data["reward_names"] = np.array(env.reward_names)
        data["reward_scales_dt"] = np.array([env.reward_scales[n] for n in env.reward_names])
        data["termination_bodies"] = np.array([body_names[i] for i in term])
        data["index_sets"] = np.array(json.dumps({k: [int(i) for i in getattr(env, k)] for k in sorted(dir(env))
                                                  if k.endswith("_indices") and ((torch.is_tensor(getattr(env, k)) and getattr(env, k).dim() == 1) or isinstance(getattr(env, k), list))}))
        assert int(outd["reset"].sum()) >= 9 and not outd["reset"][24], "the contact rows: terminating bodies reset, the other body does not"
        np.savez_compressed(os.path.join(out, fname), **data)


def gen_reward_terms(out):
    """Every implemented FF/G1 reward term (active or not) evaluated by the reference on one state."""
    N = 64
    env, g, body_names = make_ref_env(N, 9)
    randomize_state(env, g, body_names, N, 0)
    inp = snapshot_inputs(env)   # BEFORE the timers are advanced
    from isaacgym.torch_utils import quat_rotate_inverse
    env.base_lin_vel[:] = quat_rotate_inverse(env.base_quat, env.root_states[:, 7:10])
    env.base_ang_vel[:] = quat_rotate_inverse(env.base_quat, env.root_states[:, 10:13])
    env.base_projected_gravity[:] = quat_rotate_inverse(env.base_quat, env.gravity_vec)
    env.measured_heights = env._get_heights()
    env._calculate_air_time(); env._calculate_feet_height(); env._calculate_land_time()
    env.check_termination()
    names = ["action_diff", "action_diff_diff", "action_diff_knee", "cmd_diff_ang_vel_pitch", "cmd_diff_ang_vel_roll",
             "cmd_diff_ang_vel_yaw", "cmd_diff_base_height", "cmd_diff_base_orient", "cmd_diff_lin_vel_x", "cmd_diff_lin_vel_y",
             "cmd_diff_lin_vel_z", "cmd_diff_torso_orient", "collision", "dof_acc_new", "dof_tor_ankle_feet_lift_up", "dof_tor_new",
             "dof_tor_new_hip_roll", "dof_vel_new", "dof_vel_new_knee", "feet_air_force", "feet_air_height", "feet_air_time",
             "feet_land_time", "feet_speed_xy_close_to_ground", "feet_speed_z_close_to_height_target", "feet_stumble",
             "limits_dof_pos", "limits_dof_tor", "limits_dof_vel", "on_the_air", "pose_offset",
             "pose_offset_hip_yaw", "stand_still", "termination"]
    # (limits_actions is the one FF/G1 term left out: the reference has no sigma_limits_actions -> AttributeError if enabled)
    assert len(names) == 34 and names == sorted(names), len(names)
    vals = {}
    for n in names:
        v = getattr(env, "_reward_" + n)()
        vals[n] = (v.float() if torch.is_tensor(v) else torch.full((N,), float(v))).numpy().copy()
    np.savez(os.path.join(out, "reward_terms.npz"), names=np.array(names), values=np.stack([vals[n] for n in names]),
             **{"in_" + k: v for k, v in inp.items()})


# legged_gym's base reward terms (legged_robot.py:1277-1376) the FFTAI / GR1 classes do not override, with the scales
# base_reward_terms.npz enables next to the registered GR1T1 ones (legged_gym's own defaults where it has one)
BASE_TERM_SCALES = {"action_rate": -0.01, "ang_vel_xy": -0.05, "base_height": -1.0, "dof_acc": -2.5e-7, "dof_pos_limits": -10.0,
                    "dof_vel": -1e-4, "dof_vel_limits": -1.0, "feet_contact_forces": -0.01, "lin_vel_z": -2.0, "orientation": -1.0,
                    "stumble": -0.5, "torque_limits": -0.1, "torques": -1e-5, "tracking_ang_vel": 0.5, "tracking_lin_vel": 1.0}


def gen_base_reward_terms(out):
    """legged_gym's 15 base reward terms and compute_reward's total, from the reference's own post_physics_step with every base term at a
    non-zero scale next to the registered GR1T1 scales: on the plane and on the reference raster (base_height reads this step's scan).
    Rows are set so that every threshold is crossed by some rows and not by others."""
    from legged_gym.utils.terrain import Terrain
    from legged_gym.envs.base.legged_robot_config import LeggedRobotCfg
    from legged_gym.utils.helpers import class_to_dict
    names = sorted(BASE_TERM_SCALES)
    data = {"names": np.array(names), "scales": np.array([BASE_TERM_SCALES[n] for n in names])}
    N = 64
    for case in ("plane", "rough"):
        if case == "rough":
            tcfg = LeggedRobotCfg.terrain()
            tcfg.mesh_type = "heightfield"
            np.random.seed(1)
            ter = Terrain(tcfg, 64)   # the raster of terrain.npz
            env, g, body_names = make_ref_env(N, 43, terrain_obj=ter)
        else:
            env, g, body_names = make_ref_env(N, 41)
        if case == "plane":   # every _reward_* the reference's GR1T1 class resolves (its own and LeggedRobot's)
            data["resolvable"] = np.array(sorted(n[len("_reward_"):] for n in dir(type(env)) if n.startswith("_reward_")))
        for n, v in BASE_TERM_SCALES.items():
            setattr(env.cfg.rewards.scales, n, v)
        env.reward_scales = class_to_dict(env.cfg.rewards.scales)
        env._prepare_reward_function()
        env.cfg.domain_rand.push_robots = False
        noise_u = torch.rand(N, 39, generator=g)
        randomize_state(env, g, body_names, N, 0)
        if case == "rough":
            rough_poses(env, g, tcfg, ter, N)
        feet = env.feet_indices
        # threshold rows: |F| above max_contact_force, stumble on either side of |F_xy| = 5 |F_z|, a foot in the air with a sideways force
        fmax = env.cfg.rewards.max_contact_force
        env.contact_forces[13, feet[0]] = torch.tensor([30.0, 0.0, fmax + 200.0])
        env.contact_forces[14, feet[1]] = torch.tensor([0.0, 0.0, fmax - 50.0])
        env.contact_forces[15, feet[0]] = torch.tensor([60.0, 0.0, 10.0])    # |F_xy| = 6 |F_z|: stumble
        env.contact_forces[16, feet[1]] = torch.tensor([40.0, 0.0, 10.0])    # 4 |F_z|: no stumble
        env.contact_forces[17, feet[0]] = torch.tensor([0.0, 5.0, 0.0])      # F_z = 0: stumble
        env.commands[18, :2] = torch.tensor([0.07, 0.07])                    # |cmd_xy| just below 0.1
        env.commands[19, :2] = torch.tensor([0.08, 0.07])                    # just above
        inp = snapshot_inputs(env)
        vals = {}
        orig_reward = env.compute_reward

        def compute_reward():   # the terms as compute_reward sees them (after the state update, timers and this step's scan)
            for n in names:
                vals[n] = getattr(env, "_reward_" + n)().float().numpy().copy()
            vals["measured_heights"] = (env.measured_heights * torch.ones(N, 1)).numpy().copy() if not torch.is_tensor(env.measured_heights) \
                else env.measured_heights.numpy().copy()
            orig_reward()
        env.compute_reward = compute_reward
        # _reward_orientation (legged_robot.py:1287) reads self.projected_gravity, an attribute this fork renamed to base_projected_gravity
        # (legged_robot.py:165, 311): the reference raises AttributeError with orientation enabled.  The fixture evaluates the term's
        # formula on the renamed buffer (the same tensor, updated in place by the step).
        env.projected_gravity = env.base_projected_gravity
        env.reset_idx = lambda ids: None
        orig_rand_like = torch.rand_like
        torch.rand_like = lambda t, _u=noise_u: _u.clone()
        try:
            env.post_physics_step()
        finally:
            torch.rand_like = orig_rand_like
        v = np.stack([vals[n] for n in names])
        # every threshold is crossed by some rows and not by others
        for n in ("dof_pos_limits", "torque_limits", "feet_contact_forces", "stumble"):
            k = names.index(n)
            assert (v[k] > 0).any() and (v[k] == 0).any(), n
        k = names.index("dof_vel_limits")
        per_joint = (env.dof_vel.abs() - env.dof_vel_limits * env.cfg.rewards.soft_dof_vel_limit)
        assert (v[k] > 0).any() and (v[k] == 0).any() and (per_joint > 1).any() and ((per_joint > 0) & (per_joint < 1)).any()
        assert ((env.commands[:, :2].norm(dim=1) > 0.1) & (env.commands[:, :2].norm(dim=1) < 0.12)).any()
        assert ((env.commands[:, :2].norm(dim=1) < 0.1) & (env.commands[:, :2].norm(dim=1) > 0.08)).any()
        data[case + "_values"] = v
        data[case + "_rew"] = env.rew_buf.numpy().copy()
        data[case + "_measured_heights"] = vals["measured_heights"]
        data[case + "_reward_names"] = np.array(env.reward_names)
        data[case + "_episode_sums"] = np.stack([env.episode_sums[n].numpy().copy() for n in env.reward_names])
        data[case + "_noise_u"] = noise_u.numpy()
        data.update({case + "_in_" + k_: x for k_, x in inp.items()})
    np.savez_compressed(os.path.join(out, "base_reward_terms.npz"), **data)


def gen_command_curriculum(out):
    """The reference's update_command_curriculum (legged_robot.py:828-838) on a sequence of reset sets and tracking_lin_vel episode sums:
    an asymmetric start range, a max_curriculum that is not a multiple of 0.5, means just below and just above the 0.8 threshold, the
    clip at +-max_curriculum.  No RNG in this arithmetic."""
    N = 64
    env, g, _ = make_ref_env(N, 47)
    env.cfg.commands.max_curriculum = 1.7
    env.command_ranges["lin_vel_x"] = [-0.3, 0.7]
    env.reward_scales["tracking_lin_vel"] = 1.0 * env.dt
    env.episode_sums = {"tracking_lin_vel": torch.zeros(N)}
    thr = 0.8 * env.reward_scales["tracking_lin_vel"] * float(env.max_episode_length)   # mean episode sum at the threshold
    # (relative offset of the chosen envs' mean from the threshold, how many envs reset)
    plan = [(+0.30, 3), (-0.001, 5), (+0.001, 4), (-0.40, 1), (+0.25, 7), (+0.50, 2), (+0.001, 6), (+0.20, 3)]
    ids_all, sums_all, ranges = [], [], []
    for rel, k in plan:
        ids = torch.randperm(N, generator=g)[:k].sort().values
        mean = thr * (1.0 + rel)
        spread = (torch.rand(k, generator=g) - 0.5) * 0.2 * thr
        spread -= spread.mean()
        sums = torch.full((N,), 0.5 * thr)
        sums[ids] = (mean + spread).float()
        env.episode_sums["tracking_lin_vel"] = sums
        env.update_command_curriculum(ids)
        ids_all.append(np.isin(np.arange(N), ids.numpy()))
        sums_all.append(sums.numpy().copy())
        ranges.append(np.array(env.command_ranges["lin_vel_x"], dtype=np.float64))
    np.savez(os.path.join(out, "command_curriculum.npz"), reset=np.stack(ids_all), sums=np.stack(sums_all), lin_vel_x=np.stack(ranges),
             start=np.array([-0.3, 0.7]), max_curriculum=1.7, scale_dt=env.reward_scales["tracking_lin_vel"],
             max_episode_length=float(env.max_episode_length), dt=env.dt)


def gen_terrain_and_heights(out):
    from legged_gym.utils.terrain import Terrain
    from legged_gym.envs.base.legged_robot_config import LeggedRobotCfg
    tcfg = LeggedRobotCfg.terrain()
    tcfg.mesh_type = "heightfield"
    np.random.seed(1)
    ter = Terrain(tcfg, 64)
    N = 64
    env, g, _ = make_ref_env(N, 21, terrain_obj=ter)
    env.root_states[:, 0] = torch.rand(N, generator=g) * 90 - 5      # incl. negative coords and beyond-map rows
    env.root_states[:, 1] = torch.rand(N, generator=g) * 170 - 5
    env.root_states[0, 0:2] = torch.tensor([-30.0, -30.0])           # clamps to index 0
    env.root_states[1, 0:2] = torch.tensor([200.0, 300.0])           # clamps to dim-2
    env.root_states[:, 3:7] = rand_quat(N, g, tilt=0.4)
    h = env._get_heights()
    # sparse fingerprint of the raster + the deterministic tiles in full
    hs = ter.heightsamples
    np.savez_compressed(os.path.join(out, "terrain.npz"), heightsamples=hs, env_origins=ter.env_origins,
                        root=env.root_states.numpy().copy(), heights=h.numpy().copy())


def gen_terrain_all_tiles(out):
    """All seven tile families (stepping stones / gap / pit included) + the trimesh conversion, small grid."""
    from legged_gym.utils.terrain import Terrain
    from legged_gym.envs.base.legged_robot_config import LeggedRobotCfg
    tcfg = LeggedRobotCfg.terrain()
    tcfg.mesh_type = "trimesh"
    tcfg.num_rows, tcfg.num_cols, tcfg.border_size = 3, 10, 5
    tcfg.terrain_proportions = [0.1, 0.1, 0.2, 0.2, 0.1, 0.1, 0.1, 0.1]
    np.random.seed(5)
    ter = Terrain(tcfg, 30)
    v, t = ter.vertices, ter.triangles
    np.savez_compressed(os.path.join(out, "terrain_all_tiles.npz"), heightsamples=ter.heightsamples, env_origins=ter.env_origins,
                        vert_sample=v[::997].copy(), tri_sample=t[::997].copy(), vert_sum=v.astype(np.float64).sum(0),
                        tri_sum=t.astype(np.int64).sum(0), n_vert=len(v), n_tri=len(t))
    # (cfg.selected cannot be pinned: the reference's selected_terrain raises AttributeError at terrain.py:103 --
    #  self.vertical_scale / self.horizontal_scale do not exist -- and eval()s the generator name)


def gen_trimesh_tiles(out):
    """The reference's slope-corrected triangle mesh (isaacgym terrain_utils.py:286-350 convert_heightfield_to_trimesh, slope_threshold 0.75:
    legged_robot.py:903-921 passes cfg.terrain.slope_treshold) of two tiles of the curriculum raster of terrain_all_tiles.npz -- one
    pyramid-stairs tile, one discrete-obstacles tile: raster block in, vertices + triangles out.  The build's physics
    keeps the raster and models a corrected (vertical) face as a ramp over the last quarter cell before its HIGH vertex
    (csrc/grx_kernels.hip riser_weight); tests/test_terrain_golden.py ray-casts this mesh against that height function."""
    from legged_gym.utils.terrain import Terrain
    from legged_gym.envs.base.legged_robot_config import LeggedRobotCfg
    from isaacgym.terrain_utils import convert_heightfield_to_trimesh
    tcfg = LeggedRobotCfg.terrain()
    tcfg.mesh_type = "trimesh"
    tcfg.num_rows, tcfg.num_cols, tcfg.border_size = 3, 10, 5
    tcfg.terrain_proportions = [0.1, 0.1, 0.2, 0.2, 0.1, 0.1, 0.1, 0.1]
    np.random.seed(5)
    ter = Terrain(tcfg, 30)          # the raster of terrain_all_tiles.npz
    b, px = ter.border, ter.length_per_env_pixels
    data = {"horizontal_scale": tcfg.horizontal_scale, "vertical_scale": tcfg.vertical_scale, "slope_threshold": tcfg.slope_treshold}
    for name, (row, col) in (("stairs", (2, 3)), ("obstacles", (2, 6))):      # hardest level of a stairs-up column and of the discrete-obstacles column
        blk = ter.height_field_raw[b + row * px: b + (row + 1) * px, b + col * px: b + (col + 1) * px].copy()
        v, t = convert_heightfield_to_trimesh(blk, tcfg.horizontal_scale, tcfg.vertical_scale, tcfg.slope_treshold)
        moved = (np.abs(v[:, 0] / tcfg.horizontal_scale - np.rint(v[:, 0] / tcfg.horizontal_scale)) > 1e-3).sum()
        assert blk.max() - blk.min() > 20 and (np.abs(np.diff(blk.astype(np.int32), axis=0)) > tcfg.slope_treshold * tcfg.horizontal_scale / tcfg.vertical_scale).any(), name
        data[name + "_raster"] = blk.astype(np.int16)
        data[name + "_vertices"] = v.astype(np.float32)
        data[name + "_triangles"] = t.astype(np.int32)
        print(name, blk.shape, "raster range", blk.min(), blk.max(), "vertices", v.shape, "triangles", t.shape, "off-grid x", int(moved))
    np.savez_compressed(os.path.join(out, "trimesh_tiles.npz"), **data)


def gen_config(out):
    from legged_gym.envs import GR1T1Cfg, GR1T1CfgPPO, GR1T2Cfg, GR1T2CfgPPO
    from legged_gym.utils.helpers import class_to_dict

    def clean(o):
        if isinstance(o, dict):
            return {k: clean(v) for k, v in o.items()}
        if isinstance(o, (list, tuple)):
            return [clean(v) for v in o]
        if isinstance(o, np.ndarray):
            return o.tolist()
        if isinstance(o, (np.floating, np.integer)):
            return o.item()
        return o
    dump = {"GR1T1": clean(class_to_dict(GR1T1Cfg())), "GR1T1PPO": clean(class_to_dict(GR1T1CfgPPO())),
            "GR1T2": clean(class_to_dict(GR1T2Cfg())), "GR1T2PPO": clean(class_to_dict(GR1T2CfgPPO()))}
    with open(os.path.join(out, "config_dump.json"), "w") as f:
        json.dump(dump, f, indent=0, sort_keys=True)


def gen_ppo(out):
    """rsl_rl: GAE returns, minibatch index stream, one PPO.update() on fixed weights/batch."""
    from rsl_rl.modules import ActorCriticMLP
    from rsl_rl.algorithms import PPO
    torch.manual_seed(0)
    N, T, no, npri, na = 16, 8, 39, 168, 10
    ac = ActorCriticMLP(no, npri, na, actor_hidden_dims=[32, 16], critic_hidden_dims=[32, 16], activation="elu", init_noise_std=0.2)
    sd0 = {k: v.clone() for k, v in ac.state_dict().items()}
    alg = PPO(actor_critic=ac, num_learning_epochs=2, num_mini_batches=4, clip_param=0.2, gamma=0.99, lam=0.95,
              value_loss_coef=1.0, entropy_coef=0.01, learning_rate=1e-4, learning_rate_min=1e-5, learning_rate_max=1e-3,
              max_grad_norm=1.0, use_clipped_value_loss=True, schedule="adaptive", desired_kl=0.03, device="cpu",
              storage_class="RolloutStorage")
    alg.init_storage(N, T)
    g = torch.Generator().manual_seed(1)
    obs_seq = torch.randn(T + 1, N, no, generator=g)
    pri_seq = torch.randn(T + 1, N, npri, generator=g)
    rew_seq = torch.randn(T, N, generator=g)
    done_seq = torch.rand(T, N, generator=g) < 0.1
    to_seq = done_seq & (torch.rand(T, N, generator=g) < 0.5)
    eps = torch.randn(T, N, na, generator=g)
    acts = []
    with torch.inference_mode():
        for t in range(T):
            orig = torch.distributions.Normal.sample
            torch.distributions.Normal.sample = lambda self, _e=eps[t]: self.mean + self.stddev * _e
            try:
                a = alg.act(obs_seq[t], pri_seq[t])
            finally:
                torch.distributions.Normal.sample = orig
            acts.append(a.clone())
            alg.process_env_step(rew_seq[t].clone(), done_seq[t], {"time_outs": to_seq[t]})
        alg.compute_returns(pri_seq[T])
    st = alg.storage
    golden = dict(returns=st.returns.numpy().copy(), advantages=st.advantages.numpy().copy(), values=st.values.numpy().copy(),
                  rewards=st.rewards.numpy().copy(), actions=torch.stack(acts).numpy(), log_prob=st.actions_log_prob.numpy().copy(),
                  mu=st.mu.numpy().copy(), sigma=st.sigma.numpy().copy())
    torch.manual_seed(123)
    perm_probe = torch.randperm(4 * (N * T // 4))
    torch.manual_seed(123)
    vl, sl = alg.update()
    sd1 = {k: v.clone() for k, v in ac.state_dict().items()}
    np.savez(os.path.join(out, "ppo.npz"), obs=obs_seq.numpy(), pri=pri_seq.numpy(), rew=rew_seq.numpy(), done=done_seq.numpy(),
             time_outs=to_seq.numpy(), eps=eps.numpy(), perm=perm_probe.numpy(), value_loss=vl, surrogate_loss=sl,
             lr_after=alg.learning_rate, **golden,
             **{"w0_" + k: v.numpy() for k, v in sd0.items()}, **{"w1_" + k: v.detach().numpy() for k, v in sd1.items()})


# ---- the reset family: reset_idx, the terrain curriculum, command resampling, pushes, _get_env_origins (tests/golden/reset_family.npz) ----
class ScriptedDraws:
    """The random calls of one reference post_physics_step(), served from a scripted queue: each entry holds the (lower, upper, shape) the
    call must come with and the uniforms in [0, 1) it is answered from.  A call that does not match its entry, or an entry left over,
    fails the generation: a draw attributed to the wrong call cannot go unnoticed."""

    def __init__(self):
        self.queue = []

    def expect(self, lower, upper, shape, u):
        shape = tuple(int(k) for k in shape)
        self.queue.append((float(lower), float(upper), shape, torch.as_tensor(np.asarray(u, dtype=np.float32)).reshape(shape)))

    def _next(self, lower, upper, shape):
        assert self.queue, f"unscripted random call ({lower}, {upper}, {tuple(shape)})"
        lo, hi, shp, u = self.queue.pop(0)
        assert (float(lower), float(upper), tuple(shape)) == (lo, hi, shp), f"random call ({lower}, {upper}, {tuple(shape)}) where ({lo}, {hi}, {shp}) was scripted"
        return u

    def rand_float(self, lower, upper, shape, device):   # torch_rand_float (isaacgym torch_utils): (upper - lower) * rand + lower in float32
        return (upper - lower) * self._next(lower, upper, shape) + lower

    def randint_like(self, t, high):   # the build's convention for an integer draw: floor(u * high), clipped to high - 1
        return torch.clamp(torch.floor(self._next(0, high, t.shape) * high), max=high - 1).to(t.dtype)


# what a row of a reset-family case is built to do: (curriculum branch, reset cause); 16 kinds, dealt round robin over the rows
RESET_KINDS = (("up", "timeout"), ("down", "tilt"), ("neither", "contact"), ("wrap", "timeout"), ("clip", "tilt"), ("idle", None),
               ("up", "tilt"), ("down", "contact"), ("neither", "timeout"), ("wrap", "contact"), ("clip", "timeout"), ("time", None),
               ("post", "tilt"), ("idle", None), ("down_small", "tilt"), ("neither_small", "contact"))


def reset_uniforms(seed, N, step, nd):
    """The build's draws for global envs 0 .. N-1 at `step`: gro_rand(seed, env, step, stream, item) of oracle/philox.h through the
    oracle library (oracle.binding.uniforms), streams and items as reset_env, resample_commands, the push and the curriculum use them."""
    from oracle.binding import uniforms
    return {name: uniforms(seed, range(N), step, name, items) for name, items in
            (("RESET_DOF", nd), ("RESET_ROOT", 9), ("CMD_TIME", 3), ("CMD_RESET", 3), ("PUSH", 2), ("CURRICULUM", 1))}


def drawn_commands(env, u):
    """_resample_commands' result for the uniforms u (n, 3), in float32 like the reference."""
    r = env.command_ranges
    u = torch.as_tensor(u)
    c = torch.stack([(r["lin_vel_x"][1] - r["lin_vel_x"][0]) * u[:, 0] + r["lin_vel_x"][0],
                     (r["lin_vel_y"][1] - r["lin_vel_y"][0]) * u[:, 1] + r["lin_vel_y"][0],
                     (r["ang_vel_yaw"][1] - r["ang_vel_yaw"][0]) * u[:, 2] + r["ang_vel_yaw"][0]], 1)
    c[:, :2] *= (torch.norm(c[:, :2], dim=1) > 0.1).unsqueeze(1)
    return c


def deal_reset_kinds(env, U, N):
    """A kind per row: RESET_KINDS round robin, except that a row whose time-based draw falls below the 0.1 norm resamples by time and a
    row whose reset draw does resets -- the draws belong to the env index, so the rows that can show `> 0.1` zeroing are given."""
    raw_norm = lambda u: torch.norm(torch.stack([2.0 * torch.as_tensor(u[:, 0]) - 1.0, 1.0 * torch.as_tensor(u[:, 1]) - 0.5], 1), dim=1)
    assert env.command_ranges["lin_vel_x"] == [-1.0, 1.0] and env.command_ranges["lin_vel_y"] == [-0.5, 0.5]
    t_small, r_small = raw_norm(U["CMD_TIME"]) < 0.1, raw_norm(U["CMD_RESET"]) < 0.1
    kinds = [RESET_KINDS[i % 16] for i in range(N)]
    for i in range(N):
        if t_small[i] and r_small[i]:
            kinds[i] = ("post", "tilt")
        elif t_small[i] and kinds[i][0] not in ("time", "post"):
            kinds[i] = ("time", None)
        elif r_small[i] and kinds[i][1] is None:
            kinds[i] = RESET_KINDS[i % 5]
    return kinds


def reset_family_state(env, g, body_names, N, kinds, U, tcfg, ter):
    """Synthetic post-physics state in which row i does what kinds[i] says.  Heightfield (ter given): levels, origins, positions at a
    chosen distance from the origin and commands on the chosen side of every curriculum threshold, each scan point 5e-4 cells from a
    cell edge.  Every row: non-zero action / velocity history, timers, contact history and episode sums, so that reset_idx's clears show."""
    from isaacgym.torch_utils import quat_from_euler_xyz
    nd = env.num_dof
    randomize_state(env, g, body_names, N, 0)
    # the arbitrary inputs on a coarse dyadic grid (short mantissas: the fixture compresses to a third); thresholds keep their side
    for name, step in (("dof_vel", 2), ("torques", 1), ("last_actions", 16), ("last_last_actions", 16), ("last_dof_vel", 2), ("avg_feet_contact_force", 1),
                       ("avg_feet_speed_xyz", 16), ("feet_air_time", 64), ("feet_land_time", 64), ("base_heights_offset", 64), ("contact_forces", 1024)):
        t = getattr(env, name)
        t[:] = torch.round(t * step) / step
    env.dof_pos[:] = torch.round(env.dof_pos * 64) / 64
    env.root_states[:, 7:13] = torch.round(env.root_states[:, 7:13] * 16) / 16
    env.rigid_body_states[:, :, 7:10] = torch.round(env.rigid_body_states[:, :, 7:10] * 16) / 16
    env.actions = env.clip_actions(torch.round(env.actions * 16) / 16)
    env._get_env_origins()                      # terrain_types, terrain_origins, max_terrain_level; the plane: the grid of origins
    term = [int(i) for i in env.termination_contact_indices]
    env.contact_forces[:, term] = 0
    u = lambda *shape: torch.rand(*shape, generator=g)
    t_cmd = drawn_commands(env, U["CMD_TIME"])  # what a time-based resample of this step gives the row
    for i, (branch, cause) in enumerate(kinds):
        # episode length: 1000 -> 1001 times out; 499 / 999 -> a multiple of the resampling interval
        ep = int(torch.randint(0, 990, (1,), generator=g))
        ep = 498 if ep == 499 else ep
        if cause == "timeout":
            ep = 1000
        elif branch == "post":
            ep = 499
        elif branch == "time":
            ep = 499 if (i // 16) % 2 == 0 else 999
        env.episode_length_buf[i] = ep
        yaw = (u(1) * 2 - 1) * 3.14
        if cause == "tilt":                     # |g_z| = cos(1.3) = 0.267 < 0.33
            env.root_states[i, 3:7] = quat_from_euler_xyz(torch.zeros(1), torch.full((1,), 1.3 if i % 2 else -1.3), yaw)[0]
        elif branch == "idle" and i % 32 == 5:  # |g_z| = cos(1.2) = 0.362: tilted, not reset
            env.root_states[i, 3:7] = quat_from_euler_xyz(torch.zeros(1), torch.full((1,), 1.2), yaw)[0]
        else:
            env.root_states[i, 3:7] = rand_quat(1, g, tilt=0.4)[0]
        if cause == "contact":
            env.contact_forces[i, term[i % len(term)], 2] = 5.0
        # commands going in (norm, then a direction), and the distance from the env origin
        ang = u(1) * 6.28
        lvl = 1 + i % 8
        if branch in ("up", "wrap"):
            n, dist, lvl = 0.3 + 0.7 * u(1), 4.5 + 2.0 * u(1), (9 if branch == "wrap" else lvl)
        elif branch in ("down", "clip"):
            n = 0.5 + 0.5 * u(1)
            dist, lvl = (0.1 + 0.6 * u(1)) * 4.0, (0 if branch == "clip" else lvl)
        elif branch == "neither":
            n = torch.zeros(1) if i % 2 else 0.15 + 0.15 * u(1)
            dist = 10.0 * n + 0.3 + 0.6 * u(1)
        elif branch == "down_small":
            n = 0.04 + 0.05 * u(1)
            dist = 5.0 * n
        elif branch == "neither_small":
            n, dist = 0.04 + 0.05 * u(1), 1.5 + u(1)
        elif branch == "post":                  # resets on a step where it also resamples by time: the curriculum sees the NEW commands
            tn = torch.norm(t_cmd[i, :2])
            if tn > 0.1:                        # old commands zero (never down), new ones make it move down
                n, dist = torch.zeros(1), torch.clamp(5.0 * tn, max=3.0).reshape(1)
            else:                               # old commands would move it down, the new (zeroed) ones do not
                n, dist = torch.full((1,), 0.8), torch.full((1,), 2.0)
        else:                                   # idle / time: anything
            n, dist = (torch.zeros(1) if i % 4 == 0 else 1.1 * u(1)), 6.0 * u(1)
        env.commands[i, 0], env.commands[i, 1] = float(n * torch.cos(ang)), float(n * torch.sin(ang))
        if ter is None:
            env.root_states[i, 0:2] += env.env_origins[i, 0:2]
            continue
        env.terrain_levels[i] = lvl
        env.env_origins[i] = env.terrain_origins[lvl, env.terrain_types[i]]
        while True:
            a = u(1) * 6.28
            env.root_states[i, 0:2] = env.env_origins[i, 0:2] + dist * torch.cat([torch.cos(a), torch.sin(a)])
            if scan_edge_margin(env, tcfg, i) >= 5e-4:
                break
    if ter is not None:
        stand_on_terrain(env, g, tcfg, ter, N)
    else:
        torso = int(env.torso_indices[0])
        env.rigid_body_states[:, :, 0:3] = env.root_states[:, None, 0:3]
        env.rigid_body_states[:, env.feet_indices, 2] = torch.rand(N, 2, generator=g) * 0.25
        env.rigid_body_states[:, torso, 3:7] = env.root_states[:, 3:7]
    feet = env.feet_indices                     # (of the feet's positions the step reads z alone)
    env.rigid_body_states[:, feet, 0:2] = torch.round(env.rigid_body_states[:, feet, 0:2])
    env.rigid_body_states[:, feet, 2] = torch.round(env.rigid_body_states[:, feet, 2] * 1024) / 1024
    if nd == 32:
        full_body_link_orientations(env)
    for name in env.episode_sums:
        env.episode_sums[name] = torch.round((torch.rand(N, generator=g) - 0.3) * 2.0 * 4) / 4


def reset_family_margins(env, kinds, U, tcfg, rows, curriculum):
    """The conditions of the fixture, in float64 on the float32 state: no row within 1e-3 (relative) of a threshold the step compares
    against, every floor(u * high) 1e-4 from an integer, every scan point 5e-4 cells from a cell edge.  Returns (violations, counts of
    the rows `rows` per branch)."""
    N = env.num_envs
    bad, cnt = [], {}

    def count(name, mask):
        cnt[name] = int(np.asarray(mask)[rows].sum())

    def off(name, value, thr, rel=1e-3):
        value, thr = np.asarray(value, dtype=np.float64), np.asarray(thr, dtype=np.float64)
        if (np.abs(value - thr) <= rel * np.abs(thr)).any():
            bad.append(name)
    ep1 = env.episode_length_buf.numpy() + 1
    by_time = ep1 % int(env.cfg.commands.resample_command_interval) == 0
    t_raw, r_raw = (np.stack([2.0 * U[k][:, 0].astype(np.float64) - 1.0, U[k][:, 1].astype(np.float64) - 0.5], 1) for k in ("CMD_TIME", "CMD_RESET"))
    cmd = env.commands[:, :2].double().numpy().copy()
    t_norm, r_norm = np.linalg.norm(t_raw, axis=1), np.linalg.norm(r_raw, axis=1)
    cmd[by_time] = t_raw[by_time] * (t_norm[by_time] > 0.1)[:, None]        # the commands the reward and the curriculum see
    cn = np.linalg.norm(cmd, axis=1)
    q = env.root_states[:, 3:7].double().numpy()
    gz = 1.0 - 2.0 * (q[:, 0] ** 2 + q[:, 1] ** 2) / (q ** 2).sum(1)
    causes = np.array([k[1] or "" for k in kinds])
    resets = causes != ""
    off("|g_z| at 0.33", np.abs(gz), 0.33)
    assert ((np.abs(gz) < 0.33) == (causes == "tilt")).all() and ((ep1 > 1000) == (causes == "timeout")).all()
    off("time-drawn commands at the 0.1 norm", t_norm[by_time], 0.1)
    off("reset-drawn commands at the 0.1 norm", r_norm[resets], 0.1)
    off("commands at the 0.1 norm", cn[cn > 0], 0.1)
    for c in ("timeout", "tilt", "contact"):
        count("reset by " + c, causes == c)
    count("no reset", ~resets & ~by_time)
    count("time resample only", ~resets & by_time)
    count("reset and time resample", resets & by_time)
    count("time draw below 0.1", by_time & (t_norm < 0.1))
    count("time draw above 0.1", by_time & (t_norm > 0.1))
    count("reset draw below 0.1", resets & (r_norm < 0.1))
    count("reset draw above 0.1", resets & (r_norm > 0.1))
    if env.custom_origins:
        for i in range(N):
            if scan_edge_margin(env, tcfg, i) < 5e-4:
                bad.append("scan point at a cell edge")
    if curriculum:
        d = np.linalg.norm(env.root_states[:, :2].double().numpy() - env.env_origins[:, :2].double().numpy(), axis=1)
        T = float(env.max_episode_length_s)
        off("distance at env_length / 2", d, env.terrain.env_length / 2)
        off("distance at |cmd| T / 2", d[cn > 0], cn[cn > 0] * T * 0.5)
        up = d > env.terrain.env_length / 2
        down = (d < cn * T * 0.5) & ~up
        old = np.linalg.norm(env.commands[:, :2].double().numpy(), axis=1)
        down_old = (d < old * T * 0.5) & ~up
        lv = env.terrain_levels.numpy()
        top = int(env.max_terrain_level) - 1
        uc = U["CURRICULUM"][:, 0].astype(np.float64) * int(env.max_terrain_level)
        if (np.abs(uc - np.rint(uc)) < 1e-4).any():
            bad.append("floor(u * high) at an integer")
        count("up", resets & up & (lv < top))
        count("down", resets & down & (lv > 0))
        count("neither", resets & ~up & ~down)
        count("wrap from the top level", resets & up & (lv == top))
        count("clip at level 0", resets & down & (lv == 0))
        count("curriculum commands below 0.1", resets & (cn > 0) & (cn < 0.1))
        count("curriculum commands above 0.1", resets & (cn > 0.1))
        count("down with commands below 0.1", resets & down & (cn < 0.1))
        count("decision differs on the pre-resample commands", resets & by_time & (down != down_old))
    return bad, cnt


def reset_family_case(N, robot, seed, step, ter=None, tcfg=None, curriculum=True, init_done=True, dr=True, rows=slice(None),
                      strict=False, kinds=None, state_step=None, build_seed=1):
    """One live reference post_physics_step() -- reset_idx NOT stubbed -- with the build's draws injected.  Returns (record, kinds), or
    None when a condition of the fixture (reset_family_margins) does not hold for this step's draws."""
    import legged_gym.envs.base.legged_robot as LR
    env, g, body_names = make_ref_env(N, seed, terrain_obj=ter, robot=robot)
    nd = env.num_dof
    if ter is None:
        env.cfg.terrain.mesh_type = "plane"
    env.cfg.terrain.curriculum = bool(curriculum and ter is not None)
    env.cfg.domain_rand.push_robots = True
    env.cfg.domain_rand.randomize_init_dof_pos = env.cfg.domain_rand.randomize_init_base_velocity = bool(dr)
    assert not env.cfg.commands.curriculum and not env.cfg.commands.heading_command and env.cfg.env.send_timeouts
    env.cfg.noise.add_noise = False             # (the observation noise is pipeline.npz's subject; without it obs repeats pri_obs' first columns)
    U = reset_uniforms(build_seed, N, step, nd)
    if kinds is None:
        kinds = deal_reset_kinds(env, U, N)
    # (state_step: the state of another case, whose step's draws placed the rows that reset while they resample by time)
    reset_family_state(env, g, body_names, N, kinds, U if state_step is None else reset_uniforms(build_seed, N, state_step, nd), tcfg, ter)
    bad, cnt = reset_family_margins(env, kinds, U, tcfg, rows, env.cfg.terrain.curriculum)
    main = ["reset by timeout", "reset by tilt", "reset by contact", "no reset", "time resample only", "reset and time resample"]
    if env.cfg.terrain.curriculum:
        main += ["up", "down", "neither", "wrap from the top level", "clip at level 0", "curriculum commands below 0.1", "curriculum commands above 0.1"]
    if strict:
        main = list(cnt)
    if bad or any(cnt[k] < 3 for k in main):
        return None
    inp = snapshot_inputs(env)
    inp.update(terrain_levels=env.terrain_levels.numpy().astype(np.int32) if ter is not None else np.zeros(N, np.int32),
               terrain_types=env.terrain_types.numpy().astype(np.int32) if ter is not None else np.zeros(N, np.int32),
               env_origins=env.env_origins.numpy().copy(), episode_sums=np.stack([env.episode_sums[n].numpy().copy() for n in env.reward_names]))
    # the script: the calls of post_physics_step in their order (legged_robot.py:307-334, 377-440, 650-677, 717-826)
    S = ScriptedDraws()
    r = env.command_ranges
    ep1 = env.episode_length_buf + 1
    t_ids = (ep1 % env.cfg.commands.resample_command_interval == 0).nonzero().flatten().numpy()
    r_ids = np.array([i for i, k in enumerate(kinds) if k[1] is not None])

    def resample(ids, name):
        for k, key in enumerate(("lin_vel_x", "lin_vel_y", "ang_vel_yaw")):
            S.expect(r[key][0], r[key][1], (len(ids), 1), U[name][ids, k])
    resample(t_ids, "CMD_TIME")
    pushed = step % int(env.cfg.domain_rand.push_interval) == 0
    if pushed:
        S.expect(-env.cfg.domain_rand.max_push_vel_xy, env.cfg.domain_rand.max_push_vel_xy, (N, 2), U["PUSH"])
    n = len(r_ids)
    if env.cfg.terrain.curriculum and init_done:
        S.expect(0, env.max_terrain_level, (n,), U["CURRICULUM"][r_ids, 0])
    if dr:
        S.expect(0.5, 1.5, (n, nd), U["RESET_DOF"][r_ids])
    if env.custom_origins:
        S.expect(-1.0, 1.0, (n, 2), U["RESET_ROOT"][r_ids, 0:2])
    S.expect(-2 * np.pi, 2 * np.pi, (n, 1), U["RESET_ROOT"][r_ids, 2:3])
    if dr:
        S.expect(-0.5, 0.5, (n, 6), U["RESET_ROOT"][r_ids, 3:9])
    resample(r_ids, "CMD_RESET")
    env.common_step_counter = step - 1          # post_physics_step counts it up before the push test
    env.init_done = bool(init_done)
    orig = (LR.torch_rand_float, torch.randint_like)
    LR.torch_rand_float, torch.randint_like = S.rand_float, S.randint_like
    try:
        env.post_physics_step()
    finally:
        LR.torch_rand_float, torch.randint_like = orig
    assert not S.queue, f"{len(S.queue)} scripted draws were never asked for"
    assert env.common_step_counter == step and sorted(env.reset_buf.nonzero().flatten().tolist()) == sorted(r_ids.tolist())
    ex = env.extras["episode"]
    outd = dict(dof_pos=env.dof_pos.numpy().copy(), dof_vel=env.dof_vel.numpy().copy(), root=env.root_states.numpy().copy(),
                commands=env.commands.numpy().copy(), env_origins=env.env_origins.numpy().copy(),
                terrain_levels=env.terrain_levels.numpy().astype(np.int32) if ter is not None else np.zeros(N, np.int32),
                reset=env.reset_buf.numpy().astype(bool), time_out=env.time_out_buf.numpy().copy(), episode_length=env.episode_length_buf.numpy().copy(),
                pri_obs=torch.clip(env.pri_obs_buf, -100, 100).numpy().copy(), obs=torch.clip(env.obs_buf, -100, 100).numpy().copy(),
                rew=env.rew_buf.numpy().copy(), last_actions=env.last_actions.numpy().copy(), last_last_actions=env.last_last_actions.numpy().copy(),
                last_dof_vel=env.last_dof_vel.numpy().copy(), feet_air_time=env.feet_air_time.numpy().copy(),
                feet_land_time=env.feet_land_time.numpy().copy(), feet_contact=env.feet_contact.numpy().astype(bool),
                episode_sums=np.stack([env.episode_sums[n].numpy().copy() for n in env.reward_names]),
                extras_rew=np.array([float(ex["rew_" + n]) for n in env.reward_names], dtype=np.float32),
                extras_time_outs=env.extras["time_outs"].numpy().copy())
    assert set(ex) - {"terrain_level"} == {"rew_" + n for n in env.reward_names}
    if env.cfg.terrain.curriculum:
        outd["extras_terrain_level"] = np.float32(ex["terrain_level"])
    else:
        assert "terrain_level" not in ex
    rec = {"in_" + k: v for k, v in inp.items()}
    rec.update({"out_" + k: v for k, v in outd.items()})
    rec.update({"u_" + k: v for k, v in U.items()})
    rec.update(step_seed_offset=np.array([step, build_seed, 0], dtype=np.int64),   # common_step_counter, seed, env_offset of the build's handle
               reward_names=np.array(env.reward_names), branch_names=np.array(list(cnt)), branch_counts=np.array([cnt[k] for k in cnt], dtype=np.int32))
    return rec, kinds


def gen_reset_family(out):
    """tests/golden/reset_family.npz: the reference's LIVE reset path -- reset_idx and what it calls (the terrain-curriculum move,
    _reset_dofs, _reset_root_states, _resample_commands), the time-based resample, _push_robots, the buffer clears of both classes, the
    extras["episode"] means -- through one post_physics_step() per case, and _get_env_origins.

    The reference draws from torch's global generators, which the build cannot reproduce; so the build's own draws go INTO the
    reference: torch_rand_float (as legged_robot.py sees it) and torch.randint_like are replaced for the duration of the step by a
    scripted queue (ScriptedDraws) of the uniforms gro_rand(seed, env, step = common_step_counter, stream, item) of oracle/philox.h --
    RESET_DOF item j, RESET_ROOT 0-8, CMD_TIME / CMD_RESET 0-2, PUSH 0-1, CURRICULUM 0 -- computed for every env by the oracle library
    and indexed with the env ids of each call.  randint_like returns floor(u * high) clipped to high - 1: that is the build's convention,
    the reference's own integer generator is not reproducible.  The uniforms are stored; the tests check them against today's gro_rand.

    Cases (64 envs unless noted; rows are built so that every branch is taken by several rows, RESET_KINDS):
      curr       heightfield (the raster of terrain.npz), curriculum on, init_done
      push       the same state on a step where the push fires; pushed rows that reset lose the push to the reset
      nodr       the same state with randomize_init_dof_pos / randomize_init_base_velocity off
      init       the same state with init_done False, on the draws of the build's first reset_all: the levels must not move
      plane      mesh_type 'plane': grid origins, no xy offset, no curriculum
      shard      128 envs; the tests run rows 64-127 as a handle with env_offset 64 of 128
      full_body  the 32-DOF robot (build_full_body_cfg)
      origins    _get_env_origins alone: terrain_types for several (num_envs, 20), the plane grid
    The conditions under which the cases compare without excluding a row are asserted HERE (reset_family_margins): no row within 1e-3
    of a threshold, floor(u * high) 1e-4 from an integer, scan points 5e-4 cells from a cell edge, at least 3 rows per branch."""
    from legged_gym.utils.terrain import Terrain
    from legged_gym.envs.base.legged_robot_config import LeggedRobotCfg
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if repo not in sys.path:
        sys.path.insert(0, repo)
    tcfg = LeggedRobotCfg.terrain()
    tcfg.mesh_type = "heightfield"
    np.random.seed(1)
    ter = Terrain(tcfg, 64)          # the raster of terrain.npz
    data, arrays = {}, {}

    def first(steps, **kw):
        for step in steps:
            got = reset_family_case(step=step, **kw)
            if got is not None:
                return got
        raise AssertionError("no step whose draws meet the fixture's conditions")

    def store(case, rec, like=None, same_state=False):
        """The storage layout (tests/test_reset_golden.py load_case undoes it; a zip member costs ~250 bytes, a case has ~50 arrays):
          <case>_f32, <case>_f32_names   every per-row float32 array of the case, one row of the matrix per column of the array ("name:2x3"; "name:T24": a (24, rows) array as it is)
          <case>_i32, <case>_i32_names   the same for the per-row integer and boolean arrays ("name:2:|b1")
          <case>_same                    "name=@other" / "name=@other[:k]": an array equal to one already stored for this case or for the
                                         case `like` (the cases that share curr's state; obs = pri_obs' leading columns without noise; ...)
          <case>_<name>                  everything else"""
        rows = len(rec["in_root"])
        names, cols, inames, icols, same = [], [], [], [], []
        for k, v in rec.items():
            v = np.asarray(v)
            twin = None
            for n, w in arrays.items() if v.size > 16 else ():
                if not (n.startswith(case + "_") or (like and n.startswith(like + "_"))) or w.dtype != v.dtype or w.ndim != v.ndim:
                    continue
                if w.shape == v.shape and np.array_equal(w, v):
                    twin = "@" + n
                elif v.ndim == 2 and w.shape[0] == v.shape[0] and w.shape[1] > v.shape[1] and np.array_equal(w[:, :v.shape[1]], v):
                    twin = f"@{n}[:{v.shape[1]}]"
                if twin:
                    break
            if twin is not None:
                same.append(k + "=" + twin)
                continue
            arrays[case + "_" + k] = v
            if v.dtype == np.float32 and v.ndim >= 1 and v.shape[0] == rows:
                names.append(k + ":" + "x".join(str(n) for n in v.shape[1:]))
                cols.append(v.reshape(rows, -1).T)
            elif v.dtype == np.float32 and v.ndim == 2 and v.shape[1] == rows:      # (terms, rows): the episode sums
                names.append(k + ":T" + str(v.shape[0]))
                cols.append(v)
            elif v.dtype.kind in "iub" and v.ndim >= 1 and v.shape[0] == rows:
                inames.append(k + ":" + "x".join(str(n) for n in v.shape[1:]) + ":" + v.dtype.str)
                icols.append(v.reshape(rows, -1).T.astype(np.int32))
            else:
                data[case + "_" + k] = v
        assert not same_state or all(any(a.startswith(k + "=") for a in same) for k in rec if k.startswith("in_")), case   # the same state: stored once
        data[case + "_same"] = np.array(same)
        for tag, nm, cl in (("_f32", names, cols), ("_i32", inames, icols)):
            if cl:
                data[case + tag], data[case + tag + "_names"] = np.concatenate(cl), np.array(nm)
    plain = [s for s in range(3, 4000) if s % 500]
    curr, kinds = first(plain, N=64, robot="gr1t1_lower_limb", seed=51, ter=ter, tcfg=tcfg, strict=True)
    store("curr", curr)
    step = int(curr["step_seed_offset"][0])
    shared = dict(N=64, robot="gr1t1_lower_limb", seed=51, ter=ter, tcfg=tcfg, kinds=kinds, state_step=step)
    rec, _ = first(range(500, 20000, 500), **shared)
    assert np.abs(rec["out_root"][~rec["out_reset"], 7:9] - curr["out_root"][~curr["out_reset"], 7:9]).min() > 0
    store("push", rec, "curr", True)
    rec, _ = first([step], dr=False, **shared)
    store("nodr", rec, "curr", True)
    # (the build takes init_done = False in reset_all alone, whose draws are keyed by step 0x80000000 + the number of resets so far)
    rec, _ = first([0x80000000], init_done=False, **shared)
    assert np.array_equal(rec["out_terrain_levels"], rec["in_terrain_levels"]) and not np.array_equal(curr["out_terrain_levels"], curr["in_terrain_levels"])
    store("init", rec, "curr", True)
    rec, _ = first(plain, N=64, robot="gr1t1_lower_limb", seed=51, curriculum=False)
    for k in ("in_dof_pos", "in_actions", "in_torques"):     # (the seed of curr: randomize_state's arrays are the same)
        assert np.array_equal(rec[k], curr[k]), k
    store("plane", rec, "curr")
    rec, _ = first(plain, N=128, robot="gr1t1_lower_limb", seed=55, ter=ter, tcfg=tcfg, rows=slice(64, 128))
    rec["step_seed_offset"][2] = 64              # rows 64-127 are stored: what a handle with env_offset 64 of 128 envs computes
    for k in ("out_extras_rew", "out_extras_terrain_level"):   # (means over all 128 envs: a shard's statistics cover its own rows)
        del rec[k]
    for k, v in rec.items():
        if k.startswith(("in_", "out_", "u_")):
            rec[k] = np.take(v, np.arange(64, 128), axis=v.shape.index(128))
    store("shard", rec, "curr")
    rec, _ = first(plain, N=64, robot="gr1t1", seed=57, ter=ter, tcfg=tcfg)
    store("full_body", rec, "curr")
    # _get_env_origins alone (legged_robot.py:1163-1195)
    for N in (64, 100, 4095, 4096):
        for curriculum, max_init in ((True, 4), (False, 4)):
            env, _, _ = make_ref_env(N, 59, terrain_obj=ter)
            env.cfg.terrain.curriculum, env.cfg.terrain.max_init_terrain_level = curriculum, max_init
            env._get_env_origins()
            top = max_init if curriculum else env.cfg.terrain.num_rows - 1
            assert int(env.terrain_levels.min()) >= 0 and int(env.terrain_levels.max()) <= top and (N < 4095 or int(env.terrain_levels.max()) == top)
            assert env.custom_origins and torch.equal(env.env_origins, env.terrain_origins[env.terrain_levels, env.terrain_types])
            if curriculum:
                data[f"origins_types_{N}"] = env.terrain_types.numpy().astype(np.int16)
    data["origins_num_cols"] = np.int64(tcfg.num_cols)
    for N in (64, 100, 4096):
        env, _, _ = make_ref_env(N, 59)
        env.cfg.terrain.mesh_type = "plane"
        env._get_env_origins()
        assert not env.custom_origins
        data[f"origins_grid_{N}"] = env.env_origins.numpy().T.copy()      # (3, N): a coordinate per row
    path = os.path.join(out, "reset_family.npz")
    np.savez_compressed(path, **data)
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(out, "pipeline.npz")), "reset_family.npz outgrew the largest fixture"


def main():
    os.makedirs(OUT, exist_ok=True)
    install_stub()
    if len(sys.argv) > 1:            # python tools/gen_golden.py gen_pipeline_rough  -> only the named fixtures
        for name in sys.argv[1:]:
            globals()[name](OUT)
        return
    gen_quat(OUT)
    gen_torques(OUT)
    gen_control_modes(OUT)
    gen_pipeline(OUT)
    gen_pipeline_rough(OUT)
    gen_pipeline_other_robots(OUT)
    gen_reward_terms(OUT)
    gen_base_reward_terms(OUT)
    gen_command_curriculum(OUT)
    gen_terrain_and_heights(OUT)
    gen_terrain_all_tiles(OUT)
    gen_trimesh_tiles(OUT)
    gen_config(OUT)
    gen_ppo(OUT)
    gen_reset_family(OUT)
    for f in sorted(os.listdir(OUT)):
        print(f, os.path.getsize(os.path.join(OUT, f)))


if __name__ == "__main__":
    main()
