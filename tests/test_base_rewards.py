"""legged_gym's base reward terms (include/grx.h ABI 7, grx_base_reward_term): the CPU tier.

LeggedRobot's generic `_reward_*` methods (legged_robot.py:1277-1376) that the FFTAI / GR1 classes do not override are valid reward
terms of the reference's GR1T1 / GR1T2 envs.  build_config fills their table of grx_config; the library reports the same names.  The
GPU tier (tests/test_base_rewards_gpu.py) pins the kernels to the reference's own values (tests/golden/base_reward_terms.npz)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.helpers import make_cfg
from wiki_grx_gym_amd import _capi
from wiki_grx_gym_amd.envs import build_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(G, "base_reward_terms.npz")


def _lib():
    return C.CDLL(os.path.join(ROOT, "wiki-grx-gym_amd", "csrc", "libgrx_hip.so"))


def base_cfg(task="GR1T1", **kw):
    """The registered config with every base term enabled at the fixture's scales."""
    d = np.load(FIXTURE)
    cfg = make_cfg(task=task, noise=False, dr=False, **kw)
    for n, v in zip(d["names"], d["scales"]):
        setattr(cfg.rewards.scales, str(n), float(v))
    return cfg


def test_build_accepts_every_base_term():
    cfg = base_cfg()
    c, _, meta = build_config.build(cfg, cfg.sim.dt, 8)
    d = np.load(FIXTURE)
    want = dict(zip(map(str, d["names"]), d["scales"]))
    assert [c.base_reward_scale[t] for t in range(_capi.NUM_BASE_REWARD_TERMS)] == pytest.approx([want[n] for n in _capi.BASE_REWARD_TERMS])
    assert c.tracking_sigma == pytest.approx(cfg.rewards.tracking_sigma)
    assert c.max_contact_force == pytest.approx(cfg.rewards.max_contact_force)
    assert c.command_curriculum == 0
    # the FF/GR1 table is filled as before; active_terms covers both tables, alphabetically
    assert c.reward_scale[_capi.REWARD_TERMS.index("termination")] == pytest.approx(cfg.rewards.scales.termination)
    assert set(_capi.BASE_REWARD_TERMS) <= set(meta["active_terms"])
    assert meta["active_terms"] == sorted(meta["active_terms"])


def test_registered_config_leaves_the_base_table_empty():
    cfg = make_cfg()
    c, _, meta = build_config.build(cfg, cfg.sim.dt, 8)
    assert all(c.base_reward_scale[t] == 0 for t in range(_capi.NUM_BASE_REWARD_TERMS))
    assert set(meta["active_terms"]) <= set(_capi.REWARD_TERMS)


def test_an_unknown_reward_term_still_raises():
    cfg = base_cfg()
    cfg.rewards.scales.no_such_term = 1.0
    with pytest.raises(ValueError, match="reward terms without an implementation"):
        build_config.build(cfg, cfg.sim.dt, 8)


def test_library_names_and_struct_sizes_match_the_mirror():
    lib = _lib()
    api = _capi.bind(lib)
    assert api["abi_version"]() == _capi.GRX_ABI_VERSION == 7
    assert [api["base_reward_term_name"](t).decode() for t in range(_capi.NUM_BASE_REWARD_TERMS)] == list(_capi.BASE_REWARD_TERMS)
    assert api["base_reward_term_name"](_capi.NUM_BASE_REWARD_TERMS) is None
    for name, (sid, struct) in _capi.STRUCT_IDS.items():
        assert api["sizeof"](sid) == C.sizeof(struct), name


def test_header_enum_and_tensor_ids_match_the_mirror(tmp_path):
    import subprocess
    src = tmp_path / "b.c"
    src.write_text('#include <stddef.h>\n#include "grx.h"\n'
                   'int a(void){return GRX_NUM_BASE_REWARD_TERMS;} int b(void){return GRX_T_BASE_EPISODE_SUMS;}\n'
                   'int c(void){return GRX_T_BASE_EPISODE_STATS_HISTORY;} int d(void){return GRX_BREW_TRACKING_LIN_VEL;}\n'
                   'size_t e(void){return offsetof(grx_config, base_reward_scale);} size_t f(void){return offsetof(grx_config, max_curriculum);}\n')
    so = tmp_path / "b.so"
    subprocess.run(["gcc", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.e.restype = lib.f.restype = C.c_size_t
    assert lib.a() == _capi.NUM_BASE_REWARD_TERMS
    assert lib.b() == _capi.T["BASE_EPISODE_SUMS"] and lib.c() == _capi.T["BASE_EPISODE_STATS_HISTORY"]
    assert lib.d() == _capi.BASE_REWARD_TERMS.index("tracking_lin_vel")
    assert lib.e() == _capi.Config.base_reward_scale.offset and lib.f() == _capi.Config.max_curriculum.offset


def test_both_tables_cover_what_the_reference_resolves():
    """The union of the FF/GR1 table and the base table is exactly the set of `_reward_*` names the reference's GR1T1 class resolves
    (stored in the fixture by tools/gen_golden.py)."""
    d = np.load(FIXTURE)
    resolvable = set(map(str, d["resolvable"]))
    assert set(_capi.REWARD_TERMS) | set(_capi.BASE_REWARD_TERMS) == resolvable
    assert list(map(str, d["names"])) == list(_capi.BASE_REWARD_TERMS)


def test_fixture_crosses_every_threshold():
    """The fixture's rows sit on both sides of every threshold the base terms have (tools/gen_golden.py asserts it when it writes them)."""
    d = np.load(FIXTURE)
    names = list(map(str, d["names"]))
    for case in ("plane", "rough"):
        v = d[case + "_values"]
        for n in ("dof_pos_limits", "dof_vel_limits", "torque_limits", "feet_contact_forces", "stumble"):
            k = names.index(n)
            assert (v[k] > 0).any() and (v[k] == 0).any(), (case, n)
        assert np.isfinite(d[case + "_rew"]).all()
    assert d["rough_measured_heights"].std(axis=1).max() > 0.05   # base_height sees a non-uniform scan


def test_command_curriculum_fields():
    cfg = base_cfg()
    cfg.commands.curriculum = True
    cfg.commands.max_curriculum = 1.7
    c, _, _ = build_config.build(cfg, cfg.sim.dt, 8)
    assert c.command_curriculum == 1 and c.max_curriculum == pytest.approx(1.7)
    assert list(c.cmd_lin_vel_x) == pytest.approx(list(cfg.commands.ranges.lin_vel_x))


def test_command_curriculum_without_tracking_lin_vel_raises():
    """The reference raises KeyError at the first reset (legged_robot.py:836 reads episode_sums["tracking_lin_vel"]); build_config refuses the
    config up front."""
    cfg = make_cfg()
    cfg.commands.curriculum = True
    with pytest.raises(ValueError, match="tracking_lin_vel"):
        build_config.build(cfg, cfg.sim.dt, 8)


def test_command_curriculum_fixture():
    """tests/golden/command_curriculum.npz (the reference's update_command_curriculum): restated here, the decision and the clipped
    widening of every call."""
    d = np.load(os.path.join(G, "command_curriculum.npz"))
    lo, hi = d["start"]
    m = float(d["max_curriculum"])
    widened = 0
    for k in range(len(d["reset"])):
        mean = d["sums"][k][d["reset"][k]].astype(np.float32).mean() / d["max_episode_length"]
        if mean > 0.8 * d["scale_dt"]:
            lo, hi = np.clip(lo - 0.5, -m, 0.0), np.clip(hi + 0.5, 0.0, m)
            widened += 1
        assert np.allclose([lo, hi], d["lin_vel_x"][k]), k
    assert 0 < widened < len(d["reset"]) and hi == m and lo == -m   # the threshold goes both ways, the clip is reached
