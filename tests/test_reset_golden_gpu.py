"""The reference's live reset path on the HIP kernels (`-m gpu`): tests/golden/reset_family.npz (tools/gen_golden.py gen_reset_family)
through the checkers of tests/test_reset_golden.py.

Two tiers.  The debug entry (grx_debug_post_physics, apply_reset = 1) runs the post-physics half of the step kernel of every layout on
the recorded inputs: every row of every recorded output at 1e-4, the episode statistics through episode_stats().  The product step
(grx_step, no debug entry) checks what is determined by the draws whatever the physics does: the state of rows that time out and the
push of rows that do not."""
import numpy as np
import pytest
import torch

from tests import test_oracle_golden as og
from tests import test_reset_golden as rg
from tests.test_hip_golden import KERNEL_OF, LAYOUTS, pick_layout

pytestmark = pytest.mark.gpu

LOWER_LIMB_CASES = ("curr", "push", "nodr", "plane", "shard")


def make_hip_case(case, k, layout, monkeypatch, cfg_edit=None):
    """The handle of a case (64 envs; the shard: env_offset 64 of 128) on the step kernel `layout` names."""
    from wiki_grx_gym_amd.envs import build_config
    from wiki_grx_gym_amd.sim import HipSim
    pick_layout(monkeypatch, layout)
    if case == "full_body":      # the 32-DOF model runs on the tree kernels by itself
        monkeypatch.delenv("GRX_FORCE_GENERIC", raising=False)
    cfg = rg.case_cfg(case)
    if cfg_edit:
        cfg_edit(cfg)
    step, seed, off = (int(x) for x in k["step_seed_offset"])
    N = k["in_root"].shape[0]
    assert N == 64
    ter = None if case == "plane" else og.reference_raster_terrain()[0]
    c, keep, meta = build_config.build(cfg, cfg.sim.dt, N, off, N + off, seed, ter)
    sim = HipSim(c, "cuda:0", keep)
    lay = sim.layout()
    name, lpe, waves = KERNEL_OF[layout]
    assert lay["kernel"].startswith(name) and lay["lanes_per_env"] == lpe and (case == "full_body" or lay["waves_per_block"] == waves), lay
    return sim, meta, cfg, c


@LAYOUTS
@pytest.mark.parametrize("case", LOWER_LIMB_CASES)
def test_reset_family_on_the_hip_kernel(case, layout, monkeypatch):
    k = rg.load_case(rg.fixture(), case)
    sim, meta, _, _ = make_hip_case(case, k, layout, monkeypatch)
    print(case, layout, "worst:", rg.check_reset_case(sim, case, k, meta, 1e-4))
    sim.close()


@pytest.mark.parametrize("layout", ["tree", "tree16"])
def test_full_body_reset_family_on_the_tree_kernels(layout, monkeypatch):
    """RESET_DOF items 0-31 and the tree kernels' reset.  (The one-lane generic kernel takes no injection: grx_debug_post_physics refuses it.)"""
    k = rg.load_case(rg.fixture(), "full_body")
    sim, meta, _, _ = make_hip_case("full_body", k, layout, monkeypatch)
    print("full_body", layout, "worst:", rg.check_reset_case(sim, "full_body", k, meta, 1e-4))
    sim.close()


@LAYOUTS
def test_init_done_false_leaves_the_levels_on_the_hip_kernel(layout, monkeypatch):
    k = rg.load_case(rg.fixture(), "init")
    sim, meta, _, _ = make_hip_case("init", k, layout, monkeypatch)
    print("init", layout, "worst:", rg.check_init_case(sim, k, meta, 1e-4))
    sim.close()


def test_env_origins_on_the_hip_library():
    from wiki_grx_gym_amd.sim import HipSim
    rg.check_origins(lambda b: HipSim(b[0], "cuda:0", b[1]), (64,))


@pytest.mark.parametrize("layout", [8, "quad", "tree", "tree16"])      # one layout of each kernel family (the tree kernels: both group sizes)
@pytest.mark.parametrize("case", ["curr", "push"])
def test_product_step_resets_and_pushes_like_the_reference(case, layout, monkeypatch):
    """grx_step itself, push_interval = 1, at the fixture's common_step_counter.  Rows whose episode_length_buf is written to 1000 time
    out; after the step their DOF_POS, DOF_VEL, ROOT_STATES, COMMANDS, TERRAIN_LEVELS and ENV_ORIGINS are the reference's recorded ones:
    all of it is decided by the draws and by the curriculum's comparison of the PRE-reset position, which one policy step cannot carry
    across a threshold -- the rows are those the fixture puts more than 0.5 m from both.  `push`: the velocity of the rows that do not
    reset is the reference's recorded push."""
    k = rg.load_case(rg.fixture(), case)
    sim, meta, cfg, c = make_hip_case(case, k, layout, monkeypatch, rg.push_every_step)
    print(case, layout, "worst:", rg.check_product_step(sim, c, cfg, k, meta, case))
    sim.close()
