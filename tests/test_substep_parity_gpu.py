"""Every step kernel family against the fp64 oracle ONE physics sub-step at a time (tests/substep.py): fused 1 / 2 / 4 / 8 waves, quad4,
quad, tree, tree16, generic, their *_trimesh heads and one *_base entry per family.  With one sub-step per step nothing amplifies
rounding, so a row is either inside SUBSTEP_BAND -- SENS_K x what the fp32 oracle shows against the fp64 one on the same trajectory -- or
counted against the scene's caps (substep.scene_caps): no twins, no outlier fractions, no hard-cap table.  A contact impulse, friction
anchor, face contact or self-collision force that is off by a newton fails here.  The *_far cases hold the same kernels at the coordinates of
a real run's far side (189 m on the plane grid, raster cell ~1850 of the curriculum grid) to the fp32 oracle's own error there.

The oracle side of a scene is computed once and shared by the layouts next to it.  The observed maxima per (scene, layout, tensor) and their
ratio to the fp32 oracle's are printed, and appended to the jsonl file GRX_SUBSTEP_LOG names, if set (profiles/substep_hip.jsonl holds an
MI355X's)."""
import os

import pytest

from tests import substep
from tests.test_generic_gpu import pick
from tests.test_hip_parity import set_layout

pytestmark = pytest.mark.gpu

LOG = os.environ.get("GRX_SUBSTEP_LOG")   # a jsonl path, or nothing: the record is printed either way
FUSED = (1, 2, 4, 8, "quad4", "quad")
TREES = ("tree", "tree16", "generic")
CASES = ([("plane", l) for l in FUSED] + [("plane_t2", l) for l in (8, "quad")]
         + [("plane_n50", l) for l in FUSED]                                   # 50 envs: a partial block and tail lanes in every layout
         + [("plane_lowmu", l) for l in (1, 8, "quad")]
         + [("legs", l) for l in (1, 8, "quad4", "quad")]
         + [(s, l) for s in ("slope_hf", "slope_tm", "stairs_hf", "stairs_tm") for l in (1, 8, "quad")]
         + [(s, l) for s in ("full_plane", "full_stairs") for l in TREES]
         + [("base_plane", "base")] + [("base_full_plane", l) for l in TREES]   # one *_base entry per family
         # 128-256 m from the origin, where pos, the anchors and terrain_locate's cell index carry 8-32 x the rounding: the last 64 envs of a 4096-env
         # plane grid, and the far tile of the 10 x 20 curriculum raster (bands and caps of their own: substep.SUBSTEP_BAND, scene_caps)
         + [("plane_far", l) for l in FUSED] + [("plane_t2_far", l) for l in (8, "quad")] + [("base_plane_far", "base")]
         + [(s, l) for s in ("slope_hf_far", "slope_tm_far") for l in (1, 8, "quad")]
         + [(s, l) for s in ("full_plane_far", "full_slope_tm_far") for l in TREES])


def select(monkeypatch, scene, layout):
    """The kernel family and launch layout of the handles created from here on, as the policy-step tests select them."""
    if layout in TREES:
        pick(monkeypatch, layout)
    elif layout != "base":             # (the fused base entry is what the library picks for a handle with base terms)
        set_layout(monkeypatch, layout)


def assert_selected(hip, scene, layout):
    lay = hip.layout()
    if layout in TREES:
        assert lay["kernel"].startswith({"tree": "grx_step_tree", "tree16": "grx_step_tree16", "generic": "grx_step_generic"}[layout]), lay
        assert lay["lanes_per_env"] == {"tree": 8, "tree16": 16, "generic": 1}[layout], lay
    elif layout == "base":
        assert lay["kernel"].startswith("grx_step_kernel_base") and lay["lanes_per_env"] == 2, lay
    elif layout in ("quad", "quad4"):
        assert lay["lanes_per_env"] == 4 and lay["waves_per_block"] == (4 if layout == "quad4" else 8), lay
    else:
        assert lay["lanes_per_env"] == 2 and lay["waves_per_block"] == layout, lay
    assert ("_base" in lay["kernel"]) == scene.base and ("trimesh" in lay["kernel"]) == (scene.mesh == "trimesh"), lay


@pytest.mark.parametrize("name,layout", CASES, ids=[f"{s}-{l}" for s, l in CASES])
def test_one_substep_from_identical_state(name, layout, monkeypatch):
    scene = substep.SCENES[name]
    traj = substep.oracle_trajectory(name)
    select(monkeypatch, scene, layout)
    hip = substep.make_hip(scene)
    try:
        assert_selected(hip, scene, layout)
        got = substep.replay(traj, hip)
    finally:
        hip.close()
    substep.check(traj, got, str(layout), log=LOG)


def test_the_cases_cover_every_scene():
    """Every scene of tests/substep.py runs on some kernel (what a scene exercises is asserted on the CPU: tests/test_substep_parity.py)."""
    assert {s for s, _ in CASES} == set(substep.SCENES)
