"""The sub-step tier's own footing, on the CPU (tests/substep.py): SUBSTEP_BAND is SENS_K x what the fp32 oracle shows against the fp64
oracle over exactly the trajectories the GPU tests replay (tests/test_substep_parity_gpu.py), each scene reaches the contact regimes it is
there for, and the fp32 oracle itself meets the conditions the kernels are held to, with room to spare -- near the origin and, in band
classes of their own, at the far side of a real run's grid (the *_far scenes)."""
import json
import os

import pytest

from tests import substep
from tests.substep import MIN_REGIME, SCENES, SENS_K, SUBSTEP_BAND

ALLOW = 1.25       # the fp32 oracle may sit this far beyond SUBSTEP_BAND / SENS_K (another libm, another compiler) before the table is stale
NEAR = ("plane", "raster", "full")
CLASSES = NEAR + tuple(c + "_far" for c in NEAR)


@pytest.mark.parametrize("cls", CLASSES)
def test_the_band_is_the_fp32_oracles_own_error(cls):
    """Per scene of the class: (1) the fp32 oracle stays inside SUBSTEP_BAND / SENS_K x 1.25 -- a later change of the oracle cannot
    silently loosen the table --, (2) every regime counter the scene is meant to reach is >= 100 env-sub-steps, (3) the conditions of
    substep.check hold for the fp32 oracle with room to spare: no row out of band or with a differing discrete output (stairs: at most
    one of the three), contact thresholds falling the other way in at most three quarters of the allowed rows (observed: at most 5 of the
    7 that 2e-4 of 38 400 env-sub-steps allow; far scenes: in at most HALF of the allowed rows -- observed: 21-30 of the 61 that 8 x 2e-4
    allow --, and the band and the in-band condition are over the rows that are no threshold rows).  Over the class: the table is not
    looser than its measurement either (its largest entry is reached to 1 / 1.25)."""
    band = SUBSTEP_BAND[cls]
    top = {n: 0.0 for n in band}
    problems = []
    for name, scene in SCENES.items():
        if scene.cls != cls:
            continue
        mx, cmp, traj = substep.measure_fp32(name)
        counters = substep.regime_counters(traj)
        print("substep fp32:", json.dumps({"scene": name, "max": {n: float(f"{v:.3e}") for n, v in mx.items()}, "counters": counters,
                                           "flag_rows": int(cmp["flags"].sum()), "threshold_rows": int(cmp["thresholds"].sum())}))
        for n in scene.banded:
            top[n] = max(top[n], mx[n])
            if mx[n] > band[n] / SENS_K * ALLOW:
                problems.append(f"{name}: fp32 oracle {n} {mx[n]:.3e} beyond band / SENS_K x {ALLOW} = {band[n] / SENS_K * ALLOW:.3e}")
        for c in scene.reach:
            if counters[c] < MIN_REGIME:
                problems.append(f"{name}: regime {c} reached in {counters[c]} env-sub-steps only")
        if scene.slip_dominates and counters["slip"] < 0.9 * counters["foot_contact"]:
            problems.append(f"{name}: slip in {counters['slip']} of {counters['foot_contact']} env-sub-steps in foot contact only")
        out = cmp["flags"].clone()
        held = substep.banded_rows(scene, cmp)
        for n in scene.banded:
            out |= (cmp["err"][n] > band[n]) & held
        bad_cap, threshold_cap = substep.scene_caps(scene, traj.rows)
        if int(out.sum()) > bad_cap // 3:
            problems.append(f"{name}: {int(out.sum())} rows of the fp32 oracle out of band or with a differing discrete output")
        room = threshold_cap // 2 if scene.far else 3 * threshold_cap // 4
        if int(cmp["thresholds"].sum()) > room:
            problems.append(f"{name}: {int(cmp['thresholds'].sum())} rows of the fp32 oracle with a contact threshold the other way ({'half' if scene.far else '3 / 4'} of the cap: {room})")
    for n, v in top.items():
        if v * SENS_K * ALLOW < band[n]:
            problems.append(f"{cls}: SUBSTEP_BAND[{n}] = {band[n]:.3e} is looser than SENS_K x the measured {v:.3e}")
    assert not problems, "\n".join(problems)


def test_the_recorded_maxima_give_the_committed_band():
    """profiles/substep_bands.json (python -m tests.substep) is what SUBSTEP_BAND was taken from: the near scenes and classes at its top
    level, as they always were, the far ones under "far"; every far scene's reference-alone rows are in it, against the cap the kernels
    are held to: no flag row, threshold rows in at most half of the cap."""
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "substep_bands.json")) as f:
        rec = json.load(f)
    far = rec["far"]
    near_band = {c: b for c, b in SUBSTEP_BAND.items() if c in NEAR}
    far_band = {c: b for c, b in SUBSTEP_BAND.items() if c not in NEAR}
    assert rec["sens_k"] == SENS_K and set(rec["maxima"]) == {n for n, s in SCENES.items() if not s.far} and set(near_band) == set(NEAR)
    assert substep.band_from(rec["maxima"]) == near_band == rec["band"]
    assert set(far["maxima"]) == set(far["fp32_rows"]) == {n for n, s in SCENES.items() if s.far}
    assert substep.band_from(far["maxima"]) == far_band == far["band"] and set(far_band) == set(CLASSES) - set(NEAR)
    assert substep.band_from({**rec["maxima"], **far["maxima"]}) == SUBSTEP_BAND
    for name, r in far["fp32_rows"].items():
        assert r["threshold_cap"] == substep.scene_caps(SCENES[name], substep.SUBSTEPS * SCENES[name].N)[1] == 61, (name, r)
        assert r["flag_rows"] == 0 and r["threshold_rows"] <= r["threshold_cap"] // 2, (name, r)


def test_scenes_are_what_the_tier_was_designed_for():
    """One sub-step per step, near scenes on one-tile rasters with coordinates below 8 m, and a slope raster on which every cell lies in
    one plane."""
    import numpy as np
    for scene in SCENES.values():
        cfg, ter = substep.scene_cfg(scene)
        assert cfg.control.decimation == 1 and not cfg.domain_rand.push_robots
        if ter is not None and not scene.far:
            assert ter.heightsamples.shape == (80, 80) and cfg.terrain.horizontal_scale * 80 == 8.0 and cfg.terrain.border_size == 0.0
        if not scene.far:
            assert scene.env_offset == 0 and scene.total_envs is None and scene.tile is None and scene.grid is None
    h = substep.one_tile_scene("slope").heightsamples.astype(np.int64)
    assert (np.diff(h, axis=0) == 2).all() and (np.diff(h, axis=1) == 0).all()
    assert {s.cls for s in SCENES.values()} == set(CLASSES)


def test_far_scenes_are_where_a_real_run_is():
    """The far scenes are what they claim.  Every one of them has its bases at 128-256 m from the origin in x or y over the whole recorded
    trajectory (one binade of fp32 ulp: 2^-16 m); each is its near twin but for where it is (the two 32-DOF scenes also in action scale,
    friction and seed: tests/substep.py says why); the raster scenes are the near 80 x 80 slope raster in tile (9, 19) of the default
    10 x 20 curriculum grid with its 25 m border, a 1300 x 2100 raster that is zero elsewhere, with every env origin at the tile's low
    corner (72, 152) m; the plane scenes are the last 64 envs of a 4096-env grid -- ENV_ORIGINS of plane_far's handle is the tail of a
    4096-env handle's."""
    import dataclasses

    import numpy as np
    import torch
    far = {n: s for n, s in SCENES.items() if s.far}
    assert set(far) == {"plane_far", "plane_t2_far", "base_plane_far", "full_plane_far", "slope_hf_far", "slope_tm_far", "full_slope_tm_far"}
    where = dict(env_offset=0, total_envs=None, tile=None, grid=None)
    for name, scene in far.items():
        traj = substep.oracle_trajectory(name)
        far_axis = traj.pre["ROOT_STATES"][..., :2].abs().amax(-1)              # (T, N): every base, before every sub-step
        assert 128.0 <= float(far_axis.min()) and float(far_axis.max()) < 256.0, (name, float(far_axis.min()), float(far_axis.max()))
        assert 128.0 <= substep.max_xy(traj) < 256.0
        twin = name[:-4]
        if twin in SCENES:
            same = dict(where, name=twin, cls=scene.cls[:-4])
            if scene.task == "GR1T1Full":
                same.update(scales=SCENES[twin].scales, friction=SCENES[twin].friction)
            assert dataclasses.replace(scene, **same) == SCENES[twin], name
        cfg, ter = substep.scene_cfg(scene)
        if scene.ground == "plane":
            assert ter is None and (scene.env_offset, scene.total_envs, scene.N) == (4096 - 64, 4096, 64)
            continue
        assert (scene.tile, scene.grid) == ((9, 19), (10, 20)) and (scene.env_offset, scene.total_envs) == (0, None)
        assert (cfg.terrain.border_size, cfg.terrain.num_rows, cfg.terrain.num_cols, cfg.terrain.horizontal_scale) == (25.0, 10, 20, 0.1)
        hs = ter.heightsamples
        assert hs.shape == (1300, 2100) and hs.dtype == np.int16
        r0, c0 = 250 + 9 * 80, 250 + 19 * 80
        assert (r0 * 0.1 - 25.0, c0 * 0.1 - 25.0) == (72.0, 152.0)
        assert np.array_equal(hs[r0:r0 + 80, c0:c0 + 80], substep.one_tile_scene(scene.ground).heightsamples)
        rest = hs.copy()
        rest[r0:r0 + 80, c0:c0 + 80] = 0
        assert not rest.any()
        assert ter.env_origins.shape == (10, 20, 3) and (ter.env_origins == np.float32([72.0, 152.0, 0.0])).all()
        local = traj.pre["ROOT_STATES"][::substep.REPLACE_EVERY, :, :2] - torch.tensor([72.0, 152.0])     # (an env that resets goes to the corner itself)
        assert local.shape[0] == 2 and 1.0 - 1e-4 <= float(local.min()) and float(local.max()) <= 6.9 + 1e-4, (name, float(local.min()), float(local.max()))
    tail, cfg, _ = substep.make_oracle(SCENES["plane_far"], "f32")
    whole, _, _ = substep.make_oracle(dataclasses.replace(SCENES["plane_far"], N=4096, env_offset=0, total_envs=None), "f32")
    try:
        tail.reset_all(); whole.reset_all()
        org = whole.tensor("ENV_ORIGINS")
        assert org.shape == (4096, 3) and torch.equal(tail.tensor("ENV_ORIGINS"), org[-64:])
        assert float(org[-64:, 0].min()) == float(org[:, 0].max()) == 63 * cfg.env.env_spacing == 189.0 and float(org[-64:, 1].max()) == 189.0
    finally:
        tail.close(); whole.close()
