"""The sub-step tier's own footing, on the CPU (tests/substep.py): SUBSTEP_BAND is SENS_K x what the fp32 oracle shows against the fp64
oracle over exactly the trajectories the GPU tests replay (tests/test_substep_parity_gpu.py), each scene reaches the contact regimes it is
there for, and the fp32 oracle itself meets the conditions the kernels are held to, with room to spare."""
import json
import os

import pytest

from tests import substep
from tests.substep import MIN_REGIME, SCENES, SENS_K, SUBSTEP_BAND

ALLOW = 1.25       # the fp32 oracle may sit this far beyond SUBSTEP_BAND / SENS_K (another libm, another compiler) before the table is stale
CLASSES = ("plane", "raster", "full")


@pytest.mark.parametrize("cls", CLASSES)
def test_the_band_is_the_fp32_oracles_own_error(cls):
    """Per scene of the class: (1) the fp32 oracle stays inside SUBSTEP_BAND / SENS_K x 1.25 -- a later change of the oracle cannot
    silently loosen the table --, (2) every regime counter the scene is meant to reach is >= 100 env-sub-steps, (3) the conditions of
    substep.check hold for the fp32 oracle with room to spare: no row out of band or with a differing discrete output (stairs: at most
    one of the three), contact thresholds falling the other way in at most three quarters of the allowed rows (observed: at most 5 of the
    7 that 2e-4 of 38 400 env-sub-steps allow).  Over the class: the table is not looser than its measurement either (its largest entry
    is reached to 1 / 1.25)."""
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
        for n in scene.banded:
            out |= cmp["err"][n] > band[n]
        bad_cap, threshold_cap = substep.scene_caps(scene, traj.rows)
        if int(out.sum()) > bad_cap // 3:
            problems.append(f"{name}: {int(out.sum())} rows of the fp32 oracle out of band or with a differing discrete output")
        if int(cmp["thresholds"].sum()) > 3 * threshold_cap // 4:
            problems.append(f"{name}: {int(cmp['thresholds'].sum())} rows of the fp32 oracle with a contact threshold the other way (3 / 4 of the cap: {3 * threshold_cap // 4})")
    for n, v in top.items():
        if v * SENS_K * ALLOW < band[n]:
            problems.append(f"{cls}: SUBSTEP_BAND[{n}] = {band[n]:.3e} is looser than SENS_K x the measured {v:.3e}")
    assert not problems, "\n".join(problems)


def test_the_recorded_maxima_give_the_committed_band():
    """profiles/substep_bands.json (python -m tests.substep) is what SUBSTEP_BAND was taken from."""
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "substep_bands.json")) as f:
        rec = json.load(f)
    assert rec["sens_k"] == SENS_K and set(rec["maxima"]) == set(SCENES)
    assert substep.band_from(rec["maxima"]) == SUBSTEP_BAND == rec["band"]


def test_scenes_are_what_the_tier_was_designed_for():
    """One sub-step per step, one-tile rasters with coordinates below 8 m, and a slope raster on which every cell lies in one plane."""
    import numpy as np
    for scene in SCENES.values():
        cfg, ter = substep.scene_cfg(scene)
        assert cfg.control.decimation == 1 and not cfg.domain_rand.push_robots
        if ter is not None:
            assert ter.heightsamples.shape == (80, 80) and cfg.terrain.horizontal_scale * 80 == 8.0 and cfg.terrain.border_size == 0.0
    h = substep.one_tile_scene("slope").heightsamples.astype(np.int64)
    assert (np.diff(h, axis=0) == 2).all() and (np.diff(h, axis=1) == 0).all()
    assert {s.cls for s in SCENES.values()} == set(CLASSES)
