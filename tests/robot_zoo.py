"""A zoo of small synthetic robots for the tree / generic step kernels and the oracle: invented geometry in the schema of
assets/*.model.json, each as small as the branch of csrc/grx_host_tables.h (build_gen_tables, build_tree_tab, build_refresh_tab) it is
there for allows.  Nothing here reads the library back: EXPECTED_KERNEL is written by hand from the limits of csrc/grx_device.h and
DESIGN.md section 4.3.

  skew        two 3-joint legs; every joint axis oblique (unit length, negative components), every joint frame rotated: no body has
              rot0_identity, chain heads included
  deep9 / 10  one leg whose deepest body sits at depth level 9 / 10 (counted as TreeBody.step counts: a child of the base is level 0 --
              the full-body GR1's hands are at level 9): GRX_TREE_LEVELS = 10 levels hold the first, the second runs generic
  bushy4 / 5  a body with five / six children: one continues its chain, four fill TreeBody.hc[4]; the fifth side chain runs generic
  wide8 / 9 / 16 / 17   that many one-body chains on the base (TreeTab.heads0, nh0): eight fill a lane group; a schedule is built for at
              most GRX_TREE_G = 8 chains whatever the group size, so nine and more run generic with 8 AND with 16 lanes
  comb        a 4-body spine whose first three bodies carry three one-body stubs each -- nine side chains on one chain --, and a 2-body
              second leg: 11 chains, 15 DOFs.  The tree kernel packs a chain's side chains into eight 4-bit slots; 11 chains are beyond
              the eight-chain limit, so the generic kernel runs it and no chain of a model that fits has more than seven side chains
  shapes      base with 5 spheres; a chain body with 5 spheres on two URDF links (work-list chunks 2 + 2 + 1, turns 0..2); a foot with one
              sphere; a foot that is not a leaf; the torso frame on a body deeper than both feet and no forehead (nstep_kin, torso_body
              >= 1); no termination link on the base
  pairs32 / 33 / 64 / 65   that many self-collision sphere pairs: the padding boundaries of TreeTab.nsp_batches (batches of 4 x 8 and
              4 x 16); base x limb pairs; a link pair whose lower URDF link rides on the higher body (a fixed link listed late)
  gr1t2       the shipped full body assets/gr1t2.model.json through GR1T1FullBodyCfg with asset.model = "gr1t2"

(model.fill_model emits sphere pairs sorted by carrying body and matches link pairs by (min, max), so a model file cannot list a pair with the
higher body first: build_gen_tables' `ba > bb` swap is dead code for every config built through model.py.  It is reached through the
C struct instead: the scene pairs65_swapped of tests/substep.py hands every second sphere pair over as (b, a), to the oracle and the kernels alike.)

Every model stays inside the explicit damper's stability ratio GR1T1FullBodyCfg documents -- kd dt / I <= 0.5 about every joint axis, I
taken as the joint's OWN body about the axis through its origin, a lower bound of the subtree's -- (tests/test_robot_zoo.py)."""
import contextlib
import json
import os
import shutil
import tempfile

import numpy as np

from wiki_grx_gym_amd import model as grx_model
from wiki_grx_gym_amd.envs import config

KP, KD = 15.0, 0.3            # N m / rad, N m s / rad of every zoo joint
SIM_DT = 0.002
ZOO = ("skew", "deep9", "deep10", "bushy4", "bushy5", "wide8", "wide9", "wide16", "wide17", "comb", "shapes",
       "pairs32", "pairs33", "pairs64", "pairs65")
SHIPPED = ("gr1t2",)
MODELS = ZOO + SHIPPED
WITH_PAIRS = ("pairs32", "pairs33", "pairs64", "pairs65", "gr1t2")

# the step kernel a handle must report per (model, lanes per env asked for): "tree" = grx_step_tree (8 lanes) / grx_step_tree16 (16),
# "generic" = the one-lane grx_step_generic.  From the limits alone: <= 8 chains (GRX_TREE_G, both group sizes), depth levels 0..9
# (GRX_TREE_LEVELS), <= 4 side chains per body (TreeBody.hc), <= 8 rounds of the contact work list (GRX_TREE_MAXCS), padded sphere
# pairs <= 192 (GRX_MAX_PAIRS).
EXPECTED_KERNEL = {
    "skew": {8: "tree", 16: "tree"},          # 2 chains, 3 levels
    "deep9": {8: "tree", 16: "tree"},         # 2 chains, 10 levels: the last that fits
    "deep10": {8: "generic", 16: "generic"},  # 11 levels
    "bushy4": {8: "tree", 16: "tree"},        # 6 chains, hc[4] full
    "bushy5": {8: "generic", 16: "generic"},  # a fifth side chain on one body
    "wide8": {8: "tree", 16: "tree"},         # 8 chains: a full group of 8
    "wide9": {8: "generic", 16: "generic"},   # 9 chains
    "wide16": {8: "generic", 16: "generic"},
    "wide17": {8: "generic", 16: "generic"},
    "comb": {8: "generic", 16: "generic"},    # 11 chains
    "shapes": {8: "tree", 16: "tree"},        # 3 chains, 4 levels
    "pairs32": {8: "tree", 16: "tree"},       # 3 chains; 32 / 64 padded pairs
    "pairs33": {8: "tree", 16: "tree"},       # 64 / 64
    "pairs64": {8: "tree", 16: "tree"},       # 64 / 64
    "pairs65": {8: "tree", 16: "tree"},       # 96 / 128
    "gr1t2": {8: "tree", 16: "tree"},         # 5 chains, 10 levels, 126 sphere pairs -> 128 / 128
}

# SENS_K x the largest |fp32 oracle - fp64 oracle| over the band class's scenes (tests/substep.ZOO_SCENES; profiles/zoo_bands.json holds the
# maxima per scene; tests/test_robot_zoo.py measures them again and holds this table to them).  python -m tests.robot_zoo prints it.
ZOO_BAND = {
    "skew": {"DOF_POS": 7.6e-05, "DOF_VEL": 0.038, "ROOT_STATES": 0.0024, "TORQUES": 3.9e-05, "BASE_LIN_VEL": 0.00016, "BASE_ANG_VEL": 0.0025, "PROJECTED_GRAVITY": 4.9e-06, "FEET_POS": 3.9e-05, "FEET_CONTACT_FORCE": 1.2, "CONTACT_FORCES": 1.2, "AVG_FEET_FORCE": 0.39, "AVG_FEET_SPEED": 0.0015, "REW": 0.00021, "ANCHORS": 3.9e-05, "ANCHOR_SPEED": 9.6e-06},
    "deep9": {"DOF_POS": 6.4e-05, "DOF_VEL": 0.032, "ROOT_STATES": 0.00058, "TORQUES": 3.9e-05, "BASE_LIN_VEL": 6.1e-05, "BASE_ANG_VEL": 0.00055, "PROJECTED_GRAVITY": 4.2e-06, "FEET_POS": 7.7e-05, "FEET_CONTACT_FORCE": 1.7, "CONTACT_FORCES": 1.7, "AVG_FEET_FORCE": 0.79, "AVG_FEET_SPEED": 0.0024, "REW": 0.00041, "ANCHORS": 7.7e-05, "ANCHOR_SPEED": 1.5e-05},
    "deep10": {"DOF_POS": 0.00019, "DOF_VEL": 0.094, "ROOT_STATES": 0.00066, "TORQUES": 3.9e-05, "BASE_LIN_VEL": 6e-05, "BASE_ANG_VEL": 0.00065, "PROJECTED_GRAVITY": 4.2e-06, "FEET_POS": 7.7e-05, "FEET_CONTACT_FORCE": 2.6, "CONTACT_FORCES": 2.6, "AVG_FEET_FORCE": 0.86, "AVG_FEET_SPEED": 0.0032, "REW": 0.00025, "ANCHORS": 7.7e-05, "ANCHOR_SPEED": 1.2e-05},
    "bushy4": {"DOF_POS": 2.8e-05, "DOF_VEL": 0.014, "ROOT_STATES": 0.0025, "TORQUES": 3.9e-05, "BASE_LIN_VEL": 0.00018, "BASE_ANG_VEL": 0.0029, "PROJECTED_GRAVITY": 6e-06, "FEET_POS": 3.9e-05, "FEET_CONTACT_FORCE": 1.5, "CONTACT_FORCES": 1.5, "AVG_FEET_FORCE": 0.67, "AVG_FEET_SPEED": 0.0024, "REW": 5e-05, "ANCHORS": 3.9e-05, "ANCHOR_SPEED": 9.6e-06},
    "bushy5": {"DOF_POS": 3.1e-05, "DOF_VEL": 0.016, "ROOT_STATES": 0.0025, "TORQUES": 3.9e-05, "BASE_LIN_VEL": 0.00014, "BASE_ANG_VEL": 0.0026, "PROJECTED_GRAVITY": 5e-06, "FEET_POS": 3.9e-05, "FEET_CONTACT_FORCE": 1.8, "CONTACT_FORCES": 1.8, "AVG_FEET_FORCE": 0.44, "AVG_FEET_SPEED": 0.0025, "REW": 3.1e-05, "ANCHORS": 3.9e-05, "ANCHOR_SPEED": 7.2e-06},
    "wide8": {"DOF_POS": 4e-05, "DOF_VEL": 0.02, "ROOT_STATES": 0.0012, "TORQUES": 3.9e-05, "BASE_LIN_VEL": 0.00012, "BASE_ANG_VEL": 0.00099, "PROJECTED_GRAVITY": 4.2e-06, "FEET_POS": 2e-05, "FEET_CONTACT_FORCE": 0.49, "CONTACT_FORCES": 0.49, "AVG_FEET_FORCE": 0.25, "AVG_FEET_SPEED": 0.00022, "REW": 4.8e-06, "ANCHORS": 2e-05, "ANCHOR_SPEED": 7.2e-06},
    "wide9": {"DOF_POS": 4.3e-05, "DOF_VEL": 0.022, "ROOT_STATES": 0.0012, "TORQUES": 3.9e-05, "BASE_LIN_VEL": 0.00011, "BASE_ANG_VEL": 0.0012, "PROJECTED_GRAVITY": 4.2e-06, "FEET_POS": 2e-05, "FEET_CONTACT_FORCE": 0.53, "CONTACT_FORCES": 0.53, "AVG_FEET_FORCE": 0.2, "AVG_FEET_SPEED": 0.00029, "REW": 6.8e-06, "ANCHORS": 2e-05, "ANCHOR_SPEED": 4.8e-06},
    "wide16": {"DOF_POS": 3e-05, "DOF_VEL": 0.015, "ROOT_STATES": 0.00043, "TORQUES": 3.9e-05, "BASE_LIN_VEL": 5e-05, "BASE_ANG_VEL": 0.00044, "PROJECTED_GRAVITY": 4.2e-06, "FEET_POS": 2e-05, "FEET_CONTACT_FORCE": 0.42, "CONTACT_FORCES": 0.42, "AVG_FEET_FORCE": 0.14, "AVG_FEET_SPEED": 0.00011, "REW": 1.9e-06, "ANCHORS": 2e-05, "ANCHOR_SPEED": 4.8e-06},
    "wide17": {"DOF_POS": 3.3e-05, "DOF_VEL": 0.017, "ROOT_STATES": 0.00069, "TORQUES": 3.9e-05, "BASE_LIN_VEL": 9.1e-05, "BASE_ANG_VEL": 0.00071, "PROJECTED_GRAVITY": 4.2e-06, "FEET_POS": 2e-05, "FEET_CONTACT_FORCE": 0.52, "CONTACT_FORCES": 0.52, "AVG_FEET_FORCE": 0.24, "AVG_FEET_SPEED": 0.0002, "REW": 2.2e-06, "ANCHORS": 2e-05, "ANCHOR_SPEED": 4.8e-06},
    "comb": {"DOF_POS": 5.1e-05, "DOF_VEL": 0.026, "ROOT_STATES": 0.0022, "TORQUES": 3.9e-05, "BASE_LIN_VEL": 0.00017, "BASE_ANG_VEL": 0.0024, "PROJECTED_GRAVITY": 5.2e-06, "FEET_POS": 3.9e-05, "FEET_CONTACT_FORCE": 1.6, "CONTACT_FORCES": 1.6, "AVG_FEET_FORCE": 0.51, "AVG_FEET_SPEED": 0.0023, "REW": 2e-05, "ANCHORS": 3.9e-05, "ANCHOR_SPEED": 7.2e-06},
    "shapes": {"DOF_POS": 3.7e-05, "DOF_VEL": 0.019, "ROOT_STATES": 0.003, "TORQUES": 3.9e-05, "BASE_LIN_VEL": 0.00024, "BASE_ANG_VEL": 0.0028, "PROJECTED_GRAVITY": 4.2e-06, "FEET_POS": 2e-05, "FEET_CONTACT_FORCE": 0.68, "CONTACT_FORCES": 0.68, "AVG_FEET_FORCE": 0.28, "AVG_FEET_SPEED": 0.00053, "REW": 2e-05, "ANCHORS": 3.9e-05, "ANCHOR_SPEED": 2e-05},
    "pairs32": {"DOF_POS": 4.4e-05, "DOF_VEL": 0.022, "ROOT_STATES": 0.005, "TORQUES": 3.9e-05, "BASE_LIN_VEL": 0.00033, "BASE_ANG_VEL": 0.0055, "PROJECTED_GRAVITY": 1.1e-05, "FEET_POS": 2e-05, "FEET_CONTACT_FORCE": 1.0, "CONTACT_FORCES": 2.9, "AVG_FEET_FORCE": 0.31, "AVG_FEET_SPEED": 0.0028, "REW": 5.3e-05, "ANCHORS": 3.9e-05, "ANCHOR_SPEED": 2e-05},
    "pairs33": {"DOF_POS": 2.7e-05, "DOF_VEL": 0.014, "ROOT_STATES": 0.0058, "TORQUES": 3.9e-05, "BASE_LIN_VEL": 0.00025, "BASE_ANG_VEL": 0.0061, "PROJECTED_GRAVITY": 1.2e-05, "FEET_POS": 2e-05, "FEET_CONTACT_FORCE": 1.1, "CONTACT_FORCES": 1.8, "AVG_FEET_FORCE": 0.31, "AVG_FEET_SPEED": 0.0018, "REW": 6.2e-05, "ANCHORS": 3.9e-05, "ANCHOR_SPEED": 2e-05},
    "pairs64": {"DOF_POS": 0.00014, "DOF_VEL": 0.067, "ROOT_STATES": 0.0032, "TORQUES": 3.9e-05, "BASE_LIN_VEL": 0.00025, "BASE_ANG_VEL": 0.0038, "PROJECTED_GRAVITY": 7.4e-06, "FEET_POS": 2e-05, "FEET_CONTACT_FORCE": 2.9, "CONTACT_FORCES": 2.9, "AVG_FEET_FORCE": 2.8, "AVG_FEET_SPEED": 0.0029, "REW": 0.00013, "ANCHORS": 3.9e-05, "ANCHOR_SPEED": 2e-05},
    "pairs65": {"DOF_POS": 0.00014, "DOF_VEL": 0.067, "ROOT_STATES": 0.0058, "TORQUES": 3.9e-05, "BASE_LIN_VEL": 0.00037, "BASE_ANG_VEL": 0.0058, "PROJECTED_GRAVITY": 1.2e-05, "FEET_POS": 2e-05, "FEET_CONTACT_FORCE": 2.9, "CONTACT_FORCES": 2.9, "AVG_FEET_FORCE": 2.8, "AVG_FEET_SPEED": 0.0029, "REW": 0.00022, "ANCHORS": 3.9e-05, "ANCHOR_SPEED": 2e-05},
    "gr1t2": {"DOF_POS": 0.0001, "DOF_VEL": 0.05, "ROOT_STATES": 0.00024, "TORQUES": 0.00062, "BASE_LIN_VEL": 4.8e-05, "BASE_ANG_VEL": 0.00031, "PROJECTED_GRAVITY": 4.2e-06, "FEET_POS": 3.9e-05, "FEET_CONTACT_FORCE": 2.1, "CONTACT_FORCES": 2.1, "AVG_FEET_FORCE": 0.74, "AVG_FEET_SPEED": 0.0013, "REW": 6.4e-05, "ANCHORS": 5.8e-05, "ANCHOR_SPEED": 1.5e-05},
    "skew_stairs": {"DOF_POS": 7e-05, "DOF_VEL": 0.035, "ROOT_STATES": 0.0014, "TORQUES": 3.9e-05, "BASE_LIN_VEL": 0.00013, "BASE_ANG_VEL": 0.0013, "PROJECTED_GRAVITY": 4.2e-06, "FEET_POS": 9.6e-06, "FEET_CONTACT_FORCE": 1.2, "CONTACT_FORCES": 1.2, "AVG_FEET_FORCE": 1.3, "AVG_FEET_SPEED": 0.0014, "REW": 4.8e-05, "ANCHORS": 9.6e-06, "ANCHOR_SPEED": 9.6e-06},
}


# ---------------------------------------------------------------------------------------------------------------- model files
def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return [float(x) for x in v / np.linalg.norm(v)]


def _link(name, parent, xyz=(0, 0, 0), rpy=(0, 0, 0), axis=(0, 1, 0), mass=1.0, com=(0.0, 0.0, -0.04), spheres=(), joint="revolute",
          limit=(-0.8, 0.8)):
    """One URDF link with the joint that carries it.  Inertia about the COM: 0.004 / 0.005 / 0.003 kg m^2 per kg with small products
    (positive definite; about any axis >= 0.0029 kg m^2 per kg, so kd dt / I <= 0.42 for 0.5 kg)."""
    L = {"name": name, "mass": float(mass), "com": [float(x) for x in com], "com_rpy": [0.0, 0.0, 0.0],
         "inertia": [0.004 * mass, 1e-4 * mass, -5e-5 * mass, 0.005 * mass, 8e-5 * mass, 0.003 * mass],
         "collisions": [{"type": "sphere", "xyz": [float(x) for x in p], "rpy": [0.0, 0.0, 0.0], "radius": float(r)} for p, r in spheres],
         "parent": parent, "joint_name": None if parent < 0 else name.replace("_link", "") + ("_fixed" if joint == "fixed" else "_joint"),
         "joint_type": "floating" if parent < 0 else joint, "origin_xyz": [float(x) for x in xyz], "origin_rpy": [float(x) for x in rpy],
         "axis": _unit(axis) if joint == "revolute" else [0.0, 0.0, 0.0]}
    if joint == "revolute":
        L["limit"] = {"lower": float(limit[0]), "upper": float(limit[1]), "effort": 20.0, "velocity": 12.0}
    return L


def _finish(key, links, pairs=()):
    return {"robot": "zoo_" + key, "source": "tests/robot_zoo.py (synthetic)", "num_bodies": len(links),
            "num_dofs": sum(L["joint_type"] == "revolute" for L in links), "body_names": [L["name"] for L in links],
            "dof_names": [L["joint_name"] for L in links if L["joint_type"] == "revolute"], "links": links,
            "self_collision_link_pairs": [list(p) for p in pairs]}


FOOT4 = (((0.05, 0.03, -0.05), 0.025), ((0.05, -0.03, -0.05), 0.025), ((-0.04, 0.03, -0.05), 0.025), ((-0.04, -0.03, -0.05), 0.025))
TRUNK = _link("trunk_link", -1, mass=5.0, com=(0.0, 0.0, 0.02), spheres=(((0.0, 0.0, 0.0), 0.09),))
AXES = ((1, 0, 0), (0, 0, 1), (0, 1, 0))


def skew():
    links = [dict(TRUNK)]
    axes = ((1, -2, 2), (-2, 1, 2), (2, 3, -6))
    rpys = ((0.3, -0.2, 0.4), (-0.25, 0.35, -0.3), (0.2, 0.3, -0.45))
    for side, y in (("left", 0.1), ("right", -0.1)):
        s = 1.0 if side == "left" else -1.0
        p = 0
        for k, nm in enumerate(("hip", "shin", "foot")):
            links.append(_link(f"{side}_{nm}_link", p, xyz=(0.0, y, -0.05) if k == 0 else (0.01, 0.0, -0.14), rpy=tuple(s * a for a in rpys[k]),
                               axis=tuple(a * (s if i == 1 else 1.0) for i, a in enumerate(axes[k])), mass=(1.5, 1.0, 0.6)[k],
                               spheres=FOOT4 if nm == "foot" else (((0.0, 0.0, -0.07), 0.04),)))
            p = len(links) - 1
    return _finish("skew", links)


def deep(levels):
    """Left leg: a chain whose last body sits at depth level `levels` (levels + 1 bodies); right leg: two bodies."""
    links = [dict(TRUNK)]
    p = 0
    for k in range(levels + 1):
        last = k == levels
        links.append(_link("left_foot_link" if last else f"left_seg{k}_link", p, xyz=(0.0, 0.1, -0.05) if k == 0 else (0.0, 0.0, -0.07),
                           axis=AXES[k % 3], mass=0.6, com=(0.0, 0.0, -0.03), limit=(-0.5, 0.5),
                           spheres=FOOT4[:2] if last else (((0.0, 0.0, -0.035), 0.03),) if k % 2 else ()))
        p = len(links) - 1
    links.append(_link("right_hip_link", 0, xyz=(0.0, -0.1, -0.05), axis=(1, 0, 0), mass=1.5, spheres=(((0.0, 0.0, -0.07), 0.04),)))
    links.append(_link("right_foot_link", len(links) - 1, xyz=(0.0, 0.0, -0.14), axis=(0, 1, 0), mass=0.8, spheres=FOOT4))
    return _finish(f"deep{levels}", links)


def bushy(side_chains):
    """left_hip carries 1 + side_chains children: left_shin continues its chain, every stub starts one."""
    links = [dict(TRUNK)]
    links.append(_link("left_hip_link", 0, xyz=(0.0, 0.1, -0.05), axis=(1, 0, 0), mass=2.0, spheres=(((0.0, 0.0, -0.06), 0.04),)))
    hip = 1
    links.append(_link("left_shin_link", hip, xyz=(0.0, 0.0, -0.14), axis=(0, 1, 0), mass=1.0, spheres=(((0.0, 0.0, -0.07), 0.035),)))
    for k in range(side_chains):
        ang = 2 * np.pi * k / side_chains
        links.append(_link(f"stub{k}_link", hip, xyz=(0.07 * np.cos(ang), 0.07 * np.sin(ang) + 0.02, -0.03), rpy=(0.0, 0.0, ang), axis=AXES[k % 3],
                           mass=0.5, com=(0.03, 0.0, 0.0), spheres=(((0.05, 0.0, 0.0), 0.025),)))
    links.append(_link("left_foot_link", 2, xyz=(0.0, 0.0, -0.14), axis=(0, 1, 0), mass=0.6, spheres=FOOT4))
    links.append(_link("right_hip_link", 0, xyz=(0.0, -0.1, -0.05), axis=(1, 0, 0), mass=2.0, spheres=(((0.0, 0.0, -0.06), 0.04),)))
    links.append(_link("right_foot_link", len(links) - 1, xyz=(0.0, 0.0, -0.28), axis=(0, 1, 0), mass=0.8, spheres=FOOT4))
    return _finish(f"bushy{side_chains}", links)


def wide(chains):
    """`chains` one-body chains on the base, round a circle; the first two are the feet."""
    links = [dict(TRUNK)]
    for k in range(chains):
        ang = 2 * np.pi * k / chains
        name = ("left_foot_link", "right_foot_link")[k] if k < 2 else f"spoke{k}_link"
        links.append(_link(name, 0, xyz=(0.13 * np.cos(ang), 0.13 * np.sin(ang), -0.04), rpy=(0.0, 0.0, ang), axis=AXES[k % 3], mass=0.5 + 0.1 * (k % 4),
                           com=(0.02, 0.0, -0.03), spheres=FOOT4[:2 + k % 3] if k < 2 else (((0.03, 0.0, -0.06), 0.03),)))
    return _finish(f"wide{chains}", links)


def comb():
    links = [dict(TRUNK)]
    spine = []
    p = 0
    for k in range(4):     # the spine first: a body's first child continues its chain
        links.append(_link("left_foot_link" if k == 3 else f"spine{k}_link", p, xyz=(0.0, 0.1, -0.05) if k == 0 else (0.0, 0.0, -0.12), axis=AXES[(k + 1) % 3],
                           mass=1.2, spheres=FOOT4 if k == 3 else (((0.0, 0.0, -0.06), 0.035),)))
        p = len(links) - 1
        spine.append(p)
    for k in range(3):
        for t in range(3):
            ang = 2 * np.pi * t / 3 + 0.4 * k
            links.append(_link(f"tooth{k}{t}_link", spine[k], xyz=(0.06 * np.cos(ang), 0.06 * np.sin(ang), -0.05), rpy=(0.0, 0.0, ang), axis=AXES[t],
                               mass=0.5, com=(0.03, 0.0, 0.0), spheres=(((0.05, 0.0, 0.0), 0.025),) if t == 0 else ()))
    links.append(_link("right_hip_link", 0, xyz=(0.0, -0.1, -0.05), axis=(1, 0, 0), mass=2.0, spheres=(((0.0, 0.0, -0.06), 0.04),)))
    links.append(_link("right_foot_link", len(links) - 1, xyz=(0.0, 0.0, -0.36), axis=(0, 1, 0), mass=0.8, spheres=FOOT4))
    return _finish("comb", links)


def shapes():
    base = _link("trunk_link", -1, mass=5.0, com=(0.0, 0.0, 0.02),
                 spheres=(((0.06, 0.05, 0.0), 0.06), ((0.06, -0.05, 0.0), 0.06), ((-0.06, 0.05, 0.0), 0.06), ((-0.06, -0.05, 0.0), 0.06), ((0.0, 0.0, 0.07), 0.05)))
    links = [base]
    links.append(_link("left_thigh_link", 0, xyz=(0.0, 0.1, -0.05), axis=(1, 0, 0), mass=2.0,
                       spheres=(((0.0, 0.0, -0.03), 0.035), ((0.0, 0.0, -0.08), 0.035), ((0.0, 0.0, -0.13), 0.035))))          # 1
    links.append(_link("left_guard_link", 1, xyz=(0.03, 0.0, -0.06), joint="fixed", mass=0.3, com=(0.0, 0.0, 0.0),
                       spheres=(((0.02, 0.0, 0.03), 0.025), ((0.02, 0.0, -0.03), 0.025))))                                       # 2: rides on the thigh
    links.append(_link("left_foot_link", 1, xyz=(0.0, 0.0, -0.18), axis=(0, 1, 0), mass=0.8, spheres=(((0.0, 0.0, -0.04), 0.04),)))   # 3: one sphere, not a leaf
    links.append(_link("left_toe_link", 3, xyz=(0.07, 0.0, -0.03), axis=(0, 1, 0), mass=0.5, com=(0.03, 0.0, 0.0), spheres=(((0.04, 0.0, -0.01), 0.025),)))   # 4
    links.append(_link("right_foot_link", 0, xyz=(0.0, -0.1, -0.05), axis=(1, 0, 0), mass=1.5, com=(0.0, 0.0, -0.1),
                       spheres=tuple(((x, y, -0.25), 0.025) for x in (0.05, -0.04) for y in (0.03, -0.03))))                   # 5: a foot at level 0
    p = 0
    for k in range(4):                                                                                                          # 6..9: the torso frame at level 3
        links.append(_link("torso_link" if k == 3 else f"neck{k}_link", p, xyz=(0.0, 0.0, 0.08) if k == 0 else (0.0, 0.0, 0.07), rpy=(0.0, 0.0, 0.3) if k == 3 else (0, 0, 0),
                           axis=AXES[k % 3], mass=0.6, com=(0.0, 0.0, 0.03), limit=(-0.6, 0.6), spheres=(((0.0, 0.0, 0.04), 0.04),) if k == 3 else ()))
        p = len(links) - 1
    return _finish("shapes", links)


def pairs(count):
    """32 = trunk x forearm (4 x 4 spheres: base x limb) + thigh x thigh (4 x 4); 64 = those + foot x foot + left thigh x right foot; + 1 = the
    two one-sphere guards on the thighs' inner sides, fixed links listed last and right before left: the lower URDF link of that pair rides on
    the higher body, and the pair is the 33rd of the 33 in table order."""
    col = lambda dx, dz, r: tuple(((dx * i, 0.0, dz * i), r) for i in range(1, 5))
    trunk = _link("trunk_link", -1, mass=5.0, com=(0.0, 0.0, 0.02), spheres=tuple(((x, y, -0.02), 0.07) for x in (0.05, -0.05) for y in (0.05, -0.05)))
    links = [trunk]
    for side, y in (("left", 0.08), ("right", -0.08)):
        links.append(_link(f"{side}_thigh_link", 0, xyz=(0.0, y, -0.1), axis=(1, 0, 0), mass=2.0, com=(0.0, 0.0, -0.1), limit=(-0.9, 0.9), spheres=col(0.0, -0.045, 0.04)))
        links.append(_link(f"{side}_foot_link", len(links) - 1, xyz=(0.0, 0.0, -0.24), axis=(0, 1, 0), mass=0.8, limit=(-1.2, 0.4), spheres=FOOT4))
    links.append(_link("arm_link", 0, xyz=(0.08, 0.0, 0.05), axis=(0, 1, 0), mass=0.8, com=(0.05, 0.0, 0.0), limit=(-0.4, 0.4)))                                # 5
    links.append(_link("forearm_link", 5, xyz=(0.14, 0.0, 0.0), axis=(0, 0, 1), mass=0.6, com=(0.06, 0.0, 0.0), limit=(-2.8, 2.8), spheres=col(0.04, 0.0, 0.03)))   # 6
    links.append(_link("right_guard_link", 3, xyz=(0.0, 0.04, -0.1), joint="fixed", mass=0.2, com=(0.0, 0.0, 0.0), spheres=(((0.0, 0.0, 0.0), 0.03),)))          # 7
    links.append(_link("left_guard_link", 1, xyz=(0.0, -0.04, -0.1), joint="fixed", mass=0.2, com=(0.0, 0.0, 0.0), spheres=(((0.0, 0.0, 0.0), 0.03),)))          # 8
    table = {32: [(0, 6), (1, 3)], 64: [(0, 6), (1, 3), (2, 4), (1, 4)]}
    table[33], table[65] = table[32] + [(7, 8)], table[64] + [(7, 8)]
    return _finish(f"pairs{count}", links, table[count])


BUILDERS = {"skew": skew, "deep9": lambda: deep(9), "deep10": lambda: deep(10), "bushy4": lambda: bushy(4), "bushy5": lambda: bushy(5),
            "wide8": lambda: wide(8), "wide9": lambda: wide(9), "wide16": lambda: wide(16), "wide17": lambda: wide(17), "comb": comb, "shapes": shapes,
            "pairs32": lambda: pairs(32), "pairs33": lambda: pairs(33), "pairs64": lambda: pairs(64), "pairs65": lambda: pairs(65)}
# what the env pipeline is told about a model: (torso_name, terminate_after_contacts_on)
FRAMES = {k: ("trunk", ["trunk"]) for k in ZOO}
FRAMES["shapes"] = ("torso", ["torso"])


def over_limit(kind):
    """Models beyond a hard limit of include/grx.h: 33 DOFs (GRX_MAX_DOFS 32), 49 spheres (GRX_MAX_SPHERES 48)."""
    if kind == "dofs":
        return wide(33)
    raw = wide(8)
    rest = sum(len(L["collisions"]) for L in raw["links"][1:])
    raw["links"][0]["collisions"] = [{"type": "sphere", "xyz": [0.01 * i, 0.0, 0.0], "rpy": [0.0, 0.0, 0.0], "radius": 0.02} for i in range(49 - rest)]
    return raw


# ---------------------------------------------------------------------------------------------------------------- install, config
_dir = [None]


def asset_dir():
    """A temporary directory with every zoo model and the shipped ones next to them (written once per process)."""
    if _dir[0] is None:
        import atexit
        d = tempfile.mkdtemp(prefix="robot_zoo_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        shipped = os.path.join(os.path.dirname(os.path.abspath(grx_model.__file__)), "assets")
        for f in os.listdir(shipped):
            shutil.copy(os.path.join(shipped, f), d)
        for key, fn in BUILDERS.items():
            write(d, key, fn())
        _dir[0] = d
    return _dir[0]


def write(d, key, raw):
    with open(os.path.join(d, key + ".model.json"), "w") as f:
        json.dump(raw, f)


def install(monkeypatch):
    """Point wiki_grx_gym_amd.model.ASSET_DIR at the zoo for the running test; returns the directory."""
    d = asset_dir()
    monkeypatch.setattr(grx_model, "ASSET_DIR", d)
    return d


@contextlib.contextmanager
def installed():
    """install() outside a test (python -m tests.robot_zoo): ASSET_DIR points at the zoo inside the block."""
    keep, grx_model.ASSET_DIR = grx_model.ASSET_DIR, asset_dir()
    try:
        yield grx_model.ASSET_DIR
    finally:
        grx_model.ASSET_DIR = keep


def rest_height(key):
    """Height of the base origin with the lowest collision sphere on the plane: default pose, base upright."""
    import torch
    from tests.kinematics_ref import BodyKinematics
    rm = grx_model.RobotModel(key, asset_dir=asset_dir())
    root = torch.zeros(1, 13)
    root[0, 6] = 1.0
    return -lowest_point(rm, BodyKinematics(rm, "cpu"), root, torch.zeros(1, rm.num_dofs))[0].item()


def lowest_point(rm, kin, root, q):
    """(N,) world z of the lowest point of any collision sphere."""
    import torch
    R, p, _, _ = kin.body_frames(root, q, torch.zeros_like(q))
    z = [p[:, b, 2] + (R[:, b] @ torch.as_tensor(pos, dtype=torch.float32))[:, 2] - float(r) for b, pos, r, _ in rm.spheres]
    return torch.stack(z, 1).amin(1)


DROP = 0.2                    # [m] a reset leaves the lowest sphere this far above the plane

_cfg_classes = {}


def cfg_class(key):
    """GR1T1FullBodyCfg for a zoo model: asset.model, action / observation sizes, gains and default angles by name, clip ranges of length nd,
    two feet, torso and termination names that exist, no forehead, no armature."""
    if key in _cfg_classes:
        return _cfg_classes[key]
    B = config.GR1T1FullBodyCfg
    if key in SHIPPED:
        cls = type("Zoo_" + key, (B,), {"asset": config.section("asset", B.asset, model=key)})
    else:
        raw = BUILDERS[key]()
        rev = [L for L in raw["links"] if L["joint_type"] == "revolute"]
        nd = len(rev)
        lo, hi = np.array([L["limit"]["lower"] for L in rev]), np.array([L["limit"]["upper"] for L in rev])
        span = hi - lo
        torso, term = FRAMES[key]
        cls = type("Zoo_" + key, (B,), {
            "env": config.section("env", B.env, num_actions=nd, num_obs=9 + 3 * nd, num_pri_obs=9 + 3 * nd + 8 + 121),
            "asset": config.section("asset", B.asset, model=key, foot_name="foot", torso_name=torso, forehead_name="", terminate_after_contacts_on=list(term),
                                    penalize_contacts_on=[], armature=0.0),
            "init_state": config.section("init_state", B.init_state, pos=[0.0, 0.0, round(rest_height(key) + DROP, 3)], default_joint_angles={n: 0.0 for n in raw["dof_names"]}),
            "control": config.section("control", B.control, stiffness={"_joint": KP}, damping={"_joint": KD}),
            "normalization": config.section("normalization", B.normalization, actions_max=hi, actions_min=lo, clip_actions_max=hi + span,
                                            clip_actions_min=lo - span)})   # (targets beyond the limits: random actions press the joints into them)
    _cfg_classes[key] = cls
    return cls


if __name__ == "__main__":      # python -m tests.robot_zoo: measure the bands, write profiles/zoo_bands.json, print ZOO_BAND
    from tests import substep
    with installed():
        substep.write_zoo_bands()
