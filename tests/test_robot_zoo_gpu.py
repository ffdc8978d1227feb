"""The tree kernels (8 and 16 lanes per env), the one-lane generic kernel and grx_refresh on robots other than the GR1: every model of
tests/robot_zoo.py through every kernel against the fp64 oracle ONE physics sub-step at a time (tests/substep.py), 64 envs, 600 sub-steps.
Per model: dropped from 0.1-0.3 m onto the plane with the registered domain randomisation and random actions (first touch, slip, bounce,
joint limits, resets and time-outs); in flight with the joints over 90 % of their ranges where the model has self-collision pairs (pairs65 a
second time with every second sphere pair listed higher body first: build_gen_tables' swap); the stairs tile for skew.  A case asserts
  * the kernel the handle reports against robot_zoo.EXPECTED_KERNEL: a fallback must be the one the limits predict, a fit must run the
    tree kernel;
  * substep.check as it is: every banded tensor inside ZOO_BAND -- SENS_K x the fp32 oracle's own error on the same trajectory
    (tests/test_robot_zoo.py holds the table to it) --, the discrete outputs identical, threshold rows within THRESHOLD_FRAC;
  * where a tree kernel runs: GRX_T_RIGID_BODY_STATES after the last sub-step, both as grx_refresh materialises it and as the step
    kernel writes it (a second handle that publishes every step, through the last sub-step only), against tests/kinematics_ref.py on the
    published state at the 2e-5 / 2e-4 of tests/test_generic_gpu.py.  (The generic kernel publishes no link frames.)
The observed maxima and their ratio to the fp32 oracle's are appended to the jsonl file GRX_ZOO_LOG names, if set (profiles/zoo_hip.jsonl
holds an MI355X's)."""
import os

import pytest
import torch

from tests import robot_zoo, substep
from tests.helpers import STATE_TENSORS
from tests.kinematics_ref import BodyKinematics
from tests.test_generic_gpu import pick
from tests.test_kinematics import rbs_err

pytestmark = pytest.mark.gpu

LOG = os.environ.get("GRX_ZOO_LOG")
KERNELS = ("tree", "tree16", "generic")
CASES = [(name, k) for name in substep.ZOO_SCENES for k in KERNELS]     # (the layouts of a scene sit next to each other: one oracle trajectory)
ASKED = {"tree": 8, "tree16": 16}


def expected(scene, kernel):
    """(kernel name up to its template arguments, lanes per env) the handle must report."""
    head = "_trimesh" if scene.mesh == "trimesh" else ""
    if kernel == "generic" or robot_zoo.EXPECTED_KERNEL[scene.model][ASKED[kernel]] == "generic":
        return "grx_step_generic" + head, 1
    return ("grx_step_tree" + head, 8) if kernel == "tree" else ("grx_step_tree16" + head, 16)


def link_frames_match(hip, rm, what):
    """RIGID_BODY_STATES of a handle against the link frames of the state it publishes, envs that did not reset in the step."""
    live = ~hip.tensor("RESET").cpu().bool()
    got = hip.tensor("RIGID_BODY_STATES").cpu()
    own = BodyKinematics(rm, "cpu").rigid_body_states(hip.tensor("ROOT_STATES").cpu(), hip.tensor("DOF_POS").cpu(), hip.tensor("DOF_VEL").cpu())
    ep, eq, ev = rbs_err(got[:, :rm.num_links][live], own[live])
    print("zoo link frames:", what, "live", int(live.sum()), "pos", ep, "quat", eq, "vel", ev)
    assert live.sum() > hip.num_envs // 2 and ep <= 2e-5 and eq <= 2e-5 and ev <= 2e-4, (what, ep, eq, ev)


@pytest.mark.parametrize("name,kernel", CASES, ids=[f"{s}-{k}" for s, k in CASES])
def test_one_substep_from_identical_state(name, kernel, monkeypatch):
    robot_zoo.install(monkeypatch)
    scene = substep.ZOO_SCENES[name]
    traj = substep.oracle_trajectory(name)
    pick(monkeypatch, kernel)
    want, lanes = expected(scene, kernel)
    hip = substep.make_hip(scene)
    try:
        lay = hip.layout()
        assert lay["kernel"].split("<")[0] == want and lay["lanes_per_env"] == lanes, (name, kernel, lay)
        got = substep.replay(traj, hip)
        rm = substep.build_struct(scene)[3]["model"]
        if lanes > 1:
            link_frames_match(hip, rm, f"{name} / {kernel} / on refresh")
    finally:
        hip.close()
    substep.check(traj, got, kernel if lay["kernel"].startswith("grx_step_" + kernel) else f"{kernel} -> generic", log=LOG)   # (the log names what ran)
    if lanes > 1:      # the rows the step kernel writes itself: the last sub-step again, on a handle that publishes them every step
        monkeypatch.setenv("GRX_PUBLISH_EVERY_STEP", "1")
        hip = substep.make_hip(scene)
        try:
            assert hip.layout()["kernel"].split("<")[0] == want
            hip.reset_all()
            T = traj.actions.shape[0]
            for n in STATE_TENSORS:
                hip.tensor(n).copy_(traj.pre[n][T - 1].to(hip.device))
            hip.step(traj.actions[T - 1].to(hip.device), traj.delays[T - 1], T)
            torch.cuda.synchronize()
            assert torch.equal(hip.tensor("DOF_POS").cpu(), got["DOF_POS"][T - 1])      # the same sub-step, bit for bit
            link_frames_match(hip, rm, f"{name} / {kernel} / every step")
        finally:
            hip.close()


def test_the_cases_cover_every_model_on_every_kernel():
    assert {(substep.ZOO_SCENES[s].model, k) for s, k in CASES} == {(m, k) for m in robot_zoo.MODELS for k in KERNELS}
    assert {s for s, _ in CASES} == set(substep.ZOO_SCENES)
