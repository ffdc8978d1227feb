"""tests/stats_ref.py has to be right before it can judge the HIP reductions (tests/test_stats_scale_gpu.py): its rows against the f64
oracle's over a rollout with time-outs, a reset_idx and steps without a reset, against the extras["episode"] the reference itself recorded
(tests/golden/reset_family.npz), and its curriculum decision against tests/golden/command_curriculum.npz.

The oracle keeps its statistics rows in float32 (as the library does): the restatement's float64 row is rounded the same way before the
two are compared at 1e-9, and it is formed from the oracle's per-env sums and terms at the oracle's own precision (episode_terms(): the
published tensors are float32 casts, which alone move a mean by ~1e-8)."""
import os

import numpy as np
import pytest
import torch

from tests import stats_ref
from tests import test_oracle_golden as og
from tests import test_reset_golden as rg
from tests.helpers import make_cfg, make_sims, random_actions
from wiki_grx_gym_amd import _capi

NT = _capi.NUM_REWARD_TERMS


def f32_seconds(cfg):
    """grx_config.max_episode_length_s is a float: the divisor both the oracle and the kernels use"""
    return float(np.float32(cfg.env.episode_length_s))


def test_rows_of_a_rollout_equal_the_f64_oracles():
    """40 steps on the curriculum terrain with 20-step episodes, 100 envs: after every launch -- the first reset, steps on which a
    group of envs times out, steps where nobody reset, a reset_idx with duplicate ids -- the restated row equals episode_stats() and the
    launch's row of the history ring.  Rows of inactive terms are 0 whenever somebody reset (their sums never move)."""
    cfg = make_cfg(terrain="heightfield")
    cfg.env.episode_length_s = 0.4
    N = 100
    _, ora = make_sims(cfg, N, precision="f64", seed=2, hip=False)
    T = f32_seconds(cfg)
    active = np.array([getattr(cfg.rewards.scales, n, 0.0) != 0.0 for n in _capi.REWARD_TERMS])
    assert 5 <= active.sum() < NT
    hist = ora.tensor("EPISODE_STATS_HISTORY")
    seq = 0

    def check(want, what):
        got = ora.episode_stats()
        np.testing.assert_allclose(np.float32(want), got, rtol=1e-9, atol=0, err_msg=str(what))
        np.testing.assert_allclose(np.float32(want), hist[seq & (_capi.STATS_HISTORY - 1)].numpy(), rtol=1e-9, atol=0, err_msg=str(what))
        return got.astype(np.float64)

    sums, _ = ora.episode_terms()
    ora.reset_all(); seq += 1
    levels = ora.tensor("TERRAIN_LEVELS").numpy()
    prev = check(stats_ref.reset_stats(sums, np.arange(N), levels, T, np.zeros(NT + 2)), "reset_all")
    assert prev[NT] == N and (prev[:NT] == 0).all()
    gen = torch.Generator().manual_seed(0)
    # episodes of four ages (EPISODE_LENGTH is caller-writable, on_policy_runner.py:126): groups of envs time out on different steps
    ora.tensor("EPISODE_LENGTH").copy_(torch.tensor([0, 3, 7, 12])[torch.randint(0, 4, (N,), generator=gen)])
    kinds = {"none": 0, "some": 0, "time_out": 0}
    for s in range(40):
        if s == 30:      # a reset outside a step, ids listed twice and out of order
            ids = [77, 3, 99, 3, 41, 77, 0]
            sums, _ = ora.episode_terms()
            ora.reset_idx(torch.tensor(ids, dtype=torch.int32)); seq += 1
            prev = check(stats_ref.reset_stats(sums, ids, ora.tensor("TERRAIN_LEVELS").numpy(), T, prev), "reset_idx")
            assert prev[NT] == 5
        before, _ = ora.episode_terms()
        ora.step(random_actions(cfg, N, gen, 0.2), 5.0, 1 + s); seq += 1
        assert ora.last_stats_seq == seq and ora.last_stats_slot == seq & (_capi.STATS_HISTORY - 1)
        _, terms = ora.episode_terms()
        reset = ora.tensor("RESET").numpy().astype(bool)
        want = stats_ref.episode_stats(before, terms, reset, ora.tensor("TERRAIN_LEVELS").numpy(), T, prev)
        row = check(want, s)
        if reset.any():
            assert row[NT] == reset.sum() and (row[:NT][~active] == 0).all() and (row[:NT][active] != 0).sum() >= 5
        else:
            assert np.array_equal(row, prev)
        kinds["none" if not reset.any() else ("time_out" if ora.tensor("TIME_OUT").numpy().any() else "some")] += 1
        prev = row
    assert kinds["none"] >= 5 and kinds["time_out"] >= 5, kinds


@pytest.mark.parametrize("case", [c for c in rg.STEP_CASES if c != "shard"])
def test_rows_equal_the_references_recorded_extras(case):
    """The reference's own extras["episode"] of one post_physics_step() with a live reset_idx: the fixture's episode sums going in, the
    step's terms as the f64 oracle evaluates them on the recorded state (on the rows that did not reset they are the recorded change of
    the sums), the recorded reset rows and terrain levels -- at the fixture's tolerance for the f64 oracle.  (`shard`: its reference
    means run over the 128 envs of both ranks, the fixture records none.)"""
    tol = 2e-6
    k = rg.load_case(rg.fixture(), case)
    cfg = rg.case_cfg(case)
    sim, meta = rg.make_oracle(case, k, "f64")
    term_idx = rg.seed_handle(sim, k, meta, case != "plane")
    N = k["in_root"].shape[0]
    sim.debug_post_physics(og.states_from(k, "in_", N), apply_reset=True, common_step_counter=int(k["step_seed_offset"][0]))
    _, terms = sim.episode_terms()
    reset = k["out_reset"].astype(bool)
    assert 3 <= reset.sum() < N
    moved = k["out_episode_sums"].astype(np.float64) - k["in_episode_sums"]
    assert np.abs(terms[term_idx][:, ~reset] - moved[:, ~reset]).max() <= tol
    sums = np.zeros((NT, N))
    sums[term_idx] = k["in_episode_sums"]
    levels = k["out_terrain_levels"] if case != "plane" else np.zeros(N)
    row = stats_ref.episode_stats(sums, terms, reset, levels, f32_seconds(cfg), np.zeros(NT + 2))
    assert row[NT] == reset.sum()
    others = np.setdiff1d(np.arange(NT), term_idx)
    assert (row[others] == 0).all()
    if "out_extras_rew" in k:
        want = k["out_extras_rew"].astype(np.float64)
        assert want.shape == (len(term_idx),) and np.abs(want).max() > 1e-3
        err = np.abs(row[term_idx] - want)
        assert (err <= tol + tol * np.abs(want)).all(), (case, float(err.max()))
    if "out_extras_terrain_level" in k:
        assert abs(row[NT + 1] - float(k["out_extras_terrain_level"])) <= 1e-5
    # the reference's dict of a step without resets is the previous one
    prev = np.arange(NT + 2, dtype=np.float64)
    assert np.array_equal(stats_ref.episode_stats(sums, terms, np.zeros(N, bool), levels, f32_seconds(cfg), prev), prev)


def test_base_rows_and_reset_rows():
    """The base-term form is the per-term mean alone; ids listed twice count once and ids outside the batch not at all."""
    rng = np.random.default_rng(0)
    NB, N = _capi.NUM_BASE_REWARD_TERMS, 37
    sums, terms = rng.uniform(1, 2, (NB, N)), rng.uniform(-0.1, 0.1, (NB, N))
    reset = np.zeros(N, bool); reset[[0, 5, 36]] = True
    want = [np.mean([sums[t, i] + terms[t, i] for i in (0, 5, 36)]) / 20.0 for t in range(NB)]
    np.testing.assert_allclose(stats_ref.base_episode_stats(sums, terms, reset, 20.0, np.zeros(NB)), want, rtol=1e-14)
    prev = rng.uniform(0, 1, NB)
    assert np.array_equal(stats_ref.base_episode_stats(sums, terms, np.zeros(N, bool), 20.0, prev), prev)
    ids = [36, 5, 5, 0, 36, -1, N]
    assert np.array_equal(stats_ref.reset_rows(ids, N), reset)
    np.testing.assert_allclose(stats_ref.reset_stats(sums, ids, None, 20.0, prev), sums[:, reset].mean(1) / 20.0, rtol=1e-14)
    full = stats_ref.reset_stats(sums, ids, np.arange(N), 20.0, np.zeros(NB + 2))
    assert full[NB] == 3 and full[NB + 1] == 18.0


def test_curriculum_decision_follows_the_reference():
    """tests/golden/command_curriculum.npz: the reference's update_command_curriculum over eight steps (asymmetric start, the clip at
    max_curriculum, means 0.1 % either side of the threshold): the restated decision gives the recorded range after every one."""
    d = np.load(os.path.join(og.G, "command_curriculum.npz"))
    rng = tuple(map(float, d["start"]))
    moved = 0
    for k in range(len(d["reset"])):
        new = stats_ref.command_curriculum(d["sums"][k], d["reset"][k], rng, float(d["scale_dt"]), float(d["max_episode_length"]), float(d["max_curriculum"]))
        np.testing.assert_allclose(new, d["lin_vel_x"][k], rtol=0, atol=1e-12, err_msg=str(k))
        moved += new != rng
        rng = new
    assert 2 <= moved < len(d["reset"])
    assert stats_ref.command_curriculum(d["sums"][0], np.zeros(64, bool), rng, 0.02, 1000, 1.7) == rng
