"""What reduces ACROSS envs, at the block counts of real runs (`-m gpu`): GRX_T_EPISODE_STATS and its history ring, GRX_T_BASE_EPISODE_STATS
and the command curriculum, against tests/stats_ref.py (float64 numpy, checked on the CPU by tests/test_stats_ref.py) on the tensors read
back from the same handle.  Sharding cannot move these by construction, so tests/test_hip_parity.test_full_size_properties does not see
them; the sizes here are the smallest that reach each regime of stat_reduce (csrc/grx_kernels.hip: up to 64 columns one per lane, up to
448 the one-by-one loop, beyond it the body unrolled by 8 and a tail), the second trip of grx_base_stats_kernel's column loop and the
columns and envs past the 1024 threads of grx_curriculum_kernel.  Plane terrain, zero actions, injected state: EPISODE_SUMS and
TERRAIN_LEVELS are caller-writable, EPISODE_LENGTH = max_episode_length makes an env time out on the next step.  The oracle is not stepped.

Counts are exact.  The tolerance of a mean is derived, not tuned: every addend is positive, so the fp32 sum is within (longest chain of
additions) x 2^-24 relative of the exact one; the chain is the envs of a block, ceil(columns / 64) serial adds per lane and 6 butterfly
levels; two divisions and the store add three roundings.  The tests assert at twice that (-fassociative-math may regroup the adds: the
count of addends stays).  The observed error over the asserted tolerance is printed per case and, if GRX_STATS_SCALE_LOG names a json
file, merged into it (profiles/stats_scale_bounds.json holds an MI355X's)."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import stats_ref
from tests.helpers import make_cfg
from tests.test_base_rewards_gpu import curriculum_sim, force_resets, make_base_hip, max_episode_length
from wiki_grx_gym_amd import _capi
from wiki_grx_gym_amd.envs import build_config

pytestmark = pytest.mark.gpu

NT, NB, RING = _capi.NUM_REWARD_TERMS, _capi.NUM_BASE_REWARD_TERMS, _capi.STATS_HISTORY
EPS = 2.0 ** -24
LOG = os.environ.get("GRX_STATS_SCALE_LOG")
LAYOUT_ENV = ("GRX_FORCE_GENERIC", "GRX_TREE", "GRX_TREE_G", "GRX_TREE_WAVES", "GRX_GENERIC_EPB", "GRX_LANES_PER_ENV", "GRX_WAVES_PER_BLOCK", "GRX_QUAD_WAVES")


def chain_bound(envs_per_block, columns):
    """relative error bound of a mean (module docstring): the asserted tolerance is twice this"""
    return (envs_per_block + math.ceil(columns / 64) + 6 + 3) * EPS


def reset_bound(N, envs_per_block=16):
    """a reset outside a step: every reset kernel reduces its one-wave block by a 6-level butterfly, over blocks of 16 envs at the least"""
    return (6 + math.ceil(math.ceil(N / envs_per_block) / 64) + 6 + 3) * EPS


class Ratios:
    """largest observed error / asserted tolerance of one case"""

    def __init__(self, case):
        self.case, self.worst = case, 0.0

    def close(self, what, got, want, bound):
        got, want = np.atleast_1d(np.asarray(got, dtype=np.float64)), np.atleast_1d(np.asarray(want, dtype=np.float64))
        assert got.shape == want.shape, (what, got.shape, want.shape)
        tol = 2.0 * bound * np.abs(want)
        assert (tol > 0).all(), (what, "a mean of positive addends is positive")
        err = np.abs(got - want)
        ratio = float((err / tol).max())
        self.worst = max(self.worst, ratio)
        print(f"{self.case} {what}: error / tolerance {ratio:.3f} (tolerance {2.0 * bound:.2e} relative)")
        assert ratio <= 1.0, f"{self.case} {what}: error {ratio:.3f} x the tolerance of {2.0 * bound:.2e} relative, worst entry {int(np.argmax(err / tol))}"

    def file(self):
        print(f"{self.case}: largest error / tolerance {self.worst:.3f}")
        if LOG:
            rec = {}
            if os.path.exists(LOG):
                with open(LOG) as f:
                    rec = json.load(f)
            rec[self.case] = round(self.worst, 4)
            with open(LOG, "w") as f:
                json.dump(rec, f, indent=1, sort_keys=True)


# name: (task, environment of the layout, kernel prefix, lanes per env, waves per block, envs per block)
LAYOUTS = {
    "pair1": ("GR1T1", {"GRX_LANES_PER_ENV": "2", "GRX_WAVES_PER_BLOCK": "1"}, "grx_step_kernel<", 2, 1, 32),
    "pair8": ("GR1T1", {"GRX_LANES_PER_ENV": "2", "GRX_WAVES_PER_BLOCK": "8"}, "grx_step_kernel<", 2, 8, 32),
    "quad": ("GR1T1", {"GRX_LANES_PER_ENV": "4", "GRX_QUAD_WAVES": "8"}, "grx_step_kernel_quad<", 4, 8, 16),
    "tree8": ("GR1T1", {"GRX_FORCE_GENERIC": "1", "GRX_TREE": "1", "GRX_TREE_G": "8", "GRX_TREE_WAVES": "1"}, "grx_step_tree<", 8, 1, 8),
    "tree16": ("GR1T1", {"GRX_FORCE_GENERIC": "1", "GRX_TREE": "1", "GRX_TREE_G": "16", "GRX_TREE_WAVES": "1"}, "grx_step_tree16<", 16, 1, 4),
    "full16": ("GR1T1Full", {"GRX_TREE": "1", "GRX_TREE_G": "16", "GRX_TREE_WAVES": "1"}, "grx_step_tree16<", 16, 1, 4),
    "generic": ("GR1T1", {"GRX_FORCE_GENERIC": "1", "GRX_TREE": "0", "GRX_GENERIC_EPB": "16"}, "grx_step_generic<", 1, 1, 16),
}
# (layout, N, columns): the smallest N that reaches each regime
CASES = [(l, n, c) for l in ("pair1", "pair8") for n, c in ((20, 1), (2085, 66), (14341, 449), (16389, 513))] + \
        [("quad", 7173, 449), ("tree8", 3589, 449), ("tree16", 1793, 449), ("full16", 1793, 449), ("generic", 7173, 449)]
RESET_OUTSIDE = {("pair1", 16389), ("pair8", 16389), ("tree16", 1793)}


def pick(monkeypatch, layout):
    for k in LAYOUT_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in LAYOUTS[layout][1].items():
        monkeypatch.setenv(k, v)


def make_handle(monkeypatch, layout, N, columns):
    from wiki_grx_gym_amd.sim import HipSim
    task, _, kernel, lpe, waves, epb = LAYOUTS[layout]
    pick(monkeypatch, layout)
    cfg = make_cfg(task)
    c, keep, meta = build_config.build(cfg, cfg.sim.dt, N)
    assert int(c.publish_reward_terms) == 1
    sim = HipSim(c, "cuda:0", keep)
    lay = sim.layout()
    assert lay["kernel"].startswith(kernel) and (lay["lanes_per_env"], lay["waves_per_block"], lay["envs_per_block"]) == (lpe, waves, epb), lay
    assert lay["num_blocks"] == columns == math.ceil(N / epb), lay
    active = np.array([n in meta["active_terms"] and n != "termination" for n in _capi.REWARD_TERMS])
    assert 10 <= active.sum() < NT
    return sim, cfg, active, lay


def injected_sums(active, N, k, rows=NT):
    """(rows, N) float32-exact, >= 1 on the active rows (the step's own term, |.| < 1, cannot cancel them) and 0 on the others: a ramp in
    the env index plus an offset per term (a column read from another row moves the mean) and per injection k"""
    t = np.arange(rows, dtype=np.float64)[:, None]
    e = np.arange(N, dtype=np.float64)[None, :]
    v = (1.0 + t / 8.0 + k / 16.0 + e / 4096.0) * np.asarray(active, dtype=np.float64)[:, None]
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
    return v


def put(sim, name, value):
    t = sim.tensor(name)
    t.copy_(torch.as_tensor(np.ascontiguousarray(value)).to(t.dtype).to(t.device))


def get(sim, name):
    return sim.tensor(name).cpu().numpy()


def patterns(N, epb, columns):
    e = np.arange(N)
    out = [("all", np.ones(N, bool)), ("last", e == N - 1)]
    if columns > 448:
        out.append(("columns >= 448", e >= 448 * epb))
    out += [("every 97th", e % 97 == 0), ("none", np.zeros(N, bool))]
    return out


class Stepper:
    """One handle: inject, step, and check the launch's statistics both ways -- now through episode_stats() (the flush,
    grx_finalize_stats) and, after the NEXT launch, through the launch's row of the history ring, which this class overwrites in between
    so that only that launch's stats_fold_previous can have filed it (the one-lane generic kernel has no fold: its step ends with the
    reduction, and the row is left alone)."""

    def __init__(self, sim, cfg, active, lay, ratios):
        self.sim, self.cfg, self.active, self.lay, self.ratios = sim, cfg, active, lay, ratios
        self.N = sim.num_envs
        self.T = float(np.float32(cfg.env.episode_length_s))      # (grx_config.max_episode_length_s is a float)
        self.folds = "generic" not in lay["kernel"]
        self.reset_folds = self.folds and "tree" not in lay["kernel"]      # (the tree kernels reset through the generic reset kernel, which reduces its predecessor's rows only if no flush did)
        self.zero = torch.zeros(self.N, sim.num_dofs, device="cuda")
        self.counter, self.injections = 1, 0
        self.pending = None      # (slot, row) of the last launch, to be filed again by the next one
        self.hist = sim.tensor("EPISODE_STATS_HISTORY")
        sim.reset_all()
        self.seq = 1
        self.prev = sim.episode_stats().astype(np.float64)
        assert self.prev[NT] == self.N

    def inject(self):
        self.injections += 1
        sums = injected_sums(self.active, self.N, self.injections)
        put(self.sim, "EPISODE_SUMS", sums)
        levels = (np.arange(self.N) * 7 + self.injections) % 10      # (the plane's resets leave the levels; row NT + 1 is their mean)
        put(self.sim, "TERRAIN_LEVELS", levels)
        return sums, levels

    def fold_check(self, what):
        """after a launch: its predecessor's row of the ring, filed by this launch, is bit-equal to what the flush gave"""
        if self.pending is None:
            return
        slot, row = self.pending
        self.pending = None
        if self.folds:
            torch.cuda.synchronize()
            assert np.array_equal(self.hist[slot].cpu().numpy(), row), (what, "the fold filed", self.hist[slot].cpu().numpy(), "the flush gave", row)

    def after_launch(self, what, want, bound, exact):
        """the launch's row through the flush against `want`; `exact`: entries that must be equal, the others within twice `bound`"""
        sim = self.sim
        self.seq += 1
        assert sim.stats_seq() == self.seq
        slot = self.seq & (RING - 1)
        self.fold_check(what)
        row = sim.episode_stats()
        assert row[NT] == want[NT], (what, "finished episodes", row[NT], want[NT])      # a dropped or doubled column shows here outright
        if exact:
            assert np.array_equal(row, np.float32(want)), (what, row, want)
        else:
            self.ratios.close(f"{what}: means", row[:NT][self.active], want[:NT][self.active], bound)
            assert (row[:NT][~self.active] == 0).all(), what      # (tests/test_stats_ref.py: rows of inactive terms are 0)
            self.ratios.close(f"{what}: terrain level", row[NT + 1], want[NT + 1], bound)
        assert np.array_equal(self.hist[slot].cpu().numpy(), row), what
        if self.folds:
            self.hist[slot] = -7777.0
            self.pending = (slot, row)
        self.prev = row.astype(np.float64)
        return slot

    def step(self, name, rows):
        sim, N = self.sim, self.N
        sums, levels = self.inject()
        ep = np.where(rows, max_episode_length(self.cfg), 0)
        put(sim, "EPISODE_LENGTH", ep)
        prev = self.prev
        slot = sim.step(self.zero, 0.0, self.counter)
        self.counter += 1
        assert slot == (self.seq + 1) & (RING - 1) and sim.last_stats_seq == self.seq + 1
        torch.cuda.synchronize()
        reset = get(sim, "RESET").astype(bool)
        assert np.array_equal(reset, rows), (name, int(reset.sum()), int(rows.sum()))
        assert np.array_equal(get(sim, "TIME_OUT").astype(bool), rows)
        terms = get(sim, "REWARD_TERMS").astype(np.float64)
        assert (terms[~self.active] == 0).all() and np.abs(terms).max() < 1.0
        total = sums + terms
        assert total[self.active].min() > 0.5      # every addend positive: what the tolerance assumes
        assert np.array_equal(get(sim, "TERRAIN_LEVELS"), levels)
        want = stats_ref.episode_stats(sums, terms, reset, levels, self.T, prev)
        self.after_launch(name, want, chain_bound(self.lay["envs_per_block"], self.lay["num_blocks"]), exact=not rows.any())
        if not rows.any():
            assert np.array_equal(self.prev, prev)      # nobody reset: the row is kept, the ring's row repeats
        after = get(sim, "EPISODE_SUMS").astype(np.float64)
        assert (after[:, reset] == 0).all(), name
        # the others advanced by the step's term: one rounding of the add, one more if the term's scaling was contracted into it
        live = total[:, ~reset]
        assert (np.abs(after[:, ~reset] - live) <= 2.0 ** -23 * np.abs(live)).all(), name

    def reset_outside(self, name, ids):
        """reset_idx(ids) (ids None: reset_all) with injected sums: the mean over the distinct ids, their sums zeroed, the others' kept"""
        sim, N = self.sim, self.N
        sums, levels = self.inject()
        prev = self.prev
        if self.pending is not None and not self.reset_folds:      # no fold in this launch: the row goes back as the flush filed it
            slot, row = self.pending
            self.hist[slot] = torch.as_tensor(row, device="cuda")
            self.pending = None
        if ids is None:
            sim.reset_all()
            rows = np.ones(N, bool)
        else:
            sim.reset_idx(torch.as_tensor(ids, dtype=torch.int32, device="cuda"))
            rows = stats_ref.reset_rows(ids, N)
            assert len(ids) > rows.sum() > 256
        torch.cuda.synchronize()
        assert np.array_equal(get(sim, "RESET").astype(bool)[rows], np.ones(int(rows.sum()), bool))
        want = stats_ref.reset_stats(sums, np.flatnonzero(rows) if ids is None else ids, levels, self.T, prev)
        assert want[NT] == rows.sum()
        self.after_launch(name, want, reset_bound(N), exact=False)
        after = get(sim, "EPISODE_SUMS").astype(np.float64)
        assert (after[:, rows] == 0).all() and np.array_equal(after[:, ~rows], sums[:, ~rows]), name

    def finish(self):
        """one more step files the last row through the fold"""
        if self.pending is not None and self.folds:
            put(self.sim, "EPISODE_LENGTH", np.zeros(self.N, np.int64))
            self.sim.step(self.zero, 0.0, self.counter)
            self.seq += 1
            self.fold_check("last launch")


def spread_ids(N):
    """about 1000 ids over all columns (more than the 256 of a grx_mark_kernel block), out of order, some twice, the last env among them"""
    ids = np.concatenate([np.arange(0, N, max(2, N // 1000)), [N - 1, N - 1, 0, 5, 5, 4], np.arange(0, N, 97)])
    return np.random.default_rng(3).permutation(ids)


@pytest.mark.parametrize("layout,N,columns", CASES, ids=[f"{l}-{n}" for l, n, _ in CASES])
def test_episode_statistics_at_scale(layout, N, columns, monkeypatch):
    """Per layout and regime (module docstring), five steps on one handle -- every env resets; the last env alone (the ragged column);
    the envs of columns >= 448 alone, where there are such; every 97th env; nobody -- then, on the 513-column pair handles and the 16-lane
    tree handle, a reset_idx of ~1000 ids with duplicates and a reset_all.  After each launch: the count of finished episodes exact, the
    means and the mean terrain level within the derived tolerance of stats_ref on the tensors read back, the reset envs' sums zeroed and
    the others' advanced by the step's term, the flushed row bit-equal to the ring's and to what the next launch's fold files."""
    sim, cfg, active, lay = make_handle(monkeypatch, layout, N, columns)
    ratios = Ratios(f"{layout}-{N}")
    try:
        st = Stepper(sim, cfg, active, lay, ratios)
        for name, rows in patterns(N, lay["envs_per_block"], columns):
            st.step(name, rows)
        if (layout, N) in RESET_OUTSIDE:
            st.reset_outside("reset_idx", spread_ids(N))
            st.reset_outside("reset_all", None)
        st.finish()
    finally:
        sim.close()
    ratios.file()


def test_history_ring_across_the_wrap(monkeypatch):
    """130 launches on 40 envs -- a reset_all, steps, one reset_idx -- with a forced reset on every third and distinct sums each time.
    No flush: every launch's row is read right after the FOLLOWING launch (stats_fold_previous files it) and equals the reference;
    stats_slot == seq & 127 across the wrap, and row 1 then holds launch 129's statistics, not launch 1's."""
    pick(monkeypatch, "pair1")
    sim, cfg, active, lay = make_handle(monkeypatch, "pair1", 40, 2)
    N, T = 40, float(np.float32(cfg.env.episode_length_s))
    ratios = Ratios("ring-40")
    bound = chain_bound(lay["envs_per_block"], lay["num_blocks"])
    hist = sim.tensor("EPISODE_STATS_HISTORY")
    zero = torch.zeros(N, sim.num_dofs, device="cuda")
    try:
        sim.reset_all()
        first = sim.episode_stats().astype(np.float64)      # launch 1 (flushed once: the previous row of what follows)
        assert first[NT] == N and sim.stats_seq() == 1
        prev, want, forced = first, None, 0
        for seq in range(2, 131):
            rows = np.zeros(N, bool)
            if seq % 3 == 0:
                rows[[seq % N, (7 * seq) % N, (11 * seq + 3) % N]] = True
            sums = injected_sums(active, N, seq % 50)
            levels = (np.arange(N) * 3 + seq) % 10
            put(sim, "EPISODE_SUMS", sums)
            put(sim, "TERRAIN_LEVELS", levels)
            if seq == 77:      # a reset outside a step in between
                ids = [39, 0, 17, 17, 39]
                sim.reset_idx(torch.tensor(ids, dtype=torch.int32, device="cuda"))
                assert sim.stats_seq() == seq
                rows = stats_ref.reset_rows(ids, N)
                terms = np.zeros((NT, N))
            else:
                put(sim, "EPISODE_LENGTH", np.where(rows, max_episode_length(cfg), 0))
                slot = sim.step(zero, 0.0, seq)
                assert slot == seq & (RING - 1) == sim.last_stats_slot and sim.last_stats_seq == seq == sim.stats_seq()
            torch.cuda.synchronize()
            if want is not None:      # the row of launch seq - 1, filed by this launch
                got = hist[(seq - 1) & (RING - 1)].cpu().numpy()
                check_row(ratios, f"launch {seq - 1}", got, want, prev, active, bound)
                prev = got.astype(np.float64)
            forced += int(rows.any())
            if seq != 77:      # (the forced rows time out; left to zero actions for a hundred steps a robot may also fall: the step's own flags count)
                reset = get(sim, "RESET").astype(bool)
                assert (reset[rows]).all() and np.array_equal(get(sim, "TIME_OUT").astype(bool), rows), seq
                rows = reset
                terms = get(sim, "REWARD_TERMS").astype(np.float64)
                assert (sums + terms)[active].min() > 0.5
            want = stats_ref.episode_stats(sums, terms, rows, levels, T, prev)
        assert forced >= 43
        got = sim.episode_stats()      # launch 130 through the flush (no forced reset: the row of launch 129 again, unless a robot fell)
        check_row(ratios, "launch 130", got, want, prev, active, bound)
        assert np.array_equal(hist[130 & (RING - 1)].cpu().numpy(), got)
        row1 = hist[1].cpu().numpy()      # launch 129's (a forced reset of three envs), where launch 1's (the reset_all of 40) was
        assert np.array_equal(row1, np.float32(prev)) and 3 <= row1[NT] < N == first[NT]
    finally:
        sim.close()
    ratios.file()


def check_row(ratios, what, got, want, prev, active, bound):
    assert got[NT] == want[NT], (what, got[NT], want[NT])
    if np.array_equal(want, prev):      # nobody reset: the previous row, unchanged
        assert np.array_equal(got, np.float32(prev)), what
        return
    ratios.close(f"{what}: means", got[:NT][active], want[:NT][active], bound)
    assert (got[:NT][~active] == 0).all(), what
    ratios.close(f"{what}: terrain level", got[NT + 1], want[NT + 1], bound)


# ---- legged_gym's base terms and the command curriculum ------------------------------------------------------------------------------
# (tree, N, envs per block of the step kernel, its columns, columns of the first trip of the loop under test)
BASE_CASES = [(None, 4165, 32, 131, 64), (16, 4101, 4, 1026, 1024)]


def pick_base(monkeypatch, tree):
    for k in LAYOUT_ENV:
        monkeypatch.delenv(k, raising=False)
    if tree:
        monkeypatch.setenv("GRX_TREE_WAVES", "1")      # (make_base_hip / curriculum_sim set the other three)


@pytest.mark.parametrize("tree,N,epb,columns,first_trip", BASE_CASES, ids=["pair-4165", "tree16-4101"])
def test_base_episode_statistics_at_scale(tree, N, epb, columns, first_trip, monkeypatch):
    """GRX_T_BASE_EPISODE_STATS after a reset_idx (grx_base_reset_kernel: a column per 64 envs, 66 of them) and after a resetting step
    (a column per block or wave of the step kernel: 131 on the lane-pair base entry, 1026 on the 16-lane tree with one wave, i.e. two
    and 17 trips of grx_base_stats_kernel's loop), against stats_ref on the injected sums and the step's published terms."""
    pick_base(monkeypatch, tree)
    sim, cfg, _ = make_base_hip("plane", N=N, tree=tree, monkeypatch=monkeypatch)
    lay = sim.layout()
    assert (lay["envs_per_block"], lay["num_blocks"], lay["waves_per_block"]) == (epb, columns, 1), lay
    assert math.ceil(N / 64) > 64 and columns > first_trip
    ratios = Ratios(f"base-{'tree16' if tree else 'pair'}-{N}")
    T = float(np.float32(cfg.env.episode_length_s))
    on = np.ones(NB, bool)
    try:
        sim.reset_all()
        # a reset outside a step
        sums = 15.0 + injected_sums(on, N, 1, rows=NB)
        put(sim, "BASE_EPISODE_SUMS", sums)
        ids = spread_ids(N)
        rows = stats_ref.reset_rows(ids, N)
        sim.reset_idx(torch.as_tensor(ids, dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        got = get(sim, "BASE_EPISODE_STATS")
        ratios.close("reset_idx", got, stats_ref.reset_stats(sums, ids, None, T, np.zeros(NB)), reset_bound(N, 64))
        after = get(sim, "BASE_EPISODE_SUMS").astype(np.float64)
        assert (after[:, rows] == 0).all() and np.array_equal(after[:, ~rows], sums[:, ~rows])
        assert sim.episode_stats()[NT] == rows.sum()
        prev = got.astype(np.float64)
        # a step that resets every third env and the last: envs of every column, the ragged one included
        sums = 15.0 + injected_sums(on, N, 2, rows=NB)
        put(sim, "BASE_EPISODE_SUMS", sums)
        rows = np.arange(N) % 3 == 0
        rows[N - 1] = True
        force_resets(sim, rows, cfg=cfg)
        sim.step(torch.zeros(N, sim.num_dofs, device="cuda"), 0.0, 1)
        torch.cuda.synchronize()
        reset = get(sim, "RESET").astype(bool)
        assert np.array_equal(reset, rows)
        terms = get(sim, "BASE_REWARD_TERMS").astype(np.float64)
        total = sums + terms
        assert total.min() > 0.5 and (terms != 0).any(1).sum() >= 3      # positive addends: what the tolerance assumes (in free fall from the reset pose most terms are 0)
        got = get(sim, "BASE_EPISODE_STATS")
        ratios.close("step", got, stats_ref.base_episode_stats(sums, terms, reset, T, prev), chain_bound(epb, columns))
        assert sim.episode_stats()[NT] == rows.sum()
        after = get(sim, "BASE_EPISODE_SUMS").astype(np.float64)
        assert (after[:, reset] == 0).all()
        live = total[:, ~reset]
        assert (np.abs(after[:, ~reset] - live) <= 2.0 ** -23 * np.abs(live)).all()
        # a step without resets keeps the row
        force_resets(sim, np.zeros(N, bool), cfg=cfg)
        sim.step(torch.zeros(N, sim.num_dofs, device="cuda"), 0.0, 2)
        torch.cuda.synchronize()
        assert not get(sim, "RESET").any() and np.array_equal(get(sim, "BASE_EPISODE_STATS"), got)
    finally:
        sim.close()
    ratios.file()


@pytest.mark.parametrize("tree,N,epb,columns,first_trip", BASE_CASES, ids=["pair-4165", "tree16-4101"])
def test_command_curriculum_at_scale(tree, N, epb, columns, first_trip, monkeypatch):
    """grx_curriculum_kernel past its first trips.  Case A: the forced resets' tracking sums have a mean 0.1 % above the threshold only
    with the columns past `first_trip` in it (1024: the kernel's threads; 64 on the lane-pair handle: grx_base_stats_kernel's lanes) and
    10 % below it without them; case B the mirror.  COMMAND_RANGES follows stats_ref.command_curriculum both times.  Case A widens, with
    reset envs at indices >= 1024 (the redraw loop's second trip): their commands, obs[:, 0:2] and pri_obs[:, 0:2] are bit-equal to a twin
    handle's whose curriculum is off and whose configured range is the widened one."""
    pick_base(monkeypatch, tree)
    a, cfg, d = curriculum_sim(N=N, tree=tree, monkeypatch=monkeypatch)
    lay = a.layout()
    assert (lay["envs_per_block"], lay["num_blocks"], lay["waves_per_block"]) == (epb, columns, 1), lay
    scale_dt, max_cur = float(d["scale_dt"]), float(d["max_curriculum"])
    L = max_episode_length(cfg)
    assert L == float(d["max_episode_length"])
    thr = 0.8 * scale_dt * L
    widened = [max(float(d["start"][0]) - 0.5, -max_cur), min(float(d["start"][1]) + 0.5, max_cur)]
    b, _, _ = curriculum_sim(curriculum=False, lin_vel_x=widened, N=N, tree=tree, monkeypatch=monkeypatch)
    t = _capi.BASE_REWARD_TERMS.index("tracking_lin_vel")
    split = first_trip * epb      # the first env of the columns past the first trip
    lo_rows, hi_rows = np.array([3, 700, 1023, 1024, split - 1]), np.arange(N - 5, N)
    assert split <= N - 5 and hi_rows.min() >= 1024 and lo_rows.max() < split
    rows = np.zeros(N, bool)
    rows[lo_rows] = rows[hi_rows] = True
    zero = torch.zeros(N, a.num_dofs, device="cuda")
    try:
        for s in (a, b):
            s.reset_all()
        rng = tuple(map(float, d["start"]))
        for case, (low, mean) in (("A", (0.9, 1.001)), ("B", (1.1, 0.999))):
            sums = np.zeros(N, np.float32)
            sums[lo_rows] = low * thr
            sums[hi_rows] = (2.0 * mean - low) * thr
            assert (sums[lo_rows].mean() > thr) != (sums[rows].mean() > thr)      # the columns past the first trip decide
            for s in (a, b):
                force_resets(s, rows, sums, scale_dt, cfg)
            before = get(a, "BASE_EPISODE_SUMS")[t].astype(np.float64)
            counter = 1 if case == "A" else 2
            a.step(zero, 0.0, counter)
            b.step(zero, 0.0, counter)
            torch.cuda.synchronize()
            reset = get(a, "RESET").astype(bool)
            assert np.array_equal(reset, rows) and np.array_equal(get(b, "RESET").astype(bool), rows)
            tracking = before + get(a, "BASE_REWARD_TERMS")[t]
            want = stats_ref.command_curriculum(tracking, reset, rng, scale_dt, L, max_cur)
            assert (want != rng) == (case == "A"), (case, want, rng)
            got = get(a, "COMMAND_RANGES")
            assert np.allclose(got[0], want, rtol=0, atol=1e-6), (case, got[0], want)
            assert np.allclose(got[1:], [cfg.commands.ranges.lin_vel_y, cfg.commands.ranges.ang_vel_yaw])
            rng = want
            if case == "A":
                assert np.allclose(want, widened, rtol=0, atol=1e-12)
            # A's resets drew from the widened range (case B: still from it), as the twin's: the redraw's envs >= 1024 among them
            r = torch.as_tensor(rows, device="cuda")
            ca, cb = a.tensor("COMMANDS")[r], b.tensor("COMMANDS")[r]
            assert torch.equal(ca, cb), (case, ca, cb)
            assert torch.equal(a.tensor("OBS")[r][:, 0:2], b.tensor("OBS")[r][:, 0:2]) and torch.equal(a.tensor("PRI_OBS")[r][:, 0:2], b.tensor("PRI_OBS")[r][:, 0:2])
            assert (ca[-5:, 0] != 0).any() and (ca[:5, 0] != 0).any()      # (not every command was zeroed by |cmd_xy| <= 0.1)
    finally:
        a.close(); b.close()
