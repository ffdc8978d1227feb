"""float64 numpy statement of random network distillation's intrinsic reward (rl/rnd.py, include/grx_ppo.h grx_rnd_reward; DESIGN.md
4.12), written from the formulas, the inputs of its numeric tests and their bounds.  Shared by tests/test_rnd.py and
tests/test_rnd_gpu.py.

How a 30-step sequence is checked (`check_sequence`).  Every call is checked on its own: its inputs -- pred, targ, and the in/out rows
ret and rewards as the implementation holds them before the call -- are converted exactly to float64, and
    raw        |raw - r64| <= (E + 8) u r64, u = 2^-24: one rounding of the difference gives 3 u on its square, at most E roundings on a sum
               of non-negative terms in any order, the square root halves the relative error and adds its own rounding: about (E + 5) / 2 u,
               so the bound has a margin of two
    ret        |ret - fma64(gamma, ret_in, r64)| <= that bound + 2^-23 |ret64| (the fused multiply-add's own rounding, margin two)
    intrinsic  within 4 u |x64| of weight * raw / (std + eps) evaluated in float64 from the implementation's OWN float32 raw and std
    rewards    rewards_in + intrinsic in float32, bitwise
    count      exactly (step + 1) N, int64
and after the last call mean, var and std against an independent float64 trajectory (all N rows in one piece: no slabs) within the
bounds tests/obs_norm_ref.py::check sets for one column -- it is the same update; std enters through check's `y`, formed from the
implementation's own mean and std.  The per-call reading of the ret bound is the one its derivation supports: over 30 steps the
roundings of the stored float32 ret add up like a random walk (about 1.3 u |ret| after 30 steps, 4 u over a thousand rows), which no
single-call bound covers.  Against the independent trajectory ret is therefore held to the bound that follows from the single-call one
by induction: a call's error is at most gamma times the error of its input plus that call's own bound, so
    B_t = gamma B_{t-1} + (E + 8) u r64_t + 2^-23 |ret64_t|,  B_0 = 0        (r64, ret64: the trajectory's; times 1 + 2^-16 for the
                                                                               second-order terms: the bounds are relative to 1 + O(u) values)
is asserted after every call; the figure itself is printed in u."""
import functools

import numpy as np

from tests import obs_norm_ref

U = 2.0 ** -24
STEPS = 30
# the entry point takes gamma, weight and eps as float32: the reference uses those values, converted exactly like every other input
GAMMA, WEIGHT, EPS = (float(np.float32(v)) for v in (0.99, 0.1, 1e-2))


def weight_at(it, weight=0.1, schedule="constant", final_weight=None, start_it=0, end_it=0, at_it=0):
    """constant; linear: `weight` up to start_it, `final_weight` from end_it on, the straight line between; step: final_weight from at_it on"""
    final = weight if final_weight is None else final_weight
    if schedule == "constant":
        return float(weight)
    if schedule == "step":
        return float(final if it >= at_it else weight)
    assert schedule == "linear"
    return float(np.interp(it, [start_it, end_it], [weight, final])) if end_it > start_it else float(final if it > start_it else weight)


def row_norm(pred, targ):
    d = np.asarray(targ, dtype=np.float64) - np.asarray(pred, dtype=np.float64)
    return np.sqrt((d * d).sum(1))


class RefReward:
    """the state of the discounted-return normaliser and one step of the reward, float64"""

    def __init__(self, N, gamma=GAMMA, eps=EPS):
        self.gamma, self.eps = gamma, eps
        self.ret = np.zeros(N)
        self.count, self.mean, self.var, self.std = 0, 0.0, 1.0, 1.0

    def step(self, pred, targ, weight, rewards):
        """-> (raw, intrinsic, rewards + intrinsic)"""
        r = row_norm(pred, targ)
        self.ret = self.gamma * self.ret + r
        n = r.shape[0]
        self.count += n
        rate = n / self.count
        m, v = self.ret.mean(), self.ret.var()          # the Chan merge over all N in one piece: the mean, then the centred squares
        delta = m - self.mean
        self.mean = self.mean + rate * delta
        self.var = self.var + rate * (v - self.var + delta * (m - self.mean))
        self.std = np.sqrt(self.var)
        x = weight * r / (self.std + self.eps)
        return r, x, np.asarray(rewards, dtype=np.float64) + x


@functools.lru_cache(maxsize=None)
def inputs(N, E, steps=STEPS):
    """per step (pred, targ, rewards) in float32, seeded: embeddings of order one whose distance shrinks with the step, as a predictor's
    does while it learns, rewards of both signs"""
    rng = np.random.default_rng(1000 * N + E)
    out = []
    for s in range(steps):
        targ = np.float32(rng.standard_normal((N, E)))
        pred = np.float32(targ + (1.0 / (1.0 + 0.1 * s)) * rng.standard_normal((N, E)) * np.geomspace(0.05, 2.0, N)[:, None])
        rew = np.float32(rng.standard_normal(N))
        for a in (pred, targ, rew):
            a.setflags(write=False)
        out.append((pred, targ, rew))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def trajectory(N, E, steps=STEPS):
    """the independent float64 run over inputs(N, E): per step (raw, ret, intrinsic, mean, var, std, count)"""
    ref, out = RefReward(N), []
    for pred, targ, rew in inputs(N, E, steps):
        r, x, _ = ref.step(pred, targ, WEIGHT, rew)
        out.append((r, ref.ret.copy(), x, ref.mean, ref.var, ref.std, ref.count))
    return out


def check_call(E, pred, targ, ret_in, rew_in, weight, got, where="", gamma=GAMMA, eps=EPS):
    """one call: got = dict(raw, ret, intrinsic, rewards, std) as float32 numpy arrays after the call.  Prints each figure as a fraction of
    its bound, then asserts."""
    r64 = row_norm(pred, targ)
    b_raw = (E + 8) * U * r64
    e_raw = np.abs(got["raw"].astype(np.float64) - r64)
    ret64 = gamma * ret_in.astype(np.float64) + r64
    b_ret = b_raw + 2.0 ** -23 * np.abs(ret64)
    e_ret = np.abs(got["ret"].astype(np.float64) - ret64)
    x64 = weight * got["raw"].astype(np.float64) / (float(got["std"]) + eps)
    e_x = np.abs(got["intrinsic"].astype(np.float64) - x64)
    frac = lambda e, b: float(np.max(np.where(b > 0, e / np.where(b > 0, b, 1.0), np.where(e > 0, np.inf, 0.0))))
    f = (frac(e_raw, b_raw), frac(e_ret, b_ret), frac(e_x, 4 * U * np.abs(x64)))
    if where:
        print(f"rnd {where}: raw {f[0]:.3f}  ret {f[1]:.3f}  intrinsic {f[2]:.3f}  (fractions of the bounds)")
    assert got["raw"].dtype == got["ret"].dtype == got["intrinsic"].dtype == got["rewards"].dtype == np.float32
    assert f[0] <= 1.0, (where, "raw", f)
    assert f[1] <= 1.0, (where, "ret", f)
    assert f[2] <= 1.0, (where, "intrinsic", f)
    want = rew_in.astype(np.float32) + got["intrinsic"]
    assert np.array_equal(got["rewards"].view(np.uint32), want.view(np.uint32)), (where, "rewards")
    return f


def check_sequence(N, E, step_fn, where=""):
    """step_fn(pred, targ, rewards_in, weight) -> dict(raw, ret, intrinsic, rewards, mean, var, std, count) after the call (numpy; the
    implementation keeps ret and the statistics between the calls).  The checks of the module docstring."""
    traj = trajectory(N, E)
    ret_in = np.zeros(N, dtype=np.float32)
    worst, B, worst_traj = np.zeros(3), np.zeros(N), 0.0
    for s, (pred, targ, rew) in enumerate(inputs(N, E)):
        got = step_fn(pred, targ, rew, WEIGHT)
        worst = np.maximum(worst, check_call(E, pred, targ, ret_in, rew, WEIGHT, got))
        assert got["count"].dtype == np.int64 and int(got["count"]) == (s + 1) * N, (where, s, got["count"])
        ret_in = got["ret"].copy()
        B = GAMMA * B + (E + 8) * U * traj[s][0] + 2.0 ** -23 * np.abs(traj[s][1])
        f = float(np.max(np.abs(got["ret"].astype(np.float64) - traj[s][1]) / (B * (1 + 2.0 ** -16))))
        worst_traj = max(worst_traj, f)
        assert f <= 1.0, (where, "ret against the independent trajectory", s, f)
    raw64, ret64, _, m, v, sd, _ = traj[-1]
    drift = float(np.max(np.abs(got["ret"].astype(np.float64) - ret64) / np.abs(ret64)) / U)
    print(f"rnd {where} N={N} E={E}: worst per-call fractions raw {worst[0]:.3f} ret {worst[1]:.3f} intrinsic {worst[2]:.3f}; "
          f"ret against the independent trajectory after {STEPS} steps: {drift:.2f} u, worst fraction of the accumulated bound {worst_traj:.3f}")
    mean, var, std = (float(got[k]) for k in ("mean", "var", "std"))
    y = (ret64 - mean) / (std + obs_norm_ref.EPS_NORM)      # std enters through y: the implementation's own mean and std on the reference's rows
    obs_norm_ref.check(np.full(1, mean), np.full(1, var), y.reshape(-1, 1), ret64.reshape(-1, 1), np.full(1, m), np.full(1, v), np.full(1, sd),
                       where=f"rnd {where} N={N} E={E}")
