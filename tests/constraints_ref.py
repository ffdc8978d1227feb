"""A float64 numpy restatement of constraints as terminations (rl/constraints.py, include/grx_ppo_cat.h), with explicit loops
and fed fp32 inputs: the per-column violations, the running column maxima, the termination probabilities, the reward row, the previous
action rows, the counters, and the returns -- and the inputs the tests use.  tau, 1 - tau, gamma and lam enter as the fp32 numbers every
implementation is handed; the limits enter as the fp32 numbers the column table holds."""
import numpy as np

FAMILIES = ("torque", "dof_vel", "dof_pos", "action_rate", "upright")
GAMMA, LAM = 0.994, 0.9
U = 2.0 ** -24   # fp32 unit roundoff


def f32(x):
    return float(np.float32(x))


def columns(families, D, A, torque_limits=None, dof_vel_limits=None, dof_pos_limits=None, soft_torque=1.0, soft_vel=1.0):
    """[(kind, src, family, lo, hi)] for `families`, a list of (name, limit or None): the spec's order, one column per DOF / action / one"""
    cols = []
    for f, (name, limit) in enumerate(families):
        k = FAMILIES.index(name)
        if name == "torque":
            cols += [(k, j, f, 0.0, f32(np.float32(torque_limits[j]) * np.float32(soft_torque))) for j in range(D)]
        elif name == "dof_vel":
            cols += [(k, j, f, 0.0, f32(np.float32(dof_vel_limits[j]) * np.float32(soft_vel))) for j in range(D)]
        elif name == "dof_pos":
            cols += [(k, j, f, f32(dof_pos_limits[j][0]), f32(dof_pos_limits[j][1])) for j in range(D)]
        elif name == "action_rate":
            cols += [(k, j, f, 0.0, f32(limit)) for j in range(A)]
        else:
            cols += [(k, 0, f, 0.0, f32(limit))]
    return cols


def violation(col, n, src, prev):
    """c of one (env, column) in float64"""
    kind, j, _, lo, hi = col
    if kind == 0:
        return abs(float(src["torques"][n, j])) - hi
    if kind == 1:
        return abs(float(src["dof_vel"][n, j])) - hi
    if kind == 2:
        q = float(src["dof_pos"][n, j])
        return max(lo - q, q - hi)
    if kind == 3:
        return abs(float(src["actions"][n, j]) - float(prev[n, j])) - hi
    gx, gy = float(src["gravity"][n, 0]), float(src["gravity"][n, 1])
    return float(np.sqrt(gx * gx + gy * gy)) - hi


def step(cols, num_families, prob, src, dones, state, tau, reward_row, clip_zero=True, reset_counts=False):
    """one rollout step.  state: {"c_max": [C], "prev": [N, A] or None, "counts": [F]}, float64 / int; returns
    (cplus [N, C], delta [N], new reward row [N], new state)"""
    N, C = len(dones), len(cols)
    tau, omt = f32(tau), f32(np.float32(1.0) - np.float32(tau))
    cplus = np.zeros((N, C))
    for n in range(N):
        for c in range(C):
            v = violation(cols[c], n, src, state["prev"])
            cplus[n, c] = 0.0 if dones[n] else max(v, 0.0)
    c_max = np.zeros(C)
    for c in range(C):
        m = 0.0
        for n in range(N):
            m = max(m, cplus[n, c])
        c_max[c] = tau * state["c_max"][c] + omt * m
    counts = np.zeros(num_families, np.int64) if reset_counts else np.array(state["counts"], np.int64)
    for n in range(N):
        for f in range(num_families):
            counts[f] += int(any(cplus[n, c] > 0 for c in range(C) if cols[c][2] == f))
    delta, row = np.zeros(N), np.zeros(N)
    for n in range(N):
        for c in range(C):
            if c_max[c] > 0:
                delta[n] = max(delta[n], float(prob[c]) * min(max(cplus[n, c] / c_max[c], 0.0), 1.0))
        r = float(reward_row[n])
        row[n] = (1.0 - delta[n]) * (max(r, 0.0) if clip_zero else r)
    prev = None
    if state["prev"] is not None:
        prev = np.array(src["actions"], np.float64)
        prev[np.asarray(dones) != 0] = 0.0
    return cplus, delta, row, {"c_max": c_max, "prev": prev, "counts": counts}


def returns(rewards, values, dones, term_prob, last_values, gamma=GAMMA, lam=LAM):
    """raw returns [T, N] in float64: RolloutStorage.compute_returns' loop with alive = (1 - done)(1 - delta)"""
    r, v, d, p, nxt = (np.asarray(x, np.float64) for x in (rewards, values, dones, term_prob, last_values))
    gamma, lam = f32(gamma), f32(lam)
    T, N = r.shape
    ret = np.zeros_like(r)
    for n in range(N):
        adv, nx = 0.0, nxt[n]
        for t in range(T - 1, -1, -1):
            alive = (1.0 - d[t, n]) * (1.0 - p[t, n])
            delta = r[t, n] + alive * gamma * nx - v[t, n]
            adv = delta + alive * gamma * lam * adv
            ret[t, n] = adv + v[t, n]
            nx = v[t, n]
    return ret


def advantages(ret, values):
    """(advantages, [mean, unbiased std of a, mean, population variance of the returns])"""
    a = ret - np.asarray(values, np.float64)
    mean = a.mean()
    std = np.sqrt(((a - mean) ** 2).sum() / (a.size - 1)) if a.size > 1 else float("nan")
    return (a - mean) / (std + 1e-8), np.array([mean, std, ret.mean(), ret.var()])


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------
def limits(D, seed=0):
    """(torque_limits [D], dof_vel_limits [D], dof_pos_limits [D, 2]) in fp32"""
    g = np.random.default_rng(77 + seed)
    lo = -g.uniform(0.3, 1.5, D)
    return (g.uniform(30.0, 150.0, D).astype(np.float32), g.uniform(5.0, 15.0, D).astype(np.float32),
            np.stack([lo, lo + g.uniform(1.0, 3.0, D)], 1).astype(np.float32))


def sources(N, D, A, lims, rate_limit, upright_limit, step_no, seed=0, share=0.1, quiet_column=None):
    """one step's env tensors in fp32, drawn so that roughly `share` of the entries of every family violate: a value sits inside its limit
    scaled by u < 1, or outside scaled by 1 + e.  `quiet_column` (a DOF): never violated in torque, dof_vel and dof_pos.
    Returns ({"torques", "dof_vel", "dof_pos", "actions", "gravity"}, dones [N] uint8)."""
    g = np.random.default_rng(1000 * seed + 131 * N + 17 * D + A + 7919 * step_no)
    tl, vl, pl = lims

    def scaled(limit, width):
        out = g.random((N, width)) < share
        mag = np.where(out, 1.0 + g.uniform(0.01, 0.5, (N, width)), g.uniform(0.0, 0.95, (N, width)))
        if quiet_column is not None and quiet_column < width:
            mag[:, quiet_column] = np.minimum(mag[:, quiet_column], 0.9)
        return (g.choice([-1.0, 1.0], (N, width)) * mag * limit).astype(np.float32)
    mid, half = (pl[:, 0] + pl[:, 1]) / 2, (pl[:, 1] - pl[:, 0]) / 2
    pos = mid + scaled(half, D)
    # fresh N(0, s) actions every step: a_t - a_{t-1} is N(0, 2 s^2), and P(|x| > 1.645 sigma) = 0.1 (against prev = 0 it is less)
    actions = (g.standard_normal((N, A)) * rate_limit / 1.645 / np.sqrt(2.0)).astype(np.float32)
    tilt = np.where(g.random(N) < share, upright_limit * (1.0 + g.uniform(0.01, 0.3, N)), upright_limit * g.uniform(0.0, 0.95, N))
    ang = g.uniform(0, 2 * np.pi, N)
    grav = np.stack([tilt * np.cos(ang), tilt * np.sin(ang), -np.sqrt(np.maximum(1.0 - tilt ** 2, 0.0))], 1).astype(np.float32)
    dones = (g.random(N) < 0.15).astype(np.uint8)
    return {"torques": scaled(tl, D), "dof_vel": scaled(vl, D), "dof_pos": pos.astype(np.float32), "actions": actions, "gravity": grav}, dones


def rollout(T, N, seed=0, exact=True):
    """(rewards, values, dones, term_prob, last_values) in fp32: tests/gae_ref.py's magnitudes, dones at random, term_prob uniform in
    [0, 1] with exact zeros and ones mixed in"""
    g = np.random.default_rng(500 * seed + 31 * T + N)
    rewards = g.uniform(-0.05, 0.1, (T, N))
    values = 10.0 + 5.0 * g.standard_normal((T, N))
    last = 10.0 + 5.0 * g.standard_normal(N)
    dones = (g.random((T, N)) < 0.1).astype(np.uint8)
    p = g.random((T, N))
    if exact:
        pick = g.random((T, N))
        p[pick < 0.3] = 0.0
        p[pick > 0.9] = 1.0
    return rewards.astype(np.float32), values.astype(np.float32), dones, p.astype(np.float32), last.astype(np.float32)
