"""A float64 numpy restatement of grx_gae_returns / rl.value_norm, fed fp32 inputs: the GAE scan, the pooled mean and unbiased
std of the advantages, the running update of the returns' statistics, both normalisations and the PopArt rescale -- and the inputs and the
forward-error bounds the CPU tests use.  gamma, lam and eps enter as the fp32 numbers every implementation is handed."""
import numpy as np

GAMMA, LAM, EPS = 0.994, 0.9, 1e-5
PATTERNS = ("none", "all", "random", "last", "first")
U = 2.0 ** -24   # fp32 unit roundoff


def f32(x):
    return float(np.float32(x))


def inputs(T, N, pattern, seed=0):
    """(rewards, values, dones, last_values): rewards in [0, 0.1] with a few large outliers, values around 10 with spread 5"""
    g = np.random.default_rng(1000 * seed + 31 * T + N + 7 * PATTERNS.index(pattern))
    rewards = g.uniform(0.0, 0.1, (T, N))
    out = g.random((T, N)) < 0.02
    rewards[out] += g.uniform(2.0, 20.0, int(out.sum()))
    values = 10.0 + 5.0 * g.standard_normal((T, N))
    last = 10.0 + 5.0 * g.standard_normal(N)
    dones = np.zeros((T, N), np.uint8)
    if pattern == "all":
        dones[:] = 1
    elif pattern == "random":
        dones[g.random((T, N)) < 0.1] = 1
    elif pattern == "last":
        dones[T - 1] = 1
    elif pattern == "first":
        dones[0] = 1
    return rewards.astype(np.float32), values.astype(np.float32), dones, last.astype(np.float32)


def scan(rewards, values, dones, last_values, gamma=GAMMA, lam=LAM):
    """raw returns [T, N] in float64"""
    r, v, d, nxt = (np.asarray(x, np.float64) for x in (rewards, values, dones, last_values))
    gamma, lam = f32(gamma), f32(lam)
    T = r.shape[0]
    ret = np.zeros_like(r)
    adv = np.zeros(r.shape[1])
    for t in range(T - 1, -1, -1):
        alive = 1.0 - d[t]
        delta = r[t] + alive * gamma * nxt - v[t]
        adv = delta + alive * gamma * lam * adv
        ret[t] = adv + v[t]
        nxt = v[t]
    return ret


def pooled(a):
    """(mean, unbiased std); the std of one element is NaN, as torch.std's"""
    a = np.asarray(a, np.float64).ravel()
    return a.mean(), (np.sqrt(((a - a.mean()) ** 2).sum() / (a.size - 1)) if a.size > 1 else float("nan"))


def new_state(eps=EPS):
    return {"count": 0, "mean": 0.0, "var": 1.0, "std": 1.0, "scale": 1.0 + f32(eps)}


def running_update(state, m, v, n, eps=EPS):
    """EmpiricalNormalization's rule on one column; returns the new state"""
    count = state["count"] + n
    rate = n / count
    delta = m - state["mean"]
    mean = state["mean"] + rate * delta
    var = state["var"] + rate * (v - state["var"] + delta * (m - mean))
    std = np.sqrt(var)
    return {"count": count, "mean": mean, "var": var, "std": std, "scale": std + f32(eps)}


def normalise(x, state):
    return (np.asarray(x, np.float64) - state["mean"]) / state["scale"]


def denormalise(x, state):
    return np.asarray(x, np.float64) * state["scale"] + state["mean"]


def popart(W, b, old, new):
    """the output layer after the statistics moved from `old` to `new`"""
    W, b = np.asarray(W, np.float64), np.asarray(b, np.float64)
    return W * old["scale"] / new["scale"], (old["scale"] * b + old["mean"] - new["mean"]) / new["scale"]


def reference(rewards, values, dones, last_values, state=None, gamma=GAMMA, lam=LAM, eps=EPS):
    """everything one call produces.  state None: the stateless mode"""
    ret = scan(rewards, values, dones, last_values, gamma, lam)
    a = ret - np.asarray(values, np.float64)
    mean_a, std_a = pooled(a)
    out = {"returns_raw": ret, "a": a, "advantages": (a - mean_a) / (std_a + 1e-8), "stats": np.array([mean_a, std_a, ret.mean(), ret.var()])}
    if state is not None:
        new = running_update(state, ret.mean(), ret.var(), ret.size, eps)
        out.update(state=new, values=normalise(values, new), returns=normalise(ret, new))
    return out


def bounds(ref, rewards, values, last_values, calls=1):
    """absolute forward-error bounds of an fp32 evaluation of reference()'s formulas, per quantity.  The scan does at most 8 rounded operations
    per step on numbers of magnitude S and contracts (alive gamma lam < 1), a sum or mean of n terms in ANY order errs by at most n u times the
    terms' magnitude (Higham, Accuracy and Stability, 4.2), and every later quantity is a differentiable function of those: its bound is the
    first-order propagation, doubled.  `calls`: how many running updates the state has been through (each adds its own share)."""
    T, n = ref["returns_raw"].shape[0], ref["returns_raw"].size
    S = float(np.abs(rewards).max() + np.abs(values).max() + np.abs(last_values).max() + np.abs(ref["returns_raw"]).max())
    gT, gn = (8 * T + 16) * U, (n + 16) * U
    b_ret = gT * S
    b_mean = 2 * (b_ret + gn * S)                                  # of a, and of the returns
    b_std = 2 * (2 * b_ret + gn * S)                               # |d std| <= sqrt(n / (n - 1)) max |d a| + the sum's share
    s_a = ref["stats"][1]
    out = {"returns_raw": b_ret, "a": b_ret,
           "advantages": 2 * ((b_ret + b_mean) / s_a + np.abs(ref["advantages"]) * (b_std / s_a + 4 * U)),
           "stats": np.array([b_mean, b_std, b_mean, 2 * (2 * S * (b_ret + b_mean) + gn * S * S)])}
    if "state" in ref:
        st = ref["state"]
        b_m, b_v = calls * out["stats"][2] + 8 * U * S, calls * (out["stats"][3] + 4 * S * out["stats"][2]) + 16 * U * S * S
        # |sqrt(v + d) - sqrt(v)| <= min(|d| / (2 sqrt(v)), sqrt(|d|)): the second holds where the variance is (nearly) zero
        b_s = 2 * (min(b_v / (2 * st["std"]) if st["std"] > 0 else float("inf"), float(np.sqrt(b_v))) + 2 * U * st["std"])
        out["state"] = {"mean": b_m, "var": b_v, "std": b_s, "scale": b_s + 2 * U * st["scale"]}
        sc = st["scale"]
        out["values"] = 2 * (b_m / sc + np.abs(ref["values"]) * (out["state"]["scale"] / sc + 4 * U))
        out["returns"] = 2 * ((b_ret + b_m) / sc + np.abs(ref["returns"]) * (out["state"]["scale"] / sc + 4 * U))
    return out
