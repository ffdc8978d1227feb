"""A float64 numpy statement of multi-critic PPO's three operations, written from the formulas and independent of
rl/multi_critic.py: the group rewards of one rollout step with the per-head time-out bootstrap, the per-group GAE with per-group
advantage normalisation and the weighted sum, and the PPO loss with one value loss per head and its gradients -- fed the fp32 inputs every
implementation is handed.  Plus the inputs the tests share, and the way an fp32 result is held against these numbers."""
import numpy as np

from tests import lstm_ref

GAMMA, LAM = 0.994, 0.9
U = 2.0 ** -24   # fp32 unit roundoff
MARGIN = 4.0     # tests/test_recurrent_gpu.py's: "a different but equally good fp32 evaluation order"


def f32(x):
    return float(np.float32(x))


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------
def dones(T, N):
    """tests/lstm_ref.py's pattern (an env that ends at the first step, one at the last, one twice in a row, one never, one at every
    step), its six rows cycled over T steps, its last row always the rollout's last: [T, N] uint8"""
    d = lstm_ref.dones(N)
    rows = [t % 6 for t in range(T - 1)] + [5]
    return d[rows].copy()


def rollout(T, N, K, seed=0):
    """(rewards [T, N, K], values [T, N, K], dones [T, N], last_values [N, K]): group k's rewards and values live at a scale of 4^-k"""
    g = np.random.default_rng(1000 * seed + 97 * T + 13 * N + K)
    scale = 4.0 ** -np.arange(K)
    rewards = g.uniform(-0.05, 0.1, (T, N, K)) * scale
    rewards[g.random((T, N, K)) < 0.05] += 2.0
    values = (10.0 + 5.0 * g.standard_normal((T, N, K))) * scale
    last = (10.0 + 5.0 * g.standard_normal((N, K))) * scale
    return rewards.astype(np.float32), values.astype(np.float32), dones(T, N), last.astype(np.float32)


def weights(K):
    return [f32(0.5 + 0.75 * k) for k in range(K)]


def tables(N, NT, NB, K, seed=0):
    """(terms [NT, N], base_terms [NB, N] or None, term_group [NT + NB], values [N, K], time_outs [N]): terms of very different scale and
    both signs, about a third of the rows inactive (-1), every group fed by at least one row where there are rows enough"""
    g = np.random.default_rng(7 * seed + 31 * N + NT + 3 * NB + K)
    rows = NT + NB
    terms = (g.standard_normal((rows, N)) * 10.0 ** g.integers(-4, 1, (rows, 1))).astype(np.float32)
    group = g.integers(0, K, rows)
    group[g.random(rows) < 0.33] = -1
    for k in range(min(K, rows)):
        group[(k * 5) % rows] = k
    values = (10.0 * g.standard_normal((N, K))).astype(np.float32)
    to = (g.random(N) < 0.3).astype(np.uint8)
    return terms[:NT].copy(), (terms[NT:].copy() if NB else None), group.astype(np.int32), values, to


def minibatch(B, A, K, seed=0):
    """the inputs of one loss call, as a dict of fp32 arrays: ratios around 1 on both sides of the clip, value errors on both sides of it"""
    g = np.random.default_rng(11 * seed + 5 * B + 3 * A + K)
    f = lambda x: np.asarray(x, np.float32)
    std = f(g.uniform(0.3, 1.2, A))
    mu = f(g.standard_normal((B, A)))
    old_mu = f(mu + 0.05 * g.standard_normal((B, A)))
    old_sigma = f(std * g.uniform(0.9, 1.1, (B, A)))
    actions = f(old_mu + old_sigma * g.standard_normal((B, A)))
    old_logp = f((-(actions - old_mu) ** 2 / (2 * old_sigma ** 2) - np.log(old_sigma) - 0.5 * np.log(2 * np.pi)).sum(1))
    scale = 4.0 ** -np.arange(K)
    tv = f((10.0 + 5.0 * g.standard_normal((B, K))) * scale)
    value = f(tv + 0.3 * g.standard_normal((B, K)) * scale)
    returns = f(tv + 1.0 * g.standard_normal((B, K)) * scale)
    return {"mu": mu, "std": std, "value": value, "actions": actions, "old_logp": old_logp, "old_mu": old_mu, "old_sigma": old_sigma,
            "advantages": f(g.standard_normal(B)), "returns": returns, "target_values": tv}


# ---- the three operations ----------------------------------------------------------------------------------------------------------------------
def store(terms, base_terms, term_group, values, to, gamma=GAMMA):
    """(st_values [N, K], st_rewards [N, K], group sums before the bootstrap [N, K], sum of the absolute term values per env [N])"""
    v = np.asarray(values, np.float64)
    N, K = v.shape
    table = np.asarray(terms, np.float64) if base_terms is None else np.concatenate([np.asarray(terms, np.float64), np.asarray(base_terms, np.float64)])
    sums, mag = np.zeros((N, K)), np.zeros(N)
    for t, g in enumerate(term_group[:table.shape[0]]):
        if g < 0:
            continue
        sums[:, g] += table[t]
        mag += np.abs(table[t])
    r = sums.copy()
    if to is not None:
        for n in range(N):
            if to[n]:
                r[n] += f32(gamma) * v[n]
    return v, r, sums, mag


def returns(rewards, values, d, last_values, w, gamma=GAMMA, lam=LAM):
    """{returns [T, N, K], a [T, N, K], stats [K, 2], normalised [T, N, K], advantages [T, N]}"""
    r, v, last = (np.asarray(x, np.float64) for x in (rewards, values, last_values))
    T, N, K = r.shape
    gamma, lam = f32(gamma), f32(lam)
    ret = np.zeros((T, N, K))
    for k in range(K):
        for n in range(N):
            nxt, adv = last[n, k], 0.0
            for t in range(T - 1, -1, -1):
                alive = 1.0 - float(d[t, n])
                delta = r[t, n, k] + alive * gamma * nxt - v[t, n, k]
                adv = delta + alive * gamma * lam * adv
                ret[t, n, k] = adv + v[t, n, k]
                nxt = v[t, n, k]
    a = ret - v
    stats, norm, total = np.zeros((K, 2)), np.zeros((T, N, K)), np.zeros((T, N))
    for k in range(K):
        m = a[..., k].mean()
        s = np.std(a[..., k], ddof=1) if T * N > 1 else float("nan")
        stats[k] = (m, s)
        norm[..., k] = (a[..., k] - m) / (s + 1e-8)
        total += float(w[k]) * norm[..., k]
    return {"returns": ret, "a": a, "stats": stats, "normalised": norm, "advantages": total}


def loss(b, clip=0.2, vcoef=1.0, ecoef=0.01, use_clipped=True):
    """{out [4 + K], d_mu [B, A], d_std [A], d_value [B, K]} of the minibatch dict `b`; no input of minibatch() sits on a tie of a max or
    on an edge of a clamp, so the gradients are the one-sided ones"""
    x = {k: np.asarray(v, np.float64) for k, v in b.items()}
    mu, std, act = x["mu"], x["std"], x["actions"]
    B, A = mu.shape
    K = x["value"].shape[1]
    clip, vcoef, ecoef = f32(clip), f32(vcoef), f32(ecoef)
    logp = (-(act - mu) ** 2 / (2 * std ** 2) - np.log(std) - 0.5 * np.log(2 * np.pi)).sum(1)
    kl = (np.log(std / x["old_sigma"] + f32(1e-5)) + (x["old_sigma"] ** 2 + (x["old_mu"] - mu) ** 2) / (2 * std ** 2) - 0.5).sum(1)
    ratio = np.exp(logp - x["old_logp"])
    adv = x["advantages"]
    clipped_ratio = np.clip(ratio, 1.0 - clip, 1.0 + clip)
    s1, s2 = -adv * ratio, -adv * clipped_ratio
    surrogate = np.maximum(s1, s2).mean()
    inside = (ratio >= 1.0 - clip) & (ratio <= 1.0 + clip)
    g_ratio = np.where(s1 > s2, -adv, np.where(inside, -adv, 0.0))
    g_logp = g_ratio * ratio / B
    d_mu = g_logp[:, None] * (act - mu) / std ** 2
    d_std = (g_logp[:, None] * ((act - mu) ** 2 / std ** 3 - 1.0 / std)).sum(0) - ecoef / std
    heads, d_value = np.zeros(K), np.zeros((B, K))
    for k in range(K):
        v, ret, tv = x["value"][:, k], x["returns"][:, k], x["target_values"][:, k]
        if use_clipped:
            vc = tv + np.clip(v - tv, -clip, clip)
            l1, l2 = (v - ret) ** 2, (vc - ret) ** 2
            heads[k] = np.maximum(l1, l2).mean()
            in_v = np.abs(v - tv) <= clip
            gv = np.where(l1 > l2, 2 * (v - ret), np.where(in_v, 2 * (vc - ret), 0.0))
        else:
            heads[k] = ((ret - v) ** 2).mean()
            gv = -2 * (ret - v)
        d_value[:, k] = vcoef * gv / B
    value_loss = heads.sum()
    entropy = (0.5 + 0.5 * np.log(2 * np.pi) + np.log(std)).sum()
    total = surrogate + vcoef * value_loss - ecoef * entropy
    return {"out": np.concatenate([[surrogate, value_loss, total, kl.mean()], heads]), "d_mu": d_mu, "d_std": d_std, "d_value": d_value}


def loss_chain_bounds(b, ref, clip=0.2, ecoef=0.01):
    """Forward-error bounds of grx_ppo_loss's fp32 evaluation of the policy side, for what the 4x margin over torch's error cannot hold
    (the kernel adds a row's A log-probability terms in ONE fp32 chain, and byte equality with grx_ppo_loss at K = 1 forbids another sum).
    u = 2^-24, first order, every count rounded up:
      term k of a row   t = -(df^2) / (2 s^2) - log s - c, with q = df^2 / (2 s^2), l = |log s|, c = 0.5 log 2 pi:  df one rounding, its
                        square, the denominator and the quotient four more (5 u q), logf within 2 ulp (4 u l), the two subtractions and
                        the constant's own rounding (2 u (q + l + c)):  at most 7 u (q + l + c)
      the chain         A additions, each rounding a partial sum no larger than T = sum_k (q + l + c):  A u T
      so                |d logp| <= (A + 8) u T      (one u T of head room for the second-order terms)
      ratio             exp(logp - old_logp): the difference rounds (u |logp - old_logp|), expf is within 2 ulp (4 u):
                        rho = (A + 8) u T + u |logp - old_logp| + 4 u, relative
      surrogate         max and clamp are 1-Lipschitz in the ratio: a row errs by at most |adv| max(ratio, 1 + clip) (rho + 2 u); the batch
                        mean is taken in float64 and rounded once: + u |surrogate|
      d_mu[i][k]        g_logp = (-adv or 0) ratio / B, times df / s^2: eight more roundings: |d_mu| (rho + 8 u) -- for a row whose ratio is
                        not within rho of an edge of the clip (there the gradient jumps; such rows are returned in `edge`, not bounded)
      d_std[k]          sum_i g_i (x_i - y) - ecoef / s_k, x = df^2 / s^3 (seven roundings), y = 1 / s (one), their difference one, g_i
                        within rho + 3 u and the product one more:  sum_i |g_i| ((rho_i + 5 u) |x_i - y| + 7 u (x_i + y)); the sum is
                        float64, the rest three roundings: + 3 u (|sum| + ecoef / s_k); an `edge` row's whole term may be there or not:
                        + |adv_i| ratio_i / B |x_i - y| for those
    Returns {"surrogate": float, "d_mu": [B, A], "d_std": [A], "edge": bool [B]}."""
    x = {k: np.asarray(v, np.float64) for k, v in b.items()}
    mu, std, act, adv = x["mu"], x["std"], x["actions"], x["advantages"]
    B, A = mu.shape
    clip, ecoef = f32(clip), f32(ecoef)
    df = act - mu
    q, l, c = df ** 2 / (2 * std ** 2), np.abs(np.log(std)) * np.ones_like(df), 0.5 * np.log(2 * np.pi)
    T = (q + l + c).sum(1)
    logp = (-q - np.log(std) - c).sum(1)
    d = logp - x["old_logp"]
    ratio = np.exp(d)
    rho = (A + 8) * U * T + U * np.abs(d) + 4 * U
    edge = (np.abs(ratio - (1.0 - clip)) <= 2 * rho * ratio + 4 * U) | (np.abs(ratio - (1.0 + clip)) <= 2 * rho * ratio + 4 * U)
    surrogate = float((np.abs(adv) * np.maximum(ratio, 1.0 + clip) * (rho + 2 * U)).mean() + U * abs(ref["out"][0]))
    d_mu = np.abs(ref["d_mu"]) * (rho + 8 * U)[:, None]
    inside = (ratio >= 1.0 - clip) & (ratio <= 1.0 + clip)
    takes = (-adv * ratio > -adv * np.clip(ratio, 1.0 - clip, 1.0 + clip)) | inside
    g = np.where(takes, np.abs(adv) * ratio / B, 0.0)
    xs, y = df ** 2 / std ** 3, 1.0 / std
    rows = g[:, None] * ((rho + 5 * U)[:, None] * np.abs(xs - y) + 7 * U * (xs + y))
    rows[edge] = (np.abs(adv) * ratio / B)[edge, None] * np.abs(xs - y)[edge]
    total = (np.where(takes, -adv * ratio / B, 0.0)[:, None] * (xs - y)).sum(0)
    d_std = rows.sum(0) + 3 * U * (np.abs(total) + ecoef / std)
    return {"surrogate": surrogate, "d_mu": d_mu, "d_std": d_std, "edge": edge}


# ---- holding an fp32 result against float64 ----------------------------------------------------------------------------------------------------
def held(got, fp32_torch, want):
    """(error, e32, ratio) of `got` against the float64 `want`, e32 the error of the fp32 torch spelling of the same operation evaluated on
    the CPU against the same float64 values: max |.| over the tensor, as tests/test_recurrent_gpu.py holds the LSTM cell.  An e32 counts as at
    least half an fp32 ulp of the reference's largest magnitude: a one-number quantity's torch error can be zero by luck, and no fp32
    evaluation is asked to be better than its own output rounding.  NaNs must sit in the same places."""
    got, ref32, want = (np.asarray(a, np.float64) for a in (got, fp32_torch, want))
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(np.isnan(ref32), nan), "NaNs differ"
    if nan.all():
        return 0.0, 0.0, 0.0
    floor = U * float(np.abs(want[~nan]).max())   # (u |x| is at most half an ulp of x)
    e32 = max(float(np.abs(ref32 - want)[~nan].max()), floor)
    err = float(np.abs(got - want)[~nan].max())
    return err, e32, (err / e32 if e32 > 0 else 0.0)
