"""Float64 numpy restatement of policy distillation's two operations (rl/distillation.py), written from their definitions:

    loss:   d = student - teacher over all n = batch x actions elements
            mse:    loss = sum d^2 / n,                                     d loss / d student = 2 d / n
            huber:  loss = sum (|d| <= 1 ? d^2 / 2 : |d| - 1/2) / n,        d loss / d student = clamp(d, -1, 1) / n      (delta = 1)
    store:  the storage rows of this step = (student input rows, label rows, dones != 0); with the logging arrays:
            cur_rew += rewards; cur_len += 1; where done: done_rew = cur_rew, done_len = cur_len, then cur_rew = cur_len = 0;
            done_rew / done_len untouched elsewhere
"""
import numpy as np

EPS = float(np.finfo(np.float32).eps)           # 2^-23
TINY = float(np.finfo(np.float32).smallest_subnormal)
LOSSES = ("mse", "huber")


def loss_and_grad(student, teacher, loss_type):
    s, t = np.asarray(student, dtype=np.float64), np.asarray(teacher, dtype=np.float64)
    d = s - t
    n = d.size
    if loss_type == "mse":
        return float((d * d).sum() / n), 2.0 * d / n
    assert loss_type == "huber"
    a = np.abs(d)
    e = np.where(a <= 1.0, 0.5 * d * d, a - 0.5)
    return float(e.sum() / n), np.clip(d, -1.0, 1.0) / n


def loss_inputs(batch, A, seed=0):
    """student / teacher means (float32) whose |difference| lies on both sides of the Huber delta, and -- where the batch has room -- exactly
    on it (both signs) and exactly zero"""
    g = np.random.default_rng(1000 * seed + 31 * batch + A)
    t = g.standard_normal((batch, A)).astype(np.float32)
    d = (g.standard_normal((batch, A)) * np.where(g.random((batch, A)) < 0.5, 0.3, 2.5)).astype(np.float32)
    s = (t + d).astype(np.float32)
    flat_s, flat_t = s.reshape(-1), t.reshape(-1)
    for k, delta in enumerate((1.0, -1.0, 0.0)):
        if k < flat_s.size:                      # exactly representable: t is a small integer there
            flat_t[k] = np.float32(k - 1)
            flat_s[k] = np.float32(k - 1 + delta)
    return s, t


def grad_bound(want):
    """|fp32 gradient - want| allowed: one subtraction and one product with a rounded constant -- 2^-22 relative, plus one fp32 denormal"""
    return np.abs(want) * 2.0 ** -22 + TINY


def store(st_obs, st_labels, st_dones, obs, labels, dones, rewards=None, log=None):
    """one step: the three storage rows (modified in place) and, log = [cur_rew, cur_len, done_rew, done_len] float32 arrays, the episode
    bookkeeping (in place too)"""
    done = np.asarray(dones).reshape(-1) != 0
    st_obs[...] = obs
    st_labels[...] = labels
    st_dones[...] = done.astype(np.uint8).reshape(st_dones.shape)
    if log is not None:
        cur_rew, cur_len, done_rew, done_len = log
        cur_rew += np.asarray(rewards, dtype=np.float32)
        cur_len += np.float32(1.0)
        done_rew[done] = cur_rew[done]
        done_len[done] = cur_len[done]
        cur_rew[done] = 0.0
        cur_len[done] = 0.0


def store_inputs(N, D, A, pattern, seed=0):
    """rows, labels, rewards, dones ("none" / "all" / "mixed") and the four logging arrays before the step"""
    g = np.random.default_rng(7 + 1000 * seed + 100 * N + 10 * D + A)
    obs = g.standard_normal((N, D)).astype(np.float32)
    labels = g.standard_normal((N, A)).astype(np.float32)
    rewards = g.standard_normal(N).astype(np.float32)
    dones = {"none": np.zeros(N, bool), "all": np.ones(N, bool), "mixed": np.arange(N) % 3 == 0}[pattern]
    log = [g.standard_normal(N).astype(np.float32), g.integers(0, 50, N).astype(np.float32),
           g.standard_normal(N).astype(np.float32), g.integers(0, 50, N).astype(np.float32)]
    return obs, labels, rewards, dones, log


def mlp(x, weights, biases):
    """Linear -> ELU(1) -> ... -> Linear in float64 (the teacher / the student on their stacked, normalised rows)"""
    x = np.asarray(x, dtype=np.float64)
    for i, (w, b) in enumerate(zip(weights, biases)):
        x = x @ np.asarray(w, dtype=np.float64).T + np.asarray(b, dtype=np.float64)
        if i + 1 < len(weights):
            x = np.where(x > 0, x, np.expm1(np.minimum(x, 0.0)))
    return x
