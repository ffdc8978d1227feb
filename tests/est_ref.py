"""Float64 restatements for rl/estimator.py (the concurrent state estimator), written from the definition and used by
tests/test_estimator.py and tests/test_estimator_gpu.py: grx_est_forward (copy, layers, column select) and one estimator minibatch step
(mean squared error and its gradient).  numpy only."""
import numpy as np


def elu(z):
    return np.where(z > 0, z, np.expm1(np.minimum(z, 0.0)))


def mlp_ref(weights, biases, x):
    """Linear -> ELU(1) -> ... -> Linear in float64: weights[l] [out][in], biases[l] [out]; returns (output, every layer's input)"""
    h = np.asarray(x, dtype=np.float64)
    inputs = []
    for l, (w, b) in enumerate(zip(weights, biases)):
        inputs.append(h)
        z = h @ np.asarray(w, dtype=np.float64).T + np.asarray(b, dtype=np.float64)
        h = elu(z) if l + 1 < len(weights) else z
    return h, inputs


def est_forward_ref(weights, biases, x, pri=None, cols=None):
    """grx_est_forward: ([x | est(x)], pri[:, cols] or None)"""
    e, _ = mlp_ref(weights, biases, x)
    out = np.concatenate([np.asarray(x, dtype=np.float64), e], axis=1)
    if pri is None:
        return out, None
    return out, np.asarray(pri, dtype=np.float64)[:, list(cols)]


def est_step_ref(weights, biases, x, y):
    """one minibatch: loss = mean over every element of (est(x) - y)^2; returns (loss, d loss / d weights, d loss / d biases)"""
    e, inputs = mlp_ref(weights, biases, x)
    y = np.asarray(y, dtype=np.float64)
    loss = float(np.mean((e - y) ** 2))
    g = 2.0 * (e - y) / e.size
    dws, dbs = [None] * len(weights), [None] * len(weights)
    for l in range(len(weights) - 1, -1, -1):
        dws[l], dbs[l] = g.T @ inputs[l], g.sum(0)
        if l > 0:
            dh = g @ np.asarray(weights[l], dtype=np.float64)
            h = inputs[l]                              # = elu(z) of layer l - 1: elu'(z) = 1 for z > 0, elu(z) + 1 otherwise
            g = dh * np.where(h > 0, 1.0, h + 1.0)
    return loss, dws, dbs
