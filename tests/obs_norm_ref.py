"""float64 numpy statement of the empirical observation normaliser (rl/normalizer.py), the inputs of its numeric tests
and their bounds.  Shared by tests/test_obs_norm.py and tests/test_obs_norm_gpu.py."""
import functools

import numpy as np

EPS_NORM = 1e-2            # the normaliser's eps
EPS = 2.0 ** -23           # float32 machine epsilon
STEPS = 30


class RefNormalizer:
    def __init__(self, D, eps=EPS_NORM, count=0):
        self.count = int(count)
        self.mean, self.var, self.std, self.eps = np.zeros(D), np.ones(D), np.ones(D), eps

    def update(self, x):
        x = np.asarray(x, dtype=np.float64)
        n = x.shape[0]
        self.count += n
        rate = n / self.count
        mean_x, var_x = x.mean(0), x.var(0)
        delta = mean_x - self.mean
        self.mean = self.mean + rate * delta
        self.var = self.var + rate * (var_x - self.var + delta * (mean_x - self.mean))
        self.std = np.sqrt(self.var)

    def normalize(self, x):
        return (np.asarray(x, dtype=np.float64) - self.mean) / (self.std + self.eps)

    def forward(self, x, training=True):
        if training:
            self.update(x)
        return self.normalize(x)


@functools.lru_cache(maxsize=None)
def batches(rows, D, steps=STEPS):
    """the numeric tests' inputs: column c has offset linspace(-50, 50)[c] and spread geomspace(0.02, 20)[c], drifting with the step"""
    rng = np.random.default_rng(0)
    off, sd = np.linspace(-50, 50, D), np.geomspace(0.02, 20, D)
    out = [np.float32(off + sd * rng.standard_normal((rows, D)) + 0.01 * step * sd) for step in range(steps)]
    for b in out:
        b.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def reference(rows, D, steps=STEPS):
    """the reference's state after every step, float64: a list of (mean, var, std, count) (check() forms y from them)"""
    ref, out = RefNormalizer(D), []
    for x in batches(rows, D, steps):
        ref.update(x)
        out.append((ref.mean.copy(), ref.var.copy(), ref.std.copy(), ref.count))
    return out


def check(mean, var, y, x, m, v, s, where=""):
    """The bounds: the state is float32, one rounding of a stored mean costs EPS |m|; 16 covers 30 accumulated updates and the
    reduction tree.  Prints each figure as a fraction of its bound, then asserts."""
    mean, var, y = (np.asarray(a, dtype=np.float64).reshape(np.shape(r)) for a, r in ((mean, m), (var, v), (y, x)))
    x = np.asarray(x, dtype=np.float64)
    b_mean = np.maximum(16 * EPS * (np.abs(m) + s), EPS)
    b_var = np.maximum(16 * EPS * (np.abs(m) * s + v), EPS)
    b_y = np.maximum(16 * EPS * (np.abs(m) + np.abs(x - m) + s) / (s + EPS_NORM), EPS)
    y_ref = (x - m) / (s + EPS_NORM)
    f = [float((np.abs(mean - m) / b_mean).max()), float((np.abs(var - v) / b_var).max()), float((np.abs(y - y_ref) / b_y).max())]
    print(f"obs_norm {where}: mean {f[0]:.3f}  var {f[1]:.3f}  y {f[2]:.3f}  (fractions of the bounds)")
    assert f[0] <= 1.0, (where, "mean", f)
    assert f[1] <= 1.0, (where, "var", f)
    assert f[2] <= 1.0, (where, "y", f)
    return f
