"""float64 reference of a LayerNorm hidden layer's part behind the matrix product -- ELU(LayerNorm(z)) and its backward --, written from the
formulas of include/grx_ppo_ln.h in numpy, independent of the code under test; the test inputs; and the tolerance rule of the comparisons
with it (tests/test_layer_norm_gpu.py; the rule of tests/test_value_norm_gpu.py).

Tolerance rule: a kernel result may deviate from this reference by FOUR times what the fp32 torch spelling deviates from it on the same
inputs, per shape and per quantity (the largest absolute deviation over the array); the factor covers a different but equally valid
summation order.  The torch spelling's deviation counts as at least half an fp32 unit in the last place of the reference (of its largest
value, for an array): no fp32 number is expected closer to a float64 reference than its own representation error.  For a column sum both
deviations are taken relative to the sum of the terms' magnitudes, column by column -- what the rounding of a sum is proportional to; the
terms have both signs and may cancel."""
import numpy as np

EPS = 1e-5
ROWS = (1, 255, 257, 513)                      # one row; below, above one and above two of the column sums' 256-row slabs
COLS = (1, 3, 64, 65, 130, 512, 1024)          # one column; below, at and above a wave; every count of values per lane (1, 2, 4, 8, 16)


def inputs(rows, cols, seed=0):
    """fp32 arrays of one case: z [rows][cols] whose row 0 is constant (variance 0) and whose row 1 (if there is one) has mean 1e4 and unit
    spread -- what a one-pass variance gets wrong --; the other rows are random and land on both of ELU's branches; gamma, beta [cols];
    dy [rows][cols]"""
    rng = np.random.default_rng(1000 * rows + cols + seed)
    z = rng.standard_normal((rows, cols)).astype(np.float32) * np.float32(1.5) + np.float32(0.3)
    gamma = (0.5 + rng.random(cols)).astype(np.float32)
    beta = (0.5 * rng.standard_normal(cols)).astype(np.float32)
    z[0] = np.float32(0.7)
    if rows > 1:
        z[1] = (1e4 + rng.standard_normal(cols)).astype(np.float32)
    dy = rng.standard_normal((rows, cols)).astype(np.float32)
    return z, gamma, beta, dy


def forward(z, gamma, beta, eps=EPS):
    """(y, mean, rstd, xhat) in float64"""
    z, gamma, beta = (np.asarray(a, dtype=np.float64) for a in (z, gamma, beta))
    C = z.shape[1]
    m = z.sum(1, keepdims=True) / C
    v = ((z - m) ** 2).sum(1, keepdims=True) / C
    s = 1.0 / np.sqrt(v + eps)
    xh = (z - m) * s
    a = gamma * xh + beta
    y = np.where(a > 0, a, np.expm1(np.minimum(a, 0.0)))
    return y, m[:, 0], s[:, 0], xh


def backward(dy, z, gamma, beta, eps=EPS):
    """dz, the three column sums and -- for their relative deviation -- the sums of their terms' magnitudes, in float64"""
    dy, gamma = np.asarray(dy, dtype=np.float64), np.asarray(gamma, dtype=np.float64)
    y, m, s, xh = forward(z, gamma, beta, eps)
    g = dy * np.where(y > 0, 1.0, y + 1.0)
    q = g * gamma
    C = q.shape[1]
    c1 = q.sum(1, keepdims=True) / C
    c2 = (q * xh).sum(1, keepdims=True) / C
    dz = s[:, None] * (q - c1 - xh * c2)
    return {"dz": dz, "dbeta": g.sum(0), "dgamma": (g * xh).sum(0), "dbias": dz.sum(0),
            "scale": {"dbeta": np.abs(g).sum(0), "dgamma": np.abs(g * xh).sum(0), "dbias": np.abs(dz).sum(0)}}


def half_ulp(ref):
    """half an fp32 unit in the last place of the largest |ref|"""
    big = float(np.max(np.abs(ref))) if np.size(ref) else 0.0
    return 0.5 * float(np.spacing(np.float32(big)))


def deviation(got, ref, scale=None):
    """the largest |got - ref| (scale None), or the largest |got - ref| / scale over the columns (a column sum; a column of zero terms must
    be exact)"""
    d = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64))
    if scale is None:
        return float(d.max())
    safe = np.where(scale > 0, scale, 1.0)
    return float(np.where(scale > 0, d / safe, np.where(d > 0, np.inf, 0.0)).max())


def floor(ref, scale=None):
    """the least deviation the torch spelling is counted with: half an fp32 ulp of the reference, in `deviation`'s units"""
    if scale is None:
        return half_ulp(ref)
    ref, safe = np.abs(np.asarray(ref, dtype=np.float64)), np.where(scale > 0, scale, 1.0)
    h = 0.5 * np.spacing(ref.astype(np.float32)).astype(np.float64)
    return float(np.where(scale > 0, h / safe, 0.0).max())


def within(got, torch_spelling, ref, scale=None):
    """(ok, kernel deviation, torch deviation with its floor): the tolerance rule"""
    dh, dt = deviation(got, ref, scale), max(deviation(torch_spelling, ref, scale), floor(ref, scale))
    return dh <= 4.0 * dt, dh, dt
