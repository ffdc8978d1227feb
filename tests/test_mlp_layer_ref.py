"""tests/mlp_layer_ref.py judged on the CPU: its emulated fmaf against rational arithmetic, its chain against a scalar rational chain, and
the chain against the float64 reference within layer_bound on the operands of every GPU test -- so a kernel that misses the chain or the
bound in tests/test_mlp_layer_gpu.py is not missing a reference that is itself off."""
import itertools
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import mlp_layer_ref as R


def _round_f32(q):
    """a rational rounded to the nearest fp32 (ties to even), as a Fraction; normal range only"""
    if q == 0:
        return Fraction(0)
    sign, q = (-1 if q < 0 else 1), abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    assert Fraction(2) ** e <= q < Fraction(2) ** (e + 1) and -126 <= e < 127
    unit = Fraction(2) ** (e - 23)
    n, rest = divmod(q, unit)
    n = int(n)
    if rest * 2 > unit or (rest * 2 == unit and n % 2):
        n += 1
    return sign * n * unit


def _fma_frac(a, b, c):
    return _round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def _assert_fma(a, b, c, tag):
    got = R.fma32(torch.from_numpy(a), torch.from_numpy(b), torch.from_numpy(c)).numpy()
    for i in range(len(a)):
        want = _fma_frac(a[i], b[i], c[i])
        assert Fraction(float(got[i])) == want, (tag, i, float(a[i]), float(b[i]), float(c[i]), float(got[i]), float(want))
    return got


def test_round_f32_is_numpys_rounding():
    rng = np.random.default_rng(0)
    x = rng.standard_normal(2000) * np.exp2(rng.integers(-30, 30, 2000))
    for v in x:
        assert _round_f32(Fraction(float(v))) == Fraction(float(np.float32(v)))


def test_fma32_matches_rational_arithmetic_on_random_triples():
    """12 000 triples: sign and exponent spread over the module's range, the addend from far below the product (absorbed) through
    comparable (cancellation) to far above it"""
    rng = np.random.default_rng(1)
    n = 12000
    a = (rng.standard_normal(n) * np.exp2(rng.integers(-18, 18, n))).astype(np.float32)
    b = (rng.standard_normal(n) * np.exp2(rng.integers(-18, 18, n))).astype(np.float32)
    rel = np.exp2(rng.integers(-30, 30, n))
    rel[: n // 4] = 1.0                                     # a quarter with |c| ~ |a b|: cancellation
    c = (-a.astype(np.float64) * b * rel * (1 + 0.01 * rng.standard_normal(n))).astype(np.float32)
    c[::7] *= -1
    c[::50] = 0.0
    a[5::50] = 0.0
    _assert_fma(a, b, c, "random")


def _midpoint_cases():
    """acc + a b within 2^-70 relative of the fp32 midpoint between A and A + ulp(A), on either side: a = s (1 + 2^-23) 2^i,
    b = (1 - 2^-23) 2^j with a b = s h (1 - 2^-46), h = ulp(A) / 2.  From acc = A the sum is h 2^-46 below the midpoint and rounds to A;
    from acc = A + ulp(A), with s = -1, it is h 2^-46 above it and rounds to A + ulp(A).  A with an even and with an odd mantissa, both
    signs, several binades; the float64 sum acc + a b needs 70 bits and rounds ONTO the midpoint, which ties-to-even then gets wrong
    for one parity."""
    a, b, c, want = [], [], [], []
    for E, mant, sign in itertools.product((-30, -1, 0, 7, 40), (0, 1, 2, 0x7FFFFF, 0x7FFFFE, 0x2AAAAB), (1.0, -1.0)):
        A = (1.0 + mant * 2.0 ** -23) * 2.0 ** E
        ulp = 2.0 ** (E - 23)
        i = (E - 24) // 2
        j = (E - 24) - i
        for acc, s, w in ((A, 1.0, A), (A + ulp, -1.0, A + ulp)):
            a.append(sign * s * (1.0 + 2.0 ** -23) * 2.0 ** i)
            b.append((1.0 - 2.0 ** -23) * 2.0 ** j)
            c.append(sign * acc)
            want.append(sign * w)
    f = lambda v: np.asarray(v, np.float64).astype(np.float32)
    assert all(np.array_equal(f(v).astype(np.float64), np.asarray(v)) for v in (a, b, c, want))   # all fp32 values
    return f(a), f(b), f(c), f(want)


def test_fma32_rounds_once_next_to_a_midpoint():
    a, b, c, want = _midpoint_cases()
    got = _assert_fma(a, b, c, "midpoint")
    assert np.array_equal(got, want)
    exact = [Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z)) for x, y, z in zip(a, b, c)]
    # the cases are what they claim: within 2^-60 relative of the midpoint of two neighbouring fp32 values, and not on it
    for q, w in zip(exact, want):
        mids = [(Fraction(float(w)) + Fraction(float(np.nextafter(w, np.float32(to))))) / 2 for to in (-np.inf, np.inf)]
        d = min(abs(q - m) for m in mids)
        assert 0 < d <= abs(q) * Fraction(2) ** -60
    # ... and they bite: rounding the float64 sum to fp32 (two roundings) gets some of them wrong
    twice = (c.astype(np.float64) + a.astype(np.float64) * b.astype(np.float64)).astype(np.float32)
    assert (twice != want).sum() >= len(want) // 4


def test_fma_chain32_matches_a_scalar_rational_chain():
    X, W, bias = R.operands(3, 70, 3, seed=7)
    for b in (bias, None):
        got = R.fma_chain32(X, W, b)
        for r in range(3):
            for j in range(3):
                acc = Fraction(0)
                for k in range(70):
                    acc = _round_f32(Fraction(float(X[r, k])) * Fraction(float(W[j, k])) + acc)
                if b is not None:
                    acc = _round_f32(acc + Fraction(float(b[j])))
                assert Fraction(float(got[r, j])) == acc, (r, j, b is None)


def test_fma_chain32_differs_from_other_orders():
    """the chain is an ORDER: summing k backwards, or pairwise, gives other bits on ordinary data (so the GPU test that compares bits with it
    does pin the order)"""
    X, W, _ = R.operands(33, 130, 65, seed=3)
    fwd = R.fma_chain32(X, W)
    assert not torch.equal(fwd, R.fma_chain32(X.flip(1), W.flip(1)))
    assert not torch.equal(fwd, (X.unsqueeze(1) * W.unsqueeze(0)).sum(-1))
    assert torch.equal(fwd, R.fma_chain32(X, W))


def _within_bound(X, W, bias, tag):
    chain = R.fma_chain32(X, W, bias)
    err = (chain.double() - R.layer_ref64(X, W, bias, False)).abs()
    bound = R.layer_bound(X, W, bias)
    assert bool((err <= bound).all()), (tag, float((err / bound).max()))
    return float((err / bound.clamp_min(1e-300)).max())


def test_operands_stay_in_the_stated_range():
    for M, K, N in [(129, 193, 129), (4096, 39, 512)]:
        for t in R.operands(M, K, N):
            a = t.abs()
            assert bool(((a == 0) | ((a >= R.TINY) & (a <= R.HUGE))).all())
    t = R._in_range(torch.tensor([1e-7, -1e-7, 2.0 ** -20, 3e6, -3e6, 0.5]))
    assert t.tolist() == [0.0, 0.0, 2.0 ** -20, 2.0 ** 20, -2.0 ** 20, 0.5]


@pytest.mark.parametrize("K", R.EDGE_K)
def test_the_chain_is_inside_the_bound_on_the_k_edge_shapes(K):
    for M, N in R.EDGE_MN:
        X, W, bias = R.operands(M, K, N)
        _within_bound(X, W, bias, (M, K, N))
        _within_bound(X, W, None, (M, K, N, "no bias"))


@pytest.mark.parametrize("K", R.TILE_K)
def test_the_chain_is_inside_the_bound_on_the_tile_edge_shapes(K):
    """the GPU sweep takes X[:M], W[:N] of these operands for every (M, N) in TILE_M x TILE_N: a row's chain depends on that row alone"""
    X, W, bias = R.operands(max(R.TILE_M), K, max(R.TILE_N))
    _within_bound(X, W, bias, K)
    _within_bound(X, W, None, (K, "no bias"))


def test_the_chain_is_inside_the_bound_on_the_alignment_shapes():
    for M, K, N in R.ALIGN_SHAPES:
        X, W, bias = R.operands(M, K, N)
        _within_bound(X, W, bias, (M, K, N))


@pytest.mark.parametrize("shape", R.REAL_SHAPES)
def test_the_chain_is_inside_the_bound_on_the_real_run_shapes(shape):
    M, K, N = shape
    X, W, bias = R.operands(M, K, N)
    _within_bound(X[R.real_rows(M)], W, bias, shape)


def test_ulp_distance():
    a = torch.tensor([1.0, -1.0, 0.0, -0.0, 1.0, -2.0 ** -126])
    b = torch.tensor([1.0 + 2.0 ** -23, -1.0 - 2.0 ** -22, -0.0, 0.0, 1.0, 2.0 ** -126])
    assert R.ulp_distance(a, b).tolist() == [1, 2, 0, 0, 0, 2 * 0x00800000]
