"""References for grx_mlp_layer (csrc/grx_ppo.hip, mlp_layer_kernel), the f32-input MFMA layer every forward of the default path runs
through: Y = act(X W^T + bias), X [M, K], W [N, K], bias [N] or None.

Three of them, so that a failure says what kind of difference it is:
  * layer_ref64: the operation in float64 -- what the VALUE has to be;
  * layer_bound: what an fp32 evaluation that sums k one after another may be off by, per element;
  * fma_chain32: the exact fp32 result of ONE evaluation order, acc = fmaf(X[r, k], W[j, k], acc) for k = 0 .. K - 1 from acc = 0, then
    one fp32 add of the bias -- what the BITS have to be while the kernel sums in that order.
tests/test_mlp_layer_ref.py checks the third against rational arithmetic and against the first two on the CPU; tests/test_mlp_layer_gpu.py
holds the kernel to all three.  The shapes and operands of the GPU tests are defined here, so that the CPU tests see the same data.

Operands keep |x|, |w| in [2^-20, 2^20] or zero: then no product (>= 2^-40, 48 bits) and no partial sum (a multiple of 2^-87) is
subnormal or overflows, and what the matrix cores do with subnormals does not enter."""
import itertools
import math

import torch

from tests.ppo_ref import U32

TINY, HUGE = 2.0 ** -20, 2.0 ** 20

# ---- the shapes of tests/test_mlp_layer_gpu.py (a 64 x 64 output tile, a 32 x 32 MFMA tile per wave, K chunks of 64, two LDS buffers) ----
EDGE_K = (1, 2, 3, 4, 63, 64, 65, 127, 128, 129, 130, 192, 193)
EDGE_MN = ((1, 1), (33, 65), (65, 33), (64, 64), (129, 96))
TILE_K = (65, 130)
TILE_M = (1, 31, 32, 33, 63, 64, 65, 129)
TILE_N = (1, 31, 32, 33, 63, 64, 65, 127, 129)
REAL_SHAPES = ((4096, 39, 512), (4096, 168, 512), (4096, 512, 256), (4096, 256, 128), (4096, 128, 10), (4096, 128, 1), (10485, 234, 512))
ALIGN_SHAPES = ((70, 128, 97), (70, 64, 97))      # K % 4 == 0: the float4 loads are eligible
INTEGER_SHAPES =((70, 33, 64), (129, 193, 65), (5, 1, 10), (200, 512, 130))


def real_rows(M):
    """the rows of a real-run shape that get the emulated chain (every row gets the float64 bound)"""
    return [0, 31, 32, 63, 64, 2047, M - 65, M - 64, M - 1]


def _in_range(t):
    """magnitudes below 2^-20 become zero, above 2^20 are clamped (see the module docstring)"""
    return torch.where(t.abs() < TINY, torch.zeros_like(t), t).clamp(-HUGE, HUGE)


def operands(M, K, N, seed=0):
    """(X [M, K], W [N, K], bias [N]) on the CPU: N(0, 1) activations, N(0, 1 / K) weights made asymmetric (W[:, 0] += 0.01 arange(N): a
    row / column swap must not cancel), N(0, 0.1^2) biases; a function of (M, K, N, seed) alone."""
    g = torch.Generator().manual_seed(1000003 * seed + 10007 * M + 101 * K + N)
    X = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) / math.sqrt(K)
    W[:, 0] += torch.arange(N) * 0.01
    bias = torch.randn(N, generator=g) * 0.1
    return _in_range(X), _in_range(W), _in_range(bias)


def layer_ref64(X, W, bias, elu):
    """float64; ELU = where(z > 0, z, expm1(z)) (torch.nn.ELU, alpha = 1)"""
    z = X.double() @ W.double().t()
    if bias is not None:
        z = z + bias.double()
    return torch.where(z > 0, z, torch.expm1(z)) if elu else z


def layer_bound(X, W, bias):
    """Per element: (K + 2) U32 (|X| @ |W|^T + |bias|) -- a k-ordered fp32 chain of K multiply-adds plus the bias add (each of the K + 1
    roundings is relative to a partial sum no larger than the sum of the magnitudes; one more for the (1 + U32)^n terms dropped)."""
    K = X.shape[1]
    mag = X.double().abs() @ W.double().abs().t()
    if bias is not None:
        mag = mag + bias.double().abs()
    return (K + 2) * U32 * mag


def fma32(a, b, c):
    """fp32 fmaf(a, b, c) = round_to_nearest_even_fp32(a b + c), element-wise on fp32 tensors, without a hardware fma: in float64 the
    product of two fp32 values is exact (48 bits); TwoSum gives the exact error of the float64 addition; a non-zero error makes the sum
    inexact, and the float64 neighbour on the error's side is taken when the sum's last mantissa bit is even (round to odd: the sticky
    bit).  A 53-bit round-to-odd value rounds to 24 bits as the exact value would, so the single conversion to fp32 is the only rounding.
    (float32(float64(c) + p) rounds twice and is wrong whenever the float64 sum lands on an fp32 midpoint.)"""
    assert a.dtype == b.dtype == c.dtype == torch.float32
    p = a.double() * b.double()
    c = c.double()
    s = c + p
    t = s - c
    e = (c - (s - t)) + (p - t)          # TwoSum (Knuth): s + e == c + p exactly
    bits = s.view(torch.int64)
    even = (bits & 1) == 0
    away = (e > 0) == (s > 0)            # the exact value lies beyond s, away from zero (s == 0 comes with e == 0: operands are normal)
    step = torch.where(away, torch.ones_like(bits), -torch.ones_like(bits))
    bits = torch.where((e != 0) & even, bits + step, bits)
    return bits.view(torch.float64).float()


def fma_chain32(X, W, bias=None):
    """[M, N] fp32: acc = fmaf(X[r, k], W[j, k], acc) for k = 0 .. K - 1 from acc = 0, then one fp32 add of the bias; vectorised over
    (rows, columns), a Python loop over k.  Finite operands in the module's range."""
    X, W = X.float(), W.float()
    M, K = X.shape
    acc = torch.zeros(M, W.shape[0], dtype=torch.float32, device=X.device)
    for k in range(K):
        acc = fma32(X[:, k:k + 1], W[:, k].unsqueeze(0), acc)   # (broadcast to [M, N])
    return acc + bias.float() if bias is not None else acc


def ulp_distance(a, b):
    """number of fp32 values between two finite fp32 tensors, element-wise (int64); 0 iff the bits agree up to the sign of zero"""
    def key(t):
        i = t.contiguous().view(torch.int32).long()
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return (key(a) - key(b)).abs()


def edge_cases():
    """(M, K, N) of the first edge sweep: every K edge at five (M, N)"""
    return [(M, K, N) for K, (M, N) in itertools.product(EDGE_K, EDGE_MN)]
