"""grx_mlp_layer (csrc/grx_ppo.hip mlp_layer_kernel), the f32-input MFMA layer that every forward of the default path runs
through and that the head, estimator, CENet, RND, LayerNorm, recurrent and gradient-penalty kernels are compared to bit for bit -- held
here to tests/mlp_layer_ref.py at every edge of its tiling: a 64 x 64 output tile per block, a 32 x 32 MFMA tile per wave, K chunks of 64
through two LDS buffers, float4 loads where K % 4 == 0 and both operands are 16-byte aligned and scalar loads otherwise.

Three kinds of statement, kept apart so that a failure says which one broke:
  * VALUE: |Y - float64| <= layer_bound per element (the *_value tests, the integer tests, the non-finite tests) -- holds for any
    summation order; a kernel that fails one of these computes something wrong;
  * ROW / COLUMN INDEPENDENCE and determinism: the same bytes wherever a row or a weight row sits -- holds for any order that does not
    depend on the position in the tile;
  * ORDER: Y equals fma_chain32 bit for bit.  test_edge_sweep_bits, test_tile_sweep_bits, test_alignment_gives_the_same_bits and
    test_real_run_shapes carry it; a retiling that changes the order on purpose changes those assertions and nothing else.

Every operand of every call is a view inside a larger allocation whose other floats (at least GUARD on either side) are NaN, so a read
beside an operand that reaches an accumulator shows as NaN in a result; Y lies between two guard bands of a sentinel bit pattern that
must survive the call.

GRX_MLP_LAYER_PARITY_JSON=<path>: the tests also write what they measured there (profiles/mlp_layer_parity.json is such a file)."""
import ctypes as C
import json
import os

import pytest
import torch

from tests import mlp_layer_ref as R
from wiki_grx_gym_amd.rl import fused_loss as fl

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64                     # floats on either side of every operand (256 bytes: an operand's start keeps its alignment)
SENTINEL_BITS = 0x4B3C614E     # what Y and its guard bands hold before a call (12345678.0f)
NAN = float("nan")


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bytes(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _guarded(t, off=0):
    """`t` copied into a NaN-filled device buffer, GUARD + off floats from its start (off = 1: one float past a 16-byte boundary)"""
    n = t.numel()
    buf = torch.full((n + 2 * GUARD + 4,), NAN, device=DEV)
    view = buf[GUARD + off:GUARD + off + n].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 * off
    return view


def layer(X, W, bias, elu, x_off=0, w_off=0):
    """grx_mlp_layer on guarded copies of the operands (CPU or device tensors); Y [M, N], its guard bands checked"""
    lib = fl.load_ppo_library()
    (M, K), N = X.shape, W.shape[0]
    assert W.shape[1] == K and X.dtype == W.dtype == torch.float32
    Xv, Wv = _guarded(X, x_off), _guarded(W, w_off)
    bv = _guarded(bias) if bias is not None else None
    ybuf = torch.full((M * N + 2 * GUARD,), SENTINEL_BITS, dtype=torch.int32, device=DEV)
    Y = ybuf[GUARD:GUARD + M * N].view(torch.float32).view(M, N)
    rc = lib.grx_mlp_layer(M, K, N, Xv.data_ptr(), Wv.data_ptr(), bv.data_ptr() if bv is not None else None, Y.data_ptr(), int(elu), _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert bool((ybuf[:GUARD] == SENTINEL_BITS).all()) and bool((ybuf[-GUARD:] == SENTINEL_BITS).all()), ("a guard float of Y was written", M, K, N)
    assert _same_bytes(Xv, X.to(DEV)) and _same_bytes(Wv, W.to(DEV)), ("an operand was written", M, K, N)
    return Y


@pytest.fixture(scope="module")
def parity():
    rec = {}
    yield rec
    path = os.environ.get("GRX_MLP_LAYER_PARITY_JSON")
    if path and rec:
        doc = {"what": "tests/test_mlp_layer_gpu.py on one MI355X.  value: the largest |Y - float64| / layer_bound over the test's cases (at most "
                       "1).  chain: 'equal', or the largest fp32 ulp distance between Y and fma_chain32.  elu: the largest error in fp32 ulps of "
                       "the float64 expm1 of the kernel's own pre-activation, of the kernel's ELU and of torch.expm1 (fp32) on the same tensor",
               "value": {k[6:]: max(v) for k, v in sorted(rec.items()) if k.startswith("value:")},
               "chain": {k[6:]: ("equal" if max(v) == 0 else max(v)) for k, v in sorted(rec.items()) if k.startswith("chain:")},
               "elu": {k[4:]: {"kernel_ulps": max(a for a, _ in v), "torch_ulps": max(b for _, b in v)} for k, v in sorted(rec.items()) if k.startswith("elu:")}}
        with open(path, "w") as f:
            json.dump(doc, f, indent=1)


def _check_value(parity, key, Y, X, W, bias, tag):
    """elu = 0: |Y - layer_ref64| <= layer_bound per element (float64 on the device); no NaN from beside an operand"""
    X, W, bias = X.to(DEV), W.to(DEV), bias.to(DEV) if bias is not None else None
    assert not bool(torch.isnan(Y).any()), (tag, "NaN in the result: a read beside an operand")
    err = (Y.double() - R.layer_ref64(X, W, bias, False)).abs()
    bound = R.layer_bound(X, W, bias)
    ratio = float((err / bound.clamp_min(1e-300)).max())
    parity.setdefault("value:" + key, []).append(ratio)
    bad = (err > bound).nonzero()
    assert bad.numel() == 0, (tag, "first (row, column) outside the bound", bad[0].tolist(), "of", len(bad), "largest error / bound", ratio)


def _check_chain(parity, key, Y, chain, tag):
    """Y == fma_chain32: the summation ORDER (see the module docstring)"""
    chain = chain.to(DEV)
    d = R.ulp_distance(Y, chain)
    worst = int(d.max())
    parity.setdefault("chain:" + key, []).append(worst)
    if not torch.equal(Y, chain):
        bad = (Y != chain).nonzero()
        r, c = bad[0].tolist()
        print(tag, "chain: first (row, column) with other bits", (r, c), "kernel", float(Y[r, c]).hex(), "chain", float(chain[r, c]).hex(),
              "elements", len(bad), "of", Y.numel(), "largest ulp distance", worst)
    assert torch.equal(Y, chain), (tag, "largest ulp distance", worst)


def _ulps(got, ref64):
    """|got - ref64| in units of the fp32 ulp of ref64 (which must be non-zero and in fp32's normal range)"""
    _, e = torch.frexp(ref64)            # ref64 = m 2^e, 0.5 <= |m| < 1: ulp = 2^(e - 24)
    return (got.double() - ref64).abs() * torch.exp2((24 - e).double())


def _check_elu(parity, key, Y0, Y1, tag):
    """The ELU epilogue against the kernel's own elu = 0 result: positive entries keep their bits; zeros keep theirs; negative entries
    against float64 expm1 of the fp32 pre-activation -- at most 4 x the largest error of torch.expm1 (fp32) on the same tensor, that
    allowance never below 1 ulp."""
    assert not bool(torch.isnan(Y1).any()), (tag, "NaN in the ELU result")
    pos = Y0 > 0
    assert torch.equal(_bits(Y1)[pos], _bits(Y0)[pos]), (tag, "a positive entry changed under ELU")
    zero = Y0 == 0
    assert torch.equal(_bits(Y1)[zero], _bits(Y0)[zero]), (tag, "a zero changed under ELU")
    neg = Y0 < 0
    if not bool(neg.any()):
        return
    z = Y0[neg]
    ref = torch.expm1(z.double())
    k, t = float(_ulps(Y1[neg], ref).max()), float(_ulps(torch.expm1(z), ref).max())
    parity.setdefault("elu:" + key, []).append((k, t))
    assert k <= max(4.0 * t, 1.0), (tag, "ELU error in ulps: kernel", k, "torch.expm1", t)


def _chain_cpu(X, W):
    """the bias-free chain on the CPU (where tests/test_mlp_layer_ref.py judged it); the bias is one fp32 add on top"""
    return R.fma_chain32(X.cpu(), W.cpu())


def _sweep(parity, key, X, W, bias, chain, bits):
    """one (M, K, N): with and without the bias, elu 0 and 1 -- value (bits = False) or chain (bits = True) for elu = 0, the ELU rule for elu = 1"""
    tag = (key, tuple(X.shape), W.shape[0])
    for b in (bias, None):
        Y0 = layer(X, W, b, 0)
        if bits:
            _check_chain(parity, key, Y0, chain + b if b is not None else chain, tag + (b is not None,))
        else:
            _check_value(parity, key, Y0, X, W, b, tag + (b is not None,))
            _check_elu(parity, key, Y0, layer(X, W, b, 1), tag + (b is not None,))


# ---- the edge sweeps ------------------------------------------------------------------------------------------------------------
_CACHE = {}


def _edge_case(M, K, N):
    """operands and bias-free chain of one case of the K-edge sweep, computed once for the value and the bits test"""
    if (M, K, N) not in _CACHE:
        X, W, bias = R.operands(M, K, N)
        _CACHE[M, K, N] = (X, W, bias, _chain_cpu(X, W))
    return _CACHE[M, K, N]


@pytest.mark.parametrize("K", R.EDGE_K)
def test_edge_sweep_value(parity, K):
    """Every K edge (one k, one MFMA, a chunk less / exactly / plus one, both LDS buffers reused, K % 4 of every kind) at five (M, N):
    within layer_bound of float64 with and without a bias; the ELU result follows from the elu = 0 result by _check_elu's rule."""
    for M, N in R.EDGE_MN:
        X, W, bias, _ = _edge_case(M, K, N)
        _sweep(parity, "edge_sweep", X, W, bias, None, False)


@pytest.mark.parametrize("K", R.EDGE_K)
def test_edge_sweep_bits(parity, K):
    """THE SUMMATION ORDER: elu = 0, Y equals fma_chain32 -- acc = fmaf(X[r, k], W[j, k], acc) for k = 0 .. K - 1 from zero, then + bias --
    with torch.equal.  This test, test_tile_sweep_bits, test_alignment_gives_the_same_bits and the chain half of test_real_run_shapes are
    the only ones that pin the order (what DESIGN.md 4.4 and 4.13 state about v_mfma_f32_32x32x2_f32); every other test of this file holds
    for any order.  A retiling that changes the order on purpose updates these and nothing else."""
    for M, N in R.EDGE_MN:
        X, W, bias, chain = _edge_case(M, K, N)
        _sweep(parity, "edge_sweep", X, W, bias, chain, True)


def _tile_case(K):
    """X [129, K], W [129, K], bias and the bias-free chain: case (M, N) of the tile sweep is X[:M], W[:N], whose chain is chain[:M, :N]"""
    return _edge_case(max(R.TILE_M), K, max(R.TILE_N))


@pytest.mark.parametrize("K", R.TILE_K)
def test_tile_sweep_value(parity, K):
    """M and N at every edge of the 32-row MFMA tile and the 64-row block tile (one row / column, a tile less one, a full tile, one
    more, a third block) at K = 65 (one chunk plus one k) and K = 130 (two chunks plus one MFMA): value, with and without a bias, ELU."""
    X, W, bias, _ = _tile_case(K)
    for M in R.TILE_M:
        for N in R.TILE_N:
            _sweep(parity, "tile_sweep", X[:M], W[:N], bias[:N], None, False)


@pytest.mark.parametrize("K", R.TILE_K)
def test_tile_sweep_bits(parity, K):
    """the summation order (see test_edge_sweep_bits) at every (M, N) of the tile sweep"""
    X, W, bias, chain = _tile_case(K)
    for M in R.TILE_M:
        for N in R.TILE_N:
            _sweep(parity, "tile_sweep", X[:M], W[:N], bias[:N], chain[:M, :N], True)


@pytest.mark.parametrize("shape", R.ALIGN_SHAPES)
def test_alignment_gives_the_same_bits(parity, shape):
    """K % 4 == 0, where the float4 loads are eligible: X one float past a 16-byte boundary, W one float past, both, neither -- the first
    three take the scalar loads.  All four give the same bytes, and those of the chain (the ORDER again: see test_edge_sweep_bits)."""
    M, K, N = shape
    X, W, bias, chain = _edge_case(M, K, N)
    for elu in (0, 1):
        ys = {(xo, wo): layer(X, W, bias, elu, xo, wo) for xo in (0, 1) for wo in (0, 1)}
        for k, y in ys.items():
            assert not bool(torch.isnan(y).any()), (K, elu, k)
            assert _same_bytes(y, ys[0, 0]), (K, elu, "offsets (X, W)", k, "differ from the aligned call")
    _check_chain(parity, "alignment", layer(X, W, bias, 0, 1, 1), chain + bias, (K, "misaligned"))
    _check_chain(parity, "alignment", layer(X, W, bias, 0), chain + bias, (K, "aligned"))


# ---- the ELU epilogue -----------------------------------------------------------------------------------------------------------
def test_elu_epilogue(parity):
    """Pre-activations spread over [-30, 30] (the bias shifts whole columns): positive entries keep the bits of the elu = 0 result,
    negative ones are within _check_elu's allowance of float64 expm1."""
    M, K, N = 130, 70, 200
    X, W, _ = R.operands(M, K, N, seed=1)
    bias = torch.linspace(-30.0, 30.0, N)
    Y0, Y1 = layer(X, W, bias, 0), layer(X, W, bias, 1)
    assert int((Y0 < 0).sum()) > 5000 and int((Y0 > 0).sum()) > 5000 and float(Y0.min()) < -25.0
    _check_elu(parity, "elu_epilogue", Y0, Y1, "spread")
    small = layer(X * 1e-3, W * 1e-3, None, 0)        # |z| ~ 1e-6: expm1(z) ~ z, where a naive exp(z) - 1 loses every digit
    _check_elu(parity, "elu_epilogue", small, layer(X * 1e-3, W * 1e-3, None, 1), "small")


def test_elu_of_planted_preactivations():
    """X = 0, so the pre-activation is 0 + bias: -120, -88 and -17 give -1 or its fp32 neighbour; 1e-7 and 80 pass unchanged; -1e-7 is
    expm1's; nothing is NaN.  The two zeros: IEEE addition gives (+0) + (-0) = +0, so both pre-activations are +0 -- a -0 cannot be
    planted through this entry (an fmaf chain from +0 never ends in -0 either) -- and ELU keeps that zero's sign bit, as expm1 does."""
    planted = [-120.0, -88.0, -17.0, -1e-7, -0.0, 0.0, 1e-7, 80.0]
    bias = torch.tensor(planted * 9)                   # 72 columns: two tile columns
    M, K, N = 65, 130, bias.numel()
    _, W, _ = R.operands(M, K, N)
    X = torch.zeros(M, K)
    Y0, Y1 = layer(X, W, bias, 0), layer(X, W, bias, 1)
    want0 = (torch.zeros(M, N) + bias).to(DEV)
    assert _same_bytes(Y0, want0), "0 + bias is not bias"
    assert not bool(torch.isnan(Y1).any())
    col = lambda i: Y1[:, i::8]
    near = torch.tensor(-1.0 + 2.0 ** -24, device=DEV)
    for i in (0, 1, 2):
        assert bool(((col(i) == -1.0) | (col(i) == near)).all()), (planted[i], col(i)[0, 0].item())
    assert _same_bytes(col(4), Y0[:, 4::8]) and _same_bytes(col(5), Y0[:, 5::8]) and bool((_bits(col(4)) == 0).all()) and bool((_bits(col(5)) == 0).all())
    assert _same_bytes(col(6), Y0[:, 6::8]) and _same_bytes(col(7), Y0[:, 7::8])
    z = Y0[:, 3::8].contiguous()
    ref = torch.expm1(z.double())
    assert float(_ulps(col(3), ref).max()) <= max(4.0 * float(_ulps(torch.expm1(z), ref).max()), 1.0)   # (_check_elu's allowance)


# ---- exact on integers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.INTEGER_SHAPES)
def test_integer_operands_give_the_exact_product(shape):
    """X, W integers in [-8, 8], an integer bias: every product and partial sum is an integer below 2^24, so Y is the int64 product exactly
    in ANY summation order -- a k that is dropped, doubled or taken from another row cannot hide in rounding."""
    M, K, N = shape
    g = torch.Generator().manual_seed(M * K + N)
    X = torch.randint(-8, 9, (M, K), generator=g)
    W = torch.randint(-8, 9, (N, K), generator=g)
    W[:, 0] += torch.arange(N) % 5
    bias = torch.randint(-100, 101, (N,), generator=g)
    want = X @ W.t()
    assert int(want.abs().max()) + 100 < 2 ** 24
    for b in (bias, None):
        Y = layer(X.float(), W.float(), b.float() if b is not None else None, 0)
        w = (want + b if b is not None else want).to(DEV)
        assert torch.equal(Y.double(), w.double()), (shape, b is not None, "first wrong (row, column)", (Y.double() != w.double()).nonzero()[0].tolist())
    Y1 = layer(X.float(), W.float(), bias.float(), 1)
    w = (want + bias).to(DEV)
    assert torch.equal(Y1[w > 0].double(), w[w > 0].double()) and not bool(torch.isnan(Y1).any())


@pytest.mark.parametrize("shape", R.INTEGER_SHAPES)
def test_one_hot_weights_select_exactly(shape):
    """W[j] one-hot at k = (7 j) % K, X[r, k] = 1 + (r 131 + k) % 251: Y[r, j] is X[r, (7 j) % K] exactly, and a wrong entry names the
    element it holds instead."""
    M, K, N = shape
    r, k = torch.arange(M).unsqueeze(1), torch.arange(K).unsqueeze(0)
    X = (1 + (r * 131 + k) % 251).float()
    sel = (7 * torch.arange(N)) % K
    W = torch.zeros(N, K)
    W[torch.arange(N), sel] = 1.0
    Y = layer(X, W, None, 0).cpu()
    want = X[:, sel]
    if not torch.equal(Y, want):
        i, j = (Y != want).nonzero()[0].tolist()
        print(shape, "first wrong (row, column)", (i, j), "holds", float(Y[i, j]), "wants X[%d, %d] =" % (i, int(sel[j])), float(want[i, j]),
              "; that value sits at k =", (X[i] == Y[i, j]).nonzero().flatten().tolist(), "of the same row and at rows",
              (X[:, int(sel[j])] == Y[i, j]).nonzero().flatten().tolist()[:8], "of the same k")
    assert torch.equal(Y, want), shape


# ---- a row depends on that row alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [65, 4100])
def test_a_row_gives_the_same_bytes_wherever_it_sits(M):
    """One fixed 130-float row as the only row (M = 1) and at rows 0, 31, 32, 63, 64 and M - 1 of M rows of N(0, 1e3^2) data: the same
    bytes -- what "the update reproduces the rollout bit for bit" rests on.  Holds for any summation order that does not depend on the
    row's place in the tile."""
    K, N = 130, 97
    X0, W, bias = R.operands(1, K, N, seed=2)
    g = torch.Generator().manual_seed(M)
    noise = R._in_range(torch.randn(M, K, generator=g) * 1e3)
    for elu in (0, 1):
        alone = layer(X0, W, bias, elu)
        assert not bool(torch.isnan(alone).any())
        for r in (0, 31, 32, 63, 64, M - 1):
            X = noise.clone()
            X[r] = X0[0]
            Y = layer(X, W, bias, elu)
            assert _same_bytes(Y[r:r + 1], alone), (M, elu, "row", r, "largest ulp distance", int(R.ulp_distance(Y[r:r + 1], alone).max()))
        everywhere = layer(X0.expand(M, K).contiguous(), W, bias, elu)
        assert _same_bytes(everywhere, alone.expand(M, N).contiguous()), (M, elu, "the same row M times")


@pytest.mark.parametrize("N", [65, 130])
def test_a_weight_row_gives_its_column_the_same_bytes_wherever_it_sits(N):
    """one fixed weight row (and its bias) as the only one (N = 1) and at columns 0, 31, 32, 63, 64 and N - 1 among N(0, 1e3^2) rows"""
    M, K = 70, 130
    X, W0, b0 = R.operands(M, K, 1, seed=4)
    g = torch.Generator().manual_seed(N)
    noise, bnoise = R._in_range(torch.randn(N, K, generator=g) * 1e3), torch.randn(N, generator=g) * 1e3
    for elu in (0, 1):
        alone = layer(X, W0, b0, elu)
        for j in (0, 31, 32, 63, 64, N - 1):
            W, bias = noise.clone(), bnoise.clone()
            W[j], bias[j] = W0[0], b0[0]
            Y = layer(X, W, bias, elu)
            assert _same_bytes(Y[:, j:j + 1], alone), (N, elu, "column", j, "largest ulp distance", int(R.ulp_distance(Y[:, j:j + 1], alone).max()))


def test_two_calls_give_the_same_bytes():
    for M, K, N in [(129, 193, 65), (4100, 130, 96), (4096, 512, 256)]:
        X, W, bias = R.operands(M, K, N, seed=5)
        for elu in (0, 1):
            assert _same_bytes(layer(X, W, bias, elu), layer(X, W, bias, elu)), (M, K, N, elu)


# ---- non-finite inputs ----------------------------------------------------------------------------------------------------------
NF_M, NF_K, NF_N = 70, 130, 70     # a short last tile in rows and columns (64 .. 69), two K chunks and one MFMA of a third
NF_PLACES = [(0, 0), (0, NF_K - 1), (NF_M - 1, 0), (NF_M - 1, NF_K - 1), (33, 64)]   # (row or column, k): first / last row, first k / k = K - 1 of the partial chunk


def _only(Y, clean, rows=None, cols=None, rc=None):
    """Y is NaN on the given rows / columns / (row, column) pairs and holds clean's bytes everywhere else"""
    hit = torch.zeros_like(Y, dtype=torch.bool)
    if rows is not None:
        hit[rows] = True
    if cols is not None:
        hit[:, cols] = True
    if rc is not None:
        hit[rc[0], rc[1]] = True
    return bool(torch.isnan(Y[hit]).all()) and torch.equal(_bits(Y)[~hit], _bits(clean)[~hit])


@pytest.mark.parametrize("elu", [0, 1])
def test_nan_stays_in_its_row_or_column(elu):
    X, W, bias = R.operands(NF_M, NF_K, NF_N, seed=6)
    clean = layer(X, W, bias, elu)
    assert bool(torch.isfinite(clean).all())
    for i, k in NF_PLACES:
        Xn = X.clone()
        Xn[i, k] = NAN
        assert _only(layer(Xn, W, bias, elu), clean, rows=i), ("NaN in X", i, k)
        Wn = W.clone()
        Wn[i, k] = NAN
        assert _only(layer(X, Wn, bias, elu), clean, cols=i), ("NaN in W", i, k)
    for j in (0, 33, NF_N - 1):
        bn = bias.clone()
        bn[j] = NAN
        assert _only(layer(X, W, bn, elu), clean, cols=j), ("NaN in bias", j)


@pytest.mark.parametrize("elu", [0, 1])
def test_inf_times_zero_is_nan_and_inf_times_a_positive_weight_is_inf(elu):
    """+inf in X[r, k] against W[j0, k] = 0 and positive weights W[j, k] elsewhere in that k: NaN at (r, j0), +inf in the rest of row r,
    every other row the bytes of the call without the inf."""
    X, W, bias = R.operands(NF_M, NF_K, NF_N, seed=6)
    for (r, k), j0 in zip(NF_PLACES, (0, NF_N - 1, 33, NF_N - 1, 64)):
        Wz = W.clone()
        Wz[:, k] = Wz[:, k].abs() + 0.125
        Wz[j0, k] = 0.0
        clean = layer(X, Wz, bias, elu)
        Xi = X.clone()
        Xi[r, k] = float("inf")
        Y = layer(Xi, Wz, bias, elu)
        others = torch.ones(NF_M, dtype=torch.bool, device=DEV)
        others[r] = False
        assert torch.equal(_bits(Y)[others], _bits(clean)[others]), ("another row changed", r, k)
        cols = torch.ones(NF_N, dtype=torch.bool, device=DEV)
        cols[j0] = False
        assert bool(torch.isnan(Y[r, j0])) and bool((Y[r, cols] == float("inf")).all()), (r, k, j0, Y[r].tolist())


# ---- the shapes of real runs ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.REAL_SHAPES)
def test_real_run_shapes(parity, shape):
    """The layers of the walking and full-body actor-critics at 4096 envs and of a 10485-row minibatch: every row within layer_bound of
    float64; rows 0, 31, 32, 63, 64, 2047, M - 65, M - 64 and M - 1, all columns, equal the chain (the ORDER: see test_edge_sweep_bits)."""
    M, K, N = shape
    X, W, bias = R.operands(M, K, N)
    rows = R.real_rows(M)
    chain = _chain_cpu(X[rows], W)
    for b in (bias, None):
        Y0, Y1 = layer(X, W, b, 0), layer(X, W, b, 1)
        _check_value(parity, "real_run_shapes", Y0, X, W, b, (shape, b is not None))
        _check_elu(parity, "real_run_shapes", Y0, Y1, (shape, b is not None))
        _check_chain(parity, "real_run_shapes", Y0[rows], chain + b if b is not None else chain, (shape, b is not None))


# ---- rejected calls -------------------------------------------------------------------------------------------------------------
def test_layer_rejects_invalid_arguments_and_writes_nothing():
    lib = fl.load_ppo_library()
    X, W, b = torch.randn(8, 8, device=DEV), torch.randn(8, 8, device=DEV), torch.randn(8, device=DEV)
    out = torch.full((64 + 2 * GUARD,), SENTINEL_BITS, dtype=torch.int32, device=DEV)
    y = out[GUARD:].data_ptr()
    s = _stream()
    for elu in (0, 1):
        for M, K, N in [(0, 8, 8), (8, 0, 8), (8, 8, 0), (-1, 8, 8), (8, -1, 8), (8, 8, -1)]:
            assert lib.grx_mlp_layer(M, K, N, X.data_ptr(), W.data_ptr(), b.data_ptr(), y, elu, s) < 0, (M, K, N)
        assert lib.grx_mlp_layer(8, 8, 8, None, W.data_ptr(), b.data_ptr(), y, elu, s) < 0
        assert lib.grx_mlp_layer(8, 8, 8, X.data_ptr(), None, b.data_ptr(), y, elu, s) < 0
        assert lib.grx_mlp_layer(8, 8, 8, X.data_ptr(), W.data_ptr(), b.data_ptr(), None, elu, s) < 0
    torch.cuda.synchronize()
    assert bool((out == SENTINEL_BITS).all())
    assert lib.grx_mlp_layer(8, 8, 8, X.data_ptr(), W.data_ptr(), None, y, 0, s) == 0     # (a null bias is no error)
    torch.cuda.synchronize()
    assert bool((out[:GUARD] == SENTINEL_BITS).all()) and bool((out[GUARD + 64:] == SENTINEL_BITS).all()) and not bool((out[GUARD:GUARD + 64] == SENTINEL_BITS).any())
