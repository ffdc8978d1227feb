"""libgrx_ppo.so's training kernels (include/grx_ppo.h) against float64 restatements of the same operations (tests/ppo_ref.py), at
the shapes PPO trains with and at the edges of each kernel's blocking: the ELU backward + bias gradient, the minibatch loss for every
action count and on both sides of its finalize's LDS staging limit, the policy head, the optimizer tail, the minibatch gather, and one
minibatch's parameter gradients end to end against a float64 copy of the network.

Tolerances are stated from the arithmetic: U32 = 2^-24 is the fp32 unit roundoff; a sum of n fp32 terms computed one after another
is good to n * U32 * (sum of the terms' magnitudes)."""
import copy
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import ppo_ref
from tests.mlp_layer_ref import layer_bound
from tests.ppo_ref import U32
from wiki_grx_gym_amd.rl import fused_loss as fl
from wiki_grx_gym_amd.rl.modules import ActorCriticMLP
from wiki_grx_gym_amd.rl.ppo import PPO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


# ---- grx_ppo_elu_backward_colsum ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 255, 256, 257, 10485, 24576, 41943, 49152])
def test_elu_backward_colsum_matches_float64(rows):
    """dz = dy * (y > 0 ? 1 : y + 1) bit for bit (one fp32 add and one fp32 multiply, the same in any implementation), db = the column
    sums of dz within 2e-5 * max(1, |ref|) of a float64 sum (256-row slabs of fp32 adds: with |dy| ~ 0.1 the rounding of a 49152-row
    sum stays near 1e-5 absolute; a dropped slab moves it by ~1), and the second call equal to the first.  y holds exact zeros (factor 1: torch's
    elu_backward takes the y + 1 branch there), values just above -1 and positives; the slab and column edges of the blocking are
    crossed (256 rows, 64 columns)."""
    for cols in (1, 63, 64, 65, 128, 256, 512, 700):
        g = _gen(rows * 1000 + cols)
        dy = torch.randn(rows, cols, device=DEV, generator=g) * 0.1
        y = torch.nn.functional.elu(torch.randn(rows, cols, device=DEV, generator=g) * 2.0)
        u = torch.rand(rows, cols, device=DEV, generator=g)
        y = torch.where(u < 0.15, torch.zeros_like(y), y)
        y = torch.where(u > 0.9, -1.0 + torch.rand(rows, cols, device=DEV, generator=g) * 1e-5, y)
        y = torch.where((u > 0.88) & (u <= 0.9), torch.full_like(y, float(np.nextafter(np.float32(-1), np.float32(0)))), y)
        if rows * cols >= 8:
            assert (y == 0).any() and (y > 0).any() and (y < -0.99999).any()
        dz, db = fl.elu_backward_colsum(dy, y)
        want = dy * torch.where(y > 0, torch.ones_like(y), y + 1.0)
        assert torch.equal(dz, want), (rows, cols, float((dz - want).abs().max()))
        ref = want.double().sum(0)
        err = (db.double() - ref).abs()
        tol = 2e-5 * ref.abs().clamp(min=1.0)
        assert bool((err <= tol).all()), (rows, cols, float((err / tol).max()))
        dz2, db2 = fl.elu_backward_colsum(dy, y)
        assert torch.equal(dz2, dz) and torch.equal(db2, db), (rows, cols)


# ---- grx_ppo_loss ---------------------------------------------------------------------------------------------------------------
CLIP, VCOEF, ECOEF = 0.2, 1.3, 0.01


def _loss_data(B, A, seed):
    """A seeded minibatch drawn like a rollout's (actions = mu + std * eps, old policy near the new one), old log-probs spread so that
    ratios fall inside and on both sides of the clip interval; rows whose float64 arithmetic is within 1e-3 of a branch of the loss
    are moved off it (ppo_ref.loss_near_ties).  fp32 tensors on the device."""
    g = _gen(seed)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)
    std = 0.05 + 0.3 * torch.rand(A, device=DEV, generator=g)
    mu = 0.5 * r(B, A)
    actions = mu + std * r(B, A)
    old_mu = mu + 0.1 * std * r(B, A)
    old_sigma = std * (1.0 + 0.1 * torch.rand(B, A, device=DEV, generator=g))
    value = r(B, 1)
    tv, ret, adv = value + 0.3 * r(B, 1), value + r(B, 1), r(B, 1)
    logp = torch.distributions.Normal(mu.double(), std.double()).log_prob(actions.double()).sum(-1, keepdim=True)
    old_logp = (logp + 0.25 * r(B, 1).double()).float()
    for _ in range(20):
        bad = ppo_ref.loss_near_ties(mu, std, value, actions, old_logp, ret, tv, CLIP)
        if not bool(bad.any()):
            break
        b = bad.reshape(-1, 1)
        old_logp = torch.where(b, old_logp - 0.01, old_logp)
        tv = torch.where(b, tv + 0.013, tv)
        ret = torch.where(b, ret + 0.011, ret)
    assert not bool(ppo_ref.loss_near_ties(mu, std, value, actions, old_logp, ret, tv, CLIP).any())
    return dict(mu=mu, std=std, value=value, actions=actions, old_logp=old_logp, old_mu=old_mu, old_sigma=old_sigma,
                advantages=adv, returns=ret, target_values=tv)


def _fused(d, use_clipped):
    """grx_ppo_loss through its autograd wrapper: the four scalars and (backward of the total loss, gradient 1) d_mu, d_std, d_value"""
    mu, std, value = (d[k].clone().requires_grad_() for k in ("mu", "std", "value"))
    out = fl.fused_ppo_loss(mu, std, value, d["actions"], d["old_logp"], d["old_mu"], d["old_sigma"], d["advantages"], d["returns"],
                            d["target_values"], CLIP, VCOEF, ECOEF, use_clipped)
    out[2].backward()
    return out.detach(), mu.grad, std.grad, value.grad


def _check_loss(d, use_clipped, tag, rows=None):
    """grx_ppo_loss on `d` against ppo_ref.ppo_loss_ref.  rows (a bool mask [B]): only those rows of d_mu and d_value are judged, with the
    same formulas and d_mu's largest magnitude taken over them -- the other rows hold planted values that are not finite, and so are the
    batch sums."""
    out, d_mu, d_std, d_value = _fused(d, use_clipped)
    ref = ppo_ref.ppo_loss_ref(d["mu"], d["std"], d["value"], d["actions"], d["old_logp"], d["old_mu"], d["old_sigma"], d["advantages"],
                               d["returns"], d["target_values"], CLIP, VCOEF, ECOEF, use_clipped)
    B, A = d["mu"].shape
    mu, std, a = d["mu"].double(), d["std"].double(), d["actions"].double()
    # a row's ratio = exp(logp - old_logp), logp an fp32 sum of A terms: relative error <= U32 ((A + 4) sum_k |term_k| + 2 |old_logp| + 8);
    # everything per row (d_mu, the surrogate, d_std's terms) inherits it
    terms = -(a - mu) ** 2 / (2.0 * std ** 2) - torch.log(std) - ppo_ref.LOG_SQRT_2PI
    R_row = U32 * ((A + 4) * terms.abs().sum(-1) + 2.0 * d["old_logp"].double().abs().reshape(-1) + 8.0)
    R = float(R_row.max())
    keep = torch.ones(B, dtype=torch.bool, device=DEV) if rows is None else rows
    err = (d_mu.double() - ref["d_mu"]).abs()[keep]
    tol = (R_row.unsqueeze(-1) * ref["d_mu"].abs())[keep] + 4 * U32 * float(ref["d_mu"][keep].abs().max())
    assert bool(torch.isfinite(tol).all()) and bool((err <= tol).all()), (tag, "d_mu", float((err / tol).max()))
    # the value gradient: a few fp32 operations on v, tv, ret, clip -- relative to those operands' size
    ops = d["value"].double().abs() + d["target_values"].double().abs() + d["returns"].double().abs() + CLIP
    err = (d_value.double() - ref["d_value"]).abs()[keep]
    tol = (16 * U32 * 2.0 * VCOEF / B * ops)[keep]
    assert bool(torch.isfinite(tol).all()) and bool((err <= tol).all()), (tag, "d_value", float((err / tol).max()))
    if rows is not None:
        return
    # sums over the batch run in double: the error is the per-row error summed, <= R * (sum of the rows' magnitudes), plus the final rounding
    err = (d_std.double() - ref["d_std"]).abs()
    tol = R * ref["scale"]["d_std"] + 2 * U32 * ref["d_std"].abs()
    assert bool((err <= tol).all()), (tag, "d_std", float((err / tol).max()))
    # the four scalars: besides R, the value loss is a difference of its operands squared, the KL row a sum of A terms that
    # cancel to ~0 (old and new policy are close) and the entropy an fp32 sum over A in the finalize
    os_, om = d["old_sigma"].double(), d["old_mu"].double()
    kl_terms = (torch.log(std / os_ + 1e-5).abs() + (os_ ** 2 + (om - mu) ** 2) / (2.0 * std ** 2) + 0.5).sum(-1).mean()
    ent_terms = float((0.5 + ppo_ref.LOG_SQRT_2PI + torch.log(std)).abs().sum())
    extra = torch.tensor([0.0, 4 * U32 * float((ops ** 2).mean()), 0.0, (A + 4) * U32 * float(kl_terms)], dtype=torch.float64, device=DEV)
    extra[2] = VCOEF * extra[1] + ECOEF * (A + 4) * U32 * ent_terms
    err = (out.double() - ref["out"]).abs()
    tol = R * ref["scale"]["out"] + 2 * U32 * ref["out"].abs() + extra
    assert bool((err <= tol).all()), (tag, "out", out.tolist(), ref["out"].tolist(), (err / tol).tolist())


@pytest.mark.parametrize("use_clipped", [True, False])
def test_loss_every_action_count_matches_float64(use_clipped):
    """Every template instantiation of grx_ppo_loss (A = 1..32) at B = 4097 (16 full blocks and a one-row block) against float64 autograd
    of the PPO._losses spelling."""
    for A in range(1, 33):
        _check_loss(_loss_data(4097, A, 100 + A), use_clipped, ("A", A))


@pytest.mark.parametrize("B", [29952, 29953, 41943, 49152, 98304])
@pytest.mark.parametrize("A", [10, 32])
def test_loss_large_batches_both_sides_of_the_staging_limit(A, B):
    """ppo_loss_finalize stages the block partials in LDS while ceil(B / 256) * 35 <= 4096 (B <= 29952) and reads them from global memory
    above: both branches must add every block (41943: the full body at 16384 envs; 49152: 8192 envs x 24 steps / 4 minibatches)."""
    d = _loss_data(B, A, B + A)
    _check_loss(d, True, (A, B))
    if B == 98304:
        _check_loss(d, False, (A, B))


def test_loss_rejects_invalid_arguments_and_writes_nothing():
    """A = 0, A = 33 and B = 0 return a negative code before any launch: sentinel-filled outputs stay as they were."""
    lib = fl.load_ppo_library()
    B, A = 300, 32
    d = _loss_data(B, A, 5)
    sentinel = -12345.0
    out, d_mu, d_std, d_value = (torch.full(s, sentinel, device=DEV) for s in ((4,), (B, A), (A,), (B,)))
    partials = torch.full((lib.grx_ppo_loss_partials_size(B),), sentinel, device=DEV)
    ptr = lambda k: d[k].data_ptr()
    for b, a in ((B, 0), (B, 33), (0, A), (-1, A)):
        rc = lib.grx_ppo_loss(b, a, ptr("mu"), ptr("std"), ptr("value"), ptr("actions"), ptr("old_logp"), ptr("old_mu"), ptr("old_sigma"),
                              ptr("advantages"), ptr("returns"), ptr("target_values"), CLIP, VCOEF, ECOEF, 1, out.data_ptr(), d_mu.data_ptr(),
                              d_std.data_ptr(), d_value.data_ptr(), partials.data_ptr(), _stream())
        assert rc < 0, (b, a, rc)
    torch.cuda.synchronize()
    for t in (out, d_mu, d_std, d_value, partials):
        assert bool((t == sentinel).all())
    assert lib.grx_ppo_loss_partials_size(0) == 0


# ---- grx_ppo_loss where values stop being finite ------------------------------------------------------------------------------------
XB, XROWS = 257, (0, 255, 256)   # two blocks, the second of one row; planted rows: the first, and the last of either block
_NAN, _INF = float("nan"), float("inf")
# name: (what is planted, per-row?).  "std": std[k] = value for one action k (every row sees it); the rest: rows XROWS of the named tensors.
# Every planted value sits far from an fp32 threshold: sigma^2 = 1e-50 is 0 (the smallest subnormal is 1.4e-45) and 1e-36 normal with
# sigma^3 = 1e-54 = 0; exp(200 + logp) overflows for any logp these rows have (exp overflows at 88.7) and exp(70 + logp) does not (the
# rows' logp stays below 14: asserted).
EXTREMES = {
    "sigma_sq_underflow": ({"std": 1e-25}, False),
    "sigma_cube_underflow": ({"std": 1e-18}, False),
    "sigma_zero": ({"std": 0.0}, False),
    "sigma_negative": ({"std": -0.3}, False),
    "sigma_inf": ({"std": _INF}, False),
    "sigma_nan": ({"std": _NAN}, False),
    "ratio_overflow_adv_pos": ({"old_logp": -200.0, "advantages": 1.5}, True),
    "ratio_overflow_adv_neg": ({"old_logp": -200.0, "advantages": -1.5}, True),
    "ratio_overflow_adv_zero": ({"old_logp": -200.0, "advantages": 0.0}, True),
    "ratio_large_finite": ({"old_logp": -70.0}, True),
    "adv_pinf": ({"advantages": _INF}, True),
    "adv_ninf": ({"advantages": -_INF}, True),
    "returns_inf": ({"returns": _INF}, True),
    "value_inf": ({"value": _INF}, True),
    "target_values_inf": ({"target_values": _INF}, True),
    "kl_only": ({"old_sigma": 0.0}, True),
}


def _extreme_data(A, seed):
    """the base minibatch of tests/test_ppo_gpu.py::test_fused_loss_propagates_nan_like_torch at B = XB, its rows moved off the loss's
    branch points as _loss_data moves them"""
    g = _gen(seed)
    mk = lambda *s: torch.randn(*s, device=DEV, generator=g)
    B = XB
    d = dict(mu=mk(B, A) * 0.1, std=torch.full((A,), 0.3, device=DEV), value=mk(B, 1), actions=mk(B, A) * 0.3, old_logp=mk(B, 1) * 0.1 - 2,
             old_mu=mk(B, A) * 0.1, old_sigma=torch.full((B, A), 0.3, device=DEV), advantages=mk(B, 1), returns=mk(B, 1), target_values=mk(B, 1))
    ties = lambda: ppo_ref.loss_near_ties(d["mu"], d["std"], d["value"], d["actions"], d["old_logp"], d["returns"], d["target_values"], CLIP)
    for _ in range(20):
        bad = ties()
        if not bool(bad.any()):
            break
        b = bad.reshape(-1, 1)
        d["old_logp"] = torch.where(b, d["old_logp"] - 0.01, d["old_logp"])
        d["target_values"] = torch.where(b, d["target_values"] + 0.013, d["target_values"])
        d["returns"] = torch.where(b, d["returns"] + 0.011, d["returns"])
    assert not bool(ties().any())
    return d


def _plant(d, plants, k):
    """the planted copy of a minibatch: std[k], or rows XROWS (column k of a [B, A] tensor) of the named tensors"""
    d = {n: t.clone() for n, t in d.items()}
    for name, v in plants.items():
        if name == "std":
            d[name][k] = v
        elif d[name].shape[1] == 1:
            d[name][list(XROWS)] = v
        else:
            d[name][list(XROWS), k] = v
    return d


@pytest.mark.parametrize("case", list(EXTREMES))
def test_loss_at_the_extremes_shows_what_torch_shows(case):
    """grx_ppo_loss where sigma underflows or is invalid, the ratio overflows, and advantages, returns or values are infinite, B = 257,
    A in {1, 10, 32}, the value loss clipped and not, against PPO's own fp32 torch spelling on the device (ppo_ref.TorchSpelling: underflow
    and overflow are fp32 facts, float64 has no say in them).  ppo_ref.check_extremes: the loss and the mean KL are finite exactly when
    torch's are and non-finite in the same way; a finite torch loss over a non-finite torch gradient finds the kernel's gradient non-finite
    too (the step tail then skips the step); the non-finite masks of d_mu, d_value (per entry) and d_std (per action) are equal.  A planted
    row does not leak: every other row of d_mu and d_value meets _check_loss's float64 bound.  The large finite ratio (exp(70 + logp)) is
    an ordinary case for _check_loss.  No planted value had to be moved.  (Found by this: sigma_cube_underflow -- a finite loss, torch's
    d_mu all NaN through `sigma = mean * 0.0 + std`, the kernel's d_mu finite; sigma_inf -- the same entries under a loss of -inf;
    target_values_inf -- the kernel's d_value NaN (inf * 0) in the planted rows where clamp's backward selects 0.  Fixed in the kernel.)"""
    plants, per_row = EXTREMES[case]
    for A in (1, 10, 32):
        base = _extreme_data(A, 7000 + A)
        d = _plant(base, plants, A // 2)
        for use_clipped in (True, False):
            tag = (case, A, use_clipped)
            if case == "ratio_large_finite":
                lp = torch.distributions.Normal(d["mu"].double(), d["std"].double()).log_prob(d["actions"].double()).sum(-1)[list(XROWS)]
                assert float(lp.max()) < 14.0 and float(lp.min()) > -60.0, (tag, lp.tolist())   # (1e4 > the ratio's distance to either end of fp32)
                _check_loss(d, use_clipped, tag)
                continue
            want = ppo_ref.TorchSpelling(A, CLIP, VCOEF, ECOEF, use_clipped, DEV)(
                d["mu"], d["std"], d["value"], d["actions"], d["old_logp"], d["old_mu"], d["old_sigma"], d["advantages"], d["returns"], d["target_values"])
            got = _fused(d, use_clipped)
            print(tag, "kernel", got[0].tolist(), "torch", want["out"].tolist(), "non-finite d_mu / d_std / d_value: kernel",
                  [int((~torch.isfinite(x)).sum()) for x in got[1:]], "torch", [int((~torch.isfinite(want[n])).sum()) for n in ("d_mu", "d_std", "d_value")])
            ppo_ref.check_extremes(got, want, tag)
            if per_row:
                rows = torch.ones(XB, dtype=torch.bool, device=DEV)
                rows[list(XROWS)] = False
                _check_loss(d, use_clipped, tag, rows=rows)


# ---- grx_mlp_policy_head --------------------------------------------------------------------------------------------------------
def _head(lib, X, W, bias, std, eps):
    M, K = X.shape
    A = W.shape[0]
    actions, mu, sigma = (torch.full((M, A), float("nan"), device=DEV) for _ in range(3))
    logp = torch.full((M,), float("nan"), device=DEV)
    rc = lib.grx_mlp_policy_head(M, K, A, X.data_ptr(), W.data_ptr(), bias.data_ptr() if bias is not None else None, std.data_ptr(),
                                 eps.data_ptr(), actions.data_ptr(), logp.data_ptr(), mu.data_ptr(), sigma.data_ptr(), _stream())
    assert rc == 0, rc
    return {"mu": mu, "actions": actions, "sigma": sigma, "logp": logp}


def _check_head(got, X, W, bias, std, eps, tag):
    ref = ppo_ref.policy_head_ref(X, W, bias, std, eps)
    tol_mu = layer_bound(X, W, bias) + 1e-30   # a k-ordered fp32 chain of K multiply-adds plus the bias: (K + 2) U32 (|X| |W|^T + |bias|)
    e = (got["mu"].double() - ref["mu"]).abs()
    assert bool((e <= tol_mu).all()), (tag, "mu", float((e / tol_mu).max()))
    sd, ep = std.double(), eps.double()
    tol_a = tol_mu + 2 * U32 * (ref["actions"].abs() + (sd * ep).abs())
    e = (got["actions"].double() - ref["actions"]).abs()
    assert bool((e <= tol_a).all()), (tag, "actions", float((e / tol_a).max()))
    assert torch.equal(got["sigma"], std.expand_as(got["sigma"])), tag
    # logp: the kernel differences its own fp32 a and mu (d = a - mu carries U32 (|a| + |d|) of a's rounding), squares, scales by
    # 1 / (2 std^2), subtracts log std and log sqrt(2 pi), and adds the A terms in a 5-level shuffle tree
    terms = -ep ** 2 / 2.0 - torch.log(sd) - ppo_ref.LOG_SQRT_2PI
    dz = 2 * U32 * (ref["actions"].abs() + (sd * ep).abs()) / sd
    tol_l = (ep.abs() * dz + 2 * U32 * ep ** 2 + 4 * U32 * (torch.log(sd).abs() + 1.0)).sum(-1) + 8 * U32 * terms.abs().sum(-1)
    e = (got["logp"].double() - ref["logp"]).abs()
    assert bool((e <= tol_l).all()), (tag, "logp", float((e / tol_l).max()))


@pytest.mark.parametrize("A", [1, 10, 12, 31, 32])
def test_policy_head_matches_float64(A):
    """grx_mlp_policy_head: mu, actions, sigma and logp against float64, K in {1, 128, 130} (the 64-wide K chunk, a partial chunk, the
    scalar-load path for K % 4 != 0), ragged M around the 64-row tile, a per-action std; once with X one float past a 16-byte boundary
    (the scalar-load path at K = 128) and once without a bias."""
    lib = fl.load_ppo_library()
    for K in (1, 128, 130):
        for M in (1, 63, 64, 65, 4100):
            g = _gen(A * 100000 + K * 1000 + M)
            X = torch.randn(M, K, device=DEV, generator=g)
            W = torch.randn(A, K, device=DEV, generator=g) / math.sqrt(K)
            W[:, 0] += torch.arange(A, device=DEV) * 0.01   # (row / column swaps must not cancel)
            bias = torch.randn(A, device=DEV, generator=g) * 0.1
            std = torch.linspace(0.05, 1.0, A, device=DEV)[torch.randperm(A, device=DEV, generator=g)]
            eps = torch.randn(M, A, device=DEV, generator=g)
            _check_head(_head(lib, X, W, bias, std, eps), X, W, bias, std, eps, (A, K, M))
            if M in (65, 4100):
                _check_head(_head(lib, X, W, None, std, eps), X, W, None, std, eps, (A, K, M, "no bias"))
            if K == 128 and M in (65, 4100):
                buf = torch.empty(M * K + 4, device=DEV)
                Xm = buf[1:1 + M * K].view(M, K)
                Xm.copy_(X)
                assert Xm.data_ptr() % 16 == 4
                _check_head(_head(lib, Xm, W, bias, std, eps), X, W, bias, std, eps, (A, K, M, "misaligned"))


@pytest.mark.parametrize("A", [1, 10, 31, 32])
def test_policy_head_mu_is_the_layer_kernels_bits(A):
    """grx_mlp_policy_head's mu is grx_mlp_layer(X, W, bias, elu = 0) bit for bit (the same kernel body with another epilogue), with and
    without a bias: one K chunk of one k, two full chunks, two chunks plus one MFMA (scalar loads); one row and a second, one-row tile.
    tests/test_noise_std_gpu.py holds the state-dependent head to the same; tests/test_mlp_layer_gpu.py holds the layer kernel itself."""
    lib = fl.load_ppo_library()
    for K in (1, 128, 130):
        for M in (1, 65):
            g = _gen(7 + A * 100000 + K * 1000 + M)
            X = torch.randn(M, K, device=DEV, generator=g)
            W = torch.randn(A, K, device=DEV, generator=g) / math.sqrt(K)
            W[:, 0] += torch.arange(A, device=DEV) * 0.01
            std = torch.linspace(0.05, 1.0, A, device=DEV)
            eps = torch.randn(M, A, device=DEV, generator=g)
            for bias in (torch.randn(A, device=DEV, generator=g) * 0.1, None):
                mu = _head(lib, X, W, bias, std, eps)["mu"]
                y = fl._layer(lib, X, W, bias, False, _stream())
                assert torch.equal(mu.view(torch.int32), y.view(torch.int32)), (A, K, M, bias is not None, float((mu - y).abs().max()))


# ---- grx_ppo_step_tail ----------------------------------------------------------------------------------------------------------
BIG = 1024 * 4096 + 3 * 4096 + 5   # more than 1024 chunks of 4096: tail_apply_kernel reads the partials past 1024 from global memory

TAIL_SETS = {
    # the full-body actor-critic: 105 / 234 observations, 32 actions, [512, 256, 128] -- 17 tensors in parameters() order
    "full_body": [512 * 105, 512, 256 * 512, 256, 128 * 256, 128, 32 * 128, 32, 512 * 234, 512, 256 * 512, 256, 128 * 256, 128, 128, 1, 32],
    "edges": [1, 1023, 1024, 1025, 4095, 4096, 4097],
    "max_tensors": [1 + 517 * i for i in range(24)],
    "big": [7, BIG, 4097],
}
DESIRED, LR_MIN, LR_MAX = 0.01, 1e-5, 1e-3
# name: (lr, kl, adaptive, step0, clip active, loss, bad_flag)
TAIL_CASES = {
    "down": (1e-4, 3 * DESIRED, 1, 0, True, 0.7, None),
    "up": (1e-4, 0.3 * DESIRED, 1, 1000, False, 0.7, None),
    "keep": (1e-4, DESIRED, 1, 1000, True, 0.7, 0.0),
    "kl_zero": (1e-4, 0.0, 1, 0, False, 0.7, None),
    "fixed": (1e-4, 5 * DESIRED, 0, 1000, True, 0.7, None),
    "floor": (1.2e-5, 5 * DESIRED, 1, 1000, True, 0.7, None),
    "ceiling": (9e-4, 0.1 * DESIRED, 1, 0, False, 0.7, None),
    "nonfinite_loss": (1e-4, 3 * DESIRED, 1, 1000, True, float("nan"), None),
    "bad_flag": (1e-4, 0.3 * DESIRED, 1, 1000, True, 0.7, 1.0),
    # a KL that is not finite: every comparison with NaN is false (the rate stays), +inf is above 2 * desired (down) -- as torch.where decides
    "kl_nan": (1e-4, float("nan"), 1, 1000, True, 0.7, None),
    "kl_inf": (1e-4, float("inf"), 1, 0, False, 0.7, None),
}
# One gradient element replaced after the clip threshold is chosen.  name: (value, place).  NaN, +-inf and 1e20 (finite; its square, 1e40,
# is 30 times the largest float32) make the fp32 total norm non-finite: the step is skipped.  1e17 (square 1e34, 1 / 34000 of the largest
# float32) is representable: the step runs, clipped by the usual rule.
TAIL_POISON = {"nan": float("nan"), "pinf": float("inf"), "ninf": float("-inf"), "sq_overflow": 1e20}
TAIL_POISON_SETS = ("edges", "full_body", "big")
TAIL_LARGE = 1e17


def _poison_index(numels, place):
    """(tensor, element) of a poisoned-gradient place: `first` element 0 of tensor 0; `last` the last element of the last tensor; `ragged`
    the last element (in the last, partial chunk of 4096) of the largest tensor but the last whose numel is no multiple of 4096; `global`
    an element of the large tensor past 1024 chunks -- its partial is one tail_apply_kernel reads from global memory, not from LDS."""
    if place == "first":
        return 0, 0
    if place == "last":
        return len(numels) - 1, numels[-1] - 1
    if place == "ragged":
        t = max((i for i in range(len(numels) - 1) if numels[i] % 4096), key=lambda i: numels[i])
        return t, numels[t] - 1
    t = max(range(len(numels)), key=lambda i: numels[i])
    assert place == "global" and numels[t] > 1025 * 4096 + 17
    return t, 1025 * 4096 + 17


def _tail_cases():
    """(tset, case) of test_step_tail_matches_float64: every TAIL_CASES entry on every tensor set, then the poisoned and large gradients"""
    pairs = [(tset, case) for tset in TAIL_SETS for case in TAIL_CASES]
    for tset in TAIL_POISON_SETS:
        places = ["first", "last", "ragged"] + (["global"] if tset == "big" else [])
        pairs += [(tset, f"{name}@{place}@{step0}") for name in TAIL_POISON for place in places for step0 in (0, 1000)]
        pairs += [(tset, f"large@ragged@{step0}") for step0 in (0, 1000)]
    return pairs


def _tail_case(case):
    """(the TAIL_CASES tuple, poison) -- poison None or (value, place); a poisoned case: loss 0.7, no bad_flag, the clip on at step 0 and off at step 1000"""
    if case in TAIL_CASES:
        return TAIL_CASES[case], None
    name, place, step0 = case.split("@")
    step0 = int(step0)
    return (1e-4, 3 * DESIRED if step0 else 0.3 * DESIRED, 1, step0, step0 == 0, 0.7, None), (TAIL_LARGE if name == "large" else TAIL_POISON[name], place)


GUARD = 64                     # floats in front of and behind every tensor of the tail tests (256 bytes: the tensor's start keeps its alignment)
SENTINEL_BITS = 0x4B3C614E     # what the guards of param, exp_avg and exp_avg_sq hold (the gradient's hold NaN)


def _guarded(x, nan):
    """`x` copied into the middle of a buffer with GUARD floats on either side: (the view, the buffer)"""
    n = x.numel()
    buf = torch.empty(n + 2 * GUARD, device=DEV)
    if nan:
        buf.fill_(float("nan"))
    else:
        buf.view(torch.int32).fill_(SENTINEL_BITS)
    view = buf[GUARD:GUARD + n]
    view.copy_(x)
    assert view.data_ptr() % 256 == x.data_ptr() % 256 == 0
    return view, buf


def _guards_intact(buf):
    b = buf.view(torch.int32)
    return bool((b[:GUARD] == SENTINEL_BITS).all()) and bool((b[-GUARD:] == SENTINEL_BITS).all())


def _tail_state(numels, step0, seed, guards=None):
    """Parameters, gradients, both moments and step counters of a tensor set.  With `guards` (a list): every tensor sits inside a larger
    buffer between two guard bands (_guarded), the gradients' NaN -- a read past either end of a gradient turns a step that must run into
    a visible skip -- and the sentinel buffers of the other three are appended to `guards`."""
    g = _gen(seed)
    P = [torch.randn(n, device=DEV, generator=g) for n in numels]
    G = [torch.randn(n, device=DEV, generator=g) * (0.01 * (1 + i % 5)) for i, n in enumerate(numels)]
    for x in G:
        if x.numel() > 1024 * 4096:
            x[1024 * 4096:] *= 30.0   # the chunks past the 1024th carry a visible share of the norm
    if step0:
        M = [torch.randn(n, device=DEV, generator=g) * 0.01 for n in numels]
        V = [torch.rand(n, device=DEV, generator=g) * 1e-4 for n in numels]
    else:
        M = [torch.zeros(n, device=DEV) for n in numels]
        V = [torch.zeros(n, device=DEV) for n in numels]
    S = [torch.full((), float(step0), device=DEV) for _ in numels]
    if guards is not None:
        G = [_guarded(x, True)[0] for x in G]
        for xs in (P, M, V):
            for i, x in enumerate(xs):
                xs[i], buf = _guarded(x, False)
                guards.append(buf)
    return P, G, M, V, S


def _tail_structs(P, G, M, V, S, numels=None):
    t = fl._TailTensors()
    t.n = len(P)
    for i in range(min(len(P), fl.TAIL_MAX)):
        t.param[i], t.grad[i], t.exp_avg[i], t.exp_avg_sq[i], t.step[i] = (x[i].data_ptr() for x in (P, G, M, V, S))
        t.numel[i] = P[i].numel() if numels is None else numels[i]
    return t


@pytest.mark.parametrize("tset,case", _tail_cases(), ids=[f"{t}-{c}" for t, c in _tail_cases()])
def test_step_tail_matches_float64(tset, case):
    """grx_ppo_step_tail against ppo_ref.step_tail_ref (clip_grad_norm_ + Adam in float64) after the learning rate rule: the lr bit-equal
    to PPO._device_lr_update on the device, step counters exact, the clipped gradient's share of each moment within 4e-5 relative (the clip
    coefficient comes from an fp32 sum of squares over at most 1030 chunk partials: <= 1030 U32 relative, halved by the square root) plus
    a few roundings of both shares, parameters within 2 ulp plus 1e-4 of the update plus the moment tolerance carried through Adam's ratio.  A non-finite loss or bad_flag = 1
    leaves parameters, moments and step counters bit-identical and adds nothing to the statistics (the kernel multiplied the losses by 0
    there, so a NaN value loss turned sums[0] into NaN: fixed).  `sums` gets sums[0] += value loss, sums[1] += surrogate, sums[2] = kl.

    So does a gradient whose fp32 total norm is not finite, under a finite loss (TAIL_POISON: one NaN, +inf, -inf or 1e20 element, in the
    first and the last block, in a partial chunk, and in a chunk whose partial the second launch reads from global memory): the kernel
    clamped fminf(max_norm / (NaN + 1e-6), 1) = 1 and ran Adam on the unclipped gradients, and an infinite norm's coefficient 0 put
    inf * 0 = NaN into the moments.  One 1e17 element (TAIL_LARGE) is representable and must NOT skip: the same float64 comparison.
    kl = NaN / +inf: the learning rate as torch.where decides it.

    Every tensor lies between two guard bands of 64 floats inside its own allocation (_tail_state): the gradients' hold NaN, so a read
    past either end makes a step that must run skip; the others hold a bit pattern that must still be there afterwards."""
    lib = fl.load_ppo_library()
    (lr0, kl, adaptive, step0, clip_on, loss, bad_flag), poison = _tail_case(case)
    numels = TAIL_SETS[tset]
    guards = []
    P, G, M, V, S = _tail_state(numels, step0, len(case) * 31 + len(tset), guards)
    if poison is not None and poison[0] == TAIL_LARGE:
        ti, ei = _poison_index(numels, poison[1])
        G[ti][ei] = TAIL_LARGE
        poison = None
    total = math.sqrt(sum(float(x.double().pow(2).sum()) for x in G))
    max_norm = 0.5 * total if clip_on else 100.0 * total
    if poison is not None:
        ti, ei = _poison_index(numels, poison[1])
        G[ti][ei] = poison[0]
    P0, M0, V0 = ([x.clone() for x in xs] for xs in (P, M, V))
    lr_t = torch.tensor(lr0, device=DEV)
    kl_t = torch.tensor(kl, device=DEV)
    loss_t = torch.tensor(loss, device=DEV)
    vl_t = torch.tensor(float("nan") if not math.isfinite(loss) else 0.375, device=DEV)
    sl_t = torch.tensor(-0.0625, device=DEV)
    bad_t = torch.tensor(bad_flag, device=DEV) if bad_flag is not None else None
    sums = torch.tensor([1.5, -0.25, 7.0], device=DEV)
    t = _tail_structs(P, G, M, V, S)
    nb = lib.grx_ppo_step_tail_blocks(C.byref(t))
    assert nb == sum((n + 4095) // 4096 for n in numels)
    partials = torch.empty(nb, device=DEV)
    a = fl._TailArgs()
    a.loss, a.kl, a.lr, a.value_loss, a.surrogate_loss = loss_t.data_ptr(), kl_t.data_ptr(), lr_t.data_ptr(), vl_t.data_ptr(), sl_t.data_ptr()
    a.bad_flag = bad_t.data_ptr() if bad_t is not None else None
    a.sums, a.partials, a.adaptive = sums.data_ptr(), partials.data_ptr(), adaptive
    a.desired_kl, a.lr_min, a.lr_max, a.max_grad_norm = DESIRED, LR_MIN, LR_MAX, max_norm
    a.beta1, a.beta2, a.eps = 0.9, 0.999, 1e-8
    assert lib.grx_ppo_step_tail(C.byref(t), C.byref(a), _stream()) == 0
    torch.cuda.synchronize()
    assert all(_guards_intact(buf) for buf in guards), (tset, case, "a write outside a tensor")

    # the learning rate: bit-equal to the torch device rule, and to the fp32 restatement
    class _Alg:
        desired_kl, learning_rate_min, learning_rate_max = DESIRED, LR_MIN, LR_MAX
    want_lr = torch.tensor(lr0, device=DEV)
    if adaptive:
        alg = _Alg(); alg._lr_t = want_lr
        PPO._device_lr_update(alg, kl_t)
    assert float(lr_t) == float(want_lr) == float(ppo_ref.lr_rule_fp32(lr0, kl, adaptive, DESIRED, LR_MIN, LR_MAX)), (float(lr_t), float(want_lr))
    if case == "floor":
        assert float(lr_t) == np.float32(LR_MIN)
    if case == "ceiling":
        assert float(lr_t) == np.float32(LR_MAX)
    lr_used = float(lr_t)

    ref = ppo_ref.step_tail_ref(P0, G, M0, V0, [step0] * len(numels), lr_used, loss, bad_flag, np.float32(max_norm), 0.9, 0.999, 1e-8)
    if poison is None:
        assert (ref["clip"] < 0.6) if clip_on else (ref["clip"] == 1.0)
        assert ref["skipped"] == (case in ("nonfinite_loss", "bad_flag")), case
    else:
        assert ref["skipped"], case
    want_sums = sums.new_tensor([1.5, -0.25, 7.0])
    if not ref["skipped"]:
        want_sums[0] += vl_t; want_sums[1] += sl_t
    want_sums[2] = kl_t
    assert torch.equal(sums.view(torch.int32), want_sums.view(torch.int32)), (sums.tolist(), want_sums.tolist())   # (bits: kl may be NaN)
    if ref["skipped"]:
        bits = lambda x: x.view(torch.int32)
        for i in range(len(numels)):
            assert torch.equal(bits(P[i]), bits(P0[i])) and torch.equal(bits(M[i]), bits(M0[i])) and torch.equal(bits(V[i]), bits(V0[i])), (tset, case, i)
            assert float(S[i]) == step0, (tset, case, i, float(S[i]))
        return
    for i in range(len(numels)):
        assert float(S[i]) == ref["steps"][i] == step0 + 1, i
        m_ref, v_ref, p_ref = ref["exp_avg"][i], ref["exp_avg_sq"][i], ref["params"][i]
        # the moments: the clipped gradient's share carries the clip coefficient's error, both shares a few roundings
        gc = G[i].double() * ref["clip"]
        m_old, m_new = 0.9 * M0[i].double().abs(), 0.1 * gc.abs()
        tol_m = 4e-5 * m_new + 4 * U32 * (m_old + m_new)
        e = (M[i].double() - m_ref).abs()
        assert bool((e <= tol_m).all()), (tset, case, i, "exp_avg", float((e / tol_m).max()))
        v_old, v_new = 0.999 * V0[i].double(), 0.001 * gc ** 2
        tol_v = 8e-5 * v_new + 4 * U32 * (v_old + v_new)
        e = (V[i].double() - v_ref).abs()
        assert bool((e <= tol_v).all()), (tset, case, i, "exp_avg_sq", float((e / tol_v).max()))
        # the parameters: 2 ulp, 1e-4 of the update, and the moment's tolerance carried through step_size / denom
        s1 = step0 + 1.0
        denom = torch.sqrt(v_ref) / math.sqrt(1.0 - 0.999 ** s1) + 1e-8
        upd = (p_ref - P0[i].double()).abs()
        tol = 2.0 * p_ref.abs() * 2 ** -23 + 1e-4 * torch.maximum(upd, torch.full_like(upd, lr_used)) + lr_used / (1.0 - 0.9 ** s1) * tol_m / denom
        e = (P[i].double() - p_ref).abs()
        assert bool((e <= tol).all()), (tset, case, i, "param", float((e / tol).max()))


def test_step_tail_rejects_invalid_tensor_sets():
    """n = 0, n = 25 and a tensor of 0 elements: grx_ppo_step_tail_blocks and grx_ppo_step_tail return a negative code and launch nothing."""
    lib = fl.load_ppo_library()
    P, G, M, V, S = _tail_state([5, 6, 7], 0, 1)
    lr_t, kl_t, loss_t = (torch.tensor(x, device=DEV) for x in (1e-4, 0.3 * DESIRED, 0.5))
    sums = torch.tensor([1.5, -0.25, 7.0], device=DEV)
    partials = torch.zeros(8, device=DEV)
    a = fl._TailArgs()
    a.loss, a.kl, a.lr, a.value_loss, a.surrogate_loss = loss_t.data_ptr(), kl_t.data_ptr(), lr_t.data_ptr(), loss_t.data_ptr(), loss_t.data_ptr()
    a.sums, a.partials, a.adaptive = sums.data_ptr(), partials.data_ptr(), 1
    a.desired_kl, a.lr_min, a.lr_max, a.max_grad_norm = DESIRED, LR_MIN, LR_MAX, 1e-3
    a.beta1, a.beta2, a.eps = 0.9, 0.999, 1e-8
    P0 = [x.clone() for x in P]
    for n, numels in ((0, None), (25, None), (3, [5, 0, 7])):
        t = _tail_structs(P, G, M, V, S, numels)
        t.n = n
        assert lib.grx_ppo_step_tail_blocks(C.byref(t)) < 0, n
        assert lib.grx_ppo_step_tail(C.byref(t), C.byref(a), _stream()) < 0, n
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(P, P0)) and all(float(s) == 0.0 for s in S)
    assert float(lr_t) == np.float32(1e-4) and sums.tolist() == [1.5, -0.25, 7.0]


# ---- grx_ppo_gather_rows --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mb", [1, 255, 10485, 49152])
def test_gather_rows_is_index_select(mb):
    """12 tensors (the maximum) of widths 1 .. 234 gathered by an index with duplicates and the first and last rows: bit-equal to
    index_select; 13 tensors are rejected and nothing is written."""
    lib = fl.load_ppo_library()
    N = 49153
    widths = [1, 10, 32, 39, 105, 168, 234, 1, 10, 32, 39, 105]
    g = _gen(mb)
    srcs = [torch.randn(N, w, device=DEV, generator=g) for w in widths]
    dsts = [torch.full((mb, w), float("nan"), device=DEV) for w in widths]
    idx = torch.randint(0, N, (mb,), device=DEV, generator=g)
    idx[0] = N - 1
    if mb > 1:
        idx[1] = 0
        idx[-1] = idx[mb // 2]
    gather = fl.RowGather(srcs, dsts)
    gather(idx)
    for s, d in zip(srcs, dsts):
        assert torch.equal(d, s.index_select(0, idx)), d.shape
    n = 13
    extra = torch.full((mb, 3), -7.0, device=DEV)
    src = (C.c_void_p * n)(*[s.data_ptr() for s in srcs + [srcs[0]]])
    dst = (C.c_void_p * n)(*[d.data_ptr() for d in dsts + [extra]])
    w = (C.c_int * n)(*(widths + [3]))
    before = [d.clone() for d in dsts]
    assert lib.grx_ppo_gather_rows(n, src, dst, w, idx.data_ptr(), mb, _stream()) < 0
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(dsts, before)) and bool((extra == -7.0).all())


# ---- end to end: one minibatch's parameter gradients --------------------------------------------------------------------------
E2E = {
    "gr1t1": dict(no=39, npri=168, A=10, mb=24576, std=0.2, gain=1.0),
    "full_body": dict(no=105, npri=234, A=32, mb=10485, std=[0.2] * 12 + [0.05] * 20, gain=0.01),
    "config3": dict(no=39, npri=168, A=10, mb=49152, std=0.2, gain=1.0),
}


def _e2e_setup(name):
    """(ac, its float64 deepcopy, PPO with its defaults on the device, one minibatch) for an E2E configuration"""
    c = E2E[name]
    torch.manual_seed(11)
    ac = ActorCriticMLP(c["no"], c["npri"], c["A"], actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[512, 256, 128], activation="elu",
                        init_noise_std=c["std"], actor_output_gain=c["gain"])
    ac64 = copy.deepcopy(ac).double().to(DEV)
    alg = PPO(ac, clip_param=CLIP, value_loss_coef=1.0, entropy_coef=0.01, use_clipped_value_loss=True, schedule="adaptive",
              desired_kl=0.01, device=DEV)
    assert alg._fused_loss and alg._two_streams
    mb, A = c["mb"], c["A"]
    g = _gen(mb + A)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)
    obs, cobs = r(mb, c["no"]), r(mb, c["npri"])
    with torch.no_grad():
        mu64, v64 = ac64.actor(obs.double()), ac64.critic(cobs.double())
        std = ac.std.detach()
        actions = (mu64 + std.double() * r(mb, A).double()).float()
        old_mu = (mu64 + 0.1 * std.double() * r(mb, A).double()).float()
        old_sigma = std * (1.0 + 0.1 * torch.rand(mb, A, device=DEV, generator=g))
        tv, ret, adv = (v64 + 0.3 * r(mb, 1).double()).float(), (v64 + r(mb, 1).double()).float(), r(mb, 1)
        logp = torch.distributions.Normal(mu64, std.double()).log_prob(actions.double()).sum(-1, keepdim=True)
        old_logp = (logp + 0.25 * r(mb, 1).double()).float()
        for _ in range(20):
            bad = ppo_ref.loss_near_ties(mu64, std, v64, actions, old_logp, ret, tv, CLIP)
            if not bool(bad.any()):
                break
            b = bad.reshape(-1, 1)
            old_logp = torch.where(b, old_logp - 0.01, old_logp)
            tv = torch.where(b, tv + 0.013, tv)
            ret = torch.where(b, ret + 0.011, ret)
        assert not bool(ppo_ref.loss_near_ties(mu64, std, v64, actions, old_logp, ret, tv, CLIP).any())
    # (the order of PPO._minibatch_step's batch: obs, cobs, actions, target_values, advantages, returns, old_logp, old_mu, old_sigma)
    return ac, ac64, alg, [obs, cobs, actions, tv, adv, ret, old_logp, old_mu, old_sigma]


def _e2e_check(name, ac, ac64, batch, loss=None):
    """every p.grad of `ac` against the float64 copy's on the same minibatch"""
    obs, cobs, actions, tv, adv, ret, old_logp, old_mu, old_sigma = batch
    mu, value = ac64.actor(obs.double()), ac64.critic(cobs.double())
    ref = ppo_ref.ppo_loss_ref(mu, ac64.std, value, actions, old_logp, old_mu, old_sigma, adv, ret, tv, CLIP, 1.0, 0.01, True)
    ac64.zero_grad(set_to_none=True)
    torch.autograd.backward([mu, value, ac64.std], [ref["d_mu"], ref["d_value"], ref["d_std"]])
    if loss is not None:
        assert abs(float(loss) - float(ref["out"][2])) <= 1e-4 * float(ref["scale"]["out"][2]) + 1e-6 * abs(float(ref["out"][2]))
    for (n, p), q in zip(ac.named_parameters(), ac64.parameters()):
        gref = q.grad
        tol = 1e-4 * float(gref.abs().max())
        err = float((p.grad.double() - gref).abs().max())
        assert err <= tol, (name, n, err, tol)


@pytest.mark.parametrize("name", list(E2E))
def test_minibatch_parameter_gradients_match_float64(name):
    """PPO as trained (fused loss, the training MLP path: grx_mlp_layer forward, grx_ppo_elu_backward_colsum and grx_ppo_colsum
    backward, the critic on a second stream) against a float64 deepcopy of the same ActorCriticMLP: a double input takes the plain
    nn.Sequential path and the loss is the PPO._losses spelling in float64 (ppo_ref.ppo_loss_ref).  Every p.grad within
    1e-4 * max |g_ref|: the weight gradients are fp32 GEMMs summed over up to 49152 rows (U32 * sqrt(49152) ~ 1.3e-5 relative for
    random-signed terms), fed by a loss gradient good to ~1e-5 relative (see _check_loss).

    _losses runs eagerly here as the graph build's dry runs run it: two streams, under the BLAS preference update() and
    _build_graph set (PPO._blas_for_update).  (Called with both streams on torch's default hipBLASLt, the value-head weight gradient at
    minibatch 49152 came out wrong once and the step did not finish twice: _losses now keeps the critic on the actor's stream
    unless the actor's GEMMs go to rocBLAS -- see PPO._losses.)"""
    ac, ac64, alg, batch = _e2e_setup(name)
    with alg._blas_for_update():
        s, v, loss, kl = alg._losses(*batch)
        alg.optimizer.zero_grad(set_to_none=True)
        loss.backward()
    torch.cuda.synchronize()
    _e2e_check(name, ac, ac64, batch, float(loss.detach()))


@pytest.mark.parametrize("name", ["gr1t1", "config3"])
def test_captured_two_stream_step_gradients_match_float64(name):
    """The captured minibatch step itself (PPO._build_graph: dry runs, then the HIP graph of _minibatch_step with the critic on the
    second stream) replayed once on a minibatch of 24576 / 49152 rows: the gradients it leaves in p.grad equal the float64 copy's, at
    the tolerance of test_minibatch_parameter_gradients_match_float64.  (_build_graph puts the parameters back after its dry runs, so the
    replay differentiates the same weights as the copy.)"""
    ac, ac64, alg, batch = _e2e_setup(name)
    alg.init_storage(16, 2)   # (_build_graph takes its buffer widths from the storage)
    mb = batch[0].shape[0]
    alg._build_graph(mb)
    assert isinstance(alg._graph, torch.cuda.CUDAGraph)
    for buf, x in zip(alg._static, batch):
        buf.copy_(x)
    alg._graph.replay()
    torch.cuda.synchronize()
    _e2e_check(name, ac, ac64, batch)


@pytest.mark.parametrize("path", ["eager", "captured", "bucket", "fused"])
def test_skipped_steps_leave_the_update_statistics_finite(path, monkeypatch):
    """An update whose every minibatch has a NaN loss (NaN returns) skips every step: parameters stay put and the reported mean losses
    are 0, not NaN (rsl_rl skips such minibatches; the statistics once added NaN * 0).  Each tail: torch's in _update_device, in the
    captured _minibatch_step, in the bucket path's _mb_back (a one-rank process group), and libgrx_ppo.so's."""
    monkeypatch.setenv("GRX_PPO_FUSED_TAIL", "1" if path == "fused" else "0")
    monkeypatch.setenv("GRX_PPO_GRAPH", "0" if path == "eager" else "1")
    import torch.distributions
    import torch.distributed as dist
    if path == "bucket":
        monkeypatch.setenv("GRX_PPO_FORCE_BUCKET", "1")
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29647", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        torch.manual_seed(0)
        ac = ActorCriticMLP(39, 168, 10, actor_hidden_dims=[64, 32], critic_hidden_dims=[64, 32], activation="elu", init_noise_std=0.2)
        alg = PPO(ac, num_learning_epochs=2, num_mini_batches=4, clip_param=CLIP, value_loss_coef=1.0, entropy_coef=0.01,
                  use_clipped_value_loss=True, schedule="adaptive", desired_kl=0.01, device=DEV)
        assert alg._fused_tail == (path == "fused") and (alg._bucket is not None) == (path == "bucket")
        alg.init_storage(256, 8)
        st = alg.storage
        g = _gen(3)
        for t in (st.observations, st.pri_observations, st.actions, st.values, st.advantages, st.actions_log_prob, st.mu):
            t.copy_(torch.randn(t.shape, device=DEV, generator=g))
        st.sigma.copy_(0.5 + torch.rand(st.sigma.shape, device=DEV, generator=g))
        st.returns.fill_(float("nan"))
        before = [p.detach().clone() for p in ac.parameters()]
        vl, sl = alg.update()
        assert vl == 0.0 and sl == 0.0, (path, vl, sl)
        assert all(torch.equal(p, b) for p, b in zip(ac.parameters(), before))
    finally:
        if path == "bucket":
            dist.destroy_process_group()


@pytest.mark.parametrize("path", ["eager", "captured", "bucket", "fused"])
def test_nonfinite_gradients_skip_every_step(path, monkeypatch):
    """A finite loss over a non-finite gradient skips the step in every tail that clips.  `scalar` noise with sigma = 1e-18: every ratio
    is exp(-1e36) = 0 and the loss finite, but d_std holds 0 * inf = NaN -- checked first on one minibatch through PPO._losses (on a copy
    of the policy: the captured step wants parameters no eager backward has touched).  update() then leaves every parameter bit-identical
    and the step counters where they were (0, or no optimizer state at all), and reports 0.0 for both mean losses.  The paths of
    test_skipped_steps_leave_the_update_statistics_finite; before the norm joined the skip rule, torch's tails stepped on NaN gradients
    (clip_grad_norm_ spreads the NaN norm over every .grad) and libgrx_ppo.so's clamped the coefficient to 1 and ran Adam."""
    monkeypatch.setenv("GRX_PPO_FUSED_TAIL", "1" if path == "fused" else "0")
    monkeypatch.setenv("GRX_PPO_GRAPH", "0" if path == "eager" else "1")
    import torch.distributed as dist
    if path == "bucket":
        monkeypatch.setenv("GRX_PPO_FORCE_BUCKET", "1")
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29653", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        torch.manual_seed(0)
        ac = ActorCriticMLP(39, 168, 10, actor_hidden_dims=[64, 32], critic_hidden_dims=[64, 32], activation="elu", init_noise_std=1e-18)
        kw = dict(num_learning_epochs=2, num_mini_batches=4, clip_param=CLIP, value_loss_coef=1.0, entropy_coef=0.01,
                  use_clipped_value_loss=True, schedule="adaptive", desired_kl=0.01, device=DEV)
        probe = PPO(copy.deepcopy(ac), **kw)
        alg = PPO(ac, **kw)
        assert alg._fused_tail == (path == "fused") and (alg._bucket is not None) == (path == "bucket")
        alg.init_storage(256, 8)
        st = alg.storage
        g = _gen(3)
        for t in (st.observations, st.pri_observations, st.actions, st.values, st.advantages, st.actions_log_prob, st.mu, st.returns):
            t.copy_(torch.randn(t.shape, device=DEV, generator=g))
        st.sigma.copy_(0.5 + torch.rand(st.sigma.shape, device=DEV, generator=g))
        # the premise: a finite loss, a gradient that is not
        batch = next(iter(st.mini_batch_generator(4, 1)))[:9]
        with probe._blas_for_update():
            _, _, loss, _ = probe._losses(*batch)
            loss.backward()
        std_grad = probe.actor_critic.std.grad
        assert bool(torch.isfinite(loss)) and not bool(torch.isfinite(std_grad).all()), (float(loss), std_grad.tolist())
        before = [p.detach().clone() for p in ac.parameters()]
        vl, sl = alg.update()
        bits = lambda x: x.detach().view(torch.int32)
        assert all(torch.equal(bits(p), bits(b)) for p, b in zip(ac.parameters(), before)), path
        steps = [float(alg.optimizer.state[p]["step"]) for p in ac.parameters() if "step" in alg.optimizer.state.get(p, {})]
        assert all(s == 0.0 for s in steps), (path, steps)
        assert vl == 0.0 and sl == 0.0, (path, vl, sl)
    finally:
        if path == "bucket":
            dist.destroy_process_group()
