"""The action-noise options on the GPU (include/grx_ppo_noise.h grx_ppo_loss_sd / grx_mlp_policy_head_sd, rl/modules.py): the
loss against float64 (tests/noise_ref.py) at the smallest shapes that cross the kernel's edges, its consistency with grx_ppo_loss where
every row carries the same sigma, the policy head against grx_mlp_layer (bit for bit), float64 and exact integer arithmetic, row
independence, the argument checks with sentinels, determinism, the runner for the three variants (train, save, load, play, export), the
captured minibatch step against the eager one and float64, and the default path.

Tolerances are stated from the arithmetic as tests/test_ppo_kernels_gpu.py states them: U32 = 2^-24 is the fp32 unit roundoff; a sum of
n fp32 terms computed one after another is good to n * U32 * (sum of the terms' magnitudes)."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import noise_ref as R
from tests import ppo_ref
from tests.noise_ref import U32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CLIP, VCOEF, ECOEF = 0.2, 1.3, 0.01


def _fl():
    from wiki_grx_gym_amd.rl import fused_loss
    return fused_loss


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


# ---- grx_ppo_loss_sd --------------------------------------------------------------------------------------------------------------------
def _loss_data(B, A, seed, log_std, same_sigma=False):
    """tests/test_ppo_kernels_gpu.py's _loss_data with a sigma per row: the per-action std of that draw times a factor in [1, 3] per row
    and action (same_sigma: every row carries the std itself), handed to the kernel as raw = [mu | s], s = sigma or log(sigma) in fp32.
    The sigma everything else is drawn from is the one the kernel will see (s, or exp(s) in float64).  Rows whose float64 arithmetic is
    within 1e-3 of a branch of the loss are moved off it (ppo_ref.loss_near_ties with the rows' own sigma)."""
    g = _gen(seed)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)
    std = 0.05 + 0.3 * torch.rand(A, device=DEV, generator=g)
    spread = torch.ones(B, A, device=DEV) if same_sigma else 1.0 + 2.0 * torch.rand(B, A, device=DEV, generator=g)
    s = torch.log(std * spread) if log_std else std * spread
    sigma = torch.exp(s.double()) if log_std else s.double()
    mu = 0.5 * r(B, A)
    actions = (mu.double() + sigma * r(B, A).double()).float()
    old_mu = (mu.double() + 0.1 * sigma * r(B, A).double()).float()
    old_sigma = (sigma * (1.0 + 0.1 * torch.rand(B, A, device=DEV, generator=g).double())).float()
    value = r(B, 1)
    tv, ret, adv = value + 0.3 * r(B, 1), value + r(B, 1), r(B, 1)
    logp = torch.distributions.Normal(mu.double(), sigma).log_prob(actions.double()).sum(-1, keepdim=True)
    old_logp = (logp + 0.25 * r(B, 1).double()).float()
    for _ in range(20):
        bad = ppo_ref.loss_near_ties(mu, sigma, value, actions, old_logp, ret, tv, CLIP)
        if not bool(bad.any()):
            break
        b = bad.reshape(-1, 1)
        old_logp = torch.where(b, old_logp - 0.01, old_logp)
        tv = torch.where(b, tv + 0.013, tv)
        ret = torch.where(b, ret + 0.011, ret)
    assert not bool(ppo_ref.loss_near_ties(mu, sigma, value, actions, old_logp, ret, tv, CLIP).any())
    return dict(raw=torch.cat([mu, s], 1).contiguous(), std=std, value=value, actions=actions, old_logp=old_logp, old_mu=old_mu,
                old_sigma=old_sigma, advantages=adv, returns=ret, target_values=tv)


def _fused_sd(d, log_std, use_clipped):
    """grx_ppo_loss_sd through its autograd wrapper: the four scalars and (backward of the total loss, gradient 1) d_raw, d_value"""
    raw, value = d["raw"].clone().requires_grad_(), d["value"].clone().requires_grad_()
    out = _fl().fused_ppo_loss_sd(raw, value, d["actions"], d["old_logp"], d["old_mu"], d["old_sigma"], d["advantages"], d["returns"],
                                  d["target_values"], log_std, CLIP, VCOEF, ECOEF, use_clipped)
    out[2].backward()
    return out.detach(), raw.grad, value.grad


def _tolerances(d, ref, log_std, rows=None):
    """_check_loss's tolerances (tests/test_ppo_kernels_gpu.py) with a sigma per row.  A row's ratio = exp(logp - old_logp), logp an fp32
    sum of A terms: relative error <= R_row = U32 ((A + 4) sum_k |term_k| + 2 |old_logp| + 8) with the row's own sigma; everything per
    row inherits it.  The batch sums run in double: the per-row error summed, <= R * (sum of the rows' magnitudes), plus the final
    rounding; the value loss is a difference of its operands squared, the KL row and the entropy row fp32 sums of A terms.
    rows (a bool mask [B]): the gradient halves' largest magnitude is taken over those rows only (the others hold planted values that
    are not finite; only "mean", "s" and "d_value" on those rows mean anything then)."""
    B, A = d["actions"].shape
    mu, sigma, a = d["raw"][:, :A].double(), ref["sigma"], d["actions"].double()
    terms = -(a - mu) ** 2 / (2.0 * sigma ** 2) - torch.log(sigma) - R.LOG_SQRT_2PI
    R_row = U32 * ((A + 4) * terms.abs().sum(-1) + 2.0 * d["old_logp"].double().abs().reshape(-1) + 8.0)
    Rmax = float(R_row.max())
    halves = []
    for half in (ref["d_raw"][:, :A], ref["d_raw"][:, A:]):
        halves.append(R_row.unsqueeze(-1) * half.abs() + 4 * U32 * float((half if rows is None else half[rows]).abs().max()))
    ops = d["value"].double().abs() + d["target_values"].double().abs() + d["returns"].double().abs() + CLIP
    tol_value = 16 * U32 * 2.0 * VCOEF / B * ops
    os_, om = d["old_sigma"].double(), d["old_mu"].double()
    kl_terms = (torch.log(sigma / os_ + 1e-5).abs() + (os_ ** 2 + (om - mu) ** 2) / (2.0 * sigma ** 2) + 0.5).sum(-1).mean()
    ent_terms = float((0.5 + R.LOG_SQRT_2PI + torch.log(sigma)).abs().sum(-1).mean())   # the entropy's share: summed over a row, the mean over rows
    extra = torch.tensor([0.0, 4 * U32 * float((ops ** 2).mean()), 0.0, (A + 4) * U32 * float(kl_terms)], dtype=torch.float64, device=DEV)
    extra[2] = VCOEF * extra[1] + ECOEF * (A + 4) * U32 * ent_terms
    tol_out = Rmax * ref["scale"] + 2 * U32 * ref["out"].abs() + extra
    return {"R": Rmax, "R_row": R_row, "mean": halves[0], "s": halves[1], "d_value": tol_value, "out": tol_out}


def _loss_case(B, A, log_std, use_clipped):
    d = _loss_data(B, A, 1000 * A + B + (7 if log_std else 0), log_std)
    ref = R.loss_sd_ref(d["raw"], log_std, d["value"], d["actions"], d["old_logp"], d["old_mu"], d["old_sigma"], d["advantages"], d["returns"],
                        d["target_values"], CLIP, VCOEF, ECOEF, use_clipped)
    return d, ref, _tolerances(d, ref, log_std)


@pytest.mark.parametrize("use_clipped", [True, False], ids=["clipped", "unclipped"])
@pytest.mark.parametrize("log_std", [False, True], ids=["scalar", "log"])
def test_loss_sd_matches_float64(log_std, use_clipped):
    """grx_ppo_loss_sd against float64 autograd of rsl_rl's spelling with Normal on a sigma per row, A in {1, 10, 16, 17, 32} x B in
    {1, 255, 257, 4097} (one row, a block short of a row, a block and a row, 16 blocks and a row)."""
    for A in (1, 10, 16, 17, 32):
        for B in (1, 255, 257, 4097):
            d, ref, tol = _loss_case(B, A, log_std, use_clipped)
            if B > 1:
                assert float((ref["sigma"].max(0).values / ref["sigma"].min(0).values).max()) > 2.5   # the spread across rows
            out, d_raw, d_value = _fused_sd(d, log_std, use_clipped)
            tag = (A, B, log_std, use_clipped)
            err = (d_raw[:, :A].double() - ref["d_raw"][:, :A]).abs()
            print(tag, "d_raw mean half", float((err / tol["mean"]).max()))
            assert bool((err <= tol["mean"]).all()), (tag, "d_raw mean half", float((err / tol["mean"]).max()))
            err = (d_raw[:, A:].double() - ref["d_raw"][:, A:]).abs()
            print(tag, "d_raw s half", float((err / tol["s"]).max()))
            assert bool((err <= tol["s"]).all()), (tag, "d_raw s half", float((err / tol["s"]).max()))
            err = (d_value.double() - ref["d_value"]).abs()
            assert bool((err <= tol["d_value"]).all()), (tag, "d_value", float((err / tol["d_value"]).max()))
            err = (out.double() - ref["out"]).abs()
            print(tag, "out", (err / tol["out"]).tolist())
            assert bool((err <= tol["out"]).all()), (tag, "out", out.tolist(), ref["out"].tolist(), (err / tol["out"]).tolist())


@pytest.mark.parametrize("log_std", [False, True], ids=["scalar", "log"])
def test_loss_sd_is_consistent_with_the_existing_kernel(log_std):
    """Every row carries the same sigma (B = 4097, A in {10, 32}): `out` equals grx_ppo_loss's within the scalars' tolerance above, and the
    column sums of the s half, taken in float64 (divided by sigma under `log`: d s = d sigma * sigma), equal its d_std within _check_loss's
    d_std bound.  `scalar`: the mean half of d_raw equals d_mu bit for bit -- the same per-row expression on the same numbers.  `log`:
    the kernel's sigma is expf(s) and its log sigma s itself, where grx_ppo_loss gets a std rounded by another exp and takes logf of it,
    so the two rows' ratios differ in their last bits; the mean half is held to its float64 tolerance against d_mu instead."""
    fl = _fl()
    for A in (10, 32):
        d = _loss_data(4097, A, 50 + A, log_std, same_sigma=True)
        ref_sd = R.loss_sd_ref(d["raw"], log_std, d["value"], d["actions"], d["old_logp"], d["old_mu"], d["old_sigma"], d["advantages"],
                               d["returns"], d["target_values"], CLIP, VCOEF, ECOEF, True)
        tol = _tolerances(d, ref_sd, log_std)
        out, d_raw, d_value = _fused_sd(d, log_std, True)
        std = torch.exp(d["raw"][0, A:]) if log_std else d["raw"][0, A:].clone()
        assert torch.equal(d["raw"][:, A:], d["raw"][:1, A:].expand(4097, A))
        mu, std_p, value = d["raw"][:, :A].clone().requires_grad_(), std.clone().requires_grad_(), d["value"].clone().requires_grad_()
        out0 = fl.fused_ppo_loss(mu, std_p, value, d["actions"], d["old_logp"], d["old_mu"], d["old_sigma"], d["advantages"], d["returns"],
                                 d["target_values"], CLIP, VCOEF, ECOEF, True)
        out0[2].backward()
        err = (out.double() - out0.detach().double()).abs()
        assert bool((err <= tol["out"]).all()), (A, "out", out.tolist(), out0.tolist(), (err / tol["out"]).tolist())
        if not log_std:
            assert torch.equal(d_raw[:, :A], mu.grad), (A, float((d_raw[:, :A] - mu.grad).abs().max()))
        else:
            err = (d_raw[:, :A].double() - mu.grad.double()).abs()
            assert bool((err <= tol["mean"]).all()), (A, "mean half", float((err / tol["mean"]).max()))
        ref0 = ppo_ref.ppo_loss_ref(d["raw"][:, :A], std, d["value"], d["actions"], d["old_logp"], d["old_mu"], d["old_sigma"], d["advantages"],
                                    d["returns"], d["target_values"], CLIP, VCOEF, ECOEF, True)
        cols = d_raw[:, A:].double().sum(0) / (std.double() if log_std else 1.0)
        err = (cols - std_p.grad.double()).abs()
        bound = tol["R"] * ref0["scale"]["d_std"] + 2 * U32 * ref0["d_std"].abs()
        assert bool((err <= bound).all()), (A, "d_std", float((err / bound).max()))


def test_loss_sd_rejects_invalid_arguments_and_is_deterministic():
    """A = 0, A = 33, batch = 0 and a NULL required pointer return a negative code before any launch: sentinel-filled outputs stay as
    they were.  A valid call then writes every output, and a second one gives the same bytes."""
    lib = _fl().load_ppo_library()
    B, A = 300, 32
    d = _loss_data(B, A, 5, True)
    sentinel = -12345.0
    outs = {k: torch.full(s, sentinel, device=DEV) for k, s in (("out", (4,)), ("d_raw", (B, 2 * A)), ("d_value", (B,)))}
    outs["partials"] = torch.full((lib.grx_ppo_loss_sd_partials_size(B),), sentinel, device=DEV)
    assert lib.grx_ppo_loss_sd_partials_size(B) == 2 * 4 * 2 and lib.grx_ppo_loss_sd_partials_size(0) == 0
    names = ("raw", "value", "actions", "old_logp", "old_mu", "old_sigma", "advantages", "returns", "target_values")

    def call(b=B, a=A, null=None):
        p = {k: (None if k == null else t.data_ptr()) for k, t in list(d.items()) + list(outs.items())}
        return lib.grx_ppo_loss_sd(b, a, p["raw"], 1, *[p[k] for k in names[1:]], CLIP, VCOEF, ECOEF, 1, p["out"], p["d_raw"], p["d_value"],
                                   p["partials"], _stream())
    for b, a in ((B, 0), (B, 33), (0, A), (-1, A)):
        assert call(b, a) < 0, (b, a)
    for k in names + ("out", "d_raw", "d_value", "partials"):
        assert call(null=k) < 0, k
    torch.cuda.synchronize()
    assert all(bool((t == sentinel).all()) for t in outs.values())
    assert call() == 0
    torch.cuda.synchronize()
    assert all(not bool((t == sentinel).any()) for k, t in outs.items() if k != "partials") and bool(torch.isfinite(outs["out"]).all())
    first = {k: t.clone() for k, t in outs.items()}
    assert call() == 0
    torch.cuda.synchronize()
    assert all(torch.equal(first[k], outs[k]) for k in outs)


# ---- grx_ppo_loss_sd where values stop being finite ---------------------------------------------------------------------------------------
XB, XROWS = 257, (0, 255, 256)   # two blocks, the second of one row; planted rows: the first, and the last of either block
_NAN, _INF = float("nan"), float("inf")
# name: what is planted in rows XROWS ("s": column k of raw's s half; [B, A] tensors: column k).  tests/test_ppo_kernels_gpu.py's EXTREMES
# with the sigma of a row planted through its s, and the values of s the issue of a state-dependent sigma adds.
SD_ROW_EXTREMES = {
    "ratio_overflow_adv_pos": {"old_logp": -200.0, "advantages": 1.5},
    "ratio_overflow_adv_neg": {"old_logp": -200.0, "advantages": -1.5},
    "ratio_overflow_adv_zero": {"old_logp": -200.0, "advantages": 0.0},
    "ratio_large_finite": {"old_logp": -70.0},
    "adv_pinf": {"advantages": _INF},
    "adv_ninf": {"advantages": -_INF},
    "returns_inf": {"returns": _INF},
    "value_inf": {"value": _INF},
    "target_values_inf": {"target_values": _INF},
    "kl_only": {"old_sigma": 0.0},
}
SD_S_EXTREMES = {
    # `scalar`: sigma = s.  sigma^2 = 1e-50 = 0; sigma^2 = 1e-36 normal, sigma^3 = 0; invalid sigmas
    False: {"s_1e-25": 1e-25, "s_1e-18": 1e-18, "s_zero": 0.0, "s_negative": -0.3, "s_inf": _INF, "s_nan": _NAN},
    # `log`: sigma = exp(s).  exp(-57.5) = 1e-25 and exp(-41.4) = 1e-18 as above; exp(100) = inf; exp(-100) = 0 up to a subnormal
    True: {"s_log_1e-25": -57.5, "s_log_1e-18": -41.4, "s_plus_100": 100.0, "s_minus_100": -100.0, "s_inf": _INF, "s_minus_inf": -_INF, "s_nan": _NAN},
}


def _sd_extreme_data(A, seed, log_std):
    """tests/test_ppo_kernels_gpu.py's _extreme_data with raw = [mu | s], s = 0.3 or log(0.3) in every row"""
    g = _gen(seed)
    mk = lambda *s: torch.randn(*s, device=DEV, generator=g)
    B = XB
    mu, sigma = mk(B, A) * 0.1, torch.full((B, A), 0.3, device=DEV)
    d = dict(value=mk(B, 1), actions=mk(B, A) * 0.3, old_logp=mk(B, 1) * 0.1 - 2, old_mu=mk(B, A) * 0.1, old_sigma=sigma.clone(),
             advantages=mk(B, 1), returns=mk(B, 1), target_values=mk(B, 1))
    ties = lambda: ppo_ref.loss_near_ties(mu, sigma, d["value"], d["actions"], d["old_logp"], d["returns"], d["target_values"], CLIP)
    for _ in range(20):
        bad = ties()
        if not bool(bad.any()):
            break
        b = bad.reshape(-1, 1)
        d["old_logp"] = torch.where(b, d["old_logp"] - 0.01, d["old_logp"])
        d["target_values"] = torch.where(b, d["target_values"] + 0.013, d["target_values"])
        d["returns"] = torch.where(b, d["returns"] + 0.011, d["returns"])
    assert not bool(ties().any())
    d["raw"] = torch.cat([mu, torch.log(sigma) if log_std else sigma], 1).contiguous()
    return d


def _sd_cases():
    return [(log_std, name) for log_std in (False, True) for name in list(SD_ROW_EXTREMES) + list(SD_S_EXTREMES[log_std])]


@pytest.mark.parametrize("log_std,case", _sd_cases(), ids=[f"{'log' if l else 'scalar'}-{c}" for l, c in _sd_cases()])
def test_loss_sd_at_the_extremes_shows_what_torch_shows(log_std, case):
    """grx_ppo_loss_sd as tests/test_ppo_kernels_gpu.py::test_loss_at_the_extremes_shows_what_torch_shows judges grx_ppo_loss: B = 257,
    A in {1, 10, 32}, the value loss clipped and not, against PPO's own fp32 torch spelling of a state-dependent sigma on the device
    (ppo_ref.TorchSpelling), the extremes planted in rows 0, 255 and 256.  ppo_ref.check_extremes: loss and mean KL finite exactly when
    torch's are and non-finite in the same way, no non-finite torch gradient hidden under a finite loss, the non-finite masks of d_raw and
    d_value equal entry for entry.  Every other row of d_raw and d_value meets _tolerances' float64 bound: a planted row does not leak.
    The large finite ratio is an ordinary case for the float64 comparison of test_loss_sd_matches_float64.  No planted value had to be
    moved.  (Found by this: log-s_plus_100 -- the kernel's loss 5.77 where torch's is -inf, log sigma taken as s = 100 under a sigma of
    inf; scalar-s_inf -- torch's d s NaN (2 sigma * 0), the kernel's 0; target_values_inf -- d_value NaN where torch has 0.  Fixed in
    the kernel.)"""
    for A in (1, 10, 32):
        k = A // 2
        d = _sd_extreme_data(A, 7100 + A + (7 if log_std else 0), log_std)
        rows_i = list(XROWS)
        if case in SD_ROW_EXTREMES:
            for name, v in SD_ROW_EXTREMES[case].items():
                if d[name].shape[1] == 1:
                    d[name][rows_i] = v
                else:
                    d[name][rows_i, k] = v
        else:
            d["raw"][rows_i, A + k] = SD_S_EXTREMES[log_std][case]
        rows = torch.ones(XB, dtype=torch.bool, device=DEV)
        rows[rows_i] = False
        for use_clipped in (True, False):
            tag = (case, A, log_std, use_clipped)
            args = (d["value"], d["actions"], d["old_logp"], d["old_mu"], d["old_sigma"], d["advantages"], d["returns"], d["target_values"])
            ref = R.loss_sd_ref(d["raw"], log_std, *args, CLIP, VCOEF, ECOEF, use_clipped)
            out, d_raw, d_value = _fused_sd(d, log_std, use_clipped)
            finite_case = case == "ratio_large_finite"
            tol = _tolerances(d, ref, log_std, None if finite_case else rows)
            keep = torch.ones_like(rows) if finite_case else rows
            for name, got, want, t in (("d_raw mean half", d_raw[:, :A], ref["d_raw"][:, :A], tol["mean"]), ("d_raw s half", d_raw[:, A:], ref["d_raw"][:, A:], tol["s"]),
                                       ("d_value", d_value, ref["d_value"], tol["d_value"])):
                err = (got.double() - want).abs()[keep]
                assert bool(torch.isfinite(t[keep]).all()) and bool((err <= t[keep]).all()), (tag, name, float((err / t[keep]).max()))
            if finite_case:
                err = (out.double() - ref["out"]).abs()
                assert bool((err <= tol["out"]).all()), (tag, "out", out.tolist(), ref["out"].tolist(), (err / tol["out"]).tolist())
                continue
            want = ppo_ref.TorchSpelling(A, CLIP, VCOEF, ECOEF, use_clipped, DEV, noise="log" if log_std else "scalar", state_dependent=True)(
                d["raw"], None, d["value"], d["actions"], d["old_logp"], d["old_mu"], d["old_sigma"], d["advantages"], d["returns"], d["target_values"])
            print(tag, "kernel", out.tolist(), "torch", want["out"].tolist(), "non-finite d_raw / d_value: kernel",
                  [int((~torch.isfinite(x)).sum()) for x in (d_raw, d_value)], "torch", [int((~torch.isfinite(want[n])).sum()) for n in ("d_mu", "d_value")])
            ppo_ref.check_extremes((out, d_raw, None, d_value), want, tag)


# ---- grx_mlp_policy_head_sd ---------------------------------------------------------------------------------------------------------------
def _head(lib, X, W, bias, log_std, eps, fill=float("nan")):
    M, K = X.shape
    A = W.shape[0] // 2
    actions, mu, sigma = (torch.full((M, A), fill, device=DEV) for _ in range(3))
    logp = torch.full((M,), fill, device=DEV)
    rc = lib.grx_mlp_policy_head_sd(M, K, A, X.data_ptr(), W.data_ptr(), bias.data_ptr() if bias is not None else None, int(log_std),
                                    eps.data_ptr(), actions.data_ptr(), logp.data_ptr(), mu.data_ptr(), sigma.data_ptr(), _stream())
    assert rc == 0, rc
    return {"mu": mu, "actions": actions, "sigma": sigma, "logp": logp}


def _layer(lib, X, W, bias):
    """grx_mlp_layer(X, W, bias, elu = 0) on copies of their own (a half of the head's W starts wherever A * K floats end)"""
    fl = _fl()
    return fl._layer(lib, X, W.clone().contiguous(), bias.clone().contiguous() if bias is not None else None, False, _stream())


def _head_case(M, K, A, seed):
    g = _gen(seed)
    X = torch.randn(M, K, device=DEV, generator=g)
    W = torch.randn(2 * A, K, device=DEV, generator=g) / np.sqrt(K)
    W[:, 0] += torch.arange(2 * A, device=DEV) * 0.01   # (row / column swaps must not cancel)
    W[A:] *= 0.1
    bias = torch.randn(2 * A, device=DEV, generator=g) * 0.1
    eps = torch.randn(M, A, device=DEV, generator=g)
    return X, W, bias, eps


@pytest.mark.parametrize("log_std", [False, True], ids=["scalar", "log"])
def test_policy_head_sd_against_the_layer_kernel_and_float64(log_std):
    """M in {1, 31, 33, 200} x K in {1, 45, 128} x A in {1, 10, 16, 17, 32} (a row, a wave's rows short of one and one more, four blocks
    with a ragged last; one k, a partial chunk on the scalar-load path, two full chunks on the vector path; a half wave's columns short,
    full and one more of 16, and all 32).

    * mu equals grx_mlp_layer on W's mean rows bit for bit.  `scalar`: sigma equals grx_mlp_layer on the s rows bit for bit.  `log`: the
      kernel hands out sigma = expf(s), not s, and log(expf(s)) is not s in floating point: sigma is held to expf's error of one unit in
      the last place, |log(sigma) - s| <= 2^-23 = 2 U32 with the logarithm taken in float64, against the same
      layer output -- the accumulation itself is pinned bit for bit by the `scalar` run on the same operands.
    * mu and s within (K + 2) U32 sum_k |x_k w_k| of float64 (a k-ordered fp32 chain of K multiply-adds plus the bias).
    * actions and logp within test_policy_head_matches_float64's bounds (tests/test_ppo_kernels_gpu.py), taken from the kernel's own mu and
      sigma: actions = mu + sigma * eps within 2 U32 (|a| + |sigma eps|); logp: the kernel differences its own fp32 a and mu (d = a - mu
      carries U32 (|a| + |d|) of a's rounding), squares, scales by 1 / (2 sigma^2), subtracts log sigma and log sqrt(2 pi), and adds the A
      terms in a 5-level shuffle tree."""
    lib = _fl().load_ppo_library()
    for K in (1, 45, 128):
        for M in (1, 31, 33, 200):
            for A in (1, 10, 16, 17, 32):
                tag = (M, K, A, log_std)
                X, W, bias, eps = _head_case(M, K, A, A * 100000 + K * 1000 + M)
                if not log_std:
                    bias[A:] += 2.0   # (a sigma of order one: positive)
                got = _head(lib, X, W, bias, log_std, eps)
                want_mu, want_s = _layer(lib, X, W[:A], bias[:A]), _layer(lib, X, W[A:], bias[A:])
                assert torch.equal(got["mu"], want_mu), (tag, "mu")
                if log_std:
                    e = (torch.log(got["sigma"].double()) - want_s.double()).abs()
                    assert bool((e <= 2 * U32).all()), (tag, "log sigma", float(e.max() / U32))
                else:
                    assert torch.equal(got["sigma"], want_s), (tag, "sigma")
                    assert bool((got["sigma"] > 0).all())
                mu64, s64, _ = R.policy_head_sd_ref(X, W, bias, log_std)
                absprod = X.double().abs() @ W.double().abs().t() + bias.double().abs()
                tol = (K + 2) * U32 * absprod + 1e-30
                e = (got["mu"].double() - mu64).abs()
                assert bool((e <= tol[:, :A]).all()), (tag, "mu against float64", float((e / tol[:, :A]).max()))
                e = (want_s.double() - s64).abs()
                assert bool((e <= tol[:, A:]).all()), (tag, "s against float64", float((e / tol[:, A:]).max()))
                mu_, sd, ep = got["mu"].double(), got["sigma"].double(), eps.double()
                a64 = mu_ + sd * ep
                tol_a = 2 * U32 * (a64.abs() + (sd * ep).abs())
                e = (got["actions"].double() - a64).abs()
                assert bool((e <= tol_a).all()), (tag, "actions", float((e / tol_a).max()))
                logp64 = torch.distributions.Normal(mu_, sd).log_prob(a64).sum(-1)
                terms = -ep ** 2 / 2.0 - torch.log(sd) - R.LOG_SQRT_2PI
                dz = 2 * U32 * (a64.abs() + (sd * ep).abs()) / sd
                tol_l = (ep.abs() * dz + 2 * U32 * ep ** 2 + 4 * U32 * (torch.log(sd).abs() + 1.0)).sum(-1) + 8 * U32 * terms.abs().sum(-1)
                e = (got["logp"].double() - logp64).abs()
                assert bool((e <= tol_l).all()), (tag, "logp", float((e / tol_l).max()))
                again = _head(lib, X, W, bias, log_std, eps)   # the same inputs give the same bytes
                assert all(torch.equal(got[k], again[k]) for k in got), (tag, "determinism")


@pytest.mark.parametrize("structured", [False, True], ids=["random", "structured"])
@pytest.mark.parametrize("M,K,A", [(33, 45, 17), (130, 128, 32), (5, 1, 10), (200, 70, 16)])
def test_policy_head_sd_is_exact_on_integers(M, K, A, structured):
    """small integers: every product and partial sum is an integer below 2^24 (at most 128 * 64 + 8), so float32 is exact and mu and
    (`scalar`) sigma must equal the int64 result -- whatever the summation order; a wrong MFMA operand map, or a wrong map of W's two
    halves onto the tile, does not survive it.  Structured: every operand a different function of (row, k)."""
    lib = _fl().load_ppo_library()
    if structured:
        m, k, n = np.arange(M)[:, None], np.arange(K)[None, :], np.arange(2 * A)[:, None]
        x, w, b = (m + 3 * k) % 7 - 3, (2 * n + 5 * k) % 9 - 4, np.arange(2 * A) % 11 - 5
    else:
        g = np.random.default_rng(7)
        x, w, b = g.integers(-8, 9, (M, K)), g.integers(-8, 9, (2 * A, K)), g.integers(-8, 9, 2 * A)
    want = x.astype(np.int64) @ w.astype(np.int64).T + b
    f = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
    got = _head(lib, f(x), f(w), f(b), False, torch.zeros(M, A, device=DEV))
    assert np.array_equal(got["mu"].cpu().numpy().astype(np.int64), want[:, :A]) and (K == 1 or np.abs(want).max() > 16)
    assert np.array_equal(got["sigma"].cpu().numpy().astype(np.int64), want[:, A:])
    assert torch.equal(got["actions"], got["mu"])                                       # eps = 0


@pytest.mark.parametrize("log_std", [False, True], ids=["scalar", "log"])
def test_policy_head_sd_rows_do_not_depend_on_the_rows_beside_them(log_std):
    lib = _fl().load_ppo_library()
    M, K, A = 200, 45, 10
    X, W, bias, eps = _head_case(M, K, A, 9)
    if not log_std:
        bias[A:] += 2.0
    full = _head(lib, X, W, bias, log_std, eps)
    for r in (0, 31, 32, 127, 128, 199):
        one = _head(lib, X[r:r + 1].clone(), W, bias, log_std, eps[r:r + 1].clone())
        assert all(torch.equal(one[k][0], full[k][r]) for k in full), r


def test_policy_head_sd_rejects_invalid_arguments():
    lib = _fl().load_ppo_library()
    M, K, A = 70, 20, 10
    X, W, bias, eps = _head_case(M, K, A, 3)
    sentinel = -12345.0
    outs = {"actions": torch.full((M, A), sentinel, device=DEV), "logp": torch.full((M,), sentinel, device=DEV),
            "mu": torch.full((M, A), sentinel, device=DEV), "sigma": torch.full((M, A), sentinel, device=DEV)}
    ins = {"X": X, "W": W, "bias": bias, "eps": eps}

    def call(m=M, k=K, a=A, null=None):
        p = {n: (None if n == null else t.data_ptr()) for n, t in list(ins.items()) + list(outs.items())}
        return lib.grx_mlp_policy_head_sd(m, k, a, p["X"], p["W"], p["bias"], 1, p["eps"], p["actions"], p["logp"], p["mu"], p["sigma"], _stream())
    for m, k, a in ((0, K, A), (M, 0, A), (M, K, 0), (M, K, 33), (-1, K, A)):
        assert call(m, k, a) < 0, (m, k, a)
    for n in ("X", "W", "eps", "actions", "logp", "mu", "sigma"):
        assert call(null=n) < 0, n
    torch.cuda.synchronize()
    assert all(bool((t == sentinel).all()) for t in outs.values())
    assert call() == 0
    torch.cuda.synchronize()
    assert all(not bool((t == sentinel).any()) for t in outs.values())
    assert call(null="bias") == 0                                                          # (a layer without a bias is valid)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outs["logp"]).all())


# ---- the runner ------------------------------------------------------------------------------------------------------------------------------
FLAGS = {"log": ("--noise_std_type", "log"), "sd_scalar": ("--state_dependent_std",), "sd_log": ("--state_dependent_std", "--noise_std_type", "log")}


def _make(tmp_path, flags=(), steps=8, num_envs=64):
    from wiki_grx_gym_amd.envs import GR1T1Cfg, GR1T1CfgPPO
    from wiki_grx_gym_amd.utils import get_args, task_registry
    args = get_args(["--task", "GR1T1", "--headless", "--num_envs", str(num_envs), "--seed", "3", *flags])
    env, _ = task_registry.make_env("GR1T1", args=args, env_cfg=GR1T1Cfg())
    tcfg = GR1T1CfgPPO()
    tcfg.runner.num_steps_per_env = steps
    tcfg.algorithm.num_mini_batches = 4
    runner, _ = task_registry.make_alg_runner(env, name=None, args=args, train_cfg=tcfg, log_root=str(tmp_path) if tmp_path else None)
    return env, runner


def _captured_like_the_default(alg):
    """what the default does at this shape: the minibatch step and the policy step replayed from HIP graphs, the fused head in them"""
    return (alg._use_graph and isinstance(alg._graph, torch.cuda.CUDAGraph) and alg._use_act_graph
            and isinstance(alg._act_graph, torch.cuda.CUDAGraph) and alg._act_fused and alg._loss_is_fused())


@pytest.mark.parametrize("variant", list(FLAGS))
def test_train_save_load_play_export(tmp_path, monkeypatch, variant):
    from wiki_grx_gym_amd.rl.modules import ActorCriticMLP
    from wiki_grx_gym_amd.scripts.play import play
    from wiki_grx_gym_amd.utils import get_args, task_registry
    flags = list(FLAGS[variant])
    sd = "--state_dependent_std" in flags
    # (play() takes the registered config instance, which the flags write to: undone when the test ends)
    reg = task_registry.train_cfgs["GR1T1"]
    monkeypatch.setattr(reg.policy, "noise_std_type", "scalar", raising=False)
    monkeypatch.setattr(reg.policy, "state_dependent_std", False, raising=False)
    env, runner = _make(tmp_path, flags=tuple(flags))
    alg, ac = runner.alg, runner.alg.actor_critic
    assert type(ac) is ActorCriticMLP and ac.state_dependent_std == sd and alg._state_dependent == sd
    assert ac.actor.model[-1].weight.shape == ((20 if sd else 10), 128)
    before = {k: v.detach().clone() for k, v in ac.state_dict().items()}
    losses, sigmas, update = [], [], alg.update

    def recording_update():
        sigmas.append(alg.storage.sigma.clone())
        losses.append(update())
        return losses[-1]
    alg.update = recording_update
    runner.learn(num_learning_iterations=2, init_at_random_ep_len=True)
    assert len(losses) == 2 and all(np.isfinite(v) for pair in losses for v in pair), losses
    assert _captured_like_the_default(alg)
    after = ac.state_dict()
    assert all(torch.isfinite(v).all() for v in after.values())
    assert not torch.equal(before["actor.model.6.weight"], after["actor.model.6.weight"])
    if sd:
        assert not torch.equal(before["actor.model.6.weight"][10:], after["actor.model.6.weight"][10:]) and "std" not in after and "log_std" not in after
        assert bool((sigmas[0] == sigmas[0][:, :1]).all())                                  # zero s weights: one sigma for every env ...
        assert bool((sigmas[1] != sigmas[1][:, :1]).any(1).all())                           # ... and after the first update the rows differ
        assert "log" not in flags or float(sigmas[1].min()) > 0.0
    else:
        assert not torch.equal(before["log_std"], after["log_std"]) and "std" not in after
        assert torch.equal(sigmas[1][0, 0], sigmas[1][-1, -1]) and not torch.equal(sigmas[0][0, 0], sigmas[1][0, 0])
    ck = torch.load(os.path.join(runner.log_dir, "model_2.pt"), weights_only=False)
    want = {"std_type": "log" if "log" in flags else "scalar", "state_dependent": sd}
    assert ck["noise"] == want and set(ck) == {"model_state_dict", "optimizer_state_dict", "iter", "infos", "noise"}

    with pytest.raises(ValueError, match="--noise_std_type"):                               # play without the flags refuses the checkpoint
        play(get_args(["--task", "GR1T1", "--headless", "--seed", "3"]), steps=1, log_root=str(tmp_path))
    out = play(get_args(["--task", "GR1T1", "--headless", "--seed", "3"] + flags), steps=20, log_root=str(tmp_path))
    assert len(open(out["states"]).readlines()) == 20
    penv, prunner = out["env"], out["runner"]
    loaded = prunner.alg.actor_critic.state_dict()
    assert all(torch.equal(loaded[k], v) for k, v in after.items())
    policy = prunner.get_inference_policy(device=penv.device)
    jit = torch.jit.load(out["exported"])                                                   # on the CPU
    obs, worst = penv.get_observations(), 0.0
    with torch.no_grad():
        for _ in range(20):
            actions = policy(obs.detach())
            a = jit(obs.detach().cpu())
            assert a.shape == (penv.num_envs, 10) and actions.shape == (penv.num_envs, 10)
            worst = max(worst, float((a - actions.cpu()).abs().max()))
            obs = penv.step(actions.detach())[0]
    print(f"{variant}: exported module against the device policy over 20 steps: max |difference| {worst:.3g}")
    assert worst < 1e-6


def test_state_dependent_composes_with_normalisation_and_history(tmp_path):
    env, runner = _make(tmp_path, flags=("--state_dependent_std", "--empirical_normalization", "--obs_history", "3"))
    ac = runner.alg.actor_critic
    assert ac.actor.model[0].in_features == 3 * 39 and ac.actor.model[-1].out_features == 20
    losses, update = [], runner.alg.update

    def recording_update():
        losses.append(update())
        return losses[-1]
    runner.alg.update = recording_update
    runner.learn(num_learning_iterations=1)
    assert len(losses) == 1 and all(np.isfinite(v) for v in losses[0]) and _captured_like_the_default(runner.alg)
    assert all(torch.isfinite(v).all() for v in ac.state_dict().values())


def test_default_path_is_unchanged(tmp_path):
    from wiki_grx_gym_amd.rl.modules import ActorCriticMLP
    env, runner = _make(tmp_path, flags=())
    ac = runner.alg.actor_critic
    assert type(ac) is ActorCriticMLP and runner.noise is None and not runner.alg._state_dependent
    assert ac.noise_std() is ac.std and ac.inference_actor() is ac.actor and ac.actor.model[-1].weight.shape == (10, 128)
    runner.learn(num_learning_iterations=1)
    assert _captured_like_the_default(runner.alg)
    ck = torch.load(os.path.join(runner.log_dir, "model_1.pt"), weights_only=False)
    assert set(ck) == {"model_state_dict", "optimizer_state_dict", "iter", "infos"} and "noise" not in ck
    assert "std" in ck["model_state_dict"] and "log_std" not in ck["model_state_dict"]
    assert ck["model_state_dict"]["actor.model.6.weight"].shape == (10, 128)


# ---- the captured step against the eager step and float64 -------------------------------------------------------------------------------------
def test_captured_step_equals_the_eager_step():
    """State-dependent `log`, one minibatch of 4096 rows on the GR1T1 networks: the parameter gradients of the eager step (PPO._losses +
    backward, as the graph build's dry runs run it) and of the captured step (PPO._build_graph, one replay) each within
    1e-4 * max |g_ref| per tensor of a float64 copy of the policy under tests/noise_ref.py's loss, and of each other --
    test_minibatch_parameter_gradients_match_float64's bound (tests/test_ppo_kernels_gpu.py): the weight gradients are fp32 GEMMs summed
    over the rows (U32 * sqrt(4096) ~ 4e-6 relative for random-signed terms), fed by a loss gradient good to ~1e-5 relative.

    The two steps run on two copies of the policy with the same weights, as tests/test_ppo_kernels_gpu.py runs them in two tests: autograd's
    AccumulateGrad nodes remember the stream of their first backward (PPO._build_graph's comment), so parameters that have been through an
    eager backward on the default stream cannot be captured on another one afterwards."""
    from wiki_grx_gym_amd.rl.modules import ActorCriticMLP
    from wiki_grx_gym_amd.rl.ppo import PPO
    torch.manual_seed(11)
    A, mb = 10, 4096
    ac = ActorCriticMLP(39, 168, A, actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[512, 256, 128], activation="elu", init_noise_std=0.2,
                        noise_std_type="log", state_dependent_std=True)
    with torch.no_grad():
        ac.actor.model[-1].weight[A:].copy_(0.05 * torch.randn(A, 128))                    # sigma depends on the state
    ac64 = copy.deepcopy(ac).double().to(DEV)
    ac_captured = copy.deepcopy(ac)
    alg_captured = PPO(ac_captured, clip_param=CLIP, value_loss_coef=1.0, entropy_coef=0.01, use_clipped_value_loss=True, schedule="adaptive",
                       desired_kl=0.01, device=DEV)
    alg = PPO(ac, clip_param=CLIP, value_loss_coef=1.0, entropy_coef=0.01, use_clipped_value_loss=True, schedule="adaptive", desired_kl=0.01,
              device=DEV)
    assert alg._fused_loss and alg._state_dependent and alg._use_graph
    g = _gen(mb + A)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)
    obs, cobs = r(mb, 39), r(mb, 168)
    with torch.no_grad():
        mu64, sigma64 = R.policy_sigma(ac64, obs.double())
        v64 = ac64.critic.model(cobs.double())
        assert float((sigma64.max(0).values / sigma64.min(0).values).min()) > 1.01
        actions = (mu64 + sigma64 * r(mb, A).double()).float()
        old_mu = (mu64 + 0.1 * sigma64 * r(mb, A).double()).float()
        old_sigma = (sigma64 * (1.0 + 0.1 * torch.rand(mb, A, device=DEV, generator=g).double())).float()
        tv, ret, adv = (v64 + 0.3 * r(mb, 1).double()).float(), (v64 + r(mb, 1).double()).float(), r(mb, 1)
        logp = torch.distributions.Normal(mu64, sigma64).log_prob(actions.double()).sum(-1, keepdim=True)
        old_logp = (logp + 0.25 * r(mb, 1).double()).float()
        for _ in range(20):
            bad = ppo_ref.loss_near_ties(mu64, sigma64, v64, actions, old_logp, ret, tv, CLIP)
            if not bool(bad.any()):
                break
            b = bad.reshape(-1, 1)
            old_logp = torch.where(b, old_logp - 0.01, old_logp)
            tv = torch.where(b, tv + 0.013, tv)
            ret = torch.where(b, ret + 0.011, ret)
        assert not bool(ppo_ref.loss_near_ties(mu64, sigma64, v64, actions, old_logp, ret, tv, CLIP).any())
    batch = [obs, cobs, actions, tv, adv, ret, old_logp, old_mu, old_sigma]
    mean, sigma = R.policy_sigma(ac64, obs.double())
    t = R.loss_terms(mean, sigma, ac64.critic.model(cobs.double()), actions.double(), old_logp.double(), old_mu.double(), old_sigma.double(),
                     adv.double(), ret.double(), tv.double(), CLIP, 1.0, 0.01, True)
    t["loss"].backward()
    alg_captured.init_storage(16, 2)   # (_build_graph takes its buffer widths from the storage)
    alg_captured._build_graph(mb)
    assert isinstance(alg_captured._graph, torch.cuda.CUDAGraph)
    for buf, x in zip(alg_captured._static, batch):
        buf.copy_(x)
    alg_captured._graph.replay()
    torch.cuda.synchronize()
    with alg._blas_for_update():
        s, v, loss, kl = alg._losses(*batch)
        alg.optimizer.zero_grad(set_to_none=True)
        loss.backward()
    torch.cuda.synchronize()
    assert abs(float(loss.detach()) - float(t["loss"])) <= 1e-4 * (abs(float(t["surrogate"])) + float(t["value_loss"]) + 0.01 * float(t["entropy_rows"].abs().mean()))
    eager = {n: p.grad.detach().clone() for n, p in ac.named_parameters()}
    for (n, p), q in zip(ac_captured.named_parameters(), ac64.parameters()):
        tol = 1e-4 * float(q.grad.abs().max())
        assert tol > 0, n
        for what, got in (("eager", eager[n]), ("captured", p.grad)):
            err = float((got.double() - q.grad).abs().max())
            assert err <= tol, (what, n, err, tol)
        err = float((p.grad - eager[n]).abs().max())
        assert err <= tol, ("captured against eager", n, err, tol)
