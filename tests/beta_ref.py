"""float64 reference of the Beta policy's loss, built on torch.distributions.Beta / kl_divergence and autograd -- not on
rl/beta.py's own spellings, which are what the tests compare against it -- and the data the CPU and the GPU tests share."""
import torch
from torch.distributions import Beta, kl_divergence

X_MIN, X_MAX = 2.0 ** -24, 1.0 - 2.0 ** -24


def params64(raw):
    """(alpha, beta) in float64 of a raw output [B, 2A] (softplus with torch's threshold of 20)"""
    raw = raw.double()
    A = raw.shape[-1] // 2
    sp = torch.nn.functional.softplus
    return 1.0 + sp(raw[..., :A]), 1.0 + sp(raw[..., A:])


def loss64(raw, value, x, old_logp, old_alpha, old_beta, adv, ret, tv, clip, vcoef, ecoef, use_clipped):
    """-> dict of float64 tensors: out [4] = (surrogate, value loss, total, mean KL), d_raw, d_value, and the per-row logp / entropy / kl"""
    raw = raw.detach().double().requires_grad_(True)
    value = value.detach().double().reshape(-1).requires_grad_(True)
    x, old_logp, old_alpha, old_beta, adv, ret = (t.detach().double() for t in (x, old_logp.reshape(-1), old_alpha, old_beta, adv.reshape(-1),
                                                                                ret.reshape(-1)))
    alpha, beta = params64(raw)
    d = Beta(alpha, beta, validate_args=False)
    logp, ent = d.log_prob(x).sum(-1), d.entropy().sum(-1)
    kl = kl_divergence(Beta(old_alpha, old_beta, validate_args=False), Beta(alpha.detach(), beta.detach(), validate_args=False)).sum(-1)
    ratio = torch.exp(logp - old_logp)
    surr = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1.0 - clip, 1.0 + clip)).mean()
    if use_clipped:
        tv = tv.detach().double().reshape(-1)
        vc = tv + (value - tv).clamp(-clip, clip)
        vl = torch.max((value - ret).pow(2), (vc - ret).pow(2)).mean()
    else:
        vl = (ret - value).pow(2).mean()
    loss = surr + vcoef * vl - ecoef * ent.mean()
    loss.backward()
    return {"out": torch.stack([surr, vl, loss, kl.mean()]).detach(), "d_raw": raw.grad, "d_value": value.grad,
            "logp": logp.detach(), "entropy": ent.detach(), "kl": kl.detach(), "alpha": alpha.detach(), "beta": beta.detach()}


def softplus_inv(y):
    y = y.double()
    return torch.where(y > 30.0, y, torch.log(torch.expm1(y.clamp(max=30.0))))


def make_batch(B, A, setting, seed, device="cpu"):
    """one minibatch of the loss, fp32: `setting` = "init" (alpha, beta in 1..80, around what the initialisation gives) or "concentrated"
    (alpha + beta ~ 2000).  The old policy is the new one moved a little, x a draw from the old one, old_logp its log-probability in
    float64 rounded to fp32 -- so the ratios scatter around 1 and both clip branches occur."""
    g = torch.Generator().manual_seed(seed)
    if setting == "init":
        a0 = 1.0 + 79.0 * torch.rand(B, A, generator=g, dtype=torch.float64) ** 2
        b0 = 1.0 + 79.0 * torch.rand(B, A, generator=g, dtype=torch.float64) ** 2
    else:
        m = 0.1 + 0.8 * torch.rand(B, A, generator=g, dtype=torch.float64)
        s = 2000.0 * (0.9 + 0.2 * torch.rand(B, A, generator=g, dtype=torch.float64))
        a0, b0 = 1.0 + (s - 2.0) * m, 1.0 + (s - 2.0) * (1.0 - m)
    old_alpha, old_beta = a0.float(), b0.float()
    step = 0.03 if setting == "init" else 0.003
    raw = torch.cat([softplus_inv((old_alpha.double() - 1.0) * (1.0 + step * torch.randn(B, A, generator=g, dtype=torch.float64)).clamp(min=0.5) + 1e-3),
                     softplus_inv((old_beta.double() - 1.0) * (1.0 + step * torch.randn(B, A, generator=g, dtype=torch.float64)).clamp(min=0.5) + 1e-3)],
                    -1).float()
    g1 = torch._standard_gamma(old_alpha.double(), generator=g)
    g2 = torch._standard_gamma(old_beta.double(), generator=g)
    x = (g1 / (g1 + g2)).float().clamp(X_MIN, X_MAX)
    old_logp = Beta(old_alpha.double(), old_beta.double(), validate_args=False).log_prob(x.double()).sum(-1).float()
    value = torch.randn(B, generator=g)
    tv = value + 0.3 * torch.randn(B, generator=g)
    ret = value + torch.randn(B, generator=g)
    adv = torch.randn(B, generator=g)
    return tuple(t.to(device) for t in (raw, value, x, old_logp, old_alpha, old_beta, adv, ret, tv))


CLIP, VCOEF, ECOEF = 0.2, 1.0, 0.01


# ---- tolerances: an ulp-counted first-order model from the float64 partials per row (tests/test_noise_std_gpu.py::_tolerances' construction) ----
U32 = 2.0 ** -24   # the fp32 unit roundoff


def _ratio_error(d, a, b, fn_ulps):
    """R_row: what an fp32 evaluation may lose of a row's ratio = exp(logp - old_logp), relative (see tolerances)"""
    raw, value, x, old_logp, a0, b0, adv, ret, tv = (t.double() for t in d)
    A = x.shape[-1]
    s = a + b
    lg, psi = torch.lgamma, torch.digamma
    lx, l1x = torch.log(x), torch.log1p(-x)
    dla, dlb = lx - psi(a) + psi(s), l1x - psi(b) + psi(s)
    lgs = lg(a).abs() + lg(b).abs() + lg(s).abs()
    terms = ((a - 1) * lx).abs() + ((b - 1) * l1x).abs() + (lg(a) + lg(b) - lg(s)).abs()
    return (U32 * ((A + 4) * terms.sum(-1) + 2 * ((a - 1) + (b - 1)).sum(-1) + 2 * old_logp.reshape(-1).abs() + 8)
            + (dla.abs() * 4 * U32 * a + dlb.abs() * 4 * U32 * b).sum(-1) + fn_ulps["lgamma"] * U32 * lgs.sum(-1))


def _branches(d, logp, clip, margin=1e-3):
    """per row in float64: (ratio, the factor of -adv that reaches the ratio's gradient, whether the row is within `margin` -- relative, a
    number or one per row -- of a branch)"""
    raw, value, x, old_logp, a0, b0, adv, ret, tv = d
    ratio = torch.exp(logp - old_logp.double())
    adv, v, ret, tv = adv.double(), value.double(), ret.double(), tv.double()
    s1, s2 = -adv * ratio, -adv * ratio.clamp(1.0 - clip, 1.0 + clip)
    inside = (ratio >= 1.0 - clip) & (ratio <= 1.0 + clip)
    w = torch.where(s1 > s2, torch.ones_like(ratio), inside.double())
    dv = v - tv
    l1, l2 = (v - ret) ** 2, (tv + dv.clamp(-clip, clip) - ret) ** 2
    near = ((ratio - (1.0 - clip)).abs() < margin * ratio) | ((ratio - (1.0 + clip)).abs() < margin * ratio) | ((dv.abs() - clip).abs() < 1e-3) \
        | ((l1 - l2).abs() < 1e-3 * (l1 + l2 + 1e-3)) & ~((dv.abs() <= clip))
    return ratio, w, near


def move_off_ties(d, clip):
    """the batch with the rows that sit close to a branch of the loss (the ratio's clip, the value clip, the value loss's max) moved off it.
    Close: within 1e-3, and for the ratio's clip within three times what an fp32 evaluation with 2-ulp special functions may lose of the ratio
    (where alpha + beta is in the thousands that is per cents: such a row's gradient is decided by rounding, in any fp32 spelling)"""
    raw, value, x, old_logp, a0, b0, adv, ret, tv = d
    al, be = params64(raw)
    logp = Beta(al, be, validate_args=False).log_prob(x.double()).sum(-1)
    fn2 = {"lgamma": 2.0, "digamma": 2.0, "trigamma": 2.0}
    for _ in range(40):
        margin = (3.0 * _ratio_error((raw, value, x, old_logp, a0, b0, adv, ret, tv), al, be, fn2)).clamp(min=1e-3)
        _, _, near = _branches((raw, value, x, old_logp, a0, b0, adv, ret, tv), logp, clip, margin)
        if not bool(near.any()):
            break
        up = torch.exp(logp - old_logp.double()) > 1.0   # (away from 1: a row between the two clips at a wide margin leaves on its own side)
        old_logp = torch.where(near, torch.where(up, old_logp - 0.05, old_logp + 0.05), old_logp)
        tv = torch.where(near, tv + 0.013, tv)
        ret = torch.where(near, ret + 0.011, ret)
    margin = (3.0 * _ratio_error((raw, value, x, old_logp, a0, b0, adv, ret, tv), al, be, fn2)).clamp(min=1e-3)
    assert not bool(_branches((raw, value, x, old_logp, a0, b0, adv, ret, tv), logp, clip, margin)[2].any())
    return raw, value, x, old_logp, a0, b0, adv, ret, tv


def tolerances(d, ref, fn_ulps, clip=CLIP, vcoef=VCOEF, ecoef=ECOEF):
    """Tolerances of grx_ppo_loss_beta's outputs against loss64, per element, from the float64 partials of each row.

    What an fp32 evaluation may lose, counted in U32 = 2^-24:
      * alpha = 1 + softplus(p) through fp32 expf / log1pf: 4 U32 alpha (and beta likewise) -- every quantity below inherits it through
        its float64 partial derivative with respect to alpha and beta (digamma, trigamma and tetragamma differences);
      * a special-function value f: fn_ulps[name] U32 |f| -- fn_ulps is twice what profiles/beta_policy_parity.json records for
        grx_beta_functions against float64;
      * a sum of n terms: (n + 4) U32 (sum of the terms' magnitudes); a log, exp or product: a few U32 of its value.
    A row's ratio = exp(logp - old_logp) has the relative error R_row; the gradient rows inherit it through g_logp.  The batch sums run in
    double: the per-row errors averaged, plus the final rounding."""
    raw, value, x, old_logp, a0, b0, adv, ret, tv = (t.double().cpu() for t in d)
    B_, A = x.shape
    a, b = ref["alpha"].cpu(), ref["beta"].cpu()
    s = a + b
    psi, tri, tet = torch.digamma, (lambda t: torch.polygamma(1, t)), (lambda t: torch.polygamma(2, t))
    lg = torch.lgamma
    Flg, Fdg, Ftg = (fn_ulps[k] * U32 for k in ("lgamma", "digamma", "trigamma"))
    ca, cb = 4 * U32 * a, 4 * U32 * b
    lx, l1x = torch.log(x), torch.log1p(-x)
    dla, dlb = lx - psi(a) + psi(s), l1x - psi(b) + psi(s)
    dha, dhb = -(a - 1) * tri(a) + (s - 2) * tri(s), -(b - 1) * tri(b) + (s - 2) * tri(s)
    lgs = lg(a).abs() + lg(b).abs() + lg(s).abs()
    R_row = _ratio_error((raw, value, x, old_logp, a0, b0, adv, ret, tv), a, b, fn_ulps)
    ratio, w, _ = _branches(d if d[0].device.type == "cpu" else tuple(t.cpu() for t in d), ref["logp"].cpu(), clip)
    g_logp = (-adv * w * ratio / B_).abs().unsqueeze(-1)
    g_ent = ecoef / B_
    sp, sq = torch.sigmoid(raw[:, :A]), torch.sigmoid(raw[:, A:])
    E_dla = (tri(s) - tri(a)).abs() * ca + tri(s) * cb + (Fdg + 4 * U32) * (psi(a).abs() + psi(s).abs()) + 4 * U32 * lx.abs()
    E_dlb = (tri(s) - tri(b)).abs() * cb + tri(s) * ca + (Fdg + 4 * U32) * (psi(b).abs() + psi(s).abs()) + 4 * U32 * l1x.abs()
    cross = (tri(s) + (s - 2) * tet(s)).abs()
    E_dha = (cross - tri(a) - (a - 1) * tet(a)).abs() * ca + cross * cb + (Ftg + 4 * U32) * ((a - 1) * tri(a) + (s - 2) * tri(s))
    E_dhb = (cross - tri(b) - (b - 1) * tet(b)).abs() * cb + cross * ca + (Ftg + 4 * U32) * ((b - 1) * tri(b) + (s - 2) * tri(s))
    halves = []
    for half, E_l, E_h, dl, dh, sg in ((ref["d_raw"][:, :A].cpu(), E_dla, E_dha, dla, dha, sp), (ref["d_raw"][:, A:].cpu(), E_dlb, E_dhb, dlb, dhb, sq)):
        halves.append(g_logp * sg * E_l + g_ent * sg * E_h + (R_row.unsqueeze(-1) + 8 * U32) * ((g_logp * dl * sg).abs() + (g_ent * dh * sg).abs())
                      + 4 * U32 * float(half.abs().max()))
    ops = value.abs() + tv.abs() + ret.abs() + clip
    tol_value = 16 * U32 * 2.0 * vcoef / B_ * ops
    s0 = a0 + b0
    kl_terms = (lg(a).abs() + lg(b).abs() + lg(s).abs() + lg(a0).abs() + lg(b0).abs() + lg(s0).abs())
    kl_psi = (a0 - a).abs() * psi(a0).abs() + (b0 - b).abs() * psi(b0).abs() + (s - s0).abs() * psi(s0).abs()
    E_kl = ((psi(a) - psi(s) - psi(a0) + psi(s0)).abs() * ca + (psi(b) - psi(s) - psi(b0) + psi(s0)).abs() * cb
            + (Flg + (A + 4) * U32) * kl_terms + (Fdg + (A + 4) * U32) * kl_psi + 4 * U32 * (psi(a0).abs() + psi(b0).abs() + psi(s0).abs()) * (a + b))
    ent_terms = (a - 1) * psi(a).abs() + (b - 1) * psi(b).abs() + (s - 2) * psi(s).abs()
    E_ent = dha.abs() * ca + dhb.abs() * cb + (Flg + (A + 4) * U32) * lgs + (Fdg + (A + 4) * U32) * ent_terms
    surr_rows = (adv * ratio).abs()
    out = ref["out"].cpu()
    tol_out = torch.zeros(4, dtype=torch.float64)
    tol_out[0] = float((R_row * surr_rows).mean()) + 2 * U32 * float(out[0].abs()) + 2 * U32 * float(surr_rows.mean())
    tol_out[1] = 4 * U32 * float((ops ** 2).mean()) + 2 * U32 * float(out[1].abs())
    tol_out[3] = float(E_kl.sum(-1).mean()) + 2 * U32 * float(out[3].abs())
    tol_out[2] = tol_out[0] + vcoef * tol_out[1] + ecoef * float(E_ent.sum(-1).mean()) + 2 * U32 * float(out[2].abs())
    return {"R_row": R_row, "p": halves[0], "q": halves[1], "d_value": tol_value, "out": tol_out}


def loss_errors(got_out, got_d_raw, got_d_value, ref, tol):
    """the largest error / tolerance per output tensor"""
    A = ref["alpha"].shape[-1]
    g = lambda t: t.detach().double().cpu()
    return {"out": [float(v) for v in ((g(got_out) - ref["out"].cpu()).abs() / tol["out"])],
            "d_raw_p": float(((g(got_d_raw)[:, :A] - ref["d_raw"][:, :A].cpu()).abs() / tol["p"]).max()),
            "d_raw_q": float(((g(got_d_raw)[:, A:] - ref["d_raw"][:, A:].cpu()).abs() / tol["q"]).max()),
            "d_value": float(((g(got_d_value).reshape(-1) - ref["d_value"].cpu()).abs() / tol["d_value"]).max())}


def torch_fp32_loss(d, use_clipped, clip=CLIP, vcoef=VCOEF, ecoef=ECOEF):
    """rl/beta.py's torch spelling in fp32 on the CPU: (out [4], d_raw, d_value) -- the reference whose own error shows the data is fair"""
    from wiki_grx_gym_amd.rl import beta as B
    raw, value, x, old_logp, a0, b0, adv, ret, tv = (t.detach().float().cpu() for t in d)
    raw, value = raw.clone().requires_grad_(True), value.clone().requires_grad_(True)
    s, vl, loss, kl = B.loss_torch(raw, value, x, old_logp, a0, b0, adv, ret, tv, clip, vcoef, ecoef, use_clipped)
    loss.backward()
    return torch.stack([s, vl, loss, kl]).detach(), raw.grad, value.grad


# ---- grx_beta_functions against float64 ---------------------------------------------------------------------------------------------------------
def function_grid():
    """4096 log-spaced points in [1, 1e4] plus 1, 2 and the integers up to 64, as fp32"""
    import numpy as np
    t = np.concatenate([np.logspace(0.0, 4.0, 4096), np.arange(1.0, 65.0)])
    return torch.tensor(t, dtype=torch.float32)


def ulp_errors(got, ref64):
    """|got - ref| in fp32 ulps of the float64 value (the spacing of fp32 at |ref|, the subnormals' below 2^-126)"""
    ref64 = ref64.double()
    e = torch.floor(torch.log2(ref64.abs().clamp(min=2.0 ** -126)))
    return (got.double() - ref64).abs() / torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 23.0)


def function_refs(t):
    t = t.double()
    return {"lgamma": torch.lgamma(t), "digamma": torch.digamma(t), "trigamma": torch.polygamma(1, t)}


PARITY_JSON = "profiles/beta_policy_parity.json"
LOSS_CASES = [(Bn, A, setting, clipped) for setting in ("init", "concentrated") for A in (1, 10, 32) for Bn in (1, 255, 4097)
              for clipped in (True, False)]


def loss_case(Bn, A, setting, device="cpu"):
    d = move_off_ties(make_batch(Bn, A, setting, seed=1000 * A + Bn + (7 if setting == "init" else 0)), CLIP)
    return tuple(t.to(device) for t in d)
