"""Float64 restatements of the PPO kernels of libgrx_ppo.so (include/grx_ppo.h), used by tests/test_ppo_kernels_gpu.py to
judge the kernels and checked themselves against torch on the CPU by tests/test_ppo_ref.py.

Every function takes the kernel's fp32 inputs, promotes them to float64 and restates the operation the way rsl_rl spells it
(rsl_rl/algorithms/ppo.py:215-245, torch.nn.utils.clip_grad_norm_, torch.optim.Adam): no kernel code is imitated, so a
kernel that is subtly wrong disagrees with these."""
import math

import numpy as np
import torch

LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)
U32 = 2.0 ** -24   # unit roundoff of fp32


def _d(t):
    return t.detach().double()


def ppo_loss_ref(mu, std, value, actions, old_logp, old_mu, old_sigma, advantages, returns, target_values,
                 clip, value_loss_coef, entropy_coef, use_clipped_value_loss):
    """The minibatch loss of PPO._losses' torch spelling in float64 autograd, with Normal.log_prob / entropy written out.

    mu [B, A], std [A]; value, old_logp, advantages, returns, target_values [B] or [B, 1]; actions, old_mu, old_sigma [B, A].
    Returns dict: out = [surrogate, value_loss, total, mean KL], d_mu, d_std, d_value (the gradients of the total loss) and
    `scale`: for each of the four scalars and d_std, the same sum with every term replaced by its magnitude -- what the
    rounding of a sum of per-row terms is proportional to."""
    mu, std, value = (_d(t).requires_grad_() for t in (mu, std, value))
    actions, old_mu, old_sigma = _d(actions), _d(old_mu), _d(old_sigma)
    old_logp, adv, ret, tv = (_d(t).reshape(-1) for t in (old_logp, advantages, returns, target_values))
    v = value.reshape(-1)
    sigma = mu * 0.0 + std
    logp = (-(actions - mu) ** 2 / (2.0 * sigma ** 2) - torch.log(sigma) - LOG_SQRT_2PI).sum(-1)
    entropy = (0.5 + LOG_SQRT_2PI + torch.log(sigma)).sum(-1)
    with torch.no_grad():
        kl_rows = (torch.log(sigma / old_sigma + 1.e-5) + (old_sigma ** 2 + (old_mu - mu) ** 2) / (2.0 * sigma ** 2) - 0.5).sum(-1)
    ratio = torch.exp(logp - old_logp)
    surr_rows = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1.0 - clip, 1.0 + clip))
    if use_clipped_value_loss:
        clipped = tv + (v - tv).clamp(-clip, clip)
        vl_rows = torch.max((v - ret) ** 2, (clipped - ret) ** 2)
    else:
        vl_rows = (ret - v) ** 2
    surrogate, value_loss = surr_rows.mean(), vl_rows.mean()
    loss = surrogate + value_loss_coef * value_loss - entropy_coef * entropy.mean()
    d_mu, d_std, d_value = torch.autograd.grad(loss, (mu, std, value))
    with torch.no_grad():
        B = mu.shape[0]
        # d_std = sum over rows of d(surrogate row)/d(logp) * d(logp)/d(std) - entropy_coef / std; a row's term is bounded by
        # |adv| ratio / B * ((a - mu)^2 / std^3 + 1 / std)
        z2 = ((actions - mu) / sigma) ** 2
        row_std = (ratio.abs() * adv.abs() / B).unsqueeze(-1) * (z2 + 1.0) / sigma
        s_abs = (surr_rows.abs().mean(), vl_rows.abs().mean(), kl_rows.abs().mean())
        total_abs = s_abs[0] + abs(value_loss_coef) * s_abs[1] + abs(entropy_coef) * entropy.abs().mean()
        scale = {"out": torch.stack([s_abs[0], s_abs[1], total_abs, s_abs[2]]),
                 "d_std": row_std.sum(0) + abs(entropy_coef) / std.detach()}
    out = torch.stack([surrogate.detach(), value_loss.detach(), loss.detach(), kl_rows.mean()])
    return {"out": out, "d_mu": d_mu, "d_std": d_std, "d_value": d_value.reshape(value.shape), "scale": scale}


def loss_near_ties(mu, std, value, actions, old_logp, returns, target_values, clip, margin=1e-3):
    """Rows whose float64 arithmetic lies within `margin` of a branch of the loss, where fp32 rounding may take the other one:
    a ratio near 1 - clip or 1 + clip (clamp's gradient switches), |value - target| near clip, and -- with the value clipped --
    the two squared errors of torch.max near each other.  (An exact tie inside the clip interval is not a near tie: there the
    two arms of max are the same number in any precision and share the gradient half / half.)  Returns a bool mask [B]."""
    mu, std, actions = _d(mu), _d(std), _d(actions)
    old_logp, v, ret, tv = (_d(t).reshape(-1) for t in (old_logp, value, returns, target_values))
    logp = (-(actions - mu) ** 2 / (2.0 * std ** 2) - torch.log(std) - LOG_SQRT_2PI).sum(-1)
    ratio = torch.exp(logp - old_logp)
    bad = ((ratio - (1.0 - clip)).abs() < margin) | ((ratio - (1.0 + clip)).abs() < margin)
    dv = v - tv
    bad |= ((dv.abs() - clip).abs() < margin)
    vc = tv + dv.clamp(-clip, clip)
    l1, l2 = (v - ret) ** 2, (vc - ret) ** 2
    bad |= (dv.abs() > clip) & ((l1 - l2).abs() < margin * (l1 + l2 + margin))
    return bad


def policy_head_ref(X, W, bias, std, eps):
    """grx_mlp_policy_head in float64: mu = X W^T + b, actions = mu + std * eps, sigma = std broadcast,
    logp = Normal(mu, std).log_prob(actions).sum(-1)."""
    X, W, std, eps = _d(X), _d(W), _d(std), _d(eps)
    mu = X @ W.t() + (_d(bias) if bias is not None else 0.0)
    actions = mu + std * eps
    sigma = std.expand_as(mu)
    logp = torch.distributions.Normal(mu, sigma).log_prob(actions).sum(-1)
    return {"mu": mu, "actions": actions, "sigma": sigma, "logp": logp}


def lr_rule_fp32(lr, kl, adaptive, desired_kl, lr_min, lr_max):
    """PPO.update_learning_rate (ppo.py:205-213) in the arithmetic PPO._device_lr_update runs on a HIP device: fp32 scalars, lr / 1.5
    as lr times the fp32 reciprocal of 1.5 (how torch divides a device tensor by a host number), clamped.  Returns np.float32."""
    f = np.float32
    lr, kl = f(lr), f(kl)
    if not adaptive:
        return lr
    down = max(f(lr * (f(1.0) / f(1.5))), f(lr_min))
    up = min(f(lr * f(1.5)), f(lr_max))
    if kl > f(desired_kl) * f(2.0):
        return down
    if f(desired_kl) / f(2.0) > kl > f(0.0):
        return up
    return lr


def step_tail_ref(params, grads, exp_avg, exp_avg_sq, steps, lr, loss, bad_flag, max_grad_norm, beta1, beta2, eps):
    """The step tail of one minibatch in float64 after the learning rate is decided (grx_ppo_step_tail, launch 2):
    NaN-skip, nn.utils.clip_grad_norm_ (norm of the per-tensor 2-norms, max_norm / (total + 1e-6) clamped to 1, every
    gradient scaled) and torch.optim.Adam.step() (no weight decay / amsgrad / maximize; bias corrections from the step
    counter after its increment).  `lr` is the learning rate in force for this step.  Lists of tensors in, new lists out
    (params, exp_avg, exp_avg_sq, steps as float64) plus the total norm and the clip coefficient."""
    P, G, M, V = ([_d(t) for t in ts] for ts in (params, grads, exp_avg, exp_avg_sq))
    S = [float(s) for s in steps]
    bad = (not math.isfinite(float(loss))) or (bad_flag is not None and float(bad_flag) != 0.0)
    norms = torch.stack([g.reshape(-1).norm(2.0) for g in G])
    total = float(norms.norm(2.0))
    clip = min(max_grad_norm / (total + 1e-6), 1.0)
    if bad:
        return {"params": P, "exp_avg": M, "exp_avg_sq": V, "steps": S, "total": total, "clip": clip, "skipped": True}
    lr = float(lr)
    P2, M2, V2, S2 = [], [], [], []
    for p, g, m, v, s in zip(P, G, M, V, S):
        s = s + 1.0
        g = g * clip
        m = beta1 * m + (1.0 - beta1) * g
        v = beta2 * v + (1.0 - beta2) * g * g
        bc1 = 1.0 - beta1 ** s
        bc2 = 1.0 - beta2 ** s
        p = p - (lr / bc1) * m / (torch.sqrt(v) / math.sqrt(bc2) + eps)
        P2.append(p); M2.append(m); V2.append(v); S2.append(s)
    return {"params": P2, "exp_avg": M2, "exp_avg_sq": V2, "steps": S2, "total": total, "clip": clip, "skipped": False}
