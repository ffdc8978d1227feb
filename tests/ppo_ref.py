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


class TorchSpelling:
    """PPO's own fp32 torch spelling of the minibatch loss on the inputs' device -- the branch PPO._losses takes with the fused loss off,
    differentiated by autograd -- as the reference where float64 cannot serve: at the extremes, underflow of sigma^2 and overflow of exp are
    fp32 facts.  The networks of a real PPO are replaced by identities, so that _losses' `obs` IS the actor's output (mu [B, A], or the raw
    [mean | s] of a state-dependent sigma: noise "scalar" / "log" with state_dependent) and `cobs` the critic's."""

    def __init__(self, A, clip, value_loss_coef, entropy_coef, use_clipped_value_loss, device, noise="scalar", state_dependent=False):
        from wiki_grx_gym_amd.rl.modules import ActorCriticMLP
        from wiki_grx_gym_amd.rl.ppo import PPO
        ac = ActorCriticMLP(1, 1, A, actor_hidden_dims=[1], critic_hidden_dims=[1], noise_std_type=noise, state_dependent_std=state_dependent)
        self.alg = PPO(ac, clip_param=clip, value_loss_coef=value_loss_coef, entropy_coef=entropy_coef,
                       use_clipped_value_loss=use_clipped_value_loss, schedule="adaptive", desired_kl=0.01, device=device)
        self.alg._fused_loss = False
        ac.actor = ac.critic = torch.nn.Identity()
        self.ac, self.state_dependent = ac, state_dependent

    def __call__(self, mu, std, value, actions, old_logp, old_mu, old_sigma, advantages, returns, target_values):
        """dict: out = [surrogate, value_loss, total, mean KL] (fp32), d_mu (d_raw when state-dependent), d_std (None then), d_value"""
        assert not self.alg._loss_is_fused()
        mu, value = mu.detach().clone().requires_grad_(), value.detach().clone().requires_grad_()
        if not self.state_dependent:
            with torch.no_grad():
                self.ac.std.copy_(std)
            self.ac.std.grad = None
        s, v, loss, kl = self.alg._losses(mu, value, actions, target_values, advantages, returns, old_logp, old_mu, old_sigma)
        loss.backward()
        d_std = None if self.state_dependent else self.ac.std.grad.detach().clone()
        return {"out": torch.stack([s, v, loss, kl]).detach(), "d_mu": mu.grad, "d_std": d_std, "d_value": value.grad}


def same_non_finite(a, b):
    """two scalars: both finite, both NaN, or the same infinity"""
    a, b = float(a), float(b)
    if math.isfinite(a) or math.isfinite(b):
        return math.isfinite(a) and math.isfinite(b)
    return (math.isnan(a) and math.isnan(b)) or a == b


def check_extremes(got, want, tag):
    """A loss kernel's (out [4], d_mu, d_std or None, d_value) against TorchSpelling's dict where values stop being finite:
    1. out[2] is finite exactly when torch's loss is, and a non-finite one is the same NaN / infinity; the same for out[3], the mean KL;
    2. a finite torch loss over a torch gradient with a non-finite entry: the kernel's matching gradient has one too (the step tail's
       skip on a non-finite gradient norm then drops the step);
    3. the non-finite masks of d_mu and d_value are equal entry for entry, d_std's per action."""
    out, d_mu, d_std, d_value = got
    for i, name in ((2, "loss"), (3, "kl")):
        assert same_non_finite(out[i], want["out"][i]), (tag, name, float(out[i]), float(want["out"][i]))
    pairs = [("d_mu", d_mu, want["d_mu"]), ("d_value", d_value.reshape(-1), want["d_value"].reshape(-1))]
    if d_std is not None:
        pairs.append(("d_std", d_std, want["d_std"]))
    if math.isfinite(float(want["out"][2])):
        for name, g, w in pairs:
            assert bool(torch.isfinite(w).all()) or not bool(torch.isfinite(g).all()), (tag, name, "the kernel hides a non-finite gradient")
    for name, g, w in pairs:
        mg, mw = ~torch.isfinite(g), ~torch.isfinite(w)
        assert torch.equal(mg, mw), (tag, name, "non-finite entries: kernel", int(mg.sum()), "torch", int(mw.sum()), "differing", int((mg != mw).sum()))


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
    (params, exp_avg, exp_avg_sq, steps as float64) plus the total norm and the clip coefficient.

    The skip rule (include/grx_ppo.h): a non-finite loss, bad_flag != 0, or a gradient whose total norm is not finite in fp32 -- any
    non-finite element, or a float64 sum of squares above the largest float32 (callers keep that sum a factor of 10 away from the
    boundary, so the kernel's fp32 sum falls on the same side).  Where torch takes a zero-gradient Adam step (the overflow) this skips."""
    P, G, M, V = ([_d(t) for t in ts] for ts in (params, grads, exp_avg, exp_avg_sq))
    S = [float(s) for s in steps]
    bad = (not math.isfinite(float(loss))) or (bad_flag is not None and float(bad_flag) != 0.0)
    bad = bad or not all(bool(torch.isfinite(g).all()) for g in G)
    sumsq = sum(float((g * g).sum()) for g in G)
    bad = bad or not sumsq <= float(np.finfo(np.float32).max)
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
