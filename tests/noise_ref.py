"""Float64 restatements for the action-noise options (rl/modules.py `noise_std_type`, `state_dependent_std`), used by
tests/test_noise_std.py and tests/test_noise_std_gpu.py.

The loss is rsl_rl's spelling (rsl_rl/algorithms/ppo.py, ActorCritic with `noise_std_type` / `state_dependent_std`) with
torch.distributions.Normal on a sigma per row, in float64 autograd: no kernel code and none of the module's own accessors are imitated.
A policy's sigma is rebuilt here from its tensors -- `std`, exp(`log_std`), or the second half of the actor's plain nn.Sequential output."""
import math

import torch

LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)
U32 = 2.0 ** -24   # unit roundoff of fp32


def _d(t):
    return t.detach().double()


def split(raw, log_std):
    """(mean, sigma) of a raw actor output [..., 2A] = [mean | s]: sigma = s, or exp(s)"""
    A = raw.shape[-1] // 2
    s = raw[..., A:]
    return raw[..., :A], (torch.exp(s) if log_std else s)


def loss_terms(mean, sigma, value, actions, old_logp, old_mu, old_sigma, advantages, returns, target_values,
               clip, value_loss_coef, entropy_coef, use_clipped_value_loss):
    """(surrogate, value loss, total loss, mean KL) and the per-row pieces, from float64 tensors that may carry a graph; sigma [B, A]"""
    dist = torch.distributions.Normal(mean, sigma, validate_args=False)
    logp = dist.log_prob(actions).sum(-1)
    entropy = dist.entropy().sum(-1)
    v = value.reshape(-1)
    old_logp, adv, ret, tv = (t.reshape(-1) for t in (old_logp, advantages, returns, target_values))
    with torch.no_grad():
        kl_rows = (torch.log(sigma / old_sigma + 1.e-5) + (old_sigma ** 2 + (old_mu - mean) ** 2) / (2.0 * sigma ** 2) - 0.5).sum(-1)
    ratio = torch.exp(logp - old_logp)
    surr_rows = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1.0 - clip, 1.0 + clip))
    if use_clipped_value_loss:
        clipped = tv + (v - tv).clamp(-clip, clip)
        vl_rows = torch.max((v - ret) ** 2, (clipped - ret) ** 2)
    else:
        vl_rows = (ret - v) ** 2
    surrogate, value_loss = surr_rows.mean(), vl_rows.mean()
    loss = surrogate + value_loss_coef * value_loss - entropy_coef * entropy.mean()
    return {"surrogate": surrogate, "value_loss": value_loss, "loss": loss, "kl": kl_rows.mean(),
            "surr_rows": surr_rows, "vl_rows": vl_rows, "kl_rows": kl_rows, "entropy_rows": entropy, "ratio": ratio}


def loss_sd_ref(raw, log_std, value, actions, old_logp, old_mu, old_sigma, advantages, returns, target_values,
                clip, value_loss_coef, entropy_coef, use_clipped_value_loss):
    """grx_ppo_loss_sd in float64 autograd.  raw [B, 2A]; value, old_logp, advantages, returns, target_values [B] or [B, 1]; actions,
    old_mu, old_sigma [B, A].  Returns out = [surrogate, value loss, total, mean KL], d_raw, d_value (gradients of the total loss), the
    rows' sigma, and `scale`: each of the four scalars with every term replaced by its magnitude (tests/ppo_ref.py ppo_loss_ref)."""
    raw, value = _d(raw).requires_grad_(), _d(value).requires_grad_()
    mean, sigma = split(raw, log_std)
    t = loss_terms(mean, sigma, value, _d(actions), _d(old_logp), _d(old_mu), _d(old_sigma), _d(advantages), _d(returns), _d(target_values),
                   clip, value_loss_coef, entropy_coef, use_clipped_value_loss)
    d_raw, d_value = torch.autograd.grad(t["loss"], (raw, value))
    with torch.no_grad():
        s_abs = (t["surr_rows"].abs().mean(), t["vl_rows"].abs().mean(), t["kl_rows"].abs().mean())
        total_abs = s_abs[0] + abs(value_loss_coef) * s_abs[1] + abs(entropy_coef) * t["entropy_rows"].abs().mean()
        scale = torch.stack([s_abs[0], s_abs[1], total_abs, s_abs[2]])
    out = torch.stack([t["surrogate"].detach(), t["value_loss"].detach(), t["loss"].detach(), t["kl"]])
    return {"out": out, "d_raw": d_raw, "d_value": d_value.reshape(value.shape), "sigma": sigma.detach(), "scale": scale}


def policy_sigma(ac64, obs64):
    """(mean, sigma [B, A]) of a float64 copy of an ActorCriticMLP on obs64, from its tensors: the actor's plain nn.Sequential, then
    `std`, exp(`log_std`) or the second output half"""
    out = ac64.actor.model(obs64)
    if ac64.state_dependent_std:
        return split(out, ac64.noise_std_type == "log")
    sigma = torch.exp(ac64.log_std) if ac64.noise_std_type == "log" else ac64.std
    return out, out * 0.0 + sigma


def policy_head_sd_ref(X, W, bias, log_std):
    """(mu, s, sigma) of grx_mlp_policy_head_sd in float64: [mu | s] = X W^T + b, sigma = s or exp(s)"""
    raw = _d(X) @ _d(W).t() + (_d(bias) if bias is not None else 0.0)
    mu, sigma = split(raw, log_std)
    return mu, raw[..., raw.shape[-1] // 2:], sigma
