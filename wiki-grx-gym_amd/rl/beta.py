"""A Beta action distribution for PPO (Chou, Maturana & Scherer, ICML 2017): the policy's support is the env's action box.

The actor's output layer is 2A wide, raw = [p | q]; alpha = 1 + softplus(p), beta = 1 + softplus(q), both >= 1 (a unimodal density).  The
action in unit-box coordinates is x ~ Beta(alpha, beta) per joint, clamped to [2^-24, 1 - 2^-24]; the env receives a = lo + span * x.  The
rollout storage holds x (not a: x recovered from a rounded a is off by per cents close to a bound), and alpha / beta in the rows a Gaussian
policy keeps mu / sigma in.  Log-probabilities and entropies are those of x: the constant sum_k log span_k of the density in action units
cancels in PPO's ratio and is left out everywhere.

This file holds the torch spellings (the definition, the CPU path, and -- GRX_BETA_FUSED=0 -- an uncaptured path on a HIP device), the ctypes
bindings of include/grx_ppo_beta.h, the initialisation of the output layer's biases, the mean head for inference and export, and the
resolution of the action bounds.  Nothing here is imported unless `action_dist="beta"` is set."""
import ctypes as C
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ACTION_DISTS = ("gaussian", "beta")
X_MIN = 2.0 ** -24
X_MAX = 1.0 - 2.0 ** -24


def fused_enabled():
    """GRX_BETA_FUSED=0: the torch spelling on a HIP device too (not captured)"""
    return os.environ.get("GRX_BETA_FUSED", "1") != "0"


# ------------------------------------------------------------------ the torch spellings (any float dtype)
def params_torch(raw):
    """(alpha, beta) [..., A] of the actor's raw output [..., 2A]"""
    A = raw.shape[-1] // 2
    return 1.0 + F.softplus(raw[..., :A]), 1.0 + F.softplus(raw[..., A:])


def lnbeta_torch(a, b):
    return torch.lgamma(a) + torch.lgamma(b) - torch.lgamma(a + b)


def logp_torch(alpha, beta, x):
    """log p(x) per row, in unit-box coordinates"""
    return ((alpha - 1.0) * torch.log(x) + (beta - 1.0) * torch.log(1.0 - x) - lnbeta_torch(alpha, beta)).sum(-1)


def entropy_torch(alpha, beta):
    s = alpha + beta
    return (lnbeta_torch(alpha, beta) - (alpha - 1.0) * torch.digamma(alpha) - (beta - 1.0) * torch.digamma(beta)
            + (s - 2.0) * torch.digamma(s)).sum(-1)


def kl_torch(alpha0, beta0, alpha, beta):
    """KL(Beta(alpha0, beta0) || Beta(alpha, beta)) per row"""
    return (lnbeta_torch(alpha, beta) - lnbeta_torch(alpha0, beta0) + (alpha0 - alpha) * torch.digamma(alpha0)
            + (beta0 - beta) * torch.digamma(beta0) + ((alpha - alpha0) + (beta - beta0)) * torch.digamma(alpha0 + beta0)).sum(-1)


def mean_torch(alpha, beta, lo, span):
    return lo + span * (alpha / (alpha + beta))


def std_torch(alpha, beta, span):
    s = alpha + beta
    return span * torch.sqrt(alpha * beta / (s * s * (s + 1.0)))


def sample_torch(alpha, beta, lo, span):
    """(x, a, logp): two gamma draws, the clamped quotient, the env's action and log p(x)"""
    g1, g2 = torch._standard_gamma(alpha), torch._standard_gamma(beta)
    x = (g1 / (g1 + g2)).clamp(X_MIN, X_MAX)
    return x, torch.addcmul(lo, span, x), logp_torch(alpha, beta, x)


def loss_torch(raw, value, x, old_logp, old_alpha, old_beta, advantages, returns, target_values, clip_param, value_loss_coef,
               entropy_coef, use_clipped_value_loss, with_kl=True):
    """(surrogate_loss, value_loss, loss, kl_mean) of one minibatch: rl/ppo.py's _loss_terms with the Beta's log-probability, entropy and
    KL.  value / returns / target_values / advantages / old_logp: [B] or [B, 1]"""
    alpha, beta = params_torch(raw)
    logp, entropy = logp_torch(alpha, beta, x), entropy_torch(alpha, beta)
    kl_mean = torch.zeros((), device=raw.device, dtype=raw.dtype)
    if with_kl:
        with torch.no_grad():
            kl_mean = kl_torch(old_alpha, old_beta, alpha, beta).mean()
    value, returns = value.reshape(-1), returns.reshape(-1)
    ratio = torch.exp(logp - old_logp.reshape(-1))
    adv = advantages.reshape(-1)
    surrogate_loss = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1.0 - clip_param, 1.0 + clip_param)).mean()
    if use_clipped_value_loss:
        tv = target_values.reshape(-1)
        clipped = tv + (value - tv).clamp(-clip_param, clip_param)
        value_loss = torch.max((value - returns).pow(2), (clipped - returns).pow(2)).mean()
    else:
        value_loss = (returns - value).pow(2).mean()
    loss = surrogate_loss + value_loss_coef * value_loss - entropy_coef * entropy.mean()
    return surrogate_loss, value_loss, loss, kl_mean


# ------------------------------------------------------------------ the initialisation
def init_params(lo, span, init_noise_std):
    """(alpha0, beta0) [A] in float64: per joint the mode at the zero action (clamped into [0.05, 0.95] of the box) and a spread of
    init_noise_std in action units.  With alpha = 1 + kappa m, beta = 1 + kappa (1 - m) the mode is m for every kappa > 0, and
    kappa = m (1 - m) span^2 / sigma^2 - 3, floored at 0, gives the spread to a few per cent while kappa is large (the lower-limb box:
    0.200..0.206 for 0.2).  On a box that is narrow against sigma the closed form drops below 0 although a unimodal Beta with that spread
    exists (the full-body box's hip rolls: span 0.90, sigma 0.2), so kappa is the root of the exact variance
    alpha beta / ((alpha + beta)^2 (alpha + beta + 1)) = (sigma / span)^2, bracketed from the closed form and bisected; where even the
    uniform density (kappa = 0, the widest there is) is narrower than sigma, kappa is 0"""
    lo, span = np.asarray(lo, dtype=np.float64), np.asarray(span, dtype=np.float64)
    sigma = np.broadcast_to(np.asarray(init_noise_std, dtype=np.float64), lo.shape)
    m = np.clip((0.0 - lo) / span, 0.05, 0.95)
    target = (sigma / span) ** 2

    def excess(kappa):   # the variance in unit-box coordinates minus the target: falls as kappa grows
        a, b = 1.0 + kappa * m, 1.0 + kappa * (1.0 - m)
        return a * b / ((a + b) ** 2 * (a + b + 1.0)) - target
    k_lo = np.zeros_like(m)
    k_hi = np.maximum(m * (1.0 - m) / target - 3.0, 0.0) + 4.0
    for _ in range(64):   # (the closed form is within a few per cent: a doubling or two at most)
        k_hi = np.where(excess(k_hi) > 0.0, 2.0 * k_hi, k_hi)
    for _ in range(100):
        mid = 0.5 * (k_lo + k_hi)
        above = excess(mid) > 0.0
        k_lo, k_hi = np.where(above, mid, k_lo), np.where(above, k_hi, mid)
    kappa = np.where(excess(np.zeros_like(m)) <= 0.0, 0.0, 0.5 * (k_lo + k_hi))
    return 1.0 + kappa * m, 1.0 + kappa * (1.0 - m)


def softplus_inverse(y, floor=1e-30):
    """p with softplus(p) = y; a zero argument is floored at a tiny positive number"""
    y = np.maximum(np.asarray(y, dtype=np.float64), floor)
    return np.where(y > 30.0, y, np.log(np.expm1(np.minimum(y, 30.0))))


def init_biases(lo, span, init_noise_std):
    """the output layer's 2A biases [p | q] of the initial policy, float32"""
    a0, b0 = init_params(lo, span, init_noise_std)
    return torch.as_tensor(np.concatenate([softplus_inverse(a0 - 1.0), softplus_inverse(b0 - 1.0)]), dtype=torch.float32)


# ------------------------------------------------------------------ the bounds
def _bounds(lo, hi, num_actions, what):
    lo = np.broadcast_to(np.asarray(lo, dtype=np.float64).reshape(-1), (num_actions,)) if np.size(lo) in (1, num_actions) else None
    hi = np.broadcast_to(np.asarray(hi, dtype=np.float64).reshape(-1), (num_actions,)) if np.size(hi) in (1, num_actions) else None
    if lo is None or hi is None:
        raise ValueError(f"--action_dist beta: {what} must hold one value or one per action ({num_actions})")
    span = hi - lo
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(span)) and np.all(span > 0.0)):
        raise ValueError(f"--action_dist beta: {what} give a span that is not positive and finite (lo {lo.tolist()}, hi {hi.tolist()})")
    return [float(v) for v in lo], [float(v) for v in hi]


def resolve_bounds(normalization, num_actions, action_bounds=None):
    """(lo, hi) as lists of num_actions floats: the env's per-joint clip (cfg.normalization.clip_actions_min / clip_actions_max) where it has
    one -- the step kernel clips there, and the policy's support is that box --, else `action_bounds` = (LO, HI) (--action_bounds).  A
    config with only the scalar clip_actions is refused without them: +-100 is no support to spread a density over"""
    get = (lambda k: normalization.get(k)) if isinstance(normalization, dict) else (lambda k: getattr(normalization, k, None))
    cmin, cmax = get("clip_actions_min"), get("clip_actions_max")
    if cmin is not None and cmax is not None:
        if action_bounds is not None:
            print("--action_bounds is ignored: the env clips its actions per joint (normalization.clip_actions_min / clip_actions_max), "
                  "the Beta policy's support is that box")
        return _bounds(cmin, cmax, num_actions, "normalization.clip_actions_min / clip_actions_max")
    if action_bounds is None:
        raise ValueError("--action_dist beta needs per-joint action bounds: this env's config has only the scalar normalization.clip_actions "
                         f"({get('clip_actions')!r}); pass --action_bounds LO HI (train_cfg.policy.action_bounds)")
    if len(action_bounds) != 2:
        raise ValueError(f"--action_bounds takes two values LO HI, not {action_bounds!r}")
    return _bounds(action_bounds[0], action_bounds[1], num_actions, "--action_bounds")


# ------------------------------------------------------------------ inference and export
class BetaMeanHead(nn.Module):
    """the mean action lo + span * alpha / (alpha + beta), [B, A], of an actor whose output layer is [p | q]: what inference, play and the
    exported TorchScript module act on.  Plain torch; lo / span are buffers and travel with the module"""

    def __init__(self, actor, num_actions: int, lo, span):
        super().__init__()
        self.actor, self.num_actions = actor, int(num_actions)
        self.register_buffer("lo", lo.detach().clone())
        self.register_buffer("span", span.detach().clone())

    def forward(self, x):
        raw = self.actor(x)
        a = 1.0 + F.softplus(torch.narrow(raw, -1, 0, self.num_actions))
        b = 1.0 + F.softplus(torch.narrow(raw, -1, self.num_actions, self.num_actions))
        return self.lo + self.span * (a / (a + b))


# ------------------------------------------------------------------ libgrx_ppo.so (include/grx_ppo_beta.h)
_BOUND = False


def _lib():
    """libgrx_ppo.so with the Beta entry points' signatures set (once): a missing symbol is an error, there is no fallback"""
    global _BOUND
    from .fused_loss import load_ppo_library
    lib = load_ppo_library()
    if not _BOUND:
        fp = C.c_void_p
        lib.grx_ppo_loss_beta_partials_size.restype = C.c_int
        lib.grx_ppo_loss_beta_partials_size.argtypes = [C.c_int]
        lib.grx_ppo_loss_beta.restype = C.c_int
        lib.grx_ppo_loss_beta.argtypes = [C.c_int, C.c_int] + [fp] * 9 + [C.c_float, C.c_float, C.c_float, C.c_int] + [fp] * 4 + [C.c_void_p]
        lib.grx_beta_params.restype = C.c_int
        lib.grx_beta_params.argtypes = [C.c_int, C.c_int, fp, fp, fp, C.c_void_p]
        lib.grx_beta_sample.restype = C.c_int
        lib.grx_beta_sample.argtypes = [C.c_int, C.c_int] + [fp] * 9 + [C.c_void_p]
        lib.grx_beta_functions.restype = C.c_int
        lib.grx_beta_functions.argtypes = [C.c_int] + [fp] * 4 + [C.c_void_p]
        _BOUND = True
    return lib


def _f32c(x):
    return x if (x.dtype == torch.float32 and x.is_contiguous()) else x.contiguous().float()


def _stream(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


class FusedPPOLossBeta(torch.autograd.Function):
    """FusedPPOLossSD for a Beta policy (grx_ppo_loss_beta): (raw [B, 2A] = [p | q], value [B] or [B, 1]; data...) -> tensor
    [surrogate, value_loss, total_loss, mean_kl].  The kernel writes the gradient onto the actor's raw output."""

    @staticmethod
    def forward(ctx, raw, value, x, old_logp, old_alpha, old_beta, advantages, returns, target_values,
                clip_param, value_loss_coef, entropy_coef, use_clipped_value_loss):
        lib = _lib()
        B, A = x.shape
        if tuple(raw.shape) != (B, 2 * A):
            raise RuntimeError(f"fused_ppo_loss_beta: raw is {tuple(raw.shape)}, expected {(B, 2 * A)} ([p | q] of {A} actions)")
        raw_c, value_c = _f32c(raw), _f32c(value).reshape(-1)
        data = [_f32c(t) for t in (x, old_logp, old_alpha, old_beta, advantages, returns, target_values)]
        out = torch.empty(4, device=raw.device, dtype=torch.float32)
        d_raw = torch.empty_like(raw_c)
        d_value = torch.empty_like(value_c)
        partials = torch.empty(lib.grx_ppo_loss_beta_partials_size(B), device=raw.device, dtype=torch.float32)
        with torch.cuda.device(raw.device):
            rc = lib.grx_ppo_loss_beta(B, A, raw_c.data_ptr(), value_c.data_ptr(), *[t.data_ptr() for t in data],
                                       float(clip_param), float(value_loss_coef), float(entropy_coef), int(bool(use_clipped_value_loss)),
                                       out.data_ptr(), d_raw.data_ptr(), d_value.data_ptr(), partials.data_ptr(), _stream(raw))
        if rc != 0:
            raise RuntimeError(f"grx_ppo_loss_beta failed ({rc}): batch {B}, num_actions {A}")
        ctx.save_for_backward(d_raw, d_value)
        ctx.value_shape = value.shape
        return out

    @staticmethod
    def backward(ctx, g):
        d_raw, d_value = ctx.saved_tensors
        gl = g[2]   # only the total loss is differentiable
        return (d_raw * gl, (d_value * gl).reshape(ctx.value_shape)) + (None,) * 11


def fused_ppo_loss_beta(raw, value, x, old_logp, old_alpha, old_beta, advantages, returns, target_values,
                        clip_param, value_loss_coef, entropy_coef, use_clipped_value_loss):
    return FusedPPOLossBeta.apply(raw, value, x, old_logp, old_alpha, old_beta, advantages, returns, target_values,
                                  clip_param, value_loss_coef, entropy_coef, use_clipped_value_loss)


def beta_params(raw):
    """(alpha, beta) [M, A] of raw [M, 2A] through grx_beta_params"""
    lib = _lib()
    raw = _f32c(raw)
    M, A = raw.shape[0], raw.shape[1] // 2
    alpha = torch.empty(M, A, device=raw.device, dtype=torch.float32)
    beta = torch.empty_like(alpha)
    with torch.cuda.device(raw.device):
        rc = lib.grx_beta_params(M, A, raw.data_ptr(), alpha.data_ptr(), beta.data_ptr(), _stream(raw))
    if rc != 0:
        raise RuntimeError(f"grx_beta_params failed ({rc}): rows {M}, num_actions {A}")
    return alpha, beta


def beta_sample(alpha, beta, g1, g2, lo, span):
    """(x, actions, logp) through grx_beta_sample: the clamped quotient of the two gamma draws, lo + span * x, log p(x)"""
    lib = _lib()
    alpha, beta, g1, g2, lo, span = (_f32c(t) for t in (alpha, beta, g1, g2, lo, span))
    M, A = alpha.shape
    x = torch.empty_like(alpha)
    actions = torch.empty_like(alpha)
    logp = torch.empty(M, device=alpha.device, dtype=torch.float32)
    with torch.cuda.device(alpha.device):
        rc = lib.grx_beta_sample(M, A, alpha.data_ptr(), beta.data_ptr(), g1.data_ptr(), g2.data_ptr(), lo.data_ptr(), span.data_ptr(),
                                 x.data_ptr(), actions.data_ptr(), logp.data_ptr(), _stream(alpha))
    if rc != 0:
        raise RuntimeError(f"grx_beta_sample failed ({rc}): rows {M}, num_actions {A}")
    return x, actions, logp


def beta_functions(t):
    """(lgamma, digamma, trigamma) of t [n] (>= 1) as the kernels evaluate them, fp32 -- the test hook"""
    lib = _lib()
    t = _f32c(t).reshape(-1)
    outs = [torch.empty_like(t) for _ in range(3)]
    with torch.cuda.device(t.device):
        rc = lib.grx_beta_functions(t.numel(), t.data_ptr(), *[o.data_ptr() for o in outs], _stream(t))
    if rc != 0:
        raise RuntimeError(f"grx_beta_functions failed ({rc}): n {t.numel()}")
    return tuple(outs)


def rollout_sample(alpha, beta, lo, span):
    """the rollout's sample from (alpha, beta) [M, A]: two torch._standard_gamma draws, then grx_beta_sample on a HIP device (the torch
    spelling on the CPU and under GRX_BETA_FUSED=0).  -> (x, actions, logp)"""
    if alpha.is_cuda and fused_enabled():
        return beta_sample(alpha, beta, torch._standard_gamma(alpha), torch._standard_gamma(beta), lo, span)
    return sample_torch(alpha, beta, lo, span)
