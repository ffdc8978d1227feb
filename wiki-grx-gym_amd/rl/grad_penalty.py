"""The Lipschitz gradient penalty on the policy (Chen et al., "Learning Smooth Humanoid Locomotion through Lipschitz-Constrained Policies",
2024): grad_penalty_coef * P is added to the PPO loss, with

    logp_r = sum_j Normal(mu_rj, sigma_j).log_prob(a_rj)          mu = actor(x), x [B, D] the stored actor input, a [B, A] the stored actions
    P      = (1/B) sum_r || d logp_r / d x_r ||^2

P's gradient needs the second derivative of the actor, which the training path's autograd functions (rl/modules.py) do not have.  The pass
is written out here by hand, as ONE autograd function `(x, a, sigma, W_1, b_1, ..., W_L, b_L) -> (mu, P)` whose backward is one sweep up
and one ordinary backward down that the PPO gradient shares.  Layers l = 1..L, W_l [n_l, n_{l-1}], hidden outputs y_l = ELU(.), and from
the saved output  e1(y) = y > 0 ? 1 : y + 1 (ELU'),  e2(y) = y < 0 ? y + 1 : 0 (ELU''; 0 at y == 0, the side
torch's double backward takes):

    forward    y_l as the training path computes them; mu
    seed       u = (a - mu) / sigma^2                                                          [B, A]
    reverse    h_L = u;  g_{l-1} = h_l W_l;  h_{l-1} = g_{l-1} * e1(y_{l-1})                   down to g_0 [B, D];  P = (1/B) sum g_0^2
    second     gbar_0 = c (2/B) g_0                                                            (c: the gradient arriving at P, on the device)
               l = 1..L:  hbar_l = gbar_{l-1} W_l^T;  dW_l += h_l^T gbar_{l-1};  l < L:  gbar_l = hbar_l * e1(y_l),  zbar_l = hbar_l * g_l * e2(y_l)
               ubar = hbar_L;  mubar = -ubar / sigma^2;  dsigma_j = sum_r ubar_rj (-2 (a_rj - mu_rj) / sigma_j^3)
    backward   dz_L = (the gradient arriving at mu) + mubar;   dz_l = (dz_{l+1} W_{l+1}) * e1(y_l) + zbar_l;   dW_l += dz_l^T y_{l-1};  db_l = colsum(dz_l)

The element-wise steps -- seed, gate, the squared norm, the gate's backward with the bias gradient, the seed's backward with dsigma -- are
entry points of libgrx_ppo.so (include/grx_ppo_gp.h, which states every element's expression); the `*_torch` functions below are the same
formulas in plain torch: what CPU tensors use, and what GRX_GP_FUSED=0 selects on a HIP device.  The matrix products are the training
path's: X W^T through grx_mlp_layer where the training path's forward goes through it, everything else through torch matmul under the
update's BLAS preference."""
import ctypes as C
import math
import os

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable


def fused_enabled():
    return os.environ.get("GRX_GP_FUSED", "1") != "0"


def check_coef(coef, who="PPO"):
    if isinstance(coef, bool) or not (isinstance(coef, (int, float)) and math.isfinite(coef) and coef > 0):
        raise ValueError(f"{who}: --grad_penalty_coef {coef!r}: it must be a finite number above 0")
    return float(coef)


def linears_of(actor, who="PPO"):
    """[(W_l, b_l)] of an actor the pass covers: an rl.modules.MLP of Linear -> ELU(1) -> ... -> Linear with biases; ValueError otherwise"""
    from .fused_loss import _linears_of
    lin = _linears_of(actor) if hasattr(actor, "model") else None
    if lin is None or any(b is None for _, b in lin):
        raise ValueError(f"{who}: --grad_penalty_coef needs an actor of Linear -> ELU(alpha=1) -> ... -> Linear (with biases): the second-order "
                         "pass is written for that form only")
    return lin


# ---- the element-wise steps in torch (the definitions) ----------------------------------------------------------------------------------
def e1(y):
    return torch.where(y > 0, torch.ones_like(y), y + 1.0)


def e2(y):
    return torch.where(y < 0, y + 1.0, torch.zeros_like(y))


def _colsum(x):
    if x.is_cuda and x.dtype == torch.float32:   # (torch's column reduction is what a captured step avoids: rl/modules.py _TrainLinear)
        from .fused_loss import colsum
        return colsum(x)
    return x.sum(0)


def seed_torch(a, mu, sigma):
    return (a - mu) / (sigma * sigma)


def gate_torch(g, y):
    return g * e1(y)


def sqnorm_torch(g0):
    return (g0.double().square().sum() / g0.shape[0]).to(g0.dtype)


def gate_backward_torch(hbar, g, y, dY):
    """(dz, db)"""
    dz = dY * e1(y) + (hbar * g) * e2(y)
    return dz, _colsum(dz)


def seed_backward_torch(ubar, a, mu, sigma, dmu):
    """(dmu + mubar, dsigma)"""
    s2 = sigma * sigma
    return dmu - ubar / s2, _colsum(ubar * ((-2.0 * (a - mu)) / (s2 * sigma)))


# ---- the same through libgrx_ppo.so -------------------------------------------------------------------------------------------------------
def _lib():
    from .fused_loss import load_ppo_library
    return load_ppo_library()


def _stream(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _c(x):
    return x if (x.dtype == torch.float32 and x.is_contiguous()) else x.contiguous().float()


def _check(rc, name, shape):
    if rc != 0:
        raise RuntimeError(f"{name} failed ({rc}): {tuple(shape)}")


def seed_fused(a, mu, sigma):
    a, mu, sigma = _c(a), _c(mu), _c(sigma)
    u = torch.empty_like(mu)
    with torch.cuda.device(mu.device):
        _check(_lib().grx_gp_seed(mu.shape[0], mu.shape[1], a.data_ptr(), mu.data_ptr(), sigma.data_ptr(), u.data_ptr(), _stream(mu)),
               "grx_gp_seed", mu.shape)
    return u


def gate_fused(g, y):
    g, y = _c(g), _c(y)
    h = torch.empty_like(g)
    with torch.cuda.device(g.device):
        _check(_lib().grx_gp_gate(g.shape[0], g.shape[1], g.data_ptr(), y.data_ptr(), h.data_ptr(), _stream(g)), "grx_gp_gate", g.shape)
    return h


def sqnorm_fused(g0):
    g0 = _c(g0)
    lib = _lib()
    P = torch.empty((), device=g0.device, dtype=torch.float32)
    partials = torch.empty(lib.grx_gp_sqnorm_partials_size(g0.shape[0], g0.shape[1]), device=g0.device, dtype=torch.float32)
    with torch.cuda.device(g0.device):
        _check(lib.grx_gp_sqnorm(g0.shape[0], g0.shape[1], g0.data_ptr(), P.data_ptr(), partials.data_ptr(), _stream(g0)), "grx_gp_sqnorm", g0.shape)
    return P


def gate_backward_fused(hbar, g, y, dY, want_gbar=False):
    """(dz, db), or (gbar, dz, db) with want_gbar"""
    hbar, g, y, dY = _c(hbar), _c(g), _c(y), _c(dY)
    lib = _lib()
    B, n = g.shape
    dz = torch.empty_like(g)
    gbar = torch.empty_like(g) if want_gbar else None
    db = torch.empty(n, device=g.device, dtype=torch.float32)
    partials = torch.empty(lib.grx_ppo_colsum_partials_size(B, n), device=g.device, dtype=torch.float32)
    with torch.cuda.device(g.device):
        _check(lib.grx_gp_gate_backward(B, n, hbar.data_ptr(), g.data_ptr(), y.data_ptr(), dY.data_ptr(), gbar.data_ptr() if want_gbar else None,
                                        dz.data_ptr(), db.data_ptr(), partials.data_ptr(), _stream(g)), "grx_gp_gate_backward", g.shape)
    return (gbar, dz, db) if want_gbar else (dz, db)


def seed_backward_fused(ubar, a, mu, sigma, dmu):
    ubar, a, mu, sigma, dmu = _c(ubar), _c(a), _c(mu), _c(sigma), _c(dmu)
    lib = _lib()
    B, A = mu.shape
    out = torch.empty_like(mu)
    dsigma = torch.empty(A, device=mu.device, dtype=torch.float32)
    partials = torch.empty(lib.grx_ppo_colsum_partials_size(B, A), device=mu.device, dtype=torch.float32)
    with torch.cuda.device(mu.device):
        _check(lib.grx_gp_seed_backward(B, A, ubar.data_ptr(), a.data_ptr(), mu.data_ptr(), sigma.data_ptr(), dmu.data_ptr(), out.data_ptr(),
                                        dsigma.data_ptr(), partials.data_ptr(), _stream(mu)), "grx_gp_seed_backward", mu.shape)
    return out, dsigma


def _ops(x):
    """(seed, gate, sqnorm, gate_backward, seed_backward) for x's device"""
    if x.is_cuda and x.dtype == torch.float32 and fused_enabled():
        return seed_fused, gate_fused, sqnorm_fused, gate_backward_fused, seed_backward_fused
    return seed_torch, gate_torch, sqnorm_torch, gate_backward_torch, seed_backward_torch


# ---- the matrix products: the training path's (rl/modules.py) ------------------------------------------------------------------------------
def _train_path(x):
    """True where MLP.forward takes _forward_train: _TrainLinear's products and pins, grx_mlp_layer for a hidden layer's forward"""
    from . import modules as M
    return x.is_cuda and x.dtype == torch.float32 and M._TRAIN_LINEAR == "colsum"


def _through_mlp_layer(x, w):
    from . import modules as M
    return _train_path(x) and M._FUSED_ELU_BACKWARD and M._FUSED_ELU_FORWARD and x.is_contiguous() and w.is_contiguous()


class _pinned:
    """_TrainLinear's BLAS pin around the products of a one-row weight (the value head's shape; an actor with one action has it too)"""

    def __init__(self, x, w):
        self.pin = _train_path(x) and w.shape[0] == 1

    def __enter__(self):
        if self.pin:
            self.prev = torch.backends.cuda.preferred_blas_library()
            torch.backends.cuda.preferred_blas_library("cublaslt")

    def __exit__(self, *exc):
        if self.pin:
            torch.backends.cuda.preferred_blas_library(self.prev)


def _hidden_forward(x, w, b):
    if _through_mlp_layer(x, w):
        from .fused_loss import linear_elu
        return linear_elu(x, w, b)
    if _train_path(x):
        with _pinned(x, w):
            return F.elu(torch.addmm(b, x, w.t()))
    return F.elu(F.linear(x, w, b))


def _output_forward(x, w, b):
    if _train_path(x):
        with _pinned(x, w):
            return torch.addmm(b, x, w.t())
    return F.linear(x, w, b)


def _x_wt(x, w):
    """x W^T without a bias: grx_mlp_layer where the training path's hidden forward goes through it"""
    if _through_mlp_layer(x, w):
        from .fused_loss import _layer
        with torch.cuda.device(x.device):
            return _layer(_lib(), x, w, None, False, torch.cuda.current_stream(x.device).cuda_stream)
    with _pinned(x, w):
        return x @ w.t()


class GradPenalty(torch.autograd.Function):
    """(x [B, D], a [B, A], sigma [A], W_1, b_1, ..., W_L, b_L) -> (mu [B, A], P []).  mu is what the actor returns on the training path,
    bit for bit.  backward takes the gradients arriving at mu and at P and returns those of x (when asked for), sigma and every W_l, b_l; the
    actions are data."""

    @staticmethod
    def forward(ctx, x, a, sigma, *params):
        seed, gate, sqnorm, _, _ = _ops(x)
        W, b = params[0::2], params[1::2]
        L = len(W)
        ys = [x]
        for l in range(L - 1):
            ys.append(_hidden_forward(ys[-1], W[l], b[l]))
        mu = _output_forward(ys[-1], W[-1], b[-1])
        hs, gs = [None] * (L + 1), [None] * L          # h_l (l = 1..L), g_l (l = 0..L-1)
        hs[L] = seed(a, mu, sigma)
        for l in range(L, 0, -1):
            with _pinned(x, W[l - 1]):
                gs[l - 1] = hs[l] @ W[l - 1]
            if l > 1:
                hs[l - 1] = gate(gs[l - 1], ys[l - 1])
        P = sqnorm(gs[0])
        ctx.L = L
        ctx.save_for_backward(a, sigma, mu, *W, *ys, *hs[1:], *gs)
        return mu, P

    @staticmethod
    @once_differentiable
    def backward(ctx, dmu, c):
        L = ctx.L
        t = ctx.saved_tensors
        a, sigma, mu = t[:3]
        W, ys, hs, gs = t[3:3 + L], t[3 + L:3 + 2 * L], (None,) + tuple(t[3 + 2 * L:3 + 3 * L]), t[3 + 3 * L:3 + 4 * L]
        x = ys[0]
        _, gate, _, gate_backward, seed_backward = _ops(x)
        B = x.shape[0]
        if dmu is None:
            dmu = torch.zeros_like(mu)
        if c is None:
            c = torch.zeros((), device=x.device, dtype=x.dtype)
        # the sweep up: the penalty's gradient with respect to every h_l, and its direct share of the weight gradients
        gbar = gs[0] * (c * (2.0 / B))
        dW, hbars = [None] * L, [None] * (L + 1)
        for l in range(1, L + 1):
            hbars[l] = _x_wt(gbar, W[l - 1])
            with _pinned(x, W[l - 1]):
                dW[l - 1] = hs[l].t() @ gbar
            if l < L:
                gbar = gate(hbars[l], ys[l])
        # the one backward down, shared with the rest of the loss
        dz, dsigma = seed_backward(hbars[L], a, mu, sigma, dmu)
        db = [None] * L
        db[L - 1] = _colsum(dz)
        dx = None
        for l in range(L, 0, -1):
            with _pinned(x, W[l - 1]):
                dW[l - 1] = torch.addmm(dW[l - 1], dz.t(), ys[l - 1])
                if l > 1 or ctx.needs_input_grad[0]:
                    dY = dz @ W[l - 1]
            if l > 1:
                dz, db[l - 2] = gate_backward(hbars[l - 1], gs[l - 1], ys[l - 1], dY)
            elif ctx.needs_input_grad[0]:
                dx = dY
        grads = [g for pair in zip(dW, db) for g in pair]
        return (dx, None, dsigma, *grads)


def grad_penalty(actor, x, actions, sigma):
    """(mu, P) of an rl.modules.MLP actor on one minibatch"""
    lin = linears_of(actor)
    return GradPenalty.apply(x, actions, sigma, *[p for wb in lin for p in wb])
