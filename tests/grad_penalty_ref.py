"""Float64 restatements for rl/grad_penalty.py (the Lipschitz gradient penalty), written from the definition and used by
tests/test_grad_penalty.py and tests/test_grad_penalty_gpu.py: plain nn.functional.linear / elu and torch's own double backward.

    mu     = actor(x)                                   Linear -> ELU -> ... -> Linear
    logp_r = sum_j Normal(mu_rj, sigma_j).log_prob(a_rj)
    P      = (1/B) sum_r || d logp_r / d x_r ||^2        (torch.autograd.grad(logp.sum(), x, create_graph=True): rows do not mix)

The minibatch loss with parameter gradients is restated on top of tests/ppo_ref.py, as tests/smooth_ref.py's is."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import ppo_ref


def _d(t):
    return torch.as_tensor(np.asarray(t.detach().cpu().double().numpy() if torch.is_tensor(t) else t, np.float64))


def actor64(x, weights, biases):
    for i, (w, b) in enumerate(zip(weights, biases)):
        x = F.linear(x, w, b)
        if i + 1 < len(weights):
            x = F.elu(x)
    return x


def penalty(x, a, sigma, weights, biases):
    """(mu, P) in float64 autograd from float64 tensors; x must require grad; P carries the graph of the double backward"""
    mu = actor64(x, weights, biases)
    logp = torch.distributions.Normal(mu, mu * 0.0 + sigma, validate_args=False).log_prob(a).sum(-1)
    g, = torch.autograd.grad(logp.sum(), x, create_graph=True)
    return mu, g.square().sum() / x.shape[0]


def penalty_and_grads(x, a, sigma, weights, biases, dmu=None, c=1.0):
    """P and the gradients of  c P + sum(dmu * mu)  with respect to sigma and every weight and bias, from fp32 (or any) inputs promoted to
    float64.  Returns dict: P, mu, d_sigma, d_weights, d_biases."""
    x = _d(x).requires_grad_()
    a, sigma = _d(a), _d(sigma).requires_grad_()
    weights, biases = [_d(w).requires_grad_() for w in weights], [_d(b).requires_grad_() for b in biases]
    mu, P = penalty(x, a, sigma, weights, biases)
    total = c * P + ((_d(dmu) * mu).sum() if dmu is not None else 0.0)
    grads = torch.autograd.grad(total, [sigma] + weights + biases)
    L = len(weights)
    return {"P": float(P.detach()), "mu": mu.detach(), "d_sigma": grads[0], "d_weights": list(grads[1:1 + L]), "d_biases": list(grads[1 + L:])}


def case(B, D, hidden, A, seed=0, zero_row=False):
    """fp32 inputs of one case: x, a, sigma, weights, biases (PyTorch's default Linear init), dmu.  zero_row (needs B >= 3): hidden unit 0 of
    the first layer has a zero bias, row 0 of x is zero -- its pre-activation and output there are exactly 0 -- and rows 1 and 2 put that
    unit's pre-activation at +0.25 and -0.25."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + D)
    dims = [D] + list(hidden) + [A]
    weights, biases = [], []
    for n_in, n_out in zip(dims[:-1], dims[1:]):
        k = 1.0 / np.sqrt(n_in)
        weights.append((torch.rand(n_out, n_in, generator=g) * 2 - 1) * k)
        biases.append((torch.rand(n_out, generator=g) * 2 - 1) * k)
    x = torch.randn(B, D, generator=g)
    if zero_row:
        assert B >= 3 and hidden
        biases[0][0] = 0.0
        w = weights[0][0]
        x[0] = 0.0
        x[1] = 0.25 * w / float(w @ w)
        x[2] = -0.25 * w / float(w @ w)
    sigma = 0.3 + 0.5 * torch.rand(A, generator=g)
    with torch.no_grad():
        mu = actor64(x, weights, biases)
    a = mu + sigma * torch.randn(B, A, generator=g)
    dmu = torch.randn(B, A, generator=g) / B
    return x, a, sigma, weights, biases, dmu


def gp_minibatch_ref(ac64, batch, coef, clip, value_loss_coef, entropy_coef, use_clipped):
    """The minibatch loss with the penalty in float64 and its parameter gradients.
    ac64: a float64 ActorCriticMLP; batch: the nine minibatch tensors (obs, cobs, actions, target_values, advantages, returns, old_logp,
    old_mu, old_sigma).  Returns dict: out [surrogate, value_loss, total (with coef P), kl], P, grads (per parameter, in order)."""
    obs, cobs, actions, tv, adv, ret, old_logp, old_mu, old_sigma = [_d(t) for t in batch]
    for p in ac64.parameters():
        p.grad = None
    lin = [m for m in ac64.actor.model if isinstance(m, torch.nn.Linear)]
    sigma = ac64.noise_std()
    mu, P = penalty(obs.requires_grad_(), actions, sigma, [m.weight for m in lin], [m.bias for m in lin])
    value = ac64.critic(cobs)
    ref = ppo_ref.ppo_loss_ref(mu, sigma, value, actions, old_logp, old_mu, old_sigma, adv, ret, tv, clip, value_loss_coef, entropy_coef, use_clipped)
    torch.autograd.backward([mu, value, sigma, P], [ref["d_mu"], ref["d_value"], ref["d_std"], torch.tensor(float(coef), dtype=torch.float64)])
    out = ref["out"].clone()
    out[2] = float(ref["out"][2]) + float(coef) * float(P.detach())
    return {"out": out, "P": float(P.detach()), "grads": [p.grad.clone() for p in ac64.parameters()]}
