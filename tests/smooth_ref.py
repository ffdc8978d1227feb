"""Float64 restatements for rl/smooth.py (the CAPS action-smoothness regulariser), written from the definition and used by
tests/test_smooth.py and tests/test_smooth_gpu.py.

Storage rows are s = t N + e.  Minibatch row r has the source row s = idx[r], t = s // N:

    valid[r] = (t < T - 1) and dones[s] == 0
    actor input, block by block:  own obs[s] | successor obs[s + N] where valid, else obs[s] (temporal) | obs[s] + sigma eps[r] (spatial)
    L_T = sum_{r valid} sum_a (mu[r][a] - mu_succ[r][a])^2 / (A max(n_v, 1))        n_v = sum valid
    L_S = sum_r sum_a (mu[r][a] - mu_pert[r][a])^2 / (A mb)
    total = coef_t L_T + coef_s L_S;  the gradient flows to both sides of each difference; a masked pair is skipped, not multiplied by 0

The minibatch loss with parameter gradients is restated on top of tests/ppo_ref.py, as tests/symmetry_ref.py's is."""
import numpy as np
import torch

from tests import ppo_ref

MODES = {"temporal": (True, False), "spatial": (False, True), "both": (True, True)}


def valid_np(idx, N, T, dones):
    idx = np.asarray(idx, np.int64)
    return (idx // N < T - 1) & (np.asarray(dones).reshape(-1)[idx] == 0)


def gather_np(srcs, idx, N, T, dones, mode, eps=None, sigma=0.0):
    """(the gathered tensors in float64 -- tensor 0 with its extra row blocks --, valid [mb] bool)"""
    succ, pert = MODES[mode]
    idx = np.asarray(idx, np.int64)
    out = [np.asarray(s, np.float64)[idx] for s in srcs]
    v = valid_np(idx, N, T, dones)
    src0 = np.asarray(srcs[0], np.float64)
    blocks = [out[0]]
    if succ:
        blocks.append(src0[np.where(v, idx + N, idx)])
    if pert:
        blocks.append(out[0] + float(sigma) * np.asarray(eps, np.float64))
    out[0] = np.concatenate(blocks)
    return out, v


def loss_and_grad(mu, mode, valid, coef_t, coef_s):
    """(out [4] = L_T, L_S, coef_t L_T + coef_s L_S, n_v; d_mu = d out[2] / d mu) in float64.  Masked pairs are never read: whatever their
    successor rows hold -- a NaN included -- stays out of both."""
    succ, pert = MODES[mode]
    mu = np.asarray(mu, np.float64)
    R = 1 + int(succ) + int(pert)
    mb, A = mu.shape[0] // R, mu.shape[1]
    own = mu[:mb]
    d_mu = np.zeros_like(mu)
    lt = ls = 0.0
    n_v = 0
    if succ:
        v = np.asarray(valid).reshape(-1) != 0
        n_v = int(v.sum())
        d = own[v] - mu[mb:2 * mb][v]
        den = A * max(n_v, 1)
        lt = float((d * d).sum() / den)
        d_mu[:mb][v] += coef_t * 2.0 * d / den
        d_mu[mb:2 * mb][v] -= coef_t * 2.0 * d / den
    if pert:
        p = 2 if succ else 1
        d = own - mu[p * mb:(p + 1) * mb]
        ls = float((d * d).sum() / (A * mb))
        d_mu[:mb] += coef_s * 2.0 * d / (A * mb)
        d_mu[p * mb:(p + 1) * mb] -= coef_s * 2.0 * d / (A * mb)
    total = (coef_t * lt if succ else 0.0) + (coef_s * ls if pert else 0.0)
    return np.array([lt, ls, total, float(n_v)]), d_mu


def loss_inputs(mb, A, mode, mask, seed=0):
    """mu [R mb, A] float32 (successor rows a small step from their own rows, perturbed rows a smaller one) and valid [mb] uint8 with the
    mask "all" / "none" / "mixed" (mixed: at least one of each when mb > 1)"""
    succ, pert = MODES[mode]
    g = np.random.default_rng(1000 * seed + 31 * mb + A)
    own = g.standard_normal((mb, A)).astype(np.float32)
    blocks = [own]
    if succ:
        blocks.append((own + 0.3 * g.standard_normal((mb, A))).astype(np.float32))
    if pert:
        blocks.append((own + 0.05 * g.standard_normal((mb, A))).astype(np.float32))
    valid = {"all": np.ones(mb, bool), "none": np.zeros(mb, bool), "mixed": g.random(mb) < 0.6}[mask]
    if mask == "mixed" and mb > 1:
        valid[0], valid[-1] = True, False
    return np.concatenate(blocks), valid.astype(np.uint8)


def smooth_minibatch_ref(ac64, batch, succ_obs, valid, eps, mode, coef_t, coef_s, sigma, clip, value_loss_coef, entropy_coef, use_clipped):
    """The minibatch loss with smoothness in float64 and its parameter gradients.
    ac64: a float64 ActorCriticMLP; batch: the nine UNEXTENDED minibatch tensors (obs, cobs, actions, target_values, advantages, returns,
    old_logp, old_mu, old_sigma); succ_obs [mb, W]: the successor rows (anything where not valid), valid [mb], eps [mb, W].
    Returns dict: out [surrogate, value_loss, total (with the smoothness terms), kl], terms [L_T, L_S], grads (per parameter, in order)."""
    succ, pert = MODES[mode]
    b = [torch.from_numpy(np.asarray(t.detach().cpu().double().numpy())) for t in batch]
    obs, cobs, actions, tv, adv, ret, old_logp, old_mu, old_sigma = b
    v = np.asarray(valid).reshape(-1) != 0
    blocks = [obs]
    if succ:
        s = torch.from_numpy(np.asarray(succ_obs, np.float64))
        blocks.append(torch.where(torch.from_numpy(v).reshape(-1, 1), s, obs))
    if pert:
        blocks.append(obs + float(sigma) * torch.from_numpy(np.asarray(eps, np.float64)))
    for p in ac64.parameters():
        p.grad = None
    mu, value = ac64.actor(torch.cat(blocks)), ac64.critic(cobs)
    n = actions.shape[0]
    ref = ppo_ref.ppo_loss_ref(mu[:n], ac64.std, value, actions, old_logp, old_mu, old_sigma, adv, ret, tv, clip, value_loss_coef, entropy_coef,
                               use_clipped)
    out4, d_sm = loss_and_grad(mu.detach().numpy(), mode, v, coef_t, coef_s)
    d_mu = d_sm.copy()
    d_mu[:n] += ref["d_mu"].numpy()
    torch.autograd.backward([mu, value, ac64.std], [torch.from_numpy(d_mu), ref["d_value"], ref["d_std"]])
    out = ref["out"].clone()
    out[2] = float(ref["out"][2]) + out4[2]
    return {"out": out, "terms": out4[:2], "n_v": int(out4[3]), "grads": [p.grad.clone() for p in ac64.parameters()]}
