"""The float64 references of tests/ppo_ref.py against torch itself, on the CPU: they must be right before they judge a kernel
(tests/test_ppo_kernels_gpu.py)."""
import math

import numpy as np
import pytest
import torch

from tests import ppo_ref
from wiki_grx_gym_amd.rl.modules import ActorCriticMLP
from wiki_grx_gym_amd.rl.ppo import PPO


def _minibatch(B, A, mu, std, g, value):
    r = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)
    actions = mu + std * r(B, A)
    old_mu = mu + 0.1 * std * r(B, A)
    old_sigma = std * (1.0 + 0.1 * torch.rand(B, A, dtype=torch.float64, generator=g))
    logp = torch.distributions.Normal(mu, std).log_prob(actions).sum(-1, keepdim=True)
    old_logp = logp + 0.2 * r(B, 1)
    return actions, value + 0.2 * r(B, 1), r(B, 1), value + r(B, 1), old_logp, old_mu, old_sigma


@pytest.mark.parametrize("use_clipped", [True, False])
def test_loss_reference_matches_ppo_losses_in_float64(use_clipped):
    """ppo_loss_ref against PPO._losses on the CPU (torch.distributions.Normal, torch.max / clamp autograd) in float64: the four
    scalars, and the parameter gradients reached through the reference's d_mu / d_std / d_value equal the ones `_losses` gives."""
    torch.manual_seed(5)
    B, A = 300, 7
    ac = ActorCriticMLP(11, 13, A, actor_hidden_dims=[16, 8], critic_hidden_dims=[16, 8], activation="elu", init_noise_std=0.3).double()
    with torch.no_grad():
        ac.std.mul_(torch.linspace(0.5, 1.5, A, dtype=torch.float64))
    alg = PPO(ac, clip_param=0.2, value_loss_coef=1.3, entropy_coef=0.01, use_clipped_value_loss=use_clipped, schedule="adaptive",
              desired_kl=0.01, device="cpu")
    g = torch.Generator().manual_seed(7)
    obs, cobs = torch.randn(B, 11, dtype=torch.float64, generator=g), torch.randn(B, 13, dtype=torch.float64, generator=g)
    with torch.no_grad():
        mu, value = ac.actor(obs), ac.critic(cobs)
    actions, tv, adv, ret, old_logp, old_mu, old_sigma = _minibatch(B, A, mu, ac.std.detach(), g, value)
    assert not ppo_ref.loss_near_ties(mu, ac.std, value, actions, old_logp, ret, tv, 0.2).all()

    s, v, loss, kl = alg._losses(obs, cobs, actions, tv, adv, ret, old_logp, old_mu, old_sigma)
    ac.zero_grad(set_to_none=True)
    loss.backward()
    want = [p.grad.clone() for p in ac.parameters()]
    ref = ppo_ref.ppo_loss_ref(mu, ac.std, value, actions, old_logp, old_mu, old_sigma, adv, ret, tv, 0.2, 1.3, 0.01, use_clipped)
    torch.testing.assert_close(ref["out"], torch.stack([s, v, loss, kl]).detach(), rtol=1e-12, atol=1e-14)

    ac.zero_grad(set_to_none=True)
    torch.autograd.backward([ac.actor(obs), ac.critic(cobs), ac.std], [ref["d_mu"], ref["d_value"], ref["d_std"]])
    for (n, p), w in zip(ac.named_parameters(), want):
        torch.testing.assert_close(p.grad, w, rtol=1e-10, atol=1e-14, msg=n)
    # the data reaches both arms of the clipped surrogate: ratios inside the clip interval (exact ties of torch.max) and outside
    ratio = torch.exp(torch.distributions.Normal(mu, ac.std.detach()).log_prob(actions).sum(-1) - old_logp.reshape(-1))
    assert ((ratio > 0.8) & (ratio < 1.2)).any() and ((ratio < 0.8) | (ratio > 1.2)).any()


def test_loss_reference_terms_match_torch_normal():
    """log_prob / entropy as the reference writes them equal torch.distributions.Normal's, per action, float64."""
    g = torch.Generator().manual_seed(2)
    mu = torch.randn(50, 32, dtype=torch.float64, generator=g)
    std = 0.05 + torch.rand(32, dtype=torch.float64, generator=g)
    a = mu + std * torch.randn(50, 32, dtype=torch.float64, generator=g)
    ref = ppo_ref.policy_head_ref(mu, torch.eye(32, dtype=torch.float64), None, std, (a - mu) / std)   # (X W^T = mu)
    torch.testing.assert_close(ref["logp"], torch.distributions.Normal(mu, std).log_prob(a).sum(-1), rtol=1e-13, atol=1e-12)
    ent = (0.5 + ppo_ref.LOG_SQRT_2PI + torch.log(std)).sum()
    torch.testing.assert_close(ent, torch.distributions.Normal(mu[0], std).entropy().sum(), rtol=1e-14, atol=0)


def test_near_tie_mask_finds_the_branch_points():
    """loss_near_ties flags a ratio at 1 +- clip and |v - tv| at clip, and not an exact tie inside the interval."""
    A = 3
    mu = torch.zeros(4, A, dtype=torch.float64)
    std = torch.ones(A, dtype=torch.float64)
    actions = torch.zeros(4, A, dtype=torch.float64)
    logp = float(torch.distributions.Normal(0.0, 1.0).log_prob(torch.tensor(0.0, dtype=torch.float64))) * A
    old_logp = torch.tensor([logp - math.log(1.2), logp - math.log(0.8005), logp, logp], dtype=torch.float64)
    value = torch.tensor([0.0, 0.0, 0.0, 0.7], dtype=torch.float64)
    tv = torch.tensor([0.0, 0.0, 0.0, 0.5004], dtype=torch.float64)
    ret = torch.full((4,), 3.0, dtype=torch.float64)
    assert ppo_ref.loss_near_ties(mu, std, value, actions, old_logp, ret, tv, 0.2).tolist() == [True, True, False, True]


@pytest.mark.parametrize("max_norm", [0.05, 1e3])
def test_tail_reference_matches_clip_grad_norm_and_adam(max_norm):
    """step_tail_ref against nn.utils.clip_grad_norm_ + torch.optim.Adam(foreach=False) in float64 over five steps, clipping active
    (max_norm below the gradient norm) and not."""
    g = torch.Generator().manual_seed(9)
    shapes = [(7, 5), (5,), (1,), (3, 7), (1030,)]
    ps = [torch.randn(*s, dtype=torch.float64, generator=g).requires_grad_() for s in shapes]
    opt = torch.optim.Adam(ps, lr=3e-3, betas=(0.9, 0.999), eps=1e-8, foreach=False)
    P = [p.detach().clone() for p in ps]
    M = [torch.zeros_like(p) for p in P]
    V = [torch.zeros_like(p) for p in P]
    S = [0.0] * len(P)
    for it in range(5):
        grads = [torch.randn(*s, dtype=torch.float64, generator=g) * (0.1 + it) for s in shapes]
        for p, gr in zip(ps, grads):
            p.grad = gr.clone()
        total = torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False)
        opt.step()
        r = ppo_ref.step_tail_ref(P, grads, M, V, S, 3e-3, 1.0, None, max_norm, 0.9, 0.999, 1e-8)
        assert r["clip"] < 1.0 if max_norm < 1 else r["clip"] == 1.0
        assert abs(r["total"] - float(total)) <= 1e-12 * float(total)
        P, M, V, S = r["params"], r["exp_avg"], r["exp_avg_sq"], r["steps"]
        for p, q, m, v in zip(ps, P, M, V):
            st = opt.state[p]
            torch.testing.assert_close(q, p.detach(), rtol=1e-13, atol=1e-15)
            torch.testing.assert_close(m, st["exp_avg"], rtol=1e-13, atol=1e-18)
            torch.testing.assert_close(v, st["exp_avg_sq"], rtol=1e-13, atol=1e-20)
            assert float(st["step"]) == S[0] == it + 1
    # a skipped step moves nothing
    for bad in ((float("nan"), None), (float("inf"), None), (1.0, 1.0)):
        r = ppo_ref.step_tail_ref(P, grads, M, V, S, 3e-3, bad[0], bad[1], max_norm, 0.9, 0.999, 1e-8)
        assert r["skipped"] and r["steps"] == S and all(torch.equal(a, b) for a, b in zip(r["params"], P))


@pytest.mark.parametrize("step0", [0, 1000])
def test_tail_reference_skips_on_a_non_finite_gradient_norm(step0):
    """step_tail_ref's skip rule under a finite loss: one NaN, +inf, -inf or 1e20 gradient element (the last: finite, its square above
    the largest float32) gives `skipped` and untouched state; one 1e17 element (square 1e34: representable) does not skip and equals
    float64 clip_grad_norm_ + torch.optim.Adam, clipping active and not."""
    g = torch.Generator().manual_seed(17)
    shapes = [(7, 5), (1,), (1030,), (3, 7)]
    P = [torch.randn(*s, dtype=torch.float64, generator=g) for s in shapes]
    M = [torch.randn(*s, dtype=torch.float64, generator=g) * 0.01 * bool(step0) for s in shapes]
    V = [torch.rand(*s, dtype=torch.float64, generator=g) * 1e-4 * bool(step0) for s in shapes]
    S = [float(step0)] * len(P)
    grads = [torch.randn(*s, generator=g) * 0.1 for s in shapes]   # (fp32, as the kernel's)
    for value in (float("nan"), float("inf"), float("-inf"), 1e20):
        for t, e in ((0, 0), (2, 1029), (3, 20)):
            G = [x.clone() for x in grads]
            G[t].view(-1)[e] = value
            r = ppo_ref.step_tail_ref(P, G, M, V, S, 3e-3, 0.7, None, 0.05, 0.9, 0.999, 1e-8)
            assert r["skipped"] and r["steps"] == S, (value, t, e)
            for new, old in ((r["params"], P), (r["exp_avg"], M), (r["exp_avg_sq"], V)):
                assert all(torch.equal(a, b) for a, b in zip(new, old)), (value, t, e)
    G = [x.clone() for x in grads]
    G[2][517] = 1e17
    for max_norm in (0.5e17, 1e19):
        ps = [p.clone().requires_grad_() for p in P]
        opt = torch.optim.Adam(ps, lr=3e-3, betas=(0.9, 0.999), eps=1e-8, foreach=False)
        for p, gr, m, v in zip(ps, G, M, V):
            opt.state[p] = {"step": torch.tensor(float(step0)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
            p.grad = gr.double()
        total = torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False)
        opt.step()
        r = ppo_ref.step_tail_ref(P, G, M, V, S, 3e-3, 0.7, None, max_norm, 0.9, 0.999, 1e-8)
        assert not r["skipped"] and r["steps"] == [step0 + 1.0] * len(P)
        assert r["clip"] < 0.6 if max_norm < 1e18 else r["clip"] == 1.0
        assert abs(r["total"] - float(total)) <= 1e-12 * float(total)
        for p, q, m, v in zip(ps, r["params"], r["exp_avg"], r["exp_avg_sq"]):
            st = opt.state[p]
            torch.testing.assert_close(q, p.detach(), rtol=1e-13, atol=1e-15)
            torch.testing.assert_close(m, st["exp_avg"], rtol=1e-13, atol=1e-18)
            torch.testing.assert_close(v, st["exp_avg_sq"], rtol=1e-13, atol=1e-20)


def test_lr_rule_matches_the_device_update():
    """lr_rule_fp32 against PPO._device_lr_update on fp32 CPU tensors for every branch (down, up, keep, kl == 0, both clamps).  (On a
    HIP device torch divides by the host scalar 1.5 as a product with its fp32 reciprocal; the rule spells that product, so here the
    comparison allows the one-ulp difference of a true division, and the GPU module checks the kernel against the device path bit for bit.)"""
    class _Alg:
        desired_kl, learning_rate_min, learning_rate_max = 0.01, 1e-5, 1e-3
    for lr, kl in ((1e-4, 0.05), (1e-4, 0.001), (1e-4, 0.01), (1e-4, 0.0), (1.2e-5, 0.5), (9e-4, 1e-4), (1e-4, 0.02), (1e-4, 0.005)):
        a = _Alg()
        a._lr_t = torch.tensor(lr, dtype=torch.float32)
        PPO._device_lr_update(a, torch.tensor(kl, dtype=torch.float32))
        want = np.float32(a._lr_t.item())
        got = ppo_ref.lr_rule_fp32(lr, kl, True, 0.01, 1e-5, 1e-3)
        assert abs(float(got) - float(want)) <= float(np.spacing(want)), (lr, kl, got, want)
    assert ppo_ref.lr_rule_fp32(1e-4, 0.05, False, 0.01, 1e-5, 1e-3) == np.float32(1e-4)
