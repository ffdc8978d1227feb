"""Multi-critic PPO on the GPU (include/grx_ppo_mc.h: grx_mc_store, grx_mc_returns, grx_mc_loss; rl/multi_critic.py): the
bit-equalities with the entries they are modelled on, row independence, the float64 parity of what has no bit-equal twin, the argument
checks with sentinels, and the runner on the HIP device -- captured against eager, fused against GRX_MC_FUSED=0, save / load / play /
export, the second term table, the default path.

GRX_MC_PARITY_JSON=<path>: the parity tests also write their per-case error ratios there (profiles/multi_critic_parity.json is such a file)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import mc_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TS, NS, KS = (1, 2, 7), (1, 63, 64, 65, 130), (1, 2, 3, 8)
SPEC = "track=cmd_diff_lin_vel_x,cmd_diff_lin_vel_y,cmd_diff_ang_vel_yaw;rest=*"
SENTINEL = 777.0


def _M():
    from wiki_grx_gym_amd.rl import multi_critic
    return multi_critic


def _d(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _full(*shape):
    return torch.full(shape, SENTINEL, device=DEV)


def _same_bytes(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.fixture(scope="module")
def parity():
    rows = {}
    yield rows
    path = os.environ.get("GRX_MC_PARITY_JSON")
    if path and rows:
        with open(path, "w") as f:
            json.dump({"margin": R.MARGIN, "what": "max |kernel - float64| over the tensor, divided by e32 = max |the fp32 torch spelling on the "
                       "CPU - float64| of the same operation (at least u max |float64|); tests/mc_ref.py held()", "cases": rows}, f, indent=1)


def _hold(parity, case, name, got, spelled, want):
    err, e32, ratio = R.held(got.detach().cpu().double().numpy(), spelled.detach().cpu().double().numpy(), want)
    parity[f"{case},{name}"] = {"e32": e32, "error": err, "ratio": round(ratio, 3)}
    print(f"{case} {name}: error {err:.3g}, e32 {e32:.3g}, ratio {ratio:.3g}")
    assert err <= R.MARGIN * e32, (case, name, err, e32, ratio)


def _hold_pooled(parity, case, name, triples):
    """a one-number quantity over the cases of one shape: the largest error against the largest e32.  One number's fp32 error can be far
    below its typical size by luck -- a sum of cancelling terms whose rounding errors happen to cancel too --, so a single case says
    nothing about "an equally good evaluation order"; the cases of a shape together do (tests/test_value_norm_gpu.py: "arrays per case,
    one-number quantities per shape")"""
    held = [R.held(g.detach().cpu().double().numpy(), s.detach().cpu().double().numpy(), w) for g, s, w in triples]
    err, e32 = max(h[0] for h in held), max(h[1] for h in held)
    parity[f"{case},{name}"] = {"e32": e32, "error": err, "ratio": round(err / e32 if e32 > 0 else 0.0, 3), "cases": len(held)}
    print(f"{case} {name} ({len(held)} cases): error {err:.3g}, e32 {e32:.3g}, ratio {err / e32 if e32 > 0 else 0.0:.3g}")
    assert err <= R.MARGIN * e32, (case, name, err, e32)


# ---- grx_mc_returns ----------------------------------------------------------------------------------------------------------------------------
def _returns(r, v, d, last, w):
    M = _M()
    T, N, K = r.shape
    ret, adv = _full(T, N, K), _full(T, N)
    stats = M.mc_returns_hip(_d(r), _d(v), _d(d), _d(last), w, R.GAMMA, R.LAM, ret, adv)
    return ret, adv, stats


def _gae(r, v, d, last):
    """grx_gae_returns without a state on one column [T, N]"""
    from wiki_grx_gym_amd.rl.value_norm import gae_returns_hip
    T, N = r.shape
    ret, adv = _full(T, N), _full(T, N)
    gae_returns_hip(_d(r), _d(v), _d(d), _d(last), R.GAMMA, R.LAM, 1e-5, None, ret, adv)
    return ret, adv


@pytest.mark.parametrize("T", TS)
def test_one_group_is_grx_gae_returns_byte_for_byte(T):
    for N in NS:
        r, v, d, last = R.rollout(T, N, 1)
        ret, adv, _ = _returns(r, v, d, last, [1.0])
        want_ret, want_adv = _gae(r[..., 0], v[..., 0], d, last[..., 0])
        assert _same_bytes(ret[..., 0], want_ret), (T, N)
        assert _same_bytes(adv, want_adv), (T, N)
        assert bool(torch.isnan(adv).all()) == (T * N == 1)                          # T N = 1: the NaN torch.std gives


@pytest.mark.parametrize("K", KS)
def test_a_column_is_grx_gae_returns_on_that_column(K):
    for T in TS:
        for N in NS:
            r, v, d, last = R.rollout(T, N, K)
            ret, _, _ = _returns(r, v, d, last, R.weights(K))
            for k in range(K):
                want, _ = _gae(np.ascontiguousarray(r[..., k]), np.ascontiguousarray(v[..., k]), d, np.ascontiguousarray(last[..., k]))
                assert _same_bytes(ret[..., k], want), (T, N, K, k)


def test_an_envs_returns_do_not_depend_on_its_neighbours():
    for K in KS:
        r, v, d, last = R.rollout(7, 130, K)
        ret, _, _ = _returns(r, v, d, last, R.weights(K))
        for n in (0, 63, 64, 129):
            alone, _, _ = _returns(r[:, n:n + 1].copy(), v[:, n:n + 1].copy(), d[:, n:n + 1].copy(), last[n:n + 1].copy(), R.weights(K))
            assert _same_bytes(ret[:, n:n + 1], alone), (K, n)
        other = r.copy(); other[:, 1:] *= -3.0                                      # ... nor on what the others hold
        again, _, _ = _returns(other, v, d, last, R.weights(K))
        assert _same_bytes(ret[:, :1], again[:, :1])


@pytest.mark.parametrize("K", [2, 3, 8])
def test_advantages_and_stats_against_float64(K, parity):
    M = _M()
    for T in TS:
        for N in NS:
            if T * N == 1:
                continue
            r, v, d, last = R.rollout(T, N, K)
            w = R.weights(K)
            ref = R.returns(r, v, d, last, w)
            ret32, adv32, stats32 = torch.zeros(T, N, K), torch.zeros(T, N), torch.zeros(K, 2)
            M.mc_returns_torch(torch.from_numpy(r), torch.from_numpy(v), torch.from_numpy(d), torch.from_numpy(last), w, R.GAMMA, R.LAM,
                               ret32, adv32, stats32)
            ret, adv, stats = _returns(r, v, d, last, w)
            assert torch.equal(ret.cpu(), ret32)                                    # (the recursion is the torch loop's, bit for bit)
            case = f"returns,{T}x{N}x{K}"
            _hold(parity, case, "advantages", adv, adv32, ref["advantages"])
            for k in range(K):                                                      # per group: the groups' scales differ by 4^k
                _hold(parity, case, f"mean_{k}", stats[k, 0], stats32[k, 0], ref["stats"][k, 0])
                _hold(parity, case, f"std_{k}", stats[k, 1], stats32[k, 1], ref["stats"][k, 1])


def test_a_constant_group_and_a_single_transition_come_out_as_torchs():
    M = _M()
    T, N, K = 7, 65, 2
    r, v, d, last = R.rollout(T, N, K)
    d[:] = 1                                                                        # every step ends: a = r - v
    v[..., 1] = np.round(v[..., 1]); r[..., 1] = v[..., 1] + 0.5                    # group 1: a = 0.5 everywhere, exactly
    ret32, adv32, stats32 = torch.zeros(T, N, K), torch.zeros(T, N), torch.zeros(K, 2)
    M.mc_returns_torch(torch.from_numpy(r), torch.from_numpy(v), torch.from_numpy(d), torch.from_numpy(last), [1.0, 2.0], R.GAMMA, R.LAM,
                       ret32, adv32, stats32)
    ret, adv, stats = _returns(r, v, d, last, [1.0, 2.0])
    assert float(stats32[1, 1]) == 0.0 and float(stats32[1, 0]) == 0.5
    assert torch.equal(stats[1].cpu(), stats32[1]) and torch.equal(ret.cpu(), ret32)
    ref = R.returns(r, v, d, last, [1.0, 2.0])
    assert bool(torch.isfinite(adv).all()) and np.array_equal(ref["normalised"][..., 1], np.zeros((T, N)))
    err, e32, _ = R.held(adv.cpu().numpy(), adv32.numpy(), ref["advantages"])       # group 1 adds 2 * 0 / 1e-8 = 0 on both sides
    assert err <= R.MARGIN * e32
    r, v, d, last = R.rollout(1, 1, 3)                                              # T N = 1
    ret, adv, stats = _returns(r, v, d, last, R.weights(3))
    ret32, adv32, stats32 = torch.zeros(1, 1, 3), torch.zeros(1, 1), torch.zeros(3, 2)
    M.mc_returns_torch(torch.from_numpy(r), torch.from_numpy(v), torch.from_numpy(d), torch.from_numpy(last), R.weights(3), R.GAMMA, R.LAM,
                       ret32, adv32, stats32)
    assert bool(torch.isnan(adv).all()) and bool(torch.isnan(adv32).all()) and bool(torch.isnan(stats[:, 1]).all())
    assert torch.equal(stats[:, 0].cpu(), stats32[:, 0]) and torch.equal(ret.cpu(), ret32)


# ---- grx_mc_store ------------------------------------------------------------------------------------------------------------------------------
def _store(terms, base, group, values, to, K):
    M = _M()
    N = values.shape[0]
    sv, sr = _full(N, K), _full(N, K)
    M.mc_store_hip(_d(terms), _d(base) if base is not None else None, _d(group[:terms.shape[0] + (0 if base is None else base.shape[0])]),
                   _d(values), _d(to) if to is not None else None, R.GAMMA, sv, sr)
    return sv, sr


@pytest.mark.parametrize("K", KS)
def test_group_sums_are_the_fp32_chain(K):
    M = _M()
    for N in NS:
        for NT, NB in ((36, 15), (36, 0), (1, 0), (5, 3)):
            terms, base, group, values, to = R.tables(N, NT, NB, K)
            for tos in (None, to):
                sv, sr = _store(terms, base, group, values, tos, K)
                chain = [torch.zeros(N) for _ in range(K)]                          # ((0 + t_a) + t_b) + ... in table order, main table first
                table = [torch.from_numpy(x) for x in terms] + ([torch.from_numpy(x) for x in base] if base is not None else [])
                for t, g in enumerate(group[:len(table)]):
                    if g >= 0:
                        chain[g] = chain[g] + table[t]
                want = torch.stack(chain, 1)
                if tos is not None:
                    boot = torch.tensor(R.GAMMA, dtype=torch.float32) * torch.from_numpy(values)
                    want = want + torch.where(torch.from_numpy(tos).reshape(N, 1) != 0, boot, torch.zeros(N, K))
                assert _same_bytes(sr.cpu(), want), (N, NT, NB, K, tos is not None)
                assert _same_bytes(sv.cpu(), torch.from_numpy(values))
                sv32, sr32 = torch.zeros(N, K), torch.zeros(N, K)                   # ... which is the torch spelling
                M.mc_store_torch(torch.from_numpy(terms), torch.from_numpy(base) if base is not None else None, group.tolist(),
                                 torch.from_numpy(values), torch.from_numpy(tos) if tos is not None else None, R.GAMMA, sv32, sr32)
                assert _same_bytes(sr32, want)


def test_an_envs_group_rewards_do_not_depend_on_its_neighbours():
    terms, base, group, values, to = R.tables(130, 36, 15, 3)
    sv, sr = _store(terms, base, group, values, to, 3)
    for n in (0, 63, 64, 129):
        _, alone = _store(terms[:, n:n + 1].copy(), base[:, n:n + 1].copy(), group, values[n:n + 1].copy(), to[n:n + 1].copy(), 3)
        assert _same_bytes(sr[n:n + 1], alone), n


# ---- grx_mc_loss -------------------------------------------------------------------------------------------------------------------------------
def _loss(b, K, use_clipped=True):
    """grx_mc_loss on the minibatch dict `b`: (out [4 + K], d_mu, d_std, d_value)"""
    M = _M()
    t = {k: _d(x) for k, x in b.items()}
    for k in ("mu", "std", "value"):
        t[k].requires_grad_(True)
    out = M.fused_mc_loss(t["mu"], t["std"], t["value"], t["actions"], t["old_logp"], t["old_mu"], t["old_sigma"], t["advantages"], t["returns"],
                          t["target_values"], 0.2, 1.0, 0.01, use_clipped)
    out[2].backward()
    return out.detach(), t["mu"].grad, t["std"].grad, t["value"].grad


@pytest.mark.parametrize("A", [1, 10, 32])
@pytest.mark.parametrize("B", [1, 255, 257, 1000])
def test_one_head_is_grx_ppo_loss_byte_for_byte(B, A):
    from wiki_grx_gym_amd.rl.fused_loss import fused_ppo_loss
    for use_clipped in (True, False):
        b = R.minibatch(B, A, 1)
        out, d_mu, d_std, d_value = _loss(b, 1, use_clipped)
        t = {k: _d(x) for k, x in b.items()}
        for k in ("mu", "std", "value"):
            t[k].requires_grad_(True)
        want = fused_ppo_loss(t["mu"], t["std"], t["value"], t["actions"], t["old_logp"], t["old_mu"], t["old_sigma"], t["advantages"],
                              t["returns"], t["target_values"], 0.2, 1.0, 0.01, use_clipped)
        want[2].backward()
        assert _same_bytes(out[:4], want.detach()) and _same_bytes(out[4:], want.detach()[1:2]), (B, A, use_clipped)
        assert _same_bytes(d_mu, t["mu"].grad) and _same_bytes(d_std, t["std"].grad) and _same_bytes(d_value, t["value"].grad)


def _record(parity, case, name, got, spelled, want):
    """held()'s figures into the parity file, without a verdict: the case of the largest ratio under this key stays"""
    err, e32, ratio = R.held(got.detach().cpu().double().numpy(), spelled.detach().cpu().double().numpy(), want)
    if ratio >= parity.get(f"{case},{name}", {"ratio": -1.0})["ratio"]:
        parity[f"{case},{name}"] = {"e32": e32, "error": err, "ratio": round(ratio, 3),
                                    "held_by": "the chain's forward-error bound (tests/mc_ref.py loss_chain_bounds)"}
    return ratio


@pytest.mark.parametrize("K", [2, 3, 8])
def test_what_has_a_twin_is_grx_ppo_loss_byte_for_byte(K):
    """for any K the policy side does not see the heads, and a head does not see the others: the surrogate, the KL, d_mu and d_std are
    grx_ppo_loss's on the same minibatch with any one value column, and head k's loss and its d_value column are grx_ppo_loss's on column k"""
    from wiki_grx_gym_amd.rl.fused_loss import fused_ppo_loss
    for B in (1, 255, 257, 1000):
        for A in (1, 10, 32):
            for use_clipped in (True, False):
                b = R.minibatch(B, A, K)
                out, d_mu, d_std, d_value = _loss(b, K, use_clipped)
                for k in range(K):
                    t = {n: _d(x) for n, x in b.items()}
                    for n in ("value", "returns", "target_values"):
                        t[n] = t[n][:, k:k + 1].contiguous()
                    for n in ("mu", "std", "value"):
                        t[n].requires_grad_(True)
                    want = fused_ppo_loss(t["mu"], t["std"], t["value"], t["actions"], t["old_logp"], t["old_mu"], t["old_sigma"],
                                          t["advantages"], t["returns"], t["target_values"], 0.2, 1.0, 0.0, use_clipped)
                    # (entropy_coef 0 here and below: with it the total's gradient on std is the same in both, without the heads' share)
                    want[2].backward()
                    where = (B, A, K, k, use_clipped)
                    assert _same_bytes(out[0:1], want.detach()[0:1]) and _same_bytes(out[3:4], want.detach()[3:4]), where
                    assert _same_bytes(out[4 + k:5 + k], want.detach()[1:2]) and _same_bytes(d_value[:, k:k + 1], t["value"].grad), where
                    assert _same_bytes(d_mu, t["mu"].grad), where
                t = {n: _d(x) for n, x in b.items()}                               # d_std carries the entropy's share: the same coefficient
                for n in ("value", "returns", "target_values"):
                    t[n] = t[n][:, :1].contiguous()
                for n in ("mu", "std", "value"):
                    t[n].requires_grad_(True)
                fused_ppo_loss(t["mu"], t["std"], t["value"], t["actions"], t["old_logp"], t["old_mu"], t["old_sigma"], t["advantages"],
                               t["returns"], t["target_values"], 0.2, 1.0, 0.01, use_clipped)[2].backward()
                assert _same_bytes(d_std, t["std"].grad), (B, A, K, use_clipped)


@pytest.mark.parametrize("K", [2, 3, 8])
def test_loss_against_float64(K, parity):
    """grx_mc_loss's outputs and gradients against float64, four seeds and both value losses per shape.
      d_value, per head and per case, and -- one number each, so per shape: the largest error of the shape's eight cases against the largest
        e32, tests/test_value_norm_gpu.py's rule for one-number quantities -- every head's loss, their sum, the KL and the total: within the
        margin (4x) over the torch spelling's own error.  The total contains the surrogate and so inherits the chain error described next;
        it meets the margin only pooled (3.73 at 255 x 32 x 8), where the value losses' magnitude sets its scale.
      the surrogate, d_mu and d_std CANNOT meet that margin: grx_ppo_loss adds a row's A log-probability terms in one fp32 chain where
        torch's sum(dim=-1) adds them in vector lanes, and d_std's x - 1 / s cancels; byte equality with grx_ppo_loss (K = 1, and the test
        above for any K) forbids another evaluation.  Measured on the MI355X, their ratios to the spelling's error reach 7.9 (d_mu,
        257 x 32 x 3), 6.0 (d_std, 257 x 32 x 3; 5.1 at 257 x 1 x 8) and 4.3 (surrogate, 1000 x 32 x 8); they are written to the parity
        file.  What is ASSERTED for the three is the forward-error bound of that chain, derived in tests/mc_ref.py loss_chain_bounds
        (element-wise; a row whose ratio lies within its own error of an edge of the clip has no d_mu bound, its gradient jumps there)."""
    M = _M()
    names = ["surrogate", "value_loss", "loss", "kl"] + [f"head_{k}" for k in range(K)]
    for B in (1, 255, 257, 1000):
        for A in (1, 10, 32):
            pooled = {n: [] for n in names}
            shape = f"loss,{B}x{A}x{K}"
            for seed in range(4):
                for use_clipped in (True, False):
                    b = R.minibatch(B, A, K, seed)
                    ref = R.loss(b, use_clipped=use_clipped)
                    t = {k: torch.from_numpy(x).requires_grad_(k in ("mu", "std", "value")) for k, x in b.items()}
                    s, vl, total, kl, heads = M.mc_loss_torch(t["mu"], t["mu"] * 0.0 + t["std"], t["value"], t["actions"], t["old_logp"],
                                                              t["old_mu"], t["old_sigma"], t["advantages"], t["returns"], t["target_values"],
                                                              0.2, 1.0, 0.01, use_clipped)
                    total.backward()
                    out, d_mu, d_std, d_value = _loss(b, K, use_clipped)
                    spelled = [s, vl, total, kl] + list(heads)
                    for i, name in enumerate(names):
                        pooled[name].append((out[i], spelled[i], ref["out"][i]))
                    case = f"{shape},{'clipped' if use_clipped else 'plain'},seed{seed}"
                    for k in range(K):                                              # per head: the heads' scales differ by 4^k
                        err, e32, ratio = R.held(d_value[:, k].cpu().numpy(), t["value"].grad[:, k].numpy(), ref["d_value"][:, k])
                        if ratio >= parity.get(f"{shape},d_value_{k}", {"ratio": -1.0})["ratio"]:
                            parity[f"{shape},d_value_{k}"] = {"e32": e32, "error": err, "ratio": round(ratio, 3)}
                        assert err <= R.MARGIN * e32, (case, k, err, e32)
                    # the chain's quantities: the derived bound asserted, the ratio to the spelling's error recorded
                    bound = R.loss_chain_bounds(b, ref)
                    _record(parity, shape, "d_mu", d_mu, t["mu"].grad, ref["d_mu"])
                    _record(parity, shape, "d_std", d_std, t["std"].grad, ref["d_std"])
                    keep = ~bound["edge"]
                    e_mu = np.abs(d_mu.cpu().double().numpy() - ref["d_mu"])
                    assert bool((e_mu[keep] <= bound["d_mu"][keep]).all()), (case, "d_mu", float((e_mu[keep] / bound["d_mu"][keep]).max()))
                    e_std = np.abs(d_std.cpu().double().numpy() - ref["d_std"])
                    assert bool((e_std <= bound["d_std"]).all()), (case, "d_std", float((e_std / bound["d_std"]).max()))
                    e_s = abs(float(out[0]) - ref["out"][0])
                    assert e_s <= bound["surrogate"], (case, "surrogate", e_s, bound["surrogate"])
            for name in names:
                if name == "surrogate":
                    held = [R.held(g.detach().cpu().double().numpy(), sp.detach().cpu().double().numpy(), w) for g, sp, w in pooled[name]]
                    err, e32 = max(h[0] for h in held), max(h[1] for h in held)
                    parity[f"{shape},surrogate"] = {"e32": e32, "error": err, "ratio": round(err / e32, 3), "cases": len(held),
                                                    "held_by": "the chain's forward-error bound (tests/mc_ref.py loss_chain_bounds)"}
                else:
                    _hold_pooled(parity, shape, name, pooled[name])


def test_a_rows_gradients_do_not_depend_on_the_rows_beside_it():
    b = R.minibatch(257, 10, 3)
    _, d_mu, _, d_value = _loss(b, 3)
    c = {k: v.copy() for k, v in b.items()}
    for k in ("mu", "value", "actions", "returns", "advantages"):
        c[k][1:] = c[k][1:] * 1.5 + 0.25
    _, d_mu2, _, d_value2 = _loss(c, 3)
    assert _same_bytes(d_mu[:1], d_mu2[:1]) and _same_bytes(d_value[:1], d_value2[:1])
    assert not _same_bytes(d_mu[1:], d_mu2[1:])


def test_non_finite_inputs_follow_the_torch_spelling():
    """grx_ppo_loss's contract: a NaN value reaches the loss (the NaN-skip must fire), and the other head's gradients stay finite"""
    M = _M()
    b = R.minibatch(64, 10, 2)
    b["value"][3, 1] = np.nan
    out, d_mu, d_std, d_value = _loss(b, 2)
    t = {k: torch.from_numpy(x).requires_grad_(k in ("mu", "std", "value")) for k, x in b.items()}
    s, vl, total, kl, heads = M.mc_loss_torch(t["mu"], t["mu"] * 0.0 + t["std"], t["value"], t["actions"], t["old_logp"], t["old_mu"],
                                              t["old_sigma"], t["advantages"], t["returns"], t["target_values"], 0.2, 1.0, 0.01, True)
    total.backward()
    spelled = torch.stack([s, vl, total, kl] + list(heads)).detach()
    assert torch.equal(torch.isfinite(out).cpu(), torch.isfinite(spelled)) and not bool(torch.isfinite(out[2]))
    assert torch.equal(torch.isfinite(d_value).cpu(), torch.isfinite(t["value"].grad)) and bool(torch.isfinite(d_value[:, 0]).all())
    assert bool(torch.isfinite(d_mu).all()) and bool(torch.isfinite(t["mu"].grad).all())


# ---- invalid arguments leave sentinel-filled outputs untouched ----------------------------------------------------------------------------------
def test_invalid_arguments_write_nothing():
    M = _M()
    lib = M._lib()
    T, N, K, NT, NB, B, A = 2, 65, 2, 36, 15, 257, 10
    p = lambda t: t.data_ptr() if t is not None else None
    untouched = lambda *ts: all(bool((t == SENTINEL).all()) for t in ts)
    # grx_mc_store
    terms, base, group, values, to = (_d(x) for x in R.tables(N, NT, NB, K))
    sv, sr = _full(N, K), _full(N, K)
    store = lambda N_=N, K_=K, NT_=NT, NB_=NB, terms_=terms, base_=base, group_=group, values_=values, sv_=sv, sr_=sr: lib.grx_mc_store(
        N_, K_, NT_, NB_, p(terms_), p(base_), p(group_), p(values_), p(to), R.GAMMA, p(sv_), p(sr_), None)
    for rc in (store(N_=0), store(K_=0), store(K_=9), store(NT_=0), store(NB_=0), store(terms_=None), store(group_=None), store(values_=None),
               store(sv_=None), store(sr_=None), store(sv_=values), store(sr_=sv)):
        assert rc < 0
    bad = group.clone(); bad[3] = K                                                 # a map entry >= K: seen by the device alone, writes nothing
    assert store(group_=bad) == 0
    torch.cuda.synchronize()
    assert untouched(sv, sr)
    assert store() == 0
    torch.cuda.synchronize()
    assert not untouched(sr) and torch.equal(sv, values)
    # grx_mc_returns
    r, v, d, last = (_d(x) for x in R.rollout(T, N, K))
    ret, adv, stats = _full(T, N, K), _full(T, N), _full(K, 2)
    part = _full(lib.grx_mc_partials_size(T, N, K) + 2)
    w = (C.c_float * K)(1.0, 1.0)
    rets = lambda T_=T, N_=N, K_=K, r_=r, v_=v, d_=d, last_=last, w_=w, ret_=ret, adv_=adv, stats_=stats, part_=p(part): lib.grx_mc_returns(
        T_, N_, K_, p(r_), p(v_), p(d_), p(last_), w_, R.GAMMA, R.LAM, p(ret_), p(adv_), p(stats_), part_, None)
    for rc in (rets(T_=0), rets(N_=0), rets(K_=0), rets(K_=9), rets(r_=None), rets(v_=None), rets(d_=None), rets(last_=None), rets(w_=None),
               rets(ret_=None), rets(adv_=None), rets(stats_=None), rets(part_=None), rets(part_=p(part) + 4), rets(ret_=v), rets(adv_=r),
               rets(w_=(C.c_float * K)(1.0, 0.0)), rets(w_=(C.c_float * K)(float("nan"), 1.0))):
        assert rc < 0
    torch.cuda.synchronize()
    assert untouched(ret, adv, stats, part)
    # grx_mc_loss
    t = {k: _d(x) for k, x in R.minibatch(B, A, K).items()}
    out, d_mu, d_std, d_value = _full(4 + K), _full(B, A), _full(A), _full(B, K)
    lpart = _full(lib.grx_mc_loss_partials_size(B) + 2)
    names = ("mu", "std", "value", "actions", "old_logp", "old_mu", "old_sigma", "advantages", "returns", "target_values")

    def loss(B_=B, A_=A, K_=K, out_=out, d_mu_=d_mu, d_std_=d_std, d_value_=d_value, part_=p(lpart), **kw):
        a = {**t, **kw}
        return lib.grx_mc_loss(B_, A_, K_, *[p(a[n]) for n in names], 0.2, 1.0, 0.01, 1, p(out_), p(d_mu_), p(d_std_), p(d_value_), part_, None)
    for rc in (loss(B_=0), loss(A_=0), loss(A_=33), loss(K_=0), loss(K_=9), loss(out_=None), loss(d_mu_=None), loss(d_std_=None),
               loss(d_value_=None), loss(part_=None), loss(part_=p(lpart) + 4), loss(d_value_=t["value"]), loss(d_mu_=t["mu"]),
               *[loss(**{n: None}) for n in names]):
        assert rc < 0
    torch.cuda.synchronize()
    assert untouched(out, d_mu, d_std, d_value, lpart)


# ---- the runner on the HIP device ----------------------------------------------------------------------------------------------------------------
def _make(tmp_path, flags=("--reward_groups", SPEC), steps=8, num_envs=64, epochs=2, task="GR1T1", cfg=None, publish=True):
    from wiki_grx_gym_amd.envs import GR1T1Cfg, GR1T1CfgPPO, GR1T1FullBodyCfgPPO
    from wiki_grx_gym_amd.utils import get_args, task_registry
    args = get_args(["--task", task, "--headless", "--num_envs", str(num_envs), "--seed", "3", *flags])
    cfg = GR1T1Cfg() if cfg is None else cfg
    if publish:
        cfg.env.publish_reward_terms = True
    env, _ = task_registry.make_env(task, args=args, env_cfg=cfg)
    tcfg = GR1T1CfgPPO() if task == "GR1T1" else GR1T1FullBodyCfgPPO()
    tcfg.runner.num_steps_per_env = steps
    tcfg.algorithm.num_mini_batches, tcfg.algorithm.num_learning_epochs = 4, epochs
    runner, _ = task_registry.make_alg_runner(env, name=None, args=args, train_cfg=tcfg, log_root=str(tmp_path) if tmp_path else None)
    return env, runner


def _state(alg):
    return [t.detach().clone() for p in alg.actor_critic.parameters() for t in
            (p, alg.optimizer.state[p]["exp_avg"], alg.optimizer.state[p]["exp_avg_sq"])]


def test_captured_update_equals_eager_update_and_the_groups_add_up(tmp_path, monkeypatch):
    """64 envs x 8 steps, two iterations under GRX_PPO_GRAPH=1 and 0 from the same seed: parameters and Adam state bit for bit after each
    iteration; on the way, sum_k r_k before the bootstrap against the env's own reward, within the rounding of an fp32 sum of NT terms"""
    from wiki_grx_gym_amd import _capi
    M = _M()
    got = {}
    for graph in ("1", "0"):
        monkeypatch.setenv("GRX_PPO_GRAPH", graph)
        env, runner = _make(tmp_path / graph)
        alg, mc = runner.alg, runner.alg.multi_critic
        assert mc.K == 2 and alg._use_graph == (graph == "1") and alg.actor_critic.num_critic_output == 2
        store, checked = mc.store, []

        def store_and_check(step, values, time_outs, gamma):
            out = store(step, values, time_outs, gamma)
            terms = env._sim.tensor("REWARD_TERMS")
            sums = torch.zeros_like(values)
            M.mc_store_hip(terms, None, mc.term_group[:_capi.NUM_REWARD_TERMS], values, None, gamma, torch.zeros_like(values), sums)
            bound = terms.double().abs().sum(0) * _capi.NUM_REWARD_TERMS * 2.0 ** -24   # an fp32 sum of NT terms, in any order
            err = (sums.double().sum(1) - env.rew_buf.double()).abs()
            checked.append(bool((err <= bound).all()))
            return out
        if graph == "1":
            mc.store = store_and_check
        states = []
        for it in range(2):
            runner.learn(num_learning_iterations=1)
            torch.cuda.synchronize()
            states.append(_state(alg))
        if graph == "1":
            assert isinstance(alg._graph, torch.cuda.CUDAGraph) and alg._act_fused
            assert len(checked) == 16 and all(checked)
            assert alg._static[3].shape == (128, 2) and alg._static[5].shape == (128, 2)
        assert all(bool(torch.isfinite(t).all()) for t in states[-1])
        got[graph] = states
    for it in range(2):
        assert all(torch.equal(a, b) for a, b in zip(got["1"][it], got["0"][it])), it
    assert not all(torch.equal(a, b) for a, b in zip(got["1"][0], got["1"][1]))


def test_fused_against_the_torch_spelling_on_the_first_rollout(tmp_path, monkeypatch, parity):
    """the same first rollout (same seed, same initial policy) with the three entries and with GRX_MC_FUSED=0: the stored heads' values and
    group rewards bit for bit, the advantages within the margin over the spelling's own float64 error"""
    got = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("GRX_MC_FUSED", fused)
        env, runner = _make(None)
        alg = runner.alg
        assert alg._use_graph == (fused == "1")
        snap = {}
        update = alg.update

        def snap_then_update():
            mc, st = alg.multi_critic, alg.storage
            snap.update(values=mc.values.clone(), rewards=mc.rewards.clone(), returns=mc.returns.clone(), adv=st.advantages.clone(),
                        dones=st.dones.clone(), stats=mc.stats.clone())
            return update()
        alg.update = snap_then_update
        compute = alg.multi_critic.compute_returns

        def keep_last(storage, last_values, gamma, lam):
            snap["last"] = last_values.detach().clone()
            return compute(storage, last_values, gamma, lam)
        alg.multi_critic.compute_returns = keep_last
        runner.learn(num_learning_iterations=1)
        torch.cuda.synchronize()
        got[fused] = {k: v.cpu() for k, v in snap.items()}
    a, b = got["1"], got["0"]
    assert torch.equal(a["values"], b["values"]) and torch.equal(a["rewards"], b["rewards"]) and torch.equal(a["returns"], b["returns"])
    ref = R.returns(a["rewards"].numpy(), a["values"].numpy(), a["dones"].squeeze(-1).numpy(), a["last"].numpy(), [1.0, 1.0], alg.gamma, alg.lam)
    _hold(parity, "runner,8x64x2", "advantages", a["adv"].squeeze(-1), b["adv"].squeeze(-1), ref["advantages"])
    for k in range(2):
        _hold(parity, "runner,8x64x2", f"std_{k}", a["stats"][k, 1], b["stats"][k, 1], ref["stats"][k, 1])


def test_train_save_load_play_and_export(tmp_path, monkeypatch):
    from wiki_grx_gym_amd.scripts.play import play
    from wiki_grx_gym_amd.utils import get_args
    _, runner = _make(tmp_path)
    runner.learn(num_learning_iterations=2)
    tags = {}
    for line in open(os.path.join(runner.log_dir, "scalars.jsonl")):
        tags.setdefault(line.split('"tag": "')[1].split('"')[0], []).append(float(line.split('"value": ')[1].split(",")[0]))
    for name in ("track", "rest"):
        assert len(tags["Loss/value_function_" + name]) == 2 and all(np.isfinite(x) and x > 0 for x in tags["Train/adv_std_" + name])
    assert tags["Loss/value_function"][1] == pytest.approx(tags["Loss/value_function_track"][1] + tags["Loss/value_function_rest"][1], rel=1e-4)
    ck = torch.load(os.path.join(runner.log_dir, "model_2.pt"), weights_only=False)
    assert set(ck) == {"model_state_dict", "optimizer_state_dict", "iter", "infos", "multi_critic"}
    assert ck["multi_critic"] == runner.multi_critic and ck["model_state_dict"]["critic.model.6.weight"].shape[0] == 2
    _, again = _make(None)
    again.load(os.path.join(runner.log_dir, "model_2.pt"))
    assert all(torch.equal(v, again.alg.actor_critic.state_dict()[k]) for k, v in ck["model_state_dict"].items() if k != "std")
    _, plain = _make(None, flags=())
    with pytest.raises(ValueError, match="--reward_groups"):
        plain.load(os.path.join(runner.log_dir, "model_2.pt"))
    out = play(get_args(["--task", "GR1T1", "--headless", "--seed", "3"]), steps=10, log_root=str(tmp_path))   # no flag: the actor alone
    prunner, penv = out["runner"], out["env"]
    assert prunner.alg.multi_critic is None and len(open(out["states"]).readlines()) == 10
    loaded = prunner.alg.actor_critic.state_dict()
    assert all(torch.equal(v.to(loaded[k].device), loaded[k]) for k, v in ck["model_state_dict"].items() if k.startswith("actor."))
    frames = penv.get_observations().detach().clone()
    jit = torch.jit.load(out["exported"])
    with torch.no_grad():
        want = prunner.alg.actor_critic.actor.model(frames).cpu()
        assert torch.allclose(jit(frames.cpu()), want, atol=1e-5, rtol=1e-5)


def test_the_second_term_table(tmp_path):
    """GR1T1_full_body with three of legged_gym's base terms switched on: a group of base terms alone, one iteration"""
    from wiki_grx_gym_amd import _capi
    from wiki_grx_gym_amd.envs import GR1T1FullBodyCfg
    cfg = GR1T1FullBodyCfg()
    for n, v in (("torques", -1e-5), ("tracking_lin_vel", 1.0), ("action_rate", -0.01)):
        setattr(cfg.rewards.scales, n, v)
    env, runner = _make(tmp_path, flags=("--reward_groups", "base=torques,tracking_lin_vel,action_rate;rest=*", "--reward_group_weights", "2,1"),
                        task="GR1T1_full_body", cfg=cfg)
    mc = runner.alg.multi_critic
    assert mc.base_terms is not None and mc.base_terms.shape == (_capi.NUM_BASE_REWARD_TERMS, 64) and mc.groups.uses_base
    assert mc.groups.terms["base"] == ["action_rate", "torques", "tracking_lin_vel"]
    runner.learn(num_learning_iterations=1)
    torch.cuda.synchronize()
    base = env._sim.tensor("BASE_REWARD_TERMS")
    rows = [_capi.BASE_REWARD_TERMS.index(n) for n in mc.groups.terms["base"]]
    assert bool(torch.isfinite(mc.rewards).all()) and float(mc.rewards[..., 0].abs().max()) > 0
    assert float(base[rows].abs().max()) > 0
    assert all(bool(torch.isfinite(p).all()) for p in runner.alg.actor_critic.parameters())


def test_default_run_is_what_it_was_and_launches_nothing_new(tmp_path, monkeypatch):
    """two iterations without the flag, against the same run whose policy and PPO get the new keywords at their defaults: parameters bit for
    bit, and the grx_mc_* prototypes are never bound"""
    import wiki_grx_gym_amd.rl.runner as RR
    M = _M()
    monkeypatch.setattr(M, "_BOUND", None)
    _, first = _make(tmp_path / "a", flags=(), publish=False)
    first.learn(num_learning_iterations=2)
    plain_policy, plain_ppo = RR._POLICIES["ActorCriticMLP"], RR._ALGORITHMS["PPO"]
    monkeypatch.setitem(RR._POLICIES, "ActorCriticMLP", lambda *a, **k: plain_policy(*a, num_critic_outputs=1, **k))
    monkeypatch.setitem(RR._POLICIES, "ActorCritic", lambda *a, **k: plain_policy(*a, num_critic_outputs=1, **k))
    monkeypatch.setitem(RR._ALGORITHMS, "PPO", lambda **k: plain_ppo(reward_groups=None, reward_group_weights=None, **k))
    _, second = _make(tmp_path / "b", flags=(), publish=False)
    second.learn(num_learning_iterations=2)
    torch.cuda.synchronize()
    assert first.alg.multi_critic is None and second.alg.multi_critic is None and M._BOUND is None
    assert all(torch.equal(a, b) for a, b in zip(_state(first.alg), _state(second.alg)))
    ck = torch.load(os.path.join(first.log_dir, "model_2.pt"), weights_only=False)
    assert set(ck) == {"model_state_dict", "optimizer_state_dict", "iter", "infos"}
