"""The context-aided estimator network on the MI355X (rl/cenet.py, csrc/grx_ppo_cenet.hip): grx_cenet_head's exact copies,
its z bit for bit against grx_cenet_reparam and its row independence; grx_cenet_loss and the reparameterisation pair against the float64
reference (tests/cenet_ref.py), held to 4 x the error of the fp32 torch spelling of the same formulas on the CPU; repeatability, rejected
calls, the fused path against GRX_CENET_FUSED=0 through the runner, the runner end to end through the HIP env, play and the exported
module, and the untouched default path.

GRX_CENET_PARITY_JSON=<path>: the parity tests also write their per-case error ratios there (profiles/cenet_parity.json is such a file)."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests import cenet_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 4.0           # tests/test_recurrent_gpu.py's and tests/test_estimator_gpu.py's: another, equally good fp32 evaluation
U = 2.0 ** -24
EZ = [(1, 1), (3, 16), (8, 64)]
CANARY = 777.0


def _M():
    from wiki_grx_gym_amd.rl import cenet
    return cenet


def held(got, fp32_torch, want):
    """(error, e32, ratio) of `got` against the float64 `want`; e32 is the error of the fp32 torch spelling on the CPU against the same
    float64 values, max |.| over the tensor, and counts as at least half an fp32 ulp of the reference's largest magnitude (no fp32
    evaluation is asked to be better than its own output rounding: tests/mc_ref.py held()).  NaNs must sit in the same places."""
    got, ref32, want = (np.asarray(a, np.float64) for a in (got, fp32_torch, want))
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(np.isnan(ref32), nan), "NaNs differ"
    if nan.all():
        return 0.0, 0.0, 0.0
    floor = U * float(np.abs(want[~nan]).max())
    e32 = max(float(np.abs(ref32 - want)[~nan].max()), floor)
    err = float(np.abs(got - want)[~nan].max())
    return err, e32, (err / e32 if e32 > 0 else 0.0)


@pytest.fixture(scope="module")
def parity():
    rows = {}
    yield rows
    path = os.environ.get("GRX_CENET_PARITY_JSON")
    if path and rows:
        with open(path, "w") as f:
            json.dump({"margin": MARGIN, "what": "max |kernel - float64| over the tensor, divided by e32 = max |the fp32 torch spelling on the CPU "
                       "- float64| of the same formulas (at least 2^-24 max |float64|); per key the case of the largest ratio", "cases": rows}, f, indent=1)


def _hold(parity, key, got, spelled, want):
    err, e32, ratio = held(got.detach().cpu().double().numpy(), spelled.detach().double().numpy(), want)
    if ratio >= parity.get(key, {"ratio": -1.0})["ratio"]:
        parity[key] = {"e32": e32, "error": err, "ratio": round(ratio, 3)}
    assert err <= MARGIN * e32, (key, err, e32, ratio)


def _enc_out(g, mb, E, Z):
    """an encoder output whose raw columns lie below -10, inside and above 2"""
    e = torch.randn(mb, E + 2 * Z, generator=g)
    e[:, E + Z:] *= 6.0
    e[0, E + Z] = -11.5
    e[-1, -1] = 2.75
    return e


# ---- grx_cenet_head ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,Z", EZ)
@pytest.mark.parametrize("D", [39, 40, 195])
def test_head_copies_exactly_and_its_z_is_the_reparameterisation_bit_for_bit(D, E, Z, parity):
    """N = 1, one short of and one past 64, and 130 (33 passes of four rows, the last one short); D = 40 with (E, Z) = (8, 64) takes the
    dwordx4 copy (D and D + E + Z are multiples of four), every other shape the dword copy"""
    M = _M()
    for N in (1, 63, 65, 130):
        g = torch.Generator().manual_seed(1000 * N + 7 * D + E + Z)
        x, pri = 1.5 * torch.randn(N, D, generator=g), torch.randn(N, D + 13, generator=g)
        enc, eps = _enc_out(g, N, E, Z), torch.randn(N, Z, generator=g)
        cols = [int(c) for c in torch.randperm(D + 13, generator=g)[:E]]
        xd, prid, encd, epsd = x.to(DEV), pri.to(DEV), enc.to(DEV), eps.to(DEV)
        out, tg = M.head_hip(xd, encd, epsd, E, Z, prid, cols)
        assert out.shape == (N, D + E + Z) and tg.shape == (N, E)
        assert torch.equal(out[:, :D], xd) and torch.equal(out[:, D:D + E], encd[:, :E]) and torch.equal(tg, prid[:, cols]), (N, "copies")
        dec_in = M.Reparam.apply(encd, epsd, E, Z)
        assert torch.equal(out[:, D:], dec_in), (N, "z")
        ref, _ = R.head_ref(x.numpy(), enc.numpy(), eps.numpy(), E, Z)
        spelled, _ = M.head_torch(x, enc, eps, E, Z)
        _hold(parity, f"head,E{E},Z{Z}", out[:, D + E:], spelled[:, D + E:], ref[:, D + E:])
        if N == 130:
            for r in (0, 1, 3, 4, 63, 64, 127, 128, 129):   # a row's result does not depend on N
                one, otg = M.head_hip(xd[r:r + 1].contiguous(), encd[r:r + 1].contiguous(), epsd[r:r + 1].contiguous(), E, Z,
                                      prid[r:r + 1].contiguous(), cols)
                assert torch.equal(one[0], out[r]) and torch.equal(otg[0], tg[r]), r
            again, _ = M.head_hip(xd, encd, epsd, E, Z, prid, cols)
            none, ntg = M.head_hip(xd, encd, epsd, E, Z)
            assert torch.equal(again, out) and torch.equal(none, out) and ntg is None


# ---- grx_cenet_loss and the reparameterisation pair ---------------------------------------------------------------------------------------------
def _valid(which, mb):
    return {"all": np.ones(mb, np.uint8), "none": np.zeros(mb, np.uint8), "mixed": (np.arange(mb) % 3 != 1).astype(np.uint8)}[which]


@pytest.mark.parametrize("E,Z", EZ)
@pytest.mark.parametrize("mb", [1, 63, 65, 2049])
def test_loss_and_reparam_against_float64(mb, E, Z, parity):
    """F in {1, 39, 45} x valid all / none / mixed; the successor block is read in place with a leading dimension and an offset, and holds a
    NaN in every invalid row.  Every output is held on its own to MARGIN x the fp32 torch spelling's error on the CPU"""
    M = _M()
    beta = 0.7
    for F in (1, 39, 45):
        for which in ("all", "none", "mixed"):
            g = torch.Generator().manual_seed(100 * mb + 10 * F + E + Z + len(which))
            off = 3
            valid = _valid(which, mb)
            enc, y, dec = _enc_out(g, mb, E, Z), torch.randn(mb, E, generator=g), torch.randn(mb, F, generator=g)
            succ = torch.randn(mb, off + F + 2, generator=g)
            succ[torch.from_numpy(valid == 0)] = float("nan")
            eps, d_in = torch.randn(mb, Z, generator=g), torch.randn(mb, E + Z, generator=g)
            # the fp32 torch spelling on the CPU, and float64
            e32, d32 = enc.clone().requires_grad_(), dec.clone().requires_grad_()
            total32, out32 = M.loss_torch(e32, y, d32, succ, off, torch.from_numpy(valid), beta, E, Z)
            total32.backward()
            ref, d_enc, d_dec = R.loss_ref(enc.numpy(), y.numpy(), dec.numpy(), succ[:, off:off + F].numpy(), valid, beta, E, Z)
            r32 = enc.clone().requires_grad_()
            di32 = M.reparam_torch(r32, eps, E, Z)
            di32.backward(d_in)
            # the kernels
            ed, dd = enc.to(DEV).requires_grad_(), dec.to(DEV).requires_grad_()
            total, out = M.cenet_loss(ed, y.to(DEV), dd, succ.to(DEV), off, torch.from_numpy(valid).to(DEV), beta, E, Z)
            assert total.grad_fn is not None and type(total.grad_fn).__name__.startswith("Loss")
            total.backward()
            rd = enc.to(DEV).requires_grad_()
            di = M.reparam(rd, eps.to(DEV), E, Z)
            di.backward(d_in.to(DEV))
            case = f"E{E},Z{Z}"
            for i, name in enumerate(("L_est", "L_rec", "L_kl", "L")):
                _hold(parity, f"loss,{name},{case}", out[i], out32[i], ref[i])
            assert float(out[4]) == float(valid.sum()) and float(total.detach()) == float(out[3])
            _hold(parity, f"loss,d_enc_out,{case}", ed.grad, e32.grad, d_enc)
            _hold(parity, f"loss,d_dec,{case}", dd.grad, d32.grad, d_dec)
            _hold(parity, f"reparam,dec_in,{case}", di, di32, R.reparam_ref(enc.numpy(), eps.numpy(), E, Z))
            _hold(parity, f"reparam,d_enc_out,{case}", rd.grad, r32.grad, R.reparam_backward_ref(enc.numpy(), eps.numpy(), d_in.numpy(), E, Z))
            assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(ed.grad).all()) and bool(torch.isfinite(dd.grad).all())   # no NaN got out
            bad = torch.from_numpy(valid == 0).to(DEV)
            assert bool((dd.grad[bad] == 0).all()) and not bool(torch.signbit(dd.grad[bad]).any())        # exactly +0
            assert float(ed.grad[0, E + Z]) == 0.0 and float(ed.grad[-1, -1]) == 0.0 and float(rd.grad[0, E + Z]) == 0.0 and float(rd.grad[-1, -1]) == 0.0
            assert torch.equal(rd.grad[:, :E + Z], d_in.to(DEV))                                          # d v_hat and d mu pass
            if which == "none":
                assert float(out[1]) == 0.0 and bool((dd.grad == 0).all())


def test_the_same_call_gives_the_same_bytes():
    """mb = 2049: 118 blocks of partial sums for the loss, two blocks and more for every other launch"""
    M = _M()
    mb, E, Z, F, off = 2049, 8, 64, 45, 150
    g = torch.Generator().manual_seed(9)
    enc, y, dec = _enc_out(g, mb, E, Z).to(DEV), torch.randn(mb, E, generator=g).to(DEV), torch.randn(mb, F, generator=g).to(DEV)
    succ, eps = torch.randn(mb, off + F + E + Z, generator=g).to(DEV), torch.randn(mb, Z, generator=g).to(DEV)
    valid = torch.from_numpy(_valid("mixed", mb)).to(DEV)
    assert M.load_library().grx_cenet_loss_partials_size(mb, E, Z, F) == 8 * 118
    runs = []
    for _ in range(2):
        e, d = enc.clone().requires_grad_(), dec.clone().requires_grad_()
        total, out = M.cenet_loss(e, y, d, succ, off, valid, 1.0, E, Z)
        total.backward()
        r = enc.clone().requires_grad_()
        di = M.reparam(r, eps, E, Z)
        di.sum().backward()
        runs.append([out, e.grad, d.grad, di.detach(), r.grad])
    for a, b in zip(*runs):
        assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_rejected_calls_write_nothing():
    M = _M()
    lib = M.load_library()
    N, D, E, Z, F, P = 65, 40, 3, 16, 39, 53
    g = torch.Generator().manual_seed(4)
    x, enc, eps, pri = (torch.randn(N, w, generator=g).to(DEV) for w in (D, E + 2 * Z, Z, P))
    y, dec, succ = (torch.randn(N, w, generator=g).to(DEV) for w in (E, F, D + E + Z))
    valid = torch.ones(N, dtype=torch.uint8, device=DEV)
    full = lambda *s: torch.full(s, CANARY, device=DEV)
    out, tg, dec_in, d_enc, lo, d_dec = full(N, D + E + Z), full(N, E), full(N, E + Z), full(N, E + 2 * Z), full(5), full(N, F)
    part = full(lib.grx_cenet_loss_partials_size(N, E, Z, F))
    cols = (C.c_int * E)(40, 41, 42)
    p = lambda t: t.data_ptr()

    def head(N=N, D=D, E=E, Z=Z, x=p(x), enc=p(enc), eps=p(eps), P=P, pri=p(pri), cols=cols, out=p(out), tg=p(tg)):
        return lib.grx_cenet_head(N, D, E, Z, x, enc, eps, P, pri, cols, out, tg, None)
    assert head(N=0) < 0 and head(D=0) < 0 and head(D=2049) < 0 and head(E=0) < 0 and head(E=9) < 0 and head(Z=0) < 0 and head(Z=65) < 0
    assert head(x=None) < 0 and head(enc=None) < 0 and head(eps=None) < 0 and head(out=None) < 0
    assert head(P=0) < 0 and head(cols=None) < 0 and head(cols=(C.c_int * E)(0, 1, P)) < 0 and head(cols=(C.c_int * E)(-1, 1, 2)) < 0
    assert head(out=p(x)) < 0 and head(out=p(x) + 4 * (N * D - 1)) < 0 and head(out=p(enc)) < 0 and head(out=p(eps)) < 0

    def rep(mb=N, E=E, Z=Z, enc=p(enc), eps=p(eps), o=p(dec_in)):
        return lib.grx_cenet_reparam(mb, E, Z, enc, eps, o, None)

    def repb(mb=N, E=E, Z=Z, enc=p(enc), eps=p(eps), d=p(dec_in), o=p(d_enc)):
        return lib.grx_cenet_reparam_backward(mb, E, Z, enc, eps, d, o, None)
    assert rep(mb=0) < 0 and rep(E=9) < 0 and rep(Z=65) < 0 and rep(enc=None) < 0 and rep(eps=None) < 0 and rep(o=None) < 0
    assert repb(mb=0) < 0 and repb(E=0) < 0 and repb(Z=0) < 0 and repb(enc=None) < 0 and repb(eps=None) < 0 and repb(d=None) < 0 and repb(o=None) < 0

    def loss(mb=N, E=E, Z=Z, F=F, enc=p(enc), y=p(y), dec=p(dec), nxt=p(succ), ld=D + E + Z, off=D - F, valid=p(valid), beta=1.0, o=p(lo),
             de=p(d_enc), dd=p(d_dec), part=p(part)):
        return lib.grx_cenet_loss(mb, E, Z, F, enc, y, dec, nxt, ld, off, valid, beta, o, de, dd, part, None)
    assert loss(mb=0) < 0 and loss(mb=1 << 24) < 0 and loss(E=9) < 0 and loss(Z=65) < 0 and loss(F=0) < 0 and loss(F=2049) < 0
    assert loss(off=-1) < 0 and loss(ld=F - 1) < 0 and loss(off=D + E + Z - F + 1) < 0 and loss(beta=-1.0) < 0 and loss(beta=float("nan")) < 0
    for k in ("enc", "y", "dec", "nxt", "valid", "o", "de", "dd", "part"):
        assert loss(**{k: None}) < 0, k
    assert loss(part=p(part) + 4) < 0
    torch.cuda.synchronize()
    for t in (out, tg, dec_in, d_enc, lo, d_dec, part):
        assert bool((t == CANARY).all())
    assert head(pri=None) == 0                                                                     # no privileged frame: no targets
    torch.cuda.synchronize()
    assert bool((tg == CANARY).all()) and not bool((out == CANARY).any())
    assert head() == 0 and rep() == 0 and loss() == 0
    torch.cuda.synchronize()
    assert torch.equal(tg, pri[:, 40:43]) and not bool((dec_in == CANARY).any()) and not bool((lo == CANARY).any())
    assert not bool((d_dec == CANARY).any()) and not bool((d_enc == CANARY).any())


# ---- the runner through the HIP env ------------------------------------------------------------------------------------------------------------
def _make(tmp_path, flags=(), steps=8, num_envs=64):
    from wiki_grx_gym_amd.envs import GR1T1Cfg, GR1T1CfgPPO
    from wiki_grx_gym_amd.utils import get_args, task_registry
    args = get_args(["--task", "GR1T1", "--headless", "--num_envs", str(num_envs), "--seed", "3", *flags])
    env, _ = task_registry.make_env("GR1T1", args=args, env_cfg=GR1T1Cfg())   # (the registered GR1T1 task: flat terrain)
    tcfg = GR1T1CfgPPO()
    tcfg.runner.num_steps_per_env = steps
    tcfg.algorithm.num_mini_batches = 4
    runner, _ = task_registry.make_alg_runner(env, name=None, args=args, train_cfg=tcfg, log_root=str(tmp_path) if tmp_path else None)
    return env, runner


def _tags(runner):
    out = {}
    for line in open(os.path.join(runner.log_dir, "scalars.jsonl")):
        out.setdefault(line.split('"tag": "')[1].split('"')[0], []).append(float(line.split('"value": ')[1].split(",")[0]))
    return out


def _lin(net):
    mods = [m for m in net.model if isinstance(m, torch.nn.Linear)]
    return [m.weight.detach().double().cpu().numpy() for m in mods], [m.bias.detach().double().cpu().numpy() for m in mods]


def test_the_fused_path_against_the_torch_spelling_through_the_runner(monkeypatch, parity):
    """64 GR1T1 envs, T = 8, all four targets.  A fused runner collects and trains one iteration; a GRX_CENET_FUSED=0 runner is given its
    networks.  On the rows the fused runner stored, both take the rollout's step and one whole-rollout minibatch step with the same eps:
    the copies are bit-equal, and z, the five loss figures and the gradient of every weight and bias are held, fused against float64, to
    MARGIN x the unfused path's own error"""
    M = _M()
    flags = ("--cenet", "--cenet_targets", "lin_vel,base_height,feet_contact,feet_height")
    monkeypatch.setenv("GRX_CENET_FUSED", "1")
    env, fused = _make(None, flags)
    fused.learn(num_learning_iterations=1)
    monkeypatch.setenv("GRX_CENET_FUSED", "0")
    _, plain = _make(None, flags)
    a, b = fused.cenet, plain.cenet
    assert a._fused and not b._fused and isinstance(fused.alg._graph, torch.cuda.CUDAGraph)
    b.load_state_dict(a.state_dict())
    D, E, Z, F = 39, 8, 16, 39
    rows, dones = fused.alg.storage.observations, fused.alg.storage.dones
    assert rows.shape == (8, 64, D + E + Z) and bool((rows[:, :, D:] != 0).any()) and bool((a.targets != 0).any())
    # the rollout's step on the stored inputs
    x = rows[3, :, :D].contiguous()
    pri = torch.randn(64, env.num_pri_obs, device=DEV)
    outs = []
    for net in (a, b):
        torch.manual_seed(11)
        outs.append((net.step(x, pri, 2).clone(), net.targets[2].clone(), net.eps.clone()))
    (oa, ta, ea), (ob, tb, eb) = outs
    assert torch.equal(ea, eb) and torch.equal(ta, tb) and torch.equal(ta, pri[:, 39:47]) and torch.equal(oa[:, :D + E], ob[:, :D + E])
    with torch.no_grad():
        enc = M._embed(a.encoder, x)
    ref, _ = R.head_ref(x.double().cpu().numpy(), enc.double().cpu().numpy(), ea.double().cpu().numpy(), E, Z)
    _hold(parity, "runner,z", oa[:, D + E:], ob[:, D + E:].cpu(), ref[:, D + E:])
    # one minibatch step over the whole rollout
    n = 8 * 64
    idx = torch.arange(n, device=DEV)
    flat, tg, d8 = rows.flatten(0, 1), a.targets.flatten(0, 1), dones.reshape(-1)
    valid = M.valid_rows(idx, 64, 8, d8)
    succ = flat.index_select(0, torch.where(valid, idx + 64, idx)).clone()
    succ[~valid] = float("nan")
    eps = torch.randn(n, Z, device=DEV)
    grads = []
    for net in (a, b):
        net.optimizer.zero_grad(set_to_none=False)
        loss, out = net._loss(flat[:, :D].contiguous(), tg.contiguous(), succ, D - F, valid.to(torch.uint8), eps)
        loss.backward()
        grads.append((out.detach().clone(), [p.grad.detach().clone() for p in net._params]))
    want = R.step_ref(*_lin(a.encoder), *_lin(a.decoder), flat[:, :D].double().cpu().numpy(), tg.double().cpu().numpy(),
                      succ[:, D - F:D].double().cpu().numpy(), valid.cpu().numpy(), eps.double().cpu().numpy(), a.beta, E, Z)
    (out_a, ga), (out_b, gb) = grads
    for i, name in enumerate(("L_est", "L_rec", "L_kl", "L")):
        _hold(parity, f"runner,{name}", out_a[i], out_b[i].cpu(), want[0][i])
    assert float(out_a[4]) == float(valid.sum()) == float(out_b[4]) and 0 < float(valid.sum()) < n
    flat_want = [w for pair in zip(want[1], want[2]) for w in pair] + [w for pair in zip(want[3], want[4]) for w in pair]   # (weight, bias) per layer
    assert len(flat_want) == len(ga)
    for i, (g1, g2, w) in enumerate(zip(ga, gb, flat_want)):
        _hold(parity, f"runner,grad{i}", g1, g2.cpu(), w)


def test_runner_trains_saves_plays_and_exports(tmp_path, monkeypatch):
    from wiki_grx_gym_amd.scripts.play import play
    from wiki_grx_gym_amd.utils import get_args, task_registry
    # (play() takes the registered config instance, which the flags write to: undone when the test ends)
    reg = task_registry.train_cfgs["GR1T1"].runner
    for name, value in (("obs_history_length", 1), ("empirical_normalization", False), ("cenet", False), ("cenet_targets", "lin_vel"),
                        ("cenet_latent_dim", 16), ("cenet_beta", 1.0), ("cenet_encoder_dims", [128, 64]), ("cenet_decoder_dims", [64, 128]),
                        ("cenet_learning_rate", 1e-3), ("cenet_num_epochs", 1)):
        monkeypatch.setattr(reg, name, value, raising=False)
    flags = ("--cenet", "--obs_history", "3", "--empirical_normalization")
    env, runner = _make(tmp_path, flags)
    net = runner.cenet
    before = [p.detach().clone() for p in net.parameters()]
    runner.learn(num_learning_iterations=2)
    tags = _tags(runner)
    for name in ("Loss/cenet_estimation", "Loss/cenet_reconstruction", "Loss/cenet_kl"):
        assert len(tags[name]) == 2 and all(np.isfinite(v) and v > 0 for v in tags[name]), name
    assert all(not torch.equal(a, b) and bool(torch.isfinite(b).all()) for a, b in zip(before, net.parameters()))
    assert runner.alg.storage.observations.shape == (8, 64, 117 + 3 + 16) and runner.obs_normalizer.dim == 117
    assert isinstance(runner.alg._graph, torch.cuda.CUDAGraph) and type(runner.alg._gather).__name__ == "RowGather"   # PPO's captured step is what it was
    ck = torch.load(os.path.join(runner.log_dir, "model_2.pt"), weights_only=False)
    assert set(ck) == {"model_state_dict", "optimizer_state_dict", "iter", "infos", "obs_norm_state_dict", "critic_obs_norm_state_dict", "obs_history",
                       "cenet"}
    with pytest.raises(ValueError, match="pass --cenet --cenet_targets lin_vel --cenet_latent_dim 16 --cenet_encoder_dims 128 64 --cenet_decoder_dims 64 128"):
        play(get_args(["--task", "GR1T1", "--headless", "--seed", "3", "--obs_history", "3", "--empirical_normalization"]), steps=2, log_root=str(tmp_path))
    out = play(get_args(["--task", "GR1T1", "--headless", "--seed", "3", *flags]), steps=10, log_root=str(tmp_path))
    prunner, penv = out["runner"], out["env"]
    assert len(open(out["states"]).readlines()) == 10 and prunner.current_learning_iteration == 2
    sd, sd2 = net.state_dict(), prunner.cenet.state_dict()
    assert all(torch.equal(sd[k], sd2[k]) for k in sd)
    jit = torch.jit.load(out["exported"])
    policy = prunner.get_inference_policy(device=penv.device)
    # raw single frames OF THE ENV, the rows of (drawn) ended envs refilled.  Not N(0, 1) frames: the fitted normaliser turns those into
    # inputs of 150 standard deviations, at which two fp32 evaluations of one network -- this pipeline's or --estimator's -- each sit 1e-6
    # from a float64 evaluation (measured: device - exported 1.5e-6 / 1.1e-6 on such frames, 2.1e-7 / 1.8e-7 on the env's, inputs below 5)
    g = torch.Generator().manual_seed(5)
    frame = penv.get_observations().clone()
    for i in range(6):
        if i:
            dones = (torch.rand(50, generator=g) < 0.3).long()
            policy.reset(dones.to(penv.device)); jit.reset(dones)
        with torch.no_grad():
            want, got = policy(frame).cpu(), jit(frame.cpu())
        assert want.shape == got.shape == (50, penv.num_actions) and float((got - want).abs().max()) < 1e-6, i
        frame = penv.step(want.to(penv.device))[0].clone()


def _two_plain_iterations():
    torch.manual_seed(0)
    _, plain = _make(None)
    plain.learn(num_learning_iterations=2)
    assert plain.cenet is None and isinstance(plain.alg._graph, torch.cuda.CUDAGraph)
    return [p.detach().clone() for p in plain.alg.actor_critic.parameters()]


def test_default_path_is_unchanged(monkeypatch):
    """without the flag, two iterations give the same parameters whether rl/cenet.py can be imported or not: nothing of it runs"""
    first = _two_plain_iterations()
    monkeypatch.delitem(sys.modules, "wiki_grx_gym_amd.rl.cenet", raising=False)
    monkeypatch.setitem(sys.modules, "wiki_grx_gym_amd.rl.cenet", None)       # `import wiki_grx_gym_amd.rl.cenet` raises ImportError from here on
    with pytest.raises(ImportError):
        import wiki_grx_gym_amd.rl.cenet  # noqa: F401
    second = _two_plain_iterations()
    assert len(first) == len(second) and all(torch.equal(a, b) and bool(torch.isfinite(a).all()) for a, b in zip(first, second))
