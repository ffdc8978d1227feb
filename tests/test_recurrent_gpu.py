"""The recurrent actor-critic on the GPU (include/grx_ppo.h grx_lstm_cell / grx_lstm_cell_backward, rl/recurrent.py):
the cell against float64 at the smallest shapes where it can go wrong, row independence, exact integer arithmetic through the f32 MFMA,
the element-wise backward, the argument checks with canaries, LSTMSequence's gradients against float64 and against GRX_LSTM_FUSED=0, the
rollout / update contract on a real GR1T1 rollout (bit for bit), train / save / load / play / export, and the default path.

GRX_LSTM_PARITY_JSON=<path>: the cell test also writes its per-case error ratios there (profiles/lstm_parity.json is such a file)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import lstm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 4.0     # the cell against float64: within 4 x the error of the same cell evaluated in float32 by torch on the CPU


def _L():
    from wiki_grx_gym_amd.rl import recurrent
    return recurrent


def _dev(a):
    return torch.as_tensor(a).to(DEV)


@functools.lru_cache(maxsize=None)
def _rnn(D, H):
    torch.manual_seed(100 * D + H)
    return torch.nn.LSTM(D, H, 1)


@functools.lru_cache(maxsize=None)
def _cell_case(M, D, H, with_reset):
    """inputs, the float64 result, e32 = max |float32 on the CPU - float64| over h and c, and the same over the saved activations --
    computed once per shape"""
    L = _L()
    rnn = _rnn(D, H)
    p = R.params64(rnn)
    x, h, c, reset = R.cell_inputs(M, D, H)
    reset = reset if with_reset else None
    t = lambda a, dt: torch.tensor(a).to(dt)
    rs = torch.tensor(reset) if with_reset else None
    want_h, want_c = R.cell64(p, x, h, c, reset)
    acts64 = L.lstm_cell_torch(t(x, torch.float64), t(h, torch.float64), t(c, torch.float64), rs, *[p[k] for k in R.NAMES])[2]
    with torch.no_grad():
        h32, c32, a32 = L.lstm_cell_torch(t(x, torch.float32), t(h, torch.float32), t(c, torch.float32), rs, *[getattr(rnn, k) for k in R.NAMES])
    e32 = max(float((h32.double() - want_h).abs().max()), float((c32.double() - want_c).abs().max()))
    return (x, h, c, reset), (want_h, want_c, acts64), (e32, float((a32.double() - acts64).abs().max()))


@pytest.fixture(scope="module")
def parity():
    rows = {}
    yield rows
    path = os.environ.get("GRX_LSTM_PARITY_JSON")
    if path and rows:
        with open(path, "w") as f:
            json.dump({"margin": MARGIN, "what": "max |grx_lstm_cell - float64| over h and c, divided by e32 = max |torch float32 on the CPU - "
                       "float64| of the same cell; case = M x D x H, reset, acts", "cases": rows}, f, indent=1)


def _weights(D, H):
    return [getattr(_rnn(D, H), k).detach().to(DEV) for k in R.NAMES]


@pytest.mark.parametrize("acts", [False, True], ids=["no_acts", "acts"])
@pytest.mark.parametrize("with_reset", [False, True], ids=["plain", "reset"])
@pytest.mark.parametrize("H", [32, 96])
@pytest.mark.parametrize("D", [1, 45, 70])
@pytest.mark.parametrize("M", [1, 31, 33, 200])
def test_cell_against_float64(M, D, H, with_reset, acts, parity):
    L = _L()
    (x, h, c, reset), (want_h, want_c, acts64), (e32, e32_acts) = _cell_case(M, D, H, with_reset)
    hn, cn = torch.full((M, H), 777.0, device=DEV), torch.full((M, H), 777.0, device=DEV)
    a = torch.full((M, 5 * H), 777.0, device=DEV) if acts else None
    L.lstm_cell_hip(_dev(x), _dev(h), _dev(c), _dev(reset) if with_reset else None, *_weights(D, H), hn, cn, a)
    err = max(float((hn.cpu().double() - want_h).abs().max()), float((cn.cpu().double() - want_c).abs().max()))
    ratio = err / e32
    parity[f"{M}x{D}x{H},{'reset' if with_reset else 'plain'},{'acts' if acts else 'no_acts'}"] = {"e32": e32, "error": err, "ratio": round(ratio, 3)}
    print(f"grx_lstm_cell {M} x {D} x {H} reset={with_reset} acts={acts}: error {err:.3g}, e32 {e32:.3g}, ratio {ratio:.3g}")
    assert err <= MARGIN * e32, (err, e32, ratio)
    if acts:   # the saved activations, held to the same margin over THEIR float32 error (a reset row's c is small, its gates are not)
        got = a.cpu()
        err_acts = float((got.double() - acts64).abs().max())
        print(f"    saved activations: error {err_acts:.3g}, e32 {e32_acts:.3g}, ratio {err_acts / e32_acts:.3g}")
        assert err_acts <= MARGIN * e32_acts, (err_acts, e32_acts)
        assert torch.equal(got[:, 3 * H:4 * H] * got[:, 4 * H:], hn.cpu())


def test_a_row_does_not_depend_on_the_rows_beside_it():
    L = _L()
    M, D, H = 200, 45, 96
    x, h, c, reset = (_dev(a) for a in R.cell_inputs(M, D, H))
    w = _weights(D, H)
    hn, cn, an = torch.empty(M, H, device=DEV), torch.empty(M, H, device=DEV), torch.empty(M, 5 * H, device=DEV)
    L.lstm_cell_hip(x, h, c, reset, *w, hn, cn, an)
    for r in (0, 1, 31, 32, 127, 128, 198, 199):          # reset rows (r % 3 == 0) and others; the edges of a wave's and a block's rows
        h1, c1, a1 = torch.empty(1, H, device=DEV), torch.empty(1, H, device=DEV), torch.empty(1, 5 * H, device=DEV)
        L.lstm_cell_hip(x[r:r + 1].clone(), h[r:r + 1].clone(), c[r:r + 1].clone(), reset[r:r + 1].clone(), *w, h1, c1, a1)
        assert torch.equal(h1[0], hn[r]) and torch.equal(c1[0], cn[r]) and torch.equal(a1[0], an[r]), r


def _int_case(M, D, H, structured):
    g = np.random.default_rng(7)
    if structured:   # the guide's operand-order check: every operand a different function of (row, k) -- a swapped or permuted map changes G
        m, k, n = np.arange(M)[:, None], np.arange(max(D, H))[None, :], np.arange(4 * H)[:, None]
        x, hp = ((m + 3 * k[:, :D]) % 7 - 3), ((2 * m + k[:, :H]) % 5 - 2)
        wi, wh = ((2 * n + k[:, :D]) % 5 - 2), ((n + 5 * k[:, :H]) % 9 - 4)
        bi, bh = (np.arange(4 * H) % 11 - 5), (np.arange(4 * H) % 3 - 1)
    else:
        x, hp = g.integers(-8, 9, (M, D)), g.integers(-8, 9, (M, H))
        wi, wh = g.integers(-8, 9, (4 * H, D)), g.integers(-8, 9, (4 * H, H))
        bi, bh = g.integers(-8, 9, 4 * H), g.integers(-8, 9, 4 * H)
    return [np.asarray(a, dtype=np.int64) for a in (x, hp, wi, wh, bi, bh)]


@pytest.mark.parametrize("structured", [False, True], ids=["random", "structured"])
@pytest.mark.parametrize("M,D,H", [(33, 45, 96), (130, 70, 32), (5, 1, 64)])
def test_preactivations_are_exact_on_integers(M, D, H, structured):
    """small integers: every product and partial sum is an integer below 2^24 (at most (70 + 96) * 64 + 16), so float32 is exact and G must
    equal the int64 result -- whatever the summation order; a wrong MFMA operand map does not survive it"""
    L = _L()
    x, hp, wi, wh, bi, bh = _int_case(M, D, H, structured)
    reset = (np.arange(M) % 4 == 1).astype(np.uint8)
    want = x @ wi.T + (hp * (reset == 0)[:, None]) @ wh.T + bi + bh
    f = lambda a: _dev(a.astype(np.float32))
    got = L.lstm_preact_hip(f(x), f(hp), _dev(reset), f(wi), f(wh), f(bi), f(bh))
    assert np.array_equal(got.cpu().numpy().astype(np.int64), want) and np.abs(want).max() > 16
    got = L.lstm_preact_hip(f(x), f(hp), None, f(wi), f(wh), f(bi), f(bh))
    assert np.array_equal(got.cpu().numpy().astype(np.int64), x @ wi.T + hp @ wh.T + bi + bh)


@pytest.mark.parametrize("H", [32, 96])
@pytest.mark.parametrize("M", [1, 33])
def test_cell_backward_against_float64_autograd(M, H):
    """tolerance of tests/test_ppo_kernels_gpu.py::test_elu_backward_colsum_matches_float64: 2e-5 * max(|ref|, 1)"""
    L = _L()
    g = torch.Generator().manual_seed(10 * M + H)
    G = torch.randn(M, 4 * H, generator=g)
    c_prev, dh, dc_in = (torch.randn(M, H, generator=g) for _ in range(3))
    reset = torch.tensor((np.arange(M) % 3 == 0).astype(np.uint8))
    for rs, dci in ((reset, dc_in), (None, dc_in), (reset, None)):
        G64, cp64 = G.double().requires_grad_(True), c_prev.double().requires_grad_(True)
        keep = (rs == 0).double().view(-1, 1) if rs is not None else 1.0
        gi, gf, gg, go = G64.chunk(4, 1)
        i, f, gt, o = torch.sigmoid(gi), torch.sigmoid(gf), torch.tanh(gg), torch.sigmoid(go)
        c = f * (cp64 * keep) + i * gt
        h = o * torch.tanh(c)
        ((h * dh.double()).sum() + ((c * dci.double()).sum() if dci is not None else 0.0)).backward()
        acts = torch.cat([i, f, gt, o, torch.tanh(c)], 1).detach().float()
        dG, dcp = torch.full((M, 4 * H), 777.0, device=DEV), torch.full((M, H), 777.0, device=DEV)
        L.lstm_cell_backward_hip(_dev(dh), _dev(dci) if dci is not None else None, _dev(acts), _dev(c_prev), _dev(rs) if rs is not None else None, dG, dcp)
        for got, want in ((dG, G64.grad), (dcp, cp64.grad)):
            assert ((got.cpu().double() - want).abs() <= 2e-5 * want.abs().clamp_min(1.0)).all()
        if rs is not None:
            assert not dcp.cpu()[rs != 0].any()
        want_t = L.lstm_cell_backward_torch(_dev(dh), _dev(dci) if dci is not None else None, _dev(acts), _dev(c_prev), _dev(rs) if rs is not None else None)
        assert ((dG - want_t[0]).abs() <= 2e-5 * want_t[0].abs().clamp_min(1.0)).all()


def test_invalid_arguments_leave_the_outputs_untouched():
    L = _L()
    lib = L._lib()
    M, D, H = 8, 5, 32
    x, h, c, reset = (_dev(a) for a in R.cell_inputs(M, D, H))
    wi, wh, bi, bh = (torch.zeros(s, device=DEV) for s in ((4 * H, D), (4 * H, H), (4 * H,), (4 * H,)))
    hn, cn, an, pre = (torch.full(s, 777.0, device=DEV) for s in ((M, H), (M, H), (M, 5 * H), (M, 4 * H)))
    P = lambda t: t.data_ptr() if t is not None else None

    def cell(M=M, D=D, H=H, **kw):
        a = dict(x=x, hp=h, cp=c, rs=reset, wi=wi, wh=wh, bi=bi, bh=bh, h=hn, c=cn, acts=an)
        a.update(kw)
        return lib.grx_lstm_cell(M, D, H, *[P(a[k]) for k in ("x", "hp", "cp", "rs", "wi", "wh", "bi", "bh", "h", "c", "acts")], None)
    assert cell(M=0) < 0 and cell(D=0) < 0 and cell(H=0) < 0 and cell(H=16) < 0 and cell(H=48) < 0 and cell(H=1056) < 0
    for k in ("x", "hp", "cp", "wi", "wh", "bi", "bh", "h", "c"):
        assert cell(**{k: None}) < 0, k
    assert cell(h=h) < 0 and cell(c=c) < 0                                                      # in place
    both = torch.full((2 * M - 1, H), 777.0, device=DEV)
    assert lib.grx_lstm_cell(M, D, H, P(x), P(both[:M]), P(c), P(reset), P(wi), P(wh), P(bi), P(bh), P(both[M - 1:]), P(cn), P(an), None) < 0   # overlapping
    assert lib.grx_lstm_cell_preact(M, D, 48, P(x), P(h), P(reset), P(wi), P(wh), P(bi), P(bh), P(pre), None) < 0
    assert lib.grx_lstm_cell_preact(M, D, H, P(x), None, P(reset), P(wi), P(wh), P(bi), P(bh), P(pre), None) < 0
    dG, dcp = torch.full((M, 4 * H), 777.0, device=DEV), torch.full((M, H), 777.0, device=DEV)
    bwd = lambda M=M, H=H, dh=h, acts=an, cp=c, dG=dG, dcp=dcp: lib.grx_lstm_cell_backward(M, H, P(dh), P(c), P(acts), P(cp), P(reset), P(dG), P(dcp), None)
    assert bwd(M=0) < 0 and bwd(H=0) < 0 and bwd(H=40) < 0 and bwd(H=2048) < 0
    assert bwd(dh=None) < 0 and bwd(acts=None) < 0 and bwd(cp=None) < 0 and bwd(dG=None) < 0 and bwd(dcp=None) < 0
    torch.cuda.synchronize()
    for t in (hn, cn, an, pre, dG, dcp, both):
        assert bool((t == 777.0).all())
    assert cell() == 0 and bwd() == 0                                                           # ... and the valid calls do write
    torch.cuda.synchronize()
    assert not bool((hn == 777.0).any()) and not bool((dG == 777.0).any())


# ---- whole sequences -----------------------------------------------------------------------------------------------------------------------
T, N, D, H = 6, 33, 45, 32


def _sequence_case():
    g = torch.Generator().manual_seed(11)
    x = torch.randn(T, N, D, generator=g)
    h0, c0 = torch.tanh(torch.randn(N, H, generator=g)), torch.randn(N, H, generator=g)
    w = torch.randn(T, N, H, generator=g)
    return x, h0, c0, w, R.dones(N)


def _sequence_grads(mem, x, h0, c0, w, d):
    """(h, the four parameter gradients, dX) of sum(h * w) through Memory.sequence on the device"""
    for p in mem.rnn.parameters():
        p.grad = None
    xd = x.to(DEV).requires_grad_(True)
    out = mem.sequence(xd, _dev(R.resets_of(d)), h0.to(DEV), c0.to(DEV))
    (out * w.to(DEV)).sum().backward()
    return [out.detach().cpu()] + [getattr(mem.rnn, k).grad.detach().cpu().clone() for k in R.NAMES] + [xd.grad.cpu()]


def test_sequence_gradients_against_float64(monkeypatch):
    """all four parameter gradients and dX of the fused path against float64 autograd through nn.LSTM over the cut trajectories, and
    against the torch spelling on the device (GRX_LSTM_FUSED=0): each within 1e-4 * max|g_ref| per tensor
    (tests/test_ppo_gpu.py::test_minibatch_parameter_gradients_match_float64's bound)"""
    L = _L()
    torch.manual_seed(12)
    mem = L.Memory(D, H).to(DEV)
    x, h0, c0, w, d = _sequence_case()
    ref = R.lstm64(R.params64(mem.rnn), requires_grad=True)
    x64 = x.double().requires_grad_(True)
    out64 = R.sequence64(ref, x64, d, h0.double(), c0.double())
    (out64 * w.double()).sum().backward()
    want = [out64.detach()] + [getattr(ref, k).grad for k in R.NAMES] + [x64.grad]
    monkeypatch.setenv("GRX_LSTM_FUSED", "1")
    fused = _sequence_grads(mem, x, h0, c0, w, d)
    monkeypatch.setenv("GRX_LSTM_FUSED", "0")
    spelled = _sequence_grads(mem, x, h0, c0, w, d)
    for name, f, s, r in zip(("h",) + R.NAMES + ("dX",), fused, spelled, want):
        bound = 1e-4 * float(r.abs().max())
        ef, es, fs = float((f.double() - r).abs().max()), float((s.double() - r).abs().max()), float((f - s).abs().max())
        print(f"LSTMSequence {name}: fused - f64 {ef:.3g}, GRX_LSTM_FUSED=0 - f64 {es:.3g}, fused - GRX_LSTM_FUSED=0 {fs:.3g}, bound {bound:.3g}")
        assert ef <= bound and es <= bound and fs <= bound, name


# ---- the runner ----------------------------------------------------------------------------------------------------------------------------
def _make(tmp_path, flags=("--recurrent",), episode_length_s=None, steps=8, num_envs=64):
    from wiki_grx_gym_amd.envs import GR1T1Cfg, GR1T1CfgPPO
    from wiki_grx_gym_amd.utils import get_args, task_registry
    args = get_args(["--task", "GR1T1", "--headless", "--num_envs", str(num_envs), "--seed", "3", *flags])
    cfg = GR1T1Cfg()
    if episode_length_s is not None:
        cfg.env.episode_length_s = episode_length_s
    env, _ = task_registry.make_env("GR1T1", args=args, env_cfg=cfg)
    tcfg = GR1T1CfgPPO()
    tcfg.runner.num_steps_per_env = steps
    tcfg.algorithm.num_mini_batches = 4
    runner, _ = task_registry.make_alg_runner(env, name=None, args=args, train_cfg=tcfg, log_root=str(tmp_path) if tmp_path else None)
    return env, runner


def _rollout(runner):
    env, alg = runner.env, runner.alg
    with torch.inference_mode():
        obs, pri = env.get_observations(), env.get_privileged_observations()
        for _ in range(alg.storage.num_transitions_per_env):
            obs, pri, rew, dones, infos = env.step(alg.act(obs, pri))
            alg.process_env_step(rew, dones, infos)
        alg.compute_returns(pri)


def test_update_forward_reproduces_the_rollout_bit_for_bit():
    """Two real rollouts of 8 steps on 64 GR1T1 envs whose episodes last 5 steps, no optimizer step: the update's sequence forward over every
    minibatch -- from the stored h0 / c0, reset_t = dones[t - 1] -- gives the stored mu and values bit for bit.  The second rollout starts from
    the first one's final state, zero where its last step ended an episode."""
    env, runner = _make(None, episode_length_s=0.1)
    alg, ac = runner.alg, runner.alg.actor_critic
    st = alg.storage
    env.episode_length_buf = torch.randint_like(env.episode_length_buf, high=5)          # the envs end at different steps
    for rollout in range(2):
        _rollout(runner)
        inside = int(st.dones[:-1].sum())
        assert inside > 0 and 0 < int(st.dones[-1].sum()) < 64, (inside, int(st.dones[-1].sum()))
        if rollout == 0:
            assert not st.h0_a.any() and not st.c0_c.any()
        else:
            ended, alive = last_dones.view(-1).bool(), ~last_dones.view(-1).bool()
            assert not st.h0_a[ended].any() and not st.c0_a[ended].any() and not st.h0_c[ended].any() and not st.c0_c[ended].any()
            assert st.h0_a[alive].abs().sum(1).min() > 0 and st.c0_c[alive].abs().sum(1).min() > 0
        last_dones = st.dones[-1].clone()
        for enabled in (True, False):
            with torch.set_grad_enabled(enabled):
                for k, (obs, cobs, resets, start, *_rest) in enumerate(st.recurrent_mini_batch_generator(4, 1)):
                    a, b = st.env_ranges(4)[k]
                    fa, fc = ac.features(obs, cobs, resets, start)
                    with ac.on_features():
                        mu, value = ac.actor(fa), ac.evaluate(fc)
                    assert mu.requires_grad == enabled
                    assert torch.equal(mu.detach().view(8, b - a, -1), st.mu[:, a:b]), (rollout, k)
                    assert torch.equal(value.detach().view(8, b - a, 1), st.values[:, a:b]), (rollout, k)
        hidden = [t.clone() for pair in ac.get_hidden_states() for t in pair]
        alg.clear_storage()
        assert all(torch.equal(u, v) for u, v in zip(hidden, [t for pair in ac.get_hidden_states() for t in pair]))


def test_train_save_load_play_export(tmp_path, monkeypatch):
    L = _L()
    from wiki_grx_gym_amd.scripts.play import play
    from wiki_grx_gym_amd.utils import get_args, task_registry
    # (play() takes the registered config instance, which the flags write to: undone when the test ends)
    reg = task_registry.train_cfgs["GR1T1"]
    monkeypatch.setattr(reg.runner, "policy_class_name", reg.runner.policy_class_name, raising=False)
    monkeypatch.setattr(reg.policy, "rnn_hidden_size", 64, raising=False)
    flags = ["--recurrent", "--rnn_hidden_size", "64"]
    env, runner = _make(tmp_path, flags=tuple(flags), steps=16)
    ac = runner.alg.actor_critic
    assert type(ac) is L.ActorCriticRecurrent and ac.memory_a.rnn.weight_ih_l0.shape == (256, 39) and ac.memory_c.rnn.weight_ih_l0.shape == (256, 168)
    assert runner.alg._graph is None and not runner.alg._use_graph and not runner.alg._use_act_graph
    before = {k: v.detach().clone() for k, v in ac.state_dict().items()}
    losses, update = [], runner.alg.update

    def recording_update():
        losses.append(update())
        return losses[-1]
    runner.alg.update = recording_update
    runner.learn(num_learning_iterations=2, init_at_random_ep_len=True)
    assert len(losses) == 2 and all(np.isfinite(v) for pair in losses for v in pair), losses
    after = ac.state_dict()
    assert all(torch.isfinite(v).all() for v in after.values())
    assert all(not torch.equal(before[k], after[k]) for k in after if k.startswith("memory_"))
    ck = torch.load(os.path.join(runner.log_dir, "model_2.pt"), weights_only=False)
    assert ck["recurrent"] == {"hidden_size": 64} and set(ck) == {"model_state_dict", "optimizer_state_dict", "iter", "infos", "recurrent"}

    # a non-finite loss skips the step: every minibatch of this update has a NaN value loss
    _rollout(runner)
    params = {k: v.detach().clone() for k, v in ac.state_dict().items()}
    moments = [{k: v.clone() for k, v in s.items() if torch.is_tensor(v)} for s in runner.alg.optimizer.state.values()]
    runner.alg.storage.returns[:, :, 0] = float("nan")
    assert runner.alg.update() == (0.0, 0.0)
    assert all(torch.equal(v, ac.state_dict()[k]) for k, v in params.items())
    assert all(torch.equal(v, s[k]) for m, s in zip(moments, runner.alg.optimizer.state.values()) for k, v in m.items() if k != "step")
    runner.alg.clear_storage()

    with pytest.raises(ValueError, match="--recurrent"):                                   # play without the flag refuses the checkpoint
        play(get_args(["--task", "GR1T1", "--headless", "--seed", "3"]), steps=1, log_root=str(tmp_path))
    out = play(get_args(["--task", "GR1T1", "--headless", "--seed", "3"] + flags), steps=20, log_root=str(tmp_path))
    assert len(open(out["states"]).readlines()) == 20
    penv, prunner = out["env"], out["runner"]
    loaded = prunner.alg.actor_critic.state_dict()
    assert all(torch.equal(loaded[k], v) for k, v in after.items() if k != "std")
    policy = prunner.get_inference_policy(device=penv.device)
    assert isinstance(policy, L.RecurrentPolicy)
    jit = torch.jit.load(out["exported"])                                                  # on the CPU, fed env 0's and env 7's raw frames
    jit.reset_memory()
    obs, worst = penv.get_observations(), 0.0
    with torch.no_grad():
        for _ in range(20):
            actions = policy(obs.detach())
            a = jit(obs[[0, 7]].detach().cpu())
            worst = max(worst, float((a - actions[[0, 7]].cpu()).abs().max()))
            obs, _, _, dones, _ = penv.step(actions.detach())
            policy.reset(dones)
            jit.reset(dones[[0, 7]].cpu())
    print(f"recurrent policy: exported module against the device policy over 20 steps, envs 0 and 7: max |difference| {worst:.3g}")
    assert worst < 1e-5


def test_default_path_is_unchanged(tmp_path):
    from wiki_grx_gym_amd.rl.modules import ActorCriticMLP
    env, runner = _make(tmp_path, flags=())
    assert type(runner.alg.actor_critic) is ActorCriticMLP and not runner.recurrent and not runner.alg._recurrent
    assert type(runner.alg.storage).__name__ == "RolloutStorage"
    runner.learn(num_learning_iterations=1)
    ck = torch.load(os.path.join(runner.log_dir, "model_1.pt"), weights_only=False)
    assert set(ck) == {"model_state_dict", "optimizer_state_dict", "iter", "infos"} and "recurrent" not in ck
    assert not any(k.startswith("memory_") for k in ck["model_state_dict"])
