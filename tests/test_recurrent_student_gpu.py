"""The recurrent distillation student on the GPU (include/grx_ppo_bptt.h grx_lstm_bptt_step / grx_lstm_bptt_dh, rl/recurrent.py
LSTMSequenceBPTT, rl/distillation.py StudentTeacherRecurrent): the step's element-wise part against grx_lstm_cell_backward
byte for byte, its product against float64 at every tile edge, the reset-row rule, row independence, exact integer arithmetic through the
f32 MFMA, the argument checks with canaries, LSTMSequenceBPTT's gradients against float64 and against GRX_LSTM_BPTT_FUSED=0, the rollout /
update contract on a real GR1T1 rollout (bit for bit), train / save / load / play / export, and the paths that must not have moved.

GRX_BPTT_PARITY_JSON=<path>: the float64 test also writes its per-case error ratios there (profiles/recurrent_student_parity.json)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import lstm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DENORMAL = 2.0 ** -149


def _L():
    from wiki_grx_gym_amd.rl import recurrent
    return recurrent


def _dev(a):
    return torch.as_tensor(a).to(DEV) if a is not None else None


@functools.lru_cache(maxsize=None)
def _case(M, H, seed=0):
    """one step's inputs, float32 / uint8 on the CPU: dG_next, W_hh, reset_next, dh_out, dc_in, acts (in the activations' ranges), c_prev,
    reset -- computed once per shape"""
    g = torch.Generator().manual_seed(1000 * M + H + seed)
    dGn, W = torch.randn(M, 4 * H, generator=g), torch.randn(4 * H, H, generator=g) / (H ** 0.5)
    dh_out, dc_in, c_prev = (torch.randn(M, H, generator=g) for _ in range(3))
    pre = torch.randn(M, 5 * H, generator=g)
    acts = torch.cat([torch.sigmoid(pre[:, :2 * H]), torch.tanh(pre[:, 2 * H:3 * H]), torch.sigmoid(pre[:, 3 * H:4 * H]), torch.tanh(pre[:, 4 * H:])], 1)
    reset_next = torch.tensor((np.arange(M) % 3 == 0).astype(np.uint8))
    reset = torch.tensor((np.arange(M) % 4 == 1).astype(np.uint8))
    return dGn, W, reset_next, dh_out, dc_in, acts.contiguous(), c_prev, reset


def _step(L, dGn, W, rn, dh_out, dc_in, acts, c_prev, reset, tile=None):
    M, H = dh_out.shape
    dG, dcp = torch.full((M, 4 * H), 777.0, device=DEV), torch.full((M, H), 777.0, device=DEV)
    L.lstm_bptt_step_hip(dGn, W, rn, dh_out, dc_in, acts, c_prev, reset, dG, dcp, tile_units=tile)
    return dG, dcp


def _cell_backward(L, dh, dc_in, acts, c_prev, reset):
    M, H = dh.shape
    dG, dcp = torch.full((M, 4 * H), 777.0, device=DEV), torch.full((M, H), 777.0, device=DEV)
    L.lstm_cell_backward_hip(dh, dc_in, acts, c_prev, reset, dG, dcp)
    return dG, dcp


# ---- the step kernel ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,H", [(1, 32), (33, 96), (200, 160)])
def test_elementwise_part_is_the_cell_backward_byte_for_byte(M, H):
    """without a product the step IS grx_lstm_cell_backward; with one it is grx_lstm_cell_backward fed the hook's dh; every block width
    and a second call give the same bytes"""
    L = _L()
    dGn, W, rn, dh_out, dc_in, acts, c_prev, reset = (_dev(a) for a in _case(M, H))
    for dci, rs in ((dc_in, reset), (None, reset), (dc_in, None), (None, None)):
        got = _step(L, None, W, None, dh_out, dci, acts, c_prev, rs)
        want = _cell_backward(L, dh_out, dci, acts, c_prev, rs)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), ("no product", dci is None, rs is None)
        for rnx in (rn, None):
            dh = L.lstm_bptt_dh_hip(dGn, W, rnx, dh_out)
            got = _step(L, dGn, W, rnx, dh_out, dci, acts, c_prev, rs)
            want = _cell_backward(L, dh, dci, acts, c_prev, rs)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), ("product", dci is None, rs is None, rnx is None)
            again = _step(L, dGn, W, rnx, dh_out, dci, acts, c_prev, rs)
            assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])
            for tile in (32, 64, 128):
                other = _step(L, dGn, W, rnx, dh_out, dci, acts, c_prev, rs, tile=tile)
                assert torch.equal(got[0], other[0]) and torch.equal(got[1], other[1]), tile
    assert torch.equal(L.lstm_bptt_dh_hip(None, W, None, dh_out), dh_out + 0.0)


@pytest.fixture(scope="module")
def parity():
    rows = {}
    yield rows
    path = os.environ.get("GRX_BPTT_PARITY_JSON")
    if path and rows:
        with open(path, "w") as f:
            json.dump({"what": "max over outputs of |s - s64| / sum_k |dG_next W_hh|, s = grx_lstm_bptt_dh with dh_out = 0, s64 the float64 product; "
                       "the bound is 4H 2^-24 (a 4H-long fmaf chain); case = M x H, reset_next", "peak": max(r["ratio"] for r in rows.values()),
                       "cases": rows}, f, indent=1)


@pytest.mark.parametrize("with_reset", [False, True], ids=["plain", "reset_next"])
@pytest.mark.parametrize("H", [32, 96, 160])
@pytest.mark.parametrize("M", [1, 31, 33, 129, 200])
def test_dh_against_float64(M, H, with_reset, parity):
    """|s - s64| <= 4H 2^-24 sum_k |dG W| + one denormal per output: what a 4H-long fmaf chain satisfies by construction (each of the 4H
    roundings is at most 2^-24 of a partial sum, which the sum of magnitudes bounds).  s is read with dh_out = 0, where dh = s exactly; with
    a dh_out, dh is the float32 sum dh_out + s bit for bit"""
    L = _L()
    dGn, W, rn, dh_out, *_ = _case(M, H)
    rn = rn if with_reset else None
    keep = (rn == 0).double().view(-1, 1) if with_reset else 1.0
    s64 = (dGn.double() * keep) @ W.double()
    mag = (dGn.double().abs() * keep) @ W.double().abs()
    s = L.lstm_bptt_dh_hip(_dev(dGn), _dev(W), _dev(rn), torch.zeros(M, H, device=DEV))
    err = (s.cpu().double() - s64).abs()
    ratio = float((err / mag.clamp_min(1e-300)).max())
    parity[f"{M}x{H},{'reset_next' if with_reset else 'plain'}"] = {"error": float(err.max()), "ratio": ratio}
    print(f"grx_lstm_bptt_dh {M} x {H} reset_next={with_reset}: max error {float(err.max()):.3g}, max error / sum|dG W| {ratio:.3g}, bound {4 * H * 2.0 ** -24:.3g}")
    assert (err <= 4 * H * 2.0 ** -24 * mag + DENORMAL).all()
    dh = L.lstm_bptt_dh_hip(_dev(dGn), _dev(W), _dev(rn), _dev(dh_out))
    assert torch.equal(dh, _dev(dh_out) + s)


def test_a_reset_row_never_reads_dg_next():
    L = _L()
    M, H = 200, 96
    dGn, W, rn, dh_out, dc_in, acts, c_prev, reset = (_dev(a) for a in _case(M, H))
    poisoned = dGn.clone()
    poisoned[rn != 0] = float("nan")
    dh = L.lstm_bptt_dh_hip(poisoned, W, rn, dh_out)
    assert torch.equal(dh[rn != 0], dh_out[rn != 0] + 0.0) and torch.equal(dh, L.lstm_bptt_dh_hip(dGn, W, rn, dh_out))
    got, want = _step(L, poisoned, W, rn, dh_out, dc_in, acts, c_prev, reset), _step(L, dGn, W, rn, dh_out, dc_in, acts, c_prev, reset)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and bool(torch.isfinite(got[0]).all())
    assert not got[1][reset != 0].any()                                                     # ... and a row reset at its own step hands no dc back


def test_a_row_does_not_depend_on_the_rows_beside_it():
    L = _L()
    M, H = 200, 96
    dGn, W, rn, dh_out, dc_in, acts, c_prev, reset = (_dev(a) for a in _case(M, H))
    dG, dcp = _step(L, dGn, W, rn, dh_out, dc_in, acts, c_prev, reset)
    dh = L.lstm_bptt_dh_hip(dGn, W, rn, dh_out)
    for r in (0, 1, 31, 32, 127, 128, 198, 199):          # reset rows and others; the edges of a wave's and a block's rows
        one = [t[r:r + 1].clone() for t in (dGn, rn, dh_out, dc_in, acts, c_prev, reset)]
        g1, c1 = _step(L, one[0], W, one[1], *one[2:])
        assert torch.equal(g1[0], dG[r]) and torch.equal(c1[0], dcp[r]), r
        assert torch.equal(L.lstm_bptt_dh_hip(one[0], W, one[1], one[2])[0], dh[r]), r


@pytest.mark.parametrize("structured", [False, True], ids=["random", "structured"])
@pytest.mark.parametrize("M,H", [(33, 96), (130, 32), (5, 160)])
def test_the_product_is_exact_on_integers(M, H, structured):
    """small integers: every product and partial sum is an integer below 2^24 (at most 640 * 64 + 8), so float32 is exact and dh must equal
    the int64 result -- whatever the summation order; a swapped or permuted MFMA operand map does not survive the structured operands, where
    A is a function of (row, k) and B another one of (k, unit)"""
    L = _L()
    K = 4 * H
    if structured:
        m, k, j = np.arange(M)[:, None], np.arange(K), np.arange(H)[None, :]
        a, b, d = (m + 3 * k[None, :]) % 7 - 3, (j + 5 * k[:, None]) % 9 - 4, (2 * m + j) % 5 - 2
    else:
        g = np.random.default_rng(7)
        a, b, d = g.integers(-8, 9, (M, K)), g.integers(-8, 9, (K, H)), g.integers(-8, 9, (M, H))
    a, b, d = (np.asarray(t, dtype=np.int64) for t in (a, b, d))
    rn = (np.arange(M) % 4 == 1).astype(np.uint8)
    f = lambda t: _dev(t.astype(np.float32))
    got = L.lstm_bptt_dh_hip(f(a), f(b), _dev(rn), f(d))
    want = d + (a * (rn == 0)[:, None]) @ b
    assert np.array_equal(got.cpu().numpy().astype(np.int64), want) and np.abs(want).max() > 8      # (the sums are no zeros)
    got = L.lstm_bptt_dh_hip(f(a), f(b), None, f(d))
    assert np.array_equal(got.cpu().numpy().astype(np.int64), d + a @ b)


def test_invalid_arguments_leave_the_outputs_untouched():
    L = _L()
    lib = L._lib()
    M, H = 8, 32
    dGn, W, rn, dh_out, dc_in, acts, c_prev, reset = (_dev(a) for a in _case(M, H))
    dG, dcp, dh = (torch.full(s, 777.0, device=DEV) for s in ((M, 4 * H), (M, H), (M, H)))
    P = lambda t: t.data_ptr() if t is not None else None

    def step(M=M, H=H, tile=None, **kw):
        a = dict(dGn=dGn, W=W, rn=rn, dh_out=dh_out, dc_in=dc_in, acts=acts, cp=c_prev, rs=reset, dG=dG, dcp=dcp)
        a.update(kw)
        ptrs = [P(a[k]) for k in ("dGn", "W", "rn", "dh_out", "dc_in", "acts", "cp", "rs", "dG", "dcp")]
        return lib.grx_lstm_bptt_step(M, H, *ptrs, None) if tile is None else lib.grx_lstm_bptt_step_tile(tile, M, H, *ptrs, None)

    def hook(M=M, H=H, **kw):
        a = dict(dGn=dGn, W=W, rn=rn, dh_out=dh_out, dh=dh)
        a.update(kw)
        return lib.grx_lstm_bptt_dh(M, H, *[P(a[k]) for k in ("dGn", "W", "rn", "dh_out", "dh")], None)
    for call in (step, hook):
        assert call(M=0) < 0 and call(M=-3) < 0 and call(H=0) < 0 and call(H=16) < 0 and call(H=48) < 0 and call(H=1056) < 0
        assert call(M=13421773) < 0                                                            # M * 5H = 2^31 + 32
        assert call(dh_out=None) < 0 and call(W=None) < 0
    for k in ("acts", "cp", "dG", "dcp"):
        assert step(**{k: None}) < 0, k
    assert hook(dh=None) < 0 and step(tile=48) < 0 and step(tile=256) < 0
    both = torch.full((2 * M - 1, 4 * H), 777.0, device=DEV)
    assert step(dGn=both[:M], dG=both[M - 1:]) < 0 and step(dGn=both[:M], dG=both[:M]) < 0   # dG overlapping dG_next, in place
    assert hook(dGn=both[:M], dh=both[M - 1:]) < 0
    torch.cuda.synchronize()
    for t in (dG, dcp, dh, both):
        assert bool((t == 777.0).all())
    assert step() == 0 and hook() == 0 and step(dGn=None, W=None, rn=None, dc_in=None, rs=None) == 0   # ... and the valid calls do write
    torch.cuda.synchronize()
    assert not bool((dG == 777.0).any()) and not bool((dh == 777.0).any())


# ---- whole sequences -----------------------------------------------------------------------------------------------------------------------
T, N, D, H = 6, 33, 45, 32


def _sequence_grads(mem, x, h0, c0, w, d):
    """(h, the four parameter gradients, dX) of sum(h * w) through Memory.sequence_bptt on the device"""
    for p in mem.rnn.parameters():
        p.grad = None
    xd = x.to(DEV).requires_grad_(True)
    out, h_last, c_last = mem.sequence_bptt(xd, _dev(R.resets_of(d)), h0.to(DEV), c0.to(DEV))
    assert not h_last.requires_grad and not c_last.requires_grad and torch.equal(h_last, out[-1].detach())
    (out * w.to(DEV)).sum().backward()
    return [out.detach().cpu()] + [getattr(mem.rnn, k).grad.detach().cpu().clone() for k in R.NAMES] + [xd.grad.cpu()]


def test_sequence_bptt_gradients_against_float64(monkeypatch):
    """all four parameter gradients and dX of the fused backward against float64 autograd through nn.LSTM over the cut trajectories, and
    against the three-launch spelling (GRX_LSTM_BPTT_FUSED=0): each within 1e-4 * max|g_ref| per tensor, LSTMSequence's own bound"""
    L = _L()
    torch.manual_seed(12)
    mem = L.Memory(D, H).to(DEV)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(T, N, D, generator=g)
    h0, c0 = torch.tanh(torch.randn(N, H, generator=g)), torch.randn(N, H, generator=g)
    w, d = torch.randn(T, N, H, generator=g), R.dones(N)
    ref = R.lstm64(R.params64(mem.rnn), requires_grad=True)
    x64 = x.double().requires_grad_(True)
    out64 = R.sequence64(ref, x64, d, h0.double(), c0.double())
    (out64 * w.double()).sum().backward()
    want = [out64.detach()] + [getattr(ref, k).grad for k in R.NAMES] + [x64.grad]
    calls = []
    step = L.lstm_bptt_step_hip
    monkeypatch.setattr(L, "lstm_bptt_step_hip", lambda *a, **k: (calls.append(1), step(*a, **k))[1])
    monkeypatch.setenv("GRX_LSTM_BPTT_FUSED", "1")
    fused = _sequence_grads(mem, x, h0, c0, w, d)
    assert len(calls) == T                                                                    # one launch per step
    monkeypatch.setenv("GRX_LSTM_BPTT_FUSED", "0")
    spelled = _sequence_grads(mem, x, h0, c0, w, d)
    assert len(calls) == T
    for name, f, s, r in zip(("h",) + R.NAMES + ("dX",), fused, spelled, want):
        bound = 1e-4 * float(r.abs().max())
        ef, es, fs = float((f.double() - r).abs().max()), float((s.double() - r).abs().max()), float((f - s).abs().max())
        print(f"LSTMSequenceBPTT {name}: fused - f64 {ef:.3g}, GRX_LSTM_BPTT_FUSED=0 - f64 {es:.3g}, fused - spelling {fs:.3g}, bound {bound:.3g}")
        assert ef <= bound and es <= bound and fs <= bound, name


# ---- the runner ----------------------------------------------------------------------------------------------------------------------------
BASE = ["--task", "GR1T1", "--headless", "--num_envs", "64", "--seed", "3"]


def _make(root, flags, episode_length_s=None, steps=8):
    from wiki_grx_gym_amd.envs import GR1T1Cfg, GR1T1CfgPPO
    from wiki_grx_gym_amd.utils import get_args, task_registry
    args = get_args(BASE + list(flags))
    cfg = GR1T1Cfg()
    if episode_length_s is not None:
        cfg.env.episode_length_s = episode_length_s
    env, _ = task_registry.make_env("GR1T1", args=args, env_cfg=cfg)
    tcfg = GR1T1CfgPPO()
    tcfg.runner.num_steps_per_env = steps
    tcfg.algorithm.num_mini_batches = 4
    runner, _ = task_registry.make_alg_runner(env, name=None, args=args, train_cfg=tcfg, log_root=str(root) if root else None)
    return env, runner


@pytest.fixture(scope="module")
def teacher(tmp_path_factory):
    """a privileged PPO teacher on GR1T1, two iterations of 8 steps on 64 envs: the path of its checkpoint"""
    root = tmp_path_factory.mktemp("teacher")
    _, runner = _make(root, ["--privileged_actor"])
    runner.learn(num_learning_iterations=2, init_at_random_ep_len=True)
    return os.path.join(runner.log_dir, "model_2.pt")


def test_update_forward_reproduces_the_rollout_bit_for_bit(teacher):
    """Two real rollouts of 8 steps on 64 GR1T1 envs whose episodes last 5 steps, windows of 3 steps, no action noise, no optimizer step: the
    windowed forward over every env range -- from the stored h0 / c0, reset_t = dones[t - 1], the state carried from window to window --
    gives the actions act() returned, bit for bit.  The second rollout starts from the first one's final state, zero where its last step
    ended an episode"""
    from wiki_grx_gym_amd.rl.distillation import RecurrentDistillStorage, StudentTeacherRecurrent
    env, runner = _make(None, ["--distill_from", teacher, "--student_recurrent", "--rnn_hidden_size", "32", "--distill_gradient_length", "3",
                               "--distill_noise_std", "0"], episode_length_s=0.1)
    alg, ac = runner.alg, runner.alg.actor_critic
    st = alg.storage
    assert type(ac) is StudentTeacherRecurrent and type(st) is RecurrentDistillStorage and st.windows(3) == [(0, 3), (3, 6), (6, 8)]
    env.episode_length_buf = torch.randint_like(env.episode_length_buf, high=5)          # the envs end at different steps
    for rollout in range(2):
        acted = []
        with torch.inference_mode():
            obs, pri = env.get_observations(), env.get_privileged_observations()
            for _ in range(8):
                acted.append(alg.act(obs, pri).clone())
                obs, pri, rew, dones, infos = env.step(acted[-1])
                alg.process_env_step(rew, dones, infos)
        acted = torch.stack(acted)
        inside = int(st.dones[:-1].sum())
        assert inside > 0 and 0 < int(st.dones[-1].sum()) < 64, (inside, int(st.dones[-1].sum()))
        if rollout == 0:
            assert not st.h0.any() and not st.c0.any()
        else:
            ended = last_dones.view(-1).bool()
            assert not st.h0[ended].any() and not st.c0[ended].any() and st.h0[~ended].abs().sum(1).min() > 0
        last_dones = st.dones[-1].clone()
        for enabled in (True, False):
            with torch.set_grad_enabled(enabled):
                batches = alg.window_batches()
                assert len(batches) == 4
                for (a, b), ((h, c), wins) in zip(st.env_ranges(4), batches):
                    assert not h.requires_grad and len(wins) == 3
                    for (t0, t1), (x, resets, labels) in zip(st.windows(3), wins):
                        out, h, c = ac.memory_a.sequence_bptt(x, resets, h, c)
                        mu = ac.actor(out.flatten(0, 1))
                        assert mu.requires_grad == enabled and not h.requires_grad and not c.requires_grad
                        assert torch.equal(mu.detach().view(t1 - t0, b - a, -1), acted[t0:t1, a:b]), (rollout, a, t0)
        alg.clear_storage()


def test_train_save_load_play_export(teacher, tmp_path, monkeypatch):
    L = _L()
    from wiki_grx_gym_amd.rl.distillation import Distillation, StudentTeacherRecurrent
    from wiki_grx_gym_amd.scripts.play import play
    from wiki_grx_gym_amd.utils import get_args, task_registry
    # (play() takes the registered config instance, which the flags write to: undone when the test ends)
    reg = task_registry.train_cfgs["GR1T1"]
    monkeypatch.setattr(reg.runner, "policy_class_name", reg.runner.policy_class_name, raising=False)
    monkeypatch.setattr(reg.policy, "rnn_hidden_size", 32, raising=False)
    env, runner = _make(tmp_path, ["--distill_from", teacher, "--student_recurrent", "--rnn_hidden_size", "32"], steps=16)
    ac = runner.alg.actor_critic
    assert isinstance(runner.alg, Distillation) and type(ac) is StudentTeacherRecurrent and runner.alg._fused
    assert ac.memory_a.rnn.weight_ih_l0.shape == (128, 39) and ac.actor.model[0].in_features == 32 and ac.teacher.model[0].in_features == 168
    before = {k: v.detach().clone() for k, v in ac.state_dict().items()}
    runner.learn(num_learning_iterations=2, init_at_random_ep_len=True)
    assert runner.alg._tail is not None and runner.alg.num_updates == runner.alg.num_learning_epochs * 4 * 2   # epochs x ranges x windows (15 steps and 1)
    scalars = [json.loads(ln) for ln in open(os.path.join(runner.log_dir, "scalars.jsonl"))]
    behavior = [s["value"] for s in scalars if s["tag"] == "Loss/behavior"]
    print("recurrent student on GR1T1, 64 envs: Loss/behavior per iteration", behavior)
    assert len(behavior) == 2 and np.isfinite(behavior).all() and all(b > 0 for b in behavior)
    after = ac.state_dict()
    assert all(torch.isfinite(v).all() for v in after.values())
    assert all(not torch.equal(before[k], after[k]) for k in after if k.startswith(("memory_a.", "actor.")))
    assert all(torch.equal(before[k], after[k]) for k in after if k.startswith("teacher."))
    ck = torch.load(os.path.join(runner.log_dir, "model_2.pt"), weights_only=False)
    assert ck["recurrent"] == {"hidden_size": 32} and ck["obs_history"] == {"actor": 1, "critic": 1}
    assert ck["distillation"]["student"] == {"recurrent": 32, "gradient_length": 15}

    with pytest.raises(ValueError, match="--recurrent"):                                   # play without the flag refuses the checkpoint
        play(get_args(["--task", "GR1T1", "--headless", "--seed", "3"]), steps=1, log_root=str(tmp_path))
    out = play(get_args(["--task", "GR1T1", "--headless", "--seed", "3", "--recurrent", "--rnn_hidden_size", "32"]), steps=20, log_root=str(tmp_path))
    assert len(open(out["states"]).readlines()) == 20
    penv, prunner = out["env"], out["runner"]
    assert prunner.distillation is None and type(prunner.alg.actor_critic) is L.ActorCriticRecurrent
    loaded = prunner.alg.actor_critic.state_dict()
    assert all(torch.equal(loaded[k], v) for k, v in after.items() if k.startswith(("memory_a.", "actor.")))
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
    print(f"recurrent student: exported module against the device policy over 20 steps, envs 0 and 7: max |difference| {worst:.3g}")
    assert worst < 1e-5


# ---- what must not have moved ----------------------------------------------------------------------------------------------------------------
def test_cell_backward_and_lstm_sequence_are_untouched(monkeypatch):
    """grx_lstm_cell_backward against its torch spelling, tests/test_recurrent_gpu.py's bound (2e-5 * max(|ref|, 1)); LSTMSequence -- PPO's
    recurrent update -- never reaches the new entry point and gives its spelling's gradients within its own bound"""
    L = _L()
    M, Hh = 33, 96
    _, _, _, dh, dc_in, acts, c_prev, reset = (_dev(a) for a in _case(M, Hh))
    for rs, dci in ((reset, dc_in), (None, dc_in), (reset, None)):
        got = _cell_backward(L, dh, dci, acts, c_prev, rs)
        want = L.lstm_cell_backward_torch(dh, dci, acts, c_prev, rs)
        for g, w in zip(got, want):
            assert ((g - w).abs() <= 2e-5 * w.abs().clamp_min(1.0)).all()

    def refuse(*a, **k):
        raise AssertionError("LSTMSequence reached grx_lstm_bptt_step")
    monkeypatch.setattr(L, "lstm_bptt_step_hip", refuse)
    torch.manual_seed(12)
    mem = L.Memory(D, H).to(DEV)
    g = torch.Generator().manual_seed(11)
    x, h0, c0, w = torch.randn(T, N, D, generator=g), torch.randn(N, H, generator=g), torch.randn(N, H, generator=g), torch.randn(T, N, H, generator=g)
    grads = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("GRX_LSTM_FUSED", fused)
        for p in mem.rnn.parameters():
            p.grad = None
        out = mem.sequence(x.to(DEV), _dev(R.resets_of(R.dones(N))), h0.to(DEV), c0.to(DEV))
        (out * w.to(DEV)).sum().backward()
        grads[fused] = [getattr(mem.rnn, k).grad.clone() for k in R.NAMES]
    for a, b in zip(grads["1"], grads["0"]):
        assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max())


def test_default_and_recurrent_ppo_runners_are_what_they_were():
    from wiki_grx_gym_amd.rl.modules import ActorCriticMLP
    _, runner = _make(None, [])
    assert type(runner.alg.actor_critic) is ActorCriticMLP and not runner.recurrent and not runner.student_recurrent
    assert type(runner.alg.storage).__name__ == "RolloutStorage"
    _, runner = _make(None, ["--recurrent", "--rnn_hidden_size", "32"])
    assert type(runner.alg.actor_critic) is _L().ActorCriticRecurrent and runner.recurrent and not runner.student_recurrent
    assert type(runner.alg.storage).__name__ == "RecurrentRolloutStorage" and runner.distillation is None
