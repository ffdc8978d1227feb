"""The recurrent distillation student without a GPU (rl/distillation.py StudentTeacherRecurrent, rl/recurrent.py LSTMSequenceBPTT;
DESIGN.md 4.23): LSTMSequenceBPTT's torch spelling against float64, truncated-BPTT windows (exact concatenation, no gradient across a
boundary), the runner over the stub envs of tests/test_distill.py and the oracle-backed env of tests/test_recurrent.py (training,
checkpoints, resume, play-side loading, the exported module, the refusals), the NaN-skip, learnability, the flags, and the C entries'
argument checks."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from tests import lstm_ref as R
from tests.test_distill import REFERENCE_KEYS, FreshStubEnv, _runner
from tests.test_env_plumbing import oracle_backend  # noqa: F401  (the fixture)
from tests.test_obs_history import DoneStubEnv
from tests.test_recurrent import _make as _make_oracle
from wiki_grx_gym_amd.envs import GR1T1Cfg, config
from wiki_grx_gym_amd.envs.config import class_to_dict
from wiki_grx_gym_amd.rl import distillation as D
from wiki_grx_gym_amd.rl import recurrent as L
from wiki_grx_gym_amd.rl.runner import OnPolicyRunner
from wiki_grx_gym_amd.utils.helpers import export_policy_as_jit, get_args, update_cfg_from_args

CFGS = [config.GR1T1CfgPPO, config.GR1T2CfgPPO, config.GR1T1FullBodyCfgPPO]
NEW_KEYS = ("student_recurrent", "student_rnn_hidden_size", "distill_gradient_length")
T, N, DIN, H = 6, 5, 7, 32


def _sequence_inputs(dtype, n=N, d=DIN, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, n, d, generator=g, dtype=torch.float64)
    h0 = torch.tanh(torch.randn(n, H, generator=g, dtype=torch.float64))
    c0 = torch.randn(n, H, generator=g, dtype=torch.float64)
    w = torch.randn(T, n, H, generator=g, dtype=torch.float64)       # the weights of the scalar whose gradient is taken
    return x.to(dtype), h0.to(dtype), c0.to(dtype), w.to(dtype)


# ---- LSTMSequenceBPTT ------------------------------------------------------------------------------------------------------------------------
def test_sequence_bptt_gradients_against_float64_autograd():
    """the torch spelling -- the CPU path and the definition -- against float64 autograd through nn.LSTM over the cut trajectories, with the
    dones pattern of tests/lstm_ref.py: the eight LSTM tensors of two memories and both inputs, each within 1e-4 * max|reference gradient|,
    LSTMSequence's own bound (tests/test_recurrent.py)"""
    d = R.dones(N)
    assert d[0, 0] and d[T - 1, 1] and d[2, 2] and d[3, 2] and not d[:, 3].any() and d[:, 4].all()      # the five kinds of env
    torch.manual_seed(3)
    ac = L.ActorCriticRecurrent(DIN, 9, 3, rnn_hidden_size=H, actor_hidden_dims=[16, 8], critic_hidden_dims=[16, 8])
    checked = 0
    for mem, width, seed in ((ac.memory_a, DIN, 0), (ac.memory_c, 9, 1)):
        x, h0, c0, w = _sequence_inputs(torch.float32, d=width, seed=seed)
        x.requires_grad_(True)
        out, h_last, c_last = mem.sequence_bptt(x, torch.tensor(R.resets_of(d)), h0, c0)
        assert not h_last.requires_grad and not c_last.requires_grad and torch.equal(h_last, out[-1].detach())
        (out * w).sum().backward()
        ref = R.lstm64(R.params64(mem.rnn), requires_grad=True)
        x64 = x.detach().double().requires_grad_(True)
        (R.sequence64(ref, x64, d, h0.double(), c0.double()) * w.double()).sum().backward()
        for k in R.NAMES:
            got, want = getattr(mem.rnn, k).grad.double(), getattr(ref, k).grad
            assert (got - want).abs().max() <= 1e-4 * want.abs().max(), (k, float((got - want).abs().max()), float(want.abs().max()))
            checked += 1
        assert (x.grad.double() - x64.grad).abs().max() <= 1e-4 * x64.grad.abs().max()
    assert checked == 8


def _windows(length):
    return D.RecurrentDistillStorage(N, T, DIN, 3, H, "cpu").windows(length)


@pytest.mark.parametrize("length", [0, 1, 3, T])
def test_windows_with_carried_state_are_the_full_forward(length):
    wins = _windows(length)
    assert wins == {0: [(0, 6)], 1: [(t, t + 1) for t in range(6)], 3: [(0, 3), (3, 6)], T: [(0, 6)]}[length]
    assert _windows(4) == [(0, 4), (4, 6)] and _windows(15) == [(0, 6)]                         # the last window may be shorter
    torch.manual_seed(4)
    mem = L.Memory(DIN, H)
    x, h0, c0, _ = _sequence_inputs(torch.float32)
    resets = torch.tensor(R.resets_of(R.dones(N)))
    with torch.no_grad():
        want = mem.sequence(x, resets, h0, c0)
    pieces, h, c = [], h0, c0
    for t0, t1 in wins:
        out, h, c = mem.sequence_bptt(x[t0:t1], resets[t0:t1], h, c)
        assert not h.requires_grad and not c.requires_grad
        pieces.append(out)
    assert torch.equal(torch.cat(pieces).detach(), want)


def test_no_gradient_crosses_a_window_boundary():
    torch.manual_seed(5)
    mem = L.Memory(DIN, H)
    x, h0, c0, w = _sequence_inputs(torch.float32)
    resets = torch.tensor(R.resets_of(R.dones(N)))

    def second_window_grads(x1, carried=None):
        for p in mem.rnn.parameters():
            p.grad = None
        x1 = x1.clone().requires_grad_(True)
        _, h, c = mem.sequence_bptt(x1, resets[:3], h0, c0)
        assert not h.requires_grad and not c.requires_grad                                     # the start state of window 2 is data
        if carried is not None:
            h, c = carried
        out, _, _ = mem.sequence_bptt(x[3:], resets[3:], h, c)
        (out * w[3:]).sum().backward()
        assert x1.grad is None                                                                 # nothing reached window 1's inputs
        return [p.grad.clone() for p in mem.rnn.parameters()], (h, c)
    grads, carried = second_window_grads(x[:3])
    assert all(float(g.abs().max()) > 0 for g in grads)
    again, _ = second_window_grads(x[:3] + 1.0, carried)                                       # window 1 perturbed, the carried state held fixed
    assert all(torch.equal(a, b) for a, b in zip(grads, again))
    moved, _ = second_window_grads(x[:3] + 1.0)                                                # ... and not held fixed: the state does carry
    assert any(not torch.equal(a, b) for a, b in zip(grads, moved))


# ---- the runner over the stub env --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def teacher(tmp_path_factory):
    """a PPO checkpoint over the stub env whose actor reads the actor's single frames"""
    torch.manual_seed(3)
    r = _runner()
    r.learn(1)
    path = str(tmp_path_factory.mktemp("teacher") / "actor.pt")
    r.save(path)
    return path


def _student(teacher, env=None, **keys):
    torch.manual_seed(7)
    keys = {"student_recurrent": True, "student_rnn_hidden_size": 32, "distill_gradient_length": 3, **keys}
    return _runner(env, distill_from=teacher, **keys)


def _ppo_runner(policy=(), **runner_keys):
    cfg = config.GR1T1CfgPPO()
    for k, v in runner_keys.items():
        setattr(cfg.runner, k, v)
    d = class_to_dict(cfg)
    d["policy"].update(actor_hidden_dims=[32, 16], critic_hidden_dims=[32, 16])
    d["policy"].update(policy)
    d["runner"]["num_steps_per_env"] = 4
    d["algorithm"].update(num_learning_epochs=1, num_mini_batches=2)
    return OnPolicyRunner(DoneStubEnv(), d, None, device="cpu")


def test_student_layout_and_two_iterations(teacher, tmp_path):
    r = _student(teacher, algorithm={"num_learning_epochs": 2})
    alg, ac = r.alg, r.alg.actor_critic
    assert isinstance(alg, D.Distillation) and type(ac) is D.StudentTeacherRecurrent and ac.is_recurrent and r.recurrent
    assert type(alg.storage) is D.RecurrentDistillStorage and alg.storage.h0.shape == (8, 32) and alg.storage.c0.shape == (8, 32)
    assert ac.rnn_hidden_size == 32 and ac.memory_a.rnn.weight_ih_l0.shape == (128, 39) and ac.actor.model[0].in_features == 32
    assert isinstance(ac.actor, L._MemoryMLP) and ac.teacher.model[0].in_features == 39
    assert list(ac.state_dict())[:5] == ["std"] + ["memory_a.rnn." + k for k in R.NAMES]
    assert set(k.split(".")[0] for k in ac.state_dict()) == {"memory_a", "actor", "std", "teacher"}
    in_optimizer = {id(p) for g in alg.optimizer.param_groups for p in g["params"]}
    assert in_optimizer == {id(p) for p in ac.memory_a.parameters()} | {id(p) for p in ac.actor.parameters()}
    before = copy.deepcopy(ac.state_dict())
    losses, update = [], alg.update

    def recording_update():
        losses.append(update())
        return losses[-1]
    alg.update = recording_update
    r.learn(2)
    assert len(losses) == 2 and np.isfinite(losses).all() and all(v > 0 for v in losses)
    assert alg.num_updates == 2 * 2 * 2                                                         # epochs x env ranges x windows (3 steps and 1)
    after = ac.state_dict()
    assert all(not torch.equal(before[k], after[k]) for k in after if k.startswith(("memory_a.", "actor.")))
    assert all(torch.equal(before[k], after[k]) for k in after if k.startswith("teacher.") or k == "std")
    r.save(str(tmp_path / "model_2.pt"))
    ck = torch.load(tmp_path / "model_2.pt", weights_only=False)
    assert set(ck) == REFERENCE_KEYS | {"obs_history", "distillation", "recurrent"}
    assert ck["distillation"] == {"teacher_stream": "actor", "teacher_history": 1, "teacher_width": 39, "loss": "mse",
                                  "student": {"recurrent": 32, "gradient_length": 3}}
    assert ck["recurrent"] == {"hidden_size": 32} and ck["obs_history"] == {"actor": 1, "critic": 1}
    # --resume: the same flags load it, and go on training
    b = _student(teacher, algorithm={"num_learning_epochs": 2})
    b.load(str(tmp_path / "model_2.pt"))
    sb = b.alg.actor_critic.state_dict()
    assert all(torch.equal(after[k], sb[k]) for k in after) and b.current_learning_iteration == 2
    oa, ob = alg.optimizer.state_dict()["state"], b.alg.optimizer.state_dict()["state"]
    assert len(oa) == 10 and oa.keys() == ob.keys() and all(torch.equal(oa[i]["exp_avg"], ob[i]["exp_avg"]) for i in oa)
    b.learn(1)
    for other in (dict(distill_gradient_length=0), dict(student_rnn_hidden_size=64), dict(student_recurrent=False, student_rnn_hidden_size=None,
                                                                                          distill_gradient_length=None)):
        with pytest.raises(ValueError, match="recurrent|distillation"):
            _student(teacher, **other).load(str(tmp_path / "model_2.pt"))


def test_an_mlp_students_checkpoint_is_what_it_was(teacher, tmp_path):
    r = _runner(distill_from=teacher)
    assert type(r.alg.actor_critic) is D.StudentTeacher and type(r.alg.storage) is D.DistillStorage and not r.recurrent
    r.learn(1)
    r.save(str(tmp_path / "mlp.pt"))
    ck = torch.load(tmp_path / "mlp.pt", weights_only=False)
    assert set(ck) == REFERENCE_KEYS | {"obs_history", "distillation"}
    assert ck["distillation"] == {"teacher_stream": "actor", "teacher_history": 1, "teacher_width": 39, "loss": "mse"}
    assert ck["obs_history"] == {"actor": 1, "critic": 1}
    assert set(k.split(".")[0] for k in ck["model_state_dict"]) == {"actor", "std", "teacher"}
    with pytest.raises(ValueError, match="recurrent"):                                        # an MLP student is no recurrent one
        _student(teacher).load(str(tmp_path / "mlp.pt"))
    with pytest.raises(ValueError, match="--recurrent"):                                      # ... nor a recurrent actor
        _ppo_runner(policy={"rnn_hidden_size": 32}, policy_class_name="ActorCriticRecurrent").load(str(tmp_path / "mlp.pt"))


def test_refusals(teacher, monkeypatch):
    with pytest.raises(ValueError, match="--distill_from") as info:
        _runner(student_recurrent=True)
    assert "--student_recurrent" in str(info.value)
    with pytest.raises(ValueError, match="the memory replaces the stack") as info:
        _student(teacher, obs_history_length=3)
    assert "--obs_history" in str(info.value) and "--student_recurrent" in str(info.value)
    with pytest.raises(ValueError, match="--student_recurrent") as info:
        _runner(distill_from=teacher, distill_gradient_length=5)
    assert "--distill_gradient_length" in str(info.value)
    for bad in (-1, 2.5, True, "3"):
        with pytest.raises(ValueError, match="--distill_gradient_length"):
            _student(teacher, distill_gradient_length=bad)
    for bad in (40, 16, 2048, 32.0):
        with pytest.raises(ValueError, match="rnn_hidden_size"):
            _student(teacher, student_rnn_hidden_size=bad)
    # --recurrent with --distill_from stays what tests/test_recurrent.py pins, with a pointer to the new flag
    with pytest.raises(NotImplementedError, match="--distill_from") as info:
        _ppo_runner(policy={"rnn_hidden_size": 32}, policy_class_name="ActorCriticRecurrent", distill_from=teacher)
    assert "--recurrent" in str(info.value) and "--student_recurrent" in str(info.value)
    # what a distillation run refuses stays refused
    with pytest.raises(NotImplementedError, match="exact_resume"):
        _student(teacher, exact_resume=True)
    with pytest.raises(ValueError, match="bf16"):
        _student(teacher, algorithm={"precision": "bf16"})
    with pytest.raises(ValueError, match="privileged_actor"):
        _student(teacher, privileged_actor=True)
    for keys, flag in ((dict(algorithm={"symmetry": "augment"}), "--symmetry"), (dict(algorithm={"value_norm": "running"}), "--value_norm"),
                       (dict(estimator=True), "--estimator"), (dict(algorithm={"grad_penalty_coef": 0.1}), "--grad_penalty_coef")):
        with pytest.raises(ValueError, match=flag) as info:
            _student(teacher, **keys)
        assert "--distill_from" in str(info.value), flag
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    with pytest.raises(NotImplementedError, match="one process"):
        _student(teacher)


@pytest.mark.parametrize("norm", [False, True], ids=["plain", "empirical_normalization"])
def test_play_side_loading_and_export(teacher, tmp_path, capsys, norm):
    keys = {"empirical_normalization": True} if norm else {}
    s = _student(teacher, **keys)
    s.learn(2)
    s.save(str(tmp_path / "model_2.pt"))
    r = _ppo_runner(policy={"rnn_hidden_size": 32}, policy_class_name="ActorCriticRecurrent", **keys)   # play.py --recurrent --rnn_hidden_size 32
    ac = r.alg.actor_critic
    kept = {k: v.clone() for k, v in ac.state_dict().items() if k.startswith(("critic.", "memory_c."))}
    capsys.readouterr()
    r.load(str(tmp_path / "model_2.pt"))
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1 and "distilled" in lines[0] and "memory" in lines[0] and "critic" in lines[0] and "optimizer" in lines[0]
    mine, theirs = ac.state_dict(), s.alg.actor_critic.state_dict()
    assert all(torch.equal(mine[k], v) for k, v in theirs.items() if k.startswith(("memory_a.", "actor.")))
    assert all(torch.equal(mine[k], v) for k, v in kept.items()) and len(r.alg.optimizer.state_dict()["state"]) == 0
    with pytest.raises(ValueError, match="--recurrent"):                                      # a plain runner refuses it, before any load_state_dict
        _ppo_runner(**keys).load(str(tmp_path / "model_2.pt"))
    with pytest.raises(ValueError, match="--rnn_hidden_size"):
        _ppo_runner(policy={"rnn_hidden_size": 64}, policy_class_name="ActorCriticRecurrent", **keys).load(str(tmp_path / "model_2.pt"))
    # the distillation runner's own inference policy, the loaded runner's and the exported module: 8 steps with resets
    own, loaded = s.get_inference_policy(), r.get_inference_policy()
    assert isinstance(own, L.RecurrentPolicy) and isinstance(loaded, L.RecurrentPolicy) and own.memory is not s.alg.actor_critic.memory_a
    jit = torch.jit.load(export_policy_as_jit(s.alg.actor_critic, str(tmp_path / "exported"), normalizer=s.obs_normalizer if norm else None))
    jit.reset_memory()
    g = torch.Generator().manual_seed(9)
    with torch.no_grad():
        for t in range(8):
            x = torch.randn(8, 39, generator=g)
            want = own(x)
            assert torch.equal(loaded(x), want), t
            assert (jit(x) - want).abs().max() < 1e-6, t
            dones = torch.tensor([(e + t) % 3 == 0 for e in range(8)])
            for p in (own, loaded, jit):
                p.reset(dones)


def test_non_finite_loss_skips_every_step(teacher):
    r = _student(teacher)
    r.learn(1)
    ac = r.alg.actor_critic
    before = copy.deepcopy({k: v for k, v in ac.state_dict().items()})
    moments = copy.deepcopy(r.alg.optimizer.state_dict()["state"])
    r.alg.storage.labels[:, :, 1] = float("nan")             # every row: each (range, window) of this update has a NaN loss
    assert r.alg.update() == 0.0 and r.alg.num_updates == 4   # (a skipped step adds nothing to the mean)
    after = ac.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)
    now = r.alg.optimizer.state_dict()["state"]
    assert len(moments) == 10 and all(torch.equal(moments[i][k], now[i][k]) for i in moments for k in ("exp_avg", "exp_avg_sq", "step"))


def test_student_learns_a_teacher_on_its_own_stream(teacher):
    """The teacher reads the actor's single frames.  Asserted: the mean behaviour loss of iterations 16-20 is below iteration 1's, nothing
    more.  Observed on the CPU (H = 32, windows of 3 steps, 4 epochs, 2 env ranges, Adam 1e-3): 5.74 -> 0.0645 (ratio 0.011)."""
    torch.manual_seed(5)
    r = _runner(FreshStubEnv(steps=20 * 8), steps=8, distill_from=teacher, student_recurrent=True, student_rnn_hidden_size=32,
                distill_gradient_length=3, algorithm={"num_learning_epochs": 4, "learning_rate": 1e-3})
    losses, update = [], r.alg.update

    def recording_update():
        losses.append(update())
        return losses[-1]
    r.alg.update = recording_update
    r.learn(20)
    first, last = losses[0], float(np.mean(losses[15:20]))
    print(f"recurrent student: behaviour loss, iteration 1: {first:.6g}, mean of iterations 16-20: {last:.6g}, ratio {last / first:.4g}")
    assert len(losses) == 20 and np.isfinite(losses).all()
    assert last < first


# ---- the oracle-backed env ---------------------------------------------------------------------------------------------------------------------
def test_rollout_contract_on_the_oracle_backed_env(oracle_backend, tmp_path):  # noqa: F811
    """GR1T1 over the oracle, episodes of 5 steps, windows of 4 steps, no action noise: before any optimizer step the windowed forward over
    every env range gives the actions act() returned (the CPU spelling: to the bit) -- h0 / c0, the one-step reset offset and the carried
    state at once; then the run trains and its checkpoint loads into a --recurrent runner"""
    _, t = _make_oracle(tmp_path / "teacher", flags=("--privileged_actor",))
    t.learn(num_learning_iterations=1)
    path = str(tmp_path / "teacher.pt")
    t.save(path)
    cfg = GR1T1Cfg()
    cfg.env.episode_length_s = 0.1
    flags = ("--distill_from", path, "--student_recurrent", "--rnn_hidden_size", "32", "--distill_gradient_length", "4", "--distill_noise_std", "0")
    env, r = _make_oracle(tmp_path / "student", flags=flags, env_cfg=cfg)
    alg, ac, st = r.alg, r.alg.actor_critic, r.alg.storage
    assert type(ac) is D.StudentTeacherRecurrent and ac.teacher.model[0].in_features == 168 and alg.gradient_length == 4
    for rollout in range(2):
        acted = []
        with torch.inference_mode():
            obs, pri = env.get_observations(), env.get_privileged_observations()
            for _ in range(6):
                acted.append(alg.act(obs, pri).clone())
                obs, pri, rew, dones, infos = env.step(acted[-1])
                alg.process_env_step(rew, dones, infos)
        acted = torch.stack(acted)
        assert int(st.dones[:-1].sum()) > 0
        assert bool(st.h0.any()) == (rollout == 1)
        with torch.no_grad():
            for (a, b), ((h, c), wins) in zip(st.env_ranges(3), alg.window_batches()):
                for (t0, t1), (x, resets, labels) in zip(st.windows(4), wins):
                    out, h, c = ac.memory_a.sequence_bptt(x, resets, h, c)
                    assert torch.equal(ac.actor(out.flatten(0, 1)).view(t1 - t0, b - a, -1), acted[t0:t1, a:b]), (rollout, a, t0)
        alg.clear_storage()
    r.learn(num_learning_iterations=1)
    assert alg.num_updates == 2 * 3 * 2                                                        # epochs x env ranges x windows (4 steps and 2)
    ck = str(tmp_path / "student.pt")
    r.save(ck)
    _, play = _make_oracle(None)                                                               # --recurrent --rnn_hidden_size 32
    play.load(ck)
    sd = play.alg.actor_critic.state_dict()
    assert all(torch.equal(sd[k], v) for k, v in ac.state_dict().items() if k.startswith(("memory_a.", "actor.")))


# ---- flags and configs -----------------------------------------------------------------------------------------------------------------
def test_cli_flags_reach_the_runner_config():
    a = get_args([])
    assert a.student_recurrent is False and a.distill_gradient_length is None
    _, cfg = update_cfg_from_args(None, config.GR1T1CfgPPO(), a)
    assert not any(k in class_to_dict(cfg)["runner"] for k in NEW_KEYS)
    argv = ["--distill_from", "some/model_5.pt", "--student_recurrent"]
    runner = class_to_dict(update_cfg_from_args(None, config.GR1T1CfgPPO(), get_args(argv))[1])["runner"]
    assert runner["student_recurrent"] is True and runner["student_rnn_hidden_size"] == 256 and "distill_gradient_length" not in runner
    assert runner["policy_class_name"] == config.GR1T1CfgPPO.runner.policy_class_name           # --recurrent's key is left alone
    argv += ["--rnn_hidden_size", "64", "--distill_gradient_length", "0"]
    runner = class_to_dict(update_cfg_from_args(None, config.GR1T1CfgPPO(), get_args(argv))[1])["runner"]
    assert (runner["student_rnn_hidden_size"], runner["distill_gradient_length"]) == (64, 0)
    only = class_to_dict(update_cfg_from_args(None, config.GR1T1CfgPPO(), get_args(["--distill_gradient_length", "7"]))[1])["runner"]
    assert only["distill_gradient_length"] == 7 and "student_recurrent" not in only            # (the runner refuses it)


@pytest.mark.parametrize("cls", CFGS)
def test_config_classes_have_no_new_attribute(cls):
    argv = ["--distill_from", "x.pt", "--student_recurrent", "--rnn_hidden_size", "64", "--distill_gradient_length", "5"]
    for when in ("before", "after"):
        for key in NEW_KEYS:
            assert not hasattr(cls.runner, key) and key not in class_to_dict(cls())["runner"], (when, key)
        update_cfg_from_args(None, cls(), get_args(argv))


def test_default_gradient_length_is_rsl_rls(teacher):
    r = _runner(distill_from=teacher, student_recurrent=True)
    assert r.alg.gradient_length == 15 and r.alg.actor_critic.rnn_hidden_size == 256 and r.distillation["student"] == {"recurrent": 256, "gradient_length": 15}
    assert r.alg.storage.windows(15) == [(0, 4)]


# ---- the C entries ---------------------------------------------------------------------------------------------------------------------
def test_c_entries_check_their_arguments():
    """invalid sizes, NULL pointers, overlap: negative, nothing launched (no GPU needed; the pointers are never followed)"""
    lib = L._lib()
    p = lambda n: C.c_void_p(0x10000 * n)
    ok = dict(dGn=p(1), W=p(2), rn=p(3), dh_out=p(4), dc_in=p(5), acts=p(6), cp=p(7), rs=p(8), dG=p(100), dcp=p(200))

    def step(M=8, H=32, **kw):
        a = {**ok, **kw}
        return lib.grx_lstm_bptt_step(M, H, *[a[k] for k in ("dGn", "W", "rn", "dh_out", "dc_in", "acts", "cp", "rs", "dG", "dcp")], None)
    assert step(M=0) < 0 and step(H=0) < 0 and step(H=40) < 0 and step(H=1056) < 0 and step(M=13421773) < 0
    for k in ("W", "dh_out", "acts", "cp", "dG", "dcp"):
        assert step(**{k: None}) < 0, k
    assert step(dG=p(1)) < 0 and step(dG=C.c_void_p(0x10000 + 8 * 128 * 4 - 4)) < 0              # in place, overlapping by one float
    assert lib.grx_lstm_bptt_dh(8, 48, p(1), p(2), None, p(4), p(100), None) < 0
    assert lib.grx_lstm_bptt_dh(8, 32, p(1), p(2), None, None, p(100), None) < 0 and lib.grx_lstm_bptt_dh(8, 32, p(1), p(2), None, p(4), None, None) < 0
    assert lib.grx_lstm_bptt_step_tile(48, 8, 32, *[ok[k] for k in ("dGn", "W", "rn", "dh_out", "dc_in", "acts", "cp", "rs", "dG", "dcp")], None) < 0
