"""Random network distillation on the MI355X (rl/rnd.py, csrc/grx_ppo_rnd.hip): grx_rnd_reward against the float64
reference (tests/rnd_ref.py: the bounds and how a sequence is checked are stated there), its determinism and argument checks, the torch
spelling on the device, and the runner through the HIP env."""
import copy
import os

import numpy as np
import pytest
import torch

from tests import rnd_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _M():
    from wiki_grx_gym_amd.rl import rnd
    return rnd


def _lib():
    from wiki_grx_gym_amd.rl.fused_loss import load_ppo_library
    return load_ppo_library()


class HipState:
    """ret and the statistics on the device, and one call of a reward function on them (tests/test_rnd.py's TorchState, with raw)"""

    def __init__(self, N, fn):
        z = lambda *s, **k: torch.zeros(*s, device=DEV, **k)
        self.fn = fn
        self.ret, self.count, self.mean = z(N), z(1, dtype=torch.long), z(1)
        self.var, self.std = torch.ones(1, device=DEV), torch.ones(1, device=DEV)
        self.intrinsic, self.raw = z(N), z(N)

    def tensors(self):
        return [self.ret, self.count, self.mean, self.var, self.std, self.intrinsic, self.raw]

    def __call__(self, pred, targ, rew, weight):
        t = lambda a: torch.from_numpy(np.array(a)).to(DEV)
        rewards = t(rew)
        self.fn(t(pred), t(targ), R.GAMMA, weight, R.EPS, self.ret, self.count, self.mean, self.var, self.std, rewards, self.intrinsic, self.raw)
        n = lambda x: x.detach().cpu().numpy().copy()
        self.rewards = rewards
        return dict(raw=n(self.raw), ret=n(self.ret), intrinsic=n(self.intrinsic), rewards=n(rewards), mean=n(self.mean)[0], var=n(self.var)[0],
                    std=n(self.std)[0], count=n(self.count)[0])


@pytest.mark.parametrize("E", [1, 3, 32, 33, 64])
@pytest.mark.parametrize("N", [1, 63, 65, 257, 1025])
def test_entry_point_against_the_reference(N, E):
    """30 calls: one row, one short of and one past a wave, a short last slab (257, 1025: slabs of 128 rows), widths that are no multiple of 4
    and one past the 32 and at the 64 lanes that share a row"""
    R.check_sequence(N, E, HipState(N, _M().rnd_reward_hip), where="hip")


@pytest.mark.parametrize("E", [3, 32, 64, 200, 256])
def test_a_row_does_not_depend_on_the_batch(E):
    """row n of raw at N = 257 equals an N = 1 call on that row alone, bit for bit (E above 64: several elements per lane)"""
    pred, targ, rew = (torch.from_numpy(np.array(a)).to(DEV) for a in R.inputs(257, E, steps=1)[0])
    full = HipState(257, _M().rnd_reward_hip)
    full.fn(pred, targ, R.GAMMA, R.WEIGHT, R.EPS, *full.tensors()[:5], rew.clone(), full.intrinsic, full.raw)
    r64 = R.row_norm(pred.cpu().numpy(), targ.cpu().numpy())
    assert (np.abs(full.raw.double().cpu().numpy() - r64) <= (E + 8) * R.U * r64).all()
    for n in (0, 1, 63, 64, 127, 128, 255, 256):
        one = HipState(1, _M().rnd_reward_hip)
        one.fn(pred[n:n + 1].contiguous(), targ[n:n + 1].contiguous(), R.GAMMA, R.WEIGHT, R.EPS, *one.tensors()[:5], rew[n:n + 1].clone(),
               one.intrinsic, one.raw)
        assert torch.equal(one.raw[0], full.raw[n]) and torch.equal(one.ret[0], full.ret[n]), (E, n)


def test_the_same_calls_give_the_same_bytes():
    out = []
    for _ in range(2):
        st = HipState(1025, _M().rnd_reward_hip)
        rows = []
        for pred, targ, rew in R.inputs(1025, 33)[:5]:
            st(pred, targ, rew, R.WEIGHT)
            rows += [t.clone() for t in st.tensors()] + [st.rewards.clone()]
        out.append(rows)
    assert all(a.dtype == b.dtype and torch.equal(a, b) for a, b in zip(*out))


def test_rejected_calls_leave_outputs_and_state_untouched():
    lib, N, E = _lib(), 65, 8
    pred, targ = torch.randn(N, E, device=DEV), torch.randn(N, E, device=DEV)
    f = lambda n=N: torch.full((n,), 777.0, device=DEV)
    ret, mean, var, std, rewards, intrinsic, raw = f(), f(1), f(1), f(1), f(), f(), f()
    count = torch.full((1,), 777, device=DEV, dtype=torch.long)
    size = lib.grx_rnd_reward_partials_size(N)
    assert size >= 3 and lib.grx_rnd_reward_partials_size(0) == 0 and lib.grx_rnd_reward_partials_size(-1) == 0
    assert lib.grx_rnd_reward_partials_size((1 << 24) + 1) == 0
    partials = torch.full((size + 2,), 777.0, device=DEV)
    P = lambda t: t.data_ptr()
    base = dict(N=N, E=E, pred=P(pred), targ=P(targ), ret=P(ret), count=P(count), mean=P(mean), var=P(var), std=P(std), rewards=P(rewards),
                intrinsic=P(intrinsic), raw=P(raw), partials=P(partials))

    def call(**kw):
        a = {**base, **kw}
        return lib.grx_rnd_reward(a["N"], a["E"], a["pred"], a["targ"], R.GAMMA, R.WEIGHT, R.EPS, a["ret"], a["count"], a["mean"], a["var"], a["std"],
                                  a["rewards"], a["intrinsic"], a["raw"], a["partials"], None)
    assert call(N=0) < 0 and call(N=-5) < 0 and call(E=0) < 0 and call(E=257) < 0 and call(E=-1) < 0
    assert call(N=1 << 23, E=256) < 0                                                            # N * E = 2^31
    assert call(N=(1 << 24) + 1, E=1) < 0                                                        # a triple's n would not be exact
    for k in ("pred", "targ", "ret", "count", "mean", "var", "std", "rewards", "intrinsic", "partials"):
        assert call(**{k: None}) < 0, k
    assert call(partials=P(partials) + 4) < 0                                                    # 8-byte alignment
    torch.cuda.synchronize()
    assert all(bool((t == 777).all()) for t in (ret, mean, var, std, rewards, intrinsic, raw, count, partials))
    assert call(raw=None) == 0                                                                   # raw is optional ...
    torch.cuda.synchronize()
    assert bool((raw == 777).all()) and not bool((intrinsic == 777).any()) and int(count) == 777 + N
    assert call() == 0                                                                           # ... and the valid call writes it
    torch.cuda.synchronize()
    assert not bool((raw == 777).any()) and bool((partials[size:] == 777).all())


@pytest.mark.parametrize("N,E", [(65, 3), (257, 32), (1025, 64)])
def test_torch_spelling_on_the_device(N, E):
    R.check_sequence(N, E, HipState(N, _M().rnd_reward_torch), where="torch on the device")


def _filled(monkeypatch, fused, N=64, T=4, S=24, E=32):
    monkeypatch.setenv("GRX_RND_FUSED", fused)
    M = _M()
    calls = {"hip": 0, "torch": 0}
    hip, tch = M.rnd_reward_hip, M.rnd_reward_torch
    monkeypatch.setattr(M, "rnd_reward_hip", lambda *a, **k: (calls.__setitem__("hip", calls["hip"] + 1), hip(*a, **k))[1])
    monkeypatch.setattr(M, "rnd_reward_torch", lambda *a, **k: (calls.__setitem__("torch", calls["torch"] + 1), tch(*a, **k))[1])
    torch.manual_seed(11)
    rnd = M.RandomNetworkDistillation(S, N, T, DEV, num_outputs=E)
    g = torch.Generator().manual_seed(12)
    frames = [(3.0 + 2.0 * torch.randn(N, S, generator=g)).to(DEV) for _ in range(T)]
    ext = torch.randn(T, N, 1, generator=g).to(DEV)
    rows = ext.clone()
    with torch.inference_mode():
        for t in range(T):
            rnd.rollout_step(frames[t], rows[t], t)
    return rnd, rows, ext, calls


@pytest.mark.parametrize("fused", ["1", "0"])
def test_rollout_and_update_on_the_device(monkeypatch, fused):
    """GRX_RND_FUSED selects the entry point or the torch spelling: one reward call per rollout step either way, the stored rows against
    float64 from the stored embeddings, then the update: frozen target, moved predictor, a falling loss, the NaN skip"""
    rnd, rows, ext, calls = _filled(monkeypatch, fused)
    assert calls == ({"hip": 4, "torch": 0} if fused == "1" else {"hip": 0, "torch": 4})
    assert int(rnd.ret_count) == 4 * 64 and int(rnd.normalizer.count) == 4 * 64
    assert torch.equal(rows, ext + rnd.intrinsic.unsqueeze(-1))
    with torch.no_grad():
        pred = copy.deepcopy(rnd.predictor).double()(rnd.states[3].double())
    r64 = R.row_norm(pred.cpu().numpy(), rnd.targets[3].cpu().numpy())
    x64 = R.WEIGHT * r64 / (float(rnd.ret_std) + R.EPS)
    assert np.abs(rnd.intrinsic[3].double().cpu().numpy() - x64).max() <= 1e-4 * x64.max()     # (the fp32 forward of the predictor is in it)
    target = [p.detach().clone() for p in rnd.target.parameters()]
    before = [p.detach().clone() for p in rnd.predictor.parameters()]
    torch.manual_seed(13)
    losses = [rnd.update(1, 2) for _ in range(10)]
    print(f"GRX_RND_FUSED={fused}: losses {[round(x, 5) for x in losses]}")
    assert all(np.isfinite(x) for x in losses) and losses[-1] < losses[0]
    assert all(torch.equal(a, b) for a, b in zip(target, rnd.target.parameters()))
    assert all(not torch.equal(a, b) for a, b in zip(before, rnd.predictor.parameters()))
    rnd.states[1, 5, 2] = float("nan")
    before = [p.detach().clone() for p in rnd.predictor.parameters()]
    assert rnd.update(2, 1) == 0.0
    assert all(torch.equal(a, b) for a, b in zip(before, rnd.predictor.parameters()))


def test_both_paths_agree_on_the_device(monkeypatch):
    a, _, _, _ = _filled(monkeypatch, "1")
    b, _, _, _ = _filled(monkeypatch, "0")
    assert (a.intrinsic - b.intrinsic).abs().max() <= 1e-4 * a.intrinsic.abs().max()             # (two spellings of the forward and the sums)
    assert abs(float(a.ret_std) - float(b.ret_std)) <= 1e-5 * float(a.ret_std) and int(a.ret_count) == int(b.ret_count)


# ---- the runner through the HIP env ------------------------------------------------------------------------------------------------------------
def _make(tmp_path, flags=(), steps=8, num_envs=64):
    from wiki_grx_gym_amd.envs import GR1T1Cfg, GR1T1CfgPPO
    from wiki_grx_gym_amd.utils import get_args, task_registry
    args = get_args(["--task", "GR1T1", "--headless", "--num_envs", str(num_envs), "--seed", "3", *flags])
    env, _ = task_registry.make_env("GR1T1", args=args, env_cfg=GR1T1Cfg())
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


def test_runner_trains_saves_loads_and_plays(tmp_path, monkeypatch):
    from wiki_grx_gym_amd.scripts.play import play
    from wiki_grx_gym_amd.utils import get_args
    M = _M()
    calls, hip = [0], M.rnd_reward_hip
    monkeypatch.setattr(M, "rnd_reward_hip", lambda *a, **k: (calls.__setitem__(0, calls[0] + 1), hip(*a, **k))[1])
    env, runner = _make(tmp_path, ("--rnd",))
    alg, rnd = runner.alg, runner.rnd
    before = [p.detach().clone() for p in rnd.predictor.parameters()]
    policy = [p.detach().clone() for p in alg.actor_critic.parameters()]
    runner.learn(num_learning_iterations=2)
    assert calls[0] == 2 * 8                                                                     # one grx_rnd_reward call per rollout step
    assert isinstance(alg._graph, torch.cuda.CUDAGraph) and type(alg._gather).__name__ == "RowGather"   # PPO's captured step is what it was
    assert all(not torch.equal(a, b) and bool(torch.isfinite(b).all()) for a, b in zip(before, rnd.predictor.parameters()))
    assert all(not torch.equal(a, b) and bool(torch.isfinite(b).all()) for a, b in zip(policy, alg.actor_critic.parameters()))
    assert int(rnd.ret_count) == 2 * 8 * 64 and bool((rnd.intrinsic > 0).all())
    tags = _tags(runner)
    assert len(tags["Loss/rnd"]) == 2 and all(np.isfinite(v) and v > 0 for v in tags["Loss/rnd"] + tags["Train/mean_intrinsic_reward"])
    assert tags["Train/rnd_weight"] == [pytest.approx(0.1)] * 2
    ck_path = os.path.join(runner.log_dir, "model_2.pt")
    ck = torch.load(ck_path, weights_only=False)
    assert set(ck) == {"model_state_dict", "optimizer_state_dict", "iter", "infos", "rnd"}
    _, again = _make(None, ("--rnd",))
    again.load(ck_path)
    sd, sd2 = rnd.state_dict(), again.rnd.state_dict()
    assert all(torch.equal(sd[k], sd2[k]) for k in sd)
    again.learn(num_learning_iterations=1)                                                       # the restored optimizer steps on the device
    assert int(again.rnd.ret_count) == 3 * 8 * 64
    out = play(get_args(["--task", "GR1T1", "--headless", "--seed", "3"]), steps=10, log_root=str(tmp_path))     # play.py knows nothing of it
    assert len(open(out["states"]).readlines()) == 10 and out["runner"].rnd is None


@pytest.mark.parametrize("flags", [("--precision", "bf16"), ("--privileged_actor",), ("--recurrent",), ("--obs_history", "3", "--empirical_normalization"),
                                   ("--symmetry", "augment")])
def test_compositions_train_on_the_device(tmp_path, flags):
    """one iteration each beside --rnd: RND reads the raw privileged frame and writes the reward row, whatever the policy's inputs are; its
    networks stay fp32 under --precision bf16"""
    env, runner = _make(tmp_path, ("--rnd", *flags))
    rnd = runner.rnd
    before = [p.detach().clone() for p in rnd.predictor.parameters()]
    runner.learn(num_learning_iterations=1)
    assert rnd.num_states == env.num_pri_obs and rnd.normalizer.dim == env.num_pri_obs and int(rnd.ret_count) == 8 * 64
    assert rnd.predictor.precision == rnd.target.precision == "fp32" and all(p.dtype == torch.float32 for p in rnd.parameters())
    assert all(not torch.equal(a, b) and bool(torch.isfinite(b).all()) for a, b in zip(before, rnd.predictor.parameters()))
    assert all(bool(torch.isfinite(p).all()) for p in runner.alg.actor_critic.parameters())
    tags = _tags(runner)
    assert np.isfinite(tags["Loss/rnd"][0]) and tags["Train/mean_intrinsic_reward"][0] > 0


def test_default_path_runs_nothing_of_it(monkeypatch):
    M = _M()

    def boom(self, *a, **k):
        raise AssertionError("RandomNetworkDistillation constructed without --rnd")
    monkeypatch.setattr(M.RandomNetworkDistillation, "__init__", boom)
    monkeypatch.setattr(M, "rnd_reward_hip", boom)
    _, plain = _make(None)
    plain.learn(num_learning_iterations=1)
    assert plain.rnd is None and plain.alg.rnd is None and isinstance(plain.alg._graph, torch.cuda.CUDAGraph)
