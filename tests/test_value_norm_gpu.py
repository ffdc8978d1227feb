"""Value normalisation on the MI355X (rl/value_norm.py, csrc/grx_ppo_gae.hip): grx_gae_returns against the torch loop (bit
for bit where include/grx_ppo_gae.h promises it) and against the float64 reference (tests/gae_ref.py), its column independence, repeatability and
argument checks, the fused launches against GRX_GAE_FUSED=0 through the runner, the captured critic graph, save / resume / play, the
compositions, and the default path.

Tolerances of the comparisons with the float64 reference: per case and per quantity FOUR times the deviation the fp32 torch spelling on the
device (rl.value_norm.gae_returns_torch: for the advantages RolloutStorage.compute_returns' own lines, for the statistics
EmpiricalNormalization's update rule) shows from the same reference on the same inputs; the margin covers the other summation order.  That
deviation is taken as at least half an fp32 unit in the last place of the reference value (of the largest one, for an array): the reference
is formed from float64 returns, so no fp32 number is expected closer to it than its own representation error, and a torch result that lands
closer did so by chance (first run on the device, T = 1, N = 257, done at the last step: the running mean of the torch spelling 0.017 ulp
from the reference, the entry point's 1.017 ulp, the neighbouring float).
For the quantities that are ONE number per call (the four statistics and the state's mean / var / std / scale) the torch spelling's deviation
is the largest over the cases of the same shape (T, N), not the single case's: both implementations read the same fp32 returns, the
reference float64 ones, so at a small T N either result lies a few ulp from the reference, and which of the two lands nearer in one case is a
draw (second run on the device, T = 24, N = 1: the batch variance of the torch spelling under 0.5 ulp from the reference, the entry point's,
formed in float64 from the same fp32 returns, 2.25 ulp).  The arrays (advantages, normalised values and returns) are held case by case.
Both deviations are measured here and printed; GRX_VALUE_NORM_PARITY_OUT=<path> writes their maxima as JSON
(profiles/value_norm_parity.json)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import gae_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES_N = [1, 63, 65, 257, 1025]
QUANTITIES = ("advantages", "adv_mean", "adv_std", "batch_mean", "batch_var", "values", "returns", "mean", "var", "std", "scale")
STATS = ("adv_mean", "adv_std", "batch_mean", "batch_var")
SCALARS = STATS + ("mean", "var", "std", "scale")   # one number per call: held against the torch spelling's largest deviation at the shape
_PARITY = {}


def _M():
    from wiki_grx_gym_amd.rl import value_norm
    return value_norm


def _lib():
    from wiki_grx_gym_amd.rl.fused_loss import load_ppo_library
    return load_ppo_library()


def _dev(x):
    return [torch.from_numpy(np.array(a)).to(DEV) for a in x]


def _state(src=None):
    st = list(_M().ValueNormalizer("running", R.EPS, DEV).state())
    if src is not None:
        for a, b in zip(st, src):
            a.copy_(b)
    return st


def _run(fn, x, state):
    """one call of fn on device copies of x = (rewards, values, dones, last): (raw tensors, dict of float64 numpy results)"""
    r, v, d, lv = _dev(x)
    ret, adv, stats = torch.full_like(r, 7.0), torch.full_like(r, 7.0), torch.zeros(4, device=DEV)
    fn(r, v, d, lv, R.GAMMA, R.LAM, R.EPS, state, ret, adv, None, stats)
    n = lambda t: t.detach().cpu().double().numpy().copy()
    out = {"advantages": n(adv), "stats": n(stats)}
    if state is not None:
        out.update(values=n(v), returns=n(ret), count=int(state[0]), **{k: float(t) for k, t in zip(("mean", "var", "std", "scale"), state[1:])})
    return (ret, adv, v, stats), out


def _deviation(got, ref):
    """max |got - ref| per quantity (NaN where both are NaN is no deviation; a NaN on one side only is infinite), and the floor of a
    meaningful deviation: half an fp32 ulp of the largest reference value"""
    out, floor = {}, {}
    for q in QUANTITIES:
        if q in STATS:
            g, w = np.array([got["stats"][STATS.index(q)]]), np.array([ref["stats"][STATS.index(q)]])
        elif q in ("mean", "var", "std", "scale"):
            if "state" not in ref:
                continue
            g, w = np.array([got[q]]), np.array([ref["state"][q]])
        elif q in ref and q in got:
            g, w = np.asarray(got[q]), np.asarray(ref[q])
        else:
            continue
        both = np.isnan(g) & np.isnan(w)
        d = np.where(both, 0.0, np.abs(g - w))
        out[q] = float(np.where(np.isnan(d), np.inf, d).max())
        big = np.abs(w[~np.isnan(w)])
        floor[q] = 0.5 * float(np.spacing(np.float32(big.max()))) if big.size else 0.0
    return out, floor


@pytest.mark.parametrize("T", [1, 2, 24, 64])
def test_entry_point_against_the_torch_loop_and_the_reference(T):
    M = _M()
    worst, failures = {}, []
    for N in SIZES_N:
        shape = {}                                                                               # per one-number quantity: (torch, entry point) maxima
        for pattern in R.PATTERNS:
            x = R.inputs(T, N, pattern)
            # raw mode: the returns are the torch loop's, bit for bit (the loop run on the device)
            (ret_t, _, _, _), tch = _run(M.gae_returns_torch, x, None)
            (ret_h, _, v_h, _), hip = _run(M.gae_returns_hip, x, None)
            assert torch.equal(ret_h, ret_t), (T, N, pattern)
            assert torch.equal(v_h, _dev(x)[1])                                                  # the stateless mode leaves the values alone
            ref = R.reference(*x)
            cases = [("raw", tch, hip, ref)]
            # with a state: two consecutive calls, so that the second merges into statistics that have moved
            st_t, st_h, rst = _state(), _state(), R.new_state()
            for call in range(2):
                xc = R.inputs(T, N, pattern, seed=call)
                ref = R.reference(*xc, state=rst)
                _, tch = _run(M.gae_returns_torch, xc, st_t)
                _, hip = _run(M.gae_returns_hip, xc, st_h)
                assert hip["count"] == ref["state"]["count"] == (call + 1) * T * N            # exact
                rst = ref["state"]
                cases.append((f"state{call}", tch, hip, ref))
            for name, tch, hip, ref in cases:
                (dt, floor), (dh, _) = _deviation(tch, ref), _deviation(hip, ref)
                for q in dh:
                    dt[q] = max(dt[q], floor[q])
                    w = worst.setdefault(q, {"torch": 0.0, "hip": 0.0, "ratio": 0.0})
                    w["torch"], w["hip"] = max(w["torch"], dt[q]), max(w["hip"], dh[q])
                    if q in SCALARS:
                        shape[q] = (max(shape.get(q, (0.0, 0.0))[0], dt[q]), max(shape.get(q, (0.0, 0.0))[1], dh[q]))
                        continue
                    if dh[q] > 0:
                        w["ratio"] = max(w["ratio"], dh[q] / dt[q] if dt[q] > 0 else float("inf"))
                    if not dh[q] <= 4.0 * dt[q]:
                        failures.append((T, N, pattern, name, q, dh[q], dt[q]))
        for q, (dt_max, dh_max) in shape.items():
            if dh_max > 0:
                worst[q]["ratio"] = max(worst[q]["ratio"], dh_max / dt_max if dt_max > 0 else float("inf"))
            if not dh_max <= 4.0 * dt_max:
                failures.append((T, N, "all patterns", "all calls", q, dh_max, dt_max))
    print(f"T = {T}: max deviation from the float64 reference per quantity (torch spelling, entry point, largest ratio):")
    for q, w in worst.items():
        print(f"    {q:10s} torch {w['torch']:.3e}  hip {w['hip']:.3e}  ratio {w['ratio']:.3f}")
    _PARITY[f"T{T}"] = worst
    out = os.environ.get("GRX_VALUE_NORM_PARITY_OUT")
    if out:
        with open(out, "w") as f:
            json.dump({"sizes_N": SIZES_N, "patterns": list(R.PATTERNS), "bound": "hip <= 4 x max(torch, half an fp32 ulp); arrays per case, one-number quantities per shape",
                       "max_abs_deviation_from_float64": _PARITY, "failures": [list(map(str, c)) for c in failures]}, f, indent=1)
    assert not failures, failures[:10]


def test_a_column_does_not_depend_on_the_batch():
    M = _M()
    T, N = 24, 1025
    x = R.inputs(T, N, "random")
    (ret, _, _, _), _ = _run(M.gae_returns_hip, x, None)
    vals = _dev(x)[1]
    for n in (0, 63, 64, 511, 1024):
        xn = (x[0][:, n:n + 1].copy(), x[1][:, n:n + 1].copy(), x[2][:, n:n + 1].copy(), x[3][n:n + 1].copy())
        (ret1, _, _, _), _ = _run(M.gae_returns_hip, xn, None)
        assert torch.equal(ret1[:, 0], ret[:, n]), n                                             # equal bytes
        assert torch.equal(ret1[:, 0] - vals[:, n], ret[:, n] - vals[:, n])                      # ... and so the raw advantage, returns - values


def test_repeated_calls_give_the_same_bytes():
    M = _M()
    for T, N in ((24, 1025), (64, 257)):
        x = R.inputs(T, N, "random")
        start = _state()
        start[0].fill_(777); start[1].fill_(8.5); start[2].fill_(3.0); start[3].fill_(3.0 ** 0.5); start[4].fill_(3.0 ** 0.5 + R.EPS)
        runs = []
        for _ in range(3):
            st = _state(start)
            tensors, _ = _run(M.gae_returns_hip, x, st)
            runs.append([t.clone() for t in tensors] + [t.clone() for t in st])
        for other in runs[1:]:
            assert all(torch.equal(a, b) for a, b in zip(runs[0], other)), (T, N)
        assert int(runs[0][4]) == 777 + T * N


def test_rejected_calls_write_nothing():
    lib = _lib()
    T, N = 4, 70
    r, v, d, lv = _dev(R.inputs(T, N, "random"))
    v0 = v.clone()
    S = 777.0
    ret, adv, vout = torch.full((T, N), S, device=DEV), torch.full((T, N), S, device=DEV), torch.full((T, N), S, device=DEV)
    stats = torch.full((4,), S, device=DEV)
    size = lib.grx_gae_partials_size(T, N)
    assert size > 0 and size == lib.grx_gae_partials_size(1, N) and lib.grx_gae_partials_size(0, N) == 0 and lib.grx_gae_partials_size(T, 0) == 0
    assert lib.grx_gae_partials_size(1 << 12, (1 << 12) + 1) == 0 and lib.grx_gae_partials_size(1 << 12, 1 << 12) > 0
    part = torch.full((size + 2,), S, device=DEV)
    count = torch.full((1,), 777, device=DEV, dtype=torch.int64)
    mean, var, std, scale = (torch.full((1,), S, device=DEV) for _ in range(4))
    base = dict(T=T, N=N, rewards=r.data_ptr(), values=v.data_ptr(), dones=d.data_ptr(), last=lv.data_ptr(), count=count.data_ptr(),
                mean=mean.data_ptr(), var=var.data_ptr(), std=std.data_ptr(), scale=scale.data_ptr(), returns=ret.data_ptr(),
                advantages=adv.data_ptr(), values_out=vout.data_ptr(), stats=stats.data_ptr(), partials=part.data_ptr())

    def call(**kw):
        a = dict(base, **kw)
        return lib.grx_gae_returns(a["T"], a["N"], a["rewards"], a["values"], a["dones"], a["last"], R.GAMMA, R.LAM, R.EPS, a["count"], a["mean"],
                                   a["var"], a["std"], a["scale"], a["returns"], a["advantages"], a["values_out"], a["stats"], a["partials"],
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert call(T=0) < 0 and call(N=0) < 0 and call(T=-1) < 0 and call(N=-3) < 0
    assert call(T=1 << 12, N=(1 << 12) + 1) < 0                                                  # T N > 2^24 (refused before anything is read)
    for name in ("rewards", "values", "dones", "last", "returns", "advantages", "values_out", "stats", "partials"):
        assert call(**{name: None}) < 0, name                                                    # a NULL required pointer
    for name in ("count", "mean", "var", "std", "scale"):
        assert call(**{name: None}) < 0, name                                                    # a partly NULL state
    assert call(count=None, mean=None, var=None, std=None) < 0
    assert call(partials=part.data_ptr() + 4) < 0                                                # misaligned
    assert call(returns=r.data_ptr()) < 0 and call(advantages=v.data_ptr()) < 0                  # outputs overlapping inputs
    assert call(returns=v.data_ptr() + 4 * (T * N - 1)) < 0 and call(stats=lv.data_ptr()) < 0
    assert call(values_out=v.data_ptr() + 4) < 0 and call(values_out=r.data_ptr()) < 0           # (only values_out == values is allowed)
    assert call(mean=r.data_ptr()) < 0 and call(partials=d.data_ptr()) < 0
    torch.cuda.synchronize()
    for t in (ret, adv, vout, stats, part, mean, var, std, scale):
        assert bool((t == S).all())
    assert int(count) == 777 and torch.equal(v, v0)
    assert call(values_out=v.data_ptr()) == 0                                                    # in place on the values: the runner's call
    torch.cuda.synchronize()
    assert int(count) == 777 + T * N and bool((vout == S).all()) and not torch.equal(v, v0) and not bool((ret == S).any())
    assert torch.allclose(v, (v0 - mean) / scale, atol=1e-6) and float(scale) == float(std + np.float32(R.EPS))


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


def _first_rollout(monkeypatch, mode, fused):
    """two iterations; what compute_returns of iteration 0 was given and what it left in the storage"""
    monkeypatch.setenv("GRX_GAE_FUSED", fused)
    M = _M()
    calls = {"hip": 0, "torch": 0}
    hip, tch = M.gae_returns_hip, M.gae_returns_torch
    monkeypatch.setattr(M, "gae_returns_hip", lambda *a, **k: (calls.__setitem__("hip", calls["hip"] + 1), hip(*a, **k))[1])
    monkeypatch.setattr(M, "gae_returns_torch", lambda *a, **k: (calls.__setitem__("torch", calls["torch"] + 1), tch(*a, **k))[1])
    _, runner = _make(None, ("--value_norm", mode))
    vn, snaps = runner.alg.value_norm, []
    inner = vn.compute_returns

    def snap(storage, last_values, gamma, lam, critic=None):
        given = [t.clone() for t in (storage.rewards, storage.values, storage.dones, last_values)]
        inner(storage, last_values, gamma, lam, critic=critic)
        snaps.append((given, [t.clone() for t in (storage.values, storage.returns, storage.advantages)], [t.clone() for t in vn.state()]))
    vn.compute_returns = snap
    runner.learn(num_learning_iterations=2)
    return snaps[0], dict(calls), runner


@pytest.mark.parametrize("mode", ["running", "popart"])
def test_the_fused_launches_and_the_torch_path_agree_through_the_runner(monkeypatch, mode):
    (given_a, left_a, state_a), calls_a, runner = _first_rollout(monkeypatch, mode, "1")
    (given_b, left_b, state_b), calls_b, _ = _first_rollout(monkeypatch, mode, "0")
    assert calls_a == {"hip": 2, "torch": 0} and calls_b == {"hip": 0, "torch": 2}
    assert all(torch.equal(a, b) for a, b in zip(given_a, given_b))                              # iteration 0's rollout does not depend on the path
    alg = runner.alg
    gamma, lam = alg.gamma, alg.lam
    x = [t.squeeze(-1).cpu().numpy() for t in given_a]
    ref = R.reference(*x, state=R.new_state(), gamma=gamma, lam=lam)
    n = lambda t: t.squeeze(-1).cpu().double().numpy()
    half_ulp = lambda w: 0.5 * float(np.spacing(np.float32(np.abs(w).max())))                  # (the floor of the module's docstring)
    for i, q in enumerate(("values", "returns", "advantages")):
        da, db = float(np.abs(n(left_a[i]) - ref[q]).max()), float(np.abs(n(left_b[i]) - ref[q]).max())
        print(f"{mode} {q}: deviation from float64 fused {da:.3e}, torch {db:.3e}")
        assert da <= 4.0 * max(db, half_ulp(ref[q])), (q, da, db)
    assert int(state_a[0]) == int(state_b[0]) == 8 * 64
    for k, a, b in zip(("mean", "var", "std", "scale"), state_a[1:], state_b[1:]):
        da, db = abs(float(a) - ref["state"][k]), abs(float(b) - ref["state"][k])
        print(f"{mode} {k}: deviation from float64 fused {da:.3e}, torch {db:.3e}")
        assert da <= 4.0 * max(db, half_ulp(ref["state"][k])), (k, da, db)
    assert isinstance(alg._graph, torch.cuda.CUDAGraph) and type(alg._gather).__name__ == "RowGather"   # PPO's captured step is what it was

    # the captured critic graph reads the statistics by address: after they have moved, a replay returns denormalise(critic(x))
    vn = alg.value_norm
    assert int(vn.count) == 2 * 8 * 64 and float(vn.mean) != 0.0 and alg._act_graph is not None
    ac = alg.actor_critic
    g = torch.Generator().manual_seed(11)
    obs, cobs = torch.randn(64, ac.num_actor_input, generator=g).to(DEV), torch.randn(64, ac.num_critic_input, generator=g).to(DEV)
    with torch.inference_mode():
        alg.act(obs, cobs)
        alg._join_critic()
        got = alg.transition.values.clone()
        plain = ac.evaluate(cobs)
        want = vn.denormalize(plain)
    assert alg._critic_graph is not None and got.shape == want.shape == (64, 1)
    tol = 1e-4 * float(vn.scale) * (1.0 + float(plain.abs().max())) + 1e-6 * abs(float(vn.mean))   # (the fused MLP forward against torch's GEMMs)
    assert float((got - want).abs().max()) <= tol
    assert float((got - plain).abs().max()) > 10 * tol                                          # ... and not the network's normalised output


def test_runner_saves_resumes_and_plays(tmp_path, monkeypatch):
    from wiki_grx_gym_amd.scripts.play import play
    from wiki_grx_gym_amd.utils import get_args, task_registry
    # (play() takes the registered config instance and writes to it: undone when the test ends)
    reg = task_registry.train_cfgs["GR1T1"]
    monkeypatch.setattr(reg.runner, "inference_only", False, raising=False)
    monkeypatch.setattr(reg.runner, "resume", reg.runner.resume)
    flags = ("--value_norm", "popart")
    _, runner = _make(tmp_path, flags)
    runner.learn(num_learning_iterations=2)
    tags = _tags(runner)
    assert len(tags["Train/value_norm_mean"]) == 2 and all(np.isfinite(v) for v in tags["Loss/value_function"] + tags["Train/value_norm_std"])
    ck = torch.load(os.path.join(runner.log_dir, "model_2.pt"), weights_only=False)
    assert set(ck) == {"model_state_dict", "optimizer_state_dict", "iter", "infos", "value_norm"} and ck["value_norm"]["mode"] == "popart"
    _, again = _make(tmp_path, (*flags, "--resume"))
    sd, sd2 = runner.alg.value_norm.state_dict(), again.alg.value_norm.state_dict()
    assert all(torch.equal(sd[k], sd2[k]) for k in sd) and again.current_learning_iteration == 2
    again.learn(num_learning_iterations=1)
    assert int(again.alg.value_norm.count) == 3 * 8 * 64
    with pytest.raises(ValueError, match="--value_norm popart"):
        _make(tmp_path, ("--resume", "--load_run", os.path.basename(runner.log_dir)))           # a training run without the flag
    out = play(get_args(["--task", "GR1T1", "--headless", "--seed", "3", "--load_run", os.path.basename(runner.log_dir)]), steps=10,
               log_root=str(tmp_path))                                                           # play: the actor alone, the entry is ignored
    assert len(open(out["states"]).readlines()) == 10 and out["runner"].alg.value_norm is None


@pytest.mark.parametrize("flags", [("--precision", "bf16"), ("--symmetry", "both"), ("--smooth", "both"), ("--rnd",), ("--estimator",),
                                   ("--obs_history", "3", "--empirical_normalization"), ("--noise_std_type", "log")],
                         ids=lambda f: f[0].lstrip("-"))
def test_compositions_train_on_the_device(tmp_path, flags):
    _, runner = _make(tmp_path, ("--value_norm", "popart", *flags))
    runner.learn(num_learning_iterations=1)
    tags = _tags(runner)
    assert all(np.isfinite(tags[t][0]) for t in ("Loss/value_function", "Loss/surrogate", "Train/value_norm_mean", "Train/value_norm_std"))
    assert all(bool(torch.isfinite(p).all()) for p in runner.alg.actor_critic.parameters())
    assert int(runner.alg.value_norm.count) == 8 * 64


def test_default_path_runs_nothing_of_it(monkeypatch):
    _, plain = _make(None)
    plain.learn(num_learning_iterations=1)
    want = [p.detach().clone() for p in plain.alg.actor_critic.parameters()]
    M = _M()

    def boom(*a, **k):
        raise AssertionError("value normalisation ran without --value_norm")
    monkeypatch.setattr(M, "gae_returns_hip", boom)
    monkeypatch.setattr(M, "gae_returns_torch", boom)
    monkeypatch.setattr(M.ValueNormalizer, "__init__", boom)
    monkeypatch.setattr(_lib(), "grx_gae_returns", boom)
    _, patched = _make(None)
    patched.learn(num_learning_iterations=1)
    assert patched.alg.value_norm is None and isinstance(patched.alg._graph, torch.cuda.CUDAGraph)
    assert all(torch.equal(a, b) for a, b in zip(want, patched.alg.actor_critic.parameters()))   # bit for bit
    with pytest.raises(AssertionError, match="without --value_norm"):
        _make(None, ("--value_norm", "running"))                                                 # (the patch does bite with the flag)
