"""Constraints as terminations on the GPU (include/grx_ppo_cat.h: grx_cat_step, grx_cat_returns; rl/constraints.py): the step
pass against the torch spelling run on the CPU, byte for byte over consecutive steps; its independence of the envs' order; the returns
against grx_gae_returns and the torch loop, byte for byte, and their advantages and statistics against float64; the argument checks with
sentinels; and the runner on the HIP device -- fused against GRX_CAT_FUSED=0, save / load / play / export, the default path.

GRX_CAT_PARITY_JSON=<path>: the parity test also writes its per-case error ratios there (profiles/constraints_parity.json is such a file)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import constraints_ref as R
from tests import mc_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS, AS, TS = (1, 63, 65, 130), (1, 10, 32), (1, 2, 5)
ALL = (("torque", None), ("dof_vel", None), ("dof_pos", None), ("action_rate", 0.4), ("upright", 0.35))
RUN_SPEC = "torque:0.05..0.25,dof_vel:0.05..0.25,dof_pos:0.25,action_rate:0.25@0.5,upright:1.0@0.7"
SENTINEL = 777.0


def _K():
    from wiki_grx_gym_amd.rl import constraints
    return constraints


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _d(a):
    return (_t(a) if isinstance(a, np.ndarray) else a).to(DEV)


def _full(*shape, dtype=torch.float32):
    return torch.full(shape, SENTINEL, device=DEV, dtype=dtype)


def _same_bytes(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.fixture(scope="module")
def parity():
    rows = {}
    yield rows
    path = os.environ.get("GRX_CAT_PARITY_JSON")
    if path and rows:
        with open(path, "w") as f:
            json.dump({"margin": mc_ref.MARGIN, "what": "max |kernel - float64| over the tensor, divided by e32 = max |the fp32 torch spelling on "
                       "the CPU - float64| of the same operation (at least u max |float64|); tests/mc_ref.py held()", "cases": rows}, f, indent=1)


def _hold(parity, case, name, got, spelled, want):
    err, e32, ratio = mc_ref.held(got.detach().cpu().double().numpy(), spelled.detach().cpu().double().numpy(), want)
    parity[f"{case},{name}"] = {"e32": e32, "error": err, "ratio": round(ratio, 3)}
    print(f"{case} {name}: error {err:.3g}, e32 {e32:.3g}, ratio {ratio:.3g}")
    assert err <= mc_ref.MARGIN * e32, (case, name, err, e32, ratio)


# ---- grx_cat_step --------------------------------------------------------------------------------------------------------------------------------
def _tables(families, D, A, lims):
    """the same column table on the CPU and on the device"""
    K = _K()
    spec = K.ConstraintSpec([(n, 0.5, 0.5, lim) for n, lim in families])
    return [K.ColumnTable(spec, D, A, lims[0], lims[1], lims[2], 0.9, 0.95, dev) for dev in ("cpu", DEV)]


class _State:
    def __init__(self, table, N, A, dev):
        self.prev = torch.zeros(N, A, device=dev) if 3 in table.kinds else None
        self.c_max, self.counts = torch.zeros(table.C, device=dev), torch.zeros(table.F, dtype=torch.int32, device=dev)


def _src(table, src, to):
    """the five sources, None for a family the table does not hold"""
    return [to(src[n]) if k in table.kinds else None for k, n in enumerate(("torques", "dof_vel", "dof_pos", "actions", "gravity"))]


def _three_steps(families, N, D, A, clip_zero, perm=None, steps=3, tau=0.95, soa=False):
    """`steps` consecutive steps of the same inputs through the torch spelling on the CPU and through grx_cat_step; per step
    ((delta, row, c_max, prev, counts) of the spelling, the same of the kernel).  `perm`: the envs' order on the device side; `soa`: the
    device's sources are (N, k) views with strides (1, N), as the env publishes its state"""
    K = _K()
    lims = R.limits(D)
    cpu_table, dev_table = _tables(families, D, A, lims)
    g = np.random.default_rng(3 * N + A)
    prob = g.uniform(0.1, 1.0, cpu_table.C).astype(np.float32)
    tau32 = torch.tensor(tau, dtype=torch.float32)
    tau_f, omt_f = tau32.item(), (torch.tensor(1.0) - tau32).item()
    a, b = _State(cpu_table, N, A, "cpu"), _State(dev_table, N, A, DEV)
    p = np.arange(N) if perm is None else perm
    out = []
    for k in range(steps):
        src, dones = R.sources(N, D, A, lims, 0.4, 0.35, k, quiet_column=0)
        row = g.uniform(-0.05, 0.1, N).astype(np.float32)
        delta_a, row_a = torch.zeros(N), _t(row).clone()
        K.cat_step_torch(cpu_table, _t(prob), *_src(cpu_table, src, _t), _t(dones), tau_f, omt_f, clip_zero, k == 0, a.prev, a.c_max, a.counts,
                         delta_a, row_a)
        delta_b, row_b = _full(N), _d(row[p])
        to_dev = (lambda x: _d(np.ascontiguousarray(x[p].T)).t()) if soa else (lambda x: _d(x[p]))
        K.cat_step_hip(dev_table, _d(prob), *_src(dev_table, src, to_dev), _d(dones[p]), tau_f, omt_f, clip_zero, k == 0, b.prev,
                       b.c_max, b.counts, delta_b, row_b)
        torch.cuda.synchronize()
        out.append(((delta_a, row_a, a.c_max.clone(), None if a.prev is None else a.prev.clone(), a.counts.clone()),
                    (delta_b.cpu(), row_b.cpu(), b.c_max.cpu(), None if b.prev is None else b.prev.cpu(), b.counts.cpu())))
    return out, cpu_table


CASES = [(ALL, "all five"), (ALL[:1] + ALL[2:], "no dof_vel"), (ALL[3:], "action_rate and upright"), ((("upright", 0.35),), "C = 1"),
         ((("action_rate", 0.4),), "action_rate alone")]


@pytest.mark.parametrize("A", AS)
@pytest.mark.parametrize("families, what", CASES)
def test_step_is_the_torch_spelling_byte_for_byte(families, what, A):
    """delta, the reward row, c_max, prev and the counters over three consecutive steps (the running maxima and the previous actions carry
    over), every N, both clip modes, row-major and SoA sources: some rows are done, DOF 0's columns are never violated, roughly a tenth of the entries violate"""
    violated = 0
    for N in NS:
        for clip_zero in (True, False):
            steps, table = _three_steps(families, N, A, A, clip_zero, soa=not clip_zero)   # (both layouts, both clips)
            if families is ALL:
                assert table.C == 3 * A + A + 1                                                    # 5, 41, 129
            for k, (want, got) in enumerate(steps):
                for name, x, y in zip(("delta", "row", "c_max", "prev", "counts"), want, got):
                    assert (x is None and y is None) or _same_bytes(x, y), (what, N, A, clip_zero, k, name)
                quiet = [c for c in range(table.C) if int(table.kind[c]) in (0, 1, 2) and int(table.src[c]) == 0]
                assert all(float(got[2][c]) == 0.0 for c in quiet) and bool(torch.isfinite(got[0]).all())
            violated += int(steps[-1][1][4].sum())
            assert bool((steps[-1][1][0] <= 1).all()) and bool((steps[-1][1][0] >= 0).all())
    assert violated > 0                                                                            # (the inputs do violate)


def test_an_envs_probability_depends_on_the_others_through_the_maxima_alone():
    """the envs permuted: c_max and the counters are unchanged, delta, the reward row and prev permute with the envs"""
    for N, A in ((65, 10), (130, 32), (63, 1)):
        perm = np.random.default_rng(N).permutation(N)
        plain, _ = _three_steps(ALL, N, A, A, True)
        mixed, _ = _three_steps(ALL, N, A, A, True, perm=perm)
        for k in range(3):
            delta, row, c_max, prev, counts = plain[k][1]
            delta_p, row_p, c_max_p, prev_p, counts_p = mixed[k][1]
            assert _same_bytes(c_max, c_max_p) and _same_bytes(counts, counts_p), (N, A, k)
            assert _same_bytes(delta[perm], delta_p) and _same_bytes(row[perm], row_p) and _same_bytes(prev[perm], prev_p), (N, A, k)
        assert float(plain[-1][1][0].max()) > 0


# ---- grx_cat_returns -----------------------------------------------------------------------------------------------------------------------------
def _returns(r, v, d, p, last):
    K = _K()
    T, N = r.shape
    ret, adv = _full(T, N), _full(T, N)
    stats = K.cat_returns_hip(_d(r), _d(v), _d(d), _d(p), _d(last), R.GAMMA, R.LAM, ret, adv)
    torch.cuda.synchronize()
    return ret, adv, stats


def test_zero_probabilities_are_grx_gae_returns_byte_for_byte():
    from wiki_grx_gym_amd.rl.value_norm import gae_returns_hip
    for T in TS:
        for N in NS:
            r, v, d, _, last = R.rollout(T, N)
            ret, adv, stats = _returns(r, v, d, np.zeros((T, N), np.float32), last)
            want_ret, want_adv = _full(T, N), _full(T, N)
            want_stats = gae_returns_hip(_d(r), _d(v), _d(d), _d(last), R.GAMMA, R.LAM, 1e-5, None, want_ret, want_adv)
            torch.cuda.synchronize()
            assert _same_bytes(ret, want_ret) and _same_bytes(adv, want_adv) and _same_bytes(stats, want_stats), (T, N)
            assert bool(torch.isnan(adv).all()) == (T * N == 1)                                    # T N = 1: the NaN torch.std gives


def test_returns_are_the_torch_loops_and_the_advantages_hold_against_float64(parity):
    """random probabilities in [0, 1] with exact zeros and ones: the returns equal the torch loop's (run on the CPU) bit for bit; the
    advantages and the statistics are held by tests/test_multi_critic_gpu.py's yardstick -- the kernel's distance from float64 against the
    fp32 torch spelling's own, with that test's margin"""
    K = _K()
    for T in TS:
        for N in NS:
            r, v, d, p, last = R.rollout(T, N)
            assert (p == 0).any() or T * N < 4
            ret32, adv32, stats32 = torch.zeros(T, N), torch.zeros(T, N), torch.zeros(4)
            K.cat_returns_torch(_t(r), _t(v), _t(d), _t(p), _t(last), R.GAMMA, R.LAM, ret32, adv32, stats32)
            ret, adv, stats = _returns(r, v, d, p, last)
            assert _same_bytes(ret, ret32), (T, N)
            if T * N == 1:
                assert bool(torch.isnan(adv).all())
                continue
            want_adv, want_stats = R.advantages(R.returns(r, v, d, p, last), v)
            case = f"returns,{T}x{N}"
            _hold(parity, case, "advantages", adv, adv32, want_adv)
            for i, name in enumerate(("mean_a", "std_a", "mean_returns", "var_returns")):
                _hold(parity, case, name, stats[i], stats32[i], want_stats[i])


def test_an_envs_returns_do_not_depend_on_its_neighbours():
    r, v, d, p, last = R.rollout(5, 130)
    ret, _, _ = _returns(r, v, d, p, last)
    for n in (0, 63, 64, 129):
        alone, _, _ = _returns(r[:, n:n + 1].copy(), v[:, n:n + 1].copy(), d[:, n:n + 1].copy(), p[:, n:n + 1].copy(), last[n:n + 1].copy())
        assert _same_bytes(ret[:, n:n + 1], alone), n


# ---- invalid arguments leave sentinel-filled outputs untouched ----------------------------------------------------------------------------------
def test_invalid_arguments_write_nothing():
    K = _K()
    lib = K._lib()
    N, A, T = 65, 10, 2
    lims = R.limits(A)
    _, table = _tables(ALL, A, A, lims)
    src, dones = R.sources(N, A, A, lims, 0.4, 0.35, 0)
    ptr = lambda t: t.data_ptr() if t is not None else None
    untouched = lambda *ts: all(bool((t == (SENTINEL if t.dtype.is_floating_point else int(SENTINEL))).all()) for t in ts)
    t = {"kind": table.kind, "src": table.src, "family": table.family, "lo": table.lo, "hi": table.hi, "prob": _d(np.full(table.C, 0.5, np.float32)),
         "torques": _d(src["torques"]), "dof_vel": _d(src["dof_vel"]), "dof_pos": _d(src["dof_pos"]), "actions": _d(src["actions"]),
         "gravity": _d(src["gravity"]), "dones": _d(dones)}
    nb = lib.grx_cat_step_blocks(N)
    o = {"prev": _full(N, A), "c_max": _full(table.C), "counts": _full(table.F, dtype=torch.int32), "cplus": _full(N, table.C),
         "part_max": _full(nb, table.C), "part_count": _full(nb, table.F, dtype=torch.int32), "delta": _full(N), "row": _full(N)}
    ins, outs = tuple(t), tuple(o)

    def step(N_=N, C_=table.C, F_=table.F, D_=A, A_=A, kinds_=table.kind_mask, **kw):
        a = {**t, **o, **kw}
        return lib.grx_cat_step(N_, C_, F_, D_, A_, kinds_, *[ptr(a[n]) for n in ins[:-1]], a.get("strides"), ptr(a["dones"]), 0.95, 0.05, 1, 1, *[ptr(a[n]) for n in outs], None)
    for rc in (step(N_=0), step(C_=0), step(C_=257), step(F_=0), step(F_=9), step(kinds_=0), step(kinds_=32), step(D_=0), step(A_=0),
               *[step(**{n: None}) for n in ins + outs],
               step(row=o["delta"]), step(delta=t["dones"]), step(c_max=t["prob"]), step(prev=t["actions"]), step(cplus=t["torques"]),
               step(counts=t["family"]), step(part_max=o["cplus"])):
        assert rc < 0
    torch.cuda.synchronize()
    assert untouched(*o.values())
    assert step() == 0
    torch.cuda.synchronize()
    assert not untouched(o["delta"]) and not untouched(o["row"]) and not untouched(o["c_max"]) and not untouched(o["counts"])
    # grx_cat_returns
    r, v, d, p, last = (_d(x) for x in R.rollout(T, N))
    ret, adv, stats = _full(T, N), _full(T, N), _full(4)
    part = _full(lib.grx_cat_partials_size(T, N) + 2)
    rets = lambda T_=T, N_=N, r_=r, v_=v, d_=d, p_=p, last_=last, ret_=ret, adv_=adv, stats_=stats, part_=ptr(part): lib.grx_cat_returns(
        T_, N_, ptr(r_), ptr(v_), ptr(d_), ptr(p_), ptr(last_), R.GAMMA, R.LAM, ptr(ret_), ptr(adv_), ptr(stats_), part_, None)
    for rc in (rets(T_=0), rets(N_=0), rets(T_=1 << 13, N_=1 << 12), rets(r_=None), rets(v_=None), rets(d_=None), rets(p_=None),
               rets(last_=None), rets(ret_=None), rets(adv_=None), rets(stats_=None), rets(part_=None), rets(part_=ptr(part) + 4),
               rets(ret_=v), rets(adv_=r), rets(ret_=p), rets(adv_=ret)):
        assert rc < 0
    torch.cuda.synchronize()
    assert untouched(ret, adv, stats, part)
    assert rets() == 0
    torch.cuda.synchronize()
    assert not untouched(ret) and not untouched(adv)


# ---- the runner on the HIP device ----------------------------------------------------------------------------------------------------------------
def _make(tmp_path, flags=("--constraints", RUN_SPEC), steps=8, num_envs=64, epochs=2):
    from wiki_grx_gym_amd.envs import GR1T1Cfg, GR1T1CfgPPO
    from wiki_grx_gym_amd.utils import get_args, task_registry
    args = get_args(["--task", "GR1T1", "--headless", "--num_envs", str(num_envs), "--seed", "3", *flags])
    env, _ = task_registry.make_env("GR1T1", args=args, env_cfg=GR1T1Cfg())
    tcfg = GR1T1CfgPPO()
    tcfg.runner.num_steps_per_env = steps
    tcfg.algorithm.num_mini_batches, tcfg.algorithm.num_learning_epochs = 4, epochs
    runner, _ = task_registry.make_alg_runner(env, name=None, args=args, train_cfg=tcfg, log_root=str(tmp_path) if tmp_path else None)
    return env, runner


def _state(alg):
    return [t.detach().clone() for p in alg.actor_critic.parameters() for t in
            (p, alg.optimizer.state[p]["exp_avg"], alg.optimizer.state[p]["exp_avg_sq"])]


def test_fused_against_the_torch_spelling_through_the_runner(tmp_path, monkeypatch):
    """GR1T1, 64 envs, 8 steps, 2 epochs, the same seed with the two entries and with GRX_CAT_FUSED=0: storage.rewards, delta, returns and
    advantages of the first rollout byte for byte, and the parameters after the update.  (The action-rate limit of 0.5 is below the spread
    of an untrained policy's action differences, N(0, 2 sigma^2) with sigma = 1: most rows violate it)"""
    got = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("GRX_CAT_FUSED", fused)
        _, runner = _make(None, flags=("--constraints", RUN_SPEC, "--constraint_ramp_its", "4"))
        alg = runner.alg
        snap = {}
        update = alg.update

        def snap_then_update():
            st, c = alg.storage, alg.constraints
            snap.update(rewards=st.rewards.clone(), delta=c.term_prob.clone(), returns=st.returns.clone(), adv=st.advantages.clone(),
                        c_max=c.c_max.clone(), counts=c.counts.clone(), prev=c.prev.clone())
            return update()
        alg.update = snap_then_update
        runner.learn(num_learning_iterations=1)
        torch.cuda.synchronize()
        got[fused] = ({k: v.cpu() for k, v in snap.items()}, [t.cpu() for t in _state(alg)])
    (a, pa), (b, pb) = got["1"], got["0"]
    for name in ("rewards", "delta", "c_max", "counts", "prev", "returns", "adv"):
        same = _same_bytes(a[name], b[name])
        diff = (a[name].double() - b[name].double()).abs().max().item()
        print(f"{name}: byte-equal {same}, max |fused - spelling| {diff:.3g}")
    assert float(a["delta"].max()) > 0 and float(a["delta"].max()) <= 1.0
    for name in ("rewards", "delta", "c_max", "counts", "prev", "returns", "adv"):
        assert _same_bytes(a[name], b[name]), name
    assert all(_same_bytes(x, y) for x, y in zip(pa, pb))


def test_train_save_load_play_and_export(tmp_path):
    from wiki_grx_gym_amd.scripts.play import play
    from wiki_grx_gym_amd.utils import get_args
    K = _K()
    flags = ("--constraints", RUN_SPEC, "--constraint_ramp_its", "4")
    _, runner = _make(tmp_path, flags=flags)
    runner.learn(num_learning_iterations=2)
    tags = {}
    for line in open(os.path.join(runner.log_dir, "scalars.jsonl")):
        tags.setdefault(line.split('"tag": "')[1].split('"')[0], []).append(float(line.split('"value": ')[1].split(",")[0]))
    names = ["mean_termination_prob"] + [f + s for f in K.FAMILIES for s in ("_violation_rate", "_max")]
    assert sorted(t for t in tags if t.startswith("Constraint/")) == sorted("Constraint/" + n for n in names)
    assert all(len(tags["Constraint/" + n]) == 2 and all(np.isfinite(x) for x in tags["Constraint/" + n]) for n in names)
    assert tags["Constraint/action_rate_violation_rate"][0] > 0 and tags["Constraint/mean_termination_prob"][1] > 0
    c = runner.alg.constraints
    ck = torch.load(os.path.join(runner.log_dir, "model_2.pt"), weights_only=False)
    assert set(ck) == {"model_state_dict", "optimizer_state_dict", "iter", "infos", "constraints"}
    assert ck["constraints"]["spec"] == c.spec.key() and torch.equal(ck["constraints"]["c_max"], c.c_max.cpu())
    _, again = _make(None, flags=flags)
    again.load(os.path.join(runner.log_dir, "model_2.pt"))
    assert all(torch.equal(v, again.alg.actor_critic.state_dict()[k]) for k, v in ck["model_state_dict"].items() if k != "std")
    assert torch.equal(again.alg.constraints.c_max, c.c_max) and again.current_learning_iteration == 2
    again.learn(num_learning_iterations=1)                                                          # ... and trains on
    _, plain = _make(None, flags=())
    with pytest.raises(ValueError, match="--constraints"):
        plain.load(os.path.join(runner.log_dir, "model_2.pt"))
    out = play(get_args(["--task", "GR1T1", "--headless", "--seed", "3"]), steps=10, log_root=str(tmp_path))   # no flag: the actor alone
    prunner, penv = out["runner"], out["env"]
    assert prunner.alg.constraints is None and len(open(out["states"]).readlines()) == 10
    loaded = prunner.alg.actor_critic.state_dict()
    assert all(torch.equal(v.to(loaded[k].device), loaded[k]) for k, v in ck["model_state_dict"].items() if k.startswith("actor."))
    frames = penv.get_observations().detach().clone()
    jit = torch.jit.load(out["exported"])
    with torch.no_grad():
        want = prunner.alg.actor_critic.actor.model(frames).cpu()
        assert torch.allclose(jit(frames.cpu()), want, atol=1e-5, rtol=1e-5)


def test_default_run_is_what_it_was_and_launches_nothing_new(tmp_path, monkeypatch):
    """two iterations without the flag, against the same run whose PPO gets the new keywords at their defaults: parameters bit for bit; the
    grx_cat_* prototypes are never bound and none of the entries is called (counting stubs on the loaded library)"""
    import wiki_grx_gym_amd.rl.runner as RR
    from wiki_grx_gym_amd.rl.fused_loss import load_ppo_library
    K = _K()
    lib = load_ppo_library()
    calls = {}

    def counting(name):
        real = getattr(lib, name)

        def stub(*a):
            calls[name] = calls.get(name, 0) + 1
            return real(*a)
        return stub
    for name in ("grx_cat_step", "grx_cat_step_blocks", "grx_cat_returns", "grx_cat_partials_size"):
        monkeypatch.setattr(lib, name, counting(name))
    monkeypatch.setattr(K, "_BOUND", None)
    _, first = _make(tmp_path / "a", flags=())
    first.learn(num_learning_iterations=2)
    plain_ppo = RR._ALGORITHMS["PPO"]
    monkeypatch.setitem(RR._ALGORITHMS, "PPO", lambda **k: plain_ppo(constraints=None, constraint_tau=0.95, constraint_ramp_its=1000,
                                                                      constraint_reward_clip="zero", **k))
    _, second = _make(tmp_path / "b", flags=())
    second.learn(num_learning_iterations=2)
    torch.cuda.synchronize()
    assert first.alg.constraints is None and second.alg.constraints is None and K._BOUND is None and calls == {}
    assert all(torch.equal(a, b) for a, b in zip(_state(first.alg), _state(second.alg)))
    ck = torch.load(os.path.join(first.log_dir, "model_2.pt"), weights_only=False)
    assert set(ck) == {"model_state_dict", "optimizer_state_dict", "iter", "infos"}
    monkeypatch.setattr(K, "_BOUND", lib)                                                          # (the stubs do count once an entry is used)
    assert K.cat_partials(2, 65, DEV).numel() == 24 and calls == {"grx_cat_partials_size": 1}
