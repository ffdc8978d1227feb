"""What value normalisation (--value_norm) costs per PPO iteration, and what compute_returns alone takes on its three paths.
Nothing here is a target.
  full_iteration as bench.py defines it -- OnPolicyRunner.learn(1) of a GR1T1 run at 4096 envs with the registered task's PPO configuration,
    timers synchronised at both ends and at the collection / learning boundary, the median of five iterations after two warm-up iterations
    (graph captures, allocator) -- for three arms: no flag (the yardstick), --value_norm running with the three fused launches,
    --value_norm running with GRX_GAE_FUSED=0.  The arms ALTERNATE: `runs` rounds, each arm once per round in a fresh env and runner.
  compute_returns alone, on tensors of the run's shape (T = num_steps_per_env, N = 4096; rewards in [0, 0.1], values around 10): the default
    path's RolloutStorage.compute_returns (storage.py is what the parent commit has: the torch loop), grx_gae_returns with a state (three
    launches) and gae_returns_torch with a state (GRX_GAE_FUSED=0's path).  Device events around `reps` back-to-back calls after a warm-up,
    the three paths alternating over `runs` rounds in one process; microseconds per call.
`summary` holds, per arm, the median and the min / max over the rounds of each figure.
    python tools/value_norm_time.py [runs=3] [out=profiles/value_norm_step_time.json]   (the JSON line is printed too)"""
import gc, json, os, statistics, sys; sys.path.insert(0, ".")
import torch
from wiki_grx_gym_amd.envs import GR1T1Cfg, GR1T1CfgPPO
runs = int(sys.argv[1]) if len(sys.argv) > 1 else 3
assert torch.cuda.is_available(), "value_norm_time.py measures on the GPU: there is no fallback"
ARMS = {"default": ((), "1"), "value_norm_fused": (("--value_norm", "running"), "1"), "value_norm_torch": (("--value_norm", "running"), "0")}
DEV = "cuda:0"


def full_iteration(flags, fused):
    from wiki_grx_gym_amd.utils import get_args, task_registry
    os.environ["GRX_GAE_FUSED"] = fused                            # (read at every compute_returns)
    args = get_args(["--task", "GR1T1", "--headless", "--num_envs", "4096", "--seed", "1", *flags])
    env, _ = task_registry.make_env("GR1T1", args=args, env_cfg=GR1T1Cfg())
    runner, _ = task_registry.make_alg_runner(env, name=None, args=args, train_cfg=GR1T1CfgPPO(), log_root=None)
    runner.sync_timers = True
    runner.learn(2)                                                # graph captures, allocator
    ts = []
    for _ in range(5):
        runner.learn(1)
        ts.append((runner.last_collection_time + runner.last_learn_time, runner.last_collection_time, runner.last_learn_time))
    ts.sort()
    alg = runner.alg
    captured = bool(alg._use_graph and alg._graph is not None and alg._use_act_graph and alg._act_graph is not None)
    return {"median_ms": round(ts[2][0] * 1e3, 2), "collection_ms": round(ts[2][1] * 1e3, 2), "learning_ms": round(ts[2][2] * 1e3, 2),
            "min_max_ms": [round(ts[0][0] * 1e3, 2), round(ts[-1][0] * 1e3, 2)], "captured": captured}


def returns_alone(rounds, reps=50):
    from wiki_grx_gym_amd.rl import value_norm as V
    from wiki_grx_gym_amd.rl.storage import RolloutStorage
    T, N = int(GR1T1CfgPPO.runner.num_steps_per_env), 4096
    g = torch.Generator(device=DEV).manual_seed(1)
    st = RolloutStorage(N, T, [1], [1], [1], DEV)
    rewards, values = 0.1 * torch.rand(T, N, 1, device=DEV, generator=g), 10.0 + 5.0 * torch.randn(T, N, 1, device=DEV, generator=g)
    st.rewards.copy_(rewards); st.dones.copy_((torch.rand(T, N, 1, device=DEV, generator=g) < 0.02).to(torch.uint8))
    last = 10.0 + 5.0 * torch.randn(N, 1, device=DEV, generator=g)
    vn = V.ValueNormalizer("running", 1e-5, DEV)
    stats, part = torch.zeros(4, device=DEV), V.gae_partials(T, N, DEV)

    def default():
        st.compute_returns(last, 0.994, 0.9)

    def fused():
        V.gae_returns_hip(st.rewards, st.values, st.dones, last, 0.994, 0.9, vn.eps, vn.state(), st.returns, st.advantages, None, stats, part)

    def spelled():
        V.gae_returns_torch(st.rewards, st.values, st.dones, last, 0.994, 0.9, vn.eps, vn.state(), st.returns, st.advantages)
    paths, rows = {"default_torch_loop": default, "value_norm_fused": fused, "value_norm_torch": spelled}, []
    with torch.inference_mode():
        for rnd in range(1, rounds + 1):
            for name, fn in paths.items():
                st.values.copy_(values)                            # (the paths with a state normalise the values in place)
                for _ in range(5):
                    fn()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(); a.record()
                for _ in range(reps):
                    fn()
                b.record(); torch.cuda.synchronize()
                rows.append({"what": "compute_returns_alone", "arm": name, "run": rnd, "T": T, "envs": N, "reps": reps,
                             "us_per_call": round(a.elapsed_time(b) * 1e3 / reps, 2)})
                print(rows[-1], flush=True)
    return rows


rows = []
for run in range(1, runs + 1):
    for arm, (flags, fused) in ARMS.items():
        rows.append({"what": "full_iteration", "arm": arm, "run": run, "flags": list(flags), "GRX_GAE_FUSED": fused, "envs": 4096,
                     **full_iteration(flags, fused)})
        print(rows[-1], flush=True)
        gc.collect()
alone = returns_alone(runs)
summary = {}
for arm in ARMS:
    mine = [r for r in rows if r["arm"] == arm]
    summary[arm] = {k: {"median": round(statistics.median(r[k] for r in mine), 2), "min_max": [min(r[k] for r in mine), max(r[k] for r in mine)]}
                    for k in ("median_ms", "collection_ms", "learning_ms")}
summary["compute_returns_alone_us"] = {}
for arm in sorted({r["arm"] for r in alone}):
    us = [r["us_per_call"] for r in alone if r["arm"] == arm]
    summary["compute_returns_alone_us"][arm] = {"median": round(statistics.median(us), 2), "min_max": [min(us), max(us)]}
out = sys.argv[2] if len(sys.argv) > 2 else "profiles/value_norm_step_time.json"
doc = {"what": "tools/value_norm_time.py on one MI355X", "runs_per_arm": runs, "summary": summary, "rows": rows + alone}
os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
with open(out, "w") as f:
    json.dump(doc, f, indent=1)
print(json.dumps(doc))
