"""What the concurrent state estimator (--estimator) costs per PPO iteration, and whether its one-launch rollout forward
(grx_est_forward) costs less collection time than the per-layer path (GRX_EST_FUSED=0: a grx_mlp_layer launch per layer, a concatenation
and a column select).  Nothing here is a target.  full_iteration as bench.py defines it -- OnPolicyRunner.learn(1) of a GR1T1 run at 4096
envs with the registered task's PPO configuration, timers synchronised at both ends and at the collection / learning boundary, the median
of five iterations after two warm-up iterations (graph captures, allocator) -- for three arms: no flag (the yardstick: what the code does
without the option), --estimator with the fused launch, --estimator with GRX_EST_FUSED=0.  The arms ALTERNATE: `runs` rounds, each arm once
per round in a fresh env and runner.  `summary` holds, per arm, the median and the min / max over the rounds of each figure.
    python tools/estimator_time.py [runs=3] [out=profiles/estimator_step_time.json]   (the JSON line is printed too)"""
import gc, json, os, statistics, sys; sys.path.insert(0, ".")
import torch
from wiki_grx_gym_amd.envs import GR1T1Cfg, GR1T1CfgPPO
runs = int(sys.argv[1]) if len(sys.argv) > 1 else 3
assert torch.cuda.is_available(), "estimator_time.py measures on the GPU: there is no fallback"
ARMS = {"default": ((), "1"), "estimator_fused": (("--estimator",), "1"), "estimator_per_layer": (("--estimator",), "0")}


def full_iteration(flags, fused):
    from wiki_grx_gym_amd.utils import get_args, task_registry
    os.environ["GRX_EST_FUSED"] = fused                            # (read when the estimator is constructed)
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
            "min_max_ms": [round(ts[0][0] * 1e3, 2), round(ts[-1][0] * 1e3, 2)], "captured": captured,
            "estimator_fused": bool(runner.estimator._fused) if runner.estimator is not None else None}


rows = []
for run in range(1, runs + 1):
    for arm, (flags, fused) in ARMS.items():
        rows.append({"what": "full_iteration", "arm": arm, "run": run, "flags": list(flags), "GRX_EST_FUSED": fused, "envs": 4096,
                     **full_iteration(flags, fused)})
        print(rows[-1], flush=True)
        gc.collect()
summary = {}
for arm in ARMS:
    mine = [r for r in rows if r["arm"] == arm]
    summary[arm] = {k: {"median": round(statistics.median(r[k] for r in mine), 2), "min_max": [min(r[k] for r in mine), max(r[k] for r in mine)]}
                    for k in ("median_ms", "collection_ms", "learning_ms")}
out = sys.argv[2] if len(sys.argv) > 2 else "profiles/estimator_step_time.json"
doc = {"what": "tools/estimator_time.py on one MI355X", "runs_per_arm": runs, "summary": summary, "rows": rows}
os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
with open(out, "w") as f:
    json.dump(doc, f, indent=1)
print(json.dumps(doc))
