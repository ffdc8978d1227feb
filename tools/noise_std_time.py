"""What the action-noise options (--noise_std_type log, --state_dependent_std) cost per PPO iteration.  Nothing here is a
target.  full_iteration as bench.py defines it -- OnPolicyRunner.learn(1) of a GR1T1 run at 4096 envs with the registered task's PPO
configuration, timers synchronised at both ends and at the collection / learning boundary, the median of five iterations after two
warm-up iterations (graph captures, allocator) -- for the default, `log`, the state-dependent sigma and both together.  The arms ALTERNATE:
`runs` rounds, each arm once per round in a fresh env and runner; the comparison arm is the default on the same commit.
    python tools/noise_std_time.py [runs=3] [out=profiles/noise_std_step_time.json]   (the JSON line is printed too)"""
import gc, json, os, sys; sys.path.insert(0, ".")
import torch
from wiki_grx_gym_amd.envs import GR1T1Cfg, GR1T1CfgPPO
runs = int(sys.argv[1]) if len(sys.argv) > 1 else 3
assert torch.cuda.is_available(), "noise_std_time.py measures on the GPU: there is no fallback"
ARMS = {"default": (), "log": ("--noise_std_type", "log"), "state_dependent": ("--state_dependent_std",),
        "state_dependent_log": ("--state_dependent_std", "--noise_std_type", "log")}


def full_iteration(flags):
    from wiki_grx_gym_amd.utils import get_args, task_registry
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


rows = []
for run in range(1, runs + 1):
    for arm, flags in ARMS.items():
        rows.append({"what": "full_iteration", "arm": arm, "run": run, "flags": list(flags), "envs": 4096, **full_iteration(flags)})
        print(rows[-1], flush=True)
        gc.collect()
out = sys.argv[2] if len(sys.argv) > 2 else "profiles/noise_std_step_time.json"
doc = {"what": "tools/noise_std_time.py on one MI355X", "runs_per_arm": runs, "rows": rows}
os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
with open(out, "w") as f:
    json.dump(doc, f, indent=1)
print(json.dumps(doc))
