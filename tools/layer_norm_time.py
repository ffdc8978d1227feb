"""What LayerNorm hidden layers (--layer_norm) cost per PPO iteration, and what their HIP entry points save over the torch
spelling (GRX_LN_FUSED=0, which is not captured).  Nothing here is a target.  full_iteration as bench.py defines it -- OnPolicyRunner.learn(1)
of a GR1T1 run at 4096 envs with the registered task's PPO configuration, timers synchronised at both ends and at the collection / learning
boundary, the median of five iterations after two warm-up iterations (graph captures, allocator) -- for the arms: no flag (the yardstick: what
the code does without the option), the flag with the HIP entry points, the flag with GRX_LN_FUSED=0, and -- parent=DIR, a built checkout of
the parent commit -- no flag on the parent's code.  The arms ALTERNATE: `runs` rounds, each arm once per round in a fresh process (one at a
time; the parent's arm with that checkout as its working directory, running the parent's own code through the `--arm default` of this file).
`summary` holds, per arm, the median and the min / max over the rounds of each figure; the two no-flag arms agree when their ranges overlap.
`kernels` lists registers, scratch and LDS of the LayerNorm kernels (tools/kernel_resources.py on the built library).
    python tools/layer_norm_time.py [runs=3] [out=profiles/layer_norm_step_time.json] [parent=DIR]   (the JSON line is printed too)"""
import gc, json, os, statistics, subprocess, sys; sys.path.insert(0, ".")

ARMS = {"default": ((), "1"), "layer_norm_fused": (("--layer_norm",), "1"), "layer_norm_torch": (("--layer_norm",), "0")}


def full_iteration(flags, fused):
    import torch
    from wiki_grx_gym_amd.envs import GR1T1Cfg, GR1T1CfgPPO
    from wiki_grx_gym_amd.utils import get_args, task_registry
    assert torch.cuda.is_available(), "layer_norm_time.py measures on the GPU: there is no fallback"
    os.environ["GRX_LN_FUSED"] = fused                             # (read at every call)
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
    return {"median_ms": round(ts[2][0] * 1e3, 2), "collection_ms": round(ts[2][1] * 1e3, 2), "learning_ms": round(ts[2][2] * 1e3, 2),
            "min_max_ms": [round(ts[0][0] * 1e3, 2), round(ts[-1][0] * 1e3, 2)],
            "update_captured": bool(alg._use_graph and alg._graph is not None),
            "policy_step_captured_and_fused": bool(alg._use_act_graph and alg._act_graph is not None and alg._act_fused),
            "fused_step_tail": bool(alg._fused_tail)}


if len(sys.argv) > 1 and sys.argv[1] == "--arm":                    # the child: one arm, one JSON line
    flags, fused = ARMS[sys.argv[2]]
    print("ROW " + json.dumps(full_iteration(flags, fused)), flush=True)
    sys.exit(0)

pos = [a for a in sys.argv[1:] if not a.startswith("parent=")]
parent = next((a[len("parent="):] for a in sys.argv[1:] if a.startswith("parent=")), None)
runs = int(pos[0]) if pos else 3
out = pos[1] if len(pos) > 1 else "profiles/layer_norm_step_time.json"
me = os.path.abspath(__file__)
arms = [(name, name, ".") for name in ARMS] + ([("default_parent", "default", parent)] if parent else [])
rows = []
for run in range(1, runs + 1):
    for arm, key, cwd in arms:
        res = subprocess.run([sys.executable, me, "--arm", key], cwd=cwd, capture_output=True, text=True, timeout=600)
        if res.returncode != 0:                                     # (nothing more is started on the GPU after a child that failed)
            sys.exit(f"arm {arm} failed ({res.returncode}):\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}")
        row = json.loads(next(l for l in res.stdout.splitlines() if l.startswith("ROW "))[4:])
        rows.append({"what": "full_iteration", "arm": arm, "run": run, "flags": list(ARMS[key][0]), "GRX_LN_FUSED": ARMS[key][1], "envs": 4096, **row})
        print(rows[-1], flush=True)
        gc.collect()
summary = {}
for arm, _, _ in arms:
    mine = [r for r in rows if r["arm"] == arm]
    summary[arm] = {k: {"median": round(statistics.median(r[k] for r in mine), 2), "min_max": [min(r[k] for r in mine), max(r[k] for r in mine)]}
                    for k in ("median_ms", "collection_ms", "learning_ms")}
if parent:
    a, b = summary["default"]["median_ms"]["min_max"], summary["default_parent"]["median_ms"]["min_max"]
    summary["default_within_spread_of_parent"] = bool(a[0] <= b[1] and b[0] <= a[1])
a, b = summary["layer_norm_fused"]["median_ms"], summary["layer_norm_torch"]["median_ms"]
summary["fused_not_slower_than_torch_spelling"] = bool(a["median"] <= b["median"] or a["min_max"][0] <= b["min_max"][1])
sys.path.insert(0, os.path.dirname(me))
import kernel_resources as KR
lib = os.path.join("wiki-grx-gym_amd", "csrc", "libgrx_ppo.so")
kernels = [r for co in KR.code_objects(open(lib, "rb").read()) for r in KR.kernels_of(co) if r["kernel"].startswith("ln_elu_")]
doc = {"what": "tools/layer_norm_time.py on one MI355X", "runs_per_arm": runs, "summary": summary, "kernels": sorted(kernels, key=lambda r: r["kernel"]),
       "rows": rows}
os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
with open(out, "w") as f:
    json.dump(doc, f, indent=1)
print(json.dumps(doc))
