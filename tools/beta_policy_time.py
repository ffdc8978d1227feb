"""What the Beta action distribution (--action_dist beta) costs per PPO iteration.  Nothing here is a target, except that the
flagless time must lie inside the parent commit's range.
  full_iteration as bench.py defines it -- OnPolicyRunner.learn(1) of a GR1T1 run at 4096 envs on rough terrain with the registered task's
    PPO configuration, timers synchronised at both ends and at the collection / learning boundary, the median of five iterations after two
    warm-up iterations (graph captures, allocator) -- for the arms: no flag (the yardstick), no flag in a built checkout of the parent
    commit (parent=<dir>: the same measurement in a child process whose working directory is that checkout), --action_dist beta, and the
    same with GRX_BETA_FUSED=0.  The arms ALTERNATE: `runs` rounds, each arm once per round in a fresh env and runner.
  rollout_step / minibatch_step: PPO.act on the run's observations (us per call) and one captured minibatch step's replay (the eager step
    under GRX_BETA_FUSED=0), device events around `reps` back-to-back calls, for the default and the Beta policy.
  loss_alone: grx_ppo_loss_beta against the fp32 torch spelling's forward + backward on one minibatch of the run's shape.
  kernel_resources: registers, LDS and scratch of the new kernels from the compiler's own report (needs hipcc, no GPU:
    `python tools/beta_policy_time.py resources [out]` writes that block alone).
    python tools/beta_policy_time.py [runs=3] [out=profiles/beta_policy_step_time.json] [parent=<dir>]   (the JSON line is printed too)"""
import gc, json, os, re, shutil, statistics, subprocess, sys, tempfile; sys.path.insert(0, ".")
import torch
ARMS = {"default": ((), "1"), "beta_fused": (("--action_dist", "beta"), "1"), "beta_torch": (("--action_dist", "beta"), "0")}
DEV = "cuda:0"


def timed(fn, reps):
    for _ in range(5):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); a.record()
    for _ in range(reps):
        fn()
    b.record(); torch.cuda.synchronize()
    return round(a.elapsed_time(b) * 1e3 / reps, 2)


def full_iteration(flags, fused, steps=True):
    from wiki_grx_gym_amd.envs import GR1T1Cfg, GR1T1CfgPPO
    from wiki_grx_gym_amd.utils import get_args, task_registry
    os.environ["GRX_BETA_FUSED"] = fused
    args = get_args(["--task", "GR1T1", "--headless", "--num_envs", "4096", "--seed", "1", *flags])
    cfg = GR1T1Cfg()
    cfg.terrain.mesh_type, cfg.terrain.curriculum = "heightfield", True   # bench.py's "rough": the curriculum raster as a heightfield
    env, _ = task_registry.make_env("GR1T1", args=args, env_cfg=cfg)
    runner, _ = task_registry.make_alg_runner(env, name=None, args=args, train_cfg=GR1T1CfgPPO(), log_root=None)
    runner.sync_timers = True
    runner.learn(2)                                                # graph captures, allocator
    ts = []
    for _ in range(5):
        runner.learn(1)
        ts.append((runner.last_collection_time + runner.last_learn_time, runner.last_collection_time, runner.last_learn_time))
    ts.sort()
    alg = runner.alg
    row = {"median_ms": round(ts[2][0] * 1e3, 2), "collection_ms": round(ts[2][1] * 1e3, 2), "learning_ms": round(ts[2][2] * 1e3, 2),
           "min_max_ms": [round(ts[0][0] * 1e3, 2), round(ts[-1][0] * 1e3, 2)], "terrain": env.cfg.terrain.mesh_type,
           "update_captured": bool(alg._use_graph and alg._graph is not None), "act_captured": bool(alg._use_act_graph and alg._act_graph is not None)}
    if steps:   # the two steps alone, on the run's own tensors
        obs = env.get_observations()
        pri = env.get_privileged_observations()
        with torch.inference_mode():
            row["rollout_step_us"] = timed(lambda: alg.act(obs, pri if pri is not None else obs), 50)
            alg.transition.clear()
        if alg._use_graph and alg._graph is not None:
            state = [p.detach().clone() for p in alg.actor_critic.parameters()]
            row["minibatch_step_us"] = timed(alg._graph.replay, 20)
            with torch.no_grad():
                for p, v in zip(alg.actor_critic.parameters(), state):
                    p.copy_(v)
    return row


def loss_alone(rounds, reps=50):
    from tests import beta_ref as R
    from wiki_grx_gym_amd.envs import GR1T1CfgPPO
    from wiki_grx_gym_amd.rl import beta as B
    mb = 4096 * int(GR1T1CfgPPO.runner.num_steps_per_env) // int(GR1T1CfgPPO.algorithm.num_mini_batches)
    d = tuple(t.to(DEV) for t in R.make_batch(mb, 10, "init", seed=1))

    def fused():
        raw, value = d[0].clone().requires_grad_(), d[1].clone().requires_grad_()
        B.fused_ppo_loss_beta(raw, value, *d[2:], 0.2, 1.0, 0.01, True)[2].backward()

    def spelled():
        raw, value = d[0].clone().requires_grad_(), d[1].clone().requires_grad_()
        B.loss_torch(raw, value, *d[2:], 0.2, 1.0, 0.01, True)[2].backward()
    rows = []
    for r in range(1, rounds + 1):
        for name, fn in (("grx_ppo_loss_beta", fused), ("torch_spelling_fp32", spelled)):
            rows.append({"what": "loss_alone", "arm": name, "run": r, "batch": mb, "actions": 10, "reps": reps, "us_per_call": timed(fn, reps)})
            print(rows[-1], flush=True)
    return rows


def kernel_resources():
    """the compiler's resource report of csrc/grx_ppo_beta.hip, or None without hipcc"""
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))
    if hipcc is None:
        return None
    src = os.path.join("wiki-grx-gym_amd", "csrc", "grx_ppo_beta.hip")
    with tempfile.TemporaryDirectory() as tmp:
        done = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", "-o", os.path.join(tmp, "beta.o"), src,
                               "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    if done.returncode != 0:
        raise RuntimeError("hipcc failed on " + src + ": " + done.stderr[-2000:])
    keys = {"VGPRs: ": "vgprs", "SGPRs: ": "sgprs", "ScratchSize [bytes/lane]: ": "scratch_bytes_per_lane",
            "LDS Size [bytes/block]: ": "lds_bytes_per_block", "Occupancy [waves/SIMD]: ": "occupancy_waves_per_simd"}
    kernels, cur = {}, None
    for ln in done.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            short = re.search(r"\d+((?:ppo_loss_)?beta_[a-z_]+?)(?:ILi(\d+)EE|E)", m.group(1))
            cur = (short.group(1) + (f"<{short.group(2)}>" if short.group(2) else "")) if short else m.group(1)
            kernels[cur] = {}
            continue
        for key, tag in keys.items():
            if cur and key in ln and "AGPR" not in ln:
                kernels[cur][tag] = int(ln.split(key)[1].split()[0])
    return {"what": "hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Rpass-analysis=kernel-resource-usage on csrc/grx_ppo_beta.hip; "
                    "<N>: lanes per row (16 for the 10 actions of GR1T1)", "kernels": kernels,
            "max_scratch_bytes_per_lane_over_all": max(v.get("scratch_bytes_per_lane", 0) for v in kernels.values())}


if len(sys.argv) > 1 and sys.argv[1] == "resources":               # the compiler's report alone: no GPU needed
    out = sys.argv[2] if len(sys.argv) > 2 else "profiles/beta_policy_step_time.json"
    doc = json.load(open(out)) if os.path.exists(out) else {}
    doc["kernel_resources"] = kernel_resources()
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc["kernel_resources"]))
    sys.exit(0)
if len(sys.argv) > 1 and sys.argv[1] == "--child":                 # the default arm once, in whatever checkout the working directory is
    print("CHILD " + json.dumps(full_iteration((), "1", steps=False)), flush=True)
    sys.exit(0)
opts = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
pos = [a for a in sys.argv[1:] if "=" not in a]
runs = int(pos[0]) if pos else 3
out = pos[1] if len(pos) > 1 else "profiles/beta_policy_step_time.json"
parent = opts.get("parent")
assert torch.cuda.is_available(), "beta_policy_time.py measures on the GPU: there is no fallback"


def parent_iteration():
    done = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], cwd=parent, capture_output=True, text=True, timeout=300)
    line = [ln for ln in done.stdout.splitlines() if ln.startswith("CHILD ")]
    if done.returncode != 0 or not line:
        raise RuntimeError(f"the parent checkout's run failed ({done.returncode}): {done.stderr[-2000:]}")
    return json.loads(line[-1][len("CHILD "):])


rows = []
for run in range(1, runs + 1):
    for arm, (flags, fused) in ARMS.items():
        rows.append({"what": "full_iteration", "arm": arm, "run": run, "flags": list(flags), "GRX_BETA_FUSED": fused, "envs": 4096,
                     **full_iteration(flags, fused)})
        print(rows[-1], flush=True)
        gc.collect()
        if arm == "default" and parent:
            rows.append({"what": "full_iteration", "arm": "default_parent_commit", "run": run, "flags": [], "envs": 4096, **parent_iteration()})
            print(rows[-1], flush=True)
os.environ["GRX_BETA_FUSED"] = "1"
alone = loss_alone(runs)
summary = {}
for arm in sorted({r["arm"] for r in rows}):
    mine = [r for r in rows if r["arm"] == arm]
    keys = [k for k in ("median_ms", "collection_ms", "learning_ms", "rollout_step_us", "minibatch_step_us") if all(k in r for r in mine)]
    summary[arm] = {k: {"median": round(statistics.median(r[k] for r in mine), 2), "min_max": [min(r[k] for r in mine), max(r[k] for r in mine)]}
                    for k in keys}
summary["loss_alone_us"] = {}
for arm in sorted({r["arm"] for r in alone}):
    us = [r["us_per_call"] for r in alone if r["arm"] == arm]
    summary["loss_alone_us"][arm] = {"median": round(statistics.median(us), 2), "min_max": [min(us), max(us)]}
doc = {"what": "tools/beta_policy_time.py on one MI355X", "runs_per_arm": runs, "summary": summary, "rows": rows + alone}
doc["kernel_resources"] = kernel_resources()
if doc["kernel_resources"] is None and os.path.exists(out):        # (no hipcc here: the block of the file that is being replaced)
    doc["kernel_resources"] = json.load(open(out)).get("kernel_resources")
os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
with open(out, "w") as f:
    json.dump(doc, f, indent=1)
print(json.dumps(doc["summary"]))
