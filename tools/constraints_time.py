"""What constraints as terminations (--constraints) cost per PPO iteration, and what the per-step pass and compute_returns
alone take both ways.  Nothing here is a target.
  full_iteration as bench.py defines it -- OnPolicyRunner.learn(1) of a GR1T1 run at 4096 envs with the registered task's PPO configuration,
    timers synchronised at both ends and at the collection / learning boundary, the median of five iterations after two warm-up iterations
    (graph captures, allocator) -- for the arms: no flag (the yardstick), no flag in a built checkout of the parent commit (parent=<dir>:
    the same measurement in a child process whose working directory is that checkout), the five-family spec with the two fused entries,
    and the same with GRX_CAT_FUSED=0.  The arms ALTERNATE: `runs` rounds, each arm once per round in a fresh env and runner.
  the step pass alone, on tensors of the run's shape (N = 4096, the robot's 10 DOF and 10 actions: C = 41 columns): grx_cat_step (three
    launches; with its arguments prepared once, as the rollout calls it, and with the checks and the marshalling of every call) and
    cat_step_torch (GRX_CAT_FUSED=0's path).  compute_returns alone (T = num_steps_per_env): RolloutStorage.compute_returns
    (the default path), grx_cat_returns (three launches) and cat_returns_torch.  Device events around `reps` back-to-back calls after a
    warm-up, the paths alternating over `runs` rounds; microseconds per call.
  kernel_resources: registers, LDS and scratch of the new kernels from the compiler's own report (hipcc -Rpass-analysis=kernel-resource-usage
    on csrc/grx_ppo_cat.hip with the Makefile's flags).  Needs hipcc, no GPU: `python tools/constraints_time.py resources [out]` writes that
    block alone into `out`, a timing run takes it anew when hipcc is there and keeps the block of an existing `out` otherwise.
`summary` holds, per arm, the median and the min / max over the rounds of each figure.
    python tools/constraints_time.py [runs=3] [out=profiles/constraints_step_time.json] [parent=<dir>]   (the JSON line is printed too)"""
import gc, json, os, re, shutil, statistics, subprocess, sys, tempfile; sys.path.insert(0, ".")
import torch
SPEC = "torque:0.05..0.25,dof_vel:0.05..0.25,dof_pos:0.25,action_rate:0.25@1.5,upright:1.0@0.7"
ARMS = {"default": ((), "1"), "constraints_fused": (("--constraints", SPEC), "1"), "constraints_torch": (("--constraints", SPEC), "0")}
DEV = "cuda:0"


def full_iteration(flags, fused):
    from wiki_grx_gym_amd.envs import GR1T1Cfg, GR1T1CfgPPO
    from wiki_grx_gym_amd.utils import get_args, task_registry
    os.environ["GRX_CAT_FUSED"] = fused
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


def kernel_resources():
    """the compiler's resource report of csrc/grx_ppo_cat.hip, or None without hipcc"""
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))
    if hipcc is None:
        return None
    src = os.path.join("wiki-grx-gym_amd", "csrc", "grx_ppo_cat.hip")
    with tempfile.TemporaryDirectory() as tmp:
        done = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", "-o", os.path.join(tmp, "cat.o"), src,
                               "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    if done.returncode != 0:
        raise RuntimeError("hipcc failed on " + src + ": " + done.stderr[-2000:])
    keys = {"VGPRs: ": "vgprs", "SGPRs: ": "sgprs", "ScratchSize [bytes/lane]: ": "scratch_bytes_per_lane", "VGPRs Spill: ": "vgpr_spill",
            "LDS Size [bytes/block]: ": "lds_bytes_per_block", "Occupancy [waves/SIMD]: ": "occupancy_waves_per_simd"}
    kernels, cur = {}, None
    for ln in done.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            short = re.search(r"\d+(cat_[a-z_]+?_kernel)E", m.group(1))
            cur = short.group(1) if short else m.group(1)
            kernels[cur] = {}
            continue
        for key, tag in keys.items():
            if cur and key in ln and "AGPR" not in ln and (key != "VGPRs: " or "Spill" not in ln):
                kernels[cur][tag] = int(ln.split(key)[1].split()[0])
    return {"what": "hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Rpass-analysis=kernel-resource-usage on csrc/grx_ppo_cat.hip",
            "kernels": kernels, "max_scratch_bytes_per_lane_over_all": max(v.get("scratch_bytes_per_lane", 0) for v in kernels.values())}


if len(sys.argv) > 1 and sys.argv[1] == "resources":               # the compiler's report alone: no GPU needed
    out = sys.argv[2] if len(sys.argv) > 2 else "profiles/constraints_step_time.json"
    doc = json.load(open(out)) if os.path.exists(out) else {}
    doc["kernel_resources"] = kernel_resources()
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc["kernel_resources"]))
    sys.exit(0)
if len(sys.argv) > 1 and sys.argv[1] == "--child":                 # the default arm once, in whatever checkout the working directory is
    print("CHILD " + json.dumps(full_iteration((), "1")), flush=True)
    sys.exit(0)
opts = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
pos = [a for a in sys.argv[1:] if "=" not in a]
runs = int(pos[0]) if pos else 3
out = pos[1] if len(pos) > 1 else "profiles/constraints_step_time.json"
parent = opts.get("parent")
assert torch.cuda.is_available(), "constraints_time.py measures on the GPU: there is no fallback"


def parent_iteration():
    done = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], cwd=parent, capture_output=True, text=True, timeout=300)
    line = [ln for ln in done.stdout.splitlines() if ln.startswith("CHILD ")]
    if done.returncode != 0 or not line:
        raise RuntimeError(f"the parent checkout's run failed ({done.returncode}): {done.stderr[-2000:]}")
    return json.loads(line[-1][len("CHILD "):])


def timed(fn, reps):
    for _ in range(5):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); a.record()
    for _ in range(reps):
        fn()
    b.record(); torch.cuda.synchronize()
    return round(a.elapsed_time(b) * 1e3 / reps, 2)


def passes_alone(rounds, reps=50):
    from wiki_grx_gym_amd.envs import GR1T1CfgPPO
    from wiki_grx_gym_amd.rl import constraints as K
    from wiki_grx_gym_amd.rl.storage import RolloutStorage
    T, N, D = int(GR1T1CfgPPO.runner.num_steps_per_env), 4096, 10
    g = torch.Generator(device=DEV).manual_seed(1)
    rnd = lambda *s: torch.rand(*s, device=DEV, generator=g)
    st = RolloutStorage(N, T, [1], [1], [1], DEV)
    st.rewards.copy_(0.1 * rnd(T, N, 1)); st.values.copy_(10.0 + 5.0 * rnd(T, N, 1)); st.dones.copy_((rnd(T, N, 1) < 0.02).to(torch.uint8))
    last, prob_tn = 10.0 + 5.0 * rnd(N, 1), rnd(T, N) * (rnd(T, N) < 0.3)
    stats, part = torch.zeros(4, device=DEV), K.cat_partials(T, N, DEV)
    limits = torch.ones(D), torch.ones(D), torch.stack([-torch.ones(D), torch.ones(D)], 1)
    table = K.ColumnTable(K.parse_constraints(SPEC), D, D, *limits, 0.95, 0.95, DEV)
    prob = torch.full((table.C,), 0.25, device=DEV)
    # (N, k) views with strides (1, N), as the env publishes its state; about a tenth of the entries outside +-0.95
    src = [(2.2 * rnd(D, N) - 1.1).t() for _ in range(4)] + [(0.8 * rnd(3, N)).t()]
    dones = (rnd(N) < 0.02).to(torch.uint8)
    prev, c_max, counts = torch.zeros(N, D, device=DEV), torch.zeros(table.C, device=DEV), torch.zeros(table.F, dtype=torch.int32, device=DEV)
    delta, row, scratch = torch.zeros(N, device=DEV), torch.zeros(N, device=DEV), K.step_scratch(table, N, DEV)
    step = (table, prob, *src, dones, 0.95, 0.05, True, False, prev, c_max, counts, delta, row)
    prepared = K.prepare_step(*step, scratch=scratch)             # (as Constraints.step keeps one per rollout step)
    paths = {"step_fused": lambda: K.launch_step(prepared), "step_fused_with_argument_checks": lambda: K.cat_step_hip(*step, scratch=scratch),
             "step_torch": lambda: K.cat_step_torch(*step),
             "returns_default_torch_loop": lambda: st.compute_returns(last, 0.994, 0.9),
             "returns_fused": lambda: K.cat_returns_hip(st.rewards, st.values, st.dones, prob_tn, last, 0.994, 0.9, st.returns, st.advantages, stats, part),
             "returns_torch": lambda: K.cat_returns_torch(st.rewards, st.values, st.dones, prob_tn, last, 0.994, 0.9, st.returns, st.advantages, stats)}
    rows = []
    with torch.inference_mode():
        for r in range(1, rounds + 1):
            for name, fn in paths.items():
                adv = st.advantages
                rows.append({"what": "step_alone" if name.startswith("step") else "compute_returns_alone", "arm": name, "run": r, "T": T,
                             "envs": N, "columns": table.C, "reps": reps, "us_per_call": timed(fn, reps)})
                st.advantages = adv                                # (the default path rebinds it)
                print(rows[-1], flush=True)
    return rows


rows = []
for run in range(1, runs + 1):
    for arm, (flags, fused) in ARMS.items():
        rows.append({"what": "full_iteration", "arm": arm, "run": run, "flags": list(flags), "GRX_CAT_FUSED": fused, "envs": 4096,
                     **full_iteration(flags, fused)})
        print(rows[-1], flush=True)
        gc.collect()
        if arm == "default" and parent:
            rows.append({"what": "full_iteration", "arm": "default_parent_commit", "run": run, "flags": [], "envs": 4096, **parent_iteration()})
            print(rows[-1], flush=True)
alone = passes_alone(runs)
summary = {}
for arm in sorted({r["arm"] for r in rows}):
    mine = [r for r in rows if r["arm"] == arm]
    summary[arm] = {k: {"median": round(statistics.median(r[k] for r in mine), 2), "min_max": [min(r[k] for r in mine), max(r[k] for r in mine)]}
                    for k in ("median_ms", "collection_ms", "learning_ms")}
for what in ("step_alone", "compute_returns_alone"):
    summary[what + "_us"] = {}
    for arm in sorted({r["arm"] for r in alone if r["what"] == what}):
        us = [r["us_per_call"] for r in alone if r["arm"] == arm]
        summary[what + "_us"][arm] = {"median": round(statistics.median(us), 2), "min_max": [min(us), max(us)]}
doc = {"what": "tools/constraints_time.py on one MI355X", "runs_per_arm": runs, "spec": SPEC, "summary": summary, "rows": rows + alone}
doc["kernel_resources"] = kernel_resources()
if doc["kernel_resources"] is None and os.path.exists(out):        # (no hipcc here: the block of the file that is being replaced)
    doc["kernel_resources"] = json.load(open(out)).get("kernel_resources")
os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
with open(out, "w") as f:
    json.dump(doc, f, indent=1)
print(json.dumps(doc["summary"]))
