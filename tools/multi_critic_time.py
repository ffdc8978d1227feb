"""What multi-critic PPO (--reward_groups) costs per PPO iteration, what compute_returns alone takes both ways, and what
publishing the per-term reward tables costs the env step.  Nothing here is a target.
  full_iteration as bench.py defines it -- OnPolicyRunner.learn(1) of a GR1T1 run at 4096 envs with the registered task's PPO configuration,
    timers synchronised at both ends and at the collection / learning boundary, the median of five iterations after two warm-up iterations
    (graph captures, allocator) -- for the arms: no flag (the yardstick), no flag in a built checkout of the parent commit (parent=<dir>:
    the same measurement in a child process whose working directory is that checkout), the two-group spec with the three fused entries,
    and the same with GRX_MC_FUSED=0.  The arms ALTERNATE: `runs` rounds, each arm once per round in a fresh env and runner.
  compute_returns alone, on tensors of the run's shape (T = num_steps_per_env, N = 4096, K = 2): RolloutStorage.compute_returns on one
    column (the default path), grx_mc_returns (three launches) and mc_returns_torch (GRX_MC_FUSED=0's path).  Device events around `reps`
    back-to-back calls after a warm-up, the paths alternating over `runs` rounds; microseconds per call.  grx_mc_store likewise, per call.
  env_step: 200 steps of zero actions at 4096 envs with env_cfg.env.publish_reward_terms off and on, device events, alternating.
  kernel_resources: registers, LDS and scratch of the new kernels from the compiler's own report (hipcc -Rpass-analysis=kernel-resource-usage
    on csrc/grx_ppo_mc.hip with the Makefile's flags; of the loss kernel's 32 instantiations those for 1, 10 and 32 actions).  Needs hipcc,
    no GPU: `python tools/multi_critic_time.py resources [out]` writes that block alone into `out`, a timing run takes it anew when hipcc is
    there and keeps the block of an existing `out` otherwise.
`summary` holds, per arm, the median and the min / max over the rounds of each figure.
    python tools/multi_critic_time.py [runs=3] [out=profiles/multi_critic_step_time.json] [parent=<dir>]   (the JSON line is printed too)"""
import gc, json, os, re, shutil, statistics, subprocess, sys, tempfile; sys.path.insert(0, ".")
import torch
SPEC = "track=cmd_diff_lin_vel_x,cmd_diff_lin_vel_y,cmd_diff_ang_vel_yaw;rest=*"
ARMS = {"default": ((), "1"), "multi_critic_fused": (("--reward_groups", SPEC), "1"), "multi_critic_torch": (("--reward_groups", SPEC), "0")}
DEV = "cuda:0"


def full_iteration(flags, fused):
    from wiki_grx_gym_amd.envs import GR1T1Cfg, GR1T1CfgPPO
    from wiki_grx_gym_amd.utils import get_args, task_registry
    os.environ["GRX_MC_FUSED"] = fused
    args = get_args(["--task", "GR1T1", "--headless", "--num_envs", "4096", "--seed", "1", *flags])
    cfg = GR1T1Cfg()
    if flags:
        cfg.env.publish_reward_terms = True
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
    captured = bool(alg._use_graph and alg._graph is not None and alg._use_act_graph and alg._act_graph is not None)
    return {"median_ms": round(ts[2][0] * 1e3, 2), "collection_ms": round(ts[2][1] * 1e3, 2), "learning_ms": round(ts[2][2] * 1e3, 2),
            "min_max_ms": [round(ts[0][0] * 1e3, 2), round(ts[-1][0] * 1e3, 2)], "captured": captured}


def kernel_resources():
    """the compiler's resource report of csrc/grx_ppo_mc.hip, or None without hipcc"""
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))
    if hipcc is None:
        return None
    src = os.path.join("wiki-grx-gym_amd", "csrc", "grx_ppo_mc.hip")
    with tempfile.TemporaryDirectory() as tmp:
        done = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", "-o", os.path.join(tmp, "mc.o"), src,
                               "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    if done.returncode != 0:
        raise RuntimeError("hipcc failed on " + src + ": " + done.stderr[-2000:])
    keys = {"VGPRs: ": "vgprs", "SGPRs: ": "sgprs", "ScratchSize [bytes/lane]: ": "scratch_bytes_per_lane",
            "LDS Size [bytes/block]: ": "lds_bytes_per_block", "Occupancy [waves/SIMD]: ": "occupancy_waves_per_simd"}
    kernels, cur = {}, None
    for ln in done.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
            short = re.search(r"\d+(mc_[a-z_]+?)(?:ILi(\d+)EE|E)", name)
            cur = (short.group(1) + (f"<{short.group(2)}>" if short.group(2) else "")) if short else name
            kernels[cur] = {}
            continue
        for key, tag in keys.items():
            if cur and key in ln and "AGPR" not in ln:
                kernels[cur][tag] = int(ln.split(key)[1].split()[0])
    kept = {k: v for k, v in kernels.items() if "<" not in k or k in ("mc_loss_kernel<1>", "mc_loss_kernel<10>", "mc_loss_kernel<32>")}
    return {"what": "hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Rpass-analysis=kernel-resource-usage on csrc/grx_ppo_mc.hip; of "
                    "mc_loss_kernel<A> the instantiations A = 1, 10, 32", "kernels": kept,
            "max_scratch_bytes_per_lane_over_all": max(v.get("scratch_bytes_per_lane", 0) for v in kernels.values())}


if len(sys.argv) > 1 and sys.argv[1] == "resources":               # the compiler's report alone: no GPU needed
    out = sys.argv[2] if len(sys.argv) > 2 else "profiles/multi_critic_step_time.json"
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
out = pos[1] if len(pos) > 1 else "profiles/multi_critic_step_time.json"
parent = opts.get("parent")
assert torch.cuda.is_available(), "multi_critic_time.py measures on the GPU: there is no fallback"


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


def returns_alone(rounds, reps=50):
    from wiki_grx_gym_amd import _capi
    from wiki_grx_gym_amd.envs import GR1T1CfgPPO
    from wiki_grx_gym_amd.rl import multi_critic as M
    from wiki_grx_gym_amd.rl.storage import RolloutStorage
    T, N, K = int(GR1T1CfgPPO.runner.num_steps_per_env), 4096, 2
    g = torch.Generator(device=DEV).manual_seed(1)
    rnd = lambda *s: torch.rand(*s, device=DEV, generator=g)
    st = RolloutStorage(N, T, [1], [1], [1], DEV)
    st.rewards.copy_(0.1 * rnd(T, N, 1)); st.values.copy_(10.0 + 5.0 * rnd(T, N, 1)); st.dones.copy_((rnd(T, N, 1) < 0.02).to(torch.uint8))
    rewards, values, last = 0.1 * rnd(T, N, K), 10.0 + 5.0 * rnd(T, N, K), 10.0 + 5.0 * rnd(N, K)
    returns, stats, part = torch.zeros(T, N, K, device=DEV), torch.zeros(K, 2, device=DEV), M.mc_partials(T, N, K, DEV)
    terms = rnd(_capi.NUM_REWARD_TERMS, N)
    group = torch.tensor([t % 3 - 1 for t in range(_capi.NUM_REWARD_TERMS)], dtype=torch.int32, device=DEV)
    to, sv, sr = (rnd(N) < 0.01).to(torch.uint8), torch.zeros(N, K, device=DEV), torch.zeros(N, K, device=DEV)
    paths = {"default_torch_loop_one_column": lambda: st.compute_returns(last[:, :1], 0.994, 0.9),
             "multi_critic_fused": lambda: M.mc_returns_hip(rewards, values, st.dones, last, [1.0, 1.0], 0.994, 0.9, returns, st.advantages, stats, part),
             "multi_critic_torch": lambda: M.mc_returns_torch(rewards, values, st.dones, last, [1.0, 1.0], 0.994, 0.9, returns, st.advantages, stats),
             "store_fused": lambda: M.mc_store_hip(terms, None, group, values[0], to, 0.994, sv, sr),
             "store_torch": lambda: M.mc_store_torch(terms, None, group.tolist(), values[0], to, 0.994, sv, sr)}
    rows = []
    with torch.inference_mode():
        for r in range(1, rounds + 1):
            for name, fn in paths.items():
                adv = st.advantages
                rows.append({"what": "store_alone" if name.startswith("store") else "compute_returns_alone", "arm": name, "run": r, "T": T,
                             "envs": N, "groups": K, "reps": reps, "us_per_call": timed(fn, reps)})
                st.advantages = adv                                # (the default path rebinds it)
                print(rows[-1], flush=True)
    return rows


def env_step(rounds, steps=200):
    from wiki_grx_gym_amd.envs import GR1T1Cfg
    from wiki_grx_gym_amd.utils import get_args, task_registry
    rows = []
    for r in range(1, rounds + 1):
        for publish in (False, True):
            args = get_args(["--task", "GR1T1", "--headless", "--num_envs", "4096", "--seed", "1"])
            cfg = GR1T1Cfg()
            cfg.env.publish_reward_terms = publish
            env, _ = task_registry.make_env("GR1T1", args=args, env_cfg=cfg)
            env.reset()
            actions = torch.zeros(4096, env.num_actions, device=DEV)
            with torch.inference_mode():
                rows.append({"what": "env_step", "arm": "publish_reward_terms_" + ("on" if publish else "off"), "run": r, "envs": 4096,
                             "steps": steps, "us_per_step": timed(lambda: env.step(actions), steps)})
            print(rows[-1], flush=True)
            del env
            gc.collect()
    return rows


rows = []
for run in range(1, runs + 1):
    for arm, (flags, fused) in ARMS.items():
        rows.append({"what": "full_iteration", "arm": arm, "run": run, "flags": list(flags), "GRX_MC_FUSED": fused, "envs": 4096,
                     **full_iteration(flags, fused)})
        print(rows[-1], flush=True)
        gc.collect()
        if arm == "default" and parent:
            rows.append({"what": "full_iteration", "arm": "default_parent_commit", "run": run, "flags": [], "envs": 4096, **parent_iteration()})
            print(rows[-1], flush=True)
alone, steps = returns_alone(runs), env_step(runs)
summary = {}
for arm in sorted({r["arm"] for r in rows}):
    mine = [r for r in rows if r["arm"] == arm]
    summary[arm] = {k: {"median": round(statistics.median(r[k] for r in mine), 2), "min_max": [min(r[k] for r in mine), max(r[k] for r in mine)]}
                    for k in ("median_ms", "collection_ms", "learning_ms")}
for what, key in (("compute_returns_alone", "us_per_call"), ("store_alone", "us_per_call"), ("env_step", "us_per_step")):
    summary[what + "_us"] = {}
    for arm in sorted({r["arm"] for r in alone + steps if r["what"] == what}):
        us = [r[key] for r in alone + steps if r["what"] == what and r["arm"] == arm]
        summary[what + "_us"][arm] = {"median": round(statistics.median(us), 2), "min_max": [min(us), max(us)]}
doc = {"what": "tools/multi_critic_time.py on one MI355X", "runs_per_arm": runs, "spec": SPEC, "summary": summary, "rows": rows + alone + steps}
doc["kernel_resources"] = kernel_resources()
if doc["kernel_resources"] is None and os.path.exists(out):        # (no hipcc here: the block of the file that is being replaced)
    doc["kernel_resources"] = json.load(open(out)).get("kernel_resources")
os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
with open(out, "w") as f:
    json.dump(doc, f, indent=1)
print(json.dumps(doc["summary"]))
