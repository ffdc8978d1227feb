"""The second half of BASELINE.json's metric on the kernels as built: GR1T1 (registered lower-limb task) on FLAT terrain, 4096 envs,
PPO with the reference's hyper-parameters, N seeds x 1500 iterations.  Reports reward@1500 (mean of the last 100 iterations) mean +- sd
over the seeds, episode length, wall-clock and the training env-steps/s, plus which step kernel ran (grx_layout).
    python tools/train_seeds.py [iterations=1500] [seeds=3] [envs=4096] [terrain=plane] [task=GR1T1]   ->  gpurun_out/learning_curve_<terrain>_<envs>.json
(task GR1T1_full_body: the 32-DOF robot of BASELINE.json's fifth configuration on the tree kernel -> ..._full_body_<terrain>_<envs>.json)
GRX_TRAIN_PRECISION=bf16: PPO's hidden layers in bf16 (the --precision flag) -> learning_curve_<terrain>_bf16_<envs>.json
GRX_TRAIN_OBS_NORM=1: empirical observation normalisation (the --empirical_normalization flag) -> learning_curve_<terrain>_obs_norm_<envs>.json"""
import contextlib, io, json, os, sys, time
sys.path.insert(0, ".")
import numpy as np

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 1500
seeds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
envs = int(sys.argv[3]) if len(sys.argv) > 3 else 4096
terrain = sys.argv[4] if len(sys.argv) > 4 else "plane"
task = sys.argv[5] if len(sys.argv) > 5 else "GR1T1"
full = task == "GR1T1_full_body"
gr1t2 = task == "GR1T2"   # (BASELINE.json's fourth configuration: one rank's 4096-env shard of the 32768)
precision = os.environ.get("GRX_TRAIN_PRECISION")
obs_norm = os.environ.get("GRX_TRAIN_OBS_NORM") == "1"
tag = ("full_body_" if full else "gr1t2_" if gr1t2 else "") + terrain + (f"_{precision}" if precision else "") + ("_obs_norm" if obs_norm else "")
os.makedirs("gpurun_out", exist_ok=True)
runs = []
for seed in range(int(os.environ.get("GRX_TRAIN_FIRST_SEED", "1")), int(os.environ.get("GRX_TRAIN_FIRST_SEED", "1")) + seeds):
    import torch
    from wiki_grx_gym_amd.envs import GR1T1Cfg, GR1T1CfgPPO, GR1T1FullBodyCfg, GR1T1FullBodyCfgPPO, GR1T2Cfg, GR1T2CfgPPO
    from wiki_grx_gym_amd.utils import get_args, task_registry
    args = get_args(["--task", task, "--headless", "--num_envs", str(envs), "--seed", str(seed), "--max_iterations", str(iters)]
                    + (["--precision", precision] if precision else []) + (["--empirical_normalization"] if obs_norm else []))
    cfg = GR1T1FullBodyCfg() if full else GR1T2Cfg() if gr1t2 else GR1T1Cfg()
    cfg.terrain.mesh_type = terrain
    if os.environ.get("GRX_TRAIN_ONLY_POSITIVE") == "1":   # (diagnosis of the 32-DOF task: legged_robot.py:251-252's clip of the total reward at zero, off in the GR1T1 configs)
        cfg.rewards.only_positive_rewards = True
    if os.environ.get("GRX_TRAIN_ANKLE_ROLL"):   # (diagnosis of the 32-DOF task: "kp,kd" of the ankle-roll actuators, reference 0.25 / 0.01 -- practically free)
        kp_, kd_ = (float(x) for x in os.environ["GRX_TRAIN_ANKLE_ROLL"].split(","))
        cfg.control.stiffness = dict(cfg.control.stiffness, ankle_roll=kp_); cfg.control.damping = dict(cfg.control.damping, ankle_roll=kd_)
    if os.environ.get("GRX_TRAIN_TERMINATION"):   # (diagnosis: scale of the `termination` term, reference -0.0)
        cfg.rewards.scales.termination = float(os.environ["GRX_TRAIN_TERMINATION"])
    for kv in os.environ.get("GRX_TRAIN_SET", "").split(";"):      # (diagnosis) e.g. "control.stiffness['ankle_roll']=28.6;asset.armature['ankle_roll']=0.01"
        if kv.strip():
            exec("cfg." + kv.strip(), {"cfg": cfg})
    cfg.seed = seed
    env, _ = task_registry.make_env(task, args=args, env_cfg=cfg)
    layout = env._sim.layout()
    tcfg = GR1T1FullBodyCfgPPO() if full else GR1T2CfgPPO() if gr1t2 else GR1T1CfgPPO()
    tcfg.seed = seed
    if os.environ.get("GRX_TRAIN_INIT_NOISE"):   # (diagnosis of the 32-DOF task: exploration noise of the fresh policy, reference 0.2)
        tcfg.policy.init_noise_std = [float(x) for x in os.environ["GRX_TRAIN_INIT_NOISE"].split(",")] if "," in os.environ["GRX_TRAIN_INIT_NOISE"] else float(os.environ["GRX_TRAIN_INIT_NOISE"])
    if os.environ.get("GRX_TRAIN_ACTOR_GAIN"):
        tcfg.policy.actor_output_gain = float(os.environ["GRX_TRAIN_ACTOR_GAIN"])
    if os.environ.get("GRX_TRAIN_ENTROPY"):
        tcfg.algorithm.entropy_coef = float(os.environ["GRX_TRAIN_ENTROPY"])
    tcfg.runner.save_interval = 10 ** 9
    runner, tcfg = task_registry.make_alg_runner(env, name=task, args=args, train_cfg=tcfg, log_root=f"gpurun_out/train_{tag}_s{seed}")
    t0 = time.time()
    with contextlib.redirect_stdout(io.StringIO()):
        runner.learn(num_learning_iterations=iters, init_at_random_ep_len=True)
    dt = time.time() - t0
    rows = [json.loads(l) for l in open(os.path.join(runner.log_dir, "scalars.jsonl"))]
    for f_ in os.listdir(runner.log_dir):      # (gpurun merges at most 64 MiB back: the checkpoints of a curve run are not needed)
        if f_.endswith(".pt") or f_.startswith("events.out"):
            os.remove(os.path.join(runner.log_dir, f_))
    def series(tag):
        return np.array([r["value"] for r in rows if r["tag"] == tag], dtype=np.float64)
    rew, eplen = series("Train/mean_reward"), series("Train/mean_episode_length")
    res = {"seed": seed, "iterations": iters, "wall_s": dt, "train_env_steps_per_s": iters * 64 * envs / dt,
           "reward_at_end": float(rew[-100:].mean()), "episode_length_at_end": float(eplen[-100:].mean()),
           "first_iteration_with_reward_above_60": int(np.argmax(rew > 60.0)) if (rew > 60.0).any() else None,
           "first_iteration_with_episode_length_above_900": int(np.argmax(eplen > 900.0)) if (eplen > 900.0).any() else None,
           "collection_s_per_iteration": float(series("Perf/collection time")[-200:].mean()), "learning_s_per_iteration": float(series("Perf/learning_time")[-200:].mean()),
           "reward_every_50": rew[::50].round(2).tolist(), "episode_length_every_50": eplen[::50].round(1).tolist(),
           "noise_std_every_100": series("Policy/mean_noise_std")[::100].round(4).tolist()}
    runs.append(res)
    print(json.dumps({k: v for k, v in res.items() if not isinstance(v, list)}), flush=True)
    r_ = np.array([r["reward_at_end"] for r in runs]); l_ = np.array([r["episode_length_at_end"] for r in runs]); w_ = np.array([r["wall_s"] for r in runs])
    summary = {"task": ("GR1T1 full body (32 DOF), " if full else "GR1T2 (lower limb), " if gr1t2 else "GR1T1 (lower limb), ") + ("flat plane" if terrain == "plane" else terrain), "num_envs": envs, "iterations": iters, "seeds": len(runs),
               "step_kernel": layout, "precision": precision or "fp32", "empirical_normalization": obs_norm, "reward_at_end_mean": float(r_.mean()), "iterations_run": iters, "reward_at_end_sd": float(r_.std(ddof=1)) if len(runs) > 1 else None,
               "episode_length_mean": float(l_.mean()), "wall_s_mean": float(w_.mean()), "wall_s_sd": float(w_.std(ddof=1)) if len(runs) > 1 else None,
               "note": "reward_at_end = mean of Train/mean_reward over the last 100 iterations; PPO hyper-parameters of the registered GR1T1 task "
                       "(gr1t1_lower_limb_config.py; the full-body task: this build's GR1T1FullCfgPPO); no reference curve exists to compare with (Isaac Gym is absent: BASELINE.md)",
               "overrides": {k: os.environ[k] for k in ("GRX_TRAIN_ONLY_POSITIVE", "GRX_TRAIN_INIT_NOISE", "GRX_TRAIN_ANKLE_ROLL", "GRX_TRAIN_TERMINATION", "GRX_TRAIN_ENTROPY", "GRX_TRAIN_SET", "GRX_TRAIN_ACTOR_GAIN") if k in os.environ},
               "runs": runs}
    json.dump(summary, open(f"gpurun_out/learning_curve_{tag}_{envs}" + ("_overrides" if any(k in os.environ for k in ("GRX_TRAIN_ONLY_POSITIVE", "GRX_TRAIN_INIT_NOISE", "GRX_TRAIN_ANKLE_ROLL", "GRX_TRAIN_TERMINATION", "GRX_TRAIN_ENTROPY", "GRX_TRAIN_SET", "GRX_TRAIN_ACTOR_GAIN")) else "") + ".json", "w"), indent=1)
    env.close()
    del runner, env
    torch.cuda.empty_cache()
