"""One seed of GR1T1 (the registered task: flat terrain) at 4096 envs, 500 iterations, without and with `--smooth both` at the default
coefficients: what `python -m wiki_grx_gym_amd.scripts.train --task GR1T1 --headless --num_envs 4096 --max_iterations 500
--seed 1 [--smooth both]` logs, every tenth iteration -> profiles/smooth_learning_curve_gr1t1_flat_4096.json.  Observed, not a target: the
three defaults are not tuned.
    python tools/smooth_curve.py [iterations=500] [out=profiles/smooth_learning_curve_gr1t1_flat_4096.json]"""
import glob, json, os, sys, tempfile; sys.path.insert(0, ".")
from wiki_grx_gym_amd.envs import *  # noqa: F401,F403  (registers the tasks)
from wiki_grx_gym_amd.utils import get_args, task_registry
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 500
out = sys.argv[2] if len(sys.argv) > 2 else "profiles/smooth_learning_curve_gr1t1_flat_4096.json"
# (the env's action-rate / joint-acceleration reward terms: rew_action_diff, rew_action_diff_diff, rew_dof_acc_new)
TAGS = ("Train/mean_reward", "Train/mean_episode_length", "Episode/rew_action_diff", "Episode/rew_action_diff_diff", "Episode/rew_dof_acc_new",
        "Loss/smooth_temporal", "Loss/smooth_spatial", "Loss/value_function", "Loss/surrogate", "Loss/learning_rate", "Policy/mean_noise_std",
        "Perf/collection time", "Perf/learning_time")
doc = {"what": "GR1T1 flat, 4096 envs, seed 1: the default against --smooth both (coefficients 0.1 / 0.1, sigma 0.05: not tuned)",
       "iterations": [i for i in range(iters) if i % 10 == 0 or i == iters - 1]}
for arm, flags in (("default", []), ("smooth_both", ["--smooth", "both"])):
    root = tempfile.mkdtemp()
    args = get_args(["--task", "GR1T1", "--headless", "--num_envs", "4096", "--max_iterations", str(iters), "--seed", "1", *flags])
    env, _ = task_registry.make_env(name="GR1T1", args=args)
    runner, tcfg = task_registry.make_alg_runner(env=env, name="GR1T1", args=args, log_root=root)
    runner.learn(num_learning_iterations=iters, init_at_random_ep_len=True)
    rows = {}
    for line in open(glob.glob(os.path.join(root, "*", "scalars.jsonl"))[0]):
        r = json.loads(line)
        if r["tag"] in TAGS and r["step"] in doc["iterations"]:
            rows.setdefault(r["tag"], {})[r["step"]] = float(f"{r['value']:.5g}")
    doc[arm] = {t: [v.get(i) for i in doc["iterations"]] for t, v in rows.items()}
    print(arm, {t: v[-1] for t, v in doc[arm].items()}, flush=True)
    del runner, env
os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
with open(out, "w") as f:
    json.dump(doc, f, indent=1)
