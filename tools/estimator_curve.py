"""One seed of GR1T1 (the registered task: flat terrain) at 4096 envs, 300 iterations, without and with `--estimator` at its defaults
(targets lin_vel, hidden 128 64, learning rate 1e-3, one epoch: none of them tuned): what `python -m
wiki_grx_gym_amd.scripts.train --task GR1T1 --headless --num_envs 4096 --max_iterations 300 --seed 1 [--estimator]` logs, every tenth
iteration -> profiles/estimator_curve.json.  ONE seed per arm: a record of what the untuned defaults do, not a result.
    python tools/estimator_curve.py [iterations=300] [out=profiles/estimator_curve.json]"""
import glob, json, os, sys, tempfile; sys.path.insert(0, ".")
from wiki_grx_gym_amd.envs import *  # noqa: F401,F403  (registers the tasks)
from wiki_grx_gym_amd.utils import get_args, task_registry
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 300
out = sys.argv[2] if len(sys.argv) > 2 else "profiles/estimator_curve.json"
TAGS = ("Train/mean_reward", "Train/mean_episode_length", "Loss/estimator", "Loss/value_function", "Loss/surrogate", "Loss/learning_rate",
        "Policy/mean_noise_std", "Perf/collection time", "Perf/learning_time")
doc = {"what": "GR1T1 flat, 4096 envs, seed 1: the default against --estimator (targets lin_vel, hidden 128 64, lr 1e-3, 1 epoch: not tuned); "
               "ONE seed per arm, not a result",
       "iterations": [i for i in range(iters) if i % 10 == 0 or i == iters - 1]}
for arm, flags in (("default", []), ("estimator", ["--estimator"])):
    root = tempfile.mkdtemp()
    args = get_args(["--task", "GR1T1", "--headless", "--num_envs", "4096", "--max_iterations", str(iters), "--seed", "1", *flags])
    env, _ = task_registry.make_env(name="GR1T1", args=args)
    runner, tcfg = task_registry.make_alg_runner(env=env, name="GR1T1", args=args, log_root=root)
    runner.learn(num_learning_iterations=iters, init_at_random_ep_len=True)
    rows = {}
    for line in open(glob.glob(os.path.join(root, "*", "scalars.jsonl"))[0]):
        r = json.loads(line)
        if (r["tag"] in TAGS or "lin_vel" in r["tag"]) and r["step"] in doc["iterations"]:
            rows.setdefault(r["tag"], {})[r["step"]] = float(f"{r['value']:.5g}")
    doc[arm] = {t: [v.get(i) for i in doc["iterations"]] for t, v in rows.items()}
    print(arm, {t: v[-1] for t, v in doc[arm].items()}, flush=True)
    del runner, env
os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
with open(out, "w") as f:
    json.dump(doc, f, indent=1)
