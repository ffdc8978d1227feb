"""One seed of GR1T1 at 4096 envs, 200 iterations, without and with `--rnd`: what
`python -m wiki_grx_gym_amd.scripts.train --task GR1T1 --headless --num_envs 4096 --max_iterations 200 --seed 1 [--rnd]` logs, every
tenth iteration -> profiles/rnd_learning_curve_gr1t1_4096.json: the extrinsic reward (Train/mean_reward), the intrinsic reward, the RND
loss and the terrain level.  Observed, not a target: one seed, an untuned weight.
    python tools/rnd_curve.py [iterations=200] [out=profiles/rnd_learning_curve_gr1t1_4096.json] [extra train flags, e.g. --terrain heightfield]"""
import glob, json, os, sys, tempfile; sys.path.insert(0, ".")
from wiki_grx_gym_amd.envs import *  # noqa: F401,F403  (registers the tasks)
from wiki_grx_gym_amd.utils import get_args, task_registry
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 200
out = sys.argv[2] if len(sys.argv) > 2 else "profiles/rnd_learning_curve_gr1t1_4096.json"
extra = sys.argv[3:]
TAGS = ("Train/mean_reward", "Train/mean_episode_length", "Train/mean_intrinsic_reward", "Train/rnd_weight", "Loss/rnd", "Episode/terrain_level",
        "Loss/value_function", "Loss/surrogate", "Loss/learning_rate", "Perf/collection time", "Perf/learning_time")
doc = {"command": "train --task GR1T1 --headless --num_envs 4096 --max_iterations %d --seed 1 %s" % (iters, " ".join(extra)),
       "iterations": [i for i in range(iters) if i % 10 == 0 or i == iters - 1]}
for arm, flags in (("default", []), ("rnd", ["--rnd"])):
    root = tempfile.mkdtemp()
    args = get_args(["--task", "GR1T1", "--headless", "--num_envs", "4096", "--max_iterations", str(iters), "--seed", "1", *extra, *flags])
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
