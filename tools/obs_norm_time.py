"""What empirical observation normalisation (--empirical_normalization) costs per rollout step: GR1T1, 4096 envs, the
full rollout step of the runner's loop (policy, env.step, [normalisation,] storage) with the option off and on, ALTERNATED in one
process on one env, microseconds per step over windows of 40 rollouts of 24 steps, REPEATS windows each.
    python tools/obs_norm_time.py [repeats=7] [out=obs_norm_time.json]   (the JSON line is printed too)
    GRX_OBS_NORM_ONLY=on|off python tools/obs_norm_time.py    one arm only (for `rocprofv3 --kernel-trace --stats -- python ...`)"""
import json, os, statistics, sys, time; sys.path.insert(0, ".")
import torch
import wiki_grx_gym_amd.envs  # noqa
from wiki_grx_gym_amd.rl.normalizer import EmpiricalNormalization, normalize_step
from wiki_grx_gym_amd.utils import get_args, task_registry
repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 7
only = os.environ.get("GRX_OBS_NORM_ONLY")
args = get_args(["--task", "GR1T1", "--headless", "--num_envs", "4096", "--seed", "1"])
env, _ = task_registry.make_env("GR1T1", args=args)
runner, _ = task_registry.make_alg_runner(env, name="GR1T1", args=args, log_root=None)
alg, T = runner.algorithm, runner.num_steps_per_env
norms = [EmpiricalNormalization(env.num_obs).to("cuda:0"), EmpiricalNormalization(env.num_pri_obs).to("cuda:0")]
state = {"obs": env.get_observations(), "pri": env.get_privileged_observations()}


def rollout(on):
    obs, pri = state["obs"], state["pri"]
    with torch.inference_mode():
        for _ in range(T):
            a = alg.act(obs, pri)
            obs, pri, r, d, i = env.step(a)
            if on:
                obs, pri = normalize_step(norms, [obs, pri])
            alg.process_env_step(r, d, i)
    alg.clear_storage()
    state["obs"], state["pri"] = obs, pri


ROLLOUTS = 40   # per timed window: ~1000 steps, a fifth of a second


def timed(on):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(ROLLOUTS):
        rollout(on)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (T * ROLLOUTS) * 1e6


arms = [a for a in ("off", "on") if only in (None, a)]
for a in arms * 2:       # warm-up: graph capture, the normalisers' buffers
    rollout(a == "on")
ts = {a: [] for a in arms}
for _ in range(repeats):
    for a in arms:
        ts[a].append(timed(a == "on"))
out = {"task": "GR1T1", "num_envs": 4096, "steps_per_rollout": T, "rollouts_per_window": ROLLOUTS, "repeats": repeats, "widths": [env.num_obs, env.num_pri_obs],
       "launches_added_per_step": 6, "us_per_step": {a: [round(t, 1) for t in v] for a, v in ts.items()},
       "median_us_per_step": {a: round(statistics.median(v), 1) for a, v in ts.items()},
       "spread_us_per_step": {a: round(max(v) - min(v), 1) for a, v in ts.items()}}
if len(arms) == 2:
    out["added_us_per_step_median"] = round(statistics.median(ts["on"]) - statistics.median(ts["off"]), 1)
    out["added_us_per_step_paired"] = [round(b - a, 1) for a, b in zip(ts["off"], ts["on"])]
print(json.dumps(out))
json.dump(out, open(sys.argv[2] if len(sys.argv) > 2 else "obs_norm_time.json", "w"), indent=1)
