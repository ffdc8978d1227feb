"""What random network distillation (--rnd) costs.  Three measurements, nothing here is a target:
  * the reward: grx_rnd_reward (three launches) against its torch spelling (rl.rnd.rnd_reward_torch, GRX_RND_FUSED=0) at
    (N, E) = (4096, 32).  The two arms ALTERNATE in one process; a timed window is CALLS back-to-back calls between two device events,
    REPEATS windows per arm after a warm-up window, median and spread per call in microseconds.  Both arms' results are compared first.
  * one rollout_step, and RandomNetworkDistillation.update(epochs, minibatches) as the runner calls it -- GR1T1CfgPPO's counts, the
    permutation and the one read-back included --, whole and divided by its epochs x minibatches steps (gather, predictor forward, loss,
    backward, Adam), at the GR1T1 train shape.
  * full_iteration: OnPolicyRunner.learn(1) of a GR1T1 run at 4096 envs with and without --rnd, timers synchronised; with --rnd the time of
    rnd.update() inside that loop (device drained before and after) beside it.
    python tools/rnd_time.py [repeats=15] [out=profiles/rnd_step_time.json]   (the JSON line is printed too)"""
import json, os, statistics, sys; sys.path.insert(0, ".")
import torch
from wiki_grx_gym_amd.envs import GR1T1Cfg, GR1T1CfgPPO
from wiki_grx_gym_amd.rl import rnd as M
repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 15
CALLS = 200
DEV = "cuda:0"
assert torch.cuda.is_available(), "rnd_time.py measures on the GPU: there is no fallback"


def window(fn, calls=CALLS):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def measure(arms, calls=CALLS, reps=repeats):
    ts = {k: [] for k in arms}
    for fn in arms.values():
        window(fn, calls)                                         # warm-up
    for _ in range(reps):
        for k, fn in arms.items():
            ts[k].append(window(fn, calls))
    return {"median_us_per_call": {k: round(statistics.median(v), 2) for k, v in ts.items()},
            "min_max_us_per_call": {k: [round(min(v), 2), round(max(v), 2)] for k, v in ts.items()}}


rows = []
# ---- the reward ------------------------------------------------------------------------------------------------------------------------------
N, E = 4096, 32
torch.manual_seed(0)
pred, targ = torch.randn(N, E, device=DEV), torch.randn(N, E, device=DEV)


def state():
    z = lambda *s, **k: torch.zeros(*s, device=DEV, **k)
    return [z(N), z(1, dtype=torch.long), z(1), torch.ones(1, device=DEV), torch.ones(1, device=DEV), z(N), z(N), z(N)]   # ret, count, mean, var, std, rewards, intrinsic, raw


a, b = state(), state()
for _ in range(3):
    M.rnd_reward_hip(pred, targ, 0.99, 0.1, 1e-2, *a)
    M.rnd_reward_torch(pred, targ, 0.99, 0.1, 1e-2, *b)
torch.cuda.synchronize()
err = max(float((x.double() - y.double()).abs().max() / y.double().abs().max()) for x, y in zip(a, b))
assert err < 1e-5, err
with torch.inference_mode():
    rows.append({"what": "reward", "N": N, "E": E, "max_relative_difference_between_the_arms": err,
                 **measure({"hip": lambda: M.rnd_reward_hip(pred, targ, 0.99, 0.1, 1e-2, *a),
                            "torch": lambda: M.rnd_reward_torch(pred, targ, 0.99, 0.1, 1e-2, *b)})})
print(rows[-1], flush=True)

# ---- one rollout step and one minibatch step -------------------------------------------------------------------------------------------------
tcfg = GR1T1CfgPPO()
T, nmb, epochs = int(tcfg.runner.num_steps_per_env), int(tcfg.algorithm.num_mini_batches), int(tcfg.algorithm.num_learning_epochs)
for fused in ("1", "0"):
    os.environ["GRX_RND_FUSED"] = fused
    rnd = M.RandomNetworkDistillation(168, N, T, DEV)
    frame, row = torch.randn(N, 168, device=DEV), torch.zeros(N, 1, device=DEV)
    with torch.inference_mode():
        for t in range(T):
            rnd.rollout_step(frame, row, t)
        step = measure({"rollout_step": lambda: rnd.rollout_step(frame, row, 0)}, calls=50)
    rnd.update(epochs, nmb)                                         # allocations, Adam's state
    torch.cuda.synchronize()
    ts = []
    for _ in range(min(repeats, 7)):
        x, y = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        x.record()
        rnd.update(epochs, nmb)
        y.record()
        y.synchronize()
        ts.append(x.elapsed_time(y))
    rows.append({"what": "rnd steps", "GRX_RND_FUSED": fused, "envs": N, "minibatch_rows": N * T // nmb, "epochs": epochs, "minibatches": nmb,
                 "rollout_step_median_us": step["median_us_per_call"]["rollout_step"], "rollout_step_min_max_us": step["min_max_us_per_call"]["rollout_step"],
                 "update_median_ms": round(statistics.median(ts), 2), "update_min_max_ms": [round(min(ts), 2), round(max(ts), 2)],
                 "update_per_minibatch_step_median_us": round(statistics.median(ts) * 1e3 / (epochs * nmb), 1)})
    print(rows[-1], flush=True)
os.environ.pop("GRX_RND_FUSED")


# ---- full_iteration --------------------------------------------------------------------------------------------------------------------------
def full_iteration(flags):
    from wiki_grx_gym_amd.utils import get_args, task_registry
    args = get_args(["--task", "GR1T1", "--headless", "--num_envs", "4096", "--seed", "1", *flags])
    env, _ = task_registry.make_env("GR1T1", args=args, env_cfg=GR1T1Cfg())
    runner, _ = task_registry.make_alg_runner(env, name=None, args=args, train_cfg=GR1T1CfgPPO(), log_root=None)
    runner.sync_timers = True
    upd = []
    if runner.rnd is not None:                                     # rnd.update() as the loop runs it, the device drained around it
        import time
        inner = runner.rnd.update

        def timed(*a):
            torch.cuda.synchronize()
            t0 = time.time()
            out = inner(*a)
            torch.cuda.synchronize()
            upd.append(time.time() - t0)
            return out
        runner.rnd.update = timed
    runner.learn(2)                                                # graph captures, allocator
    ts = []
    for _ in range(5):
        runner.learn(1)
        ts.append((runner.last_collection_time + runner.last_learn_time, runner.last_collection_time, runner.last_learn_time))
    ts.sort()
    out = {"median_ms": round(ts[2][0] * 1e3, 2), "collection_ms": round(ts[2][1] * 1e3, 2), "learning_ms": round(ts[2][2] * 1e3, 2),
           "min_max_ms": [round(ts[0][0] * 1e3, 2), round(ts[-1][0] * 1e3, 2)]}
    if upd:
        alg = runner.alg
        out.update({"rnd_update_median_ms": round(statistics.median(upd[2:]) * 1e3, 2), "minibatch_steps": alg.num_learning_epochs * alg.num_mini_batches})
    return out


if os.environ.get("RND_TIME_FULL", "1") != "0":
    for flags in ((), ("--rnd",), (), ("--rnd",)):
        rows.append({"what": "full_iteration", "flags": list(flags), "envs": 4096, **full_iteration(flags)})
        print(rows[-1], flush=True)

out = sys.argv[2] if len(sys.argv) > 2 else "profiles/rnd_step_time.json"
doc = {"what": "tools/rnd_time.py on one MI355X", "repeats": repeats, "calls_per_window": CALLS, "rows": rows}
os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
with open(out, "w") as f:
    json.dump(doc, f, indent=1)
print(json.dumps(doc))
