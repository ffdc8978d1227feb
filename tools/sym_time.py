"""What left-right symmetry (--symmetry) costs.  Two measurements, nothing here is a target:
  * the gather: grx_sym_gather_rows (one launch for the nine minibatch tensors and both halves) against its torch spelling
    (rl.symmetry.sym_gather_torch, GRX_SYM_FUSED=0) at the GR1T1 train shape -- 4096 envs x the steps and minibatches GR1T1CfgPPO gives --,
    for "both" (every tensor mirrored or repeated) and "loss" (obs alone), with normalised (affine) maps.  The two arms ALTERNATE in one
    process; a timed window is CALLS back-to-back calls between two device events, REPEATS windows per arm after a warm-up window, median and
    spread per call in microseconds.  Both arms' results are compared before they are timed.
  * full_iteration: OnPolicyRunner.learn(1) of a GR1T1 run at 4096 envs with each mode beside the default's, timers synchronised.
    python tools/sym_time.py [repeats=15] [out=profiles/sym_step_time.json]   (the JSON line is printed too)"""
import json, os, statistics, sys; sys.path.insert(0, ".")
import torch
from wiki_grx_gym_amd.envs import GR1T1Cfg, GR1T1CfgPPO
from wiki_grx_gym_amd.rl import symmetry as S
from wiki_grx_gym_amd.rl.fused_loss import RowGather, SymGather
repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 15
CALLS = 200
DEV = "cuda:0"
assert torch.cuda.is_available(), "sym_time.py measures on the GPU: there is no fallback"


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
# ---- the gather ------------------------------------------------------------------------------------------------------------------------------
tcfg = GR1T1CfgPPO()
N, T, nmb = 4096, int(tcfg.runner.num_steps_per_env), int(tcfg.algorithm.num_mini_batches)
mb = N * T // nmb
names = ['left_hip_roll_joint', 'left_hip_yaw_joint', 'left_hip_pitch_joint', 'left_knee_pitch_joint', 'left_ankle_pitch_joint',
         'right_hip_roll_joint', 'right_hip_yaw_joint', 'right_hip_pitch_joint', 'right_knee_pitch_joint', 'right_ankle_pitch_joint']
pts = GR1T1Cfg.terrain.measured_points_x
torch.manual_seed(0)
obs_map, pri_map, act_map = S.MirrorMap(*S.frame_map(names), DEV), S.MirrorMap(*S.privileged_map(names, pts, pts), DEV), S.MirrorMap(*S.joint_map(names), DEV)
for m in (obs_map, pri_map):   # what a normaliser leaves: a scale that is no sign and an offset
    m.scale.mul_(torch.rand(m.width, device=DEV) + 0.5)
    m.offset = torch.randn(m.width, device=DEV)
maps = [obs_map, pri_map, act_map, None, None, None, None, act_map, act_map.abs_scale()]
widths = [39, 168, 10, 1, 1, 1, 1, 10, 10]
srcs = [torch.randn(nmb * mb, w, device=DEV) for w in widths]
idx = torch.randperm(nmb * mb, device=DEV)[:mb].contiguous()
plain = [torch.empty(mb, w, device=DEV) for w in widths]
row_gather = RowGather(srcs, plain)
for mode, modes in (("both", [2, 2, 2, 1, 1, 1, 1, 2, 2]), ("loss", [2, 0, 0, 0, 0, 0, 0, 0, 0])):
    a = [torch.empty(mb * (2 if m else 1), w, device=DEV) for m, w in zip(modes, widths)]
    b = [torch.empty_like(t) for t in a]
    hip = SymGather(srcs, a, modes, maps)
    hip(idx)
    S.sym_gather_torch(srcs, b, modes, maps, idx)
    torch.cuda.synchronize()
    err = max(float((x - y).abs().max()) for x, y in zip(a, b))
    assert err < 1e-5, err
    moved = sum(4 * t.numel() for t in a) + sum(4 * mb * w for w in widths)   # bytes written + source rows read once
    with torch.inference_mode():
        rows.append({"what": "gather", "mode": mode, "minibatch_rows": mb, "bytes_moved": moved, "max_abs_difference_between_the_arms": err,
                     **measure({"hip": lambda: hip(idx), "torch": lambda: S.sym_gather_torch(srcs, b, modes, maps, idx),
                                "row_gather_without_symmetry": lambda: row_gather(idx)})})
    print(rows[-1], flush=True)


# ---- full_iteration --------------------------------------------------------------------------------------------------------------------------
def full_iteration(flags):
    from wiki_grx_gym_amd.utils import get_args, task_registry
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
    return {"median_ms": round(ts[2][0] * 1e3, 2), "collection_ms": round(ts[2][1] * 1e3, 2), "learning_ms": round(ts[2][2] * 1e3, 2),
            "min_max_ms": [round(ts[0][0] * 1e3, 2), round(ts[-1][0] * 1e3, 2)]}


if os.environ.get("SYM_TIME_FULL", "1") != "0":
    for flags in ((), ("--symmetry", "augment"), ("--symmetry", "loss"), ("--symmetry", "both")):
        rows.append({"what": "full_iteration", "flags": list(flags), "envs": 4096, **full_iteration(flags)})
        print(rows[-1], flush=True)

out = sys.argv[2] if len(sys.argv) > 2 else "profiles/sym_step_time.json"
doc = {"what": "tools/sym_time.py on one MI355X", "repeats": repeats, "calls_per_window": CALLS, "rows": rows}
os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
with open(out, "w") as f:
    json.dump(doc, f, indent=1)
print(json.dumps(doc))
