"""What the recurrent distillation student (--distill_from ... --student_recurrent) costs.  Nothing here is a target:
  * the backward step: grx_lstm_bptt_step (one launch; every block width of the measurement hook) against the three-launch spelling of
    LSTMSequence.backward -- dG_next @ W_hh under the update's rocBLAS preference, addcmul, grx_lstm_cell_backward -- at (M, H) = (4096, 256)
    and (163, 256).  The arms ALTERNATE in one process; a timed window is CALLS back-to-back calls between two device events, REPEATS
    windows per arm after a warm-up window, median and spread per call in microseconds.  The arms' results are compared before they are timed.
  * one window: Memory.sequence_bptt forward plus backward at 15 steps x 4096 envs, D = 39, H = 256; fused against GRX_LSTM_BPTT_FUSED=0.
  * full_iteration: OnPolicyRunner.learn(1) of a GR1T1 distillation run at 4096 envs, 64 steps, one epoch, one env range: the MLP student,
    the recurrent student with the fused step, the recurrent student with GRX_LSTM_BPTT_FUSED=0; timers synchronised.
    python tools/bptt_time.py [repeats=9] [out=profiles/recurrent_student_step_time.json]   (the JSON line is printed too)"""
import json, os, statistics, sys, tempfile; sys.path.insert(0, ".")
import torch
from wiki_grx_gym_amd.rl import recurrent as L
repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 9
CALLS = 200
DEV = "cuda:0"
assert torch.cuda.is_available(), "bptt_time.py measures on the GPU: there is no fallback"


def window(fn, calls):
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
torch.backends.cuda.preferred_blas_library("cublas")              # rocBLAS, as Distillation.update() prefers for its products
# ---- the backward step -----------------------------------------------------------------------------------------------------------------------
H = 256
for M in (4096, 163):
    torch.manual_seed(M)
    w_hh = (torch.randn(4 * H, H, device=DEV) / 16).contiguous()
    dGn, dh_out, dc_in, c_prev = torch.randn(M, 4 * H, device=DEV), torch.randn(M, H, device=DEV), torch.randn(M, H, device=DEV), torch.randn(M, H, device=DEV)
    pre = torch.randn(M, 5 * H, device=DEV)
    acts = torch.cat([torch.sigmoid(pre[:, :2 * H]), torch.tanh(pre[:, 2 * H:3 * H]), torch.sigmoid(pre[:, 3 * H:4 * H]), torch.tanh(pre[:, 4 * H:])], 1).contiguous()
    reset = (torch.arange(M, device=DEV) % 50 == 0).to(torch.uint8)    # about 2 % of the envs end per step, as in training
    reset_next = (torch.arange(M, device=DEV) % 50 == 1).to(torch.uint8)
    keep = (reset_next == 0).float().unsqueeze(-1)
    outs = {k: (torch.empty(M, 4 * H, device=DEV), torch.empty(M, H, device=DEV)) for k in ("fused", "tile32", "tile64", "tile128", "spelling")}

    def spelled(o=outs["spelling"]):
        dh = torch.addcmul(dh_out, dGn @ w_hh, keep)
        L.lstm_cell_backward_hip(dh, dc_in, acts, c_prev, reset, *o)

    def fused(tile, o):
        return lambda: L.lstm_bptt_step_hip(dGn, w_hh, reset_next, dh_out, dc_in, acts, c_prev, reset, *o, tile_units=tile)
    arms = {"fused": fused(None, outs["fused"]), "tile32": fused(32, outs["tile32"]), "tile64": fused(64, outs["tile64"]),
            "tile128": fused(128, outs["tile128"]), "spelling": spelled}
    for fn in arms.values():
        fn()
    assert all(torch.equal(outs["fused"][i], outs[k][i]) for k in ("tile32", "tile64", "tile128") for i in (0, 1))
    err = max(float((outs["fused"][i] - outs["spelling"][i]).abs().max()) for i in (0, 1))
    assert err < 1e-3, err
    rows.append({"what": "backward step", "shape": [M, H], "flop": 2 * M * 4 * H * H, "max_abs_difference_fused_spelling": err, **measure(arms)})
    print(rows[-1], flush=True)

# ---- one window: forward plus backward ---------------------------------------------------------------------------------------------------------
T, N, D = 15, 4096, 39
torch.manual_seed(2)
mem = L.Memory(D, H).to(DEV)
x, wgt = torch.randn(T, N, D, device=DEV), torch.randn(T, N, H, device=DEV)
resets = (torch.rand(T, N, device=DEV) < 0.02).to(torch.uint8)
h0, c0 = torch.zeros(N, H, device=DEV), torch.zeros(N, H, device=DEV)


def one_window():
    for p in mem.rnn.parameters():
        p.grad = None
    out, _, _ = mem.sequence_bptt(x, resets, h0, c0)
    (out * wgt).sum().backward()


win = {}
for fused_flag in ("1", "0"):
    os.environ["GRX_LSTM_BPTT_FUSED"] = fused_flag
    win["fused" if fused_flag == "1" else "spelling"] = measure({"window": one_window}, calls=5, reps=repeats)
os.environ.pop("GRX_LSTM_BPTT_FUSED")
rows.append({"what": "one window: Memory.sequence_bptt forward + backward", "shape": {"steps": T, "envs": N, "D": D, "H": H},
             "median_us": {k: v["median_us_per_call"]["window"] for k, v in win.items()},
             "min_max_us": {k: v["min_max_us_per_call"]["window"] for k, v in win.items()}})
print(rows[-1], flush=True)


# ---- full_iteration --------------------------------------------------------------------------------------------------------------------------
def runner_for(flags, root=None):
    from wiki_grx_gym_amd.envs import GR1T1CfgPPO
    from wiki_grx_gym_amd.utils import get_args, task_registry
    args = get_args(["--task", "GR1T1", "--headless", "--num_envs", "4096", "--seed", "3", *flags])
    env, _ = task_registry.make_env("GR1T1", args=args)
    tcfg = GR1T1CfgPPO()
    tcfg.runner.num_steps_per_env = 64
    if "--distill_from" in flags:
        tcfg.algorithm.num_learning_epochs, tcfg.algorithm.num_mini_batches = 1, 1
    return task_registry.make_alg_runner(env, name=None, args=args, train_cfg=tcfg, log_root=root)[0]


def iteration_times(flags, iterations=4, warmup=2):
    runner = runner_for(flags)
    runner.sync_timers = True
    out = []
    for i in range(warmup + iterations):
        runner.learn(num_learning_iterations=1, init_at_random_ep_len=(i == 0))
        torch.cuda.synchronize()
        if i >= warmup:
            out.append((runner.last_collection_time, runner.last_learn_time))
    col, lrn = [c for c, _ in out], [l for _, l in out]
    return {"collection_s": round(statistics.median(col), 4), "learning_s": round(statistics.median(lrn), 4),
            "full_iteration_s": round(statistics.median([c + l for c, l in out]), 4), "iterations": iterations,
            "optimizer_steps_per_iteration": runner.alg.num_updates}


with tempfile.TemporaryDirectory() as tmp:
    teacher = runner_for(["--privileged_actor"], root=tmp)
    teacher.learn(num_learning_iterations=1, init_at_random_ep_len=True)
    path = os.path.join(teacher.log_dir, "model_1.pt")
    del teacher
    full = {"mlp_student": iteration_times(["--distill_from", path])}
    for fused_flag in ("1", "0"):
        os.environ["GRX_LSTM_BPTT_FUSED"] = fused_flag
        full["recurrent_student_fused" if fused_flag == "1" else "recurrent_student_spelling"] = iteration_times(
            ["--distill_from", path, "--student_recurrent", "--rnn_hidden_size", str(H)])
    os.environ.pop("GRX_LSTM_BPTT_FUSED")
print(full, flush=True)
out = {"what": "the recurrent distillation student: grx_lstm_bptt_step against the three-launch spelling, one BPTT window, a full distillation "
               "iteration (4096 envs, 64 steps, one epoch, one env range, windows of 15 steps) beside the MLP student's",
       "device": torch.cuda.get_device_name(0), "calls_per_window": CALLS, "repeats": repeats, "rows": rows, "full_iteration": full}
print(json.dumps(out))
json.dump(out, open(sys.argv[2] if len(sys.argv) > 2 else "profiles/recurrent_student_step_time.json", "w"), indent=1)
