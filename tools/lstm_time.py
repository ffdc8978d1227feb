"""What the recurrent policy (--recurrent) costs.  Three measurements, nothing here is a target:
  * the cell: grx_lstm_cell (one launch) against its torch spelling (rl.recurrent.lstm_cell_torch: two GEMMs and the element-wise
    kernels) at M = 4096, H = 256, D = GR1T1's observation (39) and privileged (168) widths.  The two arms ALTERNATE in one process; a
    timed window is CALLS back-to-back calls between two device events, REPEATS windows per arm after a warm-up window, median and
    spread per call in microseconds.  Both arms' results are compared before they are timed.
  * one recurrent minibatch step at the GR1T1 train shape (4096 envs, 64 steps, 25 minibatches of 163 envs, H = 256): PPO.update() over one
    epoch on a filled storage, divided by its 25 steps; fused against GRX_LSTM_FUSED=0.
  * full_iteration: OnPolicyRunner.learn(1) of a GR1T1 run with --recurrent beside the default's, both at 4096 envs, timers synchronised.
    python tools/lstm_time.py [repeats=15] [out=profiles/lstm_step_time.json]   (the JSON line is printed too)"""
import json, os, statistics, sys, time; sys.path.insert(0, ".")
import torch
from wiki_grx_gym_amd.rl import recurrent as L
from wiki_grx_gym_amd.rl.ppo import PPO
repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 15
CALLS = 500
DEV = "cuda:0"
assert torch.cuda.is_available(), "lstm_time.py measures on the GPU: there is no fallback"


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
# ---- the cell ------------------------------------------------------------------------------------------------------------------------------
M, H = 4096, 256
for D in (39, 168):
    torch.manual_seed(D)
    w = [p.detach().to(DEV) for p in L.Memory(D, H)._weights()]
    x, hp, cp = torch.randn(M, D, device=DEV), torch.tanh(torch.randn(M, H, device=DEV)), torch.randn(M, H, device=DEV)
    reset = (torch.arange(M, device=DEV) % 50 == 0).to(torch.uint8)   # about 2 % of the envs end per step, as in training
    h, c = torch.empty(M, H, device=DEV), torch.empty(M, H, device=DEV)
    hip = lambda: L.lstm_cell_hip(x, hp, cp, reset, *w, h, c)
    spelled = lambda: L.lstm_cell_torch(x, hp, cp, reset, *w)
    hip()
    ht, ct, _ = spelled()
    err = max(float((h - ht).abs().max()), float((c - ct).abs().max()))
    assert err < 1e-5, err
    with torch.inference_mode():
        rows.append({"what": "cell", "shape": [M, D, H], "flop": 2 * M * 4 * H * (D + H), "max_abs_difference_between_the_arms": err,
                     **measure({"hip": hip, "torch": spelled})})
    print(rows[-1], flush=True)


# ---- one recurrent minibatch step ------------------------------------------------------------------------------------------------------------
def filled_ppo():
    torch.manual_seed(1)
    ac = L.ActorCriticRecurrent(39, 168, 10, rnn_hidden_size=H, actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[512, 256, 128], init_noise_std=0.2)
    alg = PPO(actor_critic=ac, device=DEV, num_learning_epochs=1, num_mini_batches=25, learning_rate=1e-4, schedule="adaptive", desired_kl=0.01,
              entropy_coef=0.0)
    alg.init_storage(4096, 64)
    st = alg.storage
    with torch.no_grad():
        for name in ("observations", "pri_observations", "actions", "mu", "values", "returns", "advantages", "actions_log_prob"):
            getattr(st, name).normal_()
        st.sigma.fill_(0.2)
        st.dones.copy_((torch.rand(st.dones.shape, device=DEV) < 0.02).to(torch.uint8))
    return alg


step = {}
for fused in ("1", "0"):
    os.environ["GRX_LSTM_FUSED"] = fused
    alg = filled_ppo()
    step["hip" if fused == "1" else "torch"] = measure({"update": alg.update}, calls=1, reps=max(3, repeats // 3))
os.environ.pop("GRX_LSTM_FUSED")
rows.append({"what": "one recurrent minibatch step = PPO.update() of one epoch / 25", "shape": {"envs_per_minibatch": 163, "steps": 64, "H": H},
             "median_us_per_step": {k: round(v["median_us_per_call"]["update"] / 25, 1) for k, v in step.items()},
             "min_max_us_per_step": {k: [round(t / 25, 1) for t in v["min_max_us_per_call"]["update"]] for k, v in step.items()}})
print(rows[-1], flush=True)


# ---- full_iteration --------------------------------------------------------------------------------------------------------------------------
def iteration_times(flags, iterations=5, warmup=2):
    from wiki_grx_gym_amd.envs import GR1T1CfgPPO
    from wiki_grx_gym_amd.utils import get_args, task_registry
    args = get_args(["--task", "GR1T1", "--headless", "--num_envs", "4096", "--seed", "3", *flags])
    env, _ = task_registry.make_env("GR1T1", args=args)
    runner, _ = task_registry.make_alg_runner(env, name=None, args=args, train_cfg=GR1T1CfgPPO(), log_root=None)
    runner.sync_timers = True
    out = []
    for i in range(warmup + iterations):
        runner.learn(num_learning_iterations=1, init_at_random_ep_len=(i == 0))
        torch.cuda.synchronize()
        if i >= warmup:
            out.append((runner.last_collection_time, runner.last_learn_time))
    col, lrn = [c for c, _ in out], [l for _, l in out]
    return {"collection_s": round(statistics.median(col), 4), "learning_s": round(statistics.median(lrn), 4),
            "full_iteration_s": round(statistics.median([c + l for c, l in out]), 4), "iterations": iterations}


full = {"default": iteration_times([]), "recurrent": iteration_times(["--recurrent"])}
print(full, flush=True)
out = {"what": "the recurrent policy: the HIP cell against its torch spelling, one recurrent minibatch step, a full iteration beside the default's",
       "device": torch.cuda.get_device_name(0), "calls_per_window": CALLS, "repeats": repeats, "rows": rows, "full_iteration": full}
print(json.dumps(out))
json.dump(out, open(sys.argv[2] if len(sys.argv) > 2 else "profiles/lstm_step_time.json", "w"), indent=1)
