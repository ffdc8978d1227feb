"""What action-smoothness regularisation (--smooth) costs.  Nothing here is a target:
  * the captured minibatch step at 4096 envs x 24 steps, 4 minibatches (24576 rows), the GR1T1 networks: PPO.update() of EPOCHS epochs on
    a filled storage, divided by its 4 EPOCHS steps (gather + replay; the update's one read-back is in it), for the default, --smooth
    temporal / spatial / both, and both under GRX_SMOOTH_FUSED=0 (the torch gather outside and the torch loss inside the captured step).
    The arms ALTERNATE in one process; REPEATS timed updates per arm after two warm-up updates (the first captures), median and spread.
  * the gather alone and the loss alone (forward and backward) at that shape, HIP against the torch spelling, CALLS back-to-back calls
    per window between two device events.
    python tools/smooth_time.py [repeats=15] [out=profiles/smooth_step_time.json]   (the JSON line is printed too)"""
import json, os, statistics, sys; sys.path.insert(0, ".")
import torch
from wiki_grx_gym_amd.rl import smooth as S
from wiki_grx_gym_amd.rl.modules import ActorCriticMLP
from wiki_grx_gym_amd.rl.ppo import PPO
repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 15
CALLS, EPOCHS, N, T, MINI = 200, 8, 4096, 24, 4
DEV = "cuda:0"
assert torch.cuda.is_available(), "smooth_time.py measures on the GPU: there is no fallback"


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def measure(arms, calls, reps, warm=1):
    ts = {k: [] for k in arms}
    for fn in arms.values():
        for _ in range(warm):
            window(fn, calls)
    for _ in range(reps):
        for k, fn in arms.items():
            ts[k].append(window(fn, calls))
    return ({k: round(statistics.median(v), 2) for k, v in ts.items()}, {k: [round(min(v), 2), round(max(v), 2)] for k, v in ts.items()})


def filled_ppo(mode):
    torch.manual_seed(1)
    ac = ActorCriticMLP(39, 168, 10, actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[512, 256, 128], activation="elu", init_noise_std=0.2)
    alg = PPO(actor_critic=ac, device=DEV, num_learning_epochs=EPOCHS, num_mini_batches=MINI, learning_rate=1e-5, schedule="adaptive",
              desired_kl=0.01, entropy_coef=0.0, smooth=mode)
    alg.init_storage(N, T)
    st = alg.storage
    with torch.no_grad():
        for name in ("observations", "pri_observations", "actions", "mu", "values", "returns", "advantages", "actions_log_prob"):
            getattr(st, name).normal_()
        st.sigma.fill_(0.2)
        st.dones.copy_((torch.rand(st.dones.shape, device=DEV) < 0.02).to(torch.uint8))
    st.step = T
    return alg


# ---- the captured step -------------------------------------------------------------------------------------------------------------------
arms, algs = {}, {}
for name, mode, fused in (("default", None, "1"), ("temporal", "temporal", "1"), ("spatial", "spatial", "1"), ("both", "both", "1"),
                          ("both_GRX_SMOOTH_FUSED=0", "both", "0")):
    alg = algs[name] = filled_ppo(mode)

    def update(alg=alg, fused=fused):
        os.environ["GRX_SMOOTH_FUSED"] = fused
        alg.update()
    arms[name] = update
med, spread = measure(arms, calls=1, reps=repeats, warm=2)
os.environ.pop("GRX_SMOOTH_FUSED")
assert all(isinstance(a._graph, torch.cuda.CUDAGraph) for a in algs.values())
steps = EPOCHS * MINI
step = {"what": "one captured minibatch step (gather + replay) = PPO.update() / (epochs x minibatches)",
        "shape": {"envs": N, "steps": T, "minibatches": MINI, "rows_per_minibatch": N * T // MINI, "epochs_per_update": EPOCHS},
        "median_us_per_step": {k: round(v / steps, 1) for k, v in med.items()},
        "min_max_us_per_step": {k: [round(t / steps, 1) for t in v] for k, v in spread.items()},
        "actor_rows_per_step": {"default": 1, "temporal": 2, "spatial": 2, "both": 3},
        "expectation": "roughly the default's step plus the actor's forward and backward on the extra row blocks (written down, not asserted)"}
print(step, flush=True)

# ---- the gather and the loss alone ---------------------------------------------------------------------------------------------------------
alg = algs["both"]
mb = N * T // MINI
srcs = alg._smooth_sources()
idx = torch.randperm(N * T, device=DEV)[:mb].contiguous()
os.environ["GRX_SMOOTH_FUSED"] = "1"
hip_gather = alg._smooth_gatherer(srcs, alg._static)
os.environ["GRX_SMOOTH_FUSED"] = "0"
torch_gather = alg._smooth_gatherer(srcs, alg._static)
os.environ.pop("GRX_SMOOTH_FUSED")
assert type(hip_gather.gather).__name__ == "SmoothGather" and type(torch_gather.gather).__name__ != "SmoothGather"
with torch.inference_mode():
    g_med, g_spread = measure({"hip": lambda: hip_gather(idx), "torch": lambda: torch_gather(idx)}, CALLS, repeats)
mu = torch.randn(3 * mb, 10, device=DEV, requires_grad=True)
valid = (torch.rand(mb, device=DEV) < 0.9).to(torch.uint8)


def loss_arm(fused):
    def run():
        mu.grad = None
        S.smooth_loss(mu, True, True, valid, 0.1, 0.1, fused=fused)[0].backward()
    return run
l_med, l_spread = measure({"hip": loss_arm(True), "torch": loss_arm(False)}, CALLS, repeats)
parts = {"what": "the gather (nine tensors, the noise draw included) and the loss (forward + backward through autograd) alone, mode both",
         "rows": mb, "gather_median_us": g_med, "gather_min_max_us": g_spread, "loss_median_us": l_med, "loss_min_max_us": l_spread}
print(parts, flush=True)
out = {"what": "action-smoothness regularisation: the captured minibatch step per mode, and the HIP gather and loss against their torch spellings",
       "device": torch.cuda.get_device_name(0), "repeats": repeats, "calls_per_window": CALLS, "step": step, "parts": parts}
print(json.dumps(out))
json.dump(out, open(sys.argv[2] if len(sys.argv) > 2 else "profiles/smooth_step_time.json", "w"), indent=1)
