"""PPO.update() at the GR1T1 train shape (4096 envs x 64 steps, 8 epochs x 25 minibatches, the captured minibatch step), fp32 against
bf16 hidden layers (PPO(precision=...)) in the same process, the two arms interleaved update by update.
    python tools/ppo_precision_ab.py [updates=10] [out.json]   -> one JSON line (and the same result in out.json, if given)
    GRX_AB_ONLY=fp32|bf16 python tools/ppo_precision_ab.py  one arm only (for rocprofv3 --kernel-trace --stats)"""
import json, os, statistics, sys, time
sys.path.insert(0, ".")
import torch
from wiki_grx_gym_amd.rl.modules import ActorCriticMLP
from wiki_grx_gym_amd.rl.ppo import PPO

DEV, N, T = "cuda:0", 4096, 64


def make(precision):
    torch.manual_seed(0)
    ac = ActorCriticMLP(39, 168, 10, actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[512, 256, 128], activation="elu", init_noise_std=0.2)
    alg = PPO(ac, num_learning_epochs=8, num_mini_batches=25, clip_param=0.2, gamma=0.99, lam=0.95, value_loss_coef=1.0, entropy_coef=0.01,
              learning_rate=1e-4, learning_rate_min=1e-5, learning_rate_max=1e-3, max_grad_norm=1.0, use_clipped_value_loss=True,
              schedule="adaptive", desired_kl=0.03, device=DEV, precision=precision)
    alg.init_storage(N, T)
    st = alg.storage
    g = torch.Generator(device=DEV).manual_seed(1)
    for x in (st.observations, st.pri_observations, st.actions, st.rewards, st.values, st.returns, st.advantages, st.mu):
        x.copy_(torch.randn(x.shape, device=DEV, generator=g) * 0.3)
    st.sigma.fill_(0.2); st.actions_log_prob.fill_(-1.0)
    st.step = T
    return alg


def timed(alg):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    alg.update()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


updates = int(sys.argv[1]) if len(sys.argv) > 1 else 10
arms = [os.environ["GRX_AB_ONLY"]] if os.environ.get("GRX_AB_ONLY") else ["fp32", "bf16"]
algs = {p: make(p) for p in arms}
for p in arms:          # warm-up: graph capture, library initialisation
    timed(algs[p])
ts = {p: [] for p in arms}
for _ in range(updates):
    for p in arms:
        ts[p].append(timed(algs[p]))
res = {p: {"median_ms": 1e3 * statistics.median(v), "min_ms": 1e3 * min(v), "max_ms": 1e3 * max(v), "updates": len(v)} for p, v in ts.items()}
if len(arms) == 2:
    res["bf16_over_fp32"] = res["bf16"]["median_ms"] / res["fp32"]["median_ms"]
res["shape"] = "GR1T1 train: 4096 envs x 64 steps, 8 epochs x 25 minibatches of 10485, hidden [512, 256, 128], obs 39 / 168, 10 actions"
print(json.dumps(res), flush=True)
if len(sys.argv) > 2:
    json.dump(res, open(sys.argv[2], "w"), indent=1)
