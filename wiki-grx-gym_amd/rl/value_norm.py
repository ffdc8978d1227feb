"""Value normalisation for PPO: the critic network outputs a NORMALISED value, the statistics are a one-column running
normaliser of the rollout's returns, updated once per iteration (skrl's RunningStandardScaler as value_preprocessor, rl_games'
normalize_value; mode "popart": van Hasselt et al. 2016, "Learning values across many orders of magnitude", preserve outputs precisely).

    state        count (int64), mean, var, std, scale (fp32), one element each, starting at 0 / 0 / 1 / 1 / 1 + eps; scale = std + eps
    normalise    x -> (x - mean) / scale          denormalise   v -> v scale + mean          inverses of each other, no clipping
    rollout      everything the critic returns is denormalised before it is used (PPO._act_eager, the captured critic graph -- which reads
                 the state tensors by address --, compute_returns' last values): the storage's values, the time-out bootstrap and GAE work in
                 reward units
    returns      GAE in raw units and the advantages normalised as ever; then the running update from the T N raw returns (the update rule of
                 rl/normalizer.py EmpiricalNormalization); then storage.values and storage.returns are overwritten in place by their
                 normalised images under the NEW statistics.  update() reads the storage as before: the value clip is +-clip_param in
                 normalised units, Loss/value_function is in normalised units
    popart       right after the statistics move, the critic's output layer is rescaled so that the denormalised output of every input is
                 what it was:  W <- W s_old / s_new,  b <- (s_old b + mean_old - mean_new) / s_new   (s = scale).  "running" leaves the network
                 alone.  Adam's moments of that layer are left as they are

On a HIP device the pass is one entry point of libgrx_ppo.so, three launches (include/grx_ppo_gae.h grx_gae_returns); `gae_returns_torch`
is the torch spelling of the same formulas, in place on the same tensors without a host synchronisation: the CPU path and the cross-check,
and what GRX_GAE_FUSED=0 selects on a HIP device.  Not a config key: `--value_norm {running,popart}` or an assignment to
train_cfg.algorithm.value_norm sets it; without it nothing of this module is imported."""
import ctypes as C
import os

import torch
import torch.nn as nn

MODES = ("running", "popart")
MAX_ROWS = 1 << 24   # grx_gae_returns' largest T N


def fused_enabled():
    return os.environ.get("GRX_GAE_FUSED", "1") != "0"


def gae_returns_torch(rewards, values, dones, last_values, gamma, lam, eps, state, returns, advantages, values_out=None, stats=None):
    """the definition of grx_gae_returns in torch, in place: rewards / values / dones / returns / advantages (/ values_out) of one shape
    [T, N] or [T, N, 1], last_values [N] or [N, 1]; state None or (count, mean, var, std, scale), one element each; stats [4] or None.
    Without a state this is RolloutStorage.compute_returns (single rank).  No host synchronisation."""
    T = rewards.shape[0]
    adv = 0
    for step in reversed(range(T)):
        nxt = last_values if step == T - 1 else values[step + 1]
        alive = 1.0 - dones[step].float()
        delta = rewards[step] + alive * gamma * nxt - values[step]
        adv = delta + alive * gamma * lam * adv
        returns[step] = adv + values[step]
    a = returns - values
    mean_a, std_a = a.mean(), a.std()
    advantages.copy_((a - mean_a) / (std_a + 1e-8))
    m, v = returns.mean(), returns.var(unbiased=False)
    if stats is not None:
        stats.copy_(torch.stack([mean_a, std_a, m, v]))
    if state is None:
        return
    count, mean, var, std, scale = state
    n = returns.numel()
    count.add_(n)
    rate = (n / count.double()).to(mean.dtype)
    delta = m - mean
    mean.add_(rate * delta)
    var.add_(rate * (v - var + delta * (m - mean)))
    std.copy_(torch.sqrt(var))
    scale.copy_(std + eps)
    (values_out if values_out is not None else values).copy_((values - mean) / scale)
    returns.copy_((returns - mean) / scale)


def gae_partials(T, N, device):
    """the scratch one grx_gae_returns call at (T, N) needs"""
    from .fused_loss import load_ppo_library
    size = load_ppo_library().grx_gae_partials_size(T, N)
    if size < 1:
        raise RuntimeError(f"grx_gae_partials_size: invalid shape T = {T}, N = {N}")
    with torch.inference_mode(False):
        return torch.empty(size, device=device, dtype=torch.float32)


def gae_returns_hip(rewards, values, dones, last_values, gamma, lam, eps, state, returns, advantages, values_out=None, stats=None, partials=None):
    """the same through grx_gae_returns: contiguous fp32 tensors (dones uint8, count int64) on one HIP device, three launches on the current
    stream; `stats` [4] and `partials` (gae_partials) are allocated here when they are not given"""
    from .fused_loss import load_ppo_library
    lib = load_ppo_library()
    T, N = rewards.shape[0], rewards.shape[1]
    values_out = values if values_out is None else values_out
    fp = [rewards, values, returns, advantages, values_out]
    if not all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.device == rewards.device and t.numel() == T * N for t in fp) \
            or not (dones.is_cuda and dones.dtype == torch.uint8 and dones.is_contiguous() and dones.numel() == T * N) \
            or not (last_values.is_cuda and last_values.dtype == torch.float32 and last_values.is_contiguous() and last_values.numel() == N):
        raise RuntimeError("grx_gae_returns needs contiguous tensors on one HIP device: float32 rewards / values / returns / advantages "
                           "(/ values_out) and uint8 dones with T N elements, float32 last_values with N")
    if state is not None:
        count, mean, var, std, scale = state
        if not (count.is_cuda and count.dtype == torch.int64 and count.numel() == 1) \
                or not all(t.is_cuda and t.dtype == torch.float32 and t.numel() == 1 for t in (mean, var, std, scale)):
            raise RuntimeError("grx_gae_returns needs a state of one-element tensors on the HIP device: count (int64), mean / var / std / scale (float32)")
        sp = [t.data_ptr() for t in state]
    else:
        sp = [None] * 5
    if stats is None:
        with torch.inference_mode(False):
            stats = torch.empty(4, device=rewards.device, dtype=torch.float32)
    part = partials if partials is not None else gae_partials(T, N, rewards.device)
    with torch.cuda.device(rewards.device):
        rc = lib.grx_gae_returns(T, N, rewards.data_ptr(), values.data_ptr(), dones.data_ptr(), last_values.data_ptr(), float(gamma), float(lam),
                                 float(eps), *sp, returns.data_ptr(), advantages.data_ptr(), values_out.data_ptr(), stats.data_ptr(),
                                 part.data_ptr(), C.c_void_p(torch.cuda.current_stream(rewards.device).cuda_stream))
    if rc != 0:
        raise RuntimeError(f"grx_gae_returns failed ({rc}): T = {T}, N = {N}")
    return stats


def popart_rescale(linear, scale_old, mean_old, scale_new, mean_new):
    """the critic's output layer after the statistics moved from (scale_old, mean_old) to (scale_new, mean_new), in place: the denormalised
    output v scale + mean of every input is preserved.  One-element tensors on the layer's device; no host synchronisation."""
    with torch.no_grad():
        linear.weight.mul_(scale_old / scale_new)
        linear.bias.copy_((scale_old * linear.bias + mean_old - mean_new) / scale_new)


def output_layer(critic):
    """the Linear whose output is the value: the last module of an rl.modules.MLP"""
    last = critic.model[-1] if hasattr(critic, "model") else None
    if not isinstance(last, nn.Linear) or last.out_features != 1 or last.bias is None:
        raise ValueError("--value_norm popart needs a critic that ends in a Linear layer with one output and a bias")
    return last


class ValueNormalizer(nn.Module):
    """the state (buffers `count`, `mean`, `var`, `std`, `scale`: state_dict() is all of it) and the rollout's pass over the storage"""

    def __init__(self, mode="running", eps=1e-5, device="cpu"):
        super().__init__()
        if mode not in MODES:
            raise ValueError(f"--value_norm must be one of {MODES}, not {mode!r}")
        if not float(eps) > 0.0:
            raise ValueError(f"value_norm_eps must be > 0, not {eps!r}")
        self.mode, self.eps = mode, float(eps)
        self.register_buffer("count", torch.zeros(1, dtype=torch.long))
        self.register_buffer("mean", torch.zeros(1))
        self.register_buffer("var", torch.ones(1))
        self.register_buffer("std", torch.ones(1))
        self.register_buffer("scale", torch.ones(1) + self.eps)
        self.to(device)
        self._scratch, self._scratch_key = None, None

    def state(self):
        return self.count, self.mean, self.var, self.std, self.scale

    def normalize(self, x):
        return (x - self.mean) / self.scale

    def denormalize(self, v):
        return v * self.scale + self.mean

    def compute_returns(self, storage, last_values, gamma, lam, critic=None):
        """RolloutStorage.compute_returns with value normalisation: `last_values` in reward units; afterwards storage.advantages are the
        normalised advantages, storage.values / storage.returns the normalised values / returns under the statistics just updated, all
        written in place; popart: `critic`'s output layer follows the statistics"""
        st = storage
        if st.returns.numel() > MAX_ROWS:
            raise ValueError(f"--value_norm: a rollout of {st.returns.numel()} transitions per update is more than {MAX_ROWS}")
        if self.mode == "popart":
            layer = output_layer(critic)
            scale_old, mean_old = self.scale.clone(), self.mean.clone()
        last_values = last_values.detach()
        if st.returns.is_cuda and fused_enabled():
            key = (st.num_transitions_per_env, st.num_envs, st.returns.device)
            if self._scratch_key != key:
                with torch.inference_mode(False):
                    stats = torch.zeros(4, device=st.returns.device)
                self._scratch, self._scratch_key = (stats, gae_partials(key[0], key[1], key[2])), key
            gae_returns_hip(st.rewards, st.values, st.dones, last_values.contiguous(), gamma, lam, self.eps, self.state(), st.returns,
                            st.advantages, None, *self._scratch)
        else:
            gae_returns_torch(st.rewards, st.values, st.dones, last_values, gamma, lam, self.eps, self.state(), st.returns, st.advantages)
        if self.mode == "popart":
            popart_rescale(layer, scale_old, mean_old, self.scale, self.mean)

    def checkpoint(self):
        return {"mode": self.mode, "eps": self.eps, "state_dict": self.state_dict()}

    def load_checkpoint(self, saved):
        self.load_state_dict(saved["state_dict"])   # (in place: the captured critic graph reads these tensors by address)
