"""Random network distillation (Burda et al. 2018; rsl_rl 2.x `rnd_cfg`, Schwarke et al. 2023): an intrinsic reward, the
error of a trained predictor against a fixed random target network on the state the env just reached, divided by the running spread of
its own discounted return and added to the env's reward.

    rollout_step(frame, rewards_row, step):
        x = normalizer(frame)                                 RND's own EmpiricalNormalization, training mode: the frame goes in first
        r[n]   = sqrt(sum_e (target(x)[n][e] - predictor(x)[n][e])^2)
        ret[n] = gamma * ret[n] + r[n]                        the per-env discounted return of r (never reset)
        count += N; rate = N / count; m = mean(ret); v = var(ret, unbiased=False); delta = m - mean
        mean += rate * delta; var += rate * (v - var + delta * (m - mean)); std = sqrt(var)
        intrinsic[n] = weight(it) * r[n] / (std + eps);  rewards_row[n] += intrinsic[n]
    update(num_epochs, num_mini_batches):
        ONE randperm over the T x N stored rows, reused by every epoch; per minibatch: predictor forward, mse against the stored target
        embedding, backward, Adam at a fixed learning rate, no clipping; a non-finite loss skips the step

Everything between the two embeddings and the reward row is one entry point of libgrx_ppo.so, three launches (include/grx_ppo.h
grx_rnd_reward); `rnd_reward_torch` is the torch spelling of the same formulas: the CPU path and the cross-check, and what
GRX_RND_FUSED=0 selects on a HIP device.  The update reuses grx_ppo_gather_rows and grx_distill_loss (mse); it runs eagerly, without a
host round trip inside the minibatch loop.  The networks are fp32 whatever PPO's precision is.

The default weight 0.1 is a starting point, not a tuned value."""
import ctypes as C
import os

import torch
import torch.nn as nn
import torch.optim as optim

from .modules import MLP
from .normalizer import EmpiricalNormalization

SCHEDULES = ("constant", "linear", "step")
STATES = ("privileged", "obs")
MAX_OUTPUTS = 256   # grx_rnd_reward's widest row


def _fused_enabled():
    return os.environ.get("GRX_RND_FUSED", "1") != "0"


def weight_at(it, weight=0.1, schedule="constant", final_weight=None, start_it=0, end_it=0, at_it=0):
    """the intrinsic reward's weight at PPO iteration `it`: a pure function.
    constant: weight.  linear: weight up to start_it, final_weight from end_it on, the straight line in between.
    step: weight before at_it, final_weight from at_it on."""
    if schedule == "constant":
        return float(weight)
    if schedule not in SCHEDULES:
        raise ValueError(f"rnd weight schedule must be one of {SCHEDULES}, not {schedule!r}")
    final = float(weight if final_weight is None else final_weight)
    if schedule == "step":
        return float(weight) if it < at_it else final
    if it <= start_it or end_it <= start_it:
        return float(weight) if it <= start_it else final
    if it >= end_it:
        return final
    return float(weight) + (final - float(weight)) * ((it - start_it) / (end_it - start_it))


def rnd_reward_torch(pred, targ, gamma, weight, eps, ret, count, mean, var, std, rewards, intrinsic, raw=None):
    """the definition of grx_rnd_reward in torch, in place on the same tensors: ret [N], count (int64) / mean / var / std one element each,
    rewards [N] in/out, intrinsic [N] and raw [N] (or None) out.  No host synchronisation."""
    N = pred.shape[0]
    d = targ - pred
    r = torch.sqrt((d * d).sum(1))
    ret.mul_(gamma).add_(r)
    count.add_(N)
    rate = (N / count.double()).to(mean.dtype)
    m, v = ret.mean(), ret.var(unbiased=False)
    delta = m - mean
    mean.add_(rate * delta)
    var.add_(rate * (v - var + delta * (m - mean)))
    std.copy_(torch.sqrt(var))
    x = weight * r / (std + eps)
    intrinsic.copy_(x)
    rewards.add_(x)
    if raw is not None:
        raw.copy_(r)


def reward_partials(N, device):
    """the scratch one grx_rnd_reward call at N rows needs (RandomNetworkDistillation keeps one for its rollout)"""
    from .fused_loss import load_ppo_library
    size = load_ppo_library().grx_rnd_reward_partials_size(N)
    if size < 1:
        raise RuntimeError(f"grx_rnd_reward_partials_size: invalid N = {N}")
    with torch.inference_mode(False):
        return torch.empty(size, device=device, dtype=torch.float32)


def rnd_reward_hip(pred, targ, gamma, weight, eps, ret, count, mean, var, std, rewards, intrinsic, raw=None, partials=None):
    """the same through grx_rnd_reward: contiguous fp32 tensors on one HIP device (count int64), three launches on the current stream;
    `partials`: reward_partials(N, device), allocated here when it is not given"""
    from .fused_loss import load_ppo_library
    lib = load_ppo_library()
    N, E = pred.shape
    fp = [pred, targ, ret, mean, var, std, rewards, intrinsic] + ([raw] if raw is not None else [])
    if not all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.device == pred.device for t in fp) \
            or not (count.is_cuda and count.dtype == torch.int64) or targ.shape != pred.shape \
            or any(t.numel() != N for t in (ret, rewards, intrinsic)) or (raw is not None and raw.numel() != N) \
            or any(t.numel() != 1 for t in (count, mean, var, std)):
        raise RuntimeError("grx_rnd_reward needs contiguous float32 tensors on one HIP device: pred / targ [N, E], ret / rewards / intrinsic "
                           "(/ raw) with N elements, count (int64) / mean / var / std with one")
    part = partials if partials is not None else reward_partials(N, pred.device)
    with torch.cuda.device(pred.device):
        rc = lib.grx_rnd_reward(N, E, pred.data_ptr(), targ.data_ptr(), float(gamma), float(weight), float(eps), ret.data_ptr(), count.data_ptr(),
                                mean.data_ptr(), var.data_ptr(), std.data_ptr(), rewards.data_ptr(), intrinsic.data_ptr(),
                                raw.data_ptr() if raw is not None else None, part.data_ptr(),
                                C.c_void_p(torch.cuda.current_stream(pred.device).cuda_stream))
    if rc != 0:
        raise RuntimeError(f"grx_rnd_reward failed ({rc}): {N} x {E}")


class RandomNetworkDistillation(nn.Module):
    """`predictor` (trained) and `target` (frozen, saved) over one raw frame of `num_states` columns, normalised by `normalizer`; the
    discounted-return state `ret` [N], `ret_count`, `ret_mean`, `ret_var`, `ret_std` as buffers: state_dict() is all of RND but its optimizer.
    Stored per rollout: `states` (T, N, S) normalised frames, `targets` (T, N, E) the target's embeddings, `intrinsic` (T, N)."""

    def __init__(self, num_states, num_envs, num_steps, device="cpu", num_outputs=32, predictor_hidden_dims=(256, 128),
                 target_hidden_dims=(256, 128), activation="elu", weight=0.1, weight_schedule="constant", final_weight=None, start_it=0,
                 end_it=0, at_it=0, reward_gamma=0.99, eps=1e-2, learning_rate=1e-3, state="privileged"):
        super().__init__()
        if weight_schedule not in SCHEDULES:
            raise ValueError(f"rnd weight schedule must be one of {SCHEDULES}, not {weight_schedule!r}")
        if state not in STATES:
            raise ValueError(f"rnd state must be one of {STATES}, not {state!r}")
        if not 1 <= int(num_outputs) <= MAX_OUTPUTS:
            raise ValueError(f"rnd num_outputs must be in 1..{MAX_OUTPUTS}, not {num_outputs}")
        S, N, T, E = int(num_states), int(num_envs), int(num_steps), int(num_outputs)
        self.num_states, self.num_envs, self.num_steps, self.num_outputs, self.device = S, N, T, E, device
        self.config = {"state": state, "num_outputs": E, "predictor_hidden_dims": list(predictor_hidden_dims),
                       "target_hidden_dims": list(target_hidden_dims), "activation": activation, "weight": float(weight),
                       "weight_schedule": weight_schedule, "final_weight": None if final_weight is None else float(final_weight),
                       "start_it": int(start_it), "end_it": int(end_it), "at_it": int(at_it), "reward_gamma": float(reward_gamma),
                       "eps": float(eps), "learning_rate": float(learning_rate)}
        self.state, self.reward_gamma, self.eps, self.learning_rate = state, float(reward_gamma), float(eps), float(learning_rate)
        self.predictor = MLP(S, E, predictor_hidden_dims, activation)
        self.target = MLP(S, E, target_hidden_dims, activation)
        for p in self.target.parameters():
            p.requires_grad_(False)
        self.normalizer = EmpiricalNormalization(S)
        self.register_buffer("ret", torch.zeros(N))
        self.register_buffer("ret_count", torch.zeros(1, dtype=torch.long))
        self.register_buffer("ret_mean", torch.zeros(1))
        self.register_buffer("ret_var", torch.ones(1))
        self.register_buffer("ret_std", torch.ones(1))
        self.to(device)
        self.target.eval()
        self.states = torch.zeros(T, N, S, device=device)
        self.targets = torch.zeros(T, N, E, device=device)
        self.intrinsic = torch.zeros(T, N, device=device)
        self.iteration = 0   # the PPO iteration the rollout belongs to: the runner sets it, weight() reads it
        self._on_device = torch.device(device).type == "cuda"
        self._fused = self._on_device and _fused_enabled()
        self._params = list(self.predictor.parameters())
        if self._on_device:   # device-resident, as PPO's: the NaN-skip is Adam's found_inf hook, no host round trip
            self.optimizer = optim.Adam(self._params, lr=torch.tensor(self.learning_rate, device=device), fused=True, capturable=True)
            self._sums = torch.zeros(2, device=device)
        else:
            self.optimizer = optim.Adam(self._params, lr=self.learning_rate)
        self._gather, self._static = None, None
        self._partials = reward_partials(N, device) if self._fused else None

    def train(self, mode=True):
        super().train(mode)
        self.target.eval()   # frozen: whatever mode the rest is in
        return self

    def weight(self, it=None):
        c = self.config
        return weight_at(self.iteration if it is None else it, c["weight"], c["weight_schedule"], c["final_weight"], c["start_it"], c["end_it"],
                         c["at_it"])

    # ---- the rollout -------------------------------------------------------------------------------------------------------------------
    def _embed(self, mlp, x):
        if self._fused:
            from .fused_loss import mlp_can_fuse, mlp_forward
            if mlp_can_fuse(mlp, x):   # libgrx_ppo.so's inference forward: one launch per layer
                return mlp_forward(mlp, x)
        return mlp(x)

    @torch.no_grad()
    def rollout_step(self, frame, rewards_row, step):
        """one env step: `frame` [N, S] the raw frame the env just returned, `rewards_row` the rollout storage's reward row of this step
        (N elements, written by process_env_step already), which gets the intrinsic reward added in place"""
        if not 0 <= step < self.num_steps:
            raise AssertionError("Rollout buffer overflow")
        if frame.dim() != 2 or tuple(frame.shape) != (self.num_envs, self.num_states):
            raise ValueError(f"RandomNetworkDistillation: expected a frame of {(self.num_envs, self.num_states)}, got {tuple(frame.shape)}")
        if rewards_row.numel() != self.num_envs or not rewards_row.is_contiguous():
            raise ValueError("RandomNetworkDistillation: the reward row must be contiguous with one element per env")
        self.normalizer.train()
        x = self.normalizer(frame if frame.is_contiguous() else frame.contiguous())
        self.states[step].copy_(x)
        x = self.states[step]
        pred = self._embed(self.predictor, x)
        self.targets[step].copy_(self._embed(self.target, x))
        args = (pred, self.targets[step], self.reward_gamma, self.weight(), self.eps, self.ret, self.ret_count, self.ret_mean, self.ret_var,
                self.ret_std, rewards_row.view(-1), self.intrinsic[step])
        if self._fused:
            rnd_reward_hip(*args, partials=self._partials)
        else:
            rnd_reward_torch(*args)

    # ---- the update --------------------------------------------------------------------------------------------------------------------
    def _loss(self, x, y):
        from .distillation import distill_loss
        return distill_loss(self.predictor(x), y, "mse", self._fused)

    def update(self, num_epochs, num_mini_batches):
        """the predictor's regression on the stored rollout; returns the mean loss over the steps with a finite loss (0.0: none)"""
        rows = self.num_steps * self.num_envs
        mb = rows // int(num_mini_batches)
        states, targets = self.states.flatten(0, 1), self.targets.flatten(0, 1)
        indices = torch.randperm(int(num_mini_batches) * mb, requires_grad=False, device=self.device)   # one permutation, every epoch
        self.predictor.train()
        if not self._on_device:
            total, steps = 0.0, 0
            for _ in range(int(num_epochs)):
                for i in range(int(num_mini_batches)):
                    idx = indices[i * mb:(i + 1) * mb]
                    loss = self._loss(states[idx], targets[idx])
                    if not torch.isfinite(loss):
                        continue
                    self.optimizer.zero_grad(set_to_none=False)
                    loss.backward()
                    self.optimizer.step()
                    total, steps = total + loss.item(), steps + 1
            return total / steps if steps else 0.0
        sums = self._sums.zero_()
        gather = None
        if self._fused:   # the two minibatch tensors in one launch (grx_ppo_gather_rows)
            from .fused_loss import RowGather
            if self._static is None or self._static[0].shape[0] != mb:
                self._static = [torch.empty(mb, self.num_states, device=self.device), torch.empty(mb, self.num_outputs, device=self.device)]
                self._gather = RowGather([states, targets], self._static)
            gather = self._gather
        for _ in range(int(num_epochs)):
            for i in range(int(num_mini_batches)):
                idx = indices[i * mb:(i + 1) * mb]
                if gather is not None:
                    gather(idx)
                    xb, yb = self._static
                else:
                    xb, yb = states[idx], targets[idx]
                loss = self._loss(xb, yb)
                self.optimizer.zero_grad(set_to_none=False)
                loss.backward()
                with torch.no_grad():
                    loss = loss.detach()
                    bad = ~torch.isfinite(loss)
                    self.optimizer.found_inf = bad.float().reshape(())   # (fused Adam leaves parameters and moments alone where it is 1)
                    self.optimizer.grad_scale = None
                self.optimizer.step()
                with torch.no_grad():
                    sums[0] += torch.where(bad, 0.0, loss)
                    sums[1] += (~bad).float()
        total, steps = sums.tolist()                               # the only device->host transfer of the update
        return total / steps if steps else 0.0

    # ---- the checkpoint's "rnd" entry ----------------------------------------------------------------------------------------------------
    def checkpoint(self):
        return {"state_dict": self.state_dict(), "optimizer_state_dict": self.optimizer.state_dict(), "config": dict(self.config)}

    def load_checkpoint(self, saved, load_optimizer=True):
        """both networks, the normaliser, the discounted-return state and -- load_optimizer -- the optimizer of a saved "rnd" entry; the
        schedule and the learning rate stay this run's.  A checkpoint of another number of envs keeps everything but `ret`, the one per-env
        tensor, which restarts from zeros with one printed line.  ValueError when the networks or the state's width are other than this run's."""
        for k in ("state", "num_outputs", "predictor_hidden_dims", "target_hidden_dims", "activation"):
            if saved["config"][k] != self.config[k]:
                raise ValueError(f"the checkpoint's rnd entry has {k}={saved['config'][k]!r}, this run {self.config[k]!r}")
        sd = dict(saved["state_dict"])
        if tuple(sd["normalizer._mean"].shape) != (1, self.num_states):
            raise ValueError(f"the checkpoint's rnd entry holds {sd['normalizer._mean'].shape[1]} state columns, this run {self.num_states}")
        if tuple(sd["ret"].shape) != tuple(self.ret.shape):
            print(f"the checkpoint's rnd entry holds the discounted returns of {sd['ret'].shape[0]} envs, this run has {self.num_envs}: they restart "
                  "from zero (networks and statistics are kept)")
            sd["ret"] = torch.zeros_like(self.ret)
        self.load_state_dict(sd)
        if not load_optimizer:
            return
        self.optimizer.load_state_dict(saved["optimizer_state_dict"])
        if self._on_device:   # torch replaces the learning-rate tensor and may bring host step counters (PPO.load_optimizer_state)
            for g in self.optimizer.param_groups:
                g["lr"] = torch.tensor(self.learning_rate, device=self.device)
                g["fused"], g["capturable"], g["foreach"] = True, True, False
            for stt in self.optimizer.state.values():
                for k, v in list(stt.items()):
                    if torch.is_tensor(v):
                        stt[k] = v.to(device=self.device, dtype=torch.float32 if k == "step" else v.dtype)
                    elif k == "step":
                        stt[k] = torch.tensor(float(v), device=self.device)
        else:
            for g in self.optimizer.param_groups:
                g["lr"] = self.learning_rate
