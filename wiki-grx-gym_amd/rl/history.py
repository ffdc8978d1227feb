"""Observation history (humanoid-gym `frame_stack`, Isaac Lab / rsl_rl 2.x `history_length`): the policy sees the last H
frames of an observation of width D instead of one.  The stacked row of env n is H frames, OLDEST FIRST, newest last (width H * D):

    push(x, dones), after env.step returned frame x and dones:
        dones[n] false:  new[n] = concat(old[n][D:], x[n])
        dones[n] true:   new[n] = x[n] repeated H times     (the frame a finished env returns is already the first frame of its new
                                                             episode: nothing crosses an episode boundary, no artificial zeros)
    fill(x), the first frame (after construction, after env.reset(), on request):  every row is x[n] repeated H times

Push is OUT OF PLACE between two buffers that alternate: the runner keeps a reference to step t's actor input until process_env_step
stores it, after step t+1's input has been built (the normaliser's two-slot ring exists for the same reason).

Contiguous fp32 CUDA frames go through libgrx_ppo.so (include/grx_ppo.h grx_obs_history_push: one launch, pure copies); everything
else (CPU, strided input) through the torch spelling of the same definition below.  Both only copy: they agree bit for bit."""
import ctypes as C

import torch
from torch import nn


def _as_u8(dones):
    """one byte per env, as fused_loss.store_transition takes it: bool is reinterpreted, any other dtype converted"""
    if dones.dtype == torch.bool:
        return dones.view(torch.uint8)
    if dones.dtype != torch.uint8:
        return (dones != 0).to(torch.uint8)
    return dones


def stack_torch(x, dones, src, length):
    """the definition in torch: the new stacked rows [N, length * D] from the frame x [N, D], dones [N] (None: every row is filled) and
    the old rows src"""
    filled = x.repeat(1, length)
    if dones is None or length == 1:
        return filled
    shifted = torch.cat([src[:, x.shape[1]:], x], dim=1)
    return torch.where((dones != 0).view(-1, 1), filled, shifted)


class ObsHistory:
    def __init__(self, num_envs, dim, length, device="cpu"):
        self.num_envs, self.dim, self.length = int(num_envs), int(dim), int(length)
        if self.num_envs < 1 or self.dim < 1 or self.length < 1:
            raise ValueError(f"ObsHistory: num_envs, dim and length must be >= 1, got {num_envs}, {dim}, {length}")
        if self.num_envs * self.dim * self.length >= 2 ** 31:
            raise ValueError(f"ObsHistory: {num_envs} x {length} x {dim} elements do not fit a 32-bit index")
        with torch.inference_mode(False):   # (the rollout runs under inference_mode; these are written there at every step)
            self._buf = (torch.zeros(self.num_envs, self.length * self.dim, device=device, dtype=torch.float32),
                         torch.zeros(self.num_envs, self.length * self.dim, device=device, dtype=torch.float32))
        self._slot = 0          # which buffer holds the current rows
        self.primed = False     # False until the first fill: `current` is meaningless before

    @property
    def current(self):
        return self._buf[self._slot]

    # ---- which path -------------------------------------------------------------------------------------------------------------
    def _hip(self, x):
        return x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.device == self._buf[0].device

    def _check(self, x, dones):
        if x.dim() != 2 or tuple(x.shape) != (self.num_envs, self.dim):
            raise ValueError(f"ObsHistory({self.num_envs}, {self.dim}, {self.length}): expected a frame [{self.num_envs}, {self.dim}], got {tuple(x.shape)}")
        if dones is not None and dones.numel() != self.num_envs:
            raise ValueError(f"ObsHistory: expected {self.num_envs} dones, got {tuple(dones.shape)}")

    def _write(self, x, dones):
        """the rows after frame x into the buffer that is not current, which becomes current"""
        self._check(x, dones)
        src, dst = self._buf[self._slot], self._buf[self._slot ^ 1]
        if self._hip(x):
            from .fused_loss import load_ppo_library
            lib = load_ppo_library()   # (raises when the library is missing: no silent torch fallback for CUDA tensors)
            d8 = None
            if dones is not None:
                d8 = _as_u8(dones.to(x.device))
                d8 = d8 if d8.is_contiguous() else d8.contiguous()
            with torch.cuda.device(x.device):
                rc = lib.grx_obs_history_push(self.num_envs, self.dim, self.length, x.data_ptr(), d8.data_ptr() if d8 is not None else None,
                                              int(dones is None), src.data_ptr(), dst.data_ptr(),
                                              C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream))
            if rc:
                raise RuntimeError(f"grx_obs_history_push failed ({rc}): {self.num_envs} x {self.length} x {self.dim}")
        else:
            with torch.no_grad():
                dst.copy_(stack_torch(x.to(dst.dtype), dones, src, self.length))
        self._slot ^= 1
        return dst

    # ---- the surface ---------------------------------------------------------------------------------------------------------------
    def fill(self, x):
        """every row = x[n] repeated `length` times; returns the buffer just written"""
        out = self._write(x, None)
        self.primed = True
        return out

    def push(self, x, dones):
        """shift by one frame and append x; rows whose `dones` is set are refilled with x; returns the buffer just written (the buffer
        the previous call returned is left as it is)"""
        if not self.primed:
            return self.fill(x)
        return self._write(x, dones)

    def state_dict(self):
        return {"rows": self.current.detach().clone(), "primed": self.primed}

    def load_state_dict(self, state):
        rows = state["rows"]
        if tuple(rows.shape) != tuple(self.current.shape):
            raise ValueError(f"ObsHistory: saved rows {tuple(rows.shape)} do not fit {tuple(self.current.shape)} "
                             f"(num_envs {self.num_envs}, length {self.length}, width {self.dim})")
        with torch.no_grad():
            self.current.copy_(rows)
        self.primed = bool(state["primed"])


class HistoryPolicy(nn.Module):
    """policy(stacked rows) of RAW SINGLE frames: what inference and the exported TorchScript module use.  `policy`: the actor, or a
    NormalizedPolicy around it (history first, then normalisation).  forward(x [B, D]) pushes, then acts; the first call, a call after
    reset_memory() and a call with another batch size fill.  reset(dones) marks rows that the next call refills (play.py: after every
    env.step)."""

    def __init__(self, policy, dim, length):
        super().__init__()
        if int(dim) < 1 or int(length) < 1:
            raise ValueError(f"HistoryPolicy: dim and length must be >= 1, got {dim}, {length}")
        self.policy = policy
        self.dim, self.length = int(dim), int(length)
        self.primed = False
        self.register_buffer("rows", torch.zeros(0, self.length * self.dim))
        self.register_buffer("spare", torch.zeros(0, self.length * self.dim))     # the HIP push's other buffer
        self.register_buffer("pending", torch.zeros(0, dtype=torch.uint8))         # rows to refill at the next call

    @torch.jit.unused
    def _push_hip(self, x: torch.Tensor, fill: bool) -> torch.Tensor:
        from .fused_loss import load_ppo_library
        lib = load_ppo_library()
        if self.spare.shape != self.rows.shape or self.spare.device != x.device:
            self.spare = torch.empty_like(self.rows)
        with torch.cuda.device(x.device):
            rc = lib.grx_obs_history_push(x.shape[0], self.dim, self.length, x.data_ptr(), self.pending.data_ptr(), int(fill), self.rows.data_ptr(),
                                          self.spare.data_ptr(), C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream))
        if rc:
            raise RuntimeError(f"grx_obs_history_push failed ({rc}): {x.shape[0]} x {self.length} x {self.dim}")
        return self.spare

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        fill = (not self.primed) or self.rows.shape[0] != x.shape[0] or self.rows.device != x.device
        if fill:
            self.rows = torch.zeros(x.shape[0], self.length * self.dim, dtype=torch.float32, device=x.device)
            self.pending = torch.zeros(x.shape[0], dtype=torch.uint8, device=x.device)
        hip = False
        if not torch.jit.is_scripting():
            hip = x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
        if hip:
            new = self._push_hip(x, fill)
            self.spare = self.rows
        else:
            filled = x.to(torch.float32).repeat(1, self.length)
            if fill:
                new = filled
            else:
                shifted = torch.cat([self.rows[:, self.dim:], x.to(torch.float32)], dim=1)
                new = torch.where((self.pending != 0).view(-1, 1), filled, shifted)
        self.rows = new
        self.pending = torch.zeros_like(self.pending)
        self.primed = True
        return self.policy(new)

    @torch.jit.export
    def reset(self, dones: torch.Tensor):
        """rows whose `dones` is set are refilled by the next call's frame"""
        if self.primed and dones.numel() == self.pending.numel():
            self.pending = self.pending | (dones.reshape(-1) != 0).to(torch.uint8).to(self.pending.device)

    @torch.jit.export
    def reset_memory(self):
        """the next call fills every row"""
        self.primed = False
