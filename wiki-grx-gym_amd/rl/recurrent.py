"""A recurrent actor-critic (legged_gym `ActorCriticRecurrent`, rsl_rl `Memory`): one LSTM layer of hidden size H in
front of the actor's MLP and another in front of the critic's; each MLP reads its memory's h.

    cell, torch.nn.LSTM's formulas and gate order:
        G = x W_ih^T + h' W_hh^T + b_ih + b_hh          G = [i | f | g | o]
        i, f, o = sigmoid(.)   g = tanh(.)              c = f c' + i g      h = o tanh(c)
        (h', c'): the previous state, ZERO for a row whose `reset` byte is set
    rollout:  reset at step t = dones of step t - 1: `reset(dones)` only records the bytes, the next cell launch applies them
    update:   a minibatch is a contiguous range of envs over all T steps; the forward runs t = 0 .. T-1 from the state each memory had
              before the rollout's first step (zero where the rollout before ended an episode), reset_t = dones[t - 1] for t >= 1.
              That is rsl_rl's padded-trajectory forward -- every trajectory starts from the stored state, which is zero after a done --
              without the split and the padding; back-propagation through time stops at a done because the state is multiplied by
              zero there.

Contiguous fp32 tensors on a HIP device go through libgrx_ppo.so (include/grx_ppo.h grx_lstm_cell / grx_lstm_cell_backward: one launch
each); `lstm_cell_torch` / `lstm_cell_backward_torch` spell the same two operations in torch for the CPU, and GRX_LSTM_FUSED=0 forces
them on the device too.  The parameters live in a real nn.LSTM(D, H, 1) named `rnn`, so initialisation and the state-dict keys
(`memory_a.rnn.weight_ih_l0` ...) are rsl_rl's.

LSTMSequenceBPTT is the sequence for the recurrent distillation student's truncated BPTT: the same forward, the last
state returned as data for the next window, and a backward whose per-step chain is one launch (include/grx_ppo_bptt.h grx_lstm_bptt_step;
GRX_LSTM_BPTT_FUSED=0: LSTMSequence's three-launch spelling).  PPO's update keeps LSTMSequence."""
import copy
import ctypes as C
import os

import torch
import torch.nn as nn

from .modules import MLP, ActorCriticMLP, _TrainLinear, _TrainLinearELU
from .storage import RolloutStorage


def _fused_enabled():
    return os.environ.get("GRX_LSTM_FUSED", "1") != "0"


def _as_u8(t):
    """one byte per row, as fused_loss.store_transition takes it: bool is reinterpreted, any other dtype converted"""
    if t.dtype == torch.bool:
        return t.view(torch.uint8)
    return t if t.dtype == torch.uint8 else (t != 0).to(torch.uint8)


def _stream(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


# ---- the two operations in torch ---------------------------------------------------------------------------------------------------------
def lstm_cell_torch(x, h_prev, c_prev, reset, w_ih, w_hh, b_ih, b_hh):
    """(h, c, acts [M, 5H]) of one step -- the definition grx_lstm_cell implements"""
    if reset is not None:
        rs = (reset != 0).view(-1, 1)
        h_prev, c_prev = torch.where(rs, torch.zeros_like(h_prev), h_prev), torch.where(rs, torch.zeros_like(c_prev), c_prev)
    G = x @ w_ih.t() + h_prev @ w_hh.t() + b_ih + b_hh
    gi, gf, gg, go = G.chunk(4, dim=1)
    i, f, g, o = torch.sigmoid(gi), torch.sigmoid(gf), torch.tanh(gg), torch.sigmoid(go)
    c = f * c_prev + i * g
    tc = torch.tanh(c)
    return o * tc, c, torch.cat([i, f, g, o, tc], dim=1)


def lstm_cell_backward_torch(dh, dc_in, acts, c_prev, reset):
    """(dG [M, 4H], dc_prev [M, H]) -- the definition grx_lstm_cell_backward implements"""
    i, f, g, o, tc = acts.chunk(5, dim=1)
    rs = (reset != 0).view(-1, 1) if reset is not None else None
    if rs is not None:
        c_prev = torch.where(rs, torch.zeros_like(c_prev), c_prev)
    d_o = dh * tc
    d_c = dh * o * (1.0 - tc * tc)
    if dc_in is not None:
        d_c = dc_in + d_c
    dG = torch.cat([d_c * g * (i * (1.0 - i)), d_c * c_prev * (f * (1.0 - f)), d_c * i * (1.0 - g * g), d_o * (o * (1.0 - o))], dim=1)
    dc_prev = d_c * f
    if rs is not None:
        dc_prev = torch.where(rs, torch.zeros_like(dc_prev), dc_prev)
    return dG, dc_prev


# ---- ... and through libgrx_ppo.so -------------------------------------------------------------------------------------------------------
def _lib():
    from .fused_loss import load_ppo_library
    lib = load_ppo_library()   # (raises when the library is missing: no silent torch fallback for CUDA tensors)
    if not getattr(lib, "_lstm_ready", False):
        fp = C.c_void_p
        lib.grx_lstm_cell.restype = C.c_int
        lib.grx_lstm_cell.argtypes = [C.c_int] * 3 + [fp] * 11 + [C.c_void_p]
        lib.grx_lstm_cell_preact.restype = C.c_int
        lib.grx_lstm_cell_preact.argtypes = [C.c_int] * 3 + [fp] * 8 + [C.c_void_p]
        lib.grx_lstm_cell_backward.restype = C.c_int
        lib.grx_lstm_cell_backward.argtypes = [C.c_int] * 2 + [fp] * 7 + [C.c_void_p]
        lib.grx_lstm_bptt_step.restype = C.c_int
        lib.grx_lstm_bptt_step.argtypes = [C.c_int] * 2 + [fp] * 10 + [C.c_void_p]
        lib.grx_lstm_bptt_step_tile.restype = C.c_int
        lib.grx_lstm_bptt_step_tile.argtypes = [C.c_int] * 3 + [fp] * 10 + [C.c_void_p]
        lib.grx_lstm_bptt_dh.restype = C.c_int
        lib.grx_lstm_bptt_dh.argtypes = [C.c_int] * 2 + [fp] * 5 + [C.c_void_p]
        lib._lstm_ready = True
    return lib


def _ptr(t):
    return t.data_ptr() if t is not None else None


def lstm_cell_hip(x, h_prev, c_prev, reset, w_ih, w_hh, b_ih, b_hh, h, c, acts=None):
    """grx_lstm_cell into h, c (and acts): one launch.  Every tensor contiguous fp32 on one HIP device, reset uint8 or None"""
    M, D = x.shape
    H = w_hh.shape[1]
    with torch.cuda.device(x.device):
        rc = _lib().grx_lstm_cell(M, D, H, x.data_ptr(), h_prev.data_ptr(), c_prev.data_ptr(), _ptr(reset), w_ih.data_ptr(), w_hh.data_ptr(),
                                  b_ih.data_ptr(), b_hh.data_ptr(), h.data_ptr(), c.data_ptr(), _ptr(acts), _stream(x))
    if rc:
        raise RuntimeError(f"grx_lstm_cell failed ({rc}): M {M}, D {D}, H {H}")


def lstm_preact_hip(x, h_prev, reset, w_ih, w_hh, b_ih, b_hh):
    """grx_lstm_cell_preact: the pre-activations G [M, 4H] as the cell's reduction forms them (tests)"""
    M, D = x.shape
    H = w_hh.shape[1]
    G = torch.empty(M, 4 * H, device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        rc = _lib().grx_lstm_cell_preact(M, D, H, x.data_ptr(), h_prev.data_ptr(), _ptr(reset), w_ih.data_ptr(), w_hh.data_ptr(), b_ih.data_ptr(),
                                         b_hh.data_ptr(), G.data_ptr(), _stream(x))
    if rc:
        raise RuntimeError(f"grx_lstm_cell_preact failed ({rc}): M {M}, D {D}, H {H}")
    return G


def lstm_cell_backward_hip(dh, dc_in, acts, c_prev, reset, dG, dc_prev):
    M, H = dh.shape
    with torch.cuda.device(dh.device):
        rc = _lib().grx_lstm_cell_backward(M, H, dh.data_ptr(), _ptr(dc_in), acts.data_ptr(), c_prev.data_ptr(), _ptr(reset), dG.data_ptr(),
                                           dc_prev.data_ptr(), _stream(dh))
    if rc:
        raise RuntimeError(f"grx_lstm_cell_backward failed ({rc}): M {M}, H {H}")


def lstm_bptt_step_hip(dG_next, w_hh, reset_next, dh_out, dc_in, acts, c_prev, reset, dG, dc_prev, tile_units=None):
    """grx_lstm_bptt_step into dG, dc_prev: one launch for dh = dh_out + dG_next W_hh (zero where reset_next is set) and the cell's
    element-wise backward on it.  tile_units: the measurement hook grx_lstm_bptt_step_tile (tools/bptt_time.py)"""
    M, H = dh_out.shape
    lib = _lib()
    args = (M, H, _ptr(dG_next), w_hh.data_ptr(), _ptr(reset_next), dh_out.data_ptr(), _ptr(dc_in), acts.data_ptr(), c_prev.data_ptr(), _ptr(reset),
            dG.data_ptr(), dc_prev.data_ptr(), _stream(dh_out))
    with torch.cuda.device(dh_out.device):
        rc = lib.grx_lstm_bptt_step(*args) if tile_units is None else lib.grx_lstm_bptt_step_tile(int(tile_units), *args)
    if rc:
        raise RuntimeError(f"grx_lstm_bptt_step failed ({rc}): M {M}, H {H}")


def lstm_bptt_dh_hip(dG_next, w_hh, reset_next, dh_out):
    """grx_lstm_bptt_dh: dh [M, H] = dh_out + dG_next W_hh as grx_lstm_bptt_step's reduction forms it (tests)"""
    M, H = dh_out.shape
    dh = torch.empty_like(dh_out)
    with torch.cuda.device(dh_out.device):
        rc = _lib().grx_lstm_bptt_dh(M, H, _ptr(dG_next), w_hh.data_ptr(), _ptr(reset_next), dh_out.data_ptr(), dh.data_ptr(), _stream(dh_out))
    if rc:
        raise RuntimeError(f"grx_lstm_bptt_dh failed ({rc}): M {M}, H {H}")
    return dh


def _bptt_fused_enabled():
    return os.environ.get("GRX_LSTM_BPTT_FUSED", "1") != "0"


def _use_hip(x):
    """the HIP entry points serve every tensor on a HIP device (made contiguous fp32 where it is not) unless GRX_LSTM_FUSED=0"""
    return x.is_cuda and _fused_enabled()


def _f32c(t):
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.contiguous().float()


# ---- a whole sequence, with its backward ---------------------------------------------------------------------------------------------------
class LSTMSequence(torch.autograd.Function):
    """(x [T, n, D], resets [T, n] uint8, h0, c0 [n, H], W_ih, W_hh, b_ih, b_hh) -> h [T, n, H]: step t starts from step t - 1's state, or
    from zero in the rows where resets[t] is set; step 0 from (h0, c0).  h0 and c0 are data: they get no gradient.

    Forward: T cell launches that keep their activations.  Backward: for t reversed, the element-wise half (grx_lstm_cell_backward), then
    dh_{t-1} += (dG_t W_hh) where step t was not reset -- a torch matmul under the update's BLAS preference, as _TrainLinear's --; after the
    loop ONE product each for dX = dG W_ih, dW_ih = dG^T X and dW_hh = dG^T H', and the deterministic column sum of dG for both biases."""

    @staticmethod
    def forward(ctx, x, resets, h0, c0, w_ih, w_hh, b_ih, b_hh):
        T, n, _ = x.shape
        H = w_hh.shape[1]
        hip = _use_hip(x)
        if hip:
            x, h0, c0, w_ih, w_hh, b_ih, b_hh = (_f32c(t) for t in (x, h0, c0, w_ih, w_hh, b_ih, b_hh))
            resets = resets.contiguous()
        hs = x.new_empty(T + 1, n, H)      # hs[t]: the state step t starts from; hs[t + 1]: what it leaves
        cs = x.new_empty(T + 1, n, H)
        acts = x.new_empty(T, n, 5 * H)
        hs[0].copy_(h0); cs[0].copy_(c0)
        for t in range(T):
            if hip:
                lstm_cell_hip(x[t], hs[t], cs[t], resets[t], w_ih, w_hh, b_ih, b_hh, hs[t + 1], cs[t + 1], acts[t])
            else:
                h, c, a = lstm_cell_torch(x[t], hs[t], cs[t], resets[t], w_ih, w_hh, b_ih, b_hh)
                hs[t + 1].copy_(h); cs[t + 1].copy_(c); acts[t].copy_(a)
        ctx.hip = hip
        ctx.save_for_backward(x, resets, hs, cs, acts, w_ih, w_hh)
        return hs[1:]

    @staticmethod
    def backward(ctx, dh_all):
        x, resets, hs, cs, acts, w_ih, w_hh = ctx.saved_tensors
        T, n, D = x.shape
        H = w_hh.shape[1]
        hip = ctx.hip
        dh_all = _f32c(dh_all) if hip else dh_all
        keep = (resets == 0).to(x.dtype).unsqueeze(-1)           # [T, n, 1]
        dG = x.new_empty(T, n, 4 * H)
        dcs = (x.new_empty(n, H), x.new_empty(n, H))             # the two buffers dc alternates between
        dh, dc = dh_all[T - 1], None
        for t in reversed(range(T)):
            if hip:
                nxt = dcs[t & 1]
                lstm_cell_backward_hip(dh, dc, acts[t], cs[t], resets[t], dG[t], nxt)
                dc = nxt
            else:
                g, dc = lstm_cell_backward_torch(dh, dc, acts[t], cs[t], resets[t])
                dG[t].copy_(g)
            if t > 0:
                dh = torch.addcmul(dh_all[t - 1], dG[t] @ w_hh, keep[t])
        dG2 = dG.view(T * n, 4 * H)
        dx = (dG2 @ w_ih).view(T, n, D) if ctx.needs_input_grad[0] else None   # (the observations are data: no dX product in training)
        dw_ih = dG2.t() @ x.reshape(T * n, D)
        dw_hh = dG2.t() @ (hs[:-1] * keep).view(T * n, H)       # (the h' a reset row multiplied W_hh with is zero)
        if hip:
            from .fused_loss import colsum
            db = colsum(dG2)
        else:
            db = dG2.sum(0)
        return dx, None, None, None, dw_ih, dw_hh, db, db.clone()


class LSTMSequenceBPTT(torch.autograd.Function):
    """LSTMSequence for truncated back-propagation through time (the recurrent distillation student): the same forward,
    which also returns the last step's (h, c) -- data for the next window, marked non-differentiable --, and a backward whose per-step chain
    dh_t = dh_out_t + (dG_{t+1} W_hh where step t + 1 was not reset), then the cell's element-wise backward, is ONE launch
    (grx_lstm_bptt_step) instead of a product, an addcmul and grx_lstm_cell_backward.  GRX_LSTM_BPTT_FUSED=0, GRX_LSTM_FUSED=0 and CPU
    tensors take LSTMSequence's three-launch spelling, which is the definition.  The products after the loop are LSTMSequence's."""

    @staticmethod
    def forward(ctx, x, resets, h0, c0, w_ih, w_hh, b_ih, b_hh):
        T, n, _ = x.shape
        H = w_hh.shape[1]
        hip = _use_hip(x)
        if hip:
            x, h0, c0, w_ih, w_hh, b_ih, b_hh = (_f32c(t) for t in (x, h0, c0, w_ih, w_hh, b_ih, b_hh))
            resets = resets.contiguous()
        hs = x.new_empty(T + 1, n, H)      # hs[t]: the state step t starts from; hs[t + 1]: what it leaves
        cs = x.new_empty(T + 1, n, H)
        acts = x.new_empty(T, n, 5 * H)
        hs[0].copy_(h0); cs[0].copy_(c0)
        for t in range(T):
            if hip:
                lstm_cell_hip(x[t], hs[t], cs[t], resets[t], w_ih, w_hh, b_ih, b_hh, hs[t + 1], cs[t + 1], acts[t])
            else:
                h, c, a = lstm_cell_torch(x[t], hs[t], cs[t], resets[t], w_ih, w_hh, b_ih, b_hh)
                hs[t + 1].copy_(h); cs[t + 1].copy_(c); acts[t].copy_(a)
        ctx.hip, ctx.fused = hip, hip and _bptt_fused_enabled()
        ctx.save_for_backward(x, resets, hs, cs, acts, w_ih, w_hh)
        h_last, c_last = hs[T].clone(), cs[T].clone()
        ctx.mark_non_differentiable(h_last, c_last)
        return hs[1:], h_last, c_last

    @staticmethod
    def backward(ctx, dh_all, _dh_last, _dc_last):
        if not ctx.fused:
            return LSTMSequence.backward(ctx, dh_all)
        x, resets, hs, cs, acts, w_ih, w_hh = ctx.saved_tensors
        T, n, D = x.shape
        H = w_hh.shape[1]
        dh_all = _f32c(dh_all)
        dG = x.new_empty(T, n, 4 * H)
        dcs = (x.new_empty(n, H), x.new_empty(n, H))             # the two buffers dc alternates between
        dc = None
        for t in reversed(range(T)):
            nxt, last = dcs[t & 1], t == T - 1
            lstm_bptt_step_hip(None if last else dG[t + 1], w_hh, None if last else resets[t + 1], dh_all[t], dc, acts[t], cs[t], resets[t], dG[t], nxt)
            dc = nxt
        keep = (resets == 0).to(x.dtype).unsqueeze(-1)           # [T, n, 1]
        dG2 = dG.view(T * n, 4 * H)
        dx = (dG2 @ w_ih).view(T, n, D) if ctx.needs_input_grad[0] else None
        dw_ih = dG2.t() @ x.reshape(T * n, D)
        dw_hh = dG2.t() @ (hs[:-1] * keep).view(T * n, H)       # (the h' a reset row multiplied W_hh with is zero)
        from .fused_loss import colsum
        db = colsum(dG2)
        return dx, None, None, None, dw_ih, dw_hh, db, db.clone()


# ---- the modules -----------------------------------------------------------------------------------------------------------------------
def check_rnn(rnn_type, num_layers, hidden_size):
    """the constructor refusals: one LSTM layer, its hidden size what grx_lstm_cell takes; returns the hidden size"""
    if str(rnn_type).lower() != "lstm":
        raise ValueError(f"rnn_type must be 'lstm', not {rnn_type!r} (GRU is not implemented)")
    if num_layers != 1:
        raise ValueError(f"rnn_num_layers must be 1, not {num_layers!r} (stacked layers are not implemented)")
    if not isinstance(hidden_size, int) or isinstance(hidden_size, bool) or hidden_size < 32 or hidden_size > 1024 or hidden_size % 32:
        raise ValueError(f"rnn_hidden_size must be a multiple of 32 in 32..1024, not {hidden_size!r}")
    return hidden_size


class Memory(nn.Module):
    """rsl_rl's Memory: `rnn` = nn.LSTM(input_size, hidden_size, 1) holds the parameters; the state (h, c) of the last `step` is kept
    here, out of the state dict.  `rnn` given: another memory's LSTM, shared -- an inference policy with a state of its own."""

    def __init__(self, input_size, hidden_size=256, num_layers=1, type="lstm", rnn=None):
        super().__init__()
        H = check_rnn(type, num_layers, hidden_size)
        self.input_size, self.hidden_size = int(input_size), H
        self.rnn = rnn if rnn is not None else nn.LSTM(self.input_size, H, 1)
        self._state, self._slot, self._reset = None, 0, None

    def _weights(self):
        r = self.rnn
        return r.weight_ih_l0, r.weight_hh_l0, r.bias_ih_l0, r.bias_hh_l0

    # ---- step mode ---------------------------------------------------------------------------------------------------------------
    def _ensure_state(self, n, device):
        st = self._state
        if st is None or st[0].shape[1] != n or st[0].device != torch.device(device):
            with torch.inference_mode(False):   # (the rollout runs under inference_mode; these are written there at every step)
                self._state = (torch.zeros(2, n, self.hidden_size, device=device), torch.zeros(2, n, self.hidden_size, device=device))
            self._slot, self._reset = 0, None
        return self._state

    def _cell(self, x, h_prev, c_prev, reset, h, c):
        w = [p.detach() for p in self._weights()]
        if _use_hip(x):
            lstm_cell_hip(_f32c(x), h_prev, c_prev, reset, *w, h, c)
        else:
            with torch.no_grad():
                hn, cn, _ = lstm_cell_torch(x.to(h.dtype), h_prev, c_prev, reset, *w)
                h.copy_(hn); c.copy_(cn)

    def step(self, x):
        """advance by one frame x [n, D]: returns h [n, H] (valid until the step after the next: the two state buffers alternate)"""
        hs, cs = self._ensure_state(x.shape[0], x.device)
        src, dst = self._slot, self._slot ^ 1
        self._cell(x, hs[src], cs[src], self._reset, hs[dst], cs[dst])
        self._slot, self._reset = dst, None
        return hs[dst]

    def peek(self, x):
        """what step(x) would return, computed into scratch: the state and the pending reset are left as they are"""
        hs, cs = self._ensure_state(x.shape[0], x.device)
        h, c = torch.empty_like(hs[0]), torch.empty_like(cs[0])
        self._cell(x, hs[self._slot], cs[self._slot], self._reset, h, c)
        return h

    def reset(self, dones=None):
        """dones [n]: rows whose state the NEXT step takes as zero.  Only recorded here, by reference where the dtype allows: the bytes
        are read when that step runs (the env's next step, which rewrites them, comes after it).  None: every row, now"""
        if dones is None:
            self._state = None
            return
        d = _as_u8(dones.reshape(-1))
        if self._state is not None and d.device != self._state[0].device:
            d = d.to(self._state[0].device)
        self._reset = d if d.is_contiguous() else d.contiguous()

    def hidden_states(self):
        """(h, c) as the last step left them (None before the first); a pending reset is not applied"""
        if self._state is None:
            return None
        return self._state[0][self._slot], self._state[1][self._slot]

    def start_state(self, n, device):
        """(h, c) the next step starts from, as new tensors: the pending reset applied"""
        hs, cs = self._ensure_state(n, device)
        h, c = hs[self._slot].clone(), cs[self._slot].clone()
        if self._reset is not None:
            rs = (self._reset != 0).view(-1, 1)
            h.masked_fill_(rs, 0.0); c.masked_fill_(rs, 0.0)
        return h, c

    # ---- sequence mode -----------------------------------------------------------------------------------------------------------
    def sequence(self, x, resets, h0, c0):
        """x [T, n, D], resets [T, n] uint8 (row t: the rows step t takes from zero), (h0, c0) [n, H] -> h [T, n, H], differentiable in
        the LSTM's parameters (and x)"""
        return LSTMSequence.apply(x, resets, h0, c0, *self._weights())

    def sequence_bptt(self, x, resets, h0, c0):
        """`sequence` for one window of truncated back-propagation through time: (h [T, n, H], h_last, c_last [n, H]); the last state is
        data for the next window (no gradient), the backward's per-step chain is one launch (LSTMSequenceBPTT)"""
        return LSTMSequenceBPTT.apply(x, resets, h0, c0, *self._weights())


class _TrainLinearOut(torch.autograd.Function):
    """An MLP's output layer in the update, y = x W^T + b through grx_mlp_layer -- the kernel the rollout's policy step runs, so that the
    update's forward reproduces the rollout's outputs bit for bit; the backward is _TrainLinear's."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        from .fused_loss import _layer, load_ppo_library
        with torch.cuda.device(x.device):
            y = _layer(load_ppo_library(), x, weight, bias, False, torch.cuda.current_stream(x.device).cuda_stream)
        ctx.save_for_backward(x, weight)
        return y

    backward = _TrainLinear.backward


class _MemoryMLP(MLP):
    """The MLP behind a memory.  On a HIP device, with Linear -> ELU(1) hidden layers, every forward -- the rollout's (no gradient) and the
    update's -- runs its layers through libgrx_ppo.so's grx_mlp_layer, so that both give the same bits for the same rows."""

    @torch.jit.unused
    def _forward_hip(self, x):
        from .fused_loss import _linears_of, mlp_forward
        lin = _linears_of(self)
        if not torch.is_grad_enabled():
            return mlp_forward(self, x)
        for w, b in lin[:-1]:
            x = _TrainLinearELU.apply(x, w, b, False)
        return _TrainLinearOut.apply(x, *lin[-1])

    def fusable(self, x):
        from .fused_loss import mlp_can_fuse
        return _fused_enabled() and self.precision == "fp32" and x.is_contiguous() and mlp_can_fuse(self, x)

    def forward(self, x):
        if not torch.jit.is_scripting():
            if x.is_cuda and x.dim() == 2 and self.fusable(x):
                return self._forward_hip(x)
        return super().forward(x)


class ActorCriticRecurrent(ActorCriticMLP):
    """legged_gym's ActorCriticRecurrent: `memory_a` / `memory_c` in front of `actor` / `critic`, whose input width is the hidden size.
    act / evaluate / act_inference advance their memory by one step; `features` runs whole sequences for the update; inside
    `on_features()` the three take memory outputs instead of observations (PPO._losses then serves both policies unchanged)."""
    is_recurrent = True

    def __init__(self, actor_num_input, critic_num_input, actor_num_output, rnn_type="lstm", rnn_hidden_size=256, rnn_num_layers=1, **kwargs):
        for k in ("actor_num_input", "critic_num_input"):
            kwargs.pop(k, None)
        H = check_rnn(rnn_type, rnn_num_layers, rnn_hidden_size)   # (the refusals, before anything is built)
        super().__init__(H, H, actor_num_output, **kwargs)
        for name in ("actor", "critic"):   # the same layers and values as _MemoryMLP
            old = getattr(self, name)
            new = _MemoryMLP(old.input_size, old.output_size, old.hidden_dims, kwargs.get("activation", "elu"))
            new.load_state_dict(old.state_dict())
            setattr(self, name, new)
        self.num_actor_input, self.num_critic_input = int(actor_num_input), int(critic_num_input)   # what the storage keeps: observations
        self.rnn_hidden_size = H
        self.memory_a = Memory(actor_num_input, H)
        self.memory_c = Memory(critic_num_input, H)
        self._on_features = False

    def set_precision(self, precision):
        if precision != "fp32":
            raise ValueError(f"ActorCriticRecurrent: precision={precision!r} is not available, the recurrent policy runs in fp32")

    def reset(self, dones=None):
        self.memory_a.reset(dones)
        self.memory_c.reset(dones)

    def get_hidden_states(self):
        return self.memory_a.hidden_states(), self.memory_c.hidden_states()

    class _Features:
        def __init__(self, ac):
            self.ac = ac

        def __enter__(self):
            self.ac._on_features = True

        def __exit__(self, *exc):
            self.ac._on_features = False

    def on_features(self):
        return ActorCriticRecurrent._Features(self)

    def update_distribution(self, observations):
        super().update_distribution(observations if self._on_features else self.memory_a.step(observations))

    def act_inference(self, observations):
        return self.actor(observations if self._on_features else self.memory_a.step(observations))

    def evaluate(self, critic_observations=None, **_):
        return self.critic(critic_observations if self._on_features else self.memory_c.step(critic_observations))

    def evaluate_bootstrap(self, critic_observations):
        """the value of the observations the rollout ended on, from the critic's memory as it is and into scratch: the memory does not
        advance (rsl_rl's compute_returns calls evaluate(), whose memory then sees these observations twice)"""
        return self.critic(self.memory_c.peek(critic_observations))

    def rollout_step(self, obs, critic_obs):
        """(actions, values, log-prob, mean, sigma) of one rollout step; both memories advance.  On a HIP device: the two cells, then the
        MLPs through libgrx_ppo.so's inference forward, the actor's output layer fused with the sampling and the log-probability"""
        fa, fc = self.memory_a.step(obs), self.memory_c.step(critic_obs)
        if fa.is_cuda and self.num_actor_output <= 32 and self.actor.fusable(fa) and self.critic.fusable(fc):
            from .fused_loss import mlp_forward, policy_act
            eps = torch.randn(fa.shape[0], self.num_actor_output, device=fa.device)
            std = self.noise_std().detach()
            actions, logp, mu, sigma = policy_act(self.actor, std, fa, eps)
            return actions, mlp_forward(self.critic, fc), logp, mu, sigma
        with self.on_features():
            actions = self.act(fa).detach()
            values = self.evaluate(fc).detach()
        return actions, values, self.get_actions_log_prob(actions).detach(), self.action_mean.detach(), self.action_std.detach()

    def features(self, obs, critic_obs, resets, start):
        """the update's forward through both memories: obs [T, n, D], critic_obs [T, n, Dc], resets [T, n] uint8, start = (h0_a, c0_a,
        h0_c, c0_c) -> the memories' outputs, flattened step-major to [T n, H] each"""
        fa = self.memory_a.sequence(obs, resets, start[0], start[1])
        fc = self.memory_c.sequence(critic_obs, resets, start[2], start[3])
        return fa.flatten(0, 1), fc.flatten(0, 1)


def _normal(t):
    """t, or a copy when t is an inference tensor (compute_returns rebinds the advantages under the runner's inference_mode, and a whole-range
    slice of them is a view): autograd cannot save those"""
    return t.clone() if t.is_inference() else t


# ---- the storage -----------------------------------------------------------------------------------------------------------------------
class RecurrentRolloutStorage(RolloutStorage):
    """RolloutStorage plus what a recurrent update needs: the state both memories had before the rollout's first step, [N, H] each, and
    rsl_rl's `recurrent_mini_batch_generator` order -- contiguous env ranges over all T steps, in order, no permutation, tail dropped."""

    def __init__(self, num_envs, num_transitions_per_env, actor_obs_shape, critic_obs_shape, actions_shape, hidden_size, device, **kwargs):
        super().__init__(num_envs, num_transitions_per_env, actor_obs_shape, critic_obs_shape, actions_shape, device, **kwargs)
        z = lambda: torch.zeros(num_envs, hidden_size, device=device)
        self.h0_a, self.c0_a, self.h0_c, self.c0_c = z(), z(), z(), z()

    def set_start_states(self, actor_state, critic_state):
        for dst, src in zip((self.h0_a, self.c0_a, self.h0_c, self.c0_c), (*actor_state, *critic_state)):
            dst.copy_(src)

    def env_ranges(self, num_mini_batches):
        n = self.num_envs // num_mini_batches
        if n < 1:
            raise ValueError(f"a recurrent minibatch is a range of envs: num_mini_batches={num_mini_batches} exceeds num_envs={self.num_envs}")
        return [(i * n, (i + 1) * n) for i in range(num_mini_batches)]

    def recurrent_mini_batch_generator(self, num_mini_batches, num_epochs=8):
        """per minibatch: (obs [T, n, D], critic_obs [T, n, Dc], resets [T, n] uint8, (h0_a, c0_a, h0_c, c0_c) [n, H], then actions,
        values, advantages, returns, log-probs, mu, sigma flattened step-major to [T n, .])"""
        cobs_all = self.pri_observations if self.pri_observations is not None else self.observations
        cols = (self.actions, self.values, self.advantages, self.returns, self.actions_log_prob, self.mu, self.sigma)
        for _ in range(num_epochs):
            for a, b in self.env_ranges(num_mini_batches):
                resets = torch.zeros(self.num_transitions_per_env, b - a, dtype=torch.uint8, device=self.dones.device)
                resets[1:] = self.dones[:-1, a:b, 0]                      # step t starts from zero where step t - 1 ended an episode
                start = tuple(s[a:b].contiguous() for s in (self.h0_a, self.c0_a, self.h0_c, self.c0_c))
                yield (self.observations[:, a:b].contiguous(), cobs_all[:, a:b].contiguous(), resets, start,
                       *[_normal(c[:, a:b].flatten(0, 1)) for c in cols])


# ---- inference and export ----------------------------------------------------------------------------------------------------------------
class RecurrentPolicy(nn.Module):
    """The inference policy of a recurrent actor: raw frames in (normalised first when `normalizer` is given), a memory state of its
    own -- the training memories are left alone --, `reset(dones)` / `reset_memory()` as rl.history.HistoryPolicy has them."""

    def __init__(self, actor_critic, normalizer=None):
        super().__init__()
        self.memory = Memory(actor_critic.memory_a.input_size, actor_critic.rnn_hidden_size, rnn=actor_critic.memory_a.rnn)
        self.actor, self.normalizer = actor_critic.actor, normalizer

    def forward(self, x):
        if self.normalizer is not None:
            x = self.normalizer(x)
        return self.actor(self.memory.step(x))

    def reset(self, dones):
        self.memory.reset(dones)

    def reset_memory(self):
        self.memory.reset(None)


class ExportedRecurrentPolicy(nn.Module):
    """What export_policy_as_jit scripts for a recurrent actor -- plain torch, loads without libgrx_ppo.so: an nn.LSTM with `hidden_state` /
    `cell_state` buffers (legged_gym's PolicyExporterLSTM), the actor's layers, the normaliser folded in front when there is one.  One
    raw frame [B, D] per call; `reset(dones)` zeroes the state of the rows that ended, `reset_memory()` of all."""

    def __init__(self, actor_critic, normalizer=None):
        super().__init__()
        self.rnn = copy.deepcopy(actor_critic.memory_a.rnn).to("cpu")
        self.actor = copy.deepcopy(actor_critic.actor.model).to("cpu")
        self.normalize = normalizer is not None
        D = self.rnn.input_size
        self.register_buffer("mean", normalizer._mean.detach().clone().to("cpu") if self.normalize else torch.zeros(1, D))
        self.register_buffer("scale", (normalizer._std + normalizer.eps).detach().clone().to("cpu") if self.normalize else torch.ones(1, D))
        self.register_buffer("hidden_state", torch.zeros(1, 1, self.rnn.hidden_size))
        self.register_buffer("cell_state", torch.zeros(1, 1, self.rnn.hidden_size))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.hidden_state.shape[1] != x.shape[0]:
            self.hidden_state = torch.zeros(1, x.shape[0], self.hidden_state.shape[2], dtype=self.hidden_state.dtype, device=x.device)
            self.cell_state = torch.zeros_like(self.hidden_state)
        if self.normalize:   # (rl.normalizer.NormalizedPolicy's arithmetic, frozen statistics)
            x = (x - self.mean) / self.scale
        out, (h, c) = self.rnn(x.unsqueeze(0), (self.hidden_state, self.cell_state))
        self.hidden_state = h
        self.cell_state = c
        return self.actor(out.squeeze(0))

    @torch.jit.export
    def reset(self, dones: torch.Tensor):
        if dones.numel() == self.hidden_state.shape[1]:
            keep = (dones.reshape(1, -1, 1) == 0).to(self.hidden_state.dtype).to(self.hidden_state.device)
            self.hidden_state = self.hidden_state * keep
            self.cell_state = self.cell_state * keep

    @torch.jit.export
    def reset_memory(self):
        self.hidden_state = torch.zeros_like(self.hidden_state)
        self.cell_state = torch.zeros_like(self.cell_state)
