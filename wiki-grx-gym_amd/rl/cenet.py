"""A context-aided estimator network (CENet: Nahrendra, Yu & Myung, "DreamWaQ: Learning Robust Quadrupedal Locomotion With Implicit
Terrain Imagination via Deep Reinforcement Learning", ICRA 2023; the estimator of HIMLoco and DWL is built around the same idea; DESIGN.md
4.21): an encoder over the actor's input that regresses the unobserved privileged columns, as rl/estimator.py does, AND emits a stochastic
latent z that a decoder must predict the next frame from, with a KL term that keeps z small.  [v_hat | z] is appended to the actor's input.

    pipeline:  raw frame -> observation history -> empirical normalisation -> x [N, D] -> [x | v_hat | z] [N, D + E + Z] -> actor, storage, update
    enc(x)   = [v_hat (E) | mu (Z) | raw (Z)]         enc = MLP(D, E + 2Z, cenet_encoder_dims, "elu")
    lv       = clamp(raw, -10, 2)                     torch.clamp's gradient: zero where the clamp saturates
    sigma    = exp(lv / 2),  z = fma(sigma, eps, mu)  eps ~ N(0, 1)
    dec([v_hat | z]) -> the newest frame of the successor row's x      dec = MLP(E + Z, F, cenet_decoder_dims, "elu"), F one actor frame
    step(x, pri, slot):
        eps is drawn once into a static [N, Z] buffer;  out[n] = [x[n] | v_hat | z];  targets[slot][n] = pri[n][target columns]
    update(rows, dones, num_mini_batches), after PPO's update, on the rollout just collected:
        ONE randperm, reused by each of the num_epochs passes; per minibatch a fresh eps, and with valid = (t < T - 1) and dones[s] == 0
            L_est = sum_r sum_e (v_hat - v)^2 / (mb E)
            L_rec = sum_{r valid} sum_f (dec - x[s + N][D - F:D])^2 / (F max(n_v, 1))
            L_kl  = sum_r sum_j (mu^2 + exp(lv) - lv - 1) / 2 / mb
            L     = L_est + L_rec + beta L_kl
        backward, Adam at a fixed learning rate, no clipping; a non-finite loss skips the step.  The mask is a select: an invalid row adds
        exactly 0 to L_rec and gets exactly zero gradient, whatever its successor holds.

Targets, their canonical order and columns, and the alignment rule (slot, `carry`, `begin_rollout`) are rl/estimator.py's.  [v_hat | z] is
stored as E + Z more columns of the observation row and is data: PPO's gradient never reaches the encoder, PPO's update is untouched.
Inference and the exported module use z = mu (CENetPolicy).

`head_torch`, `reparam_torch` and `loss_torch` are the definitions of grx_cenet_head, grx_cenet_reparam(_backward) and grx_cenet_loss
(include/grx_ppo_cenet.h) in torch: the CPU path, and what GRX_CENET_FUSED=0 selects on a HIP device.  The encoder's rollout layers go
through grx_mlp_layer whatever GRX_CENET_FUSED says; both networks train on the path rl.modules.MLP takes on a HIP device; the update's
gather is grx_smooth_gather_rows as it is.  The networks are fp32.

None of the defaults (targets lin_vel, latent 16, beta 1.0, encoder 128 64, decoder 64 128, learning rate 1e-3, one epoch) is tuned.
DreamWaQ's AdaBoot and a privileged-state decoder are not implemented."""
import ctypes as C
import os

import torch
import torch.nn as nn
import torch.optim as optim

from .estimator import TARGETS, check_layout, parse_targets, target_columns  # noqa: F401  (re-exported: the targets are the estimator's)
from .modules import MLP

MAX_TARGETS, MAX_LATENT, MAX_INPUT, MAX_FRAME = 8, 64, 2048, 2048   # include/grx_ppo_cenet.h
MAX_LAYERS, MAX_WIDTH = 3, 1024
LV_MIN, LV_MAX = -10.0, 2.0
_LIB = None


def fused_enabled():
    return os.environ.get("GRX_CENET_FUSED", "1") != "0"


def check_dims(dims, flag):
    dims = [int(h) for h in dims]
    if not 1 <= len(dims) <= MAX_LAYERS or any(not 1 <= h <= MAX_WIDTH for h in dims):
        raise ValueError(f"--{flag} takes 1 to {MAX_LAYERS} hidden layers of width 1..{MAX_WIDTH} each, not {dims}")
    return dims


def check_values(latent_dim, beta, learning_rate, num_epochs):
    if not 1 <= int(latent_dim) <= MAX_LATENT:
        raise ValueError(f"--cenet_latent_dim must be in 1..{MAX_LATENT}, not {latent_dim}")
    if not (float(beta) >= 0.0 and float(beta) < float("inf")):
        raise ValueError(f"--cenet_beta must be finite and not negative, not {beta}")
    if int(num_epochs) < 1 or not float(learning_rate) > 0.0:
        raise ValueError(f"--cenet_num_epochs must be >= 1 and --cenet_learning_rate > 0, got {num_epochs} and {learning_rate}")


def load_library():
    """libgrx_ppo.so with the grx_cenet_* entries declared (only a run with --cenet gets here)"""
    global _LIB
    if _LIB is None:
        from .fused_loss import load_ppo_library
        lib = load_ppo_library()
        if not hasattr(lib, "grx_cenet_head"):
            raise RuntimeError("libgrx_ppo.so has no grx_cenet_head: rebuild it (csrc/grx_ppo_cenet.hip); there is no fallback on a HIP device")
        fp, i = C.c_void_p, C.c_int
        lib.grx_cenet_head.restype = i
        lib.grx_cenet_head.argtypes = [i, i, i, i, fp, fp, fp, i, fp, C.POINTER(C.c_int), fp, fp, C.c_void_p]
        lib.grx_cenet_reparam.restype = i
        lib.grx_cenet_reparam.argtypes = [i, i, i, fp, fp, fp, C.c_void_p]
        lib.grx_cenet_reparam_backward.restype = i
        lib.grx_cenet_reparam_backward.argtypes = [i, i, i, fp, fp, fp, fp, C.c_void_p]
        lib.grx_cenet_loss_partials_size.restype = i
        lib.grx_cenet_loss_partials_size.argtypes = [i, i, i, i]
        lib.grx_cenet_loss.restype = i
        lib.grx_cenet_loss.argtypes = [i, i, i, i, fp, fp, fp, fp, i, i, fp, C.c_float, fp, fp, fp, fp, C.c_void_p]
        _LIB = lib
    return _LIB


def _stream(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _ok(*ts):
    return all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in ts)


# ---- the torch spelling: the definition ----------------------------------------------------------------------------------------------------
def reparam_torch(enc_out, eps, E, Z):
    """[v_hat | z] [mb, E + Z] from enc_out [mb, E + 2Z] and eps [mb, Z]"""
    v, mu, raw = enc_out[:, :E], enc_out[:, E:E + Z], enc_out[:, E + Z:E + 2 * Z]
    sigma = torch.exp(0.5 * raw.clamp(LV_MIN, LV_MAX))
    return torch.cat([v, torch.addcmul(mu, sigma, eps)], dim=1)   # (addcmul rounds once on a HIP device, as the kernel's fmaf)


def head_torch(x, enc_out, eps, E, Z, pri=None, cols=None):
    """the definition of grx_cenet_head: ([x | v_hat | z], pri[:, cols] or None)"""
    out = torch.cat([x, reparam_torch(enc_out, eps, E, Z)], dim=1)
    if pri is None:
        return out, None
    idx = cols if torch.is_tensor(cols) else torch.as_tensor(list(cols), dtype=torch.long, device=pri.device)
    return out, pri.index_select(1, idx)


def loss_torch(enc_out, targets, dec, succ, off, valid, beta, E, Z):
    """the definition of grx_cenet_loss: (L, [L_est, L_rec, L_kl, L, n_v] detached); succ [mb, ld] holds the decoder's target of row r
    in columns [off, off + F)"""
    mb, F = dec.shape
    v, mu, raw = enc_out[:, :E], enc_out[:, E:E + Z], enc_out[:, E + Z:E + 2 * Z]
    lv = raw.clamp(LV_MIN, LV_MAX)
    d = v - targets
    l_est = (d * d).sum() / (mb * E)
    m = valid.reshape(-1, 1) != 0
    zero = dec.new_zeros(())
    d = torch.where(m, dec - succ[:, off:off + F], zero)          # (a select: a masked row's successor reaches neither the sum nor the gradient)
    n_v = m.sum().clamp(min=1).to(dec.dtype)
    l_rec = (d * d).sum() / (F * n_v)
    l_kl = (0.5 * (mu * mu + torch.exp(lv) - lv - 1.0)).sum() / mb
    total = l_est + l_rec + beta * l_kl
    return total, torch.stack([l_est.detach(), l_rec.detach(), l_kl.detach(), total.detach(), m.sum().to(dec.dtype)])


# ---- the same through libgrx_ppo.so --------------------------------------------------------------------------------------------------------
def head_hip(x, enc_out, eps, E, Z, pri=None, cols=None, out=None, targets=None):
    """grx_cenet_head, one launch on the current stream: contiguous fp32 tensors on one HIP device; `cols` a sequence of E ints; `out`
    [N, D + E + Z] / `targets` [N, E] are allocated here when they are not given"""
    lib = load_library()
    N, D = x.shape
    if not _ok(x, enc_out, eps) or tuple(enc_out.shape) != (N, E + 2 * Z) or tuple(eps.shape) != (N, Z):
        raise RuntimeError("grx_cenet_head needs contiguous float32 x [N, D], enc_out [N, E + 2Z] and eps [N, Z] on a HIP device")
    with torch.inference_mode(False):
        if out is None:
            out = torch.empty(N, D + E + Z, device=x.device, dtype=torch.float32)
        if pri is not None and targets is None:
            targets = torch.empty(N, E, device=x.device, dtype=torch.float32)
    P, carr = 0, None
    if pri is not None:
        if not _ok(pri, targets) or pri.dim() != 2 or pri.shape[0] != N or len(cols) != E or targets.numel() != N * E:
            raise RuntimeError(f"grx_cenet_head needs a contiguous float32 pri [N, P], targets [N, E] and {E} target columns")
        P, carr = pri.shape[1], (C.c_int * E)(*[int(c) for c in cols])
    if not _ok(out) or tuple(out.shape) != (N, D + E + Z):
        raise RuntimeError("grx_cenet_head needs a contiguous float32 out [N, D + E + Z] on x's device")
    with torch.cuda.device(x.device):
        rc = lib.grx_cenet_head(N, D, E, Z, x.data_ptr(), enc_out.data_ptr(), eps.data_ptr(), P, pri.data_ptr() if pri is not None else None,
                                carr, out.data_ptr(), targets.data_ptr() if pri is not None else None, _stream(x))
    if rc != 0:
        raise RuntimeError(f"grx_cenet_head failed ({rc}): {N} x {D}, E {E}, Z {Z}")
    return out, (targets if pri is not None else None)


class Reparam(torch.autograd.Function):
    """(enc_out [mb, E + 2Z], eps [mb, Z]) -> dec_in [mb, E + Z] through grx_cenet_reparam; backward through grx_cenet_reparam_backward"""

    @staticmethod
    def forward(ctx, enc_out, eps, E, Z):
        lib = load_library()
        mb = enc_out.shape[0]
        dec_in = torch.empty(mb, E + Z, device=enc_out.device, dtype=torch.float32)
        with torch.cuda.device(enc_out.device):
            rc = lib.grx_cenet_reparam(mb, E, Z, enc_out.data_ptr(), eps.data_ptr(), dec_in.data_ptr(), _stream(enc_out))
        if rc != 0:
            raise RuntimeError(f"grx_cenet_reparam failed ({rc}): mb {mb}, E {E}, Z {Z}")
        ctx.save_for_backward(enc_out, eps)
        ctx.sizes = (E, Z)
        return dec_in

    @staticmethod
    def backward(ctx, g):
        enc_out, eps = ctx.saved_tensors
        E, Z = ctx.sizes
        lib = load_library()
        g = g if (g.is_contiguous() and g.dtype == torch.float32) else g.contiguous().float()
        d = torch.empty_like(enc_out)
        with torch.cuda.device(enc_out.device):
            rc = lib.grx_cenet_reparam_backward(enc_out.shape[0], E, Z, enc_out.data_ptr(), eps.data_ptr(), g.data_ptr(), d.data_ptr(),
                                                _stream(enc_out))
        if rc != 0:
            raise RuntimeError(f"grx_cenet_reparam_backward failed ({rc})")
        return d, None, None, None


class Loss(torch.autograd.Function):
    """(enc_out, dec) -> (the scalar L, out [5] = (L_est, L_rec, L_kl, L, n_v)) of grx_cenet_loss; the scalar carries the gradient --
    backward hands out the stored d_enc_out and d_dec times the gradient arriving at it --, out is there to be read"""

    _sizes = {}

    @staticmethod
    def forward(ctx, enc_out, dec, targets, succ, off, valid, beta, E, Z):
        lib = load_library()
        mb, F = dec.shape
        key = (mb, E, Z, F)
        size = Loss._sizes.get(key)
        if size is None:
            size = Loss._sizes[key] = lib.grx_cenet_loss_partials_size(mb, E, Z, F)
        if size < 1 or tuple(enc_out.shape) != (mb, E + 2 * Z) or targets.numel() != mb * E or succ.shape[0] != mb or succ.stride(1) != 1:
            raise RuntimeError(f"grx_cenet_loss: invalid shapes enc_out {tuple(enc_out.shape)}, dec {tuple(dec.shape)}, succ {tuple(succ.shape)}")
        dev = enc_out.device
        out = torch.empty(5, device=dev, dtype=torch.float32)
        d_enc, d_dec = torch.empty_like(enc_out), torch.empty_like(dec)
        partials = torch.empty(size, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            rc = lib.grx_cenet_loss(mb, E, Z, F, enc_out.data_ptr(), targets.data_ptr(), dec.data_ptr(), succ.data_ptr(), int(succ.stride(0)),
                                    int(off), valid.data_ptr(), float(beta), out.data_ptr(), d_enc.data_ptr(), d_dec.data_ptr(),
                                    partials.data_ptr(), _stream(enc_out))
        if rc != 0:
            raise RuntimeError(f"grx_cenet_loss failed ({rc}): mb {mb}, E {E}, Z {Z}, F {F}")
        ctx.save_for_backward(d_enc, d_dec)
        ctx.mark_non_differentiable(out)
        return out[3].reshape(()), out

    @staticmethod
    def backward(ctx, g, _):
        d_enc, d_dec = ctx.saved_tensors
        return d_enc * g, d_dec * g, None, None, None, None, None, None, None


def reparam(enc_out, eps, E, Z, fused=True):
    """dec_in = [v_hat | z]: grx_cenet_reparam for contiguous fp32 tensors on a HIP device, the torch spelling otherwise"""
    if fused and _ok(enc_out, eps):
        return Reparam.apply(enc_out, eps, E, Z)
    return reparam_torch(enc_out, eps, E, Z)


def cenet_loss(enc_out, targets, dec, succ, off, valid, beta, E, Z, fused=True):
    """(L, [L_est, L_rec, L_kl, L, n_v]): grx_cenet_loss for contiguous fp32 tensors on a HIP device -- succ's rows may be strided, it is read
    in place --, the torch spelling otherwise"""
    if fused and _ok(enc_out, targets, dec) and succ.is_cuda and succ.dtype == torch.float32 and valid.dtype == torch.uint8 and valid.is_contiguous():
        return Loss.apply(enc_out, dec, targets, succ, off, valid, beta, E, Z)
    return loss_torch(enc_out, targets, dec, succ, off, valid, beta, E, Z)


def valid_rows(idx, N, T, dones):
    """valid[r] = (idx[r] // N < T - 1) and dones[idx[r]] == 0: grx_smooth_gather_rows' rule; dones [T N] uint8"""
    return (torch.div(idx, N, rounding_mode="floor") < T - 1) & (dones.reshape(-1).index_select(0, idx) == 0)


class CENetPolicy(nn.Module):
    """actor([x | v_hat | mu]): what inference and the exported TorchScript module put behind the history and the normaliser -- z = mu, no
    noise; [v_hat | mu] are the first E + Z columns of the encoder's output"""

    def __init__(self, actor, encoder, width: int):
        super().__init__()
        self.actor, self.encoder, self.width = actor, encoder, int(width)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.actor(torch.cat([x, self.encoder(x)[..., :self.width]], dim=-1))


def _embed(net, x):
    """net(x) without autograd: on a HIP device through grx_mlp_layer, one launch per layer"""
    if x.is_cuda:
        from .fused_loss import mlp_can_fuse, mlp_forward
        if mlp_can_fuse(net, x):
            return mlp_forward(net, x)
    return net(x)


class CENet(nn.Module):
    """`encoder`: MLP(D, E + 2Z) over the actor's input, `decoder`: MLP(E + Z, F); state_dict() is both.  Stored per rollout: `targets`
    (T, N, E), the labels of the storage's observation rows; `carry` (N, E), those of the row the next rollout starts with; `eps` (N, Z),
    the rollout step's noise."""

    def __init__(self, num_inputs, frame, num_obs, num_pri_obs, num_envs, num_steps, device="cpu", targets=("lin_vel",), latent_dim=16, beta=1.0,
                 encoder_dims=(128, 64), decoder_dims=(64, 128), learning_rate=1e-3, num_epochs=1):
        super().__init__()
        names = parse_targets(targets)
        enc_dims, dec_dims = check_dims(encoder_dims, "cenet_encoder_dims"), check_dims(decoder_dims, "cenet_decoder_dims")
        check_values(latent_dim, beta, learning_rate, num_epochs)
        D, F, N, T, Z = int(num_inputs), int(frame), int(num_envs), int(num_steps), int(latent_dim)
        if not 1 <= D <= MAX_INPUT:
            raise ValueError(f"--cenet: the actor's input has {D} columns, the encoder takes 1..{MAX_INPUT}")
        if not 1 <= F <= min(D, MAX_FRAME):
            raise ValueError(f"--cenet: a frame of {F} columns does not fit the actor's input of {D}")
        self.cols = target_columns(names, num_obs)
        E = len(self.cols)
        if E > MAX_TARGETS:
            raise ValueError(f"--cenet: {E} target columns, at most {MAX_TARGETS}")
        if max(self.cols) >= int(num_pri_obs):
            raise ValueError(f"--cenet: target column {max(self.cols)} is outside the privileged frame of {num_pri_obs} columns")
        self.num_inputs, self.frame, self.num_targets, self.latent_dim = D, F, E, Z
        self.num_outputs = E + Z                                           # the columns appended to the actor's input
        self.num_pri_obs, self.num_envs, self.num_steps, self.device = int(num_pri_obs), N, T, device
        self.config = {"targets": names, "latent_dim": Z, "encoder_dims": enc_dims, "decoder_dims": dec_dims, "activation": "elu"}
        self.beta, self.learning_rate, self.num_epochs = float(beta), float(learning_rate), int(num_epochs)
        self.encoder = MLP(D, E + 2 * Z, enc_dims, "elu")
        self.decoder = MLP(E + Z, F, dec_dims, "elu")
        self.to(device)
        self.targets = torch.zeros(T, N, E, device=device)
        self.carry = torch.zeros(N, E, device=device)
        self.eps = torch.zeros(N, Z, device=device)
        self._cols_t = torch.tensor(self.cols, dtype=torch.long, device=device)
        self._on_device = torch.device(device).type == "cuda"
        self._fused = self._on_device and fused_enabled()
        self._params = list(self.encoder.parameters()) + list(self.decoder.parameters())
        if self._on_device:   # device-resident, as the estimator's: the NaN-skip is Adam's found_inf hook, no host round trip
            self.optimizer = optim.Adam(self._params, lr=torch.tensor(self.learning_rate, device=device), fused=True, capturable=True)
            self._sums = torch.zeros(4, device=device)
        else:
            self.optimizer = optim.Adam(self._params, lr=self.learning_rate)
        self._gather, self._static, self._gather_src = None, None, None
        self.last_losses = (0.0, 0.0, 0.0)

    # ---- the rollout -------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, x, pri, slot):
        """x [N, D] the actor's input, pri [N, P] the raw privileged frame of the same env step -> [x | v_hat | z] [N, D + E + Z], a new
        tensor; the frame's target columns go to targets[slot], or to `carry` (slot None)"""
        E, Z = self.num_targets, self.latent_dim
        if x.dim() != 2 or tuple(x.shape) != (self.num_envs, self.num_inputs):
            raise ValueError(f"CENet: expected an input of {(self.num_envs, self.num_inputs)}, got {tuple(x.shape)}")
        if pri.dim() != 2 or tuple(pri.shape) != (self.num_envs, self.num_pri_obs):
            raise ValueError(f"CENet: expected a privileged frame of {(self.num_envs, self.num_pri_obs)}, got {tuple(pri.shape)}")
        if slot is not None and not 0 <= slot < self.num_steps:
            raise AssertionError("Rollout buffer overflow")
        dst = self.carry if slot is None else self.targets[slot]
        x = x if x.is_contiguous() else x.contiguous()
        torch.randn(self.eps.shape, out=self.eps)
        enc_out = _embed(self.encoder, x)
        if self._fused:
            out, _ = head_hip(x, enc_out, self.eps, E, Z, pri if pri.is_contiguous() else pri.contiguous(), self.cols, targets=dst)
            return out
        out, y = head_torch(x, enc_out, self.eps, E, Z, pri, self._cols_t)
        dst.copy_(y)
        return out

    @torch.no_grad()
    def begin_rollout(self):
        """before rollout step 0: the targets of the row this rollout starts with are the ones parked last"""
        self.targets[0].copy_(self.carry)

    # ---- the update --------------------------------------------------------------------------------------------------------------------
    def _loss(self, x, y, succ, off, valid, eps):
        """one minibatch: x [mb, D], y [mb, E], succ [mb, ld] with the decoder's target in columns [off, off + F), valid [mb] uint8,
        eps [mb, Z] -> (L, [L_est, L_rec, L_kl, L, n_v])"""
        E, Z = self.num_targets, self.latent_dim
        enc_out = self.encoder(x)
        dec = self.decoder(reparam(enc_out, eps, E, Z, self._fused))
        return cenet_loss(enc_out, y, dec, succ, off, valid, self.beta, E, Z, self._fused)

    def update(self, rows, dones, num_mini_batches):
        """the update on the stored rollout: `rows` (T, N, D + E + Z) the storage's observation rows, whose first D columns are the input
        and whose row s + N is row s one step later; `dones` (T, N[, 1]) uint8.  Returns the mean (L_est, L_rec, L_kl) over the steps with
        a finite loss (zeros: none)"""
        D, E, Z, F = self.num_inputs, self.num_targets, self.latent_dim, self.frame
        T, N, OW = self.num_steps, self.num_envs, D + E + Z
        if tuple(rows.shape) != (T, N, OW):
            raise ValueError(f"CENet.update: expected rows of {(T, N, OW)}, got {tuple(rows.shape)}")
        if dones.numel() != T * N or dones.dtype != torch.uint8:
            raise ValueError(f"CENet.update: expected {T * N} uint8 dones, got {tuple(dones.shape)} {dones.dtype}")
        n, nmb = T * N, int(num_mini_batches)
        mb = n // nmb
        wide, targets, dones = rows.flatten(0, 1), self.targets.flatten(0, 1), dones.reshape(-1)
        indices = torch.randperm(nmb * mb, requires_grad=False, device=self.device)   # one permutation, every epoch
        self.encoder.train(); self.decoder.train()
        off = D - F
        if not self._on_device:
            total, steps = [0.0, 0.0, 0.0], 0
            for _ in range(self.num_epochs):
                for i in range(nmb):
                    idx = indices[i * mb:(i + 1) * mb]
                    v = valid_rows(idx, N, T, dones)
                    succ = wide.index_select(0, torch.where(v, idx + N, idx))
                    eps = torch.randn(mb, Z, device=self.device)
                    loss, parts = self._loss(wide[idx, :D], targets[idx], succ, off, v.to(torch.uint8), eps)
                    if not torch.isfinite(loss):
                        continue
                    self.optimizer.zero_grad(set_to_none=False)
                    loss.backward()
                    self.optimizer.step()
                    total, steps = [a + float(b) for a, b in zip(total, parts[:3])], steps + 1
            self.last_losses = tuple(a / steps for a in total) if steps else (0.0, 0.0, 0.0)
            return self.last_losses
        sums = self._sums.zero_()
        if self._static is None or self._static[1].shape[0] != mb or self._gather_src != (wide.data_ptr(), dones.data_ptr()):
            # the wide rows with their successors behind them, and the labels, in one launch (grx_smooth_gather_rows, want_succ)
            from .smooth import SmoothGather
            self._static = [torch.empty(2 * mb, OW, device=self.device), torch.empty(mb, E, device=self.device),
                            torch.empty(mb, dtype=torch.uint8, device=self.device), torch.empty(mb, Z, device=self.device)]
            self._gather = SmoothGather([wide, targets], self._static[:2], N, T, dones, True, False, None, 0.0, self._static[2])
            self._gather_src = (wide.data_ptr(), dones.data_ptr())
        both, yb, valid, eps = self._static
        for _ in range(self.num_epochs):
            for i in range(nmb):
                self._gather(indices[i * mb:(i + 1) * mb])
                torch.randn(eps.shape, out=eps)
                xb = both[:mb, :D].contiguous()   # (the training MLP takes contiguous rows: a copy of the minibatch, not of the rollout)
                loss, parts = self._loss(xb, yb, both[mb:], off, valid, eps)
                self.optimizer.zero_grad(set_to_none=False)
                loss.backward()
                with torch.no_grad():
                    loss = loss.detach()
                    bad = ~torch.isfinite(loss)
                    self.optimizer.found_inf = bad.float().reshape(())   # (fused Adam leaves parameters and moments alone where it is 1)
                    self.optimizer.grad_scale = None
                self.optimizer.step()
                with torch.no_grad():
                    sums[:3] += torch.where(bad, torch.zeros_like(parts[:3]), parts[:3])
                    sums[3] += (~bad).float()
        *total, steps = sums.tolist()                              # the only device->host transfer of the update
        self.last_losses = tuple(a / steps for a in total) if steps else (0.0, 0.0, 0.0)
        return self.last_losses

    # ---- the checkpoint's "cenet" entry ------------------------------------------------------------------------------------------------------
    def checkpoint(self):
        return {"state_dict": self.state_dict(), "optimizer_state_dict": self.optimizer.state_dict(), "config": dict(self.config)}

    def load_checkpoint(self, saved, load_optimizer=True):
        """the networks and -- load_optimizer -- the optimizer of a saved "cenet" entry; the learning rate stays this run's.  ValueError when
        the targets, the latent width, the hidden layers or the input width are other than this run's"""
        for k in self.config:
            if saved["config"][k] != self.config[k]:
                raise ValueError(f"the checkpoint's cenet entry has {k}={saved['config'][k]!r}, this run {self.config[k]!r}")
        w = saved["state_dict"]["encoder.model.0.weight"]
        if w.shape[1] != self.num_inputs:
            raise ValueError(f"the checkpoint's cenet entry reads {w.shape[1]} input columns, this run {self.num_inputs}")
        self.load_state_dict(saved["state_dict"])   # (in place)
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
