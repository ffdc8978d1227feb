"""Action-smoothness regularisation of the policy (CAPS: Mysore et al., "Regularizing Action Policies for Smooth Control", ICRA 2021;
DESIGN.md 4.14): two terms on the actor's mean action, added to the PPO loss.

Storage rows are s = t N + e (T rollout steps, N envs).  Minibatch row r has the source row s = idx[r], t = s // N, and

    valid[r] = (t < T - 1) and dones[s] == 0         (row s + N is the same env one step later; after a done it is a reset observation)

The actor runs on R mb rows, R = 1 + [temporal] + [spatial], in this block order:

    own:        obs[s]
    successor:  obs[s + N] where valid, else obs[s] again                 (temporal)
    perturbed:  fmaf(sigma, eps[r], obs[s]),  eps ~ N(0, 1) per step       (spatial)

and with mu = actor(those rows), n_v = sum valid, A actions:

    L_T = sum_{r valid} sum_a (mu[r][a] - mu_succ[r][a])^2 / (A max(n_v, 1))
    L_S = sum_r sum_a (mu[r][a] - mu_pert[r][a])^2 / (A mb)
    loss = PPO loss on rows [0, mb) + coef_t L_T + coef_s L_S

Squares, not the paper's norm (no gradient at a zero difference, which a masked row holds exactly).  Gradients flow to both sides of each
difference.  The mask is a select: an invalid row adds exactly 0 and gets exactly zero gradient, whatever its successor block holds.

`smooth_gather_torch` / `smooth_loss_torch` are the definitions of grx_smooth_gather_rows / grx_smooth_loss (include/grx_ppo_smooth.h) in
torch: what CPU tensors use, and what GRX_SMOOTH_FUSED=0 selects on a HIP device (the cross-check, as GRX_SYM_FUSED is to the mirrored
gather)."""
import ctypes as C
import math
import os

import torch

MODES = ("temporal", "spatial", "both")


def fused_enabled():
    return os.environ.get("GRX_SMOOTH_FUSED", "1") != "0"


def blocks(mode):
    """(has_succ, has_pert) of a mode"""
    if mode not in MODES:
        raise ValueError(f"smooth must be one of {MODES}, not {mode!r}")
    return mode in ("temporal", "both"), mode in ("spatial", "both")


def check_values(coef_t, coef_s, sigma, who="PPO"):
    for name, v in (("--smooth_temporal_coef", coef_t), ("--smooth_spatial_coef", coef_s), ("--smooth_sigma", sigma)):
        if not (isinstance(v, (int, float)) and math.isfinite(v) and v >= 0):
            raise ValueError(f"{who}: --smooth with {name} {v!r}: it must be finite and not negative")


# ---- the gather ----------------------------------------------------------------------------------------------------------------------
def smooth_gather_torch(srcs, dsts, idx, N, T, dones, want_succ, want_pert, eps, sigma, valid):
    """grx_smooth_gather_rows in torch: dsts[t][:mb] = srcs[t][idx] for every tensor; behind tensor 0 the successor rows (want_succ; valid
    [mb] uint8 is written) and the perturbed rows (want_pert; eps [mb, W]).  dones: [T N] uint8."""
    mb = idx.numel()
    for src, dst in zip(srcs, dsts):
        dst[:mb].copy_(src.index_select(0, idx))
    src, dst = srcs[0], dsts[0]
    if want_succ:
        v = (torch.div(idx, N, rounding_mode="floor") < T - 1) & (dones.reshape(-1).index_select(0, idx) == 0)
        valid.copy_(v)
        dst[mb:2 * mb].copy_(src.index_select(0, torch.where(v, idx + N, idx)))
    if want_pert:
        p = 2 if want_succ else 1
        # (addcmul rounds once on a HIP device, as the kernel's fmaf; on the CPU the product may be rounded first: within 2^-23 (|sigma eps| + |x|))
        dst[p * mb:(p + 1) * mb].copy_(torch.addcmul(dst[:mb], eps, eps.new_full((), float(sigma))))


class SmoothGather:
    """idx -> the minibatch with its successor / perturbed rows behind tensor 0, for a fixed set of (src, dst) pairs in one launch of
    grx_smooth_gather_rows.  The pointer tables are built once; eps and valid are fixed buffers the caller refills / reads."""

    def __init__(self, srcs, dsts, N, T, dones, want_succ, want_pert, eps, sigma, valid):
        from .fused_loss import load_ppo_library
        self.lib = load_ppo_library()
        n = len(srcs)
        R = 1 + int(bool(want_succ)) + int(bool(want_pert))
        mb = dsts[0].shape[0] // R
        ok = lambda t: t.dtype == torch.float32 and t.is_contiguous()
        assert n == len(dsts) and all(ok(s) and ok(d) and s.shape[1:] == d.shape[1:] for s, d in zip(srcs, dsts))
        assert dsts[0].shape[0] == R * mb and all(d.shape[0] == mb for d in dsts[1:]) and srcs[0].shape[0] == N * T
        assert not want_pert or (ok(eps) and tuple(eps.shape) == (mb, srcs[0].shape[1]))
        assert not want_succ or (dones.dtype == torch.uint8 and dones.is_contiguous() and dones.numel() == N * T
                                 and valid.dtype == torch.uint8 and valid.is_contiguous() and valid.numel() == mb)
        self.n, self.mb, self.device = n, mb, srcs[0].device
        self.src = (C.c_void_p * n)(*[s.data_ptr() for s in srcs])
        self.dst = (C.c_void_p * n)(*[d.data_ptr() for d in dsts])
        self.w = (C.c_int * n)(*[int(s[0].numel()) for s in srcs])
        self.N, self.T, self.want_succ, self.want_pert, self.sigma = int(N), int(T), int(bool(want_succ)), int(bool(want_pert)), float(sigma)
        self.dones = dones.data_ptr() if want_succ else None
        self.eps = eps.data_ptr() if want_pert else None
        self.valid = valid.data_ptr() if want_succ else None
        self.keep = (srcs, dsts, dones, eps, valid)

    def __call__(self, idx):
        assert idx.dtype == torch.int64 and idx.is_contiguous() and idx.numel() == self.mb
        with torch.cuda.device(self.device):
            rc = self.lib.grx_smooth_gather_rows(self.n, self.src, self.dst, self.w, idx.data_ptr(), self.mb, self.N, self.T, self.dones,
                                                 self.want_succ, self.want_pert, self.eps, self.sigma, self.valid,
                                                 torch.cuda.current_stream(self.device).cuda_stream)
        if rc:
            raise RuntimeError(f"grx_smooth_gather_rows failed ({rc})")


class NoisyGather:
    """a gather with the step's noise drawn in front of it: eps ~ N(0, 1) by torch.randn from the generator of eps's device, into the
    fixed buffer the gather reads (eps None: no draw)"""

    def __init__(self, eps, gather):
        self.eps, self.gather = eps, gather

    def __call__(self, idx):
        if self.eps is not None:
            torch.randn(self.eps.shape, out=self.eps)
        self.gather(idx)


# ---- the loss ------------------------------------------------------------------------------------------------------------------------
def smooth_loss_torch(mu, has_succ, has_pert, valid, coef_t, coef_s):
    """the definition: (coef_t L_T + coef_s L_S, [L_T, L_S] detached) from mu [R mb, A] (a term that is off is 0)"""
    R = 1 + int(bool(has_succ)) + int(bool(has_pert))
    mb, A = mu.shape[0] // R, mu.shape[1]
    own = mu[:mb]
    zero = mu.new_zeros(())
    total, lt, ls = zero, zero, zero
    if has_succ:
        v = valid.reshape(-1, 1) != 0
        d = torch.where(v, own - mu[mb:2 * mb], zero)     # (a select: a masked row's successor reaches neither the sum nor the gradient)
        n_v = v.sum().clamp(min=1).to(mu.dtype)
        lt = (d * d).sum() / (A * n_v)
        total = total + coef_t * lt
    if has_pert:
        p = 2 if has_succ else 1
        d = own - mu[p * mb:(p + 1) * mb]
        ls = (d * d).sum() / (A * mb)
        total = total + coef_s * ls
    return total, torch.stack([lt.detach(), ls.detach()])


class SmoothLoss(torch.autograd.Function):
    """mu [R mb, A] -> (the scalar coef_t L_T + coef_s L_S, out [4] = (L_T, L_S, that scalar, n_v)) of grx_smooth_loss; the scalar carries
    the gradient -- backward hands out the stored d_mu times the gradient arriving at it --, out is there to be read (L_T, L_S)."""

    _sizes = {}   # (mb, A) -> floats of scratch

    @staticmethod
    def forward(ctx, mu, has_succ, has_pert, valid, coef_t, coef_s):
        from .fused_loss import load_ppo_library
        lib = load_ppo_library()
        R = 1 + int(bool(has_succ)) + int(bool(has_pert))
        mb, A = mu.shape[0] // R, mu.shape[1]
        size = SmoothLoss._sizes.get((mb, A))
        if size is None:
            size = SmoothLoss._sizes[(mb, A)] = lib.grx_smooth_loss_partials_size(mb, A)
        if size < 1 or mu.shape[0] != R * mb:
            raise RuntimeError(f"grx_smooth_loss: invalid shape {tuple(mu.shape)} for {R} row blocks")
        dev = mu.device
        out = torch.empty(4, device=dev, dtype=torch.float32)
        d_mu = torch.empty_like(mu)
        partials = torch.empty(size, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            rc = lib.grx_smooth_loss(mb, A, mu.data_ptr(), int(bool(has_succ)), int(bool(has_pert)), valid.data_ptr() if has_succ else None,
                                     float(coef_t), float(coef_s), out.data_ptr(), d_mu.data_ptr(), partials.data_ptr(),
                                     C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        if rc != 0:
            raise RuntimeError(f"grx_smooth_loss failed ({rc}): mb {mb}, num_actions {A}")
        ctx.save_for_backward(d_mu)
        ctx.mark_non_differentiable(out)
        return out[2].reshape(()), out

    @staticmethod
    def backward(ctx, g, _):
        d_mu, = ctx.saved_tensors
        return d_mu * g, None, None, None, None, None


def smooth_loss(mu, has_succ, has_pert, valid, coef_t, coef_s, fused=True):
    """(coef_t L_T + coef_s L_S, [L_T, L_S]): grx_smooth_loss for a contiguous fp32 [R mb, A] tensor on a HIP device, the torch spelling
    otherwise"""
    if fused and mu.is_cuda and mu.dtype == torch.float32 and mu.is_contiguous() and mu.dim() == 2:
        loss, out = SmoothLoss.apply(mu, has_succ, has_pert, valid, coef_t, coef_s)
        return loss, out[:2]
    return smooth_loss_torch(mu, has_succ, has_pert, valid, coef_t, coef_s)
