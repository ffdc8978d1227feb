"""PPO minibatch loss through libgrx_ppo.so (include/grx_ppo.h): forward value and gradients from one HIP kernel.

The expression is rsl_rl/algorithms/ppo.py:215-245 with torch.distributions.Normal's log_prob / entropy; the
torch spelling of the same arithmetic lives in ppo.py (`_loss_torch`) and is what CPU tensors use.  On a GPU the
~100 element-wise kernels that expression and its autograd backward expand to are one launch plus a 64-thread
finalize; the result enters autograd through `FusedPPOLoss`, whose backward hands out the stored gradients.
"""
import ctypes as C
import os

import torch

_LIB = None


def load_ppo_library():
    """libgrx_ppo.so next to the step library (built in-tree by __graft_entry__.build() / make -C csrc)."""
    global _LIB
    if _LIB is None:
        path = os.environ.get("GRX_PPO_LIB") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc", "libgrx_ppo.so")
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(there is no silent fallback for CUDA tensors; set GRX_PPO_FUSED_LOSS=0 to use the torch expression)")
        lib = C.CDLL(path)
        fp = C.c_void_p
        lib.grx_ppo_loss.restype = C.c_int
        lib.grx_ppo_loss.argtypes = [C.c_int, C.c_int] + [fp] * 10 + [C.c_float, C.c_float, C.c_float, C.c_int] + [fp] * 5 + [C.c_void_p]
        lib.grx_ppo_loss_partials_size.restype = C.c_int
        lib.grx_ppo_loss_partials_size.argtypes = [C.c_int]
        lib.grx_ppo_colsum.restype = C.c_int
        lib.grx_ppo_colsum.argtypes = [C.c_int, C.c_int, fp, fp, fp, C.c_void_p]
        lib.grx_ppo_colsum_partials_size.restype = C.c_int
        lib.grx_ppo_colsum_partials_size.argtypes = [C.c_int, C.c_int]
        lib.grx_ppo_store_transition.restype = C.c_int
        lib.grx_ppo_store_transition.argtypes = [C.c_int] * 4 + [fp] * 10 + [C.c_float] + [fp] * 13 + [C.c_void_p]
        lib.grx_ppo_elu_backward_colsum.restype = C.c_int
        lib.grx_ppo_elu_backward_colsum.argtypes = [C.c_int, C.c_int, fp, fp, fp, fp, fp, C.c_void_p]
        lib.grx_ppo_gather_rows.restype = C.c_int
        lib.grx_ppo_gather_rows.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int), fp, C.c_int, C.c_void_p]
        lib.grx_mlp_layer.restype = C.c_int
        lib.grx_mlp_layer.argtypes = [C.c_int] * 3 + [fp] * 4 + [C.c_int, C.c_void_p]
        lib.grx_mlp_layer_bf16.restype = C.c_int
        lib.grx_mlp_layer_bf16.argtypes = [C.c_int] * 3 + [fp] * 4 + [C.c_int, C.c_void_p]
        lib.grx_mlp_input_grad_bf16.restype = C.c_int
        lib.grx_mlp_input_grad_bf16.argtypes = [C.c_int] * 3 + [fp] * 3 + [C.c_void_p]
        lib.grx_mlp_weight_grad_bf16_partials_size.restype = C.c_int
        lib.grx_mlp_weight_grad_bf16_partials_size.argtypes = [C.c_int] * 3
        lib.grx_mlp_weight_grad_bf16.restype = C.c_int
        lib.grx_mlp_weight_grad_bf16.argtypes = [C.c_int] * 3 + [fp] * 4 + [C.c_void_p]
        lib.grx_mlp_policy_head.restype = C.c_int
        lib.grx_mlp_policy_head.argtypes = [C.c_int] * 3 + [fp] * 9 + [C.c_void_p]
        lib.grx_ppo_step_tail.restype = C.c_int
        lib.grx_ppo_step_tail.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.grx_ppo_step_tail_blocks.restype = C.c_int
        lib.grx_ppo_step_tail_blocks.argtypes = [C.c_void_p]
        # the observation normaliser (rl/normalizer.py)
        lib.grx_obs_norm_partials_size.restype = C.c_int
        lib.grx_obs_norm_partials_size.argtypes = [C.c_int, C.c_int]
        lib.grx_obs_norm_moments.restype = C.c_int
        lib.grx_obs_norm_moments.argtypes = [C.c_int, C.c_int, fp, fp, C.c_void_p]
        lib.grx_obs_norm_merge.restype = C.c_int
        lib.grx_obs_norm_merge.argtypes = [C.c_int, C.c_int, C.c_int] + [fp] * 5 + [C.c_void_p]
        lib.grx_obs_norm_combine.restype = C.c_int
        lib.grx_obs_norm_combine.argtypes = [C.c_int, C.c_int, fp, fp, C.c_void_p]
        lib.grx_obs_norm_apply.restype = C.c_int
        lib.grx_obs_norm_apply.argtypes = [C.c_int, C.c_int, fp, fp, fp, C.c_float, fp, C.c_void_p]
        lib.grx_obs_norm_step.restype = C.c_int
        lib.grx_obs_norm_step.argtypes = [C.c_int, C.c_int] + [fp] * 6 + [C.c_float, fp, C.c_void_p]
        # the observation history (rl/history.py)
        lib.grx_obs_history_push.restype = C.c_int
        lib.grx_obs_history_push.argtypes = [C.c_int] * 3 + [fp, fp, C.c_int, fp, fp, C.c_void_p]
        # policy distillation (rl/distillation.py)
        lib.grx_distill_loss_partials_size.restype = C.c_int
        lib.grx_distill_loss_partials_size.argtypes = [C.c_int, C.c_int]
        lib.grx_distill_loss.restype = C.c_int
        lib.grx_distill_loss.argtypes = [C.c_int, C.c_int, fp, fp, C.c_int, fp, fp, fp, C.c_void_p]
        lib.grx_distill_store.restype = C.c_int
        lib.grx_distill_store.argtypes = [C.c_int] * 3 + [fp] * 11 + [C.c_void_p]
        # left-right symmetry (rl/symmetry.py)
        pp = C.POINTER(C.c_void_p)
        lib.grx_sym_gather_rows.restype = C.c_int
        lib.grx_sym_gather_rows.argtypes = [C.c_int, pp, pp, C.POINTER(C.c_int), C.POINTER(C.c_int), pp, pp, pp, fp, C.c_int, C.c_void_p]
        # random network distillation (rl/rnd.py)
        lib.grx_rnd_reward_partials_size.restype = C.c_int
        lib.grx_rnd_reward_partials_size.argtypes = [C.c_int]
        lib.grx_rnd_reward.restype = C.c_int
        lib.grx_rnd_reward.argtypes = [C.c_int, C.c_int, fp, fp, C.c_float, C.c_float, C.c_float] + [fp] * 9 + [C.c_void_p]
        # a state-dependent action noise (rl/modules.py state_dependent_std)
        lib.grx_ppo_loss_sd_partials_size.restype = C.c_int
        lib.grx_ppo_loss_sd_partials_size.argtypes = [C.c_int]
        lib.grx_ppo_loss_sd.restype = C.c_int
        lib.grx_ppo_loss_sd.argtypes = [C.c_int, C.c_int, fp, C.c_int] + [fp] * 8 + [C.c_float, C.c_float, C.c_float, C.c_int] + [fp] * 4 + [C.c_void_p]
        lib.grx_mlp_policy_head_sd.restype = C.c_int
        lib.grx_mlp_policy_head_sd.argtypes = [C.c_int] * 3 + [fp] * 3 + [C.c_int] + [fp] * 5 + [C.c_void_p]
        # the action-smoothness regulariser (rl/smooth.py)
        lib.grx_smooth_gather_rows.restype = C.c_int
        lib.grx_smooth_gather_rows.argtypes = ([C.c_int, pp, pp, C.POINTER(C.c_int), fp, C.c_int, C.c_int, C.c_int, fp, C.c_int, C.c_int, fp,
                                                C.c_float, fp, C.c_void_p])
        lib.grx_smooth_loss_partials_size.restype = C.c_int
        lib.grx_smooth_loss_partials_size.argtypes = [C.c_int, C.c_int]
        lib.grx_smooth_loss.restype = C.c_int
        lib.grx_smooth_loss.argtypes = [C.c_int, C.c_int, fp, C.c_int, C.c_int, fp, C.c_float, C.c_float, fp, fp, fp, C.c_void_p]
        # the concurrent state estimator's rollout forward (rl/estimator.py)
        lib.grx_est_forward.restype = C.c_int
        lib.grx_est_forward.argtypes = [fp, C.c_int, C.c_int, fp, C.c_int, fp, C.POINTER(C.c_int), fp, fp, C.c_void_p]
        # the GAE scan with value normalisation (rl/value_norm.py)
        lib.grx_gae_partials_size.restype = C.c_int
        lib.grx_gae_partials_size.argtypes = [C.c_int, C.c_int]
        lib.grx_gae_returns.restype = C.c_int
        lib.grx_gae_returns.argtypes = [C.c_int, C.c_int] + [fp] * 4 + [C.c_float] * 3 + [fp] * 10 + [C.c_void_p]
        # the Lipschitz gradient penalty's element-wise passes (rl/grad_penalty.py)
        lib.grx_gp_seed.restype = C.c_int
        lib.grx_gp_seed.argtypes = [C.c_int, C.c_int] + [fp] * 4 + [C.c_void_p]
        lib.grx_gp_gate.restype = C.c_int
        lib.grx_gp_gate.argtypes = [C.c_int, C.c_int] + [fp] * 3 + [C.c_void_p]
        lib.grx_gp_sqnorm_partials_size.restype = C.c_int
        lib.grx_gp_sqnorm_partials_size.argtypes = [C.c_int, C.c_int]
        lib.grx_gp_sqnorm.restype = C.c_int
        lib.grx_gp_sqnorm.argtypes = [C.c_int, C.c_int] + [fp] * 3 + [C.c_void_p]
        lib.grx_gp_gate_backward.restype = C.c_int
        lib.grx_gp_gate_backward.argtypes = [C.c_int, C.c_int] + [fp] * 8 + [C.c_void_p]
        lib.grx_gp_seed_backward.restype = C.c_int
        lib.grx_gp_seed_backward.argtypes = [C.c_int, C.c_int] + [fp] * 8 + [C.c_void_p]
        # LayerNorm + ELU behind a hidden layer's product (rl/modules.py _TrainLinearLNELU)
        lib.grx_ln_elu_forward.restype = C.c_int
        lib.grx_ln_elu_forward.argtypes = [C.c_int, C.c_int, fp, fp, fp, C.c_float, fp, fp, fp, C.c_void_p]
        lib.grx_ln_elu_backward_partials_size.restype = C.c_int
        lib.grx_ln_elu_backward_partials_size.argtypes = [C.c_int, C.c_int]
        lib.grx_ln_elu_backward.restype = C.c_int
        lib.grx_ln_elu_backward.argtypes = [C.c_int, C.c_int] + [fp] * 11 + [C.c_void_p]
        _LIB = lib
    return _LIB


TAIL_MAX = 24


class _TailTensors(C.Structure):   # include/grx_ppo.h grx_ppo_tail_tensors
    _fields_ = [("n", C.c_int), ("pad", C.c_int), ("param", C.c_void_p * TAIL_MAX), ("grad", C.c_void_p * TAIL_MAX),
                ("exp_avg", C.c_void_p * TAIL_MAX), ("exp_avg_sq", C.c_void_p * TAIL_MAX), ("step", C.c_void_p * TAIL_MAX),
                ("numel", C.c_longlong * TAIL_MAX)]


class _TailArgs(C.Structure):      # grx_ppo_tail_args
    _fields_ = [("loss", C.c_void_p), ("bad_flag", C.c_void_p), ("kl", C.c_void_p), ("lr", C.c_void_p), ("value_loss", C.c_void_p),
                ("surrogate_loss", C.c_void_p), ("sums", C.c_void_p), ("partials", C.c_void_p), ("adaptive", C.c_int), ("pad", C.c_int),
                ("desired_kl", C.c_float), ("lr_min", C.c_float), ("lr_max", C.c_float), ("max_grad_norm", C.c_float),
                ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double)]


class StepTail:
    """grx_ppo_step_tail for one torch.optim.Adam (fused, capturable, one param group, no weight decay / amsgrad / maximize): the adaptive
    learning rate, the NaN-skip, clip_grad_norm_ and Adam.step() of a PPO minibatch step in two launches.  The optimizer's own state tensors
    (exp_avg, exp_avg_sq, step) are updated in place -- created here, as torch creates them lazily, if the optimizer has not stepped yet --,
    so optimizer.state_dict() / load_state_dict() and checkpoints are those of the torch path."""

    @staticmethod
    def supported(optimizer, params):
        g = optimizer.param_groups
        return (len(g) == 1 and len(params) <= TAIL_MAX and not g[0].get("amsgrad") and not g[0].get("maximize") and g[0].get("weight_decay", 0) == 0
                and all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() for p in params))

    def __init__(self, optimizer, params, lr_t):
        self.lib = load_ppo_library()
        self.opt, self.params, self.lr_t = optimizer, list(params), lr_t
        self.t, self.a = _TailTensors(), _TailArgs()
        self.key, self.partials = None, None

    def _state(self, p):
        st = self.opt.state[p]
        if "exp_avg" not in st:   # torch's lazy initialisation (optim/adam.py _init_group), capturable / fused: the step counter is a device scalar
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    def __call__(self, loss, kl, value_loss, surrogate_loss, sums, adaptive, desired_kl, lr_min, lr_max, max_grad_norm, bad_flag=None):
        t, a = self.t, self.a
        sts = [self._state(p) for p in self.params]
        key = tuple(x.data_ptr() for p, st in zip(self.params, sts) for x in (p, st["exp_avg"], st["exp_avg_sq"], st["step"]))
        if key != self.key:
            t.n = len(self.params)
            for i, (p, st) in enumerate(zip(self.params, sts)):
                if not (st["step"].is_cuda and st["step"].dtype == torch.float32 and st["exp_avg"].is_contiguous() and st["exp_avg_sq"].is_contiguous()):
                    raise RuntimeError("StepTail: the optimizer state is not torch's fused / capturable layout")
                t.param[i], t.exp_avg[i], t.exp_avg_sq[i], t.step[i], t.numel[i] = p.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), st["step"].data_ptr(), p.numel()
            nb = self.lib.grx_ppo_step_tail_blocks(C.byref(t))
            if nb < 1:
                raise RuntimeError("grx_ppo_step_tail_blocks failed")
            self.partials = torch.empty(nb, device=self.params[0].device, dtype=torch.float32)
            self.key = key
        for i, p in enumerate(self.params):
            g = p.grad
            if g is None or not g.is_contiguous() or g.dtype != torch.float32:
                raise RuntimeError("StepTail: every parameter needs a contiguous fp32 .grad")
            t.grad[i] = g.data_ptr()
        g0 = self.opt.param_groups[0]
        a.loss, a.kl, a.lr = loss.data_ptr(), kl.data_ptr(), self.lr_t.data_ptr()
        a.bad_flag = bad_flag.data_ptr() if bad_flag is not None else None
        a.value_loss, a.surrogate_loss = value_loss.data_ptr(), surrogate_loss.data_ptr()
        a.sums = sums.data_ptr() if sums is not None else None
        a.partials = self.partials.data_ptr()
        a.adaptive = int(bool(adaptive))
        a.desired_kl, a.lr_min, a.lr_max, a.max_grad_norm = float(desired_kl or 0.0), float(lr_min), float(lr_max), float(max_grad_norm)
        a.beta1, a.beta2, a.eps = float(g0["betas"][0]), float(g0["betas"][1]), float(g0["eps"])
        dev = self.params[0].device
        with torch.cuda.device(dev):
            rc = self.lib.grx_ppo_step_tail(C.byref(t), C.byref(a), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        if rc != 0:
            raise RuntimeError(f"grx_ppo_step_tail failed ({rc})")


def _f32c(x):
    return x if (x.dtype == torch.float32 and x.is_contiguous()) else x.contiguous().float()


class FusedPPOLoss(torch.autograd.Function):
    """(mu [B, A], std [A], value [B] or [B, 1]; data...) -> tensor [surrogate, value_loss, total_loss, mean_kl]."""

    @staticmethod
    def forward(ctx, mu, std, value, actions, old_logp, old_mu, old_sigma, advantages, returns, target_values,
                clip_param, value_loss_coef, entropy_coef, use_clipped_value_loss):
        lib = load_ppo_library()
        B, A = mu.shape
        mu_c, std_c, value_c = _f32c(mu), _f32c(std), _f32c(value).reshape(-1)
        data = [_f32c(t) for t in (actions, old_logp, old_mu, old_sigma, advantages, returns, target_values)]
        out = torch.empty(4, device=mu.device, dtype=torch.float32)
        d_mu = torch.empty_like(mu_c)
        d_std = torch.empty_like(std_c)
        d_value = torch.empty_like(value_c)
        partials = torch.empty(lib.grx_ppo_loss_partials_size(B), device=mu.device, dtype=torch.float32)
        stream = torch.cuda.current_stream(mu.device).cuda_stream
        with torch.cuda.device(mu.device):
            rc = lib.grx_ppo_loss(B, A, mu_c.data_ptr(), std_c.data_ptr(), value_c.data_ptr(), *[t.data_ptr() for t in data],
                                  float(clip_param), float(value_loss_coef), float(entropy_coef), int(bool(use_clipped_value_loss)),
                                  out.data_ptr(), d_mu.data_ptr(), d_std.data_ptr(), d_value.data_ptr(), partials.data_ptr(), C.c_void_p(stream))
        if rc != 0:
            raise RuntimeError(f"grx_ppo_loss failed ({rc}): batch {B}, num_actions {A}")
        ctx.save_for_backward(d_mu, d_std, d_value)
        ctx.value_shape = value.shape
        return out

    @staticmethod
    def backward(ctx, g):
        d_mu, d_std, d_value = ctx.saved_tensors
        gl = g[2]   # only the total loss is differentiable
        return (d_mu * gl, d_std * gl, (d_value * gl).reshape(ctx.value_shape)) + (None,) * 11


def fused_ppo_loss(mu, std, value, actions, old_logp, old_mu, old_sigma, advantages, returns, target_values,
                   clip_param, value_loss_coef, entropy_coef, use_clipped_value_loss):
    return FusedPPOLoss.apply(mu, std, value, actions, old_logp, old_mu, old_sigma, advantages, returns, target_values,
                              clip_param, value_loss_coef, entropy_coef, use_clipped_value_loss)


class FusedPPOLossSD(torch.autograd.Function):
    """FusedPPOLoss for a state-dependent sigma (grx_ppo_loss_sd): (raw [B, 2A] = [mean | s], value [B] or [B, 1]; data...) -> tensor
    [surrogate, value_loss, total_loss, mean_kl].  The kernel writes the gradient onto the actor's raw output: no split, cat or
    exp-backward launches around it."""

    @staticmethod
    def forward(ctx, raw, value, actions, old_logp, old_mu, old_sigma, advantages, returns, target_values,
                log_std, clip_param, value_loss_coef, entropy_coef, use_clipped_value_loss):
        lib = load_ppo_library()
        B, A = actions.shape
        if tuple(raw.shape) != (B, 2 * A):
            raise RuntimeError(f"fused_ppo_loss_sd: raw is {tuple(raw.shape)}, expected {(B, 2 * A)} ([mean | s] of {A} actions)")
        raw_c, value_c = _f32c(raw), _f32c(value).reshape(-1)
        data = [_f32c(t) for t in (actions, old_logp, old_mu, old_sigma, advantages, returns, target_values)]
        out = torch.empty(4, device=raw.device, dtype=torch.float32)
        d_raw = torch.empty_like(raw_c)
        d_value = torch.empty_like(value_c)
        partials = torch.empty(lib.grx_ppo_loss_sd_partials_size(B), device=raw.device, dtype=torch.float32)
        stream = torch.cuda.current_stream(raw.device).cuda_stream
        with torch.cuda.device(raw.device):
            rc = lib.grx_ppo_loss_sd(B, A, raw_c.data_ptr(), int(bool(log_std)), value_c.data_ptr(), *[t.data_ptr() for t in data],
                                     float(clip_param), float(value_loss_coef), float(entropy_coef), int(bool(use_clipped_value_loss)),
                                     out.data_ptr(), d_raw.data_ptr(), d_value.data_ptr(), partials.data_ptr(), C.c_void_p(stream))
        if rc != 0:
            raise RuntimeError(f"grx_ppo_loss_sd failed ({rc}): batch {B}, num_actions {A}")
        ctx.save_for_backward(d_raw, d_value)
        ctx.value_shape = value.shape
        return out

    @staticmethod
    def backward(ctx, g):
        d_raw, d_value = ctx.saved_tensors
        gl = g[2]   # only the total loss is differentiable
        return (d_raw * gl, (d_value * gl).reshape(ctx.value_shape)) + (None,) * 12


def fused_ppo_loss_sd(raw, value, actions, old_logp, old_mu, old_sigma, advantages, returns, target_values,
                      log_std, clip_param, value_loss_coef, entropy_coef, use_clipped_value_loss):
    return FusedPPOLossSD.apply(raw, value, actions, old_logp, old_mu, old_sigma, advantages, returns, target_values,
                                log_std, clip_param, value_loss_coef, entropy_coef, use_clipped_value_loss)


def colsum(x):
    """Sum over dim 0 of a CUDA fp32 matrix [rows, cols] through grx_ppo_colsum (deterministic; HIP-graph safe)."""
    lib = load_ppo_library()
    x = _f32c(x)
    rows, cols = x.shape
    out = torch.empty(cols, device=x.device, dtype=torch.float32)
    partials = torch.empty(lib.grx_ppo_colsum_partials_size(rows, cols), device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        rc = lib.grx_ppo_colsum(rows, cols, x.data_ptr(), out.data_ptr(), partials.data_ptr(),
                                C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream))
    if rc != 0:
        raise RuntimeError(f"grx_ppo_colsum failed ({rc}): {rows} x {cols}")
    return out


def elu_backward_colsum(dy, y):
    """(dz, db): dz = dy * ELU'(y) from the layer's output y, db = dz.sum(0) -- one pass (grx_ppo_elu_backward_colsum)"""
    lib = load_ppo_library()
    dy, y = _f32c(dy), _f32c(y)
    rows, cols = dy.shape
    dz = torch.empty_like(dy)
    out = torch.empty(cols, device=dy.device, dtype=torch.float32)
    partials = torch.empty(lib.grx_ppo_colsum_partials_size(rows, cols), device=dy.device, dtype=torch.float32)
    with torch.cuda.device(dy.device):
        rc = lib.grx_ppo_elu_backward_colsum(rows, cols, dy.data_ptr(), y.data_ptr(), dz.data_ptr(), out.data_ptr(), partials.data_ptr(),
                                             C.c_void_p(torch.cuda.current_stream(dy.device).cuda_stream))
    if rc != 0:
        raise RuntimeError(f"grx_ppo_elu_backward_colsum failed ({rc}): {rows} x {cols}")
    return dz, out


def store_transition(storage, step, obs, pri, actions, mu, sigma, values, logp, rewards, dones, time_outs, gamma, log=None):
    """One rollout step's bookkeeping through grx_ppo_store_transition (include/grx_ppo.h): the storage rows of `step`,
    the time-out bootstrap, and -- log = (cur_rew, cur_len, done_rew_row, done_len_row) -- the runner's episode sums."""
    lib = load_ppo_library()
    N = storage.num_envs
    ptr = lambda t: t.data_ptr() if t is not None else None
    for t in (obs, pri, actions, mu, sigma, values, logp, rewards):
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise RuntimeError("store_transition needs contiguous float32 CUDA tensors")
    def as_u8(t):   # the kernel reads one byte per env: bool is reinterpreted, any other dtype (a reference-style long reset_buf) converted
        if t.dtype == torch.bool:
            t = t.view(torch.uint8)
        elif t.dtype != torch.uint8:
            t = (t != 0).to(torch.uint8)
        if not (t.is_cuda and t.is_contiguous() and t.numel() == N):
            raise RuntimeError("store_transition needs contiguous CUDA dones / time_outs with one entry per env")
        return t
    d8 = as_u8(dones)
    t8 = None if time_outs is None else as_u8(time_outs)
    sp = storage.pri_observations
    lg = log if log is not None else (None, None, None, None)
    with torch.cuda.device(obs.device):
        rc = lib.grx_ppo_store_transition(
            N, obs.shape[1], pri.shape[1] if (pri is not None and sp is not None) else 0, actions.shape[1],
            ptr(obs), ptr(pri) if sp is not None else None, ptr(actions), ptr(mu), ptr(sigma), ptr(values), ptr(logp), ptr(rewards), ptr(d8), ptr(t8),
            float(gamma), ptr(storage.observations[step]), ptr(sp[step]) if sp is not None else None, ptr(storage.actions[step]), ptr(storage.mu[step]),
            ptr(storage.sigma[step]), ptr(storage.values[step]), ptr(storage.actions_log_prob[step]), ptr(storage.rewards[step]), ptr(storage.dones[step]),
            ptr(lg[0]), ptr(lg[1]), ptr(lg[2]), ptr(lg[3]), C.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream))
    if rc != 0:
        raise RuntimeError(f"grx_ppo_store_transition failed ({rc})")


def _linears_of(mlp):
    """(weight, bias) of every nn.Linear of an rl.modules.MLP if it is Linear -> ELU(1) -> ... -> Linear, else None."""
    mods = list(mlp.model)
    lin = []
    for i, m in enumerate(mods):
        if i % 2 == 0:
            if not isinstance(m, torch.nn.Linear):
                return None
            lin.append((m.weight, m.bias))
        elif not (isinstance(m, torch.nn.ELU) and m.alpha == 1.0):
            return None
    return lin if len(mods) % 2 == 1 else None


LN_MAX_COLS = 1024   # include/grx_ppo_ln.h GRX_LN_MAX_COLS


def ln_fused():
    """False under GRX_LN_FUSED=0: a LayerNorm hidden layer runs its torch spelling (rl/modules.py _TrainLinearLNELU), nothing of it is fused"""
    return os.environ.get("GRX_LN_FUSED", "1") != "0"


def _layers_of(mlp):
    """(weight, bias, norm) of every nn.Linear of an rl.modules.MLP -- norm the nn.LayerNorm behind a hidden layer, or None -- if it is
    Linear -> [LayerNorm ->] ELU(1) -> ... -> Linear, else None.  (_linears_of keeps refusing a LayerNorm network: bf16, the gradient
    penalty and the estimator's fused forward do not cover it.)"""
    mods = list(mlp.model)
    layers, i = [], 0
    while i < len(mods):
        m = mods[i]
        if not isinstance(m, torch.nn.Linear):
            return None
        if i + 1 == len(mods):
            layers.append((m.weight, m.bias, None))
            return layers
        norm = None
        if isinstance(mods[i + 1], torch.nn.LayerNorm):
            norm = mods[i + 1]
            if not (norm.elementwise_affine and norm.bias is not None and tuple(norm.normalized_shape) == (m.out_features,)
                    and m.out_features <= LN_MAX_COLS):
                return None
            i += 1
        if not (i + 1 < len(mods) and isinstance(mods[i + 1], torch.nn.ELU) and mods[i + 1].alpha == 1.0):
            return None
        layers.append((m.weight, m.bias, norm))
        i += 2
    return None   # (no output layer behind the last activation)


def mlp_can_fuse(mlp, x):
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2):
        return False
    layers = _layers_of(mlp)
    return layers is not None and (ln_fused() or all(n is None for _, _, n in layers))


def ln_elu_forward(z, gamma, beta, eps, stats=True):
    """(y, mean, rstd) = ELU(LayerNorm(z)) per row through grx_ln_elu_forward (one launch); stats=False (inference): (y, None, None)"""
    lib = load_ppo_library()
    z = _f32c(z)
    rows, cols = z.shape
    y = torch.empty_like(z)
    mean, rstd = (torch.empty(rows, device=z.device, dtype=torch.float32) for _ in range(2)) if stats else (None, None)
    with torch.cuda.device(z.device):
        rc = lib.grx_ln_elu_forward(rows, cols, z.data_ptr(), _f32c(gamma).data_ptr(), _f32c(beta).data_ptr(), float(eps), y.data_ptr(),
                                    mean.data_ptr() if stats else None, rstd.data_ptr() if stats else None,
                                    C.c_void_p(torch.cuda.current_stream(z.device).cuda_stream))
    if rc != 0:
        raise RuntimeError(f"grx_ln_elu_forward failed ({rc}): {rows} x {cols}")
    return y, mean, rstd


def ln_elu_backward(dy, y, z, mean, rstd, gamma):
    """(dz, dgamma, dbeta, dbias) of ELU(LayerNorm(z)) through grx_ln_elu_backward: three launches, the column sums in grx_ppo_colsum's order"""
    lib = load_ppo_library()
    dy, y, z, gamma = _f32c(dy), _f32c(y), _f32c(z), _f32c(gamma)
    rows, cols = dy.shape
    dz = torch.empty_like(dy)
    dgamma, dbeta, dbias = (torch.empty(cols, device=dy.device, dtype=torch.float32) for _ in range(3))
    partials = torch.empty(max(1, lib.grx_ln_elu_backward_partials_size(rows, cols)), device=dy.device, dtype=torch.float32)
    with torch.cuda.device(dy.device):
        rc = lib.grx_ln_elu_backward(rows, cols, dy.data_ptr(), y.data_ptr(), z.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
                                     dz.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), dbias.data_ptr(), partials.data_ptr(),
                                     C.c_void_p(torch.cuda.current_stream(dy.device).cuda_stream))
    if rc != 0:
        raise RuntimeError(f"grx_ln_elu_backward failed ({rc}): {rows} x {cols}")
    return dz, dgamma, dbeta, dbias


def _layer(lib, x, w, b, elu, stream, bf16=False):
    y = torch.empty(x.shape[0], w.shape[0], device=x.device, dtype=torch.float32)
    fn = lib.grx_mlp_layer_bf16 if bf16 else lib.grx_mlp_layer
    rc = fn(x.shape[0], x.shape[1], w.shape[0], x.data_ptr(), w.data_ptr(), b.data_ptr() if b is not None else None, y.data_ptr(), int(elu), stream)
    if rc:
        raise RuntimeError(f"{'grx_mlp_layer_bf16' if bf16 else 'grx_mlp_layer'} failed ({rc}): {tuple(x.shape)} x {tuple(w.shape)}")
    return y


def _hidden(lib, x, w, b, norm, stream, bf16=False):
    """one hidden layer of the inference forward: the product with bias + ELU in its epilogue, or -- norm, an nn.LayerNorm -- the bare
    product and grx_ln_elu_forward behind it (no mean / rstd outputs)"""
    if norm is None:
        return _layer(lib, x, w, b, True, stream, bf16)
    z = _layer(lib, x, w, b, False, stream)
    y = torch.empty_like(z)
    rc = lib.grx_ln_elu_forward(z.shape[0], z.shape[1], z.data_ptr(), _f32c(norm.weight).data_ptr(), _f32c(norm.bias).data_ptr(), float(norm.eps),
                                y.data_ptr(), None, None, stream)
    if rc:
        raise RuntimeError(f"grx_ln_elu_forward failed ({rc}): {tuple(z.shape)}")
    return y


def _bf16_hidden(mlp):
    """True when an rl.modules.MLP multiplies its hidden layers in bf16 (MLP.set_precision)"""
    return getattr(mlp, "precision", "fp32") == "bf16"


def linear_elu(x, weight, bias, bf16=False):
    """ELU(x W^T + b) through grx_mlp_layer, or grx_mlp_layer_bf16 with bf16 operands (one launch)"""
    lib = load_ppo_library()
    with torch.cuda.device(x.device):
        return _layer(lib, _f32c(x), _f32c(weight), bias, True, torch.cuda.current_stream(x.device).cuda_stream, bf16)


def input_grad_bf16(dz, weight):
    """dX = bf16(dZ) . bf16(W) through grx_mlp_input_grad_bf16: dz [M, N], weight [N, K] -> [M, K] (fp32)"""
    lib = load_ppo_library()
    dz, weight = _f32c(dz), _f32c(weight)
    (M, N), K = dz.shape, weight.shape[1]
    dx = torch.empty(M, K, device=dz.device, dtype=torch.float32)
    with torch.cuda.device(dz.device):
        rc = lib.grx_mlp_input_grad_bf16(M, N, K, dz.data_ptr(), weight.data_ptr(), dx.data_ptr(),
                                         C.c_void_p(torch.cuda.current_stream(dz.device).cuda_stream))
    if rc:
        raise RuntimeError(f"grx_mlp_input_grad_bf16 failed ({rc}): {M} x {N} x {K}")
    return dx


def weight_grad_bf16(dz, x):
    """dW = bf16(dZ)^T . bf16(X) through grx_mlp_weight_grad_bf16 (batch slabs added in a fixed order): dz [M, N], x [M, K] -> [N, K]"""
    lib = load_ppo_library()
    dz, x = _f32c(dz), _f32c(x)
    (M, N), K = dz.shape, x.shape[1]
    dw = torch.empty(N, K, device=dz.device, dtype=torch.float32)
    partials = torch.empty(max(1, lib.grx_mlp_weight_grad_bf16_partials_size(M, N, K)), device=dz.device, dtype=torch.float32)
    with torch.cuda.device(dz.device):
        rc = lib.grx_mlp_weight_grad_bf16(M, N, K, dz.data_ptr(), x.data_ptr(), dw.data_ptr(), partials.data_ptr(),
                                          C.c_void_p(torch.cuda.current_stream(dz.device).cuda_stream))
    if rc:
        raise RuntimeError(f"grx_mlp_weight_grad_bf16 failed ({rc}): {M} x {N} x {K}")
    return dw


def mlp_forward(mlp, x):
    """Inference forward of an rl.modules.MLP through libgrx_ppo.so: one MFMA launch per layer (bias + ELU in the epilogue); the
    hidden layers with bf16 operands when the MLP is set to bf16 (the output layer stays fp32)."""
    lib = load_ppo_library()
    lin = _layers_of(mlp)
    bf16 = _bf16_hidden(mlp)
    x = _f32c(x)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    with torch.cuda.device(x.device):
        for w, b, norm in lin[:-1]:
            x = _hidden(lib, x, w, b, norm, stream, bf16)
        w, b, _ = lin[-1]
        x = _layer(lib, x, w, b, False, stream)
    return x


def policy_act(mlp, std, x, eps, state_dependent=None):
    """actor forward + sample + log-prob: (actions, logp [M], mu, sigma) -- the hidden layers as in mlp_forward, the output
    layer fused with `mu + std * eps` and Normal.log_prob summed over the actions.  state_dependent "scalar" / "log": the output
    layer is [mean | s] (2A rows) and sigma = s or exp(s) per row (grx_mlp_policy_head_sd, still one launch); `std` is not read."""
    lib = load_ppo_library()
    lin = _layers_of(mlp)
    bf16 = _bf16_hidden(mlp)
    x = _f32c(x)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    with torch.cuda.device(x.device):
        for w, b, norm in lin[:-1]:
            x = _hidden(lib, x, w, b, norm, stream, bf16)
        w, b, _ = lin[-1]
        M, A = x.shape[0], w.shape[0] // (2 if state_dependent is not None else 1)
        actions, mu, sigma = (torch.empty(M, A, device=x.device, dtype=torch.float32) for _ in range(3))
        logp = torch.empty(M, device=x.device, dtype=torch.float32)
        if state_dependent is not None:
            rc = lib.grx_mlp_policy_head_sd(M, x.shape[1], A, x.data_ptr(), _f32c(w).data_ptr(), b.data_ptr() if b is not None else None,
                                            int(state_dependent == "log"), _f32c(eps).data_ptr(), actions.data_ptr(), logp.data_ptr(),
                                            mu.data_ptr(), sigma.data_ptr(), stream)
            if rc:
                raise RuntimeError(f"grx_mlp_policy_head_sd failed ({rc})")
            return actions, logp, mu, sigma
        rc = lib.grx_mlp_policy_head(M, x.shape[1], A, x.data_ptr(), w.data_ptr(), b.data_ptr() if b is not None else None,
                                     _f32c(std).data_ptr(), _f32c(eps).data_ptr(), actions.data_ptr(), logp.data_ptr(),
                                     mu.data_ptr(), sigma.data_ptr(), stream)
        if rc:
            raise RuntimeError(f"grx_mlp_policy_head failed ({rc})")
    return actions, logp, mu, sigma


class RowGather:
    """dst[t] = src[t][idx] for a fixed set of (src, dst) pairs in one launch (grx_ppo_gather_rows): the pointer tables are
    built once, a call passes the index slice."""

    def __init__(self, srcs, dsts):
        self.lib = load_ppo_library()
        n = len(srcs)
        assert n == len(dsts) and all(s.dtype == torch.float32 and s.is_contiguous() and d.is_contiguous() and d.dtype == torch.float32
                                      and s.shape[1:] == d.shape[1:] for s, d in zip(srcs, dsts))
        self.n, self.mb, self.device = n, dsts[0].shape[0], srcs[0].device
        self.src = (C.c_void_p * n)(*[s.data_ptr() for s in srcs])
        self.dst = (C.c_void_p * n)(*[d.data_ptr() for d in dsts])
        self.w = (C.c_int * n)(*[int(s[0].numel()) for s in srcs])
        self.keep = (srcs, dsts)

    def __call__(self, idx):
        assert idx.dtype == torch.int64 and idx.is_contiguous() and idx.numel() == self.mb
        with torch.cuda.device(self.device):
            rc = self.lib.grx_ppo_gather_rows(self.n, self.src, self.dst, self.w, idx.data_ptr(), self.mb,
                                              torch.cuda.current_stream(self.device).cuda_stream)
        if rc:
            raise RuntimeError(f"grx_ppo_gather_rows failed ({rc})")


class SymGather:
    """RowGather with the minibatch's mirror image behind it (grx_sym_gather_rows, rl/symmetry.py): dst[t][:mb] = src[t][idx] and
    dst[t][mb:] = that again (modes[t] == 1), its mirror image under maps[t] (2) or nothing (0: dst[t] has mb rows), for a fixed set of
    (src, dst) pairs in one launch.  The pointer tables are built once: the maps' tensors are rewritten in place, never replaced.
    idx None: row r itself (the stand-alone "mirror these rows" call)."""

    def __init__(self, srcs, dsts, modes, maps):
        self.lib = load_ppo_library()
        n = len(srcs)
        assert n == len(dsts) == len(modes) == len(maps)
        rows = [d.shape[0] // (2 if m else 1) for d, m in zip(dsts, modes)]
        assert all(s.dtype == torch.float32 and s.is_contiguous() and d.is_contiguous() and d.dtype == torch.float32 and s.shape[1:] == d.shape[1:]
                   and d.shape[0] == r * (2 if m else 1) and r == rows[0] for s, d, m, r in zip(srcs, dsts, modes, rows))
        self.n, self.mb, self.device = n, rows[0], srcs[0].device
        self.src = (C.c_void_p * n)(*[s.data_ptr() for s in srcs])
        self.dst = (C.c_void_p * n)(*[d.data_ptr() for d in dsts])
        self.w = (C.c_int * n)(*[int(s[0].numel()) for s in srcs])
        self.modes = (C.c_int * n)(*[int(m) for m in modes])
        for m, mp, w in zip(modes, maps, self.w):
            assert m != 2 or (mp is not None and mp.width == w and mp.perm.dtype == torch.int32 and mp.perm.is_contiguous()
                              and mp.scale.dtype == torch.float32 and mp.scale.is_contiguous()
                              and (mp.offset is None or (mp.offset.dtype == torch.float32 and mp.offset.is_contiguous())))
        ptr = lambda t: t.data_ptr() if t is not None else None
        self.perm = (C.c_void_p * n)(*[ptr(mp.perm) if m == 2 else None for m, mp in zip(modes, maps)])
        self.scale = (C.c_void_p * n)(*[ptr(mp.scale) if m == 2 else None for m, mp in zip(modes, maps)])
        self.offset = (C.c_void_p * n)(*[ptr(mp.offset) if m == 2 else None for m, mp in zip(modes, maps)])
        self.keep = (srcs, dsts, maps)

    def __call__(self, idx=None):
        assert idx is None or (idx.dtype == torch.int64 and idx.is_contiguous() and idx.numel() == self.mb)
        with torch.cuda.device(self.device):
            rc = self.lib.grx_sym_gather_rows(self.n, self.src, self.dst, self.w, self.modes, self.perm, self.scale, self.offset,
                                              idx.data_ptr() if idx is not None else None, self.mb,
                                              torch.cuda.current_stream(self.device).cuda_stream)
        if rc:
            raise RuntimeError(f"grx_sym_gather_rows failed ({rc})")


class MirrorRows:
    """x [rows, W] -> mirror(x) under one map, through grx_sym_gather_rows without an index (the stand-alone "mirror these rows" call): the
    output buffer and the pointer tables are built once, a call sets the source pointer.  The entry point's contract writes the rows
    themselves in front of their mirror image; what is handed out is the second half.  The result is overwritten by the next call."""

    def __init__(self, rows, m, device):
        self.lib = load_ppo_library()
        assert m.perm.dtype == torch.int32 and m.perm.is_contiguous() and m.scale.dtype == torch.float32 and m.scale.is_contiguous()
        self.rows, self.map, self.device = int(rows), m, device
        self.dst = torch.empty(2 * self.rows, m.width, device=device)
        self.src = (C.c_void_p * 1)(None)
        self.dstp = (C.c_void_p * 1)(self.dst.data_ptr())
        self.w, self.modes = (C.c_int * 1)(m.width), (C.c_int * 1)(2)
        self.perm, self.scale = (C.c_void_p * 1)(m.perm.data_ptr()), (C.c_void_p * 1)(m.scale.data_ptr())
        self.offset = (C.c_void_p * 1)(m.offset.data_ptr() if m.offset is not None else None)

    def __call__(self, x):
        assert x.dtype == torch.float32 and x.is_contiguous() and tuple(x.shape) == (self.rows, self.map.width) and x.device == self.dst.device
        self.src[0] = x.data_ptr()
        with torch.cuda.device(self.device):
            rc = self.lib.grx_sym_gather_rows(1, self.src, self.dstp, self.w, self.modes, self.perm, self.scale, self.offset, None, self.rows,
                                              torch.cuda.current_stream(self.device).cuda_stream)
        if rc:
            raise RuntimeError(f"grx_sym_gather_rows failed ({rc})")
        return self.dst[self.rows:]
