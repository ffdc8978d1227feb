"""Actor-critic MLP policy with the semantics of rsl_rl's ActorCriticMLP (reference:
rsl_rl/modules/actor_critic_mlp.py:10-231, mlp.py:7-42): separate actor / critic MLPs with ELU
(or the named activation) between hidden layers and a linear output, one learnable std per action,
``Normal(mean, mean*0 + std)``, log-prob / entropy summed over actions, default PyTorch init.

State-dict layout (``actor.model.<i>.weight`` ..., ``critic.model.<i>...``, ``std``) equals the
reference's so checkpoints (``model_<it>.pt``) interchange; ``load_state_dict`` reproduces the
reference quirk of overwriting ``std`` with ``set_noise_std`` unless ``set_std=False``
(actor_critic_mlp.py:116-134).  Opt-in: ``noise_std_type="log"`` holds ``log_std`` instead of ``std``,
``state_dependent_std=True`` no noise parameter at all -- the actor's output layer is ``[mean | s]``."""
import torch
import torch.nn as nn
from torch.distributions import Normal

PRECISIONS = ("fp32", "bf16")   # PPO(precision=...): the hidden layers' matrix products
_ACTIVATIONS = {"elu": nn.ELU, "selu": nn.SELU, "relu": nn.ReLU, "crelu": nn.ReLU, "lrelu": nn.LeakyReLU,
                "tanh": nn.Tanh, "sigmoid": nn.Sigmoid}


def get_activation(name):
    """rsl_rl/utils/utils.py:231-254"""
    if name not in _ACTIVATIONS:
        print("invalid activation function!")
        return None
    return _ACTIVATIONS[name]()


import os

_FUSED_ELU_FORWARD = os.environ.get("GRX_PPO_FUSED_FWD", "1") != "0"   # ... and their forward through grx_mlp_layer (bias + ELU epilogue)
_FUSED_ELU_BACKWARD = os.environ.get("GRX_PPO_FUSED_ELU", "1") != "0"   # hidden layers: ELU backward + bias gradient in one pass (_TrainLinearELU)
_TRAIN_LINEAR = os.environ.get("GRX_PPO_LINEAR", "colsum")   # "torch": plain nn.Linear autograd on a HIP device too


class _TrainLinear(torch.autograd.Function):
    """nn.Linear as PPO trains it on a HIP device: y = x W^T + b, with two departures from torch's autograd formula.

    * The bias gradient is libgrx_ppo.so's deterministic column sum (`fused_loss.colsum`), not torch's column reduction:
      replayed from a captured HIP graph with other GPU work between replays, at::native's reduce kernel returned garbage
      for one [10485, 128] -> [128] case (the critic's last hidden bias) while every other tensor matched an fp64
      reference to 1e-7 (tools/gpu_ppo_graph_check.py).  With this function the captured step and the eager step agree
      bit for bit, rollouts in between included.
    * A one-column layer (the value head) pins its three GEMV-shaped products to hipBLASLt: PPO prefers rocBLAS for the
      duration of update() (2x faster weight-gradient GEMMs at these shapes), but rocBLAS's pick for [1, B] x [B, H]
      takes 570 us at B = 10^4 against hipBLASLt's 32 us (tools/gpu_gemm_probe.py).  torch's BLAS preference is a
      process-global flag read at call time, so it is flipped around those products only."""

    @staticmethod
    def _blas(pin):
        prev = torch.backends.cuda.preferred_blas_library()
        if pin:
            torch.backends.cuda.preferred_blas_library("cublaslt")
        return prev

    @staticmethod
    def forward(ctx, x, weight, bias):
        prev = _TrainLinear._blas(weight.shape[0] == 1)
        try:
            y = torch.addmm(bias, x, weight.t())
        finally:
            torch.backends.cuda.preferred_blas_library(prev)
        ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    def backward(ctx, dy):
        from .fused_loss import colsum
        x, weight = ctx.saved_tensors
        prev = _TrainLinear._blas(weight.shape[0] == 1)
        try:
            dx = dy @ weight if ctx.needs_input_grad[0] else None   # (the first layer's input is data: no dX product)
            return dx, dy.t() @ x, colsum(dy)
        finally:
            torch.backends.cuda.preferred_blas_library(prev)


class _TrainLinearELU(torch.autograd.Function):
    """ELU(x W^T + b) of a hidden layer as PPO trains it on a HIP device: _TrainLinear's products, with the ELU's backward and the
    bias gradient in ONE pass over dY (fused_loss.elu_backward_colsum: dZ = dY * ELU'(Y) from the saved OUTPUT, column sums of dZ)
    instead of an elu_backward launch followed by the column sum.

    bf16=True (MLP.set_precision("bf16")): the three products -- Y, dX, dW -- run on libgrx_ppo.so's bf16 kernels, which round
    both operands to bf16 as they load them and accumulate in fp32.  The bias gradient, the ELU backward and every tensor in
    memory stay fp32."""

    @staticmethod
    def forward(ctx, x, weight, bias, bf16):
        ctx.bf16 = bf16
        if bf16:
            from .fused_loss import linear_elu
            y = linear_elu(x, weight, bias, bf16=True)
        elif _FUSED_ELU_FORWARD and x.is_contiguous() and weight.is_contiguous():
            from .fused_loss import linear_elu
            y = linear_elu(x, weight, bias)   # libgrx_ppo.so: f32 MFMA, bias + ELU in the epilogue (one launch)
        else:
            prev = _TrainLinear._blas(weight.shape[0] == 1)
            try:
                y = torch.nn.functional.elu(torch.addmm(bias, x, weight.t()))
            finally:
                torch.backends.cuda.preferred_blas_library(prev)
        ctx.save_for_backward(x, weight, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        from .fused_loss import elu_backward_colsum
        x, weight, y = ctx.saved_tensors
        dz, db = elu_backward_colsum(dy, y)
        if ctx.bf16:
            from .fused_loss import input_grad_bf16, weight_grad_bf16
            dx = input_grad_bf16(dz, weight) if ctx.needs_input_grad[0] else None   # (the first layer's input is data: no dX product)
            return dx, weight_grad_bf16(dz, x), db, None
        prev = _TrainLinear._blas(weight.shape[0] == 1)
        try:
            dx = dz @ weight if ctx.needs_input_grad[0] else None   # (the first layer's input is data: no dX product)
            return dx, dz.t() @ x, db, None
        finally:
            torch.backends.cuda.preferred_blas_library(prev)


def ln_elu_torch(x, weight, bias, gamma, beta, eps):
    """the torch spelling of a LayerNorm hidden layer's forward: ELU(LayerNorm(x W^T + b)) and the product z it normalises"""
    z = torch.addmm(bias, x, weight.t())
    return torch.nn.functional.elu(torch.nn.functional.layer_norm(z, (z.shape[-1],), gamma, beta, eps)), z


def ln_elu_backward_torch(dy, y, z, gamma, eps):
    """the torch spelling of include/grx_ppo_ln.h's backward formulas: (dz, dgamma, dbeta, dbias), the three batch sums by torch's own
    column reduction (which is why this spelling is not captured)"""
    m = z.mean(-1, keepdim=True)
    d = z - m
    s = 1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + eps)
    xh = d * s
    g = dy * torch.where(y > 0, torch.ones_like(y), y + 1.0)
    q = g * gamma
    c1, c2 = q.mean(-1, keepdim=True), (q * xh).mean(-1, keepdim=True)
    dz = s * ((q - c1) - xh * c2)
    return dz, (g * xh).sum(0), g.sum(0), dz.sum(0)


class _TrainLinearLNELU(torch.autograd.Function):
    """ELU(LayerNorm(x W^T + b)) of a hidden layer of MLP(layer_norm=True) as PPO trains it.  On a HIP device: the product
    through grx_mlp_layer without its ELU epilogue, then grx_ln_elu_forward (y, and the rows' mean and 1 / std for the backward);
    grx_ln_elu_backward gives dz -- the gradient arriving at the product -- and the three batch sums dgamma, dbeta and the Linear's bias
    gradient in grx_ppo_colsum's order, so no torch column reduction enters the captured step; dX and dW are _TrainLinear's products.
    GRX_LN_FUSED=0 on a HIP device, and the function applied to CPU tensors: the torch spelling of the same formulas (ln_elu_torch,
    ln_elu_backward_torch; not captured).  (MLP.forward itself sends CPU tensors through the plain modules under torch's autograd.)"""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, eps):
        from .fused_loss import ln_fused
        ctx.eps, ctx.fused = float(eps), bool(x.is_cuda and ln_fused())
        if ctx.fused:
            from .fused_loss import _f32c, _layer, ln_elu_forward, load_ppo_library
            with torch.cuda.device(x.device):
                z = _layer(load_ppo_library(), _f32c(x), _f32c(weight), bias, False, torch.cuda.current_stream(x.device).cuda_stream)
            y, mean, rstd = ln_elu_forward(z, gamma, beta, ctx.eps)
            ctx.save_for_backward(x, weight, gamma, z, y, mean, rstd)
            return y
        prev = _TrainLinear._blas(x.is_cuda and weight.shape[0] == 1)
        try:
            y, z = ln_elu_torch(x, weight, bias, gamma, beta, ctx.eps)
        finally:
            torch.backends.cuda.preferred_blas_library(prev)
        ctx.save_for_backward(x, weight, gamma, z, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        if ctx.fused:
            from .fused_loss import ln_elu_backward
            x, weight, gamma, z, y, mean, rstd = ctx.saved_tensors
            dz, dgamma, dbeta, db = ln_elu_backward(dy, y, z, mean, rstd, gamma)
        else:
            x, weight, gamma, z, y = ctx.saved_tensors
            dz, dgamma, dbeta, db = ln_elu_backward_torch(dy, y, z, gamma, ctx.eps)
        prev = _TrainLinear._blas(x.is_cuda and weight.shape[0] == 1)   # (a one-column layer: _TrainLinear's hipBLASLt pin)
        try:
            dx = dz @ weight if ctx.needs_input_grad[0] else None   # (the first layer's input is data: no dX product)
            return dx, dz.t() @ x, db, dgamma, dbeta, None
        finally:
            torch.backends.cuda.preferred_blas_library(prev)


class MLP(nn.Module):
    def __init__(self, input_size, output_size, hidden_dims=(256, 256, 256), activation="relu", layer_norm=False, layer_norm_eps=1e-5, **_):
        super().__init__()
        self.input_size, self.output_size, self.hidden_dims = input_size, output_size, list(hidden_dims)
        # layer_norm: every hidden layer is Linear -> LayerNorm -> ELU, the output layer stays a bare Linear
        self.layer_norm, self.layer_norm_eps = bool(layer_norm), float(layer_norm_eps)
        if self.layer_norm and activation != "elu":
            raise ValueError(f"MLP: layer_norm=True needs activation='elu' (the fused LayerNorm + ELU pass), not {activation!r}")
        if self.layer_norm and not self.layer_norm_eps > 0.0:
            raise ValueError(f"MLP: layer_norm_eps must be above 0, not {layer_norm_eps!r}")
        if self.layer_norm and any(not 1 <= int(h) <= 1024 for h in hidden_dims):
            raise ValueError(f"MLP: layer_norm=True covers hidden widths of 1..1024 (include/grx_ppo_ln.h), not {list(hidden_dims)}")
        dims = [input_size] + list(hidden_dims)
        layers = []
        for a, b in zip(dims[:-1], dims[1:]):
            if self.layer_norm:
                layers += [nn.Linear(a, b), nn.LayerNorm(b, eps=self.layer_norm_eps), get_activation(activation)]
            else:
                layers += [nn.Linear(a, b), get_activation(activation)]
        layers.append(nn.Linear(dims[-1], output_size))
        self.model = nn.Sequential(*layers)
        self.precision = "fp32"

    def set_precision(self, precision):
        """"fp32" (default) or "bf16": the hidden layers' products with bf16 operands and fp32 accumulation (libgrx_ppo.so, HIP
        devices only; the output layer, the parameters and every activation stay fp32).  bf16 needs Linear -> ELU(1) hidden layers."""
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {PRECISIONS}, not {precision!r}")
        if precision == "bf16":
            from .fused_loss import _linears_of
            if _linears_of(self) is None:
                raise ValueError("precision='bf16' needs an MLP of Linear -> ELU(alpha=1) hidden layers")
        self.precision = precision

    @torch.jit.unused
    def _forward_bf16(self, x):
        if not (x.is_cuda and x.dtype == torch.float32):
            raise RuntimeError("an MLP set to precision='bf16' runs on a HIP device with fp32 input only (there is no CPU path)")
        if torch.is_grad_enabled():
            return self._forward_train(x, bf16=True)
        from .fused_loss import mlp_forward   # (inference: the kernels the rollout's captured policy step runs)
        return mlp_forward(self, x.reshape(-1, x.shape[-1])).reshape(*x.shape[:-1], self.output_size)

    @torch.jit.unused
    def _forward_train(self, x, bf16=False):
        mods = list(self.model)
        i = 0
        while i < len(mods):
            m = mods[i]
            if isinstance(m, nn.Linear) and i + 2 < len(mods) and isinstance(mods[i + 1], nn.LayerNorm) and isinstance(mods[i + 2], nn.ELU) \
                    and mods[i + 2].alpha == 1.0 and mods[i + 1].elementwise_affine and mods[i + 1].bias is not None:
                x = _TrainLinearLNELU.apply(x, m.weight, m.bias, mods[i + 1].weight, mods[i + 1].bias, mods[i + 1].eps)
                i += 3
                continue
            if isinstance(m, nn.Linear) and i + 1 < len(mods) and isinstance(mods[i + 1], nn.ELU) and mods[i + 1].alpha == 1.0 \
                    and (_FUSED_ELU_BACKWARD or bf16):
                x = _TrainLinearELU.apply(x, m.weight, m.bias, bf16)
                i += 2
                continue
            x = _TrainLinear.apply(x, m.weight, m.bias) if isinstance(m, nn.Linear) else m(x)
            i += 1
        return x

    def forward(self, x):
        if not torch.jit.is_scripting():   # (export_policy_as_jit scripts this module: the plain path)
            if self.precision == "bf16":
                return self._forward_bf16(x)
            if x.is_cuda and torch.is_grad_enabled() and x.dtype == torch.float32 and _TRAIN_LINEAR == "colsum":
                return self._forward_train(x)   # training on a HIP device: see _TrainLinear
        return self.model(x)


NOISE_STD_TYPES = ("scalar", "log")   # ActorCriticMLP(noise_std_type=...): sigma is the parameter, or exp of it


class MeanHead(nn.Module):
    """the first `num_actions` outputs of an actor whose output layer is [mean | s] (state_dependent_std): what inference, play and
    the exported TorchScript module act on"""

    def __init__(self, actor, num_actions: int):
        super().__init__()
        self.actor, self.num_actions = actor, int(num_actions)

    def forward(self, x):
        return torch.narrow(self.actor(x), -1, 0, self.num_actions)


class ActorCriticMLP(nn.Module):
    """Two options for the exploration noise, both off by default:

    * noise_std_type="log" (rsl_rl 2.x): the module holds `log_std` instead of `std`, sigma = exp(log_std) -- it cannot reach zero.
    * state_dependent_std=True (rsl_rl 3.x): no noise parameter; the actor's output layer has 2A outputs [mean | s] and sigma = s
      ("scalar") or exp(s) ("log") per state.  The s rows start at zero weight and a bias of init_noise_std resp. log(init_noise_std + 1e-7).

    `noise_std()` is the differentiable [A] sigma of the first three parametrisations; every reader goes through it."""

    def __init__(self, actor_num_input, critic_num_input, actor_num_output, actor_hidden_dims=(256, 256, 256),
                 critic_hidden_dims=(256, 256, 256), activation="elu", fixed_std=False, init_noise_std=1.0,
                 set_std=True, set_noise_std=1.0, actor_output_activation=None, critic_output_activation=None, actor_output_gain=1.0,
                 noise_std_type="scalar", state_dependent_std=False, layer_norm=False, layer_norm_eps=1e-5, num_critic_outputs=1,
                 action_dist="gaussian", action_bounds=None, **kwargs):
        if kwargs:
            print("ActorCritic.__init__ got unexpected arguments, which will be ignored: " + str(list(kwargs)))
        if noise_std_type not in NOISE_STD_TYPES:
            raise ValueError(f"noise_std_type must be one of {NOISE_STD_TYPES}, not {noise_std_type!r}")
        state_dependent_std = bool(state_dependent_std)
        # action_dist="beta" (rl/beta.py): the output layer is [p | q], the policy a Beta on the action box `action_bounds` =
        # (lo, hi); "gaussian" builds the module exactly as before and imports nothing of rl/beta.py
        if action_dist not in ("gaussian", "beta"):
            raise ValueError(f"action_dist must be 'gaussian' or 'beta', not {action_dist!r}")
        beta_dist = action_dist == "beta"
        if beta_dist:
            if noise_std_type != "scalar":
                raise ValueError(f"--action_dist beta and --noise_std_type {noise_std_type} exclude each other: a Beta policy has no noise parameter")
            if state_dependent_std:
                raise ValueError("--action_dist beta and --state_dependent_std exclude each other: a Beta policy has no sigma to emit")
            if fixed_std:
                raise ValueError("--action_dist beta and fixed_std exclude each other: a Beta policy has no std parameter to fix")
            if actor_output_activation is not None:
                raise ValueError(f"--action_dist beta and actor_output_activation={actor_output_activation!r} exclude each other: the output "
                                 "layer is [p | q], an activation on it is not defined")
            if layer_norm:
                raise ValueError("--action_dist beta and --layer_norm exclude each other: the combination is not pinned")
            if int(num_critic_outputs) != 1:
                raise ValueError("--action_dist beta and --reward_groups exclude each other: the multi-critic loss is a Gaussian policy's")
            if action_bounds is None:
                raise ValueError("action_dist='beta' needs action_bounds=(lo, hi), one value or one per action each (the runner takes them "
                                 "from env.cfg.normalization.clip_actions_min / clip_actions_max, or --action_bounds)")
        if state_dependent_std and actor_output_activation is not None:
            raise ValueError(f"state_dependent_std with actor_output_activation={actor_output_activation!r}: the output layer is [mean | s], "
                             "an activation on it is not defined")
        if state_dependent_std and fixed_std:
            raise ValueError("state_dependent_std with fixed_std: the actor emits its own sigma, there is no parameter to fix")
        super().__init__()
        self.noise_std_type, self.state_dependent_std = noise_std_type, state_dependent_std
        self.num_actor_input, self.num_actor_output = actor_num_input, actor_num_output
        # num_critic_outputs: one value head per reward group of --reward_groups; 1 builds the critic exactly as before
        if int(num_critic_outputs) != num_critic_outputs or not 1 <= int(num_critic_outputs) <= 8:
            raise ValueError(f"num_critic_outputs must be an integer in 1..8, not {num_critic_outputs!r}")
        self.num_critic_input, self.num_critic_output = critic_num_input, int(num_critic_outputs)
        # layer_norm: LayerNorm between every hidden layer's product and its ELU, in actor and critic.  Off: the MLPs are
        # built exactly as before
        self.layer_norm = bool(layer_norm)
        ln = {"layer_norm": True, "layer_norm_eps": layer_norm_eps} if self.layer_norm else {}
        self.action_dist = action_dist
        wide = state_dependent_std or beta_dist   # (a 2A-wide output layer: [mean | s], or [p | q])
        self.actor = MLP(actor_num_input, 2 * actor_num_output if wide else actor_num_output, actor_hidden_dims, activation, **ln)
        self.critic = MLP(critic_num_input, self.num_critic_output, critic_hidden_dims, activation, **ln)
        A = actor_num_output
        init = torch.as_tensor(init_noise_std, dtype=torch.float32) * torch.ones(A)
        last = [m for m in self.actor.model if isinstance(m, nn.Linear)][-1]
        if actor_output_gain != 1.0:   # (not in the reference, whose layers keep PyTorch's default init: 1.0.  The build-defined 32-DOF task starts its
            with torch.no_grad():      #  policy near the zero action -- the PD targets' default pose --: envs/config.py GR1T1FullBodyCfgPPO)
                last.weight[:A].mul_(float(actor_output_gain)); last.bias[:A].mul_(float(actor_output_gain))   # (the mean rows: all of them without state_dependent_std)
        if state_dependent_std:   # rsl_rl 3.x: sigma starts at init_noise_std in every state
            with torch.no_grad():
                last.weight[A:].zero_()
                last.bias[A:].copy_(torch.log(init + 1e-7) if noise_std_type == "log" else init)
        if beta_dist:   # the q rows get the gain too; the biases put the initial policy's mode at the zero action, its spread at init_noise_std
            from .beta import _bounds, init_biases
            lo, hi = _bounds(action_bounds[0], action_bounds[1], A, "action_bounds")
            lo, span = torch.tensor(lo, dtype=torch.float64), torch.tensor(hi, dtype=torch.float64) - torch.tensor(lo, dtype=torch.float64)
            with torch.no_grad():
                if actor_output_gain != 1.0:
                    last.weight[A:].mul_(float(actor_output_gain))
                last.bias.copy_(init_biases(lo.numpy(), span.numpy(), init.double().numpy()))
            # (buffers of the module: they travel in the state dict, and with the mean head into the exported policy)
            self.register_buffer("action_lo", lo.float())
            self.register_buffer("action_span", span.float())
            self._alpha = self._beta = self.unit_actions = None
        self.fixed_std, self.init_noise_std = fixed_std, init_noise_std
        # (a number, as in the reference -- actor_critic_mlp.py -- or one value per action: the 32-DOF task starts its upper-body joints quieter)
        if beta_dist:
            pass   # (no noise parameter)
        elif not state_dependent_std and noise_std_type == "log":
            self.log_std = nn.Parameter(torch.log(init))
        elif not state_dependent_std:
            self.std = nn.Parameter(init.clone())
        # (a scalar or one value per action -- GR1T1FullBodyCfgPPO --: a buffer, so that the fixed_std paths see a tensor on the module's device)
        self.register_buffer("init_std", init.clone(), persistent=False)
        self.set_std, self.set_noise_std = set_std, set_noise_std
        self.distribution = None
        Normal.set_default_validate_args = False

    is_recurrent = False

    def noise_std(self):
        """the [A] sigma as the loss differentiates it: `std`, exp(`log_std`), or the init_noise_std buffer under fixed_std"""
        if self.state_dependent_std:
            raise RuntimeError("state_dependent_std: sigma is a function of the state (the actor's second output half), there is no [A] sigma")
        if self.action_dist == "beta":
            raise RuntimeError("action_dist='beta': the policy has no noise parameter (action_std is the Beta's own spread)")
        if self.fixed_std:
            return self.init_std
        return torch.exp(self.log_std) if self.noise_std_type == "log" else self.std

    def split_raw(self, raw):
        """(mean, sigma) of a state-dependent actor's raw output [..., 2A]"""
        A = self.num_actor_output
        s = raw[..., A:]
        return raw[..., :A], (torch.exp(s) if self.noise_std_type == "log" else s)

    def inference_actor(self):
        """the module whose output is the mean action: `actor`, or its first A outputs under state_dependent_std"""
        if self.action_dist == "beta":   # (the Beta's mean in action units; lo / span travel with the head)
            from .beta import BetaMeanHead
            return BetaMeanHead(self.actor, self.num_actor_output, self.action_lo, self.action_span)
        return MeanHead(self.actor, self.num_actor_output) if self.state_dependent_std else self.actor

    def assign_noise_std(self, std):
        """sigma := std [A] in place, whichever parameter holds it (a distilled student's fixed noise into an ordinary policy)"""
        if self.state_dependent_std or self.action_dist == "beta":
            raise RuntimeError("state_dependent_std / action_dist='beta': there is no noise parameter to set")
        with torch.no_grad():
            if self.noise_std_type == "log":
                self.log_std.copy_(torch.log(std))
            else:
                self.std.copy_(std)

    def load_state_dict(self, state_dict, strict=True):
        state_dict = dict(state_dict)
        if self.state_dependent_std or self.action_dist == "beta":   # (no noise parameter: nothing to overwrite)
            return super().load_state_dict(state_dict, strict)
        if self.noise_std_type == "log":   # (the reference's set_std / set_noise_std overwrite belongs to `std`: a log_std loads as saved)
            if self.fixed_std:
                with torch.no_grad():
                    self.log_std.copy_(torch.log(torch.as_tensor(self.init_noise_std, dtype=torch.float32) * torch.ones_like(self.log_std)))
                self.log_std.requires_grad = False
                state_dict["log_std"] = self.log_std.detach().clone()
            return super().load_state_dict(state_dict, strict)
        if self.set_std:
            state_dict["std"] = torch.ones_like(state_dict["std"]) * self.set_noise_std
        # (the reference rebinds self.std.data here, actor_critic_mlp.py:116-134; copying IN PLACE gives the same values and keeps
        #  the storage the captured act / update graphs and the optimizer state point at)
        if self.fixed_std:
            with torch.no_grad():
                self.std.copy_(torch.as_tensor(self.init_noise_std, dtype=torch.float32) * torch.ones_like(self.std))
            self.std.requires_grad = False
            state_dict["std"] = self.std.detach().clone()
        return super().load_state_dict(state_dict, strict)

    def set_precision(self, precision):
        """the hidden layers of actor and critic in "fp32" or "bf16" (MLP.set_precision; PPO(precision=...) calls this)"""
        self.actor.set_precision(precision)
        self.critic.set_precision(precision)

    def reset(self, dones=None):
        pass

    def forward(self, *a, **k):
        raise NotImplementedError

    @property
    def action_mean(self):
        if self.action_dist == "beta":   # (in action units, for logging)
            from .beta import mean_torch
            return mean_torch(self._alpha, self._beta, self.action_lo, self.action_span)
        return self.distribution.mean

    @property
    def action_std(self):
        if self.action_dist == "beta":   # (likewise)
            from .beta import std_torch
            return std_torch(self._alpha, self._beta, self.action_span)
        return self.distribution.stddev

    @property
    def entropy(self):
        if self.action_dist == "beta":   # (of x, in unit-box coordinates: sum log span is left out, as in the log-probability)
            from .beta import entropy_torch
            return entropy_torch(self._alpha, self._beta)
        return self.distribution.entropy().sum(dim=-1)

    def beta_params(self):
        """(alpha, beta) of the last update_distribution under action_dist='beta'"""
        return self._alpha, self._beta

    def update_distribution(self, observations):
        if self.action_dist == "beta":
            from .beta import params_torch
            self._alpha, self._beta = params_torch(self.actor(observations))
            return
        if self.state_dependent_std:
            mean, std = self.split_raw(self.actor(observations))
            self.distribution = Normal(mean, std)
            return
        mean = self.actor(observations)
        std = self.noise_std().to(mean.device)
        self.distribution = Normal(mean, mean * 0.0 + std)

    def act(self, observations, **_):
        self.update_distribution(observations)
        if self.action_dist == "beta":   # the env's action; `unit_actions` keeps x, which is what the storage and get_actions_log_prob take
            from .beta import sample_torch
            with torch.no_grad():
                self.unit_actions, actions, _ = sample_torch(self._alpha.detach(), self._beta.detach(), self.action_lo, self.action_span)
            return actions
        return self.distribution.sample()

    def get_actions_log_prob(self, actions):
        if self.action_dist == "beta":   # (`actions` in unit-box coordinates: x, not lo + span x)
            from .beta import logp_torch
            return logp_torch(self._alpha, self._beta, actions)
        return self.distribution.log_prob(actions).sum(dim=-1)

    def act_inference(self, observations):
        if self.action_dist == "beta":
            from .beta import mean_torch, params_torch
            return mean_torch(*params_torch(self.actor(observations)), self.action_lo, self.action_span)
        if self.state_dependent_std:
            return self.actor(observations)[..., :self.num_actor_output]
        return self.actor(observations)

    def evaluate(self, critic_observations=None, **_):
        return self.critic(critic_observations)
