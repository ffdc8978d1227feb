"""PPO with rsl_rl semantics (reference: rsl_rl/algorithms/ppo.py:10-333): clipped surrogate, clipped
value loss, entropy bonus, adaptive-KL learning rate (x / 1.5 outside [kl/2, 2 kl], clamped),
NaN-skip, grad-norm clip 1.0, one Adam step per minibatch, time-out bootstrap.

Multi-GPU (the one addition): envs are sharded over ranks, every rank holds a replica of
the 436 885-parameter model.  Per optimizer step ONE flat fp32 bucket (gradients + the minibatch KL
appended as the last element) is all-reduced over RCCL/xGMI and averaged, so every rank takes the
same adaptive-LR decision and the same Adam step: replicas stay bit-identical without broadcasting.
At 1.75 MB the collective is latency-bound; a single fused bucket keeps it at one launch."""
import contextlib
import os

import torch
import torch.distributed as dist
from .fused_loss import fused_ppo_loss, fused_ppo_loss_sd, mlp_can_fuse, mlp_forward, policy_act
import torch.nn as nn
import torch.optim as optim

from .modules import PRECISIONS, ActorCriticMLP  # noqa: F401
from .storage import RolloutStorage


def _collective_path():
    """True when gradients go through the flat bucket + all-reduce: more than one rank, or GRX_PPO_FORCE_BUCKET=1 with
    an initialised process group (lets a single-GPU box exercise the RCCL path: the all-reduce is then an identity)."""
    return _world() > 1 or (os.environ.get("GRX_PPO_FORCE_BUCKET") == "1" and dist.is_available() and dist.is_initialized())


def _capture_mode():
    """With a process group alive, ProcessGroupNCCL's watchdog thread polls its events (hipEventQuery) at any time; under the
    default "global" capture mode that call from ANOTHER thread invalidates a capture in progress and takes the process
    down.  "thread_local" confines the legality check to the capturing thread."""
    return "thread_local" if dist.is_available() and dist.is_initialized() else "global"


def _noise_std(ac):
    """the differentiable [A] sigma of a policy: ActorCriticMLP.noise_std() (`std`, or exp(`log_std`)); a policy class without the accessor holds `std`"""
    return ac.noise_std() if hasattr(ac, "noise_std") else ac.std


def _world():
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


@contextlib.contextmanager
def _graph_capture(graph, stream):
    """torch.cuda.graph(...) with Python's cyclic garbage collector held off for the duration of the capture.  A collection that
    fires inside a capture -- on this thread, or on autograd's worker thread, which runs the Python backward of FusedPPOLoss /
    _TrainLinear -- may finalise an object that owns device memory (an env handle: grx_destroy -> hipFree / hipHostFree, a torch
    tensor's storage, an event): a free is not a capturable operation, the capture is invalidated and the HIP runtime or the
    autograd thread aborts the process.  Seen once in three runs of the full GPU suite in round 4 (129 tests' worth of garbage
    before the capture in test_rccl_bucket_path_matches_reference); a training job that drops an env while the update graph is being
    built would hit the same."""
    import gc
    was_enabled = gc.isenabled()
    gc.collect()
    gc.disable()
    try:
        with torch.cuda.graph(graph, stream=stream, capture_error_mode=_capture_mode()):
            yield
    finally:
        if was_enabled:
            gc.enable()


class PPO:
    def __init__(self, actor_critic=None, num_learning_epochs=1, num_mini_batches=1, clip_param=0.2, gamma=0.998, lam=0.95,
                 value_loss_coef=1.0, entropy_coef=0.0, learning_rate=1e-3, learning_rate_min=1e-5, learning_rate_max=1e-2,
                 weight_decay=0.0, max_grad_norm=1.0, use_clipped_value_loss=True, schedule="fixed", desired_kl=0.01,
                 device="cpu", storage_class="RolloutStorage", precision="fp32", symmetry=None, symmetry_coef=1.0, symmetry_maps=None,
                 smooth=None, smooth_temporal_coef=0.1, smooth_spatial_coef=0.1, smooth_sigma=0.05, value_norm=None, value_norm_eps=1e-5,
                 grad_penalty_coef=None, reward_groups=None, reward_group_weights=None, constraints=None, constraint_tau=0.95,
                 constraint_ramp_its=1000, constraint_reward_clip="zero", **kwargs):
        if kwargs:
            print("PPO.__init__ got unexpected arguments, which will be ignored: " + str(list(kwargs)))
        # precision="bf16": every hidden layer of actor and critic multiplies bf16 operands into fp32 accumulators -- in the rollout's
        # policy step and in every product of the update (rl/modules.py MLP.set_precision).  Output heads, parameters, gradients, Adam
        # state and activations stay fp32.  Not a config key: `--precision` or an assignment to train_cfg.algorithm sets it.
        if precision not in PRECISIONS:
            raise ValueError(f"PPO: precision must be one of {PRECISIONS}, not {precision!r}")
        if precision == "bf16" and torch.device(device).type != "cuda":
            raise ValueError(f"PPO: precision='bf16' runs on a HIP device only, not on {device!r} (there is no CPU path)")
        if precision != "fp32" and not hasattr(actor_critic, "set_precision"):
            raise ValueError(f"PPO: {type(actor_critic).__name__} has no set_precision(): precision={precision!r} is not available")
        self.precision = precision
        self.device = device
        self.desired_kl, self.schedule, self.mean_kl = desired_kl, schedule, 0.0
        self.learning_rate, self.learning_rate_min, self.learning_rate_max = learning_rate, learning_rate_min, learning_rate_max
        self.actor_critic = actor_critic.to(device)
        if precision == "bf16" and getattr(actor_critic, "layer_norm", False):   # (before set_precision's own refusal, which does not name the flag)
            raise ValueError("PPO: --layer_norm and --precision bf16 exclude each other: the bf16 products cover Linear -> ELU hidden layers only")
        if hasattr(self.actor_critic, "set_precision"):
            self.actor_critic.set_precision(precision)
        self.storage_class = storage_class
        self.storage, self.transition = None, None
        # On a HIP device the whole update runs without host synchronisation: the adaptive learning rate lives in a
        # device scalar consumed by the fused Adam kernel, the NaN-skip uses Adam's found_inf hook, and the loss
        # statistics are read back once per update().  (The reference does three .item() per minibatch, ppo.py:264,308-309.)
        self._device_lr = torch.device(device).type == "cuda"
        # ... and, single rank, the whole minibatch step (forward, losses, backward, adaptive LR, clip, fused Adam) is
        # captured ONCE in a HIP graph and replayed 200x per update (GRX_PPO_GRAPH=0: eager).  The captured step equals the
        # eager one bit for bit, rollouts in between included (tests/test_ppo_gpu.py) -- provided no torch column reduction
        # is inside it: see rl/modules.py:_TrainLinear.
        self._use_graph = self._device_lr and os.environ.get("GRX_PPO_GRAPH", "1") not in ("0", "")
        if self._use_graph:
            from . import modules
            if modules._TRAIN_LINEAR != "colsum":   # torch's column reduction goes wrong under graph replay
                print("PPO: GRX_PPO_LINEAR=" + modules._TRAIN_LINEAR + " -> the minibatch step runs eagerly (GRX_PPO_GRAPH=0)")
                self._use_graph = False
        # ... and everything between the networks' outputs and their gradients is one HIP kernel (rl/fused_loss.py)
        self._fused_loss = self._device_lr and os.environ.get("GRX_PPO_FUSED_LOSS", "1") != "0"
        self._fused_store = self._device_lr and os.environ.get("GRX_PPO_FUSED_STORE", "1") != "0"
        # ... and everything behind loss.backward() -- adaptive learning rate, NaN-skip, gradient clip, Adam -- is two launches of
        # libgrx_ppo.so (rl/fused_loss.py StepTail) instead of ~20 small torch kernels on the step's critical path (GRX_PPO_FUSED_TAIL=0: torch)
        self._fused_tail = self._device_lr and os.environ.get("GRX_PPO_FUSED_TAIL", "1") != "0"
        self._tail = None
        self._graph, self._graph_mb, self._static, self._sums, self._restore_opt = None, None, None, None, None
        # ... and so is the rollout's policy step (GRX_PPO_ACT_GRAPH=0: eager)
        self._use_act_graph = self._device_lr and os.environ.get("GRX_PPO_ACT_GRAPH", "1") not in ("0", "")
        self._act_graph, self._act_key, self._act_in, self._act_out = None, None, None, None
        # inside the captured step the critic runs on a second stream (GRX_PPO_TWO_STREAMS=0: one stream); eagerly the extra
        # stream bookkeeping costs more than the overlap gives
        self._two_streams = self._use_graph and os.environ.get("GRX_PPO_TWO_STREAMS", "1") != "0"
        self._aux_stream = None
        # a recurrent policy (rl/recurrent.py): the rollout's policy step and the minibatch step run eagerly, nothing is captured
        self._recurrent = bool(getattr(actor_critic, "is_recurrent", False))
        # a state-dependent action noise (rl/modules.py): the actor's output is [mean | s], the loss and the rollout's head
        # take it in that form (grx_ppo_loss_sd, grx_mlp_policy_head_sd); captured as the default is
        self._state_dependent = bool(getattr(actor_critic, "state_dependent_std", False))
        if self._state_dependent:
            if self._recurrent:
                raise ValueError("PPO: --state_dependent_std and --recurrent exclude each other: a recurrent policy with a state-dependent "
                                 "sigma is not implemented")
            if symmetry is not None:
                raise ValueError("PPO: --state_dependent_std and --symmetry exclude each other: a mirror map of the [mean | s] output is "
                                 "not implemented")
            if _world() > 1:
                raise NotImplementedError("PPO: --state_dependent_std with a world size above 1 is not implemented: it trains in one "
                                          "process only")
        # a Beta action distribution (rl/beta.py): the actor's output is [p | q], the storage holds x in unit-box coordinates
        # and alpha / beta in mu / sigma's rows, the loss is grx_ppo_loss_beta; the minibatch step is captured as the default is, the
        # rollout's policy step runs eagerly (two torch gamma draws).  None of rl/beta.py is imported without it
        self._beta = getattr(actor_critic, "action_dist", "gaussian") == "beta"
        if self._beta:
            self._init_beta(symmetry, smooth, grad_penalty_coef, reward_groups)
        if self._recurrent:
            if _world() > 1:
                raise NotImplementedError("PPO: a recurrent policy trains in one process only")
            self._use_graph = self._use_act_graph = self._two_streams = False
        # layer normalisation in the hidden layers (rl/modules.py MLP(layer_norm=True)): Linear -> LayerNorm -> ELU, trained
        # through _TrainLinearLNELU and captured as the default is.  Not a config key: `--layer_norm` or an assignment to train_cfg.policy sets it
        self._layer_norm = bool(getattr(actor_critic, "layer_norm", False))
        if self._layer_norm:
            self._init_layer_norm(grad_penalty_coef)
        if self._device_lr:
            # rsl_rl's `Normal.set_default_validate_args = False` (actor_critic.py) is an assignment, not a call, so the
            # reference validates (and host-syncs) on every Normal(); here the validation really is off
            torch.distributions.Distribution.set_default_validate_args(False)
            self._lr_t = torch.tensor(float(learning_rate), device=device)
            self.optimizer = optim.Adam(self.actor_critic.parameters(), lr=self._lr_t, weight_decay=weight_decay, fused=True,
                                        capturable=True)
        else:
            self.optimizer = optim.Adam(self.actor_critic.parameters(), lr=learning_rate, weight_decay=weight_decay)
        self.clip_param, self.num_learning_epochs, self.num_mini_batches = clip_param, num_learning_epochs, num_mini_batches
        self.value_loss_coef, self.entropy_coef, self.gamma, self.lam = value_loss_coef, entropy_coef, gamma, lam
        self.max_grad_norm, self.use_clipped_value_loss = max_grad_norm, use_clipped_value_loss
        # left-right symmetry (rl/symmetry.py): "augment" extends every minibatch by its mirror image, "loss" adds
        # symmetry_coef * mse(actor(mirror(obs)), mirror(actor(obs)).detach()), "both" does both.  Not a config key: `--symmetry` /
        # `--symmetry_coef` or an assignment to train_cfg.algorithm sets it; None runs nothing of it
        self.symmetry, self._sym, self.symmetry_coef, self.mean_symmetry_loss = None, None, 0, 0.0
        if symmetry is not None:
            self._init_symmetry(symmetry, symmetry_coef, symmetry_maps)
        # action smoothness (rl/smooth.py): "temporal" adds smooth_temporal_coef * mse(actor(s_t), actor(s_t+1)) over the pairs
        # that are trajectory steps, "spatial" smooth_spatial_coef * mse(actor(s_t), actor(s_t + smooth_sigma * eps)), "both" both: the
        # successor and the perturbed rows ride behind the minibatch's actor input.  Not a config key: `--smooth` / `--smooth_*` or an
        # assignment to train_cfg.algorithm sets it; None runs nothing of it
        self.smooth, self.mean_smooth_temporal, self.mean_smooth_spatial = None, 0.0, 0.0
        if smooth is not None:
            self._init_smooth(smooth, smooth_temporal_coef, smooth_spatial_coef, smooth_sigma)
        # random network distillation (rl/rnd.py): the runner builds it under `--rnd` and assigns it; None runs nothing of it
        self.rnd = None
        # value normalisation (rl/value_norm.py): the critic's output is a normalised value, denormalised wherever the rollout
        # uses it; the statistics follow the rollout's returns once per iteration ("popart": the critic's output layer follows them too).  Not
        # a config key: `--value_norm` or an assignment to train_cfg.algorithm sets it; None imports nothing of it
        self.value_norm = None
        if value_norm is not None:
            self._init_value_norm(value_norm, value_norm_eps)
        # the Lipschitz gradient penalty (rl/grad_penalty.py): grad_penalty_coef * mean_r ||d logp_r / d x_r||^2 joins the loss,
        # its second-order pass written out by hand and sharing the actor's one backward.  Not a config key: `--grad_penalty_coef` or an
        # assignment to train_cfg.algorithm sets it; None imports nothing of it
        self.grad_penalty_coef, self.mean_grad_penalty = None, 0.0
        if grad_penalty_coef is not None:
            self._init_grad_penalty(grad_penalty_coef)
        # multi-critic PPO (rl/multi_critic.py): the critic has a value head per group of reward terms, GAE and the advantage
        # normalisation run per group, the value loss is the sum over the heads.  Not a config key: `--reward_groups` or an assignment to
        # train_cfg.algorithm sets it (the runner parses the spec against the env's active terms); None imports nothing of it
        self.multi_critic = None
        if reward_groups is not None:
            self._init_multi_critic(reward_groups, reward_group_weights)
        # constraints as terminations (rl/constraints.py): a constraint violation becomes a termination probability per
        # (step, env) that scales the stored reward and the discount inside GAE; the update is untouched.  Not a config key: `--constraints`
        # / `--constraint_*` or assignments to train_cfg.algorithm set it; None imports nothing of it
        self.constraints = None
        if constraints is not None:
            self._init_constraints(constraints, constraint_tau, constraint_ramp_its, constraint_reward_clip)
        self.num_updates = 0
        self._params = [p for p in self.actor_critic.parameters() if p.requires_grad]
        n = sum(p.numel() for p in self._params)
        # multi-rank: every .grad is a VIEW into one flat fp32 bucket [grads | minibatch KL | non-finite-loss flag], so the
        # single all-reduce per optimizer step needs no per-parameter copies in either direction
        # (each view starts on a 256-byte boundary like a separately allocated .grad would: torch's multi-tensor kernels pick
        #  their vector width -- and with it the summation order of the gradient norm -- from the pointer alignment)
        n = sum(-(-p.numel() // 64) * 64 for p in self._params)
        self._nflat = n
        self._bucket = torch.zeros(n + 2, device=device) if _collective_path() else None
        self._mid = torch.zeros(2, device=device) if _collective_path() else None   # value / surrogate loss between the two halves
        self._graph_back = None
        if self._bucket is not None:
            self._install_flat_grads()

    def _install_flat_grads(self):
        for p, o in zip(self._params, self._offsets()):
            p.grad = self._bucket[o:o + p.numel()].view_as(p)

    def _init_symmetry(self, symmetry, symmetry_coef, maps):
        from .symmetry import MODES
        if symmetry not in MODES:
            raise ValueError(f"PPO: symmetry must be None or one of {MODES}, not {symmetry!r}")
        if self._recurrent:
            raise ValueError("PPO: --symmetry and --recurrent exclude each other: a mirrored minibatch of a recurrent policy is not implemented")
        if _world() > 1:
            raise NotImplementedError("PPO: --symmetry with a world size above 1 is not implemented: it trains in one process only")
        if maps is None:
            raise ValueError(f"PPO: symmetry={symmetry!r} needs symmetry_maps (rl.symmetry.build_maps(env, ...))")
        ac = self.actor_critic
        if (maps.obs.width, maps.cobs.width, maps.actions.width) != (ac.num_actor_input, ac.num_critic_input, ac.num_actor_output):
            raise ValueError(f"PPO: the symmetry maps are {maps.obs.width} / {maps.cobs.width} / {maps.actions.width} columns wide, the policy's actor "
                             f"input / critic input / actions {ac.num_actor_input} / {ac.num_critic_input} / {ac.num_actor_output}")
        self.symmetry, self._sym = symmetry, maps
        self.symmetry_coef = float(symmetry_coef) if symmetry in ("loss", "both") else 0
        self._sym_sum = torch.zeros(1, device=self.device)     # the update's sum of mirror losses (finite steps), read back once per update
        self._sym_bufs, self._sym_bufs_gather, self._sym_mirror = None, None, None
        # the nine minibatch tensors (obs, cobs, actions, values, advantages, returns, old_logp, old_mu, old_sigma): how each gets its second half
        self._sym_modes = [2, 2, 2, 1, 1, 1, 1, 2, 2] if symmetry in ("augment", "both") else [2, 0, 0, 0, 0, 0, 0, 0, 0]
        self._sym_tensor_maps = [maps.obs, maps.cobs, maps.actions, None, None, None, None, maps.actions, maps.sigma]

    def _init_beta(self, symmetry, smooth, grad_penalty_coef, reward_groups):
        """what --action_dist beta does not combine with in PPO (the runner refuses the rest: it owns those options)"""
        why = "the Beta policy's loss, rollout step and storage cover the plain fp32 MLP policy on the plain minibatch"
        if self._recurrent:
            raise ValueError(f"PPO: --action_dist beta and --recurrent exclude each other: {why}")
        if symmetry is not None:
            raise ValueError("PPO: --action_dist beta and --symmetry exclude each other: a mirror map of the [p | q] output is not implemented")
        if smooth is not None:
            raise ValueError("PPO: --action_dist beta and --smooth exclude each other: a smoothness loss on the [p | q] output is not implemented")
        if grad_penalty_coef is not None:
            raise ValueError(f"PPO: --action_dist beta and --grad_penalty_coef exclude each other: the penalty differentiates a Gaussian's "
                             f"log-probability; {why}")
        if reward_groups is not None:
            raise ValueError("PPO: --action_dist beta and --reward_groups exclude each other: the multi-critic loss is a Gaussian policy's")
        if getattr(self.actor_critic, "layer_norm", False):
            raise ValueError("PPO: --action_dist beta and --layer_norm exclude each other: the combination is not pinned")
        if self.precision == "bf16":
            raise ValueError(f"PPO: --action_dist beta and --precision bf16 exclude each other: {why}")
        if _world() > 1:
            raise NotImplementedError("PPO: --action_dist beta with a world size above 1 is not implemented: it trains in one process only")
        if self.actor_critic.num_actor_output > 32:
            raise ValueError(f"PPO: --action_dist beta covers 1..32 actions (include/grx_ppo_beta.h), not {self.actor_critic.num_actor_output}")
        self._use_act_graph = False   # the rollout's policy step draws from torch's gamma sampler: eager
        from .beta import fused_enabled
        if self._use_graph and not fused_enabled():   # (the torch spelling is not what the captured step is pinned on)
            print("PPO: GRX_BETA_FUSED=0 -> the minibatch step runs eagerly (GRX_PPO_GRAPH=0)")
            self._use_graph = self._two_streams = False

    def _act_beta(self, actor_observations, critic_observations):
        """act() for a Beta policy: (x, values, logp, alpha, beta, a).  On a HIP device the actor's raw output through the inference forward
        (fused_loss.mlp_forward), grx_beta_params, two torch._standard_gamma draws, grx_beta_sample; elsewhere the torch spelling"""
        from . import beta as B
        ac = self.actor_critic
        with torch.no_grad():
            on_hip = actor_observations.is_cuda and not torch.is_grad_enabled()
            fuse = (on_hip and os.environ.get("GRX_PPO_FUSED_MLP", "1") != "0" and mlp_can_fuse(ac.actor, actor_observations)
                    and mlp_can_fuse(ac.critic, critic_observations))
            raw = mlp_forward(ac.actor, actor_observations) if fuse else ac.actor(actor_observations)
            values = mlp_forward(ac.critic, critic_observations) if fuse else ac.evaluate(critic_observations)
            if self.value_norm is not None:   # (the network's output is a normalised value: the storage and GAE work in reward units)
                values = self.value_norm.denormalize(values)
            alpha, beta = B.beta_params(raw) if (raw.is_cuda and B.fused_enabled()) else B.params_torch(raw)
            x, a, logp = B.rollout_sample(alpha, beta, ac.action_lo, ac.action_span)
        return x, values, logp, alpha, beta, a

    def _init_layer_norm(self, grad_penalty_coef):
        if self._recurrent:
            raise ValueError("PPO: --layer_norm and --recurrent exclude each other: the recurrent policy's MLPs have no LayerNorm path")
        if grad_penalty_coef is not None:
            raise ValueError("PPO: --layer_norm and --grad_penalty_coef exclude each other: the penalty's second-order pass covers "
                             "Linear -> ELU hidden layers only")
        if _world() > 1:
            raise NotImplementedError("PPO: --layer_norm with a world size above 1 is not implemented: it trains in one process only")
        from .fused_loss import ln_fused
        if self._use_graph and not ln_fused():   # the torch spelling's batch sums are torch column reductions (rl/modules.py:_TrainLinear)
            print("PPO: GRX_LN_FUSED=0 -> the minibatch step runs eagerly (GRX_PPO_GRAPH=0)")
            self._use_graph = self._two_streams = False

    def _init_value_norm(self, mode, eps):
        if self._recurrent:
            raise ValueError("PPO: --value_norm and --recurrent exclude each other: denormalising a recurrent critic's rollout and bootstrap "
                             "values is not implemented")
        if _world() > 1:
            raise NotImplementedError("PPO: --value_norm with a world size above 1 is not implemented: the return statistics are per process")
        from .value_norm import ValueNormalizer, output_layer
        self.value_norm = ValueNormalizer(mode, eps, self.device)
        if mode == "popart":
            output_layer(self.actor_critic.critic)   # (raises on a critic whose output layer cannot be rescaled)

    def _init_grad_penalty(self, coef):
        from .grad_penalty import check_coef, linears_of
        why = "the penalty's second-order pass covers the plain fp32 MLP actor on one minibatch of stored rows"
        if self._recurrent:
            raise ValueError(f"PPO: --grad_penalty_coef and --recurrent exclude each other: {why}")
        if self.symmetry is not None:
            raise ValueError(f"PPO: --grad_penalty_coef and --symmetry exclude each other: {why}")
        if self.smooth is not None:
            raise ValueError(f"PPO: --grad_penalty_coef and --smooth exclude each other: {why}")
        if self._state_dependent:
            raise ValueError(f"PPO: --grad_penalty_coef and --state_dependent_std exclude each other: {why}, with one sigma per action")
        if self.precision == "bf16":
            raise ValueError(f"PPO: --grad_penalty_coef and --precision bf16 exclude each other: {why}")
        if _world() > 1:
            raise NotImplementedError("PPO: --grad_penalty_coef with a world size above 1 is not implemented: it trains in one process only")
        coef = check_coef(coef)
        linears_of(self.actor_critic.actor)   # (raises on an actor the pass does not cover)
        self.grad_penalty_coef = coef
        self._gp_sum = torch.zeros(1, device=self.device)   # the update's sum of P (finite steps), read back once per update

    def _init_multi_critic(self, groups, weights):
        why = "the per-group critic, GAE and value loss cover the plain fp32 MLP policy on the plain minibatch"
        if self._recurrent:
            raise ValueError(f"PPO: --reward_groups and --recurrent exclude each other: {why}")
        if self.value_norm is not None:
            raise ValueError("PPO: --reward_groups and --value_norm exclude each other: return statistics per value head are not implemented")
        if self.symmetry is not None:
            raise ValueError(f"PPO: --reward_groups and --symmetry exclude each other: {why}")
        if self.smooth is not None:
            raise ValueError(f"PPO: --reward_groups and --smooth exclude each other: {why}")
        if self.grad_penalty_coef is not None:
            raise ValueError(f"PPO: --reward_groups and --grad_penalty_coef exclude each other: {why}")
        if self._state_dependent:
            raise ValueError("PPO: --reward_groups and --state_dependent_std exclude each other: the multi-critic loss takes one sigma per "
                             "action")
        if self._layer_norm:
            raise ValueError(f"PPO: --reward_groups and --layer_norm exclude each other: {why}")
        if self.precision == "bf16":
            raise ValueError(f"PPO: --reward_groups and --precision bf16 exclude each other: {why}")
        if _world() > 1:
            raise NotImplementedError("PPO: --reward_groups with a world size above 1 is not implemented: the advantage statistics are per "
                                      "process")
        from .multi_critic import MultiCritic, fused_enabled
        mc = MultiCritic(groups, weights, self.device)
        heads = getattr(self.actor_critic, "num_critic_output", 1)
        if heads != mc.K:
            raise ValueError(f"PPO: --reward_groups names {mc.K} groups, the critic has {heads} outputs (ActorCriticMLP(num_critic_outputs="
                             f"{mc.K}))")
        self.multi_critic = mc
        if self._use_graph and not fused_enabled():   # (the torch spelling's per-head means are not what the captured step is pinned on)
            print("PPO: GRX_MC_FUSED=0 -> the minibatch step runs eagerly (GRX_PPO_GRAPH=0)")
            self._use_graph = self._two_streams = False

    def _init_constraints(self, spec, tau, ramp_its, reward_clip):
        why = "the combination is not pinned"
        if self._recurrent:
            raise ValueError(f"PPO: --constraints and --recurrent exclude each other: {why}")
        if self.value_norm is not None:
            raise ValueError("PPO: --constraints and --value_norm exclude each other: both replace compute_returns")
        if self.multi_critic is not None:
            raise ValueError("PPO: --constraints and --reward_groups exclude each other: both replace compute_returns")
        if self.symmetry is not None:
            raise ValueError(f"PPO: --constraints and --symmetry exclude each other: {why}")
        if self.smooth is not None:
            raise ValueError(f"PPO: --constraints and --smooth exclude each other: {why}")
        if self.grad_penalty_coef is not None:
            raise ValueError(f"PPO: --constraints and --grad_penalty_coef exclude each other: {why}")
        if self._state_dependent:
            raise ValueError(f"PPO: --constraints and --state_dependent_std exclude each other: {why}")
        if self._layer_norm:
            raise ValueError(f"PPO: --constraints and --layer_norm exclude each other: {why}")
        if self._beta:
            raise ValueError(f"PPO: --constraints and --action_dist beta exclude each other: {why}")
        if self.precision == "bf16":
            raise ValueError(f"PPO: --constraints and --precision bf16 exclude each other: {why}")
        if _world() > 1:
            raise NotImplementedError("PPO: --constraints with a world size above 1 is not implemented: the column maxima are per process")
        from .constraints import Constraints
        self.constraints = Constraints(spec, tau, ramp_its, reward_clip, self.device)

    def _init_smooth(self, smooth, coef_t, coef_s, sigma):
        from .smooth import blocks, check_values
        succ, pert = blocks(smooth)
        if self._recurrent:
            raise ValueError("PPO: --smooth and --recurrent exclude each other: successor rows of a recurrent policy's minibatch are not implemented")
        if self.symmetry is not None:
            raise ValueError("PPO: --smooth and --symmetry exclude each other: both extend the minibatch")
        if self._state_dependent:
            raise ValueError("PPO: --smooth and --state_dependent_std exclude each other: a smoothness loss on the [mean | s] output is "
                             "not implemented")
        if _world() > 1:
            raise NotImplementedError("PPO: --smooth with a world size above 1 is not implemented: it trains in one process only")
        check_values(coef_t, coef_s, sigma)
        self.smooth, self._smooth_succ, self._smooth_pert = smooth, succ, pert
        self.smooth_temporal_coef, self.smooth_spatial_coef, self.smooth_sigma = float(coef_t), float(coef_s), float(sigma)
        self._smooth_sum = torch.zeros(2, device=self.device)   # the update's sums of L_T and L_S (finite steps), read back once per update
        self._smooth_bufs, self._smooth_bufs_gather, self._smooth_eps, self._smooth_valid = None, None, None, None

    def init_storage(self, num_envs, num_transitions_per_env, **_):
        ac = self.actor_critic
        if self.smooth is not None and self._smooth_succ and num_transitions_per_env < 2:
            raise ValueError(f"PPO: --smooth {self.smooth} with num_transitions_per_env={num_transitions_per_env}: a rollout of one step holds no "
                             "successor row (use --smooth spatial or a longer rollout)")
        self.transition = RolloutStorage.Transition()
        if self._recurrent:
            from .recurrent import RecurrentRolloutStorage
            self.storage = RecurrentRolloutStorage(num_envs, num_transitions_per_env, [ac.num_actor_input], [ac.num_critic_input],
                                                   [ac.num_actor_output], ac.rnn_hidden_size, self.device)
            return
        self.storage = RolloutStorage(num_envs, num_transitions_per_env, [ac.num_actor_input], [ac.num_critic_input],
                                      [ac.num_actor_output], self.device)
        if self.multi_critic is not None:   # (the K-wide values / rewards / returns beside it)
            self.multi_critic.init_storage(num_envs, num_transitions_per_env)
        if self.constraints is not None:   # (the [T, N] termination probabilities beside it)
            self.constraints.init_storage(num_envs, num_transitions_per_env)

    def test_mode(self):
        self.actor_critic.eval()

    def train_mode(self):
        self.actor_critic.train()

    def _act_eager(self, actor_observations, critic_observations, capturable=False):
        ac = self.actor_critic
        if capturable:   # Normal.sample() = torch.normal(mean, std) checks std >= 0 on the host: not capturable
            ac.update_distribution(actor_observations)
            actions = (ac.action_mean + ac.action_std * torch.randn_like(ac.action_mean)).detach()
        else:
            actions = ac.act(actor_observations).detach()
        values = ac.evaluate(critic_observations).detach()
        if self.value_norm is not None:   # (the network's output is a normalised value: the storage and GAE work in reward units)
            values = self.value_norm.denormalize(values)
        logp = ac.get_actions_log_prob(actions).detach()
        return actions, values, logp, ac.action_mean.detach(), ac.action_std.detach()

    def _act_graphed(self, actor_observations, critic_observations):
        """The rollout's policy step replayed from HIP graphs on static input / output buffers -- TWO of them: the actor
        (MLP forward, sample, log-prob: what env.step() waits for) on the current stream, the critic (MLP forward: only the
        storage needs it) on a side stream, where it overlaps the env step that follows (the step kernel leaves half of the
        chip idle at 4096 envs).  process_env_step() waits for the critic before it stores the transition.  The outputs are
        consumed (env.step, the storage kernel) before the next call overwrites them.  The sampling draws from torch's default
        generator, which CUDA graphs advance per replay."""
        self._ensure_act_graph(actor_observations, critic_observations)
        cur = torch.cuda.current_stream(self.device)
        self._ev_obs.record(cur)                       # this step's observations are final on the current stream
        self._act_side.wait_event(self._ev_obs)
        with torch.cuda.stream(self._act_side):
            self._act_in[1].copy_(critic_observations)
            self._critic_graph.replay()
            self._ev_critic.record(self._act_side)
        self._critic_pending = True
        self._act_in[0].copy_(actor_observations)
        self._act_graph.replay()
        return self._act_out

    def _ensure_act_graph(self, actor_observations, critic_observations):
        """Capture the two policy-step graphs of _act_graphed for these observation shapes, unless they exist already."""
        key = (tuple(actor_observations.shape), tuple(critic_observations.shape))
        ac = self.actor_critic
        cur = torch.cuda.current_stream(self.device)
        if self._act_graph is None or self._act_key != key:
            # (not under inference_mode, where the runner calls act(): tensors created there -- the static buffers, the
            #  generator's graph state -- would be inference tensors that later captures / replays may not update)
            with torch.inference_mode(False), torch.no_grad():
                self._act_in = (torch.zeros_like(actor_observations), torch.zeros_like(critic_observations))

                # GRX_PPO_FUSED_MLP (default on): the two MLP forwards through libgrx_ppo.so -- one MFMA launch per layer with
                # bias + ELU in the epilogue, the actor's output layer fused with the sampling and the log-probability
                # (rl/fused_loss.py: mlp_forward / policy_act) -- instead of 8 library GEMMs, 6 ELU kernels and ~20 small
                # distribution kernels per rollout step
                fuse = (os.environ.get("GRX_PPO_FUSED_MLP", "1") != "0" and mlp_can_fuse(ac.actor, self._act_in[0])
                        and mlp_can_fuse(ac.critic, self._act_in[1]) and ac.num_actor_output <= 32)
                self._act_fused = fuse

                def actor_part():
                    if fuse:
                        eps = torch.randn(self._act_in[0].shape[0], ac.num_actor_output, device=self.device)
                        # (fixed_std: update_distribution -- and so the update's log-prob -- uses init_noise_std, not the parameter)
                        if getattr(ac, "state_dependent_std", False):   # (the output layer is [mean | s]: sigma per row, still one head launch)
                            return policy_act(ac.actor, None, self._act_in[0], eps, state_dependent=ac.noise_std_type)
                        std = ac.init_std.clone() if getattr(ac, "fixed_std", False) else _noise_std(ac).detach()
                        return policy_act(ac.actor, std, self._act_in[0], eps)
                    ac.update_distribution(self._act_in[0])   # Normal.sample() checks std >= 0 on the host: not capturable
                    actions = (ac.action_mean + ac.action_std * torch.randn_like(ac.action_mean)).detach()
                    return actions, ac.get_actions_log_prob(actions).detach(), ac.action_mean.detach(), ac.action_std.detach()

                def critic_part():
                    v = mlp_forward(ac.critic, self._act_in[1]) if fuse else ac.evaluate(self._act_in[1]).detach()
                    if self.value_norm is not None:   # (captured: a replay reads the statistics' tensors, so it sees them as they are then)
                        v = self.value_norm.denormalize(v)
                    return v
                side = torch.cuda.Stream(device=self.device)
                self._act_side = torch.cuda.Stream(device=self.device)
                side.wait_stream(cur)
                with torch.cuda.stream(side):
                    for _ in range(2):
                        actor_part(); critic_part()
                cur.wait_stream(side)
                self._act_graph = torch.cuda.CUDAGraph()
                with _graph_capture(self._act_graph, side):
                    a_out = actor_part()
                self._critic_graph = torch.cuda.CUDAGraph()
                with _graph_capture(self._critic_graph, side):
                    v_out = critic_part()
                self._act_out = (a_out[0], v_out, a_out[1], a_out[2], a_out[3])
                self._ev_obs, self._ev_critic = torch.cuda.Event(), torch.cuda.Event()
            self._act_key = key

    def _join_critic(self):
        """values of the current policy step are ready on the current stream from here on"""
        if getattr(self, "_critic_pending", False):
            torch.cuda.current_stream(self.device).wait_event(self._ev_critic)
            self._critic_pending = False

    def act(self, actor_observations, critic_observations):
        t = self.transition
        if self._recurrent:
            return self._act_recurrent(actor_observations, critic_observations)
        if self._beta:   # the storage takes x and (alpha, beta); the env takes a = lo + span x
            t.actions, t.values, t.actions_log_prob, t.action_mean, t.action_sigma, env_actions = self._act_beta(actor_observations,
                                                                                                              critic_observations)
            t.observations, t.critic_observations = actor_observations, critic_observations
            return env_actions
        if self._use_act_graph and actor_observations.is_cuda and not torch.is_grad_enabled():
            t.actions, t.values, t.actions_log_prob, t.action_mean, t.action_sigma = self._act_graphed(actor_observations, critic_observations)
        else:
            t.actions, t.values, t.actions_log_prob, t.action_mean, t.action_sigma = self._act_eager(actor_observations, critic_observations)
        t.observations, t.critic_observations = actor_observations, critic_observations
        return t.actions

    def _act_recurrent(self, actor_observations, critic_observations):
        """act() for a recurrent policy: both memories advance by one step (a cell launch each, the reset of the envs that just ended
        folded in), then the two MLPs on the memories' outputs.  Eager."""
        t, ac, st = self.transition, self.actor_critic, self.storage
        if st.step == 0:   # what both memories start this rollout from: the update's forward starts there too
            n, dev = actor_observations.shape[0], actor_observations.device
            st.set_start_states(ac.memory_a.start_state(n, dev), ac.memory_c.start_state(n, dev))
        with torch.no_grad():
            t.actions, t.values, t.actions_log_prob, t.action_mean, t.action_sigma = ac.rollout_step(actor_observations, critic_observations)
        t.observations, t.critic_observations = actor_observations, critic_observations
        return t.actions

    def act_inference(self, obs):
        return self.actor_critic.act_inference(obs)

    def process_env_step(self, rewards, dones, infos, log=None):
        """ppo.py:184-197.  On a HIP device everything here -- the time-out bootstrap, the nine row copies of
        RolloutStorage.add_transitions and (log = (cur_rew, cur_len, done_rew_row, done_len_row)) the runner's running episode
        reward / length -- is ONE kernel (include/grx_ppo.h grx_ppo_store_transition)."""
        t = self.transition
        st = self.storage
        self._join_critic()
        if self.multi_critic is not None:   # the heads' values and the group rewards into their own rows; the scalar store gets sum_k v_k
            t.values = self.multi_critic.store(st.step, t.values, infos.get("time_outs"), self.gamma)
        if self._fused_store and rewards.is_cuda and t.observations is not None and t.observations.is_contiguous():
            if st.step >= st.num_transitions_per_env:
                raise AssertionError("Rollout buffer overflow")
            from .fused_loss import store_transition
            pri = t.critic_observations if st.pri_observations is not None else None
            store_transition(st, st.step, t.observations, pri, t.actions, t.action_mean, t.action_sigma, t.values, t.actions_log_prob,
                             rewards if rewards.is_contiguous() else rewards.contiguous(), dones, infos.get("time_outs"), self.gamma, log)
            st.step += 1
            t.clear()
            self.actor_critic.reset(dones)
            return
        if log is not None:   # the torch spelling of the runner's bookkeeping (on_policy_runner.py:170-181)
            cur_rew, cur_len, done_rew, done_len = log
            cur_rew += rewards; cur_len += 1
            d = dones > 0
            done_rew.copy_(cur_rew); done_len.copy_(cur_len)
            cur_rew *= ~d; cur_len *= ~d
        t.rewards = rewards.clone()
        t.dones = dones
        if "time_outs" in infos:   # bootstrap on time-outs (ppo.py:190-191)
            t.rewards += self.gamma * torch.squeeze(t.values * infos["time_outs"].unsqueeze(1).to(self.device), 1)
        self.storage.add_transitions(t)
        t.clear()
        self.actor_critic.reset(dones)

    def rnd_step(self, frame, step):
        """after process_env_step of rollout step `step`: the intrinsic reward of the raw frame the env just returned, added to the
        storage's reward row of that step in place (the row holds the env's reward and the time-out bootstrap by then)"""
        if self.multi_critic is not None:   # (the runner refuses the pair before it builds anything; a caller that assigns `rnd` itself ends here)
            raise ValueError("PPO: --reward_groups and --rnd exclude each other: the intrinsic reward belongs to no group")
        if self.constraints is not None:   # (likewise)
            raise ValueError("PPO: --constraints and --rnd exclude each other: the order of the two edits of the reward row is not pinned")
        self.rnd.rollout_step(frame, self.storage.rewards[step], step)

    def constraint_step(self, step):
        """after process_env_step of rollout step `step`: the step's termination probabilities from the env's tensors as they are now, and
        the storage's reward row of that step scaled by (1 - delta) in place (the row holds the env's reward and the time-out bootstrap by then)"""
        self.constraints.step(step, self.storage)

    def compute_returns(self, last_critic_obs):
        self._join_critic()
        if self._recurrent:   # from the critic's memory as it is, into scratch: the memory does not advance
            last_values = self.actor_critic.evaluate_bootstrap(last_critic_obs).detach()
            self.storage.compute_returns(last_values, self.gamma, self.lam)
            return
        last_values = self.actor_critic.evaluate(last_critic_obs).detach()
        if self.value_norm is not None:   # GAE in reward units, the statistics' update, then the storage's values / returns normalised in place
            self.value_norm.compute_returns(self.storage, self.value_norm.denormalize(last_values), self.gamma, self.lam,
                                            critic=self.actor_critic.critic)
            return
        if self.multi_critic is not None:   # GAE and the advantage normalisation per group, the advantages their weighted sum
            self.multi_critic.compute_returns(self.storage, last_values, self.gamma, self.lam)
            return
        if self.constraints is not None:   # the storage's loop with alive = (1 - done)(1 - delta), the advantages normalised as ever
            self.constraints.compute_returns(self.storage, last_values, self.gamma, self.lam)
            return
        self.storage.compute_returns(last_values, self.gamma, self.lam)

    def update_learning_rate(self, kl_mean):
        if kl_mean > self.desired_kl * 2.0:
            self.learning_rate = max(self.learning_rate_min, self.learning_rate / 1.5)
        elif self.desired_kl / 2.0 > kl_mean > 0.0:
            self.learning_rate = min(self.learning_rate_max, self.learning_rate * 1.5)

    def _sync_gradients(self, kl_mean, bad=None):
        """ONE collective per optimizer step: [flat grads | KL | bad] summed over ranks, averaged.  The gradients already
        live in the bucket (backward accumulated into the views after _zero_flat_grads).  Returns (KL, any-rank-bad)."""
        b, n = self._bucket, self._nflat
        b[n] = kl_mean
        b[n + 1] = 0.0 if bad is None else bad.to(b.dtype)
        dist.all_reduce(b)
        b /= _world()
        return b[n], b[n + 1] > 0

    def _zero_flat_grads(self):
        if any(p.grad is None or p.grad.data_ptr() != self._bucket.data_ptr() + 4 * o for p, o in zip(self._params, self._offsets())):
            self._install_flat_grads()   # (someone ran zero_grad(set_to_none=True) in between)
        self._bucket.zero_()

    def _offsets(self):
        o = 0
        for p in self._params:
            yield o
            o += -(-p.numel() // 64) * 64

    def _device_lr_update(self, kl_mean):
        """update_learning_rate() on the device (same branches as ppo.py:205-213)."""
        lr = self._lr_t
        down = torch.clamp(lr / 1.5, min=self.learning_rate_min)
        up = torch.clamp(lr * 1.5, max=self.learning_rate_max)
        new = torch.where(kl_mean > self.desired_kl * 2.0, down,
                          torch.where((kl_mean < self.desired_kl / 2.0) & (kl_mean > 0.0), up, lr))
        lr.copy_(new)

    def update(self):
        if self._recurrent:
            return self._update_recurrent()
        if self.symmetry is not None:
            return self._update_symmetry()
        if self.smooth is not None:
            return self._update_smooth()
        if self.grad_penalty_coef is not None:
            return self._update_gp()
        if self.multi_critic is not None:
            return self._update_mc()
        if self._beta and not self._device_lr:   # (the CPU loop below spells out the Gaussian's KL)
            return self._update_beta_cpu()
        if self._device_lr:
            # For these GEMM shapes (batch ~10^4 rows, 39..512 columns, fp32) rocBLAS's kernel choices beat hipBLASLt's by 2x
            # on the weight-gradient products dY^T X (27-48 us against 66-73 us, tools/gpu_gemm_probe.py).  torch's BLAS
            # preference is process-global, so it is switched for the update only (GRX_PPO_BLAS=hipblaslt leaves it alone).
            with self._blas_for_update():
                if self._use_graph:
                    return self._update_graphed()
                return self._update_device()
        mean_value_loss, mean_surrogate_loss = 0.0, 0.0
        ac, multi = self.actor_critic, _collective_path()
        adaptive = self.desired_kl is not None and self.schedule == "adaptive"
        for (obs, cobs, actions, target_values, advantages, returns, old_logp, old_mu, old_sigma, _, _) in \
                self.storage.mini_batch_generator(self.num_mini_batches, self.num_learning_epochs):
            ac.act(obs)
            logp = ac.get_actions_log_prob(actions)
            value = ac.evaluate(cobs)
            mu, sigma, entropy = ac.action_mean, ac.action_std, ac.entropy
            kl_mean = None
            if adaptive:
                with torch.inference_mode():
                    kl = torch.sum(torch.log(sigma / old_sigma + 1.e-5) + (old_sigma.square() + (old_mu - mu).square())
                                   / (2.0 * sigma.square()) - 0.5, axis=-1)
                    kl_mean = kl.mean()
                if not multi:
                    self._apply_kl(kl_mean.item())
            ratio = torch.exp(logp - torch.squeeze(old_logp))
            adv = torch.squeeze(advantages)
            surrogate_loss = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1.0 - self.clip_param, 1.0 + self.clip_param)).mean()
            if self.use_clipped_value_loss:
                clipped = target_values + (value - target_values).clamp(-self.clip_param, self.clip_param)
                value_loss = torch.max((value - returns).pow(2), (clipped - returns).pow(2)).mean()
            else:
                value_loss = (returns - value).pow(2).mean()
            loss = surrogate_loss + self.value_loss_coef * value_loss - self.entropy_coef * entropy.mean()
            if not multi and torch.isnan(loss):
                continue
            if multi:
                self._zero_flat_grads()
            else:
                self.optimizer.zero_grad()
            loss.backward()
            if multi:
                kl_avg, bad = self._sync_gradients(kl_mean if kl_mean is not None else torch.zeros((), device=self.device),
                                                   ~torch.isfinite(loss.detach()))
                if adaptive:
                    self._apply_kl(kl_avg.item())
                if bool(bad) or not bool(torch.isfinite(self._bucket[:self._nflat]).all()):
                    continue   # NaN-skip must be a collective decision: the averaged bucket is identical on every rank
            if not torch.isfinite(nn.utils.clip_grad_norm_(ac.parameters(), self.max_grad_norm)):
                continue   # (a gradient whose norm is not finite skips the step too: include/grx_ppo.h grx_ppo_step_tail)
            self.optimizer.step()
            mean_value_loss += value_loss.item()
            mean_surrogate_loss += surrogate_loss.item()
        self.num_updates = self.num_learning_epochs * self.num_mini_batches
        return mean_value_loss / self.num_updates, mean_surrogate_loss / self.num_updates

    def _update_recurrent(self):
        """update() for a recurrent policy: rsl_rl's recurrent_mini_batch_generator order (env ranges over all T steps, no permutation),
        both memories run over the whole rollout from its stored start state (ActorCriticRecurrent.features), and the flattened outputs go
        through _losses and the step's tail as they are.  Eager; on a HIP device without a host round trip inside the loop."""
        ac = self.actor_critic
        adaptive = self.desired_kl is not None and self.schedule == "adaptive"
        sums = torch.zeros(3, device=self.device)        # value loss, surrogate loss, last KL
        self.num_updates = self.num_learning_epochs * self.num_mini_batches
        with self._blas_for_update() if self._device_lr else contextlib.nullcontext():
            for (obs, cobs, resets, start, actions, target_values, advantages, returns, old_logp, old_mu, old_sigma) in \
                    self.storage.recurrent_mini_batch_generator(self.num_mini_batches, self.num_learning_epochs):
                fa, fc = ac.features(obs, cobs, resets, start)
                with ac.on_features():
                    surrogate_loss, value_loss, loss, kl_mean = self._losses(fa, fc, actions, target_values, advantages, returns,
                                                                              old_logp, old_mu, old_sigma)
                if not self._device_lr:
                    if adaptive:
                        self._apply_kl(kl_mean.item())
                    if not torch.isfinite(loss):
                        continue
                    self.optimizer.zero_grad()
                    loss.backward()
                    if not torch.isfinite(nn.utils.clip_grad_norm_(ac.parameters(), self.max_grad_norm)):
                        continue   # (a gradient whose norm is not finite skips the step too: include/grx_ppo.h grx_ppo_step_tail)
                    self.optimizer.step()
                    sums[0] += value_loss.detach(); sums[1] += surrogate_loss.detach()
                    continue
                self.optimizer.zero_grad(set_to_none=False)
                loss.backward()
                if self._step_tail(loss, kl_mean, value_loss, surrogate_loss, sums, adaptive):
                    continue
                if adaptive:
                    self._device_lr_update(kl_mean)
                bad = self._clip_found_inf(~torch.isfinite(loss.detach()))
                self.optimizer.step()
                with torch.no_grad():
                    sums[0] += torch.where(bad, 0.0, value_loss.detach())   # (a skipped step adds nothing)
                    sums[1] += torch.where(bad, 0.0, surrogate_loss.detach())
                    sums[2] = kl_mean
        host = sums.tolist()                           # the only device->host transfer of the update on a HIP device
        if self._device_lr:
            self.mean_kl = host[2]
            self.learning_rate = float(self._lr_t.item())
        return host[0] / self.num_updates, host[1] / self.num_updates

    @contextlib.contextmanager
    def _blas_for_update(self):
        """torch's BLAS preference for the update: rocBLAS (GRX_PPO_BLAS=hipblaslt: left alone), put back afterwards"""
        prev_blas = torch.backends.cuda.preferred_blas_library()
        if os.environ.get("GRX_PPO_BLAS", "rocblas") == "rocblas":
            torch.backends.cuda.preferred_blas_library("cublas")
        try:
            yield
        finally:
            torch.backends.cuda.preferred_blas_library(prev_blas)

    def _losses(self, obs, cobs, actions, target_values, advantages, returns, old_logp, old_mu, old_sigma):
        """(surrogate_loss, value_loss, loss, kl_mean) of one minibatch -- ppo.py:215-245.

        On a HIP device: the actor / critic forward in torch, everything after it in ONE kernel that also produces the
        gradients (rl/fused_loss.py -> libgrx_ppo.so; GRX_PPO_FUSED_LOSS=0 keeps the torch expression of _loss_terms)."""
        mu, value = self._forward(obs, cobs)
        return self._loss_terms(mu, value, actions, target_values, advantages, returns, old_logp, old_mu, old_sigma)

    def _loss_is_fused(self):
        ac = self.actor_critic
        if self._beta:   # (GRX_BETA_FUSED=0: the torch spelling on a HIP device too)
            from .beta import fused_enabled
            if not fused_enabled():
                return False
        return self._fused_loss and not ac.fixed_std and ac.num_actor_output <= 32   # the kernel's action-count limit

    def _forward(self, obs, cobs, actor=None):
        """(mu, value): the actor's and the critic's forward of one minibatch (state_dependent_std: mu is the actor's raw [mean | s]).
        actor: what runs in the actor's place and whose result is handed back as mu (the gradient penalty's function)"""
        ac = self.actor_critic
        if actor is not None:
            if not self._loss_is_fused():
                return actor(obs), ac.evaluate(cobs)
        elif (self._state_dependent or self._beta) and not self._loss_is_fused():
            return ac.actor(obs), ac.evaluate(cobs)   # (the raw output [mean | s] or [p | q]: _loss_terms splits it)
        elif not self._loss_is_fused():
            ac.update_distribution(obs)   # (the torch spelling in _loss_terms reads sigma from the distribution)
            return ac.action_mean, ac.evaluate(cobs)
        else:
            actor = ac.actor
        # (only while the actor's GEMMs go to rocBLAS -- update() / _build_graph's preference: with torch's default hipBLASLt on BOTH
        #  streams, the value head's weight gradient at minibatch 49152 came out wrong once and the step did not finish twice)
        if self._two_streams and torch.backends.cuda.preferred_blas_library() == torch._C._BlasBackend.Cublas:
            # actor and critic are independent until the loss: the critic's forward (and, through autograd's stream
            # bookkeeping, its backward) runs on a second stream
            cur = torch.cuda.current_stream(self.device)
            if self._aux_stream is None:
                self._aux_stream = torch.cuda.Stream(device=self.device)
            self._aux_stream.wait_stream(cur)
            with torch.cuda.stream(self._aux_stream):
                value = ac.evaluate(cobs)
            mu = actor(obs)
            cur.wait_stream(self._aux_stream)
            value.record_stream(cur)
            return mu, value
        mu = actor(obs)
        return mu, ac.evaluate(cobs)

    def _loss_terms(self, mu, value, actions, target_values, advantages, returns, old_logp, old_mu, old_sigma):
        """(surrogate_loss, value_loss, loss, kl_mean) from _forward's outputs; mu may be the first rows of what the actor returned
        (symmetry "loss": the mirrored rows behind them have no PPO loss)"""
        ac = self.actor_critic
        adaptive = self.desired_kl is not None and self.schedule == "adaptive"
        if self.multi_critic is not None:   # (value / returns / target_values are [mb, K]: the value loss is the sum over the heads)
            return self.multi_critic.loss(mu, _noise_std(ac), value, actions, old_logp, old_mu, old_sigma, advantages, returns, target_values,
                                          self.clip_param, self.value_loss_coef, self.entropy_coef, self.use_clipped_value_loss, adaptive,
                                          self._loss_is_fused())
        if self._beta:   # (mu is the raw [p | q], actions are x, old_mu / old_sigma the rollout's alpha / beta)
            from . import beta as B
            if self._loss_is_fused():
                out = B.fused_ppo_loss_beta(mu, value, actions, old_logp, old_mu, old_sigma, advantages, returns, target_values,
                                            self.clip_param, self.value_loss_coef, self.entropy_coef, self.use_clipped_value_loss)
                kl_mean = out[3].detach() if adaptive else torch.zeros((), device=self.device)
                return out[0], out[1], out[2], kl_mean
            return B.loss_torch(mu, value, actions, old_logp, old_mu, old_sigma, advantages, returns, target_values, self.clip_param,
                                self.value_loss_coef, self.entropy_coef, self.use_clipped_value_loss, with_kl=adaptive)
        if self._state_dependent and self._loss_is_fused():   # (mu is the raw [mean | s]: the gradient lands on it in one launch)
            out = fused_ppo_loss_sd(mu, value, actions, old_logp, old_mu, old_sigma, advantages, returns, target_values,
                                    ac.noise_std_type == "log", self.clip_param, self.value_loss_coef, self.entropy_coef,
                                    self.use_clipped_value_loss)
            kl_mean = out[3].detach() if adaptive else torch.zeros((), device=self.device)
            return out[0], out[1], out[2], kl_mean
        if self._loss_is_fused():
            out = fused_ppo_loss(mu, _noise_std(ac), value, actions, old_logp, old_mu, old_sigma, advantages, returns, target_values,
                                 self.clip_param, self.value_loss_coef, self.entropy_coef, self.use_clipped_value_loss)
            kl_mean = out[3].detach() if adaptive else torch.zeros((), device=self.device)
            return out[0], out[1], out[2], kl_mean
        if self._state_dependent:
            mu, sigma = ac.split_raw(mu)
        else:
            sigma = ac.action_std[:mu.shape[0]]
        dist_ = torch.distributions.Normal(mu, sigma, validate_args=False)
        logp, entropy = dist_.log_prob(actions).sum(dim=-1), dist_.entropy().sum(dim=-1)
        kl_mean = torch.zeros((), device=self.device)
        if adaptive:
            with torch.no_grad():
                kl_mean = torch.sum(torch.log(sigma / old_sigma + 1.e-5) + (old_sigma.square() + (old_mu - mu).square())
                                    / (2.0 * sigma.square()) - 0.5, axis=-1).mean()
        ratio = torch.exp(logp - torch.squeeze(old_logp))
        adv = torch.squeeze(advantages)
        surrogate_loss = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1.0 - self.clip_param, 1.0 + self.clip_param)).mean()
        if self.use_clipped_value_loss:
            clipped = target_values + (value - target_values).clamp(-self.clip_param, self.clip_param)
            value_loss = torch.max((value - returns).pow(2), (clipped - returns).pow(2)).mean()
        else:
            value_loss = (returns - value).pow(2).mean()
        loss = surrogate_loss + self.value_loss_coef * value_loss - self.entropy_coef * entropy.mean()
        return surrogate_loss, value_loss, loss, kl_mean

    # ------------------------------------------------------------------ left-right symmetry (rl/symmetry.py)
    def _sym_gatherer(self, srcs, dsts):
        """idx -> the minibatch with its mirrored half in dsts: one launch of grx_sym_gather_rows on a HIP device (GRX_SYM_FUSED=0, CPU
        tensors: rl.symmetry.sym_gather_torch, the same arithmetic in torch)"""
        from .symmetry import fused_enabled, sym_gather_torch
        if srcs[0].is_cuda and fused_enabled():
            from .fused_loss import SymGather
            return SymGather(srcs, dsts, self._sym_modes, self._sym_tensor_maps)
        return lambda idx: sym_gather_torch(srcs, dsts, self._sym_modes, self._sym_tensor_maps, idx)

    def _mirror_actions(self, mu):
        """mirror_actions(mu) for mu [mb, A] (detached): one grx_sym_gather_rows call without an index on a HIP device, through a
        MirrorRows kept per shape (its pointer tables and its output buffer are built once)"""
        from .symmetry import fused_enabled
        m = self._sym.actions
        if not (mu.is_cuda and fused_enabled()):
            return m(mu)
        key = (tuple(mu.shape), mu.device)
        if self._sym_mirror is None or self._sym_mirror[0] != key:
            from .fused_loss import MirrorRows
            self._sym_mirror = (key, MirrorRows(mu.shape[0], m, mu.device))
        return self._sym_mirror[1](mu)

    def _losses_sym(self, obs, cobs, actions, target_values, advantages, returns, old_logp, old_mu, old_sigma):
        """_losses on a minibatch whose second half is the mirror image of its first (symmetry "augment" / "both": every tensor has
        2 mb rows; "loss": obs alone, the PPO loss and the critic see the mb rows there are), plus the mirror loss
        mse(mu[mb:], mirror_actions(mu[:mb]).detach()) through grx_distill_loss: added to the loss with symmetry_coef ("loss" / "both"),
        logged only ("augment")."""
        from .distillation import distill_loss
        mb, n = obs.shape[0] // 2, actions.shape[0]   # rows of the unmirrored half; rows the PPO loss sees
        mu, value = self._forward(obs, cobs)
        surrogate_loss, value_loss, loss, kl_mean = self._loss_terms(mu[:n], value, actions, target_values, advantages, returns,
                                                                     old_logp, old_mu, old_sigma)
        with torch.no_grad():
            target = self._mirror_actions(mu[:mb].detach())
        if self.symmetry == "augment":
            with torch.no_grad():
                sym = distill_loss(mu[mb:].detach(), target, "mse")
        else:
            sym = distill_loss(mu[mb:], target, "mse")
            loss = loss + self.symmetry_coef * sym
        with torch.no_grad():   # (a step the NaN-skip drops adds nothing, as with the other statistics)
            s = sym.detach().reshape(1)
            self._sym_sum += torch.where(torch.isfinite(loss.detach()).reshape(1), s, torch.zeros_like(s))
        return surrogate_loss, value_loss, loss, kl_mean

    def _sym_sources(self):
        st = self.storage
        flat = lambda x: x.flatten(0, 1)
        cobs = st.pri_observations if st.pri_observations is not None else st.observations
        return [flat(x) for x in (st.observations, cobs, st.actions, st.values, st.advantages, st.returns, st.actions_log_prob, st.mu, st.sigma)]

    def _update_symmetry(self):
        """update() with symmetry on: the maps take the normalisers' statistics as they are now (in place), every minibatch is gathered
        WITH its mirrored half into fixed buffers, and the step is the captured one, the eager device one or the CPU one below"""
        self._sym.refresh()
        self._sym_sum.zero_()
        if self._device_lr:
            with self._blas_for_update():
                out = self._update_graphed() if self._use_graph else self._update_sym_eager()
        else:
            out = self._update_sym_eager()
        self.mean_symmetry_loss = float(self._sym_sum.item()) / self.num_updates   # one extra 4-byte read-back per update
        return out

    def _update_sym_eager(self):
        """the eager paths: on a HIP device _update_graphed's loop with the step run, not replayed (the arithmetic of _update_device);
        on the CPU update()'s host-side adaptive learning rate, NaN-skip, clip and Adam"""
        st = self.storage
        mb = st.num_envs * st.num_transitions_per_env // self.num_mini_batches
        srcs = self._sym_sources()
        if self._sym_bufs is None or self._sym_bufs[0].shape[0] != 2 * mb or self._sym_bufs[0].device != srcs[0].device:
            self._sym_bufs = [torch.zeros(mb * (2 if m else 1), s.shape[1], device=s.device) for m, s in zip(self._sym_modes, srcs)]
            self._sym_bufs_gather = None
        key = tuple(s.data_ptr() for s in srcs)
        if self._sym_bufs_gather is None or self._sym_bufs_gather[0] != key:
            self._sym_bufs_gather = (key, self._sym_gatherer(srcs, self._sym_bufs))
        gather, bufs = self._sym_bufs_gather[1], self._sym_bufs
        indices = torch.randperm(self.num_mini_batches * mb, requires_grad=False, device=self.device)   # RS:63-112: one permutation, reused
        adaptive = self.desired_kl is not None and self.schedule == "adaptive"
        sums = torch.zeros(3, device=self.device)        # value loss, surrogate loss, last KL
        self.num_updates = self.num_learning_epochs * self.num_mini_batches
        for _ in range(self.num_learning_epochs):
            for i in range(self.num_mini_batches):
                gather(indices[i * mb:(i + 1) * mb])
                if self._device_lr:
                    self._minibatch_step(bufs, sums)
                    continue
                surrogate_loss, value_loss, loss, kl_mean = self._losses_sym(*bufs)
                if adaptive:
                    self._apply_kl(kl_mean.item())
                if not torch.isfinite(loss):
                    continue
                self.optimizer.zero_grad()
                loss.backward()
                if not torch.isfinite(nn.utils.clip_grad_norm_(self.actor_critic.parameters(), self.max_grad_norm)):
                    continue   # (a gradient whose norm is not finite skips the step too: include/grx_ppo.h grx_ppo_step_tail)
                self.optimizer.step()
                sums[0] += value_loss.detach(); sums[1] += surrogate_loss.detach()
        host = sums.tolist()
        if self._device_lr:
            self.mean_kl = host[2]
            self.learning_rate = float(self._lr_t.item())
        return host[0] / self.num_updates, host[1] / self.num_updates

    # ------------------------------------------------------------------ action smoothness (rl/smooth.py)
    def _smooth_rows(self):
        return 1 + int(self._smooth_succ) + int(self._smooth_pert)

    def _smooth_alloc(self, mb, width):
        """the two buffers beside the minibatch: the step's noise eps [mb, W] (spatial) and the pairs' valid bytes [mb] (temporal)"""
        self._smooth_eps = torch.zeros(mb, width, device=self.device) if self._smooth_pert else None
        self._smooth_valid = torch.zeros(mb, dtype=torch.uint8, device=self.device) if self._smooth_succ else None

    def _smooth_gatherer(self, srcs, dsts, draw=True):
        """idx -> the minibatch in dsts, the successor / perturbed rows behind its actor input: one launch of grx_smooth_gather_rows on a HIP
        device (GRX_SMOOTH_FUSED=0, CPU tensors: rl.smooth.smooth_gather_torch, the same arithmetic in torch).  draw: a fresh eps ~ N(0, 1)
        from the device's generator in front of every gather (outside the captured step, next to the gather)"""
        from .smooth import NoisyGather, SmoothGather, fused_enabled, smooth_gather_torch
        st = self.storage
        N, T, dones = st.num_envs, st.num_transitions_per_env, st.dones.reshape(-1)
        args = (N, T, dones, self._smooth_succ, self._smooth_pert, self._smooth_eps, self.smooth_sigma, self._smooth_valid)
        if srcs[0].is_cuda and fused_enabled():
            gather = SmoothGather(srcs, dsts, *args)
        else:
            gather = lambda idx: smooth_gather_torch(srcs, dsts, idx, *args)
        return NoisyGather(self._smooth_eps if draw else None, gather)

    def _losses_smooth(self, obs, cobs, actions, target_values, advantages, returns, old_logp, old_mu, old_sigma):
        """_losses on a minibatch whose actor input has the successor and / or the perturbed rows behind its mb rows: the PPO loss, the
        critic and the KL see the mb rows there are, the actor runs on all of them, and coef_t L_T + coef_s L_S (grx_smooth_loss) joins the
        loss."""
        from .smooth import fused_enabled, smooth_loss
        n = actions.shape[0]
        mu, value = self._forward(obs, cobs)
        surrogate_loss, value_loss, loss, kl_mean = self._loss_terms(mu[:n], value, actions, target_values, advantages, returns,
                                                                     old_logp, old_mu, old_sigma)
        sm, terms = smooth_loss(mu, self._smooth_succ, self._smooth_pert, self._smooth_valid, self.smooth_temporal_coef,
                                self.smooth_spatial_coef, fused=fused_enabled())
        loss = loss + sm
        with torch.no_grad():   # (a step the NaN-skip drops adds nothing, as with the other statistics)
            self._smooth_sum += torch.where(torch.isfinite(loss.detach()).reshape(1), terms, torch.zeros_like(terms))
        return surrogate_loss, value_loss, loss, kl_mean

    def _smooth_sources(self):
        return self._sym_sources()   # (the same nine storage tensors, flattened to [T N, .])

    def _update_smooth(self):
        """update() with smoothness on: every minibatch is gathered WITH its extra actor rows into fixed buffers, and the step is the
        captured one, the eager device one or the CPU one below"""
        self._smooth_sum.zero_()
        if self._device_lr:
            with self._blas_for_update():
                out = self._update_graphed() if self._use_graph else self._update_smooth_eager()
        else:
            out = self._update_smooth_eager()
        host = self._smooth_sum.tolist()   # one extra 8-byte read-back per update
        self.mean_smooth_temporal, self.mean_smooth_spatial = host[0] / self.num_updates, host[1] / self.num_updates
        return out

    def _update_smooth_eager(self):
        """the eager paths, as _update_sym_eager: on a HIP device _update_graphed's loop with the step run, not replayed; on the CPU
        update()'s host-side adaptive learning rate, NaN-skip, clip and Adam"""
        st = self.storage
        mb = st.num_envs * st.num_transitions_per_env // self.num_mini_batches
        srcs = self._smooth_sources()
        R = self._smooth_rows()
        if self._smooth_bufs is None or self._smooth_bufs[0].shape[0] != R * mb or self._smooth_bufs[0].device != srcs[0].device:
            self._smooth_bufs = [torch.zeros(mb * (R if t == 0 else 1), s.shape[1], device=s.device) for t, s in enumerate(srcs)]
            self._smooth_alloc(mb, srcs[0].shape[1])
            self._smooth_bufs_gather = None
        key = tuple(s.data_ptr() for s in srcs)
        if self._smooth_bufs_gather is None or self._smooth_bufs_gather[0] != key:
            self._smooth_bufs_gather = (key, self._smooth_gatherer(srcs, self._smooth_bufs))
        gather, bufs = self._smooth_bufs_gather[1], self._smooth_bufs
        indices = torch.randperm(self.num_mini_batches * mb, requires_grad=False, device=self.device)   # RS:63-112: one permutation, reused
        adaptive = self.desired_kl is not None and self.schedule == "adaptive"
        sums = torch.zeros(3, device=self.device)        # value loss, surrogate loss, last KL
        self.num_updates = self.num_learning_epochs * self.num_mini_batches
        for _ in range(self.num_learning_epochs):
            for i in range(self.num_mini_batches):
                gather(indices[i * mb:(i + 1) * mb])
                if self._device_lr:
                    self._minibatch_step(bufs, sums)
                    continue
                surrogate_loss, value_loss, loss, kl_mean = self._losses_smooth(*bufs)
                if adaptive:
                    self._apply_kl(kl_mean.item())
                if not torch.isfinite(loss):
                    continue
                self.optimizer.zero_grad()
                loss.backward()
                if not torch.isfinite(nn.utils.clip_grad_norm_(self.actor_critic.parameters(), self.max_grad_norm)):
                    continue   # (a gradient whose norm is not finite skips the step too: include/grx_ppo.h grx_ppo_step_tail)
                self.optimizer.step()
                sums[0] += value_loss.detach(); sums[1] += surrogate_loss.detach()
        host = sums.tolist()
        if self._device_lr:
            self.mean_kl = host[2]
            self.learning_rate = float(self._lr_t.item())
        return host[0] / self.num_updates, host[1] / self.num_updates

    # ------------------------------------------------------------------ the Lipschitz gradient penalty (rl/grad_penalty.py)
    def _losses_gp(self, obs, cobs, actions, target_values, advantages, returns, old_logp, old_mu, old_sigma):
        """_losses with the actor run by rl.grad_penalty.GradPenalty: mu bit-equal to the actor's own, P = mean_r ||d logp_r / d obs_r||^2 of
        the stored actions beside it, and grad_penalty_coef * P joins the loss.  The PPO gradient arriving at mu and the penalty's gradient
        go down the actor in that function's one backward."""
        from .grad_penalty import grad_penalty
        ac = self.actor_critic
        sigma = _noise_std(ac)
        pen = []

        def actor(x):
            mu, P = grad_penalty(ac.actor, x, actions, sigma)
            pen.append(P)
            return mu
        mu, value = self._forward(obs, cobs, actor=actor)
        if not self._loss_is_fused():   # (the torch spelling in _loss_terms reads sigma from the distribution)
            ac.distribution = torch.distributions.Normal(mu, mu * 0.0 + sigma, validate_args=False)
        surrogate_loss, value_loss, loss, kl_mean = self._loss_terms(mu, value, actions, target_values, advantages, returns,
                                                                     old_logp, old_mu, old_sigma)
        loss = loss + self.grad_penalty_coef * pen[0]
        with torch.no_grad():   # (a step the NaN-skip drops adds nothing, as with the other statistics)
            P = pen[0].detach().reshape(1)
            self._gp_sum += torch.where(torch.isfinite(loss.detach()).reshape(1), P, torch.zeros_like(P))
        return surrogate_loss, value_loss, loss, kl_mean

    def _update_gp(self):
        """update() with the gradient penalty on: the captured step, the eager device one or the CPU one below, on the plain minibatch"""
        self._gp_sum.zero_()
        if self._device_lr:
            with self._blas_for_update():
                out = self._update_graphed() if self._use_graph else self._update_device()
        else:
            out = self._update_gp_cpu()
        self.mean_grad_penalty = float(self._gp_sum.item()) / self.num_updates   # one extra 4-byte read-back per update
        return out

    def _update_gp_cpu(self):
        """update()'s CPU loop -- host-side adaptive learning rate, NaN-skip, clip and Adam -- around _losses_gp"""
        adaptive = self.desired_kl is not None and self.schedule == "adaptive"
        mean_value_loss, mean_surrogate_loss = 0.0, 0.0
        for (obs, cobs, actions, target_values, advantages, returns, old_logp, old_mu, old_sigma, _, _) in \
                self.storage.mini_batch_generator(self.num_mini_batches, self.num_learning_epochs):
            surrogate_loss, value_loss, loss, kl_mean = self._losses_gp(obs, cobs, actions, target_values, advantages, returns,
                                                                        old_logp, old_mu, old_sigma)
            if adaptive:
                self._apply_kl(kl_mean.item())
            if not torch.isfinite(loss):
                continue
            self.optimizer.zero_grad()
            loss.backward()
            if not torch.isfinite(nn.utils.clip_grad_norm_(self.actor_critic.parameters(), self.max_grad_norm)):
                continue   # (a gradient whose norm is not finite skips the step too: include/grx_ppo.h grx_ppo_step_tail)
            self.optimizer.step()
            mean_value_loss += value_loss.item()
            mean_surrogate_loss += surrogate_loss.item()
        self.num_updates = self.num_learning_epochs * self.num_mini_batches
        return mean_value_loss / self.num_updates, mean_surrogate_loss / self.num_updates

    # ------------------------------------------------------------------ multi-critic PPO (rl/multi_critic.py)
    def _mc_batches(self):
        """the minibatches with the K-wide values / returns in the scalar columns' places"""
        return self.multi_critic.mini_batch_generator(self.storage, self.num_mini_batches, self.num_learning_epochs)

    def _update_mc(self):
        """update() with reward groups on: the captured step, the eager device one or the CPU one below, on the plain minibatch"""
        mc = self.multi_critic
        mc.head_sum.zero_()
        if self._device_lr:
            with self._blas_for_update():
                out = self._update_graphed() if self._use_graph else self._update_device()
        else:
            out = self._update_mc_cpu()
        mc.mean_head_losses = [h / self.num_updates for h in mc.head_sum.tolist()]   # one extra 4 K-byte read-back per update
        return out

    def _update_mc_cpu(self):
        """update()'s CPU loop -- host-side adaptive learning rate, NaN-skip, clip and Adam -- on the K-wide minibatches"""
        adaptive = self.desired_kl is not None and self.schedule == "adaptive"
        mean_value_loss, mean_surrogate_loss = 0.0, 0.0
        for (obs, cobs, actions, target_values, advantages, returns, old_logp, old_mu, old_sigma, _, _) in self._mc_batches():
            surrogate_loss, value_loss, loss, kl_mean = self._losses(obs, cobs, actions, target_values, advantages, returns,
                                                                     old_logp, old_mu, old_sigma)
            if adaptive:
                self._apply_kl(kl_mean.item())
            if not torch.isfinite(loss):
                continue
            self.optimizer.zero_grad()
            loss.backward()
            if not torch.isfinite(nn.utils.clip_grad_norm_(self.actor_critic.parameters(), self.max_grad_norm)):
                continue   # (a gradient whose norm is not finite skips the step too: include/grx_ppo.h grx_ppo_step_tail)
            self.optimizer.step()
            mean_value_loss += value_loss.item()
            mean_surrogate_loss += surrogate_loss.item()
        self.num_updates = self.num_learning_epochs * self.num_mini_batches
        return mean_value_loss / self.num_updates, mean_surrogate_loss / self.num_updates

    def _update_beta_cpu(self):
        """update()'s CPU loop -- host-side adaptive learning rate, NaN-skip, clip and Adam -- around _losses for a Beta policy"""
        adaptive = self.desired_kl is not None and self.schedule == "adaptive"
        mean_value_loss, mean_surrogate_loss = 0.0, 0.0
        for (obs, cobs, actions, target_values, advantages, returns, old_logp, old_mu, old_sigma, _, _) in \
                self.storage.mini_batch_generator(self.num_mini_batches, self.num_learning_epochs):
            surrogate_loss, value_loss, loss, kl_mean = self._losses(obs, cobs, actions, target_values, advantages, returns,
                                                                     old_logp, old_mu, old_sigma)
            if adaptive:
                self._apply_kl(kl_mean.item())
            if not torch.isfinite(loss):
                continue
            self.optimizer.zero_grad()
            loss.backward()
            if not torch.isfinite(nn.utils.clip_grad_norm_(self.actor_critic.parameters(), self.max_grad_norm)):
                continue   # (a gradient whose norm is not finite skips the step too: include/grx_ppo.h grx_ppo_step_tail)
            self.optimizer.step()
            mean_value_loss += value_loss.item()
            mean_surrogate_loss += surrogate_loss.item()
        self.num_updates = self.num_learning_epochs * self.num_mini_batches
        return mean_value_loss / self.num_updates, mean_surrogate_loss / self.num_updates

    def _update_device(self):
        """Same arithmetic as update(), no host round-trips inside the minibatch loop."""
        ac, multi = self.actor_critic, _collective_path()
        adaptive = self.desired_kl is not None and self.schedule == "adaptive"
        sums = torch.zeros(3, device=self.device)        # value loss, surrogate loss, last KL
        losses = self._losses if self.grad_penalty_coef is None else self._losses_gp
        batches = self._mc_batches() if self.multi_critic is not None else \
            self.storage.mini_batch_generator(self.num_mini_batches, self.num_learning_epochs)
        for (obs, cobs, actions, target_values, advantages, returns, old_logp, old_mu, old_sigma, _, _) in batches:
            surrogate_loss, value_loss, loss, kl_mean = losses(obs, cobs, actions, target_values, advantages, returns,
                                                               old_logp, old_mu, old_sigma)
            if multi:
                self._zero_flat_grads()
            else:
                self.optimizer.zero_grad(set_to_none=False)
            loss.backward()
            if not multi and self._step_tail(loss, kl_mean, value_loss, surrogate_loss, sums, adaptive):
                continue
            with torch.no_grad():
                bad = ~torch.isfinite(loss)
                if multi:
                    kl_mean, bad = self._sync_gradients(kl_mean, bad)
                    bad = bad | ~torch.isfinite(self._bucket[:self._nflat]).all()
            if multi and self._step_tail(value_loss, kl_mean, value_loss, surrogate_loss, sums, adaptive, bad_flag=bad.float()):
                continue
            if adaptive:
                self._device_lr_update(kl_mean)
            bad = self._clip_found_inf(bad)
            self.optimizer.step()
            with torch.no_grad():
                sums[0] += torch.where(bad, 0.0, value_loss.detach())   # (a skipped step adds nothing, also when its losses are NaN: NaN * 0 is NaN)
                sums[1] += torch.where(bad, 0.0, surrogate_loss.detach())
                sums[2] = kl_mean
        self.num_updates = self.num_learning_epochs * self.num_mini_batches
        host = sums.tolist()                           # the only device->host transfer of the update
        self.mean_kl = host[2]
        self.learning_rate = float(self._lr_t.item())
        return host[0] / self.num_updates, host[1] / self.num_updates

    # ------------------------------------------------------------------ HIP-graph minibatch step
    def _minibatch_step(self, batch, sums):
        """One PPO minibatch step on static tensors (the arithmetic of _update_device)."""
        obs, cobs, actions, target_values, advantages, returns, old_logp, old_mu, old_sigma = batch
        adaptive = self.desired_kl is not None and self.schedule == "adaptive"
        losses = self._losses if self.symmetry is None else self._losses_sym
        if self.smooth is not None:   # (the actor's input has R mb rows; the pairs' valid bytes are a static buffer beside the batch)
            losses = self._losses_smooth
        if self.grad_penalty_coef is not None:   # (the same nine tensors: the penalty reads the actor's input and the stored actions)
            losses = self._losses_gp
        surrogate_loss, value_loss, loss, kl_mean = losses(obs, cobs, actions, target_values, advantages, returns,
                                                           old_logp, old_mu, old_sigma)
        # grads dropped, not zero-filled: backward then WRITES each .grad (from the graph's private pool on replay) instead of
        # accumulating into a zeroed one -- one fill and one add kernel less per parameter and step (GRX_PPO_GRAD_NONE=0: fill)
        self.optimizer.zero_grad(set_to_none=os.environ.get("GRX_PPO_GRAD_NONE", "1") != "0")
        loss.backward()
        if self._step_tail(loss, kl_mean, value_loss, surrogate_loss, sums, adaptive):
            return
        if adaptive:
            self._device_lr_update(kl_mean)
        bad = self._clip_found_inf(~torch.isfinite(loss.detach()))
        self.optimizer.step()
        with torch.no_grad():
            sums[0] += torch.where(bad, 0.0, value_loss.detach())   # (a skipped step adds nothing, also when its losses are NaN: NaN * 0 is NaN)
            sums[1] += torch.where(bad, 0.0, surrogate_loss.detach())
            sums[2] = kl_mean

    def _clip_found_inf(self, bad):
        """clip_grad_norm_, then the NaN-skip (ppo.py:297-299) without a sync: the fused Adam kernel leaves parameters, moments and step
        counters untouched when found_inf is set (the GradScaler hook).  A step is skipped when `bad` (a non-finite loss) or when the
        gradients' total norm, which clip_grad_norm_ returns, is not finite -- the rule of grx_ppo_step_tail (include/grx_ppo.h) and of the
        multi-rank paths; torch alone would step on NaN or zeroed gradients there.  Returns the decision, for the statistics."""
        total_norm = nn.utils.clip_grad_norm_(self.actor_critic.parameters(), self.max_grad_norm, foreach=True)
        with torch.no_grad():
            bad = bad | ~torch.isfinite(total_norm)
            self.optimizer.found_inf = bad.float().reshape(())
            self.optimizer.grad_scale = None
        return bad

    def _step_tail(self, loss, kl_mean, value_loss, surrogate_loss, sums, adaptive, bad_flag=None):
        """Adaptive learning rate, NaN-skip, clip_grad_norm_, Adam.step() and the update's statistics through libgrx_ppo.so (two launches);
        False: not available here (GRX_PPO_FUSED_TAIL=0, an optimizer configuration it does not cover) -- the caller runs the torch tail."""
        if not self._fused_tail:
            return False
        if self._tail is None:
            from .fused_loss import StepTail
            if not StepTail.supported(self.optimizer, self._params) or any(p.grad is None for p in self._params):
                self._fused_tail = False
                return False
            self._tail = StepTail(self.optimizer, self._params, self._lr_t)
        with torch.no_grad():
            self._tail(loss.detach(), kl_mean.detach(), value_loss.detach(), surrogate_loss.detach(), sums, adaptive, self.desired_kl,
                       self.learning_rate_min, self.learning_rate_max, self.max_grad_norm, bad_flag=bad_flag)
        return True

    # ... and with more than one rank the step is captured as TWO halves around the one eager RCCL all-reduce:
    #   front  = zero the flat bucket, forward, fused loss, backward (accumulating into the bucket's views), KL and the
    #            non-finite flag into the bucket's tail
    #   (dist.all_reduce(bucket) -- enqueued on the same stream between the two replays; no host synchronisation)
    #   back   = average, adaptive learning rate from the AVERAGED KL, collective NaN-skip, clip, fused Adam, statistics
    def _mb_front(self, batch):
        obs, cobs, actions, target_values, advantages, returns, old_logp, old_mu, old_sigma = batch
        surrogate_loss, value_loss, loss, kl_mean = self._losses(obs, cobs, actions, target_values, advantages, returns,
                                                                  old_logp, old_mu, old_sigma)
        self._zero_flat_grads()
        loss.backward()
        with torch.no_grad():
            b, n = self._bucket, self._nflat
            b[n] = kl_mean
            b[n + 1] = (~torch.isfinite(loss)).float()
            self._mid[0] = value_loss.detach()
            self._mid[1] = surrogate_loss.detach()

    def _mb_back(self, sums):
        adaptive = self.desired_kl is not None and self.schedule == "adaptive"
        b, n = self._bucket, self._nflat
        with torch.no_grad():
            b /= _world()
            kl_mean = b[n]
            bad = (b[n + 1] > 0) | ~torch.isfinite(b[:n]).all()
        if self._step_tail(self._mid[0], kl_mean, self._mid[0], self._mid[1], sums, adaptive, bad_flag=bad.float()):
            return   # (the collective NaN decision travels as the flag; _mid[0], the value loss, stands in for the total loss: not finite -> bad anyway)
        if adaptive:
            self._device_lr_update(kl_mean)
        with torch.no_grad():
            self.optimizer.found_inf = bad.float().reshape(())
            self.optimizer.grad_scale = None
        nn.utils.clip_grad_norm_(self.actor_critic.parameters(), self.max_grad_norm, foreach=True)
        self.optimizer.step()
        with torch.no_grad():
            sums[0] += torch.where(bad, 0.0, self._mid[0])   # (a skipped step adds nothing, also when its losses are NaN: NaN * 0 is NaN)
            sums[1] += torch.where(bad, 0.0, self._mid[1])
            sums[2] = kl_mean

    def _build_graph(self, mb):
        st, dev = self.storage, self.device
        widths = [st.observations.shape[-1], (st.pri_observations if st.pri_observations is not None else st.observations).shape[-1],
                  st.actions.shape[-1], 1, 1, 1, 1, st.mu.shape[-1], st.sigma.shape[-1]]
        if self.multi_critic is not None:   # (the stored values and the returns are K wide)
            widths[3] = widths[5] = self.multi_critic.K
        rows = [mb] * len(widths) if self.symmetry is None else [mb * (2 if m else 1) for m in self._sym_modes]   # (symmetry: the mirrored half behind)
        if self.smooth is not None:   # (smoothness: the successor / perturbed rows behind the actor's input, eps and valid beside the batch)
            rows[0] = mb * self._smooth_rows()
            self._smooth_alloc(mb, widths[0])
        self._static = [torch.zeros(r, w, device=dev) for r, w in zip(rows, widths)]
        self._sums = torch.zeros(3, device=dev)
        # warm-up runs real optimizer steps (allocator / lazy-state initialisation): snapshot and restore everything they touch
        ac_state = [p.detach().clone() for p in self.actor_critic.parameters()]   # (not load_state_dict: it rewrites std, AC:116-134)
        lr0 = self._lr_t.clone()
        self._static[8].fill_(1.0)   # sigma > 0 for the dry runs
        if self._beta:   # (x inside the box, alpha = beta = 1 likewise)
            self._static[2].fill_(0.5); self._static[7].fill_(1.0)
        # The GEMM kernels are chosen when the graph is captured.  For these shapes (batch ~10^4 rows, 39..512 columns,
        # fp32) rocBLAS's choices beat hipBLASLt's by 2x on the weight-gradient products dY^T X (27-48 us against
        # 66-73 us, tools/gpu_gemm_probe.py).  The preference is process-global in torch, so it is switched for the
        # dry runs (the library initialises itself there, outside the capture) and the capture only, then put back.
        prev_blas = torch.backends.cuda.preferred_blas_library()
        if os.environ.get("GRX_PPO_BLAS", "rocblas") == "rocblas":
            torch.backends.cuda.preferred_blas_library("cublas")
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        multi = _collective_path()
        with torch.cuda.stream(side):
            for _ in range(3):
                if multi:   # (every rank builds its graphs at the same point of the run: the dry-run collectives pair up)
                    self._mb_front(self._static)
                    dist.all_reduce(self._bucket)
                    self._mb_back(self._sums)
                else:
                    self._minibatch_step(self._static, self._sums)
        torch.cuda.current_stream(dev).wait_stream(side)
        if os.environ.get("GRX_PPO_GRAPH", "1") == "2":   # debugging aid: static buffers, eager replay
            class _Eager:
                def __init__(s, fn): s.fn = fn
                def replay(s): s.fn()
            if multi:
                self._graph = _Eager(lambda: self._mb_front(self._static))
                self._graph_back = _Eager(lambda: self._mb_back(self._sums))
            else:
                self._graph = _Eager(lambda: self._minibatch_step(self._static, self._sums))
        elif multi:
            self._graph, self._graph_back = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            with _graph_capture(self._graph, side):
                self._mb_front(self._static)
            with _graph_capture(self._graph_back, side):
                self._mb_back(self._sums)
        else:
            self._graph = torch.cuda.CUDAGraph()
            # capture on the stream the dry runs used: autograd's AccumulateGrad nodes remember the stream they were
            # created on, and one that differs from the capture stream runs (and allocates) outside the capture
            with _graph_capture(self._graph, side):
                self._minibatch_step(self._static, self._sums)
        torch.backends.cuda.preferred_blas_library(prev_blas)
        # restore: parameters, Adam moments/step counters, learning rate
        with torch.no_grad():
            for p, v in zip(self.actor_critic.parameters(), ac_state):
                p.copy_(v)
        for stt in self.optimizer.state.values():
            for v in stt.values():
                if torch.is_tensor(v):
                    v.zero_()
        self._lr_t.copy_(lr0)
        if self._restore_opt is not None:
            self._load_opt_tensors(self._restore_opt)
        self._graph_mb = mb

    def _opt_tensors(self):
        return [{k: v.clone() for k, v in stt.items() if torch.is_tensor(v)} for stt in self.optimizer.state.values()]

    def _load_opt_tensors(self, saved):
        for stt, sv in zip(self.optimizer.state.values(), saved):
            for k, v in sv.items():
                stt[k].copy_(v)

    def _ensure_update_graph(self):
        st = self.storage
        mb = st.num_envs * st.num_transitions_per_env // self.num_mini_batches
        if self._graph is None or self._graph_mb != mb:
            # capture after the optimizer already ran (resume / later iterations): keep its moments
            self._restore_opt = self._opt_tensors() if len(self.optimizer.state) else None
            with self._blas_for_update():
                self._build_graph(mb)
        return mb

    def _update_graphed(self):
        mb = self._ensure_update_graph()
        st = self.storage
        flat = lambda x: x.flatten(0, 1)
        cobs = st.pri_observations if st.pri_observations is not None else st.observations
        srcs = [flat(x) for x in (st.observations, cobs, st.actions, st.values, st.advantages, st.returns, st.actions_log_prob, st.mu, st.sigma)]
        if self.multi_critic is not None:   # (the two K-wide tensors in the scalar value and return columns' places)
            srcs[3], srcs[5] = flat(self.multi_critic.values), flat(self.multi_critic.returns)
            self.multi_critic.head_sum.zero_()   # (the dry runs of a capture added to it)
        indices = torch.randperm(self.num_mini_batches * mb, requires_grad=False, device=self.device)   # RS:63-112: one permutation, reused
        self._sums.zero_()
        if self.symmetry is not None:
            self._sym_sum.zero_()   # (the dry runs of a capture added to it)
        if self.smooth is not None:
            self._smooth_sum.zero_()   # (likewise)
        if self.grad_penalty_coef is not None:
            self._gp_sum.zero_()   # (likewise)
        multi = _collective_path()
        gather = None
        if self._fused_store:   # (libgrx_ppo.so is in use)
            key = tuple(s.data_ptr() for s in srcs) + tuple(b.data_ptr() for b in self._static)
            if getattr(self, "_gather_key", None) != key:
                from .fused_loss import RowGather
                if self.smooth is not None:
                    self._gather, self._gather_key = self._smooth_gatherer(srcs, self._static), key
                else:
                    self._gather, self._gather_key = (RowGather(srcs, self._static) if self.symmetry is None else self._sym_gatherer(srcs, self._static)), key
            gather = self._gather
        elif self.symmetry is not None:
            gather = self._sym_gatherer(srcs, self._static)
        elif self.smooth is not None:
            gather = self._smooth_gatherer(srcs, self._static)
        for _ in range(self.num_learning_epochs):
            for i in range(self.num_mini_batches):
                idx = indices[i * mb:(i + 1) * mb]
                if gather is not None:
                    gather(idx)   # the nine minibatch tensors in one launch
                else:
                    for buf, src in zip(self._static, srcs):
                        torch.index_select(src, 0, idx, out=buf)
                self._graph.replay()
                if multi:
                    dist.all_reduce(self._bucket)
                    self._graph_back.replay()
        self.num_updates = self.num_learning_epochs * self.num_mini_batches
        host = self._sums.tolist()                     # the only device->host transfer of the update
        self.mean_kl = host[2]
        self.learning_rate = float(self._lr_t.item())
        return host[0] / self.num_updates, host[1] / self.num_updates

    def _apply_kl(self, kl_value):
        self.mean_kl = kl_value
        self.update_learning_rate(kl_value)
        for g in self.optimizer.param_groups:
            g["lr"] = self.learning_rate

    def load_optimizer_state(self, state_dict):
        """optimizer.load_state_dict() for the device-resident update.  torch replaces param_groups[*]['lr'] with a NEW tensor
        (or, from a reference rsl_rl checkpoint, a float with capturable=False / fused=None): the adaptive learning rate would
        then be written to an orphaned `_lr_t`, the NaN-skip hook ignored, and graphs captured earlier would keep updating the
        old Adam moments.  Re-attach `_lr_t`, force the fused capturable configuration, move the step counters to the device
        and drop every captured graph."""
        self.optimizer.load_state_dict(state_dict)
        if self._device_lr:
            lr = self.optimizer.param_groups[0]["lr"]
            with torch.no_grad():
                self._lr_t.copy_(torch.as_tensor(float(lr), device=self.device))
            for g in self.optimizer.param_groups:
                g["lr"] = self._lr_t
                g["fused"], g["capturable"], g["foreach"] = True, True, False
            for stt in self.optimizer.state.values():
                for k, v in list(stt.items()):
                    if torch.is_tensor(v) and (v.device != self._lr_t.device or (k == "step" and v.dtype != torch.float32)):
                        stt[k] = v.to(device=self.device, dtype=torch.float32 if k == "step" else v.dtype)
                    elif k == "step" and not torch.is_tensor(v):
                        stt[k] = torch.tensor(float(v), device=self.device)
            self.learning_rate = float(lr)
        else:
            self.learning_rate = float(self.optimizer.param_groups[0]["lr"])
        self.invalidate_graphs()

    def prepare_graphs(self, actor_observations, critic_observations):
        """Capture now the graphs act() and update() would capture on first use.  Their warm-up runs draw from torch's CUDA generator
        (the policy's action noise); an exact resume captures them first and sets the generator to the saved state afterwards
        (OnPolicyRunner.load_train_state)."""
        if self._use_act_graph and actor_observations.is_cuda:
            self._ensure_act_graph(actor_observations, critic_observations)
        if self._use_graph and self.storage is not None:
            self._ensure_update_graph()

    def get_train_state(self):
        """What update() carries from one iteration to the next besides parameters and Adam state: the adaptive learning rate
        (host value and the device scalar Adam reads), the last mean KL and the precision."""
        return {"learning_rate": float(self.learning_rate), "mean_kl": float(self.mean_kl), "precision": self.precision,
                "lr_t": self._lr_t.detach().cpu().clone() if self._device_lr else None}

    def set_train_state(self, state):
        if state["precision"] != self.precision:
            raise ValueError(f"PPO: the training state was saved with precision={state['precision']!r}, this PPO runs {self.precision!r}")
        self.learning_rate, self.mean_kl = state["learning_rate"], state["mean_kl"]
        if self._device_lr:
            with torch.no_grad():
                self._lr_t.copy_(state["lr_t"].to(self._lr_t.device))   # (in place: Adam's param group and captured graphs read this tensor)
        else:
            for g in self.optimizer.param_groups:
                g["lr"] = self.learning_rate

    def invalidate_graphs(self):
        """captured policy / minibatch graphs refer to the tensors they were captured with: recapture on next use"""
        self._graph, self._graph_back, self._graph_mb, self._static, self._restore_opt = None, None, None, None, None
        self._act_graph, self._act_key, self._critic_pending = None, None, False

    def clear_storage(self):
        self.storage.clear()
