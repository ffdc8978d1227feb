"""Teacher-student policy distillation (humanoid-gym / Isaac Lab / rsl_rl 2.x `Distillation` + `StudentTeacher`): a
student that reads deployable frames is rolled out, and its mean action is regressed on the mean action a frozen teacher takes on its
own (usually privileged) stream -- DAgger.

    act(obs, teacher_obs):   actions = student(obs) + std * eps      (std: a fixed tensor, not trained)
                             labels  = teacher(teacher_obs)
    process_env_step:        the storage row of this step keeps (obs, labels, dones); rewards only feed the episode bookkeeping
    update():                ONE randperm over the T x N rows, reused by every epoch; per minibatch: student forward, behaviour loss,
                             backward, clip_grad_norm_, Adam at a fixed learning rate; a non-finite loss skips the step
    behaviour loss:          torch's mse_loss or huber_loss (delta 1), reduction="mean" over all batch x actions elements

The loss (with its gradient) and the per-step store are one HIP entry point each (include/grx_ppo.h grx_distill_loss /
grx_distill_store) for contiguous fp32 tensors on a HIP device; their torch spellings below serve CPU tensors and strided input, and
GRX_DISTILL_FUSED=0 forces them on the device too.  Nothing here is captured in a HIP graph: the step runs eagerly, without host
synchronisation inside the minibatch loop (the mean behaviour loss is read back once per update).

A recurrent student (`--student_recurrent`, StudentTeacherRecurrent) has an LSTM over single frames in front of its MLP:
    act():      at the rollout's step 0 the memory's state goes to the storage (h0, c0); one cell launch, then the MLP on h
    update():   truncated back-propagation through time -- windows of `gradient_length` steps over contiguous env ranges, the state
                carried from window to window as data, one optimizer step per (range, window); the backward's per-step chain is one
                launch (rl.recurrent.LSTMSequenceBPTT, include/grx_ppo_bptt.h grx_lstm_bptt_step)"""
import contextlib
import ctypes as C
import os

import torch
import torch.distributed as dist
import torch.nn as nn
import torch.nn.functional as F
import torch.optim as optim

from .fused_loss import RowGather, StepTail, load_ppo_library, mlp_can_fuse, mlp_forward, policy_act
from .modules import MLP

LOSSES = ("mse", "huber")


def _fused_enabled():
    return os.environ.get("GRX_DISTILL_FUSED", "1") != "0"


def _hip_ok(*tensors):
    return all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in tensors)


_SAME_DEVICE = contextlib.nullcontext()


def _device(dev):
    """torch.cuda.device(dev), or nothing when dev is the current device already (the context manager costs more than the launch)"""
    return _SAME_DEVICE if torch.cuda.current_device() == dev.index else torch.cuda.device(dev)


# ---- the behaviour loss ----------------------------------------------------------------------------------------------------------
def distill_loss_torch(student_mu, teacher_mu, loss_type="mse"):
    """the definition: torch's own loss, mean over every element"""
    if loss_type == "mse":
        return F.mse_loss(student_mu, teacher_mu, reduction="mean")
    if loss_type == "huber":
        return F.huber_loss(student_mu, teacher_mu, reduction="mean", delta=1.0)
    raise ValueError(f"distillation loss must be one of {LOSSES}, not {loss_type!r}")


class FusedDistillLoss(torch.autograd.Function):
    """(student_mu [B, A], teacher_mu [B, A]) -> the mean behaviour loss (0-dim); backward hands out grx_distill_loss's gradient"""

    _sizes = {}   # (batch, A) -> floats of scratch: the minibatch shape of a run is fixed, the step is bound by the host's enqueue

    @staticmethod
    def forward(ctx, student_mu, teacher_mu, huber):
        lib = load_ppo_library()
        B, A = student_mu.shape
        size = FusedDistillLoss._sizes.get((B, A))
        if size is None:
            size = FusedDistillLoss._sizes[(B, A)] = lib.grx_distill_loss_partials_size(B, A)
        if size < 1:
            raise RuntimeError(f"grx_distill_loss_partials_size: invalid shape {B} x {A}")
        dev = student_mu.device
        out = torch.empty(1, device=dev, dtype=torch.float32)
        d_mu = torch.empty_like(student_mu)
        partials = torch.empty(size, device=dev, dtype=torch.float32)
        with _device(dev):
            rc = lib.grx_distill_loss(B, A, student_mu.data_ptr(), teacher_mu.data_ptr(), int(bool(huber)), out.data_ptr(), d_mu.data_ptr(),
                                      partials.data_ptr(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        if rc != 0:
            raise RuntimeError(f"grx_distill_loss failed ({rc}): batch {B}, num_actions {A}")
        ctx.save_for_backward(d_mu)
        return out.reshape(())

    @staticmethod
    def backward(ctx, g):
        d_mu, = ctx.saved_tensors
        return d_mu * g, None, None


def distill_loss(student_mu, teacher_mu, loss_type="mse", fused=True):
    """the mean behaviour loss: grx_distill_loss for contiguous fp32 [B, A] tensors on a HIP device, the torch spelling otherwise"""
    if loss_type not in LOSSES:
        raise ValueError(f"distillation loss must be one of {LOSSES}, not {loss_type!r}")
    if fused and student_mu.dim() == 2 and student_mu.shape == teacher_mu.shape and _hip_ok(student_mu, teacher_mu):
        return FusedDistillLoss.apply(student_mu, teacher_mu, loss_type == "huber")
    return distill_loss_torch(student_mu, teacher_mu, loss_type)


# ---- the storage and the per-step store --------------------------------------------------------------------------------------------
class DistillStorage:
    """(T, N, .) rows of one rollout: what the student acted on, the teacher's labels, the dones"""

    def __init__(self, num_envs, num_transitions_per_env, obs_dim, num_actions, device):
        T, N = int(num_transitions_per_env), int(num_envs)
        self.observations = torch.zeros(T, N, int(obs_dim), device=device)
        self.labels = torch.zeros(T, N, int(num_actions), device=device)
        self.dones = torch.zeros(T, N, 1, device=device, dtype=torch.uint8)
        self.num_transitions_per_env, self.num_envs, self.step, self.device = T, N, 0, device

    def clear(self):
        self.step = 0


def store_torch(storage, step, obs, labels, dones, rewards=None, log=None):
    """the definition of one step's store: the three rows of `step`, and -- log = (cur_rew, cur_len, done_rew_row, done_len_row) -- the
    runner's running episode reward / length (the torch spelling in PPO.process_env_step)"""
    if log is not None:
        cur_rew, cur_len, done_rew, done_len = log
        cur_rew += rewards; cur_len += 1
        d = dones.reshape(-1) != 0
        done_rew.copy_(torch.where(d, cur_rew, done_rew)); done_len.copy_(torch.where(d, cur_len, done_len))   # (untouched elsewhere)
        cur_rew.masked_fill_(d, 0.0); cur_len.masked_fill_(d, 0.0)   # (+0, as the kernel writes it: `x *= ~d` leaves -0 for a negative sum)
    storage.observations[step].copy_(obs)
    storage.labels[step].copy_(labels)
    storage.dones[step].copy_((dones != 0).view(-1, 1))


def _as_u8(t):
    """one byte per env: bool is reinterpreted, any other dtype converted (fused_loss.store_transition's rule)"""
    if t.dtype == torch.bool:
        return t.view(torch.uint8)
    if t.dtype != torch.uint8:
        return (t != 0).to(torch.uint8)
    return t


def store_hip(storage, step, obs, labels, dones, rewards=None, log=None):
    """the same through grx_distill_store: one launch"""
    lib = load_ppo_library()
    N = storage.num_envs
    d8 = _as_u8(dones)
    if not (d8.is_cuda and d8.is_contiguous() and d8.numel() == N):
        raise RuntimeError("grx_distill_store needs contiguous CUDA dones with one entry per env")
    if tuple(obs.shape) != tuple(storage.observations.shape[1:]) or tuple(labels.shape) != tuple(storage.labels.shape[1:]):
        raise RuntimeError(f"grx_distill_store: rows {tuple(obs.shape)} / {tuple(labels.shape)} do not fit the storage")
    if not 0 <= step < storage.num_transitions_per_env:
        raise AssertionError("Rollout buffer overflow")
    ptr = lambda t: t.data_ptr() if t is not None else None
    lg = log if log is not None else (None, None, None, None)
    if log is not None and not (_hip_ok(rewards, *log) and all(t.numel() == N for t in (rewards, *log))):
        raise RuntimeError("grx_distill_store needs contiguous float32 CUDA rewards and logging arrays with one entry per env")
    with _device(obs.device):
        rc = lib.grx_distill_store(N, obs.shape[1], labels.shape[1], ptr(obs), ptr(labels), ptr(rewards) if log is not None else None, ptr(d8),
                                   ptr(storage.observations[step]), ptr(storage.labels[step]), ptr(storage.dones[step]),
                                   ptr(lg[0]), ptr(lg[1]), ptr(lg[2]), ptr(lg[3]), C.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream))
    if rc != 0:
        raise RuntimeError(f"grx_distill_store failed ({rc})")


# ---- the teacher, read from a PPO checkpoint -----------------------------------------------------------------------------------------
def read_teacher(loaded, path, num_obs, num_pri_obs, num_actions):
    """What a checkpoint says about the policy it holds: the stream its actor reads ("privileged" with `privileged_actor`, else "actor"),
    that stream's history length, frame width and frozen normaliser statistics (or None), the actor's hidden sizes (from the shapes of
    actor.model.*.weight) and its tensors.  ValueError when the actor's first layer does not fit history x frame width."""
    sd = loaded["model_state_dict"]
    if bool((loaded.get("noise") or {}).get("state_dependent", False)):
        raise ValueError(f"{path} was trained with --state_dependent_std: --distill_from and --state_dependent_std exclude each other, a "
                         "teacher whose output layer is [mean | s] is not implemented")
    layers = sorted((int(k.split(".")[2]), k) for k in sd if k.startswith("actor.model.") and k.endswith(".weight"))
    if not layers:
        raise ValueError(f"{path} holds no actor (no actor.model.*.weight in its model_state_dict)")
    shapes = [tuple(sd[k].shape) for _, k in layers]
    privileged = bool(loaded.get("privileged_actor", False))
    hist = loaded.get("obs_history", {"actor": 1, "critic": 1})
    length = int(hist["critic" if privileged else "actor"])
    frame = num_pri_obs if privileged else num_obs
    if frame is None:
        raise ValueError(f"{path} was trained with --privileged_actor, this env has no privileged observations")
    width = shapes[0][1]
    if width != length * frame:
        raise ValueError(f"{path}: the teacher's first layer takes {width} inputs, its stream gives {length} frames x {frame} = {length * frame} "
                         f"({'privileged' if privileged else 'actor'} observations of this env)")
    if shapes[-1][0] != num_actions:
        raise ValueError(f"{path}: the teacher has {shapes[-1][0]} actions, this env {num_actions}")
    norm = loaded.get("critic_obs_norm_state_dict" if privileged else "obs_norm_state_dict")
    return {"stream": "privileged" if privileged else "actor", "history": length, "frame": int(frame), "width": int(width),
            "hidden": [s[0] for s in shapes[:-1]], "norm": norm,
            "state": {k[len("actor."):]: v for k, v in sd.items() if k.startswith("actor.")}}


class StudentTeacher(nn.Module):
    """`actor`: the student, an MLP on the runner's actor stream, the only trained part.  `teacher`: a frozen MLP (requires_grad False, always
    in eval mode).  `std`: the rollout's fixed action noise, a buffer.  State dict: actor.*, std, teacher.* -- no critic."""
    is_recurrent = False

    def __init__(self, student_num_input, teacher_num_input, num_actions, actor_hidden_dims=(256, 256, 256), teacher_hidden_dims=(256, 256, 256),
                 activation="elu", noise_std=0.1, **_):
        super().__init__()
        self.num_actor_input, self.num_actor_output, self.num_teacher_input = int(student_num_input), int(num_actions), int(teacher_num_input)
        self.actor = MLP(student_num_input, num_actions, actor_hidden_dims, activation)
        self.teacher = MLP(teacher_num_input, num_actions, teacher_hidden_dims, activation)
        for p in self.teacher.parameters():
            p.requires_grad_(False)
        self.teacher.eval()
        self.register_buffer("std", float(noise_std) * torch.ones(num_actions))

    def load_teacher(self, actor_state):
        """the tensors of a checkpoint's actor (read_teacher(...)["state"]) into the teacher"""
        self.teacher.load_state_dict(actor_state)
        self.teacher.eval()

    def train(self, mode=True):
        super().train(mode)
        self.teacher.eval()   # frozen: whatever mode the student is in
        return self

    def reset(self, dones=None):
        pass

    def forward(self, *a, **k):
        raise NotImplementedError

    def act(self, observations, **_):
        mean = self.actor(observations)
        return mean + self.std * torch.randn_like(mean)

    def act_inference(self, observations):
        return self.actor(observations)

    def evaluate(self, teacher_observations, **_):
        """the label: the teacher's mean action on its own stream"""
        with torch.no_grad():
            return self.teacher(teacher_observations)


class StudentTeacherRecurrent(StudentTeacher):
    """`--student_recurrent` (rsl_rl 2.x `StudentTeacherRecurrent` with an MLP teacher): the student is `memory_a`, one LSTM
    layer of hidden size H over single actor frames, in front of `actor`, an MLP of input width H -- the attribute names
    rl.recurrent.RecurrentPolicy and ExportedRecurrentPolicy read.  The teacher stays the frozen MLP on its own stream.
    State dict: memory_a.rnn.*, actor.*, std, teacher.*"""
    is_recurrent = True

    def __init__(self, student_num_input, teacher_num_input, num_actions, actor_hidden_dims=(256, 256, 256), teacher_hidden_dims=(256, 256, 256),
                 activation="elu", noise_std=0.1, rnn_hidden_size=256, **_):
        from .recurrent import Memory, _MemoryMLP, check_rnn
        H = check_rnn("lstm", 1, rnn_hidden_size)   # (the refusal, before anything is built)
        nn.Module.__init__(self)
        self.num_actor_input, self.num_actor_output, self.num_teacher_input = int(student_num_input), int(num_actions), int(teacher_num_input)
        self.rnn_hidden_size = H
        self.memory_a = Memory(student_num_input, H)
        self.actor = _MemoryMLP(H, num_actions, actor_hidden_dims, activation)
        self.teacher = MLP(teacher_num_input, num_actions, teacher_hidden_dims, activation)
        for p in self.teacher.parameters():
            p.requires_grad_(False)
        self.teacher.eval()
        self.register_buffer("std", float(noise_std) * torch.ones(num_actions))

    def student_parameters(self):
        return list(self.memory_a.parameters()) + list(self.actor.parameters())

    def reset(self, dones=None):
        self.memory_a.reset(dones)

    def act(self, observations, **_):
        mean = self.actor(self.memory_a.step(observations))
        return mean + self.std * torch.randn_like(mean)

    def act_inference(self, observations):
        return self.actor(self.memory_a.step(observations))


class RecurrentDistillStorage(DistillStorage):
    """DistillStorage plus the state the student's memory had before the rollout's first step, [N, H] each, and the update's env ranges
    (rl.recurrent.RecurrentRolloutStorage.env_ranges' rule: contiguous, in order, the tail dropped)"""

    def __init__(self, num_envs, num_transitions_per_env, obs_dim, num_actions, hidden_size, device):
        super().__init__(num_envs, num_transitions_per_env, obs_dim, num_actions, device)
        self.h0 = torch.zeros(self.num_envs, int(hidden_size), device=device)
        self.c0 = torch.zeros(self.num_envs, int(hidden_size), device=device)

    def set_start_state(self, state):
        self.h0.copy_(state[0]); self.c0.copy_(state[1])

    def env_ranges(self, num_mini_batches):
        from .recurrent import RecurrentRolloutStorage
        return RecurrentRolloutStorage.env_ranges(self, num_mini_batches)

    def windows(self, gradient_length):
        """[t0, t1) of every truncated-BPTT window: gradient_length steps each, the last one maybe shorter; 0: the whole rollout"""
        T = self.num_transitions_per_env
        L = T if gradient_length == 0 else min(int(gradient_length), T)
        return [(t0, min(t0 + L, T)) for t0 in range(0, T, L)]


class _Transition:
    def __init__(self):
        self.clear()

    def clear(self):
        self.observations = self.labels = self.actions = None


def _world():
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


class Distillation:
    """The algorithm behind `--distill_from`: PPO's surface for the runner (act, process_env_step, compute_returns, update, storage,
    optimizer), PPO's keyword arguments accepted and -- where distillation has no use for them -- ignored."""

    def __init__(self, actor_critic=None, num_learning_epochs=1, num_mini_batches=1, learning_rate=1e-3, max_grad_norm=1.0, weight_decay=0.0,
                 device="cpu", loss_type="mse", precision="fp32", gradient_length=15, **_):
        if precision != "fp32":
            raise ValueError(f"Distillation: precision={precision!r} is not available, the student trains in fp32")
        if loss_type not in LOSSES:
            raise ValueError(f"Distillation: distill_loss must be one of {LOSSES}, not {loss_type!r}")
        if _world() > 1:
            raise NotImplementedError("Distillation: one process only")
        self.device, self.loss_type, self.precision = device, loss_type, precision
        self.actor_critic = actor_critic.to(device)
        self.num_learning_epochs, self.num_mini_batches = int(num_learning_epochs), int(num_mini_batches)
        self.learning_rate, self.max_grad_norm = float(learning_rate), float(max_grad_norm)
        self.mean_kl, self.num_updates = 0.0, 0
        self.storage, self.transition = None, _Transition()
        self._on_device = torch.device(device).type == "cuda"
        self._fused = self._on_device and _fused_enabled()         # the two grx_distill_* entry points
        # a recurrent student (StudentTeacherRecurrent): the memory's parameters train too, the update is truncated BPTT
        self._recurrent = bool(getattr(self.actor_critic, "is_recurrent", False))
        self.gradient_length = int(gradient_length)
        if self._recurrent and self.gradient_length < 0:
            raise ValueError(f"Distillation: distill_gradient_length must be an integer >= 0 (0: the whole rollout), not {gradient_length!r}")
        self._params = self.actor_critic.student_parameters() if self._recurrent else [p for p in self.actor_critic.actor.parameters()]
        if self._on_device:
            # PPO's device-resident optimizer: the learning rate is a device scalar, the NaN-skip needs no host round trip
            self._lr_t = torch.tensor(self.learning_rate, device=device)
            self.optimizer = optim.Adam(self._params, lr=self._lr_t, weight_decay=weight_decay, fused=True, capturable=True)
        else:
            self._lr_t = None
            self.optimizer = optim.Adam(self._params, lr=self.learning_rate, weight_decay=weight_decay)
        self._use_tail = self._on_device and os.environ.get("GRX_PPO_FUSED_TAIL", "1") != "0"
        self._tail, self._gather, self._gather_key, self._static = None, None, None, None
        self._sums = torch.zeros(3, device=device) if self._on_device else None
        self._zero = torch.zeros((), device=device) if self._on_device else None

    # ---- the rollout -----------------------------------------------------------------------------------------------------------------
    def init_storage(self, num_envs, num_transitions_per_env, **_):
        ac = self.actor_critic
        if self._recurrent:
            self.storage = RecurrentDistillStorage(num_envs, num_transitions_per_env, ac.num_actor_input, ac.num_actor_output, ac.rnn_hidden_size,
                                                   self.device)
            return
        self.storage = DistillStorage(num_envs, num_transitions_per_env, ac.num_actor_input, ac.num_actor_output, self.device)

    def test_mode(self):
        self.actor_critic.eval()

    def train_mode(self):
        self.actor_critic.train()

    def act(self, observations, teacher_observations):
        ac, t = self.actor_critic, self.transition
        if self._recurrent:
            return self._act_recurrent(observations, teacher_observations)
        with torch.no_grad():
            if (self._on_device and ac.num_actor_output <= 32 and mlp_can_fuse(ac.actor, observations)
                    and mlp_can_fuse(ac.teacher, teacher_observations)):
                # libgrx_ppo.so's inference forward: one launch per layer, the student's output layer fused with the sampling
                eps = torch.randn(observations.shape[0], ac.num_actor_output, device=observations.device)
                t.actions = policy_act(ac.actor, ac.std, observations, eps)[0]
                t.labels = mlp_forward(ac.teacher, teacher_observations)
            else:
                t.actions = ac.act(observations).detach()
                t.labels = ac.evaluate(teacher_observations).detach()
        t.observations = observations
        return t.actions

    def _act_recurrent(self, observations, teacher_observations):
        """a recurrent student's step: the memory's state before the rollout's first step goes to the storage, then one cell launch, the
        student's MLP and the sampling on h, the teacher's label on its own stream"""
        ac, t, st = self.actor_critic, self.transition, self.storage
        with torch.no_grad():
            if st.step == 0:
                st.set_start_state(ac.memory_a.start_state(observations.shape[0], observations.device))
            h = ac.memory_a.step(observations)
            if (self._on_device and ac.num_actor_output <= 32 and ac.actor.fusable(h) and mlp_can_fuse(ac.teacher, teacher_observations)):
                eps = torch.randn(h.shape[0], ac.num_actor_output, device=h.device)
                t.actions = policy_act(ac.actor, ac.std, h, eps)[0]
                t.labels = mlp_forward(ac.teacher, teacher_observations)
            else:
                mean = ac.actor(h)
                t.actions = (mean + ac.std * torch.randn_like(mean)).detach()
                t.labels = ac.evaluate(teacher_observations).detach()
        t.observations = observations
        return t.actions

    def act_inference(self, obs):
        return self.actor_critic.act_inference(obs)

    def process_env_step(self, rewards, dones, infos, log=None):
        t, st = self.transition, self.storage
        if st.step >= st.num_transitions_per_env:
            raise AssertionError("Rollout buffer overflow")
        if self._fused and _hip_ok(t.observations, t.labels) and dones.is_cuda:
            d = dones if dones.is_contiguous() else dones.contiguous()
            r = None
            if log is not None:
                r = rewards if _hip_ok(rewards) else rewards.contiguous().float()
            store_hip(st, st.step, t.observations, t.labels, d, r, log)
        else:
            store_torch(st, st.step, t.observations, t.labels, dones, rewards, log)
        st.step += 1
        t.clear()
        self.actor_critic.reset(dones)

    def compute_returns(self, last_teacher_obs):
        pass   # (rewards play no part)

    # ---- the update ------------------------------------------------------------------------------------------------------------------
    @contextlib.contextmanager
    def _blas_for_update(self):
        """rocBLAS for the update's matrix products, as PPO.update() prefers at these shapes (GRX_PPO_BLAS=hipblaslt: left alone)"""
        prev = torch.backends.cuda.preferred_blas_library()
        if os.environ.get("GRX_PPO_BLAS", "rocblas") == "rocblas":
            torch.backends.cuda.preferred_blas_library("cublas")
        try:
            yield
        finally:
            torch.backends.cuda.preferred_blas_library(prev)

    def _step(self, obs, labels):
        """forward, behaviour loss, backward of one minibatch; the gradients are in .grad afterwards"""
        loss = distill_loss(self.actor_critic.actor(obs), labels, self.loss_type, self._fused)
        self.optimizer.zero_grad(set_to_none=False)
        return loss

    def window_batches(self):
        """what a recurrent student's update walks, in order: per env range (a, b) its start state (h0, c0)[a:b] and, per window [t0, t1),
        (observations [t1 - t0, b - a, D], resets [t1 - t0, b - a] uint8, labels [(t1 - t0)(b - a), A]).  resets[t] = dones[t - 1]: a step
        starts from zero where the step before ended an episode; none at the rollout's step 0 (h0 / c0 hold that reset already)"""
        st = self.storage
        resets = torch.zeros(st.num_transitions_per_env, st.num_envs, dtype=torch.uint8, device=st.dones.device)
        resets[1:] = st.dones[:-1, :, 0]
        out = []
        for a, b in st.env_ranges(self.num_mini_batches):
            wins = [(st.observations[t0:t1, a:b].contiguous(), resets[t0:t1, a:b].contiguous(), st.labels[t0:t1, a:b].flatten(0, 1))
                    for t0, t1 in st.windows(self.gradient_length)]
            out.append(((st.h0[a:b].contiguous(), st.c0[a:b].contiguous()), wins))
        return out

    def _update_recurrent(self):
        """truncated back-propagation through time: per epoch and env range the state starts at (h0, c0) and is carried from window to
        window as data -- no gradient, and from the parameters of that moment, as rsl_rl's Distillation carries it --; one optimizer step
        per (range, window)"""
        ac, batches = self.actor_critic, self.window_batches()
        self.num_updates = self.num_learning_epochs * sum(len(wins) for _, wins in batches)
        ctx = self._blas_for_update() if self._on_device else contextlib.nullcontext()
        sums = self._sums.zero_() if self._on_device else None
        total = 0.0
        with ctx:
            for _ in range(self.num_learning_epochs):
                for (h, c), wins in batches:
                    for obs, resets, labels in wins:
                        out, h, c = ac.memory_a.sequence_bptt(obs, resets, h, c)
                        loss = distill_loss(ac.actor(out.flatten(0, 1)), labels, self.loss_type, self._fused)
                        self.optimizer.zero_grad(set_to_none=False)
                        if self._on_device:   # (no host round trip inside the loop)
                            loss.backward()
                            self._tail_step(loss.detach(), sums)
                            continue
                        if not torch.isfinite(loss):
                            continue
                        loss.backward()
                        if not torch.isfinite(nn.utils.clip_grad_norm_(self._params, self.max_grad_norm)):
                            continue
                        self.optimizer.step()
                        total += loss.item()
        return sums[0].item() / self.num_updates if self._on_device else total / self.num_updates

    def update(self):
        if self._recurrent:
            return self._update_recurrent()
        st = self.storage
        mb =st.num_envs * st.num_transitions_per_env // self.num_mini_batches
        obs, labels = st.observations.flatten(0, 1), st.labels.flatten(0, 1)
        indices = torch.randperm(self.num_mini_batches * mb, requires_grad=False, device=self.device)   # one permutation, reused by every epoch
        self.num_updates = self.num_learning_epochs * self.num_mini_batches
        if self._on_device:
            with self._blas_for_update():
                return self._update_device(obs, labels, indices, mb)
        total = 0.0
        for _ in range(self.num_learning_epochs):
            for i in range(self.num_mini_batches):
                idx = indices[i * mb:(i + 1) * mb]
                loss = self._step(obs[idx], labels[idx])
                if not torch.isfinite(loss):
                    continue
                loss.backward()
                if not torch.isfinite(nn.utils.clip_grad_norm_(self._params, self.max_grad_norm)):
                    continue   # (a gradient whose norm is not finite skips the step too: include/grx_ppo.h grx_ppo_step_tail)
                self.optimizer.step()
                total += loss.item()
        return total / self.num_updates

    def _update_device(self, obs, labels, indices, mb):
        """the same arithmetic without a host round trip inside the loop"""
        sums = self._sums.zero_()
        gather = None
        if self._fused:   # (libgrx_ppo.so is in use): the two minibatch tensors in one launch
            if self._static is None or self._static[0].shape[0] != mb:
                self._static = [torch.empty(mb, obs.shape[1], device=self.device), torch.empty(mb, labels.shape[1], device=self.device)]
            key = (obs.data_ptr(), labels.data_ptr(), self._static[0].data_ptr(), self._static[1].data_ptr())
            if self._gather_key != key:
                self._gather, self._gather_key = RowGather([obs, labels], self._static), key
            gather = self._gather
        for _ in range(self.num_learning_epochs):
            for i in range(self.num_mini_batches):
                idx = indices[i * mb:(i + 1) * mb]
                if gather is not None:
                    gather(idx)
                    xb, yb = self._static
                else:
                    xb, yb = obs[idx], labels[idx]
                loss = self._step(xb, yb)
                loss.backward()
                self._tail_step(loss.detach(), sums)
        return sums[0].item() / self.num_updates                  # the only device->host transfer of the update

    def _tail_step(self, loss, sums):
        """NaN-skip, clip_grad_norm_, Adam at the fixed learning rate, sums[0] += loss (finite steps only): two launches of
        libgrx_ppo.so (fused_loss.StepTail, its adaptive rule off), or the torch tail with fused Adam's found_inf hook"""
        if self._use_tail and self._tail is None:
            if StepTail.supported(self.optimizer, self._params) and all(p.grad is not None for p in self._params):
                self._tail = StepTail(self.optimizer, self._params, self._lr_t)
            else:
                self._use_tail = False
        with torch.no_grad():
            if self._use_tail:
                self._tail(loss, self._zero, loss, loss, sums, False, None, self.learning_rate, self.learning_rate, self.max_grad_norm)
                return
        total_norm = nn.utils.clip_grad_norm_(self._params, self.max_grad_norm, foreach=True)
        with torch.no_grad():   # (a gradient norm that is not finite skips the step as a non-finite loss does: the rule of grx_ppo_step_tail)
            bad = ~torch.isfinite(loss) | ~torch.isfinite(total_norm)
            self.optimizer.found_inf = bad.float().reshape(())
            self.optimizer.grad_scale = None
        self.optimizer.step()
        with torch.no_grad():
            sums[0] += torch.where(bad, 0.0, loss)   # (a skipped step adds nothing)

    # ---- what the runner's save / load expect ------------------------------------------------------------------------------------------
    def load_optimizer_state(self, state_dict):
        """optimizer.load_state_dict() that keeps the device-resident configuration (PPO.load_optimizer_state: torch replaces the
        learning-rate tensor and may bring host step counters)"""
        self.optimizer.load_state_dict(state_dict)
        if self._on_device:
            for g in self.optimizer.param_groups:
                g["lr"] = self._lr_t
                g["fused"], g["capturable"], g["foreach"] = True, True, False
            for stt in self.optimizer.state.values():
                for k, v in list(stt.items()):
                    if torch.is_tensor(v) and (v.device != self._lr_t.device or (k == "step" and v.dtype != torch.float32)):
                        stt[k] = v.to(device=self.device, dtype=torch.float32 if k == "step" else v.dtype)
                    elif k == "step" and not torch.is_tensor(v):
                        stt[k] = torch.tensor(float(v), device=self.device)
            self._tail = None
        else:
            for g in self.optimizer.param_groups:
                g["lr"] = self.learning_rate

    def invalidate_graphs(self):
        pass   # (nothing is captured)

    def prepare_graphs(self, *_):
        pass

    def clear_storage(self):
        self.storage.clear()
