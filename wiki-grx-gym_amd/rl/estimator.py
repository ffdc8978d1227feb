"""A concurrently trained state estimator (Ji et al., "Concurrent Training of a Control Policy and a State Estimator", RA-L 2022; the
estimator half of HIMLoco, DreamWaQ and the humanoid-gym forks): a small MLP that regresses quantities the actor cannot
observe -- base linear velocity, base height, foot contacts, foot heights: the first eight columns behind the copied actor frame of the
privileged frame -- from the actor's own input.  Its output is appended to the actor's input; it is trained by supervision on the rollout
the policy just collected, after PPO's update.

    pipeline:  raw frame -> observation history -> empirical normalisation -> x [N, D] -> [x | est(x)] [N, D + E] -> actor, storage, update
    step(x, pri, slot):
        out[n]           = [x[n] | est(x[n])]                  what alg.act, the storage and PPO's update see
        targets[slot][n] = pri[n][target columns]              the raw privileged frame: before its history and normalisation
    update(rows, num_mini_batches):
        ONE randperm over the T x N stored rows, reused by each of the num_epochs passes; per minibatch: est forward on the first D columns of the stored
        rows, mse against `targets`, backward, Adam at a fixed learning rate, no clipping; a non-finite loss skips the step

The alignment rule.  The storage row of rollout step t holds the actor input built from the frame the env returned BEFORE action t, and
the privileged frame returned together with that frame is its label: x and pri of one `step` call belong to the same env.step (or to the
same get_observations / get_privileged_observations pair), and `slot` is the rollout step at which the returned row will be acted on --
t + 1 for the frames env.step returned at step t.  The frames of the last step are acted on in the next rollout: slot None parks their
targets in `carry`, and `begin_rollout` moves them into targets[0]; the observations learn() starts from go the same way.  An env that
ended at step t returns the reset frame and the reset privileged frame together, so the rows after a done are aligned like every other.

PPO's update is untouched: the estimator's parameters change only after it, so the estimate computed during the rollout is what the current
estimator gives for every stored row -- it is stored as E more columns of the observation row, and is data: PPO's gradient never reaches
the estimator.

The rollout's step is one entry point of libgrx_ppo.so, one launch (include/grx_ppo_est.h grx_est_forward); `est_forward_torch` is the
torch spelling of the same thing: the CPU path and the cross-check, and what GRX_EST_FUSED=0 selects on a HIP device (there the layers go
through grx_mlp_layer, one launch each, then a concatenation and a column select -- bit-equal to the fused launch).  The update reuses
grx_ppo_gather_rows and grx_distill_loss (mse) whatever GRX_EST_FUSED says.  The network is fp32 whatever PPO's precision is.

None of the defaults (targets lin_vel, hidden 128 64, learning rate 1e-3, one epoch) is tuned."""
import ctypes as C
import os

import torch
import torch.nn as nn
import torch.optim as optim

from .modules import MLP

# name -> offsets behind the copied actor frame in the raw privileged frame (envs/grx_env.py; rl/symmetry.py privileged_tail_map: 3 + 1 + 2 + 2)
TARGETS = {"lin_vel": (0, 1, 2), "base_height": (3,), "feet_contact": (4, 5), "feet_height": (6, 7)}
TAIL = 8             # the privileged columns between the copied actor frame and the height scan
MAX_LAYERS, MAX_WIDTH, MAX_INPUT = 4, 256, 2048   # include/grx_ppo_est.h


def _fused_enabled():
    return os.environ.get("GRX_EST_FUSED", "1") != "0"


def parse_targets(targets):
    """a comma-separated string or a sequence of names -> the chosen names in canonical order; ValueError for an unknown name, a duplicate
    or nothing"""
    names = [t.strip() for t in targets.split(",")] if isinstance(targets, str) else [str(t) for t in targets]
    names = [t for t in names if t]
    if not names:
        raise ValueError(f"--estimator_targets is empty: pass a comma-separated subset of {tuple(TARGETS)}")
    for t in names:
        if t not in TARGETS:
            raise ValueError(f"--estimator_targets: unknown target {t!r}, must be a subset of {tuple(TARGETS)}")
    if len(set(names)) != len(names):
        raise ValueError(f"--estimator_targets: a target is named twice in {names}")
    return [t for t in TARGETS if t in names]


def target_columns(targets, num_obs):
    """the columns of the raw privileged frame the targets sit in"""
    return [int(num_obs) + o for t in parse_targets(targets) for o in TARGETS[t]]


def check_layout(env):
    """the privileged frame must be [actor frame | 8 columns | height scan] (symmetry.build_maps checks the same); ValueError otherwise"""
    if env.num_pri_obs is None:
        raise ValueError("--estimator: this env has no privileged observations to take the targets from")
    points = 0
    terrain = getattr(getattr(env, "cfg", None), "terrain", None)
    if terrain is not None and getattr(terrain, "measure_heights", False):
        points = len(terrain.measured_points_x) * len(terrain.measured_points_y)
    if env.num_pri_obs != env.num_obs + TAIL + points:
        raise ValueError(f"--estimator: num_pri_obs={env.num_pri_obs} is not num_obs + {TAIL} + {points} height points = "
                         f"{env.num_obs + TAIL + points}: the privileged frame is not [actor frame | lin_vel 3 | base_height 1 | "
                         "feet_contact 2 | feet_height 2 | height scan], the target columns are not known")


def check_hidden_dims(hidden_dims):
    dims = [int(h) for h in hidden_dims]
    if not 1 <= len(dims) <= MAX_LAYERS - 1 or any(not 1 <= h <= MAX_WIDTH for h in dims):
        raise ValueError(f"--estimator_hidden_dims takes 1 to {MAX_LAYERS - 1} hidden layers of width 1..{MAX_WIDTH} each, not {dims}")
    return dims


def _embed(net, x):
    """est(x) without autograd: on a HIP device through grx_mlp_layer, one launch per layer"""
    if x.is_cuda:
        from .fused_loss import mlp_can_fuse, mlp_forward
        if mlp_can_fuse(net, x):
            return mlp_forward(net, x)
    return net(x)


def est_forward_torch(net, x, pri=None, cols=None):
    """the definition of grx_est_forward in torch: ([x | net(x)], pri[:, cols] or None)"""
    out = torch.cat([x, _embed(net, x)], dim=1)
    if pri is None:
        return out, None
    idx = cols if torch.is_tensor(cols) else torch.as_tensor(list(cols), dtype=torch.long, device=pri.device)
    return out, pri.index_select(1, idx)


class _Net(C.Structure):   # include/grx_ppo_est.h grx_est_net
    _fields_ = [("n_layers", C.c_int), ("widths", C.c_int * MAX_LAYERS), ("W", C.c_void_p * MAX_LAYERS), ("bias", C.c_void_p * MAX_LAYERS)]


def net_struct(net):
    """the grx_est_net of an rl.modules.MLP of Linear -> ELU(1) -> ... -> Linear (the parameters' device pointers as they are now)"""
    from .fused_loss import _linears_of
    lin = _linears_of(net)
    if lin is None or not 2 <= len(lin) <= MAX_LAYERS:
        raise RuntimeError(f"grx_est_forward needs an MLP of Linear -> ELU(1) hidden layers with 2..{MAX_LAYERS} Linear layers")
    s = _Net()
    s.n_layers = len(lin)
    for i, (w, b) in enumerate(lin):
        if not (w.is_cuda and w.dtype == torch.float32 and w.is_contiguous() and (b is None or (b.is_contiguous() and b.dtype == torch.float32))):
            raise RuntimeError("grx_est_forward needs contiguous float32 parameters on a HIP device")
        s.widths[i], s.W[i], s.bias[i] = w.shape[0], w.data_ptr(), (b.data_ptr() if b is not None else None)
    return s


def est_forward_hip(net, x, pri=None, cols=None, out=None, targets=None, struct=None):
    """the same through grx_est_forward, one launch on the current stream: contiguous fp32 tensors on one HIP device; `cols` a sequence of
    ints; `out` [N, D + E] / `targets` [N, E] are allocated here when they are not given; `struct`: net_struct(net), built here otherwise"""
    from .fused_loss import load_ppo_library
    lib = load_ppo_library()
    s = struct if struct is not None else net_struct(net)
    N, D = x.shape
    E = int(s.widths[s.n_layers - 1])
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()):
        raise RuntimeError("grx_est_forward needs a contiguous float32 x [N, D] on a HIP device")
    with torch.inference_mode(False):
        if out is None:
            out = torch.empty(N, D + E, device=x.device, dtype=torch.float32)
        if pri is not None and targets is None:
            targets = torch.empty(N, E, device=x.device, dtype=torch.float32)
    P, carr = 0, None
    if pri is not None:
        if not (pri.is_cuda and pri.dtype == torch.float32 and pri.is_contiguous() and pri.dim() == 2 and pri.shape[0] == N
                and pri.device == x.device) or len(cols) != E:
            raise RuntimeError(f"grx_est_forward needs a contiguous float32 pri [N, P] on x's device and {E} target columns")
        P, carr = pri.shape[1], (C.c_int * E)(*[int(c) for c in cols])
        if not (targets.is_contiguous() and targets.dtype == torch.float32 and targets.numel() == N * E and targets.device == x.device):
            raise RuntimeError("grx_est_forward needs a contiguous float32 targets [N, E] on x's device")
    if not (out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == (N, D + E) and out.device == x.device):
        raise RuntimeError("grx_est_forward needs a contiguous float32 out [N, D + E] on x's device")
    with torch.cuda.device(x.device):
        rc = lib.grx_est_forward(C.addressof(s), N, D, x.data_ptr(), P, pri.data_ptr() if pri is not None else None, carr, out.data_ptr(),
                                 targets.data_ptr() if pri is not None else None,
                                 C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream))
    if rc != 0:
        raise RuntimeError(f"grx_est_forward failed ({rc}): {N} x {D} -> {E}")
    return out, (targets if pri is not None else None)


class EstimatorPolicy(nn.Module):
    """actor([x | est(x)]): what inference and the exported TorchScript module put behind the history and the normaliser"""

    def __init__(self, actor, estimator):
        super().__init__()
        self.actor, self.estimator = actor, estimator

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.actor(torch.cat([x, self.estimator(x)], dim=-1))


class StateEstimator(nn.Module):
    """`net`: MLP(D, E, hidden_dims, activation) over the actor's input; state_dict() is the network.  Stored per rollout: `targets`
    (T, N, E), the labels of the storage's observation rows; `carry` (N, E), those of the row the next rollout starts with."""

    def __init__(self, num_inputs, num_obs, num_pri_obs, num_envs, num_steps, device="cpu", targets=("lin_vel",), hidden_dims=(128, 64),
                 activation="elu", learning_rate=1e-3, num_epochs=1):
        super().__init__()
        names = parse_targets(targets)
        dims = check_hidden_dims(hidden_dims)
        D, N, T = int(num_inputs), int(num_envs), int(num_steps)
        if not 1 <= D <= MAX_INPUT:
            raise ValueError(f"--estimator: the actor's input has {D} columns, the estimator takes 1..{MAX_INPUT}")
        if activation != "elu":
            raise ValueError(f"--estimator: activation must be 'elu', not {activation!r}")
        if int(num_epochs) < 1 or not float(learning_rate) > 0.0:
            raise ValueError(f"--estimator_num_epochs must be >= 1 and --estimator_learning_rate > 0, got {num_epochs} and {learning_rate}")
        self.cols = target_columns(names, num_obs)
        E = len(self.cols)
        if max(self.cols) >= int(num_pri_obs):
            raise ValueError(f"--estimator: target column {max(self.cols)} is outside the privileged frame of {num_pri_obs} columns")
        self.num_inputs, self.num_outputs, self.num_pri_obs, self.num_envs, self.num_steps, self.device = D, E, int(num_pri_obs), N, T, device
        self.config = {"targets": names, "hidden_dims": dims, "activation": activation}
        self.learning_rate, self.num_epochs = float(learning_rate), int(num_epochs)
        self.net = MLP(D, E, dims, activation)
        self.to(device)
        self.targets = torch.zeros(T, N, E, device=device)
        self.carry = torch.zeros(N, E, device=device)
        self._cols_t = torch.tensor(self.cols, dtype=torch.long, device=device)
        self._on_device = torch.device(device).type == "cuda"
        self._fused = self._on_device and _fused_enabled()
        self._params = list(self.net.parameters())
        if self._on_device:   # device-resident, as RND's: the NaN-skip is Adam's found_inf hook, no host round trip
            self.optimizer = optim.Adam(self._params, lr=torch.tensor(self.learning_rate, device=device), fused=True, capturable=True)
            self._sums = torch.zeros(2, device=device)
        else:
            self.optimizer = optim.Adam(self._params, lr=self.learning_rate)
        self._gather, self._static, self._gather_src = None, None, None
        self._struct = net_struct(self.net) if self._fused else None   # (Adam and load_state_dict write the parameters in place)

    # ---- the rollout -------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, x, pri, slot):
        """x [N, D] the actor's input, pri [N, P] the raw privileged frame of the same env step -> [x | est(x)] [N, D + E], a new tensor;
        the frame's target columns go to targets[slot], or to `carry` (slot None)"""
        if x.dim() != 2 or tuple(x.shape) != (self.num_envs, self.num_inputs):
            raise ValueError(f"StateEstimator: expected an input of {(self.num_envs, self.num_inputs)}, got {tuple(x.shape)}")
        if pri.dim() != 2 or tuple(pri.shape) != (self.num_envs, self.num_pri_obs):
            raise ValueError(f"StateEstimator: expected a privileged frame of {(self.num_envs, self.num_pri_obs)}, got {tuple(pri.shape)}")
        if slot is not None and not 0 <= slot < self.num_steps:
            raise AssertionError("Rollout buffer overflow")
        dst = self.carry if slot is None else self.targets[slot]
        x = x if x.is_contiguous() else x.contiguous()
        if self._fused:
            out, _ = est_forward_hip(self.net, x, pri if pri.is_contiguous() else pri.contiguous(), self.cols, targets=dst, struct=self._struct)
            return out
        out, y = est_forward_torch(self.net, x, pri, self._cols_t)
        dst.copy_(y)
        return out

    @torch.no_grad()
    def begin_rollout(self):
        """before rollout step 0: the targets of the row this rollout starts with are the ones parked last"""
        self.targets[0].copy_(self.carry)

    # ---- the update --------------------------------------------------------------------------------------------------------------------
    def _loss(self, x, y):
        from .distillation import distill_loss
        return distill_loss(self.net(x), y, "mse", self._on_device)

    def update(self, rows, num_mini_batches):
        """the regression on the stored rollout: `rows` (T, N, D + E) the storage's observation rows, whose first D columns are the input;
        returns the mean loss over the steps with a finite loss (0.0: none)"""
        D, E = self.num_inputs, self.num_outputs
        if tuple(rows.shape) != (self.num_steps, self.num_envs, D + E):
            raise ValueError(f"StateEstimator.update: expected rows of {(self.num_steps, self.num_envs, D + E)}, got {tuple(rows.shape)}")
        n = self.num_steps * self.num_envs
        nmb = int(num_mini_batches)
        mb = n // nmb
        wide, targets = rows.flatten(0, 1), self.targets.flatten(0, 1)
        indices = torch.randperm(nmb * mb, requires_grad=False, device=self.device)   # one permutation, every epoch
        self.net.train()
        if not self._on_device:
            total, steps = 0.0, 0
            for _ in range(self.num_epochs):
                for i in range(nmb):
                    idx = indices[i * mb:(i + 1) * mb]
                    loss = self._loss(wide[idx, :D], targets[idx])
                    if not torch.isfinite(loss):
                        continue
                    self.optimizer.zero_grad(set_to_none=False)
                    loss.backward()
                    self.optimizer.step()
                    total, steps = total + loss.item(), steps + 1
            return total / steps if steps else 0.0
        sums = self._sums.zero_()
        from .fused_loss import RowGather
        if self._static is None or self._static[0].shape[0] != mb or self._gather_src != wide.data_ptr():   # the wide rows and the labels in one launch
            self._static = [torch.empty(mb, D + E, device=self.device), torch.empty(mb, E, device=self.device)]
            self._gather = RowGather([wide, targets], self._static)
            self._gather_src = wide.data_ptr()
        for _ in range(self.num_epochs):
            for i in range(nmb):
                self._gather(indices[i * mb:(i + 1) * mb])
                xb = self._static[0][:, :D].contiguous()   # (the training MLP takes contiguous rows: a copy of the minibatch, not of the rollout)
                loss = self._loss(xb, self._static[1])
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

    # ---- the checkpoint's "estimator" entry ------------------------------------------------------------------------------------------------
    def checkpoint(self):
        return {"state_dict": self.state_dict(), "optimizer_state_dict": self.optimizer.state_dict(), "config": dict(self.config)}

    def load_checkpoint(self, saved, load_optimizer=True):
        """the network and -- load_optimizer -- the optimizer of a saved "estimator" entry; the learning rate stays this run's.  ValueError
        when the targets, the hidden layers or the input width are other than this run's"""
        for k in ("targets", "hidden_dims", "activation"):
            if saved["config"][k] != self.config[k]:
                raise ValueError(f"the checkpoint's estimator entry has {k}={saved['config'][k]!r}, this run {self.config[k]!r}")
        w = saved["state_dict"]["net.model.0.weight"]
        if w.shape[1] != self.num_inputs:
            raise ValueError(f"the checkpoint's estimator entry reads {w.shape[1]} input columns, this run {self.num_inputs}")
        self.load_state_dict(saved["state_dict"])   # (in place: the device pointers grx_est_forward was given stay valid)
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
