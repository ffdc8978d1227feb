"""Constraints as terminations for PPO (Chane-Sane, Leziart, Flayols, Stasse, Soueres, Mansard, "CaT: Constraints as
Terminations for Legged Locomotion Reinforcement Learning", IROS 2024): a constraint violation becomes a probability delta of ending the
episode at that step.  delta scales the reward and the discount inside GAE; there is no extra critic and no multiplier, and a family of
constraints takes one hyper-parameter, its maximum termination probability.

    spec         `family:p[@L],family:p[@L],...`; p is one number in [0, 1] or `p_lo..p_hi`, ramped over --constraint_ramp_its iterations.
                 The families, a violation being positive (C columns in the spec's order, 1 <= C <= 256):
                     torque        one column per DOF      |torques| - soft_torque_limit * torque_limits
                     dof_vel       one per DOF             |dof_vel| - soft_dof_vel_limit * dof_vel_limits
                     dof_pos       one per DOF             max(lo - dof_pos, dof_pos - hi) with env.dof_pos_limits (already soft)
                     action_rate   one per action          |actions - prev| - L          (`@L` required)
                     upright       one                     sqrt(g_x g_x + g_y g_y) - L    (`@L` required) on base_projected_gravity
                 `actions` is the env's ACTIONS tensor (what the kernel applied), `prev` a copy of its rows of the step before: zero for a
                 row whose previous step ended an episode, zero before the first step
    per step     c+ = max(c, 0), zero in every column of a row whose dones byte is set (its state has been reset already);
                 m = max over the envs of c+;  c_max <- tau c_max + (1 - tau) m   (per column, starting at 0, updated BEFORE it is used);
                 delta = max over the columns of p_col clip(c+ / c_max, 0, 1), a column with c_max = 0 contributing 0;
                 storage.rewards[t] <- (1 - delta) max(row, 0)   (--constraint_reward_clip none: (1 - delta) row), after process_env_step
                 has stored the row; `Mean reward` and the episode statistics stay the env's
    returns      RolloutStorage.compute_returns' loop with alive = (1 - done)(1 - delta), then (a - mean) / (std + 1e-8)
    schedule     p(it) = p_lo + (p_hi - p_lo) min(it / R, 1), it the runner's learning iteration

Every operation is rounded to fp32 on its own.  On a HIP device the step and the returns are two entry points of libgrx_ppo.so
(include/grx_ppo_cat.h: grx_cat_step, grx_cat_returns), bit-equal to `cat_step_torch` / `cat_returns_torch` below, which are the definition,
the CPU path, and what GRX_CAT_FUSED=0 selects on a HIP device.  Not a config key: `--constraints` / `--constraint_*` or assignments to
train_cfg.algorithm set it; without it nothing of this module is imported."""
import ctypes as C
import math
import os

import torch

FAMILIES = ("torque", "dof_vel", "dof_pos", "action_rate", "upright")   # a family's position is its kind (include/grx_ppo_cat.h GRX_CAT_*)
NEEDS_LIMIT = ("action_rate", "upright")
REWARD_CLIPS = ("zero", "none")
MAX_COLUMNS = 256       # GRX_CAT_MAX_COLUMNS
MAX_ROWS = 1 << 24      # grx_cat_returns' largest T N

_BOUND = None           # libgrx_ppo.so with the grx_cat_* prototypes set up: None until a fused call needs them


def fused_enabled():
    return os.environ.get("GRX_CAT_FUSED", "1") != "0"


def _lib():
    global _BOUND
    if _BOUND is None:
        from .fused_loss import load_ppo_library
        lib = load_ppo_library()
        fp = C.c_void_p
        lib.grx_cat_step_blocks.restype = C.c_int
        lib.grx_cat_step_blocks.argtypes = [C.c_int]
        lib.grx_cat_step.restype = C.c_int
        lib.grx_cat_step.argtypes = ([C.c_int] * 6 + [fp] * 11 + [C.POINTER(C.c_longlong), fp, C.c_float, C.c_float, C.c_int, C.c_int] + [fp] * 8
                                     + [C.c_void_p])
        lib.grx_cat_partials_size.restype = C.c_int
        lib.grx_cat_partials_size.argtypes = [C.c_int] * 2
        lib.grx_cat_returns.restype = C.c_int
        lib.grx_cat_returns.argtypes = [C.c_int] * 2 + [fp] * 5 + [C.c_float, C.c_float] + [fp] * 4 + [C.c_void_p]
        _BOUND = lib
    return _BOUND


# ---------------------------------------------------------------------------------------------------------------- the spec
class ConstraintSpec:
    """a parsed spec: `families`, in the spec's order, of (name, p_lo, p_hi, limit or None)"""

    def __init__(self, families):
        self.families = [(str(n), float(lo), float(hi), None if lim is None else float(lim)) for n, lo, hi, lim in families]

    @property
    def names(self):
        return [f[0] for f in self.families]

    def key(self):
        """something to compare and to save: the families IN ORDER (a family's position fixes its columns)"""
        return [[n, lo, hi, lim] for n, lo, hi, lim in self.families]

    def text(self):
        """the spec as --constraints takes it"""
        num = lambda x: repr(float(x))
        return ",".join(n + ":" + (num(lo) if lo == hi else num(lo) + ".." + num(hi)) + ("" if lim is None else "@" + num(lim))
                        for n, lo, hi, lim in self.families)

    def probabilities(self, it, ramp_its):
        """every family's maximum termination probability at learning iteration `it`"""
        s = min(float(it) / float(ramp_its), 1.0)
        return [lo + (hi - lo) * s for _, lo, hi, _ in self.families]


def _number(text, what, entry):
    try:
        x = float(text)
    except ValueError:
        raise ValueError(f"--constraints: {text!r} is not a number ({what} of {entry!r})") from None
    if not math.isfinite(x):
        raise ValueError(f"--constraints: {what} of {entry!r} must be finite, not {text!r}")
    return x


def parse_constraints(spec):
    """`family:p[@L],...` -> ConstraintSpec (a ConstraintSpec passes through).  Raises ValueError on anything the module's docstring rules
    out; an unknown family lists the known ones."""
    if isinstance(spec, ConstraintSpec):
        return spec
    if not isinstance(spec, str) or not spec.strip():
        raise ValueError(f"--constraints needs a spec `family:p[@L],family:p[@L],...`, not {spec!r}")
    families = []
    for entry in spec.split(","):
        entry = entry.strip()
        if not entry:
            continue
        name, sep, rhs = entry.partition(":")
        name = name.strip()
        if not sep or not rhs.strip():
            raise ValueError(f"--constraints: {entry!r} is not `family:p[@L]`")
        if name not in FAMILIES:
            raise ValueError(f"--constraints: {name!r} is not a constraint family; the known ones are {', '.join(FAMILIES)}")
        if name in [f[0] for f in families]:
            raise ValueError(f"--constraints: family {name!r} appears twice")
        prob, at, limit = rhs.partition("@")
        if name in NEEDS_LIMIT:
            if not at or not limit.strip():
                raise ValueError(f"--constraints: {name} needs its limit, `{name}:p@L`, not {entry!r}")
            lim = _number(limit.strip(), "the limit", entry)
            if lim < 0.0:
                raise ValueError(f"--constraints: the limit of {entry!r} must be >= 0")
        else:
            if at:
                raise ValueError(f"--constraints: {name} takes no `@L` (its limits are the env's: {entry!r})")
            lim = None
        lo, dots, hi = prob.partition("..")
        p_lo = _number(lo.strip(), "the probability", entry)
        p_hi = _number(hi.strip(), "the probability", entry) if dots else p_lo
        if not (0.0 <= p_lo <= 1.0 and 0.0 <= p_hi <= 1.0):
            raise ValueError(f"--constraints: the probabilities of {entry!r} must be in [0, 1]")
        families.append((name, p_lo, p_hi, lim))
    if not families:
        raise ValueError(f"--constraints needs a spec `family:p[@L],family:p[@L],...`, not {spec!r}")
    return ConstraintSpec(families)


def check_options(tau, ramp_its, reward_clip):
    """(tau, ramp_its, reward_clip) as PPO keeps them; raises ValueError by the option's name"""
    try:
        t = float(tau)
    except (TypeError, ValueError):
        raise ValueError(f"--constraint_tau must be a number in [0, 1), not {tau!r}") from None
    if not 0.0 <= t < 1.0:
        raise ValueError(f"--constraint_tau must be in [0, 1), not {tau!r}")
    if isinstance(ramp_its, bool) or not isinstance(ramp_its, int) and not (isinstance(ramp_its, float) and ramp_its.is_integer()):
        raise ValueError(f"--constraint_ramp_its must be an integer >= 1, not {ramp_its!r}")
    if int(ramp_its) < 1:
        raise ValueError(f"--constraint_ramp_its must be an integer >= 1, not {ramp_its!r}")
    if reward_clip not in REWARD_CLIPS:
        raise ValueError(f"--constraint_reward_clip must be one of {REWARD_CLIPS}, not {reward_clip!r}")
    return t, int(ramp_its), reward_clip


# ---------------------------------------------------------------------------------------------------------------- the column table
class ColumnTable:
    """a spec expanded against a robot: per column its kind, source index, family, lo and hi; per family its column range"""

    def __init__(self, spec, num_dof, num_actions, torque_limits=None, dof_vel_limits=None, dof_pos_limits=None, soft_torque_limit=1.0,
                 soft_dof_vel_limit=1.0, device="cpu"):
        f32 = lambda x: torch.as_tensor(x, dtype=torch.float32).detach().to("cpu")
        kind, src, fam, lo, hi, self.ranges = [], [], [], [], [], []
        for f, (name, _, _, limit) in enumerate(spec.families):
            k = FAMILIES.index(name)
            c0 = len(kind)
            if name in ("torque", "dof_vel"):
                lim, soft = (torque_limits, soft_torque_limit) if name == "torque" else (dof_vel_limits, soft_dof_vel_limit)
                if lim is None or f32(lim).numel() != num_dof:
                    raise ValueError(f"--constraints: {name} needs the env's {name if name == 'torque' else 'dof_vel'}_limits, one per DOF ({num_dof})")
                scaled = f32(lim).reshape(-1) * float(soft)   # (one fp32 product per DOF, formed once)
                width, los, his = num_dof, [0.0] * num_dof, scaled.tolist()
            elif name == "dof_pos":
                if dof_pos_limits is None or tuple(f32(dof_pos_limits).shape) != (num_dof, 2):
                    raise ValueError(f"--constraints: dof_pos needs the env's dof_pos_limits [{num_dof}, 2]")
                lims = f32(dof_pos_limits)
                width, los, his = num_dof, lims[:, 0].tolist(), lims[:, 1].tolist()
            elif name == "action_rate":
                width, los, his = num_actions, [0.0] * num_actions, [limit] * num_actions
            else:
                width, los, his = 1, [0.0], [limit]
            kind += [k] * width
            src += list(range(width))
            fam += [f] * width
            lo += los
            hi += his
            self.ranges.append((c0, c0 + width))
        self.C, self.F, self.num_dof, self.num_actions = len(kind), len(spec.families), int(num_dof), int(num_actions)
        if not 1 <= self.C <= MAX_COLUMNS:
            raise ValueError(f"--constraints: the spec expands into {self.C} columns, the number of columns must be in 1..{MAX_COLUMNS}")
        self.kinds = [FAMILIES.index(n) for n in spec.names]
        self.kind_mask = sum(1 << k for k in self.kinds)
        i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=device)
        self.kind, self.src, self.family = i32(kind), i32(src), i32(fam)
        self.lo, self.hi = torch.tensor(lo, dtype=torch.float32, device=device), torch.tensor(hi, dtype=torch.float32, device=device)

    def column_probabilities(self, per_family):
        return [p for p, (c0, c1) in zip(per_family, self.ranges) for _ in range(c1 - c0)]


# ---------------------------------------------------------------------------------------------------------------- the torch spelling
def _sqrt32(x):
    """the correctly rounded fp32 square root.  torch.sqrt on a float32 CPU tensor is not that on every build (a vector math library's
    sqrt is off by one ulp on a few per cent of its arguments); the float64 root of a float32 number, rounded to float32, is (53 >= 2 * 24 + 2
    bits: the double rounding is innocuous), and it is what sqrtf gives in the kernel"""
    return torch.sqrt(x.double()).to(x.dtype)


def violations_torch(table, torques, dof_vel, dof_pos, actions, prev, gravity, dones):
    """c+ [N, C]: every column's violation, zero where it is none and in a done row"""
    cols = []
    for k, (c0, c1) in zip(table.kinds, table.ranges):
        lo, hi = table.lo[c0:c1], table.hi[c0:c1]
        if k == 0:
            c = torques.abs() - hi
        elif k == 1:
            c = dof_vel.abs() - hi
        elif k == 2:
            c = torch.maximum(lo - dof_pos, dof_pos - hi)
        elif k == 3:
            c = (actions - prev).abs() - hi
        else:
            gx, gy = gravity[:, 0:1], gravity[:, 1:2]
            c = _sqrt32(gx * gx + gy * gy) - hi
        cols.append(c)
    c = torch.cat(cols, dim=1)
    cplus = torch.where(c > 0, c, torch.zeros_like(c))
    return torch.where(dones.reshape(-1, 1) != 0, torch.zeros_like(cplus), cplus)


def cat_step_torch(table, prob, torques, dof_vel, dof_pos, actions, gravity, dones, tau, one_minus_tau, clip_zero, reset_counts, prev,
                   c_max, counts, term_prob_row, reward_row):
    """the definition of grx_cat_step, in place on prev [N, A] (or None), c_max [C], counts [F] (int32), term_prob_row [N], reward_row [N]
    (or [N, 1]); prob [C], dones [N] (uint8 / bool), tau / one_minus_tau python floats that are fp32 values.  No host synchronisation."""
    cplus = violations_torch(table, torques, dof_vel, dof_pos, actions, prev, gravity, dones)
    m = cplus.max(dim=0).values
    c_max.copy_(tau * c_max + one_minus_tau * m)
    rows = torch.stack([(cplus[:, c0:c1] > 0).any(dim=1).sum() for c0, c1 in table.ranges]).to(counts.dtype)
    counts.copy_(rows if reset_counts else counts + rows)
    live = c_max > 0
    ratio = torch.clamp(cplus / torch.where(live, c_max, torch.ones_like(c_max)), max=1.0)
    terms = torch.where(live, prob * ratio, torch.zeros_like(ratio))
    delta = terms.max(dim=1).values
    term_prob_row.copy_(delta.reshape(term_prob_row.shape))
    r = reward_row.reshape(-1)
    if clip_zero:
        r = torch.where(r < 0, torch.zeros_like(r), r)
    reward_row.copy_(((1.0 - delta) * r).reshape(reward_row.shape))
    if prev is not None:
        prev.copy_(torch.where(dones.reshape(-1, 1) != 0, torch.zeros_like(actions), actions))


def cat_returns_torch(rewards, values, dones, term_prob, last_values, gamma, lam, returns, advantages, stats=None):
    """the definition of grx_cat_returns, in place: rewards / values / dones / returns / advantages of one shape [T, N] or [T, N, 1],
    term_prob [T, N], last_values [N] or [N, 1]; stats [4] or None.  With term_prob == 0 this is RolloutStorage.compute_returns (single
    rank).  No host synchronisation."""
    T = rewards.shape[0]
    adv = 0
    for step in reversed(range(T)):
        nxt = last_values.reshape(values[step].shape) if step == T - 1 else values[step + 1]
        alive = (1.0 - dones[step].float()) * (1.0 - term_prob[step].reshape(dones[step].shape))
        delta = rewards[step] + alive * gamma * nxt - values[step]
        adv = delta + alive * gamma * lam * adv
        returns[step] = adv + values[step]
    a = returns - values
    mean_a, std_a = a.mean(), a.std()
    advantages.copy_((a - mean_a) / (std_a + 1e-8))
    if stats is not None:
        stats.copy_(torch.stack([mean_a, std_a, returns.mean(), returns.var(unbiased=False)]))


# ---------------------------------------------------------------------------------------------------------------- through libgrx_ppo.so
def _ok(t, dtype=torch.float32):
    return t.is_cuda and t.dtype == dtype and t.is_contiguous()


def _u8(dones):
    return dones.view(torch.uint8) if dones.dtype == torch.bool else dones


def step_scratch(table, N, device):
    """(cplus [N, C], part_max [nb, C], part_count [nb, F]): what one grx_cat_step call at N envs needs"""
    nb = _lib().grx_cat_step_blocks(N)
    if nb < 1:
        raise RuntimeError(f"grx_cat_step_blocks: invalid N = {N}")
    with torch.inference_mode(False):
        return (torch.empty(N, table.C, device=device), torch.empty(nb, table.C, device=device),
                torch.empty(nb, table.F, device=device, dtype=torch.int32))


def prepare_step(table, prob, torques, dof_vel, dof_pos, actions, gravity, dones, tau, one_minus_tau, clip_zero, reset_counts, prev, c_max,
                 counts, term_prob_row, reward_row, scratch=None):
    """everything one grx_cat_step call is handed, checked once: (device, argument tuple without the stream, what keeps the memory alive).
    The rollout calls the same step of the same tensors every iteration: Constraints.step keeps one of these per rollout step"""
    dones = _u8(dones)
    N = dones.numel()
    D, A = table.num_dof, table.num_actions
    srcs = ((torques, D), (dof_vel, D), (dof_pos, D), (actions, A), (gravity, 3))   # (the env's views are strided: (1, N) over SoA storage)
    strided = lambda t, w: t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (N, w) and all(s >= 0 for s in t.stride())
    if not all(t is None or (strided(t, w) and t.device == dones.device) for t, w in srcs) \
            or not (prev is None or (_ok(prev) and prev.numel() == N * A and prev.device == dones.device)) \
            or not all(_ok(t) and t.numel() == table.C and t.device == dones.device for t in (prob, c_max, table.lo, table.hi)) \
            or not all(_ok(t, torch.int32) and t.numel() == table.C for t in (table.kind, table.src, table.family)) \
            or not (_ok(counts, torch.int32) and counts.numel() == table.F) or not _ok(dones, torch.uint8) \
            or not (_ok(term_prob_row) and term_prob_row.numel() == N and _ok(reward_row) and reward_row.numel() == N):
        raise RuntimeError("grx_cat_step needs tensors on one HIP device: float32 sources [N, D] / [N, A] / [N, 3] (any non-negative strides), "
                           "contiguous float32 prev [N, A], prob / c_max [C], term_prob_row / reward_row [N], int32 counts [F] and uint8 dones [N]")
    strides = (C.c_longlong * 10)(*[x for t, _ in srcs for x in ((0, 0) if t is None else t.stride())])
    scratch = scratch if scratch is not None else step_scratch(table, N, dones.device)
    cplus, part_max, part_count = scratch
    ptr = lambda t: t.data_ptr() if t is not None else None
    args = (N, table.C, table.F, D, A, table.kind_mask, ptr(table.kind), ptr(table.src), ptr(table.family), ptr(table.lo), ptr(table.hi), ptr(prob),
            ptr(torques), ptr(dof_vel), ptr(dof_pos), ptr(actions), ptr(gravity), strides, ptr(dones), float(tau), float(one_minus_tau),
            int(bool(clip_zero)), int(bool(reset_counts)), ptr(prev), ptr(c_max), ptr(counts), ptr(cplus), ptr(part_max), ptr(part_count),
            ptr(term_prob_row), ptr(reward_row))
    keep = (table, prob, torques, dof_vel, dof_pos, actions, gravity, dones, prev, c_max, counts, scratch, term_prob_row, reward_row)
    return dones.device, args, keep


def launch_step(prepared):
    """grx_cat_step on the current stream with prepare_step's arguments: three launches"""
    device, args, _ = prepared
    with torch.cuda.device(device):
        rc = _lib().grx_cat_step(*args, C.c_void_p(torch.cuda.current_stream(device).cuda_stream))
    if rc != 0:
        raise RuntimeError(f"grx_cat_step failed ({rc}): N = {args[0]}, C = {args[1]}, F = {args[2]}, D = {args[3]}, A = {args[4]}")


def cat_step_hip(*args, **kwargs):
    """the same through grx_cat_step: three launches on the current stream; `scratch` (step_scratch) is allocated here when not given"""
    launch_step(prepare_step(*args, **kwargs))


def cat_partials(T, N, device):
    """the scratch one grx_cat_returns call at (T, N) needs"""
    size = _lib().grx_cat_partials_size(T, N)
    if size < 1:
        raise RuntimeError(f"grx_cat_partials_size: invalid shape T = {T}, N = {N}")
    with torch.inference_mode(False):
        return torch.empty(size, device=device, dtype=torch.float32)


def cat_returns_hip(rewards, values, dones, term_prob, last_values, gamma, lam, returns, advantages, stats=None, partials=None):
    """the same through grx_cat_returns: three launches on the current stream; `stats` [4] and `partials` (cat_partials) are allocated
    here when they are not given.  Returns stats."""
    lib = _lib()
    T, N = rewards.shape[0], rewards.shape[1]
    dones = _u8(dones)
    if not all(_ok(t) and t.device == rewards.device and t.numel() == T * N for t in (rewards, values, term_prob, returns, advantages)) \
            or not (_ok(dones, torch.uint8) and dones.numel() == T * N) or not (_ok(last_values) and last_values.numel() == N):
        raise RuntimeError("grx_cat_returns needs contiguous tensors on one HIP device: float32 rewards / values / term_prob / returns / "
                           "advantages and uint8 dones with T N elements, float32 last_values with N")
    if stats is None:
        with torch.inference_mode(False):
            stats = torch.empty(4, device=rewards.device, dtype=torch.float32)
    part = partials if partials is not None else cat_partials(T, N, rewards.device)
    with torch.cuda.device(rewards.device):
        rc = lib.grx_cat_returns(T, N, rewards.data_ptr(), values.data_ptr(), dones.data_ptr(), term_prob.data_ptr(), last_values.data_ptr(),
                                 float(gamma), float(lam), returns.data_ptr(), advantages.data_ptr(), stats.data_ptr(), part.data_ptr(),
                                 C.c_void_p(torch.cuda.current_stream(rewards.device).cuda_stream))
    if rc != 0:
        raise RuntimeError(f"grx_cat_returns failed ({rc}): T = {T}, N = {N}")
    return stats


# ---------------------------------------------------------------------------------------------------------------- what PPO holds
class Constraints:
    """the spec, its options, the per-column state c_max, the previous action rows, the rollout's [T, N] termination probabilities beside
    RolloutStorage's tensors, and the two passes over them"""

    def __init__(self, spec, tau=0.95, ramp_its=1000, reward_clip="zero", device="cpu"):
        self.spec = parse_constraints(spec)
        self.tau_option, self.ramp_its, self.reward_clip = check_options(tau, ramp_its, reward_clip)
        self.device = device
        tau32 = torch.tensor(self.tau_option, dtype=torch.float32)
        self.tau, self.one_minus_tau = tau32.item(), (torch.tensor(1.0) - tau32).item()   # two fp32 values, the difference formed in fp32
        self.table = None                                  # bind
        self.sources = None                                # (torques, dof_vel, dof_pos, actions, gravity): the env's tensors, bind
        self.c_max = self.counts = self.prob = self.prev = None
        self.term_prob = None                              # [T, N]: init_storage
        self.stats = torch.zeros(4, device=device)         # grx_cat_returns' statistics of the last rollout
        self.iteration = 0
        self._pending_c_max = None                         # a checkpoint's c_max loaded before bind
        self._scratch, self._scratch_key, self._partials, self._partials_key = None, None, None, None
        self._calls = {}                                   # rollout step -> (the tensors' addresses, prepare_step's result)

    def entry(self):
        """what a checkpoint's "constraints" entry holds beside the state"""
        return {"spec": self.spec.key(), "tau": self.tau_option, "ramp_its": self.ramp_its, "reward_clip": self.reward_clip}

    def bind(self, env):
        """the env's tensors (zero-copy views the step pass reads every step) and its limits, once"""
        names, dev = self.spec.names, self.device
        src = lambda attr: getattr(env, attr).to(dev) if torch.device(dev).type == "cpu" else getattr(env, attr)
        need = {"torque": "torques", "dof_vel": "dof_vel", "dof_pos": "dof_pos", "action_rate": "actions", "upright": "base_projected_gravity"}
        for fam in names:
            if getattr(env, need[fam], None) is None:
                raise ValueError(f"--constraints: {fam} needs env.{need[fam]}, which this env does not publish")
        num_dof = int(env.dof_pos.shape[1]) if getattr(env, "dof_pos", None) is not None else int(env.num_actions)
        rewards = env.cfg.rewards
        self.table = ColumnTable(self.spec, num_dof, int(env.num_actions), getattr(env, "torque_limits", None), getattr(env, "dof_vel_limits", None),
                                 getattr(env, "dof_pos_limits", None), float(getattr(rewards, "soft_torque_limit", 1.0)),
                                 float(getattr(rewards, "soft_dof_vel_limit", 1.0)), dev)
        self.sources = lambda: tuple(src(need[f]) if f in names else None for f in FAMILIES)
        Cn, F = self.table.C, self.table.F
        self.c_max = torch.zeros(Cn, device=dev)
        self.counts = torch.zeros(F, dtype=torch.int32, device=dev)
        self.prob = torch.zeros(Cn, device=dev)
        self.prev = torch.zeros(int(env.num_envs), int(env.num_actions), device=dev) if "action_rate" in names else None
        if self._pending_c_max is not None:
            pending, self._pending_c_max = self._pending_c_max, None
            self._set_c_max(pending)
        self.set_iteration(self.iteration)

    def init_storage(self, num_envs, num_transitions_per_env):
        self.term_prob = torch.zeros(num_transitions_per_env, num_envs, device=self.device)

    def set_iteration(self, it):
        """once per learning iteration: the C probabilities of this iteration into their device tensor"""
        self.iteration = int(it)
        if self.table is not None:
            p = self.table.column_probabilities(self.spec.probabilities(self.iteration, self.ramp_its))
            self.prob.copy_(torch.tensor(p, dtype=torch.float32))

    def _fused(self, t):
        return t.is_cuda and fused_enabled()

    def step(self, t, storage):
        """rollout step t, after process_env_step has stored it: delta into term_prob[t], storage.rewards[t] edited in place"""
        if self.table is None:
            raise RuntimeError("--constraints: no env is bound (Constraints.bind)")
        if self.term_prob is None or tuple(self.term_prob.shape) != (storage.num_transitions_per_env, storage.num_envs):
            raise RuntimeError("--constraints: the termination probabilities' tensor does not match the storage (Constraints.init_storage)")
        torques, dof_vel, dof_pos, actions, gravity = self.sources()
        dones, row = storage.dones[t].reshape(-1), storage.rewards[t]
        args = (self.table, self.prob, torques, dof_vel, dof_pos, actions, gravity, dones, self.tau, self.one_minus_tau,
                self.reward_clip == "zero", t == 0, self.prev, self.c_max, self.counts, self.term_prob[t], row)
        if self._fused(row):
            key = (storage.num_envs, row.device)
            if self._scratch_key != key:
                self._scratch, self._scratch_key, self._calls = step_scratch(self.table, storage.num_envs, row.device), key, {}
            # (the argument checks and the ctypes marshalling cost more host time than the three launches take: once per rollout step
            #  and tensor addresses, not once per call)
            where = (row.data_ptr(), dones.data_ptr(), self.term_prob[t].data_ptr()) + tuple(0 if x is None else x.data_ptr() for x in (torques, dof_vel, dof_pos, actions, gravity))
            call = self._calls.get(t)
            if call is None or call[0] != where:
                call = self._calls[t] = (where, prepare_step(*args, scratch=self._scratch))
            launch_step(call[1])
        else:
            cat_step_torch(*args)

    def compute_returns(self, storage, last_values, gamma, lam):
        """once per iteration: storage.returns and storage.advantages in place, the discount scaled by (1 - delta)"""
        st = storage
        T, N = st.num_transitions_per_env, st.num_envs
        if T * N > MAX_ROWS:
            raise ValueError(f"--constraints: a rollout of {T * N} transitions per update is more than {MAX_ROWS}")
        last_values = last_values.detach()
        if self._fused(st.returns):
            key = (T, N, st.returns.device)
            if self._partials_key != key:
                self._partials, self._partials_key = cat_partials(T, N, st.returns.device), key
            cat_returns_hip(st.rewards, st.values, st.dones, self.term_prob, last_values.contiguous(), gamma, lam, st.returns, st.advantages,
                            self.stats, self._partials)
        else:
            cat_returns_torch(st.rewards, st.values, st.dones, self.term_prob, last_values, gamma, lam, st.returns, st.advantages, self.stats)

    def scalars(self):
        """the logged figures of the rollout just collected, one read-back: {"mean_termination_prob": ., "<family>_violation_rate": .,
        "<family>_max": .}"""
        rows = float(self.term_prob.numel())
        vals = torch.cat([self.term_prob.mean().reshape(1), self.counts.float() / rows,
                          torch.stack([self.c_max[c0:c1].max() for c0, c1 in self.table.ranges])]).tolist()
        F = self.table.F
        out = {"mean_termination_prob": vals[0]}
        for f, name in enumerate(self.spec.names):
            out[name + "_violation_rate"] = vals[1 + f]
            out[name + "_max"] = vals[1 + F + f]
        return out

    def checkpoint(self):
        return {**self.entry(), "c_max": self.c_max.detach().cpu().clone()}

    def _set_c_max(self, saved):
        saved = torch.as_tensor(saved, dtype=torch.float32)
        if tuple(saved.shape) != tuple(self.c_max.shape):
            raise ValueError(f"--constraints: the checkpoint's c_max has {saved.numel()} columns, this robot's spec expands into "
                             f"{self.c_max.numel()}")
        self.c_max.copy_(saved)

    def load_checkpoint(self, saved):
        """c_max of a checkpoint's entry (the spec was compared by the caller); prev restarts at zero"""
        if self.c_max is None:
            self._pending_c_max = saved["c_max"]
        else:
            self._set_c_max(saved["c_max"])
        if self.prev is not None:
            self.prev.zero_()
