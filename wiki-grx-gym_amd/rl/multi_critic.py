"""Multi-critic PPO: the reward terms are split into K named GROUPS, the critic has one value head per group, GAE runs
per group, every group's advantage is normalised on its own, and the policy sees the weighted sum of the normalised group advantages
(HoST's stand-up controller, multi-critic parkour / keyframing policies).  A large dense group then no longer sets the scale in which a
small or sparse one has to be seen.

    spec         `name=term,term,...;name=term,...`; `*` (in at most one group) stands for every active term not named elsewhere.  An
                 active term is one whose scale is not zero in this task, from either term table, `termination` included.  Every active
                 term belongs to exactly one group, 1 <= K <= 8
    rollout      per env step the group rewards r_k[n] = sum of the step's per-term rewards (GRX_T_REWARD_TERMS, GRX_T_BASE_REWARD_TERMS) of
                 group k, in table index order, the main table first, one fp32 chain from zero; per head the time-out bootstrap
                 r_k += gamma v_k time_out.  v_k and r_k go to two tensors [T][N][K] of their own.  The ordinary transition store runs
                 unchanged with the env's own reward; its scalar value column holds sum_k v_k, for logging only
    returns      per group the GAE recursion of RolloutStorage.compute_returns on column k: returns_k, a_k = returns_k - v_k, then
                 A_k = (a_k - mean(a_k)) / (std_unbiased(a_k) + 1e-8) and advantages = sum_k w_k A_k, added in group order from zero; no
                 second normalisation.  K = 1, w = 1: RolloutStorage.compute_returns exactly
    loss         PPO's total with the value term replaced by sum_k L_k, L_k the clipped (or plain) value loss of head k against returns_k
                 and the stored v_k; the same clip_param and value_loss_coef for every head

On a HIP device the three operations are entry points of libgrx_ppo.so (include/grx_ppo_mc.h: grx_mc_store, grx_mc_returns, grx_mc_loss);
`mc_store_torch`, `mc_returns_torch` and `mc_loss_torch` are the definition, the CPU path, and what GRX_MC_FUSED=0 selects on a HIP device.
Not a config key: `--reward_groups` / `--reward_group_weights` or assignments to train_cfg.algorithm set it; without it nothing of this
module is imported, and the grx_mc_* prototypes are bound on the first call that needs them."""
import ctypes as C
import math
import os

import torch

MAX_GROUPS = 8          # include/grx_ppo_mc.h GRX_MC_MAX_GROUPS
MAX_ROWS = 1 << 24      # grx_mc_returns' largest T N

_BOUND = None           # libgrx_ppo.so with the grx_mc_* prototypes set up: None until a fused call needs them


def fused_enabled():
    return os.environ.get("GRX_MC_FUSED", "1") != "0"


def _lib():
    global _BOUND
    if _BOUND is None:
        from .fused_loss import load_ppo_library
        lib = load_ppo_library()
        fp = C.c_void_p
        lib.grx_mc_store.restype = C.c_int
        lib.grx_mc_store.argtypes = [C.c_int] * 4 + [fp] * 5 + [C.c_float, fp, fp, C.c_void_p]
        lib.grx_mc_partials_size.restype = C.c_int
        lib.grx_mc_partials_size.argtypes = [C.c_int] * 3
        lib.grx_mc_returns.restype = C.c_int
        lib.grx_mc_returns.argtypes = [C.c_int] * 3 + [fp] * 4 + [C.POINTER(C.c_float), C.c_float, C.c_float] + [fp] * 4 + [C.c_void_p]
        lib.grx_mc_loss_partials_size.restype = C.c_int
        lib.grx_mc_loss_partials_size.argtypes = [C.c_int]
        lib.grx_mc_loss.restype = C.c_int
        lib.grx_mc_loss.argtypes = [C.c_int] * 3 + [fp] * 10 + [C.c_float] * 3 + [C.c_int] + [fp] * 5 + [C.c_void_p]
        _BOUND = lib
    return _BOUND


# ---------------------------------------------------------------------------------------------------------------- the group spec
class RewardGroups:
    """a parsed spec: `names` in the spec's order, `terms[name]` the group's active terms in table order (main table first), and
    `term_group`, one entry per row of the main table followed by one per row of the base table: the row's group, or -1"""

    def __init__(self, names, terms, term_group, num_main, num_base):
        self.names, self.terms, self.term_group = list(names), {n: list(terms[n]) for n in names}, [int(g) for g in term_group]
        self.num_main, self.num_base = int(num_main), int(num_base)

    @property
    def K(self):
        return len(self.names)

    @property
    def uses_base(self):
        return any(g >= 0 for g in self.term_group[self.num_main:])

    def entry(self, weights):
        """the "multi_critic" entry of a checkpoint"""
        return {"groups": {n: list(self.terms[n]) for n in self.names}, "weights": [float(w) for w in weights]}


def parse_reward_groups(spec, active, main_table, base_table=()):
    """`spec` against a task: `active` the names of its active terms, `main_table` / `base_table` the two term tables' names in index
    order.  Raises ValueError on anything the module's docstring rules out; an unknown or inactive name lists the active ones."""
    if not isinstance(spec, str) or not spec.strip():
        raise ValueError(f"--reward_groups needs a spec `name=term,term,...;name=...`, not {spec!r}")
    table = list(main_table) + list(base_table)
    active = [t for t in table if t in set(active)]   # table order
    names, listed, star = [], {}, None
    for part in spec.split(";"):
        part = part.strip()
        if not part:
            continue
        if "=" not in part:
            raise ValueError(f"--reward_groups: {part!r} is not `name=term,term,...`")
        name, _, rhs = part.partition("=")
        name = name.strip()
        if not name or not all(c.isalnum() or c in "_-" for c in name):
            raise ValueError(f"--reward_groups: {name!r} is not a group name (letters, digits, _ and -)")
        if name in listed:
            raise ValueError(f"--reward_groups: group {name!r} appears twice")
        terms = [t.strip() for t in rhs.split(",") if t.strip()]
        if not terms:
            raise ValueError(f"--reward_groups: group {name!r} lists no term")
        names.append(name)
        listed[name] = []
        for t in terms:
            if t == "*":
                if star is not None:
                    raise ValueError("--reward_groups: `*` may appear in one group only")
                star = name
                continue
            if t not in active:
                why = "is not a reward term" if t not in table else "is not active in this task (its scale is 0)"
                raise ValueError(f"--reward_groups: {t!r} {why}; the active terms are {', '.join(active)}")
            owner = [n for n in names if t in listed[n]]
            if owner:
                raise ValueError(f"--reward_groups: term {t!r} is in two groups ({owner[0]!r} and {name!r})" if owner[0] != name
                                 else f"--reward_groups: term {t!r} appears twice in group {name!r}")
            listed[name].append(t)
    if not 1 <= len(names) <= MAX_GROUPS:
        raise ValueError(f"--reward_groups: {len(names)} groups, the number of groups must be in 1..{MAX_GROUPS}")
    taken = {t for n in names for t in listed[n]}
    rest = [t for t in active if t not in taken]
    if star is not None:
        listed[star] += rest
    elif rest:
        raise ValueError(f"--reward_groups: the active terms {', '.join(rest)} are in no group (add them, or `*` to one group)")
    empty = [n for n in names if not listed[n]]
    if empty:
        raise ValueError(f"--reward_groups: group {empty[0]!r} holds no active term")
    group_of = {t: k for k, n in enumerate(names) for t in listed[n]}
    terms = {n: [t for t in table if group_of.get(t) == k] for k, n in enumerate(names)}
    return RewardGroups(names, terms, [group_of.get(t, -1) for t in table], len(main_table), len(base_table))


def parse_weights(weights, K):
    """K weights, each finite and > 0: None (all 1.0), a `w1,...,wK` string or a sequence"""
    if weights is None:
        return [1.0] * K
    if isinstance(weights, str):
        try:
            weights = [float(w) for w in weights.split(",") if w.strip()]
        except ValueError:
            raise ValueError(f"--reward_group_weights must be `w1,...,wK`, not {weights!r}") from None
    try:
        w = [float(x) for x in weights]
    except TypeError:
        raise ValueError(f"--reward_group_weights must be `w1,...,wK`, not {weights!r}") from None
    if len(w) != K:
        raise ValueError(f"--reward_group_weights: {len(w)} weights for {K} groups of --reward_groups")
    if any(not (math.isfinite(x) and x > 0.0) for x in w):
        raise ValueError(f"--reward_group_weights: every weight must be finite and > 0, not {w}")
    return w


# ---------------------------------------------------------------------------------------------------------------- the torch spelling
def mc_store_torch(terms, base_terms, term_group, values, time_outs, gamma, st_values, st_rewards):
    """the definition of grx_mc_store: terms [NT, N], base_terms [NB, N] or None, term_group a list of NT (+ NB) ints, values [N, K],
    time_outs [N] (bool / uint8) or None; writes st_values / st_rewards [N, K] in place"""
    N, K = values.shape
    NT = terms.shape[0]
    cols = [torch.zeros(N, dtype=values.dtype, device=values.device) for _ in range(K)]
    for t, g in enumerate(term_group):
        if g < 0:
            continue
        if not g < K:
            raise ValueError(f"mc_store: term {t} feeds group {g}, there are {K}")
        cols[g] = cols[g] + (terms[t] if t < NT else base_terms[t - NT])
    r = torch.stack(cols, dim=1)
    if time_outs is not None:
        r = r + torch.where(time_outs.reshape(N, 1) != 0, gamma * values, torch.zeros_like(values))
    st_values.copy_(values)
    st_rewards.copy_(r)


def mc_returns_torch(rewards, values, dones, last_values, weights, gamma, lam, returns, advantages, stats=None):
    """the definition of grx_mc_returns, in place: rewards / values / returns [T, N, K], dones [T, N] or [T, N, 1], last_values [N, K],
    advantages [T, N] or [T, N, 1], stats [K, 2] or None.  No host synchronisation."""
    T, N, K = rewards.shape
    adv = 0
    for step in reversed(range(T)):
        nxt = last_values if step == T - 1 else values[step + 1]
        alive = 1.0 - dones[step].float().reshape(N, 1)
        delta = rewards[step] + alive * gamma * nxt - values[step]
        adv = delta + alive * gamma * lam * adv
        returns[step] = adv + values[step]
    a = returns - values
    out = torch.zeros(T, N, dtype=rewards.dtype, device=rewards.device)
    rows = []
    for k in range(K):
        ak = a[..., k].contiguous()
        m, s = ak.mean(), ak.std()
        out = out + float(weights[k]) * ((ak - m) / (s + 1e-8))
        rows.append(torch.stack([m, s]))
    advantages.copy_(out.reshape(advantages.shape))
    if stats is not None:
        stats.copy_(torch.stack(rows))


def mc_loss_torch(mu, sigma, value, actions, old_logp, old_mu, old_sigma, advantages, returns, target_values, clip_param,
                  value_loss_coef, entropy_coef, use_clipped_value_loss, adaptive=True):
    """the definition of grx_mc_loss, differentiable: mu / sigma / actions / old_mu / old_sigma [B, A], value / returns / target_values
    [B, K], old_logp / advantages [B] or [B, 1] -> (surrogate_loss, value_loss, loss, kl_mean, head_losses [K]).  PPO._loss_terms' torch
    expression with the value term summed over the heads."""
    dist_ = torch.distributions.Normal(mu, sigma, validate_args=False)
    logp, entropy = dist_.log_prob(actions).sum(dim=-1), dist_.entropy().sum(dim=-1)
    kl_mean = torch.zeros((), device=mu.device, dtype=mu.dtype)
    if adaptive:
        with torch.no_grad():
            kl_mean = torch.sum(torch.log(sigma / old_sigma + 1.e-5) + (old_sigma.square() + (old_mu - mu).square())
                                / (2.0 * sigma.square()) - 0.5, axis=-1).mean()
    ratio = torch.exp(logp - old_logp.reshape(-1))
    adv = advantages.reshape(-1)
    surrogate_loss = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1.0 - clip_param, 1.0 + clip_param)).mean()
    heads = []
    for k in range(value.shape[1]):
        v, ret = value[:, k:k + 1], returns[:, k:k + 1]
        if use_clipped_value_loss:
            tv = target_values[:, k:k + 1]
            clipped = tv + (v - tv).clamp(-clip_param, clip_param)
            heads.append(torch.max((v - ret).pow(2), (clipped - ret).pow(2)).mean())
        else:
            heads.append((ret - v).pow(2).mean())
    value_loss = heads[0]
    for h in heads[1:]:
        value_loss = value_loss + h
    loss = surrogate_loss + value_loss_coef * value_loss - entropy_coef * entropy.mean()
    return surrogate_loss, value_loss, loss, kl_mean, torch.stack([h.detach() for h in heads])


# ---------------------------------------------------------------------------------------------------------------- through libgrx_ppo.so
def _ok(t, dtype=torch.float32):
    return t.is_cuda and t.dtype == dtype and t.is_contiguous()


def mc_store_hip(terms, base_terms, term_group, values, time_outs, gamma, st_values, st_rewards):
    """the same through grx_mc_store (one launch on the current stream): term_group an int32 tensor of NT (+ NB) entries on the device"""
    lib = _lib()
    N, K = values.shape
    NT, NB = terms.shape[0], (base_terms.shape[0] if base_terms is not None else 0)
    if time_outs is not None:
        if time_outs.dtype == torch.bool:
            time_outs = time_outs.view(torch.uint8)
        elif time_outs.dtype != torch.uint8:
            time_outs = (time_outs != 0).to(torch.uint8)
    if not all(_ok(t) for t in (terms, values, st_values, st_rewards)) or (base_terms is not None and not _ok(base_terms)) \
            or not _ok(term_group, torch.int32) or term_group.numel() != NT + NB or terms.shape[1] != N \
            or (base_terms is not None and base_terms.shape[1] != N) or st_values.numel() != N * K or st_rewards.numel() != N * K \
            or (time_outs is not None and not (_ok(time_outs, torch.uint8) and time_outs.numel() == N)):
        raise RuntimeError("grx_mc_store needs contiguous tensors on one HIP device: float32 terms [NT, N] (/ base_terms [NB, N]), values / "
                           "st_values / st_rewards [N, K], an int32 term_group [NT + NB], uint8 time_outs [N]")
    ptr = lambda t: t.data_ptr() if t is not None else None
    with torch.cuda.device(values.device):
        rc = lib.grx_mc_store(N, K, NT, NB, ptr(terms), ptr(base_terms), ptr(term_group), ptr(values), ptr(time_outs), float(gamma),
                              ptr(st_values), ptr(st_rewards), C.c_void_p(torch.cuda.current_stream(values.device).cuda_stream))
    if rc != 0:
        raise RuntimeError(f"grx_mc_store failed ({rc}): N = {N}, K = {K}, NT = {NT}, NB = {NB}")


def mc_partials(T, N, K, device):
    """the scratch one grx_mc_returns call at (T, N, K) needs"""
    size = _lib().grx_mc_partials_size(T, N, K)
    if size < 1:
        raise RuntimeError(f"grx_mc_partials_size: invalid shape T = {T}, N = {N}, K = {K}")
    with torch.inference_mode(False):
        return torch.empty(size, device=device, dtype=torch.float32)


def mc_returns_hip(rewards, values, dones, last_values, weights, gamma, lam, returns, advantages, stats=None, partials=None):
    """the same through grx_mc_returns: three launches on the current stream; `stats` [K, 2] and `partials` (mc_partials) are allocated
    here when they are not given.  Returns stats."""
    lib = _lib()
    T, N, K = rewards.shape
    if not all(_ok(t) and t.device == rewards.device for t in (rewards, values, returns, advantages, last_values)) \
            or values.numel() != T * N * K or returns.numel() != T * N * K or advantages.numel() != T * N or last_values.numel() != N * K \
            or not (_ok(dones, torch.uint8) and dones.numel() == T * N):
        raise RuntimeError("grx_mc_returns needs contiguous tensors on one HIP device: float32 rewards / values / returns [T, N, K], "
                           "advantages [T, N], last_values [N, K] and uint8 dones [T, N]")
    if stats is None:
        with torch.inference_mode(False):
            stats = torch.empty(K, 2, device=rewards.device, dtype=torch.float32)
    part = partials if partials is not None else mc_partials(T, N, K, rewards.device)
    w = (C.c_float * K)(*[float(x) for x in weights])
    with torch.cuda.device(rewards.device):
        rc = lib.grx_mc_returns(T, N, K, rewards.data_ptr(), values.data_ptr(), dones.data_ptr(), last_values.data_ptr(), w, float(gamma),
                                float(lam), returns.data_ptr(), advantages.data_ptr(), stats.data_ptr(), part.data_ptr(),
                                C.c_void_p(torch.cuda.current_stream(rewards.device).cuda_stream))
    if rc != 0:
        raise RuntimeError(f"grx_mc_returns failed ({rc}): T = {T}, N = {N}, K = {K}")
    return stats


class FusedMCLoss(torch.autograd.Function):
    """(mu [B, A], std [A], value [B, K]; data...) -> tensor [surrogate, value_loss, total_loss, mean_kl, L_0 .. L_K-1] (grx_mc_loss)"""

    @staticmethod
    def forward(ctx, mu, std, value, actions, old_logp, old_mu, old_sigma, advantages, returns, target_values,
                clip_param, value_loss_coef, entropy_coef, use_clipped_value_loss):
        from .fused_loss import _f32c
        lib = _lib()
        B, A = mu.shape
        K = value.shape[1]
        mu_c, std_c, value_c = _f32c(mu), _f32c(std), _f32c(value)
        data = [_f32c(t) for t in (actions, old_logp, old_mu, old_sigma, advantages, returns, target_values)]
        if tuple(data[5].shape) != (B, K) or tuple(data[6].shape) != (B, K):
            raise RuntimeError(f"fused_mc_loss: returns / target_values are {tuple(data[5].shape)} / {tuple(data[6].shape)}, expected {(B, K)}")
        out = torch.empty(4 + K, device=mu.device, dtype=torch.float32)
        d_mu, d_std, d_value = torch.empty_like(mu_c), torch.empty_like(std_c), torch.empty_like(value_c)
        partials = torch.empty(lib.grx_mc_loss_partials_size(B), device=mu.device, dtype=torch.float32)
        stream = torch.cuda.current_stream(mu.device).cuda_stream
        with torch.cuda.device(mu.device):
            rc = lib.grx_mc_loss(B, A, K, mu_c.data_ptr(), std_c.data_ptr(), value_c.data_ptr(), *[t.data_ptr() for t in data],
                                 float(clip_param), float(value_loss_coef), float(entropy_coef), int(bool(use_clipped_value_loss)),
                                 out.data_ptr(), d_mu.data_ptr(), d_std.data_ptr(), d_value.data_ptr(), partials.data_ptr(), C.c_void_p(stream))
        if rc != 0:
            raise RuntimeError(f"grx_mc_loss failed ({rc}): batch {B}, num_actions {A}, groups {K}")
        ctx.save_for_backward(d_mu, d_std, d_value)
        return out

    @staticmethod
    def backward(ctx, g):
        d_mu, d_std, d_value = ctx.saved_tensors
        gl = g[2]   # only the total loss is differentiable
        return (d_mu * gl, d_std * gl, d_value * gl) + (None,) * 11


def fused_mc_loss(mu, std, value, actions, old_logp, old_mu, old_sigma, advantages, returns, target_values,
                  clip_param, value_loss_coef, entropy_coef, use_clipped_value_loss):
    return FusedMCLoss.apply(mu, std, value, actions, old_logp, old_mu, old_sigma, advantages, returns, target_values,
                             clip_param, value_loss_coef, entropy_coef, use_clipped_value_loss)


# ---------------------------------------------------------------------------------------------------------------- what PPO holds
class MultiCritic:
    """the groups, their weights, the two K-wide storage tensors beside RolloutStorage's and the rollout's passes over them"""

    def __init__(self, groups, weights=None, device="cpu"):
        if not isinstance(groups, RewardGroups):
            raise ValueError("PPO: reward_groups must be an rl.multi_critic.RewardGroups (parse_reward_groups(spec, ...)), "
                             f"not {type(groups).__name__}")
        self.groups, self.K, self.device = groups, groups.K, device
        self.weights = parse_weights(weights, self.K)
        # (grx_mc_store cannot see a bad map entry from the host -- its launch then writes nothing, silently: checked here, once)
        if len(groups.term_group) != groups.num_main + groups.num_base or any(not -1 <= g < self.K for g in groups.term_group):
            raise ValueError(f"PPO: reward_groups' term_group must hold {groups.num_main + groups.num_base} entries in -1..{self.K - 1}, "
                             f"not {groups.term_group}")
        self.term_group = torch.tensor(groups.term_group, dtype=torch.int32, device=device)
        self.terms = self.base_terms = None          # the step kernel's per-term tables: bind_tables
        self.values = self.rewards = self.returns = None   # [T, N, K]: init_storage
        self.stats = torch.zeros(self.K, 2, device=device)        # (mean, unbiased std) of every group's raw advantage, last rollout
        self.head_sum = torch.zeros(self.K, device=device)        # the update's sums of the heads' value losses (finite steps)
        self.mean_head_losses = [0.0] * self.K
        self._partials, self._partials_key = None, None

    def entry(self):
        return self.groups.entry(self.weights)

    def bind_tables(self, terms, base_terms=None):
        """the per-term reward tables [NT, N] / [NB, N] the env's step kernel writes (GRX_T_REWARD_TERMS, GRX_T_BASE_REWARD_TERMS)"""
        g = self.groups
        if terms is None or terms.shape[0] != g.num_main:
            raise ValueError(f"--reward_groups: the reward-term table has {None if terms is None else terms.shape[0]} rows, the groups were "
                             f"parsed against {g.num_main}")
        if g.uses_base and (base_terms is None or base_terms.shape[0] != g.num_base):
            raise ValueError("--reward_groups: a group holds base reward terms, the env publishes no base reward-term table")
        self.terms, self.base_terms = terms, (base_terms if g.uses_base else None)

    def init_storage(self, num_envs, num_transitions_per_env):
        z = lambda: torch.zeros(num_transitions_per_env, num_envs, self.K, device=self.device)
        self.values, self.rewards, self.returns = z(), z(), z()

    def _fused(self, t):
        return t.is_cuda and fused_enabled()

    def store(self, step, values, time_outs, gamma):
        """one rollout step: the group rewards from the tables as the step kernel left them, the per-head bootstrap, rows `step` of
        values / rewards; returns sum_k v_k [N, 1] for the scalar transition store"""
        if self.terms is None:
            raise RuntimeError("--reward_groups: no reward-term tables are bound (MultiCritic.bind_tables)")
        if tuple(values.shape) != tuple(self.values[step].shape):
            raise RuntimeError(f"--reward_groups: the critic returned values of shape {tuple(values.shape)}, expected "
                               f"{tuple(self.values[step].shape)} (one head per group)")
        if self._fused(values):
            tg = self.term_group if self.base_terms is not None else self.term_group[:self.groups.num_main]
            mc_store_hip(self.terms, self.base_terms, tg, values if values.is_contiguous() else values.contiguous(), time_outs, gamma,
                         self.values[step], self.rewards[step])
        else:
            mc_store_torch(self.terms.to(values.device), None if self.base_terms is None else self.base_terms.to(values.device),
                           self.groups.term_group, values, None if time_outs is None else time_outs.to(values.device), gamma,
                           self.values[step], self.rewards[step])
        return values.sum(dim=-1, keepdim=True)

    def compute_returns(self, storage, last_values, gamma, lam):
        """once per iteration: returns_k [T, N, K] and storage.advantages [T, N, 1], in place"""
        st = storage
        T, N = st.num_transitions_per_env, st.num_envs
        if T * N > MAX_ROWS:
            raise ValueError(f"--reward_groups: a rollout of {T * N} transitions per update is more than {MAX_ROWS}")
        last_values = last_values.detach()
        if self._fused(self.returns):
            key = (T, N, self.K, self.returns.device)
            if self._partials_key != key:
                self._partials, self._partials_key = mc_partials(T, N, self.K, self.returns.device), key
            mc_returns_hip(self.rewards, self.values, st.dones, last_values.contiguous(), self.weights, gamma, lam, self.returns,
                           st.advantages, self.stats, self._partials)
        else:
            mc_returns_torch(self.rewards, self.values, st.dones, last_values, self.weights, gamma, lam, self.returns, st.advantages,
                             self.stats)

    def mini_batch_generator(self, storage, num_mini_batches, num_epochs=8):
        """RolloutStorage.mini_batch_generator with the K-wide values / returns in the scalar columns' places"""
        st = storage
        batch = st.num_envs * st.num_transitions_per_env
        mb = batch // num_mini_batches
        indices = torch.randperm(num_mini_batches * mb, requires_grad=False, device=st.device)
        flat = lambda x: x.flatten(0, 1)
        obs = flat(st.observations)
        cobs = flat(st.pri_observations) if st.pri_observations is not None else obs
        cols = [flat(x) for x in (st.actions, self.values, st.advantages, self.returns, st.actions_log_prob, st.mu, st.sigma)]
        for _ in range(num_epochs):
            for i in range(num_mini_batches):
                idx = indices[i * mb:(i + 1) * mb]
                yield (obs[idx], cobs[idx], *[c[idx] for c in cols], (None, None), None)

    def loss(self, mu, std, value, actions, old_logp, old_mu, old_sigma, advantages, returns, target_values, clip_param, value_loss_coef,
             entropy_coef, use_clipped_value_loss, adaptive, fused):
        """(surrogate_loss, value_loss, loss, kl_mean) of one minibatch; the heads' own losses are added to `head_sum` (a step whose loss
        is not finite adds nothing)"""
        if fused and self._fused(mu):
            out = fused_mc_loss(mu, std, value, actions, old_logp, old_mu, old_sigma, advantages, returns, target_values, clip_param,
                                value_loss_coef, entropy_coef, use_clipped_value_loss)
            kl_mean = out[3].detach() if adaptive else torch.zeros((), device=mu.device)
            res, heads = (out[0], out[1], out[2], kl_mean), out[4:].detach()
        else:
            sigma = mu * 0.0 + std   # (ActorCriticMLP.update_distribution's sigma)
            *res, heads = mc_loss_torch(mu, sigma, value, actions, old_logp, old_mu, old_sigma, advantages, returns, target_values,
                                        clip_param, value_loss_coef, entropy_coef, use_clipped_value_loss, adaptive)
            res = tuple(res)
        with torch.no_grad():
            self.head_sum += torch.where(torch.isfinite(res[2].detach()), heads, torch.zeros_like(heads))
        return res
