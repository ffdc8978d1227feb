"""Left-right symmetry for PPO (rsl_rl 2.x `symmetry_cfg`): the mirror maps of the GR1 robots' observations and actions,
and the minibatch gather that appends a minibatch's mirror image.

A map for a tensor of width W is (perm int32 [W], scale f32 [W], offset f32 [W] or None):

    mirror(x)[j] = scale[j] * x[perm[j]] + offset[j]

The joint map J comes from the joint NAMES alone: the partner of a joint swaps its side token (left <-> right; a name without one is its
own partner), the sign is -1 for a roll or yaw joint and +1 for a pitch joint -- reflecting the robot in its sagittal (x, z) plane
reverses rotations about x and z and keeps those about y.  Anything else is refused, never guessed.  The observation frame
(9 + 3 nd columns, gr1t1.py:281-313) and the privileged tail (3 + 1 + 2 + 2 + the height scan) map column by column, see
`frame_map` / `privileged_tail_map`; a history tiles the frame map; under empirical normalisation the stored rows are normalised, and
`normalized` folds "de-normalise, mirror, normalise" into scale and offset.

`sym_gather_torch` is the definition of grx_sym_gather_rows (include/grx_ppo.h) in torch: what CPU tensors use, and what
GRX_SYM_FUSED=0 selects on a HIP device (the cross-check, as GRX_LSTM_FUSED is to the LSTM cell)."""
import os

import torch

MODES = ("augment", "loss", "both")
SIDES = ("left", "right")
MAX_WIDTH = 2048   # include/grx_ppo.h GRX_SYM_MAX_WIDTH: what the gather kernel's LDS staging holds


def _partner_name(name):
    tokens = name.split("_")
    sides = [i for i, t in enumerate(tokens) if t in SIDES]
    if not sides:
        return name
    if len(sides) > 1:
        raise ValueError(f"symmetry: joint {name!r} carries more than one side token: its mirror partner cannot be told from its name")
    i = sides[0]
    tokens[i] = SIDES[1 - SIDES.index(tokens[i])]
    return "_".join(tokens)


def joint_map(dof_names):
    """(perm, sign) lists of the joint mirror map J, from the joint names alone"""
    names = list(dof_names)
    index = {n: i for i, n in enumerate(names)}
    perm, sign = [], []
    for n in names:
        p = _partner_name(n)
        if p not in index:
            raise ValueError(f"symmetry: joint {n!r} has no mirror partner {p!r} in this robot")
        kinds = [k for k in ("roll", "yaw", "pitch") if k in n]
        if len(kinds) != 1:
            raise ValueError(f"symmetry: joint {n!r} is named neither roll, yaw nor pitch (or more than one of them): its mirror sign "
                             "cannot be told from its name")
        perm.append(index[p])
        sign.append(1.0 if kinds[0] == "pitch" else -1.0)
    return perm, sign


def _concat(parts):
    """[(perm within the part, sign), ...] -> (perm, sign) of the concatenated columns"""
    perm, sign, o = [], [], 0
    for p, s in parts:
        perm += [o + k for k in p]
        sign += list(s)
        o += len(p)
    return perm, sign


def frame_map(dof_names):
    """one observation frame (gr1t1.py:281-313): commands (vx, vy, yaw rate) (+, -, -), base angular velocity (-, +, -), projected
    gravity (+, -, +), then dof_pos_offset, dof_vel and actions through J"""
    J = joint_map(dof_names)
    ident = [0, 1, 2]
    return _concat([(ident, [1.0, -1.0, -1.0]), (ident, [-1.0, 1.0, -1.0]), (ident, [1.0, -1.0, 1.0]), J, J, J])


def height_perm(points_x, points_y):
    """the scan's permutation: the sample at (x, y) comes from the sample at (x, -y); the scan is laid out x-major
    (envs/build_config.py: `for x in measured_points_x for y in measured_points_y`)"""
    xs, ys = [float(x) for x in points_x], [float(y) for y in points_y]
    where = {}
    for k, y in enumerate(ys):
        where.setdefault(round(y, 9), k)
    other = []
    for y in ys:
        k = where.get(round(-y, 9))
        if k is None:
            raise ValueError(f"symmetry: measured_points_y {ys} is not symmetric about 0 (no sample at y = {-y})")
        other.append(k)
    ny = len(ys)
    return [ix * ny + other[iy] for ix in range(len(xs)) for iy in range(ny)]


def privileged_tail_map(points_x=(), points_y=()):
    """base linear velocity (+, -, +), base height offset +, feet_contact swapped, feet_height swapped, the height scan permuted"""
    hp = height_perm(points_x, points_y) if len(points_x) and len(points_y) else []
    return _concat([([0, 1, 2], [1.0, -1.0, 1.0]), ([0], [1.0]), ([1, 0], [1.0, 1.0]), ([1, 0], [1.0, 1.0]), (hp, [1.0] * len(hp))])


def privileged_map(dof_names, points_x=(), points_y=()):
    """one privileged frame: the (noise-free) observation frame, then the privileged tail"""
    return _concat([frame_map(dof_names), privileged_tail_map(points_x, points_y)])


def tiled(m, history):
    """the map of `history` stacked frames"""
    return _concat([m] * int(history))


def check_map(perm, width, what="map"):
    """a map's perm must be a permutation of 0..width-1 (the gather kernel trusts it)"""
    p = [int(k) for k in perm]
    if len(p) != width or any(k < 0 or k >= width for k in p):
        raise ValueError(f"symmetry: the {what}'s perm has an entry outside 0..{width - 1} or not {width} entries")
    if sorted(p) != list(range(width)):
        raise ValueError(f"symmetry: the {what}'s perm is not a permutation")


def normalized(perm, sign, mean, std, eps):
    """(scale, offset) of "de-normalise, mirror, normalise" for rows stored as (x - mean) / (std + eps):
    scale[j] = s_j (std[p_j] + eps) / (std[j] + eps), offset[j] = (s_j mean[p_j] - mean[j]) / (std[j] + eps)"""
    d = std + eps
    return sign * d[perm] / d, (sign * mean[perm] - mean) / d


def apply_map(x, perm, scale, offset=None):
    """mirror(x) along the last dimension (torch; the definition)"""
    y = x.index_select(-1, perm.long()) * scale
    return y if offset is None else y + offset


class MirrorMap:
    """one tensor's map as device tensors that are REWRITTEN IN PLACE (a normaliser's statistics move): the gather's pointer arguments
    never see a new address"""

    def __init__(self, perm, sign, device, what="map"):
        check_map(perm, len(perm), what)
        if len(perm) > MAX_WIDTH:
            raise ValueError(f"symmetry: the {what} is {len(perm)} columns wide, the mirrored gather stages at most {MAX_WIDTH} "
                             "(shorten --obs_history / --critic_obs_history, or drop --symmetry)")
        self.width = len(perm)
        self.perm = torch.tensor(perm, dtype=torch.int32, device=device)
        self.sign = torch.tensor(sign, dtype=torch.float32, device=device)
        self.scale = self.sign.clone()
        self.offset = None
        self._perm_long = self.perm.long()

    @torch.no_grad()
    def set_normalizer(self, norm):
        """fold the normaliser's current statistics into scale / offset, in place"""
        mean, std = norm._mean.reshape(-1).to(self.sign.device), norm._std.reshape(-1).to(self.sign.device)
        scale, offset = normalized(self._perm_long, self.sign, mean, std, norm.eps)
        self.scale.copy_(scale)
        if self.offset is None:
            self.offset = torch.empty_like(self.scale)
        self.offset.copy_(offset)

    def abs_scale(self):
        """the same permutation with |scale| and no offset (a standard deviation's map); a view of nothing: a tensor of its own"""
        m = object.__new__(MirrorMap)
        m.width, m.perm, m.sign, m._perm_long = self.width, self.perm, self.sign.abs(), self._perm_long
        m.scale, m.offset = self.scale.abs(), None
        return m

    def __call__(self, x):
        return apply_map(x, self._perm_long, self.scale, self.offset)


class SymmetryMaps:
    """what PPO needs: the maps of the actor's input, the critic's input, the actions and sigma"""

    def __init__(self, obs, cobs, actions, obs_normalizer=None, critic_obs_normalizer=None):
        self.obs, self.cobs, self.actions = obs, cobs, actions
        self.sigma = actions.abs_scale()
        self.obs_normalizer, self.critic_obs_normalizer = obs_normalizer, critic_obs_normalizer
        self.refresh()   # (the offset tensors exist from here on: a gather built later keeps their addresses)

    def refresh(self):
        """once per update(): the normalisers' statistics as they are now (no normaliser: nothing to do)"""
        if self.obs_normalizer is not None:
            self.obs.set_normalizer(self.obs_normalizer)
        if self.critic_obs_normalizer is not None and self.cobs is not self.obs:
            self.cobs.set_normalizer(self.critic_obs_normalizer)


def env_maps(env):
    """(frame map, privileged frame map or None, joint map) of an env as (perm, sign) lists"""
    names = list(env.dof_names)
    J = joint_map(names)
    frame = frame_map(names)
    if len(frame[0]) != env.num_obs:
        raise ValueError(f"symmetry: this env's observation has {env.num_obs} columns, the mirror map knows the {len(frame[0])}-column "
                         "frame 9 + 3 * num_dof only")
    pri = None
    if env.num_pri_obs is not None:
        t = env.cfg.terrain
        measure = bool(getattr(t, "measure_heights", False))
        pri = privileged_map(names, t.measured_points_x if measure else (), t.measured_points_y if measure else ())
        if len(pri[0]) != env.num_pri_obs:
            raise ValueError(f"symmetry: this env's privileged observation has {env.num_pri_obs} columns, the mirror map covers {len(pri[0])}")
    return frame, pri, J


def build_maps(env, device, obs_history=1, critic_obs_history=1, privileged_actor=False, obs_normalizer=None, critic_obs_normalizer=None):
    """the runner's maps: the frame maps tiled by the history lengths; a privileged actor's map IS the critic's"""
    frame, pri, J = env_maps(env)
    critic = MirrorMap(*tiled(pri, critic_obs_history), device, "critic observation map") if pri is not None else None
    if privileged_actor:
        if critic is None:
            raise ValueError("symmetry with --privileged_actor: this env has no privileged observations")
        actor = critic
    else:
        actor = MirrorMap(*tiled(frame, obs_history), device, "observation map")
    if privileged_actor:
        obs_normalizer = critic_obs_normalizer
    if critic is None:   # no privileged observations: the critic reads the actor's tensor
        critic, critic_obs_normalizer = actor, obs_normalizer
    return SymmetryMaps(actor, critic, MirrorMap(*J, device, "action map"), obs_normalizer, critic_obs_normalizer)


# ---- the gather ------------------------------------------------------------------------------------------------------------------------
def fused_enabled():
    return os.environ.get("GRX_SYM_FUSED", "1") != "0"


def sym_gather_torch(srcs, dsts, modes, maps, idx=None):
    """grx_sym_gather_rows in torch: for every tensor t and r < mb, dst[t][r] = src[t][idx[r]] (idx None: src[t][r]) and
    dst[t][mb + r] = that row again (mode 1), its mirror image maps[t](row) (mode 2: fmaf(scale, row[perm], offset), a plain product
    without an offset) or nothing (mode 0: dst[t] has mb rows)."""
    for src, dst, mode, m in zip(srcs, dsts, modes, maps):
        if mode not in (0, 1, 2):
            raise ValueError(f"sym_gather_torch: mode {mode}")
        mb = dst.shape[0] // (2 if mode else 1)
        rows = src[:mb] if idx is None else src.index_select(0, idx)
        dst[:mb].copy_(rows)
        if mode == 1:
            dst[mb:].copy_(rows)
        elif mode == 2:
            picked = rows.index_select(-1, m._perm_long)
            # (addcmul rounds once on a HIP device, as the kernel's fmaf; on the CPU the product is rounded first: within 2^-23 (|scale x| + |offset|))
            dst[mb:].copy_(picked * m.scale if m.offset is None else torch.addcmul(m.offset.expand_as(picked), picked, m.scale))
