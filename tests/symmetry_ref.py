"""Float64 numpy restatements for rl/symmetry.py, used by tests/test_symmetry.py and tests/test_symmetry_gpu.py.

The maps are derived here a second time, from LABELS: every column of an observation gets a name ("dof_pos:left_hip_roll_joint",
"heights:-0.3:0.2", ...), the mirror image of a name and its sign are written down per kind of quantity, and the permutation is looked
up by name -- no index arithmetic shared with rl/symmetry.py.  The gather and the augmented loss are restated on top of tests/ppo_ref.py."""
import numpy as np
import torch

from tests import ppo_ref


def _swap_side(name):
    if "left" in name:
        return name.replace("left", "right")
    if "right" in name:
        return name.replace("right", "left")
    return name


def _joint_sign(name):
    return 1.0 if "pitch" in name else -1.0   # (roll, yaw)


def frame_labels(dof_names):
    """(label, mirrored label, sign) per column of one observation frame (gr1t1.py:281-313)"""
    cols = [("cmd:vx", "cmd:vx", 1.0), ("cmd:vy", "cmd:vy", -1.0), ("cmd:yaw", "cmd:yaw", -1.0),
            ("ang:x", "ang:x", -1.0), ("ang:y", "ang:y", 1.0), ("ang:z", "ang:z", -1.0),
            ("grav:x", "grav:x", 1.0), ("grav:y", "grav:y", -1.0), ("grav:z", "grav:z", 1.0)]
    for kind in ("dof_pos", "dof_vel", "actions"):
        cols += [(f"{kind}:{n}", f"{kind}:{_swap_side(n)}", _joint_sign(n)) for n in dof_names]
    return cols


def privileged_labels(dof_names, xs, ys):
    cols = frame_labels(dof_names)
    cols += [("lin:x", "lin:x", 1.0), ("lin:y", "lin:y", -1.0), ("lin:z", "lin:z", 1.0), ("height_offset", "height_offset", 1.0)]
    cols += [("contact:left", "contact:right", 1.0), ("contact:right", "contact:left", 1.0)]
    cols += [("feet_height:left", "feet_height:right", 1.0), ("feet_height:right", "feet_height:left", 1.0)]
    cols += [(f"heights:{x:.4f}:{y:.4f}", f"heights:{x:.4f}:{-y + 0.0:.4f}", 1.0) for x in xs for y in ys]   # (+ 0.0: no "-0.0000")
    return [(a.replace("-0.0000", "0.0000"), b.replace("-0.0000", "0.0000"), s) for a, b, s in cols]


def map_from_labels(cols, history=1):
    """(perm int64, sign float64) of `history` stacked frames"""
    cols = [(f"{h}|{a}", f"{h}|{b}", s) for h in range(history) for a, b, s in cols]
    where = {a: i for i, (a, _, _) in enumerate(cols)}
    assert len(where) == len(cols)
    return np.array([where[b] for _, b, _ in cols], dtype=np.int64), np.array([s for _, _, s in cols], dtype=np.float64)


def joint_map_ref(dof_names):
    names = list(dof_names)
    return np.array([names.index(_swap_side(n)) for n in names], dtype=np.int64), np.array([_joint_sign(n) for n in names])


def normalized_ref(perm, sign, mean, std, eps):
    """de-normalise, mirror, normalise as ONE affine map, float64"""
    mean, std = np.asarray(mean, np.float64), np.asarray(std, np.float64)
    d = std + eps
    return sign * d[perm] / d, (sign * mean[perm] - mean) / d


def mirror_np(x, perm, scale, offset=None):
    y = np.asarray(x, np.float64)[..., perm] * scale
    return y if offset is None else y + offset


def gather_np(srcs, modes, maps, idx, mb):
    """grx_sym_gather_rows in numpy float64: maps[t] = (perm, scale, offset or None) for mode 2"""
    out = []
    for src, mode, m in zip(srcs, modes, maps):
        rows = np.asarray(src, np.float64)[:mb] if idx is None else np.asarray(src, np.float64)[np.asarray(idx)]
        if mode == 0:
            out.append(rows.copy())
        elif mode == 1:
            out.append(np.concatenate([rows, rows]))
        else:
            out.append(np.concatenate([rows, mirror_np(rows, *m)]))
    return out


def augmented_loss_ref(ac64, batch, maps, mode, coef, clip, value_loss_coef, entropy_coef, use_clipped):
    """The symmetric minibatch loss in float64 and its parameter gradients.
    ac64: a float64 ActorCriticMLP; batch: the nine UNMIRRORED minibatch tensors (obs, cobs, actions, target_values, advantages, returns,
    old_logp, old_mu, old_sigma); maps: dict obs / cobs / actions -> (perm, scale, offset or None) in float64.
    Returns dict: out [surrogate, value_loss, total (with coef * sym where the mode adds it), kl], sym, grads (per parameter, in order)."""
    b = [np.asarray(t.detach().cpu().double().numpy()) for t in batch]
    mb = b[0].shape[0]
    sig = (maps["actions"][0], np.abs(maps["actions"][1]), None)
    if mode in ("augment", "both"):
        modes = [2, 2, 2, 1, 1, 1, 1, 2, 2]
        tmaps = [maps["obs"], maps["cobs"], maps["actions"], None, None, None, None, maps["actions"], sig]
    else:
        modes, tmaps = [2] + [0] * 8, [maps["obs"]] + [None] * 8
    full = [torch.from_numpy(x) for x in gather_np(b, modes, tmaps, None, mb)]
    obs, cobs, actions, tv, adv, ret, old_logp, old_mu, old_sigma = full
    for p in ac64.parameters():
        p.grad = None
    mu, value = ac64.actor(obs), ac64.critic(cobs)
    n = actions.shape[0]
    ref = ppo_ref.ppo_loss_ref(mu[:n], ac64.std, value, actions, old_logp, old_mu, old_sigma, adv, ret, tv, clip, value_loss_coef, entropy_coef,
                               use_clipped)
    target = mirror_np(mu[:mb].detach().numpy(), *maps["actions"])
    diff = mu[mb:].detach().numpy() - target
    sym = float(np.mean(diff ** 2))
    d_mu = np.zeros(tuple(mu.shape))
    d_mu[:n] += ref["d_mu"].numpy()
    total = float(ref["out"][2])
    if mode in ("loss", "both"):
        d_mu[mb:] += coef * 2.0 * diff / diff.size
        total += coef * sym
    torch.autograd.backward([mu, value, ac64.std], [torch.from_numpy(d_mu), ref["d_value"], ref["d_std"]])
    out = ref["out"].clone()
    out[2] = total
    return {"out": out, "sym": sym, "grads": [p.grad.clone() for p in ac64.parameters()], "full": full}


def mirror_record(d, pre, jperm, jsign):
    """The left-right mirror image of the pipeline-state fields `pre`* of a golden fixture, field by field by physical meaning:
    root position y -> -y, quaternion (x, y, z, w) -> (-x, y, -z, w), linear velocity y negated, angular velocity x and z negated;
    q, qd, the action buffers and the torques through the joint map; commands (vx, vy, yaw rate) -> (vx, -vy, -yaw rate); the per-foot
    fields swapped, their vectors' y negated.  Everything else (episode length, height offset, termination contact) is a scalar of the
    whole robot and stays."""
    m = {k: np.array(d[k]) for k in d.files if k.startswith(pre)}
    for k in ("dof_pos", "dof_vel", "actions", "last_actions", "last_last_actions", "last_dof_vel", "torques"):
        m[pre + k] = m[pre + k][..., jperm] * jsign.astype(m[pre + k].dtype)
    root = m[pre + "root"]
    for col in (1, 3, 5, 8, 10, 12):   # y | qx, qz | vy | wx, wz
        root[:, col] *= -1
    m[pre + "commands"] = m[pre + "commands"] * np.array([1.0, -1.0, -1.0], dtype=m[pre + "commands"].dtype)
    m[pre + "torso_quat"] = m[pre + "torso_quat"] * np.array([-1.0, 1.0, -1.0, 1.0], dtype=m[pre + "torso_quat"].dtype)
    for k in ("air_time", "land_time", "contact_last", "avg_force"):
        m[pre + k] = m[pre + k][:, ::-1].copy()
    for k in ("feet_force", "feet_pos", "avg_speed"):
        v = m[pre + k][:, ::-1].copy()
        v[..., 1] *= -1
        m[pre + k] = v
    return m
