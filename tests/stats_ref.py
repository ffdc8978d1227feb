"""The quantities that reduce ACROSS envs, restated in float64 numpy with no oracle and no kernel in them: extras["episode"] of a step
and of a reset outside a step (legged_robot.py:387-388, 420-428), the same over legged_gym's base terms, and the command curriculum's
decision (legged_robot.py:828-838).  tests/test_stats_ref.py checks these against the f64 oracle and the reference's recorded values;
tests/test_stats_scale_gpu.py then judges the HIP reductions with them."""
import numpy as np


def _means(total, rows, episode_length_s):
    """mean over the finished episodes `rows` of every term's sum, / max_episode_length_s (legged_robot.py:422-424)"""
    return total[:, rows].sum(axis=1) / rows.sum() / float(episode_length_s)


def episode_stats(sums_before, reward_terms, reset, terrain_levels_after, episode_length_s, prev):
    """The GRX_NUM_REWARD_TERMS + 2 statistics row of a step.  sums_before, reward_terms: (T, N), the episode sums going into the step and
    the step's scaled terms; reset: (N,) bool; terrain_levels_after: (N,), after the step's curriculum moves; prev: the row before.
    Per term the mean over the reset envs of sums_before + reward_terms, / episode_length_s; [T] the number of finished episodes;
    [T + 1] the mean terrain level over ALL envs.  Nobody reset: reset_idx returns early and the previous dict stays (every entry of it)."""
    reset = np.asarray(reset).astype(bool)
    if not reset.any():
        return np.array(prev, dtype=np.float64)
    total = np.asarray(sums_before, dtype=np.float64) + np.asarray(reward_terms, dtype=np.float64)
    return np.concatenate([_means(total, reset, episode_length_s), [float(reset.sum())],
                           [np.asarray(terrain_levels_after, dtype=np.float64).mean()]])


def base_episode_stats(sums_before, reward_terms, reset, episode_length_s, prev):
    """The same over the GRX_NUM_BASE_REWARD_TERMS rows of legged_gym's base terms (GRX_T_BASE_EPISODE_STATS: the means alone)."""
    reset = np.asarray(reset).astype(bool)
    if not reset.any():
        return np.array(prev, dtype=np.float64)
    return _means(np.asarray(sums_before, dtype=np.float64) + np.asarray(reward_terms, dtype=np.float64), reset, episode_length_s)


def reset_rows(env_ids, num_envs):
    """(N,) bool: the envs a reset_idx(env_ids) outside a step resets -- duplicates once, ids outside [0, N) not at all."""
    ids = np.asarray(env_ids, dtype=np.int64).reshape(-1)
    rows = np.zeros(num_envs, bool)
    rows[ids[(ids >= 0) & (ids < num_envs)]] = True
    return rows


def reset_stats(sums, env_ids, terrain_levels_after, episode_length_s, prev):
    """reset_idx(env_ids) outside a step: no reward is added, the means run over the DISTINCT listed envs.  sums: (T, N) before the reset.
    terrain_levels_after None: the base terms' row (means alone)."""
    sums = np.asarray(sums, dtype=np.float64)
    rows = reset_rows(env_ids, sums.shape[1])
    zero = np.zeros_like(sums)
    if terrain_levels_after is None:
        return base_episode_stats(sums, zero, rows, episode_length_s, prev)
    return episode_stats(sums, zero, rows, terrain_levels_after, episode_length_s, prev)


def command_curriculum(tracking_sums, reset, lin_vel_x, scale_dt, max_episode_length, max_curriculum):
    """update_command_curriculum (legged_robot.py:828-838) for the envs `reset` of a step: tracking_sums (N,) are their tracking_lin_vel
    episode sums with the step's own term in them; scale_dt the term's scale x dt (reward_scales holds that product).  The mean per step
    above 0.8 x scale x dt widens lin_vel_x by 0.5 either way, clipped to [-max_curriculum, 0] and [0, max_curriculum].
    Returns (lo, hi); the range stays when nobody reset."""
    reset = np.asarray(reset).astype(bool)
    lo, hi = float(lin_vel_x[0]), float(lin_vel_x[1])
    if not reset.any():
        return lo, hi
    mean = np.asarray(tracking_sums, dtype=np.float64)[reset].mean()
    if mean / float(max_episode_length) > 0.8 * float(scale_dt):
        lo = float(np.clip(lo - 0.5, -float(max_curriculum), 0.0))
        hi = float(np.clip(hi + 0.5, 0.0, float(max_curriculum)))
    return lo, hi
