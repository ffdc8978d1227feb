"""numpy statement of the observation history (rl/history.py), the seeded frames and `dones` patterns of its tests.
Shared by tests/test_obs_history.py and tests/test_obs_history_gpu.py.  The operation only copies: every comparison against this
reference is exact (array_equal / torch.equal), there is no tolerance."""
import functools

import numpy as np

PATTERNS = ("none", "all", "every_other", "single")   # (the first step's fill is what RefHistory.push does while it is not primed)


class RefHistory:
    """rows [N, H * D]: H frames per env, oldest first, newest last"""

    def __init__(self, N, D, H):
        self.N, self.D, self.H = N, D, H
        self.rows = None

    def fill(self, x):
        x = np.asarray(x, dtype=np.float32)
        assert x.shape == (self.N, self.D)
        self.rows = np.tile(x, (1, self.H))
        return self.rows

    def push(self, x, dones):
        if self.rows is None:
            return self.fill(x)
        x = np.asarray(x, dtype=np.float32)
        new = np.empty_like(self.rows)
        for n in range(self.N):
            if dones[n]:
                for h in range(self.H):
                    new[n, h * self.D:(h + 1) * self.D] = x[n]
            else:
                new[n, :(self.H - 1) * self.D] = self.rows[n, self.D:]
                new[n, (self.H - 1) * self.D:] = x[n]
        self.rows = new
        return new


@functools.lru_cache(maxsize=None)
def frames(N, D, steps):
    """seeded frames [steps][N, D] float32; every value is distinct enough that a misplaced copy shows"""
    rng = np.random.default_rng(1000 * N + 10 * D + steps)
    out = np.float32(rng.standard_normal((steps, N, D)) + np.arange(steps)[:, None, None])
    out.setflags(write=False)
    return out


def dones(pattern, N, step):
    """[N] bool for push number `step` (0: the first push after the fill)"""
    d = np.zeros(N, dtype=bool)
    if pattern == "all":
        d[:] = step % 2 == 1
    elif pattern == "every_other":
        d[(step % 2)::2] = True
    elif pattern == "single":
        d[(7 * step + N // 2) % N] = True
    elif pattern != "none":
        raise ValueError(pattern)
    return d


@functools.lru_cache(maxsize=None)
def reference(N, D, H, pattern, steps):
    """the rows after the fill with frame 0 and after each of `steps` pushes of frames 1 .. steps: a tuple of steps + 1 read-only arrays"""
    ref, x = RefHistory(N, D, H), frames(N, D, steps + 1)
    out = [ref.fill(x[0]).copy()]
    for t in range(steps):
        out.append(ref.push(x[t + 1], dones(pattern, N, t)).copy())
    for a in out:
        a.setflags(write=False)
    return tuple(out)


def stack_table(table, done_steps, H):
    """The stacked rows a runner builds from a table of raw frames [T + 1][N, D]: entry 0 fills, step t >= 1 pushes table[t] with
    dones = done_steps.get(t, ()) (a collection of env indices).  Returns [T + 1][N, H * D]."""
    table = np.asarray(table, dtype=np.float32)
    N, D = table.shape[1:]
    ref = RefHistory(N, D, H)
    out = [ref.fill(table[0]).copy()]
    for t in range(1, table.shape[0]):
        d = np.zeros(N, dtype=bool)
        d[list(done_steps.get(t, ()))] = True
        out.append(ref.push(table[t], d).copy())
    return np.stack(out)
