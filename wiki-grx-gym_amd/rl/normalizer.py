"""Empirical observation normalisation (rsl_rl 2.x `empirical_normalization`): the running mean and variance of
every observation column over everything seen, and y = (x - mean) / (std + eps).

    update(x), x [n, D]:  count += n;  rate = n / count
                          mean_x = mean(x, 0);  var_x = var(x, 0, unbiased=False);  delta = mean_x - _mean
                          _mean += rate * delta
                          _var  += rate * (var_x - _var + delta * (mean_x - _mean))      # the _mean just updated
                          _std   = sqrt(_var)
    forward(x):           training mode: update(x) first; then (x - _mean) / (_std + eps).  Eval mode leaves the state alone.

which is the exact pooled population mean and variance.  `count` is an int64: a float32 count stops being exact after 2^24 samples.

Contiguous fp32 CUDA tensors go through libgrx_ppo.so (include/grx_ppo.h grx_obs_norm_*: moments, merge, apply -- three launches,
deterministic); everything else (CPU, other dtypes, strided input) through the torch spelling of the same formulas below.

With more than one rank a step's batch is the union of the ranks' batches: every rank forms (n, mean, M2) of its shard, ONE
all_gather collects them -- `normalize_step` packs the triples of all its normalisers into one buffer --, and every rank merges the
`world` triples in rank order (Chan et al.) before the update above, so every rank holds bit-identical statistics."""
import ctypes as C

import torch
import torch.distributed as dist
from torch import nn


def _world():
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def _chan_merge(triples):
    """[(n, mean, M2), ...] merged in list order; n: 0-dim tensors"""
    n, m, M2 = triples[0]
    for nb, mb, Mb in triples[1:]:
        nab = n + nb
        d = mb - m
        m = m + d * (nb / nab)
        M2 = M2 + Mb + d * d * (n * nb / nab)
        n = nab
    return n, m, M2


class EmpiricalNormalization(nn.Module):
    def __init__(self, shape, eps=1e-2):
        super().__init__()
        D = int(shape[-1]) if isinstance(shape, (tuple, list, torch.Size)) else int(shape)
        self.dim, self.eps = D, float(eps)
        self.register_buffer("_mean", torch.zeros(1, D))
        self.register_buffer("_var", torch.ones(1, D))
        self.register_buffer("_std", torch.ones(1, D))
        self.register_buffer("count", torch.tensor(0, dtype=torch.long))
        # HIP path: the slab partials of the last shape, and the two output buffers training-mode forward() alternates between -- the
        # runner stores step t's observations (PPO.process_env_step) after step t+1's have been normalised, as the env's _obs_ring
        self._partials, self._partials_key, self._ring, self._slot = None, None, None, 0

    @property
    def mean(self):
        return self._mean.squeeze(0).clone()

    @property
    def std(self):
        return self._std.squeeze(0).clone()

    # ---- which path -------------------------------------------------------------------------------------------------------------
    def _hip(self, x):
        return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] == self.dim and x.is_contiguous()
                and self._mean.device == x.device and self._mean.is_contiguous() and self._var.is_contiguous() and self._std.is_contiguous())

    def _lib(self):
        from .fused_loss import load_ppo_library
        return load_ppo_library()   # (raises when the library is missing: no silent torch fallback for CUDA tensors)

    @staticmethod
    def _stream(x):
        return C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)

    # ---- torch spelling ------------------------------------------------------------------------------------------------------------
    def _update_from_moments(self, n, mean_x, var_x):
        """the running update; n: a Python int or a 0-dim integer tensor"""
        self.count.add_(n)
        rate = (n / self.count.double()).to(self._mean.dtype)
        delta = mean_x - self._mean
        self._mean.add_(rate * delta)
        self._var.add_(rate * (var_x - self._var + delta * (mean_x - self._mean)))
        self._std.copy_(torch.sqrt(self._var))

    def _check(self, x):
        if x.dim() != 2 or x.shape[1] != self.dim or x.shape[0] < 1:
            raise ValueError(f"EmpiricalNormalization({self.dim}): expected [n >= 1, {self.dim}], got {tuple(x.shape)}")

    def _local_triple(self, x, out=None):
        """(n, mean, M2) of this rank's batch as one flat [3 * D] fp32 tensor (n repeated per column)"""
        if self._hip(x):
            lib, rows = self._lib(), x.shape[0]
            out = out if out is not None else torch.empty(3 * self.dim, device=x.device, dtype=torch.float32)
            part = self._moments_hip(x)
            with torch.cuda.device(x.device):
                rc = lib.grx_obs_norm_combine(part.numel() // (3 * self.dim), self.dim, part.data_ptr(), out.data_ptr(), self._stream(x))
            if rc:
                raise RuntimeError(f"grx_obs_norm_combine failed ({rc}): {rows} x {self.dim}")
            return out
        xf = x.to(self._mean.dtype)
        m = xf.mean(0)
        t = torch.cat([torch.full_like(m, float(x.shape[0])), m, ((xf - m) ** 2).sum(0)])
        if out is not None:
            out.copy_(t)
            return out
        return t

    def _merge_triples(self, gathered, offset=0):
        """gathered [world, width]: this normaliser's triples start at column `offset` of every rank's row"""
        D = self.dim
        if gathered.is_cuda and gathered.dtype == torch.float32 and gathered.is_contiguous() and self._mean.device == gathered.device:
            with torch.cuda.device(gathered.device):
                rc = self._lib().grx_obs_norm_merge(gathered.shape[0], D, gathered.shape[1], gathered.data_ptr() + 4 * offset, self.count.data_ptr(),
                                                    self._mean.data_ptr(), self._var.data_ptr(), self._std.data_ptr(), self._stream(gathered))
            if rc:
                raise RuntimeError(f"grx_obs_norm_merge failed ({rc})")
            return
        rows = gathered[:, offset:offset + 3 * D].reshape(gathered.shape[0], 3, D)
        n, m, M2 = _chan_merge([(r[0, 0], r[1], r[2]) for r in rows])
        self._update_from_moments(n.round().long(), m.unsqueeze(0), (M2 / n).unsqueeze(0))

    # ---- HIP path ------------------------------------------------------------------------------------------------------------------
    def _partials_for(self, x):
        if self._partials is None or self._partials_key != (x.shape[0], x.device):
            size = self._lib().grx_obs_norm_partials_size(x.shape[0], self.dim)
            if size < 1:
                raise RuntimeError(f"grx_obs_norm_partials_size: invalid shape {x.shape[0]} x {self.dim}")
            with torch.inference_mode(False):
                self._partials = torch.empty(size, device=x.device, dtype=torch.float32)
            self._partials_key = (x.shape[0], x.device)
        return self._partials

    def _ring_slot(self, x):
        if self._ring is None or self._ring[0].shape != x.shape or self._ring[0].device != x.device:
            with torch.inference_mode(False):
                self._ring = (torch.empty_like(x), torch.empty_like(x))
        y = self._ring[self._slot]
        self._slot ^= 1
        return y

    def _step_hip(self, x):
        """update(x) and the normalised x (into the ring) through ONE call: grx_obs_norm_step's three launches"""
        part, y = self._partials_for(x), self._ring_slot(x)
        with torch.cuda.device(x.device):
            rc = self._lib().grx_obs_norm_step(x.shape[0], self.dim, x.data_ptr(), part.data_ptr(), self.count.data_ptr(), self._mean.data_ptr(),
                                               self._var.data_ptr(), self._std.data_ptr(), self.eps, y.data_ptr(), self._stream(x))
        if rc:
            raise RuntimeError(f"grx_obs_norm_step failed ({rc}): {tuple(x.shape)}")
        return y

    def _moments_hip(self, x):
        lib, (rows, D) = self._lib(), x.shape
        self._partials_for(x)
        with torch.cuda.device(x.device):
            rc = lib.grx_obs_norm_moments(rows, D, x.data_ptr(), self._partials.data_ptr(), self._stream(x))
        if rc:
            raise RuntimeError(f"grx_obs_norm_moments failed ({rc}): {rows} x {D}")
        return self._partials

    def _apply_hip(self, x, ring):
        y = self._ring_slot(x) if ring else torch.empty_like(x)
        with torch.cuda.device(x.device):
            rc = self._lib().grx_obs_norm_apply(x.shape[0], self.dim, x.data_ptr(), self._mean.data_ptr(), self._std.data_ptr(), self.eps, y.data_ptr(),
                                                self._stream(x))
        if rc:
            raise RuntimeError(f"grx_obs_norm_apply failed ({rc}): {tuple(x.shape)}")
        return y

    # ---- the surface ---------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def update(self, x):
        self._check(x)
        if _world() > 1:
            return _update_all_ranks([self], [x])
        if self._hip(x):
            part = self._moments_hip(x)
            return self._merge_triples(part.view(-1, 3 * self.dim))
        xf = x.to(self._mean.dtype)
        self._update_from_moments(x.shape[0], xf.mean(0, keepdim=True), xf.var(0, unbiased=False, keepdim=True))

    @torch.no_grad()
    def normalize(self, x, ring=False):
        """(x - mean) / (std + eps) with the statistics as they are (what eval-mode forward() returns)"""
        self._check(x)
        if self._hip(x):
            return self._apply_hip(x, ring)
        return (x - self._mean) / (self._std + self.eps)

    def forward(self, x):
        if self.training:
            return normalize_step([self], [x])[0]
        return self.normalize(x)


def _update_all_ranks(norms, xs):
    """update() of several normalisers over the union of the ranks' batches with ONE all_gather, issued on the current stream (no host
    synchronisation): every rank's packed row is [triple of norms[0] | triple of norms[1] | ...]"""
    world = dist.get_world_size()
    width = sum(3 * n.dim for n in norms)
    send = torch.empty(width, device=xs[0].device, dtype=torch.float32)
    o = 0
    for n, x in zip(norms, xs):
        n._local_triple(x, out=send[o:o + 3 * n.dim])
        o += 3 * n.dim
    gathered = torch.empty(world, width, device=send.device, dtype=torch.float32)
    dist.all_gather(list(gathered.unbind(0)), send)
    o = 0
    for n in norms:
        n._merge_triples(gathered, o)
        o += 3 * n.dim


@torch.no_grad()
def normalize_step(norms, xs):
    """Training-mode forward of several normalisers on one env step's tensors (the runner's actor and critic observations): the
    statistics take the step in, the tensors come back normalised; with more than one rank, one collective for all of them."""
    for n, x in zip(norms, xs):
        n._check(x)
    if _world() > 1:
        _update_all_ranks(norms, xs)
    else:
        return [n._step_hip(x) if n._hip(x) else (n.update(x), n.normalize(x))[1] for n, x in zip(norms, xs)]
    return [n.normalize(x, ring=True) for n, x in zip(norms, xs)]


class NormalizedPolicy(nn.Module):
    """actor((x - mean) / (std + eps)) with frozen statistics: what export_policy_as_jit scripts when it is given a normaliser"""

    def __init__(self, actor, normalizer):
        super().__init__()
        self.actor = actor
        self.register_buffer("mean", normalizer._mean.detach().clone())
        self.register_buffer("scale", (normalizer._std + normalizer.eps).detach().clone())

    def forward(self, x):
        return self.actor((x - self.mean) / self.scale)
