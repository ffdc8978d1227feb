"""PPO(precision="bf16"): libgrx_ppo.so's bf16 products (grx_mlp_layer_bf16, grx_mlp_input_grad_bf16, grx_mlp_weight_grad_bf16)
against float64 references, and the training path built on them.

The references round the operands to bf16 exactly as the kernels do (fp32 -> bf16, round to nearest even: torch's conversion) and
multiply the rounded values in float64.  What remains is the kernels' fp32 accumulation: a sum of n products good to
n * U32 * sum |a * b| (U32 = 2^-24), plus a few roundings of the epilogue (bias, ELU)."""
import copy
import ctypes as C
import math

import pytest
import torch

from tests import ppo_ref
from tests.ppo_ref import U32
from wiki_grx_gym_amd.rl import fused_loss as fl
from wiki_grx_gym_amd.rl.modules import ActorCriticMLP
from wiki_grx_gym_amd.rl.ppo import PPO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def rb(t):
    """the kernels' operand rounding in float64: fp32 -> bf16 (round to nearest even, NaN kept) -> float64"""
    return t.float().to(torch.bfloat16).double()


def _check(got, ref, mag, n, tag, extra=0.0):
    """|got - ref| <= (n + 2) * U32 * mag + extra (+ 4 U32 |ref| for the epilogue's roundings), elementwise"""
    err = (got.double() - ref).abs()
    tol = (n + 2) * U32 * mag + 4 * U32 * ref.abs() + extra + 1e-30
    assert bool(torch.isfinite(got).all()), tag
    assert bool((err <= tol).all()), (tag, float((err / tol).max()))


def _layer_bf16(X, W, b, elu):
    Y = torch.full((X.shape[0], W.shape[0]), float("nan"), device=DEV)
    rc = fl.load_ppo_library().grx_mlp_layer_bf16(X.shape[0], X.shape[1], W.shape[0], X.data_ptr(), W.data_ptr(),
                                                    b.data_ptr() if b is not None else None, Y.data_ptr(), int(elu), _stream())
    assert rc == 0
    return Y


# the GR1T1 (39 / 168 observations) and full-body (105 / 234) training shapes, rollout (4096) and minibatch (10485, 24576) rows, and
# the edges of the 128 x 64 x 64 blocking
LAYER_SHAPES = [(4096, 39, 512), (4096, 512, 256), (4096, 256, 128), (10485, 168, 512), (10485, 105, 512), (10485, 234, 512),
                (24576, 512, 256), (10485, 256, 128), (1, 39, 512), (1, 1, 1), (129, 39, 65), (127, 70, 130), (200, 65, 63), (3, 4, 1)]


@pytest.mark.parametrize("M,K,N", LAYER_SHAPES)
def test_layer_bf16_matches_float64(M, K, N):
    """Y = ELU(bf16(X) bf16(W)^T + b) and, without ELU and bias, bf16(X) bf16(W)^T, against float64 on the rounded operands.  A row's
    result does not depend on the batch: the first rows computed alone equal their values in the full batch bit for bit."""
    g = _gen(M * 7 + K * 3 + N)
    X = torch.randn(M, K, device=DEV, generator=g)
    W = torch.randn(N, K, device=DEV, generator=g) / math.sqrt(K)
    b = 0.1 * torch.randn(N, device=DEV, generator=g)
    z = rb(X) @ rb(W).t()
    mag = rb(X).abs() @ rb(W).abs().t()
    Y = _layer_bf16(X, W, b, True)
    _check(Y, torch.nn.functional.elu(z + b.double()), mag + b.double().abs(), K, ("elu", M, K, N))
    Y0 = _layer_bf16(X, W, None, False)
    _check(Y0, z, mag, K, ("plain", M, K, N))
    r = min(M, 5)
    assert torch.equal(_layer_bf16(X[:r].clone(), W, b, True), Y[:r])


# (M, N, K): dX [M][K] = dZ [M][N] . W [N][K] for the hidden layers after the first, and edges
INPUT_SHAPES = [(10485, 256, 512), (10485, 128, 256), (24576, 256, 512), (4096, 128, 256), (1, 1, 1), (1, 128, 512), (129, 65, 70),
                (300, 130, 39), (257, 3, 5)]


@pytest.mark.parametrize("M,N,K", INPUT_SHAPES)
def test_input_grad_bf16_matches_float64(M, N, K):
    g = _gen(M * 5 + N * 3 + K)
    dZ = 0.01 * torch.randn(M, N, device=DEV, generator=g)
    W = torch.randn(N, K, device=DEV, generator=g) / math.sqrt(K)
    dX = torch.full((M, K), float("nan"), device=DEV)
    assert fl.load_ppo_library().grx_mlp_input_grad_bf16(M, N, K, dZ.data_ptr(), W.data_ptr(), dX.data_ptr(), _stream()) == 0
    _check(dX, rb(dZ) @ rb(W), rb(dZ).abs() @ rb(W).abs(), N, ("dX", M, N, K))
    assert torch.equal(fl.input_grad_bf16(dZ, W), dX)


# (M, N, K): dW [N][K] = dZ^T . X summed over M batch rows, every hidden layer of both networks at the minibatch sizes, and edges
WEIGHT_SHAPES = [(10485, 512, 39), (10485, 512, 168), (10485, 256, 512), (10485, 128, 256), (24576, 512, 105), (49152, 512, 234),
                 (4096, 256, 512), (1, 1, 1), (1, 512, 39), (255, 130, 70), (300, 65, 39), (1000, 7, 3)]


@pytest.mark.parametrize("M,N,K", WEIGHT_SHAPES)
def test_weight_grad_bf16_matches_float64_and_is_deterministic(M, N, K):
    g = _gen(M * 3 + N * 5 + K)
    dZ = 0.01 * torch.randn(M, N, device=DEV, generator=g)
    X = torch.nn.functional.elu(torch.randn(M, K, device=DEV, generator=g))
    dW = fl.weight_grad_bf16(dZ, X)
    _check(dW, rb(dZ).t() @ rb(X), rb(dZ).abs().t() @ rb(X).abs(), M + 64, ("dW", M, N, K))   # (+ the slab sums)
    for _ in range(2):
        assert torch.equal(fl.weight_grad_bf16(dZ, X), dW)


def test_bf16_entries_reject_invalid_arguments_and_write_nothing():
    lib = fl.load_ppo_library()
    X, W = torch.randn(8, 8, device=DEV), torch.randn(8, 8, device=DEV)
    out = torch.full((64,), -3.0, device=DEV)
    p = torch.zeros(4096, device=DEV)
    s = _stream()
    for M, K, N in [(0, 8, 8), (8, 0, 8), (8, 8, 0), (-1, 8, 8)]:
        assert lib.grx_mlp_layer_bf16(M, K, N, X.data_ptr(), W.data_ptr(), None, out.data_ptr(), 1, s) < 0
        assert lib.grx_mlp_input_grad_bf16(M, K, N, X.data_ptr(), W.data_ptr(), out.data_ptr(), s) < 0
        assert lib.grx_mlp_weight_grad_bf16(M, K, N, X.data_ptr(), W.data_ptr(), out.data_ptr(), p.data_ptr(), s) < 0
        assert lib.grx_mlp_weight_grad_bf16_partials_size(M, K, N) == 0
    assert lib.grx_mlp_layer_bf16(8, 8, 8, None, W.data_ptr(), None, out.data_ptr(), 1, s) < 0
    assert lib.grx_mlp_layer_bf16(8, 8, 8, X.data_ptr(), W.data_ptr(), None, None, 1, s) < 0
    assert lib.grx_mlp_input_grad_bf16(8, 8, 8, X.data_ptr(), None, out.data_ptr(), s) < 0
    assert lib.grx_mlp_weight_grad_bf16(8, 8, 8, X.data_ptr(), W.data_ptr(), out.data_ptr(), None, s) < 0
    assert lib.grx_mlp_weight_grad_bf16(8, 8, 8, X.data_ptr(), None, out.data_ptr(), p.data_ptr(), s) < 0
    torch.cuda.synchronize()
    assert bool((out == -3.0).all())


def test_operands_are_rounded_to_bf16():
    """Operands with low mantissa bits set (bf16 values times 1 + 2^-10, which round back to them): the bf16 kernels match the float64
    product of the bf16 values, and the fp32 kernel on the same data is off it by far more than that tolerance (positive operands: the
    products' relative offset of ~2^-9 does not cancel)."""
    M, K, N = 512, 256, 128
    g = _gen(5)
    Xr = torch.randn(M, K, device=DEV, generator=g).abs().bfloat16().float()
    Wr = (torch.randn(N, K, device=DEV, generator=g).abs() / 16).bfloat16().float()
    X, W = Xr * (1 + 2.0 ** -10), Wr * (1 + 2.0 ** -10)
    assert torch.equal(X.bfloat16().float(), Xr) and not torch.equal(X, Xr)
    ref, mag = Xr.double() @ Wr.double().t(), Xr.double().abs() @ Wr.double().abs().t()
    Y = _layer_bf16(X, W, None, False)
    _check(Y, ref, mag, K, "forward")
    Y32 = fl._layer(fl.load_ppo_library(), X, W, None, False, torch.cuda.current_stream(DEV).cuda_stream)
    tol = (K + 2) * U32 * mag
    assert bool(((Y32.double() - ref).abs() > 20 * tol).all())
    dZ = torch.randn(M, N, device=DEV, generator=g).bfloat16().float() * (1 + 2.0 ** -10)
    _check(fl.input_grad_bf16(dZ, W), rb(dZ) @ Wr.double(), rb(dZ).abs() @ Wr.double().abs(), N, "dX")
    assert not torch.equal(fl.input_grad_bf16(dZ, W), dZ @ W)
    _check(fl.weight_grad_bf16(dZ, X), rb(dZ).t() @ Xr.double(), rb(dZ).abs().t() @ Xr.double().abs(), M + 64, "dW")


# ---- the training path: one minibatch's parameter gradients ---------------------------------------------------------------------
class _Ref64LinearELU(torch.autograd.Function):
    """a hidden layer in float64 with the kernels' bf16 operands: Y = ELU(rb(X) rb(W)^T + b), dX = rb(dZ) rb(W), dW = rb(dZ)^T rb(X),
    db = sum dZ (fp32 in the product, unrounded)"""

    @staticmethod
    def forward(ctx, x, w, b):
        y = torch.nn.functional.elu(rb(x) @ rb(w).t() + b)
        ctx.save_for_backward(x, w, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        dz = dy * torch.where(y > 0, torch.ones_like(y), y + 1.0)
        return rb(dz) @ rb(w), rb(dz).t() @ rb(x), dz.sum(0)


def _ref64(mlp64, x):
    lin = fl._linears_of(mlp64)
    for w, b in lin[:-1]:
        x = _Ref64LinearELU.apply(x, w, b)
    w, b = lin[-1]
    return x @ w.t() + b


CLIP = 0.2
E2E = {"gr1t1": dict(no=39, npri=168, A=10, mb=10485, std=0.2, gain=1.0),
       "full_body": dict(no=105, npri=234, A=32, mb=10485, std=[0.2] * 12 + [0.05] * 20, gain=0.01)}


def _e2e_setup(name):
    c = E2E[name]
    torch.manual_seed(11)
    ac = ActorCriticMLP(c["no"], c["npri"], c["A"], actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[512, 256, 128], activation="elu",
                        init_noise_std=c["std"], actor_output_gain=c["gain"])
    ac64 = copy.deepcopy(ac).double().to(DEV)
    alg = PPO(ac, clip_param=CLIP, value_loss_coef=1.0, entropy_coef=0.01, use_clipped_value_loss=True, schedule="adaptive",
              desired_kl=0.01, device=DEV, precision="bf16")
    assert alg._fused_loss and alg._two_streams and ac.actor.precision == "bf16" and ac.critic.precision == "bf16"
    mb, A = c["mb"], c["A"]
    g = _gen(mb + A)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)
    obs, cobs = r(mb, c["no"]), r(mb, c["npri"])
    with torch.no_grad():
        mu64, v64 = _ref64(ac64.actor, obs.double()), _ref64(ac64.critic, cobs.double())
        std = ac.std.detach()
        actions = (mu64 + std.double() * r(mb, A).double()).float()
        old_mu = (mu64 + 0.1 * std.double() * r(mb, A).double()).float()
        old_sigma = std * (1.0 + 0.1 * torch.rand(mb, A, device=DEV, generator=g))
        tv, ret, adv = (v64 + 0.3 * r(mb, 1).double()).float(), (v64 + r(mb, 1).double()).float(), r(mb, 1)
        logp = torch.distributions.Normal(mu64, std.double()).log_prob(actions.double()).sum(-1, keepdim=True)
        old_logp = (logp + 0.25 * r(mb, 1).double()).float()
        for _ in range(20):
            bad = ppo_ref.loss_near_ties(mu64, std, v64, actions, old_logp, ret, tv, CLIP)
            if not bool(bad.any()):
                break
            b = bad.reshape(-1, 1)
            old_logp = torch.where(b, old_logp - 0.01, old_logp)
            tv = torch.where(b, tv + 0.013, tv)
            ret = torch.where(b, ret + 0.011, ret)
        assert not bool(ppo_ref.loss_near_ties(mu64, std, v64, actions, old_logp, ret, tv, CLIP).any())
    return ac, ac64, alg, [obs, cobs, actions, tv, adv, ret, old_logp, old_mu, old_sigma]


def _e2e_check(name, ac, ac64, batch):
    """every p.grad of `ac` against the float64 copy with bf16-rounded hidden-layer operands, within 2e-3 * max |g_ref|.  The fp32 sums
    alone would stay near 1e-5 of it (test_ppo_kernels_gpu); what dominates here is the rounding itself: an operand whose fp32 value (in
    the kernels) and float64 value (in the copy) lie on two sides of a bf16 rounding boundary rounds to neighbours 2^-8 apart.  That
    happens to about (fp32 error) / (bf16 step) of the operands, in every product of the forward and the backward, and the differences
    carry on through the layers: 4e-4 (GR1T1) and 8e-4 (full body) of max |g_ref| measured on the MI355X."""
    obs, cobs, actions, tv, adv, ret, old_logp, old_mu, old_sigma = batch
    mu, value = _ref64(ac64.actor, obs.double()), _ref64(ac64.critic, cobs.double())
    ref = ppo_ref.ppo_loss_ref(mu, ac64.std, value, actions, old_logp, old_mu, old_sigma, adv, ret, tv, CLIP, 1.0, 0.01, True)
    ac64.zero_grad(set_to_none=True)
    torch.autograd.backward([mu, value, ac64.std], [ref["d_mu"], ref["d_value"], ref["d_std"]])
    for (n, p), q in zip(ac.named_parameters(), ac64.parameters()):
        tol = 2e-3 * float(q.grad.abs().max())
        err = float((p.grad.double() - q.grad).abs().max())
        assert err <= tol, (name, n, err, tol)


def _eager_grads(alg, batch):
    with alg._blas_for_update():
        alg._losses(*batch)[2].backward()
    torch.cuda.synchronize()
    grads = [p.grad.clone() for p in alg._params]
    alg.optimizer.zero_grad(set_to_none=True)
    return grads


@pytest.mark.parametrize("name", list(E2E))
def test_bf16_minibatch_gradients_match_float64_eager_and_captured(name):
    """One minibatch in bf16 mode, eagerly (twice: bit-identical) and replayed from the captured two-stream step (PPO._build_graph):
    the captured gradients equal the eager ones bit for bit, and both match the float64 copy."""
    ac, ac64, alg, batch = _e2e_setup(name)
    g1 = _eager_grads(alg, batch)
    g2 = _eager_grads(alg, batch)
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))
    for p, g in zip(alg._params, g1):
        p.grad = g.clone()
    _e2e_check(name, ac, ac64, batch)
    alg.init_storage(16, 2)   # (_build_graph takes its buffer widths from the storage)
    alg._build_graph(batch[0].shape[0])
    assert isinstance(alg._graph, torch.cuda.CUDAGraph)
    for buf, x in zip(alg._static, batch):
        buf.copy_(x)
    alg._graph.replay()
    torch.cuda.synchronize()
    for (n, p), g in zip(ac.named_parameters(), g1):
        assert torch.equal(p.grad, g), n


# ---- rollout and update -------------------------------------------------------------------------------------------------------
def _rollout(alg, N, T, no, npri, seed):
    g = _gen(seed)
    torch.manual_seed(seed)
    with torch.inference_mode():
        for _ in range(T):
            obs, cobs = torch.randn(N, no, device=DEV, generator=g), torch.randn(N, npri, device=DEV, generator=g)
            alg.act(obs, cobs)
            alg.process_env_step(torch.randn(N, device=DEV, generator=g), torch.rand(N, device=DEV, generator=g) < 0.05, {})
        alg.compute_returns(torch.randn(N, npri, device=DEV, generator=g))


def _ppo(precision=None, **kw):
    torch.manual_seed(21)
    ac = ActorCriticMLP(39, 168, 10, actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[512, 256, 128], activation="elu", init_noise_std=0.3)
    args = dict(num_learning_epochs=kw.get("epochs", 1), num_mini_batches=kw.get("mbs", 1), schedule="adaptive", desired_kl=0.01,
                entropy_coef=0.01, device=DEV)
    if precision is not None:
        args["precision"] = precision
    return PPO(ac, **args)


def _head_tol(mlp, x_in, y, K):
    """(K + 2) U32 sum |h w| + 4 U32 |y| for an output layer: the hidden part through the bf16 kernels (bit-identical in both paths)"""
    lin = fl._linears_of(mlp)
    with torch.no_grad():
        h = x_in
        for w, b in lin[:-1]:
            h = fl.linear_elu(h, w, b, bf16=True)
        w, b = lin[-1]
        return (K + 2) * U32 * (h.double().abs() @ w.double().abs().t() + b.double().abs()) + 4 * U32 * y.double().abs()


def test_bf16_rollout_and_first_minibatch_agree():
    """After a bf16 rollout (captured policy step), the update's forward of the stored observations reproduces the stored action means and
    values to fp32-accumulation tolerance of the output layers -- the hidden layers run the same bf16 kernel on the same rows -- and the
    first minibatch's KL is that of two identical policies (the 1e-5 inside rsl_rl's log(sigma / old_sigma + 1e-5)) within 1e-6."""
    N, T = 1024, 8
    alg = _ppo("bf16")
    alg.init_storage(N, T)
    _rollout(alg, N, T, 39, 168, seed=4)
    assert alg._act_fused
    st, ac = alg.storage, alg.actor_critic
    obs, cobs = st.observations.flatten(0, 1), st.pri_observations.flatten(0, 1)
    # (the training path, with autograd; detached at once: a live graph would keep the parameters' AccumulateGrad nodes, and with them
    #  the stream this forward ran on, into the update's captured step -- see PPO._build_graph)
    mu, v = ac.actor(obs).detach(), ac.critic(cobs).detach()
    for got, want, mlp, x, K in ((mu, st.mu.flatten(0, 1), ac.actor, obs, 128), (v, st.values.flatten(0, 1), ac.critic, cobs, 128)):
        err = (got.double() - want.double()).abs()
        tol = _head_tol(mlp, x, want, K)
        assert bool((err <= tol).all()), float((err / tol).max())
    alg.update()
    assert abs(alg.mean_kl - 10 * math.log1p(1e-5)) <= 1e-6, alg.mean_kl


def test_fp32_precision_is_the_default_path_bit_for_bit():
    """PPO(precision="fp32") and PPO without the argument: identical rollouts and identical parameters after one update."""
    N, T = 512, 8
    runs = []
    for precision in (None, "fp32"):
        alg = _ppo(precision, epochs=2, mbs=2)
        assert alg.precision == "fp32" and alg.actor_critic.actor.precision == "fp32"
        alg.init_storage(N, T)
        _rollout(alg, N, T, 39, 168, seed=9)
        st = alg.storage
        stored = [x.clone() for x in (st.actions, st.mu, st.values, st.actions_log_prob, st.returns)]
        losses = alg.update()
        runs.append((stored, [p.detach().clone() for p in alg.actor_critic.parameters()], losses, alg.learning_rate))
    (s0, p0, l0, lr0), (s1, p1, l1, lr1) = runs
    assert all(torch.equal(a, b) for a, b in zip(s0, s1))
    assert all(torch.equal(a, b) for a, b in zip(p0, p1))
    assert l0 == l1 and lr0 == lr1
