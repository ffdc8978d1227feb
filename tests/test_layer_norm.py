"""LayerNorm hidden layers (rl/modules.py MLP(layer_norm=True), include/grx_ppo_ln.h) on the CPU: the module's structure and
state-dict keys, the flag, the torch spelling of _TrainLinearLNELU against float64 autograd, a training run over the oracle-backed env with
checkpoint, load, refusals by name and the exported TorchScript module, every refusal, the default path, and the C entry points' argument
checks.

The bound of the gradient comparison is 1e-4 max |want| per tensor, the bound tests/test_grad_penalty.py and tests/test_smooth.py use for the
same kind of comparison (fp32 formulas against float64 autograd)."""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn as nn

from tests.test_env_plumbing import oracle_backend  # noqa: F401  (the fixture)
from tests.test_smooth import _NoEnv, _make, _train_cfg
from wiki_grx_gym_amd.envs import config
from wiki_grx_gym_amd.envs.config import class_to_dict
from wiki_grx_gym_amd.rl import fused_loss, modules
from wiki_grx_gym_amd.rl.modules import MLP, ActorCriticMLP, _TrainLinearLNELU
from wiki_grx_gym_amd.rl.ppo import PPO
from wiki_grx_gym_amd.rl.runner import OnPolicyRunner
from wiki_grx_gym_amd.utils import export_policy_as_jit, get_args
from wiki_grx_gym_amd.utils.helpers import update_cfg_from_args

TOL = 1e-4
DEFAULT_KEYS = {"model_state_dict", "optimizer_state_dict", "iter", "infos"}


def test_structure_and_state_dict_keys():
    m = MLP(24, 10, [130, 64], "elu", layer_norm=True, layer_norm_eps=1e-4)
    kinds = [type(x) for x in m.model]
    assert kinds == [nn.Linear, nn.LayerNorm, nn.ELU, nn.Linear, nn.LayerNorm, nn.ELU, nn.Linear]          # the output layer stays bare
    assert [x.normalized_shape for x in m.model if isinstance(x, nn.LayerNorm)] == [(130,), (64,)]
    assert all(x.eps == 1e-4 and x.elementwise_affine for x in m.model if isinstance(x, nn.LayerNorm))
    assert MLP(24, 10, [8], "elu", layer_norm=True).model[1].eps == 1e-5
    keys = [f"model.{i}.{p}" for i in (0, 1, 3, 4, 6) for p in ("weight", "bias")]
    assert list(m.state_dict()) == keys
    plain = nn.Sequential(nn.Linear(24, 130), nn.LayerNorm(130, eps=1e-4), nn.ELU(), nn.Linear(130, 64), nn.LayerNorm(64, eps=1e-4), nn.ELU(),
                          nn.Linear(64, 10))
    plain.load_state_dict({k[len("model."):]: v for k, v in m.state_dict().items()})                     # a plain torch Sequential of the layout
    x = torch.randn(5, 24)
    assert torch.equal(plain(x), m(x))
    # off: the module, its keys and the random numbers its construction draws are what they were
    torch.manual_seed(11); a = MLP(24, 10, [130, 64], "elu"); after_a = torch.rand(1)
    torch.manual_seed(11); b = MLP(24, 10, [130, 64], "elu", layer_norm=False); after_b = torch.rand(1)
    assert torch.equal(after_a, after_b)
    assert list(a.state_dict()) == list(b.state_dict()) and all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))
    assert [type(x) for x in b.model] == [nn.Linear, nn.ELU, nn.Linear, nn.ELU, nn.Linear] and not b.layer_norm
    for act in ("relu", "tanh", "selu"):
        with pytest.raises(ValueError, match="elu"):
            MLP(24, 10, [8], act, layer_norm=True)
    with pytest.raises(ValueError, match="1024"):
        MLP(24, 10, [2048], "elu", layer_norm=True)
    ac = ActorCriticMLP(39, 168, 10, actor_hidden_dims=[32, 16], critic_hidden_dims=[16], activation="elu", layer_norm=True)
    assert ac.layer_norm and ac.actor.layer_norm and ac.critic.layer_norm
    assert isinstance(ac.actor.model[1], nn.LayerNorm) and isinstance(ac.critic.model[1], nn.LayerNorm)
    torch.manual_seed(5); p0 = ActorCriticMLP(39, 168, 10, actor_hidden_dims=[32, 16], critic_hidden_dims=[16], activation="elu")
    torch.manual_seed(5); p1 = ActorCriticMLP(39, 168, 10, actor_hidden_dims=[32, 16], critic_hidden_dims=[16], activation="elu", layer_norm=False)
    assert list(p0.state_dict()) == list(p1.state_dict()) and all(torch.equal(u, v) for u, v in zip(p0.parameters(), p1.parameters()))
    # _linears_of keeps refusing it (bf16, the gradient penalty, the estimator's fused forward); _layers_of describes it
    assert fused_loss._linears_of(m) is None and len(fused_loss._linears_of(a)) == 3
    lay = fused_loss._layers_of(m)
    assert [n is not None for _, _, n in lay] == [True, True, False] and lay[0][0] is m.model[0].weight and lay[0][2] is m.model[1]
    assert [n for _, _, n in fused_loss._layers_of(a)] == [None, None, None]
    assert fused_loss._layers_of(MLP(24, 10, [8], "tanh")) is None
    with pytest.raises(ValueError, match="bf16"):
        m.set_precision("bf16")


def test_flag_reaches_the_config_and_is_no_config_key():
    assert get_args([]).layer_norm is False and get_args(["--layer_norm"]).layer_norm is True
    plain = class_to_dict(update_cfg_from_args(None, config.GR1T1CfgPPO(), get_args([]))[1])
    assert "layer_norm" not in plain["policy"]
    assert plain == class_to_dict(config.GR1T1CfgPPO())                                                  # the default config dict is unchanged
    tcfg = update_cfg_from_args(None, config.GR1T1CfgPPO(), get_args(["--layer_norm"]))[1]
    assert tcfg.policy.layer_norm is True
    d = class_to_dict(tcfg)
    del d["policy"]["layer_norm"]
    assert d == plain                                                                                    # the one key, nothing else
    for cls in (config.GR1T1CfgPPO, config.GR1T2CfgPPO, config.GR1T1FullBodyCfgPPO):                      # not a config key
        assert not [k for k in vars(cls.policy) if k.startswith("layer_norm")]


@pytest.mark.parametrize("B,K,N", [(1, 5, 1), (7, 6, 3), (65, 39, 130), (257, 24, 64)])
def test_torch_spelling_against_float64_autograd(B, K, N):
    """forward and all six gradients (x, W, b, gamma, beta -- and none for eps) of the torch spelling -- what the function runs on CPU
    tensors and, under GRX_LN_FUSED=0, on a HIP device -- against float64 autograd of nn.Linear -> nn.LayerNorm -> nn.ELU"""
    g = torch.Generator().manual_seed(100 * B + N)
    r = lambda *s: torch.randn(*s, generator=g)
    x, W, b, gamma, beta, dy = r(B, K), r(N, K) / K ** 0.5, 0.1 * r(N), 0.5 + torch.rand(N, generator=g), 0.5 * r(N), r(B, N)
    lin, ln = nn.Linear(K, N).double(), nn.LayerNorm(N, eps=1e-5).double()
    with torch.no_grad():
        lin.weight.copy_(W); lin.bias.copy_(b); ln.weight.copy_(gamma); ln.bias.copy_(beta)
    x64 = x.double().requires_grad_()
    want_y = nn.functional.elu(ln(lin(x64)))
    want = torch.autograd.grad((want_y * dy.double()).sum(), [x64, lin.weight, lin.bias, ln.weight, ln.bias])
    want_y = want_y.detach()
    leaves = [t.clone().requires_grad_() for t in (x, W, b, gamma, beta)]
    y = _TrainLinearLNELU.apply(*leaves, 1e-5)
    got = torch.autograd.grad((y * dy).sum(), leaves)
    assert len(got) == 5 and y.dtype == torch.float32
    assert float((y.detach().double() - want_y).abs().max()) <= TOL * max(1.0, float(want_y.abs().max()))
    for name, a, w in zip(("x", "W", "b", "gamma", "beta"), got, want):
        # (+ 1e-9: at N = 1 xhat is 0, so every gradient but beta's is exactly 0 and float64 autograd returns its own rounding, 1e-15)
        err, lim = float((a.double() - w).abs().max()), TOL * float(w.abs().max()) + 1e-9
        print(f"{(B, K, N)} d{name}: max err {err:.3e}, bound {lim:.3e}")
        assert err <= lim, (name, err, lim)
    # the first layer's input is data: no dX product
    leaves[0] = x.clone()
    y = _TrainLinearLNELU.apply(*leaves, 1e-5)
    got2 = torch.autograd.grad((y * dy).sum(), leaves[1:])
    assert all(torch.equal(a, b_) for a, b_ in zip(got[1:], got2))


def _policy(**kw):
    return ActorCriticMLP(39, 168, 10, actor_hidden_dims=[32, 16], critic_hidden_dims=[32, 16], activation="elu", init_noise_std=0.4, **kw)


def test_ppo_refusals(monkeypatch):
    assert PPO(_policy(layer_norm=True), device="cpu")._layer_norm and not PPO(_policy(), device="cpu")._layer_norm
    with pytest.raises(ValueError, match="--grad_penalty_coef") as info:
        PPO(_policy(layer_norm=True), device="cpu", grad_penalty_coef=0.1)
    assert "--layer_norm" in str(info.value)
    # (precision="bf16" needs a HIP device: tests/test_layer_norm_gpu.py)
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    monkeypatch.setattr(dist, "get_rank", lambda *a: 0)
    with pytest.raises(NotImplementedError, match="world size") as info:
        PPO(_policy(layer_norm=True), device="cpu")
    assert "--layer_norm" in str(info.value)


def _cfg_dict(flags=("--layer_norm",), runner=(), algorithm=(), policy=()):
    d = class_to_dict(update_cfg_from_args(None, _train_cfg(), get_args(list(flags)))[1])
    d["runner"].update(runner); d["algorithm"].update(algorithm); d["policy"].update(policy)
    return d


def test_runner_refusals(monkeypatch, tmp_path):
    r = OnPolicyRunner(_NoEnv(), _cfg_dict(), None, "cpu")                                               # the flag alone is fine
    assert r.layer_norm == {"enabled": True, "eps": 1e-5} and r.alg._layer_norm and r.alg.actor_critic.layer_norm
    assert OnPolicyRunner(_NoEnv(), _cfg_dict(flags=()), None, "cpu").layer_norm is None
    for keys in (dict(runner={"empirical_normalization": True}), dict(runner={"obs_history_length": 3, "critic_obs_history_length": 2}),
                 dict(runner={"privileged_actor": True}), dict(algorithm={"rnd": True}), dict(algorithm={"value_norm": "popart"}),
                 dict(algorithm={"smooth": "both"}), dict(policy={"noise_std_type": "log"}),
                 dict(policy={"state_dependent_std": True, "noise_std_type": "log"})):
        assert OnPolicyRunner(_NoEnv(), _cfg_dict(**keys), None, "cpu").alg._layer_norm, keys             # ... and with what it composes with
    for keys, exc, other in ((dict(runner={"policy_class_name": "ActorCriticRecurrent"}, policy={"rnn_hidden_size": 32}), ValueError, "--recurrent"),
                             (dict(algorithm={"precision": "bf16"}), ValueError, "--precision bf16"),
                             (dict(algorithm={"grad_penalty_coef": 0.002}), ValueError, "--grad_penalty_coef"),
                             (dict(runner={"distill_from": str(tmp_path / "teacher.pt")}), ValueError, "--distill_from"),
                             (dict(runner={"exact_resume": True}), NotImplementedError, "--exact_resume"),
                             (dict(policy={"activation": "tanh"}), ValueError, "elu")):
        with pytest.raises(exc, match=other) as info:
            OnPolicyRunner(_NoEnv(), _cfg_dict(**keys), None, "cpu")
        assert "--layer_norm" in str(info.value), keys                                                   # the message names both options
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    monkeypatch.setattr(dist, "get_rank", lambda *a: 0)
    with pytest.raises(NotImplementedError, match="world size") as info:
        OnPolicyRunner(_NoEnv(), _cfg_dict(), None, "cpu")
    assert "--layer_norm" in str(info.value)


def test_cpu_training_run_checkpoint_load_and_export(oracle_backend, tmp_path):  # noqa: F811
    _, runner = _make(tmp_path / "ln", ("--layer_norm",))
    alg = runner.alg
    assert alg._layer_norm and isinstance(alg.actor_critic.actor.model[1], nn.LayerNorm)
    before = [p.detach().clone() for p in alg.actor_critic.parameters()]
    runner.learn(num_learning_iterations=2)
    assert all(not torch.equal(a, b) and bool(torch.isfinite(b).all()) for a, b in zip(before, alg.actor_critic.parameters()))
    path = os.path.join(runner.log_dir, "model_2.pt")
    ck = torch.load(path, weights_only=False)
    assert set(ck) == DEFAULT_KEYS | {"layer_norm"} and ck["layer_norm"] == {"enabled": True, "eps": 1e-5}
    assert "actor.model.1.weight" in ck["model_state_dict"] and "critic.model.4.bias" in ck["model_state_dict"]
    _, again = _make(tmp_path / "again", ("--layer_norm",))
    again.load(path)                                                                                    # it loads (what --resume does)
    loaded = again.alg.actor_critic.state_dict()
    assert all(torch.equal(v, loaded[k]) for k, v in alg.actor_critic.state_dict().items() if k != "std") and again.current_learning_iteration == 2
    _, plain = _make(tmp_path / "plain", ())
    with pytest.raises(ValueError, match="--layer_norm"):                                               # ... by name, not by a state-dict key error
        plain.load(path)
    plain.learn(num_learning_iterations=1)
    plain_path = os.path.join(plain.log_dir, "model_1.pt")
    assert set(torch.load(plain_path, weights_only=False)) == DEFAULT_KEYS and plain.layer_norm is None  # no key without the flag
    with pytest.raises(ValueError, match="--layer_norm"):                                               # ... and the other way round
        again.load(plain_path)
    # the exported TorchScript module follows act_inference
    exported = export_policy_as_jit(alg.actor_critic, str(tmp_path / "exported"))
    jit = torch.jit.load(exported)
    x = torch.randn(64, 39)
    with torch.no_grad():
        want = alg.actor_critic.act_inference(x)
    assert float((jit(x) - want).abs().max()) < 1e-6                                                    # tests/test_play_gpu.py's tolerance


def test_default_path_runs_nothing_of_it(oracle_backend, tmp_path, monkeypatch):  # noqa: F811
    # (what carries weight on the CPU: no nn.LayerNorm module, no checkpoint key, no new import.  The patches guard the function and the
    #  entry points' wrappers, which a CPU run does not reach with the flag either -- MLP.forward runs the plain modules there)
    def boom(*a, **k):
        raise AssertionError("the default path reached the LayerNorm code")
    monkeypatch.setattr(_TrainLinearLNELU, "apply", boom)
    monkeypatch.setattr(modules, "ln_elu_torch", boom)
    monkeypatch.setattr(fused_loss, "ln_elu_forward", boom)
    monkeypatch.setattr(fused_loss, "ln_elu_backward", boom)
    before = {m for m in sys.modules if m.startswith("wiki_grx_gym_amd.rl")}
    _, runner = _make(tmp_path, ())
    runner.learn(num_learning_iterations=1)
    assert {m for m in sys.modules if m.startswith("wiki_grx_gym_amd.rl")} == before                     # rl imports nothing new
    assert not [m for m in before if "layer_norm" in m or m.endswith(".ln")]                            # (there is no module of its own)
    assert set(torch.load(os.path.join(runner.log_dir, "model_1.pt"), weights_only=False)) == DEFAULT_KEYS
    assert not [type(m) for m in runner.alg.actor_critic.modules() if isinstance(m, nn.LayerNorm)]


# ---- the C entry points, without a GPU --------------------------------------------------------------------------------------------------
def test_entry_points_are_exported_and_refuse_bad_arguments():
    lib = fused_loss.load_ppo_library()
    names = ("grx_ln_elu_forward", "grx_ln_elu_backward", "grx_ln_elu_backward_partials_size")
    for name in names:
        assert hasattr(lib, name), name
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "grx_ppo_ln.h")).read()
    assert all(f"int {n}(" in hdr for n in names) and '#include "grx_ppo_ln.h"' in open(os.path.join(root, "include", "grx_ppo.h")).read()
    assert lib.grx_ln_elu_backward_partials_size(513, 130) == 3 * 3 * 130 and lib.grx_ln_elu_backward_partials_size(1, 1) == 3
    assert lib.grx_ln_elu_backward_partials_size(256, 1024) == 3 * 1024
    for rows, cols in ((0, 4), (4, 0), (-1, 4), (4, 1025), (1 << 21, 1024)):
        assert lib.grx_ln_elu_backward_partials_size(rows, cols) == 0
    p = C.c_void_p(0x1000)    # (never dereferenced: every call below is refused before a launch)
    for rows, cols in ((0, 4), (-1, 4), (4, 0), (4, -1), (4, 1025), (1 << 21, 1024)):                     # rows < 1, cols < 1, cols > 1024, 2^31 elements
        assert lib.grx_ln_elu_forward(rows, cols, p, p, p, 1e-5, p, p, p, None) < 0
        assert lib.grx_ln_elu_forward(rows, cols, p, p, p, 1e-5, p, None, None, None) < 0
        assert lib.grx_ln_elu_backward(rows, cols, *([p] * 11), None) < 0
    for k in range(4):                                                                                   # a null pointer: z, gamma, beta, y
        args = [p, p, p, 1e-5, p, p, p]
        args[k if k < 3 else 4] = None
        assert lib.grx_ln_elu_forward(4, 4, *args, None) < 0
    assert lib.grx_ln_elu_forward(4, 4, p, p, p, 1e-5, p, p, None, None) < 0                              # one of mean / rstd alone
    assert lib.grx_ln_elu_forward(4, 4, p, p, p, 1e-5, p, None, p, None) < 0
    for k in range(11):
        args = [p] * 11; args[k] = None
        assert lib.grx_ln_elu_backward(4, 4, *args, None) < 0
    assert lib.grx_ln_elu_backward(65536 * 256, 1, *([p] * 11), None) < 0                                 # more slabs than a grid has rows
