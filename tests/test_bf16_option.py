"""PPO(precision=...) without a GPU: option validation, how the choice reaches PPO (the --precision flag, an assignment on a train
cfg instance, OnPolicyRunner), that the config classes keep no such key, and the C ABI of the bf16 entries (ctypes, no launch)."""
import ctypes as C
import os

import pytest
import torch

from wiki_grx_gym_amd.envs import config
from wiki_grx_gym_amd.envs.config import class_to_dict
from wiki_grx_gym_amd.rl import fused_loss as fl
from wiki_grx_gym_amd.rl.modules import MLP, ActorCriticMLP
from wiki_grx_gym_amd.rl.ppo import PPO
from wiki_grx_gym_amd.rl.runner import OnPolicyRunner
from wiki_grx_gym_amd.utils.helpers import get_args, update_cfg_from_args


def _ac(activation="elu"):
    return ActorCriticMLP(39, 168, 10, actor_hidden_dims=[64, 32], critic_hidden_dims=[64, 32], activation=activation)


def test_default_precision_is_fp32():
    alg = PPO(_ac(), device="cpu")
    assert alg.precision == "fp32"
    assert alg.actor_critic.actor.precision == "fp32" and alg.actor_critic.critic.precision == "fp32"
    assert PPO(_ac(), device="cpu", precision="fp32").precision == "fp32"


@pytest.mark.parametrize("bad", ["fp16", "BF16", "tf32", "", None, 16])
def test_unknown_precision_raises(bad):
    with pytest.raises(ValueError):
        PPO(_ac(), device="cpu", precision=bad)


def test_bf16_needs_a_hip_device():
    with pytest.raises(ValueError, match="HIP"):
        PPO(_ac(), device="cpu", precision="bf16")


def test_bf16_mlp_has_no_cpu_path_and_needs_elu():
    m = MLP(39, 10, [64, 32], "elu")
    m.set_precision("bf16")
    with pytest.raises(RuntimeError, match="HIP"):
        m(torch.zeros(4, 39))
    m.set_precision("fp32")
    assert m(torch.zeros(4, 39)).shape == (4, 10)
    with pytest.raises(ValueError):
        MLP(39, 10, [64, 32], "relu").set_precision("bf16")
    with pytest.raises(ValueError):
        m.set_precision("fp16")


def test_scripted_export_of_a_bf16_mlp_runs_in_fp32():
    m = MLP(39, 10, [64, 32], "elu")
    x = torch.randn(3, 39)
    want = m(x)
    m.set_precision("bf16")
    assert torch.equal(torch.jit.script(m)(x), want)


def test_cli_flag():
    assert get_args([]).precision is None
    assert get_args(["--precision", "bf16"]).precision == "bf16"
    assert get_args(["--precision", "fp32"]).precision == "fp32"
    with pytest.raises(SystemExit):
        get_args(["--precision", "fp16"])


@pytest.mark.parametrize("cls", [config.GR1T1CfgPPO, config.GR1T2CfgPPO])
def test_train_cfg_has_no_precision_key_unless_set(cls):
    cfg = cls()
    _, cfg = update_cfg_from_args(None, cfg, get_args([]))
    assert "precision" not in class_to_dict(cfg)["algorithm"]
    _, cfg = update_cfg_from_args(None, cfg, get_args(["--precision", "bf16"]))
    assert class_to_dict(cfg)["algorithm"]["precision"] == "bf16"
    assert "precision" not in class_to_dict(cls())["algorithm"]   # (set on the instance's section, not on the class)


class _Env:
    num_envs, num_obs, num_pri_obs, num_actions = 8, 39, 168, 10

    def reset(self):
        pass


def _runner(cfg):
    d = class_to_dict(cfg)
    d["policy"].update(actor_hidden_dims=[64, 32], critic_hidden_dims=[64, 32])
    return OnPolicyRunner(_Env(), d, None, device="cpu")


def test_precision_reaches_ppo_through_the_runner():
    """class_to_dict carries an assigned cfg.algorithm.precision into OnPolicyRunner's PPO(**algorithm_cfg)"""
    cfg = config.GR1T1CfgPPO()
    assert _runner(cfg).alg.precision == "fp32"
    cfg.algorithm.precision = "fp32"
    assert _runner(cfg).alg.precision == "fp32"
    cfg.algorithm.precision = "bf16"   # reaches PPO, which refuses bf16 on the CPU
    with pytest.raises(ValueError, match="HIP"):
        _runner(cfg)
    _, cfg2 = update_cfg_from_args(None, config.GR1T1CfgPPO(), get_args(["--precision", "bf16"]))
    with pytest.raises(ValueError, match="HIP"):
        _runner(cfg2)


def test_libgrx_ppo_exports_the_bf16_entries():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "wiki-grx-gym_amd", "csrc", "libgrx_ppo.so")
    lib = C.CDLL(path)
    for name in ("grx_mlp_layer_bf16", "grx_mlp_input_grad_bf16", "grx_mlp_weight_grad_bf16", "grx_mlp_weight_grad_bf16_partials_size"):
        assert hasattr(lib, name), name
    f = lib.grx_mlp_weight_grad_bf16_partials_size
    f.restype, f.argtypes = C.c_int, [C.c_int] * 3
    assert f(0, 8, 8) == 0 and f(8, 0, 8) == 0 and f(8, 8, 0) == 0
    assert f(1, 1, 1) == 1
    n = f(10485, 512, 39)
    assert n > 0 and n % (512 * 39) == 0
    assert fl.load_ppo_library().grx_mlp_weight_grad_bf16_partials_size(10485, 512, 39) == n
