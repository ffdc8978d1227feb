"""Exact resume without a GPU: how the option reaches the runner (the --exact_resume flag, an assignment on a train cfg instance), that
no config class gains a key, the sidecar's name and lookup next to model_<it>.pt, the refusals (missing sidecar, more than one rank) and
the C ABI of the snapshot entries (ctypes, no launch)."""
import ctypes as C
import os

import pytest
import torch

from wiki_grx_gym_amd import _capi
from wiki_grx_gym_amd.envs import config
from wiki_grx_gym_amd.envs.config import class_to_dict
from wiki_grx_gym_amd.rl import runner as runner_mod
from wiki_grx_gym_amd.rl.runner import OnPolicyRunner, train_state_path
from wiki_grx_gym_amd.utils.helpers import get_args, get_load_path, update_cfg_from_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Env:
    num_envs, num_obs, num_pri_obs, num_actions = 8, 39, 168, 10

    def reset(self):
        pass


def _runner(cfg):
    d = class_to_dict(cfg)
    d["policy"].update(actor_hidden_dims=[64, 32], critic_hidden_dims=[64, 32])
    return OnPolicyRunner(_Env(), d, None, device="cpu")


def test_cli_flag():
    assert get_args([]).exact_resume is False
    assert get_args(["--exact_resume"]).exact_resume is True
    assert get_args(["--resume", "--exact_resume", "--checkpoint", "10"]).checkpoint == 10


@pytest.mark.parametrize("cls", [config.GR1T1CfgPPO, config.GR1T2CfgPPO, config.GR1T1FullBodyCfgPPO])
def test_train_cfg_has_no_exact_resume_key_unless_set(cls):
    _, cfg = update_cfg_from_args(None, cls(), get_args([]))
    assert "exact_resume" not in class_to_dict(cfg)["runner"]
    _, cfg = update_cfg_from_args(None, cfg, get_args(["--exact_resume"]))
    assert class_to_dict(cfg)["runner"]["exact_resume"] is True
    assert "exact_resume" not in class_to_dict(cls())["runner"]


def test_option_reaches_the_runner():
    cfg = config.GR1T1CfgPPO()
    assert _runner(cfg).exact_resume is False
    cfg.runner.exact_resume = True
    assert _runner(cfg).exact_resume is True
    _, cfg2 = update_cfg_from_args(None, config.GR1T1CfgPPO(), get_args(["--exact_resume"]))
    assert _runner(cfg2).exact_resume is True


def test_sidecar_name_and_lookup(tmp_path):
    assert train_state_path(os.path.join("a", "b", "model_300.pt")) == os.path.join("a", "b", "train_state_300.pt")
    assert "model" not in os.path.basename(train_state_path("model_7.pt"))
    run = tmp_path / "Oct16_00-00-00_run"
    run.mkdir()
    for it in (0, 2, 10, 4):
        (run / f"model_{it}.pt").write_bytes(b"")
        (run / f"train_state_{it}.pt").write_bytes(b"")
    assert get_load_path(str(tmp_path)) == str(run / "model_10.pt")
    assert get_load_path(str(tmp_path), checkpoint=2) == str(run / "model_2.pt")


def test_missing_sidecar_raises(tmp_path):
    cfg = config.GR1T1CfgPPO()
    cfg.runner.exact_resume = True
    r = _runner(cfg)
    (tmp_path / "model_3.pt").write_bytes(b"")
    with pytest.raises(FileNotFoundError, match="train_state_3.pt"):
        r.load_train_state(str(tmp_path / "model_3.pt"))


def test_more_than_one_rank_raises(monkeypatch):
    monkeypatch.setattr(runner_mod.dist, "is_initialized", lambda: True)
    monkeypatch.setattr(runner_mod.dist, "get_world_size", lambda: 2)
    monkeypatch.setattr(runner_mod.dist, "get_rank", lambda: 0)
    cfg = config.GR1T1CfgPPO()
    cfg.runner.exact_resume = True
    with pytest.raises(NotImplementedError, match="one process"):
        _runner(cfg)


def test_default_save_is_unchanged(tmp_path):
    """without the option save() writes model_<it>.pt with exactly the reference's keys and nothing else"""
    r = _runner(config.GR1T1CfgPPO())
    r.save(str(tmp_path / "model_5.pt"))
    assert os.listdir(tmp_path) == ["model_5.pt"]
    ck = torch.load(tmp_path / "model_5.pt", weights_only=False)
    assert set(ck) == {"model_state_dict", "optimizer_state_dict", "iter", "infos"} and ck["iter"] == 0


def test_c_entries_are_exported_and_check_their_arguments():
    for s in ("grx_state_bytes", "grx_save_state", "grx_load_state"):
        assert s in _capi.EXPORTED_SYMBOLS
    lib = C.CDLL(os.path.join(ROOT, "wiki-grx-gym_amd", "csrc", "libgrx_hip.so"))
    api = _capi.bind(lib, "grx_")
    n = C.c_int64(0)
    buf = (C.c_uint8 * 64)()
    assert api["state_bytes"](None, C.byref(n)) == -1
    assert api["save_state"](None, C.cast(buf, C.c_void_p), 64, None) == -1
    assert api["load_state"](None, C.cast(buf, C.c_void_p), 64, None) == -1
    assert b"null" in api["last_error"]()
