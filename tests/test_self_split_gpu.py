"""Lane-quad layouts: the two halves of a leg share the leg x leg self-collision pairs of their env (grx_self.h: even / odd rank of
the overlap mask, then one add over the halves).  From the same crossed-legs state, one step of the eight- and four-wave lane-quad
kernels must give the lane-pair kernel's forces to rounding, and every leg x leg pair must stay an internal force of its env."""
import pytest
import torch

from tests.helpers import make_cfg, make_sims, random_actions
from tests.test_hip_parity import set_layout


def _crossed_legs_step(monkeypatch, layout, N=96):
    set_layout(monkeypatch, layout)
    cfg = make_cfg(task="GR1T1", dr=True, push=False)
    hip, ora = make_sims(cfg, N, seed=5)
    ora.reset_all()
    g = torch.Generator().manual_seed(7)
    root = ora.tensor("ROOT_STATES").clone()
    root[:, 2] = 3.0                                                        # in flight: the legs touch only each other
    root[:, 7:13] = torch.randn(N, 6, generator=g) * 0.3
    q = torch.tensor([[-0.45, 0.0, -0.3, 0.6, -0.3, 0.45, 0.0, -0.3, 0.6, -0.3]]).repeat(N, 1)      # hips adducted past each other
    q += (torch.rand(N, 10, generator=g) - 0.5) * torch.tensor([0.5, 0.8, 0.8, 0.6, 0.4] * 2)
    qd = torch.randn(N, 10, generator=g) * 2.0
    hip.set_state(root.cuda().contiguous(), q.cuda().contiguous(), qd.cuda().contiguous())
    a = random_actions(cfg, N, g, 1.0)
    hip.step(a.cuda(), 5.0, 1)
    torch.cuda.synchronize()
    out = {n: hip.tensor(n).cpu().double().clone() for n in ("CONTACT_FORCES", "DOF_VEL", "ROOT_STATES")}
    hip.close(); ora.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["quad", "quad4"])
def test_quad_self_collision_split_matches_the_lane_pair_kernel(layout, monkeypatch):
    ref = _crossed_legs_step(monkeypatch, 8)
    got = _crossed_legs_step(monkeypatch, layout)
    cf = got["CONTACT_FORCES"]
    loaded = cf.abs().sum(2) > 1.0
    assert int(loaded.any(1).sum()) > 48, "most envs must have their legs in contact"
    assert float(cf.sum(1).abs().max()) < 1e-3 * max(1.0, float(cf.abs().max()))      # internal forces: every env sums to zero
    scale = max(1.0, float(ref["CONTACT_FORCES"].abs().max()))
    d = float((cf - ref["CONTACT_FORCES"]).abs().max())
    assert d < 2e-3 * scale, (d, scale)
    for n in ("DOF_VEL", "ROOT_STATES"):
        d = float((got[n] - ref[n]).abs().max())
        assert d < 1e-3 * max(1.0, float(ref[n].abs().max())), (n, d)
