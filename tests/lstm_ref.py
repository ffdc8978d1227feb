"""Float64 reference of the recurrent policy's LSTM (rl/recurrent.py): torch.nn.LSTMCell / torch.nn.LSTM in float64 with
the module's parameters loaded by name.  A sequence with resets is NOT run through a masked recurrence here: each env's T steps are cut
after its dones and every piece goes through nn.LSTM on its own -- the first from (h0, c0), every later one from zero.  That is rsl_rl's
padded-trajectory semantics, written independently of the code under test."""
import numpy as np
import torch
from torch import nn

NAMES = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")

# dones [T = 6][n = 5]: env 0 ends at t = 0, env 1 at t = T - 1, env 2 twice in a row, env 3 never, env 4 at every step
DONES = np.array([[1, 0, 0, 0, 1],
                  [0, 0, 0, 0, 1],
                  [0, 0, 1, 0, 1],
                  [0, 0, 1, 0, 1],
                  [0, 0, 0, 0, 1],
                  [0, 1, 0, 0, 1]], dtype=np.uint8)


def dones(n):
    """the pattern above repeated over n rows: [6, n] uint8"""
    return np.tile(DONES, (1, -(-n // 5)))[:, :n].copy()


def resets_of(d):
    """what the update's forward takes: row t = the rows step t starts from zero = dones[t - 1]; row 0 is empty"""
    r = np.zeros_like(d)
    r[1:] = d[:-1]
    return r


def params64(rnn):
    """an nn.LSTM's four tensors by name, float64 on the CPU"""
    return {k: getattr(rnn, k).detach().cpu().double().clone() for k in NAMES}


def lstm64(params, requires_grad=False):
    H, D = params["weight_hh_l0"].shape[1], params["weight_ih_l0"].shape[1]
    m = nn.LSTM(D, H, 1).double()
    m.load_state_dict({k: params[k] for k in NAMES})
    for p in m.parameters():
        p.requires_grad_(requires_grad)
    return m


def cell64(params, x, h, c, reset=None):
    """(h, c) of one step through nn.LSTMCell in float64; reset [M]: the rows whose previous state is taken as zero"""
    H, D = params["weight_hh_l0"].shape[1], params["weight_ih_l0"].shape[1]
    cell = nn.LSTMCell(D, H).double()
    cell.load_state_dict({"weight_ih": params["weight_ih_l0"], "weight_hh": params["weight_hh_l0"], "bias_ih": params["bias_ih_l0"],
                          "bias_hh": params["bias_hh_l0"]})
    h, c = torch.as_tensor(h).double().clone(), torch.as_tensor(c).double().clone()
    if reset is not None:
        rs = torch.as_tensor(np.asarray(reset)) != 0
        h[rs] = 0.0
        c[rs] = 0.0
    with torch.no_grad():
        return cell(torch.as_tensor(x).double(), (h, c))


def sequence64(m, x, d, h0, c0):
    """h [T, n, H] of the float64 module m over x [T, n, D] with dones d [T, n]: per env, cut after every done, each piece through m"""
    T, n, _ = x.shape
    d = np.asarray(d)
    cols = []
    for e in range(n):
        pieces, start = [], 0
        state = (h0[e].reshape(1, 1, -1), c0[e].reshape(1, 1, -1))
        for t in range(T):
            if d[t, e] or t == T - 1:
                out, _ = m(x[start:t + 1, e:e + 1], state)
                pieces.append(out)
                start = t + 1
                state = (torch.zeros_like(state[0]), torch.zeros_like(state[1]))
        cols.append(torch.cat(pieces, dim=0))
    return torch.cat(cols, dim=1)


def cell_inputs(M, D, H, seed=0):
    """(x, h_prev, c_prev, reset) as float32 / uint8 numpy arrays: h in (-1, 1), c of order one, every third row reset"""
    g = np.random.default_rng(seed + 1000 * M + 10 * D + H)
    x = g.standard_normal((M, D)).astype(np.float32)
    h = np.tanh(g.standard_normal((M, H))).astype(np.float32)
    c = g.standard_normal((M, H)).astype(np.float32)
    reset = (np.arange(M) % 3 == 0).astype(np.uint8)
    return x, h, c, reset
