"""Float64 restatements for rl/cenet.py (the context-aided estimator network), written from the formulas and used by
tests/test_cenet.py and tests/test_cenet_gpu.py: the head ([x | v_hat | z] and the column select), the reparameterisation and its
backward, the three losses with the gradients with respect to the encoder's and the decoder's outputs, and one whole minibatch step with
the gradient of every weight and bias of both networks.  numpy only.

    enc_out = [v_hat (E) | mu (Z) | raw (Z)],  lv = clip(raw, -10, 2),  sigma = exp(lv / 2),  z = sigma eps + mu
    L_est = sum (v_hat - v)^2 / (mb E);  L_rec = sum_{valid} (dec - next)^2 / (F max(n_v, 1));  L_kl = sum (mu^2 + exp(lv) - lv - 1) / 2 / mb
    L = L_est + L_rec + beta L_kl;  d lv / d raw = 1 for -10 <= raw <= 2, else 0"""
import numpy as np

LV_MIN, LV_MAX = -10.0, 2.0


def elu(z):
    return np.where(z > 0, z, np.expm1(np.minimum(z, 0.0)))


def mlp_ref(weights, biases, x):
    """Linear -> ELU(1) -> ... -> Linear: (output, every layer's input)"""
    h = np.asarray(x, dtype=np.float64)
    inputs = []
    for l, (w, b) in enumerate(zip(weights, biases)):
        inputs.append(h)
        z = h @ np.asarray(w, dtype=np.float64).T + np.asarray(b, dtype=np.float64)
        h = elu(z) if l + 1 < len(weights) else z
    return h, inputs


def mlp_backward_ref(weights, inputs, g):
    """(d weights, d biases, d input) from the gradient g at the output"""
    dws, dbs = [None] * len(weights), [None] * len(weights)
    for l in range(len(weights) - 1, -1, -1):
        dws[l], dbs[l] = g.T @ inputs[l], g.sum(0)
        g = g @ np.asarray(weights[l], dtype=np.float64)
        if l > 0:
            h = inputs[l]                              # = elu(z) of layer l - 1: elu'(z) = 1 for z > 0, elu(z) + 1 otherwise
            g = g * np.where(h > 0, 1.0, h + 1.0)
    return dws, dbs, g


def split(enc_out, E, Z):
    e = np.asarray(enc_out, dtype=np.float64)
    return e[:, :E], e[:, E:E + Z], e[:, E + Z:E + 2 * Z]


def unsaturated(raw):
    return (raw >= LV_MIN) & (raw <= LV_MAX)


def reparam_ref(enc_out, eps, E, Z):
    """dec_in = [v_hat | z]"""
    v, mu, raw = split(enc_out, E, Z)
    sigma = np.exp(0.5 * np.clip(raw, LV_MIN, LV_MAX))
    return np.concatenate([v, sigma * np.asarray(eps, dtype=np.float64) + mu], axis=1)


def reparam_backward_ref(enc_out, eps, d_dec_in, E, Z):
    """d enc_out from d dec_in: d v_hat passes, d mu = dz, d raw = dz sigma eps / 2 where the clamp is not saturated"""
    _, _, raw = split(enc_out, E, Z)
    d = np.asarray(d_dec_in, dtype=np.float64)
    dz = d[:, E:]
    sigma = np.exp(0.5 * np.clip(raw, LV_MIN, LV_MAX))
    d_raw = np.where(unsaturated(raw), dz * 0.5 * sigma * np.asarray(eps, dtype=np.float64), 0.0)
    return np.concatenate([d[:, :E], dz, d_raw], axis=1)


def head_ref(x, enc_out, eps, E, Z, pri=None, cols=None):
    """([x | v_hat | z], pri[:, cols] or None)"""
    out = np.concatenate([np.asarray(x, dtype=np.float64), reparam_ref(enc_out, eps, E, Z)], axis=1)
    return out, (None if pri is None else np.asarray(pri, dtype=np.float64)[:, list(cols)])


def loss_ref(enc_out, targets, dec, nxt, valid, beta, E, Z):
    """(out = [L_est, L_rec, L_kl, L, n_v], d L / d enc_out, d L / d dec); nxt [mb, F] may hold anything in rows where valid is 0"""
    v, mu, raw = split(enc_out, E, Z)
    dec, y = np.asarray(dec, dtype=np.float64), np.asarray(targets, dtype=np.float64)
    mb, F = dec.shape
    ok = np.asarray(valid).reshape(-1) != 0
    n_v = int(ok.sum())
    lv = np.clip(raw, LV_MIN, LV_MAX)
    l_est = ((v - y) ** 2).sum() / (mb * E)
    diff = np.zeros_like(dec)
    diff[ok] = dec[ok] - np.asarray(nxt, dtype=np.float64)[ok]     # (a select: a masked row's successor is never read)
    l_rec = (diff ** 2).sum() / (F * max(n_v, 1))
    l_kl = (0.5 * (mu * mu + np.exp(lv) - lv - 1.0)).sum() / mb
    total = l_est + l_rec + beta * l_kl
    d_v = 2.0 * (v - y) / (mb * E)
    d_mu = beta * mu / mb
    d_raw = np.where(unsaturated(raw), beta * 0.5 * (np.exp(lv) - 1.0) / mb, 0.0)
    d_dec = 2.0 * diff / (F * max(n_v, 1))
    return np.array([l_est, l_rec, l_kl, total, float(n_v)]), np.concatenate([d_v, d_mu, d_raw], axis=1), d_dec


def step_ref(enc_w, enc_b, dec_w, dec_b, x, targets, nxt, valid, eps, beta, E, Z):
    """one minibatch through both networks: (out [5], d encoder weights, d encoder biases, d decoder weights, d decoder biases)"""
    enc_out, enc_in = mlp_ref(enc_w, enc_b, x)
    dec_in = reparam_ref(enc_out, eps, E, Z)
    dec, dec_inputs = mlp_ref(dec_w, dec_b, dec_in)
    out, d_enc, d_dec = loss_ref(enc_out, targets, dec, nxt, valid, beta, E, Z)
    ddw, ddb, d_dec_in = mlp_backward_ref(dec_w, dec_inputs, d_dec)
    d_enc = d_enc + reparam_backward_ref(enc_out, eps, d_dec_in, E, Z)
    dew, deb, _ = mlp_backward_ref(enc_w, enc_in, d_enc)
    return out, dew, deb, ddw, ddb
