"""float64 oracle of the logits decode (include/beast_hip.h, beast_logits_expect / _bwd).

For a row l[0..V) and tau > 0:
    z = l / tau, zmax = max z, e = exp(z - zmax), s = sum e
    mean = clamp(sum e x / s, -1, 1), x_v = 2v/(V-1) - 1
    amax = the lowest v with l_v == max l          (raw logits)
    grad_l_v = (g / tau) (e_v / s) (x_v - mean)       (mean before the clamp, whose derivative is 1)
Rows run along the last axis; everything is vectorised over the leading ones.
"""
import numpy as np


def bins(V):
    """x_v = 2v/(V-1) - 1, float64 [V]."""
    return 2.0 * np.arange(V, dtype=np.float64) / (V - 1) - 1.0


def expect(logits, tau=1.0):
    """(mean [...], amax [...] int64, stats [..., 2] = (zmax, s)) of logits [..., V]."""
    l = np.asarray(logits, dtype=np.float64)
    z = l / tau
    zmax = z.max(-1, keepdims=True)
    with np.errstate(invalid="ignore"):
        e = np.exp(z - zmax)
    s = e.sum(-1)
    mean = np.clip((e * bins(l.shape[-1])).sum(-1) / s, -1.0, 1.0)
    amax = np.argmax(l, axis=-1).astype(np.int64)          # numpy's argmax returns the first maximum
    return mean, amax, np.stack([zmax[..., 0], s], -1)


def grad(logits, grad_mean, tau=1.0):
    """grad_logits [..., V] for the upstream gradient grad_mean [...]."""
    l = np.asarray(logits, dtype=np.float64)
    V = l.shape[-1]
    _, amax, stats = expect(l, tau)
    with np.errstate(invalid="ignore"):
        p = np.exp(l / tau - stats[..., :1]) / stats[..., 1:]
    g = np.asarray(grad_mean, dtype=np.float64)[..., None]
    # x_v - mean measured from the bin c that holds the maximum: x_v - x_c = 2 (v - c) / (V-1) has one
    # rounding and mean - x_c = sum_u p_u (x_u - x_c) has no term for u = c, so a peaked row (mean
    # within 2^-53 of x_c, where bins - mean would cancel to 0) keeps its relative accuracy
    d = 2.0 * (np.arange(V, dtype=np.float64) - amax[..., None]) / (V - 1)
    mu = (p * d).sum(-1, keepdims=True)
    return (g / tau) * p * (d - mu)
