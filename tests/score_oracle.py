"""float64 oracle of scoring tokens under logits (include/beast_hip.h, beast_score_rows / _bwd).

For a row l[0..V), temperature tau and a kept set (tests/sample_oracle.py: ``kept_mask``), with
z = l / tau, zmax = max z, e_v = exp(z_v - zmax) (``sample_oracle.shifted``) and S2 = sum_kept e:
    log pi_v = (z_v - zmax) - log S2 for kept v;  pi_v = 0 and log pi_v = -inf outside the kept set
    logprob_s = log pi_{t_s - tok_offset};  exactly 0 where t_s == ignore_index (as given); NaN for
                any other token outside [tok_offset, tok_offset + V)
    a draw takes part in the backward where its token is in range, not ignored and logprob_s > -inf
    H  = -sum_kept pi_v log pi_v                     terms with pi_v == 0 are exactly 0
    KL = sum_kept pi_v (log pi_v - log rho_v)        rho = softmax(ref / tau) over all V bins;
                                                     +inf where rho_v == 0 < pi_v
    grad_v = (1/tau) [ sum_s g_s 1[t_s = v] - pi_v sum_s g_s - g_H pi_v (log pi_v + H)
                       + g_KL pi_v (log pi_v - log rho_v - KL) ]      (sums over the draws that take part)
    grad_v = 0 where pi_v == 0; a row with an out-of-range token is NaN.
Every function takes the kept mask explicitly: the kept set is a constant of the backward.  Rows run
along the last axis; everything is vectorised over the leading ones, tokens are [S, ...].
"""
import numpy as np

import sample_oracle as SO

IGNORE = -100


def log_pi(logits, kept, temperature=1.0):
    """(log pi [..., V], pi [..., V]) on the kept set given."""
    d, e = SO.shifted(logits, temperature)
    kept = np.asarray(kept, dtype=bool)
    e = np.where(kept, e, 0.0)
    s2 = e.sum(-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(kept, d - np.log(s2), -np.inf), e / s2


def classify(tokens, V, tok_offset=0, ignore_index=IGNORE):
    """(bin [S, ...] int64 clipped into range, ignored [S, ...], bad [S, ...])."""
    t = np.asarray(tokens, dtype=np.int64)
    ignored = t == ignore_index
    rel = t - tok_offset
    bad = ~ignored & ((rel < 0) | (rel >= V))
    return np.clip(rel, 0, V - 1), ignored, bad


def logprob(logits, kept, tokens, temperature=1.0, tok_offset=0, ignore_index=IGNORE):
    """(logprob [S, ...], takes part [S, ...] bool)."""
    lp, _ = log_pi(logits, kept, temperature)
    V = lp.shape[-1]
    rel, ignored, bad = classify(tokens, V, tok_offset, ignore_index)
    out = np.take_along_axis(np.broadcast_to(lp, rel.shape + (V,)), rel[..., None], -1)[..., 0]
    out = np.where(ignored, 0.0, np.where(bad, np.nan, out))
    return out, ~ignored & ~bad & (out > -np.inf)


def _log_rho(ref, temperature):
    d, e = SO.shifted(ref, temperature)
    with np.errstate(divide="ignore"):
        return d - np.log(e.sum(-1, keepdims=True))


def entropy(logits, kept, temperature=1.0):
    lp, pi = log_pi(logits, kept, temperature)
    with np.errstate(invalid="ignore"):
        return -np.where(pi > 0, pi * lp, 0.0).sum(-1)


def kl(logits, ref, kept, temperature=1.0):
    lp, pi = log_pi(logits, kept, temperature)
    with np.errstate(invalid="ignore"):
        return np.where(pi > 0, pi * (lp - _log_rho(ref, temperature)), 0.0).sum(-1)


def grad(logits, kept, temperature=1.0, tokens=None, g_logprob=None, g_entropy=None, g_kl=None, ref=None,
         tok_offset=0, ignore_index=IGNORE):
    """grad_logits [..., V] for the upstream gradients given (each may be None)."""
    lp, pi = log_pi(logits, kept, temperature)
    V = lp.shape[-1]
    inner = np.zeros(lp.shape)
    q = np.zeros(lp.shape)                      # pi_v multiplies -q_v
    bad_row = np.zeros(lp.shape[:-1], dtype=bool)
    if g_logprob is not None:
        _, part = logprob(logits, kept, tokens, temperature, tok_offset, ignore_index)
        rel, _, bad = classify(tokens, V, tok_offset, ignore_index)
        g = np.where(part, np.asarray(g_logprob, dtype=np.float64), 0.0)
        onehot = rel[..., None] == np.arange(V)
        inner += (g[..., None] * onehot).sum(0)
        q += g.sum(0)[..., None]
        bad_row = bad.any(0)
    with np.errstate(invalid="ignore"):
        if g_entropy is not None:
            H = entropy(logits, kept, temperature)
            q += np.asarray(g_entropy, dtype=np.float64)[..., None] * (lp + H[..., None])
        if g_kl is not None:
            D = kl(logits, ref, kept, temperature)
            q -= np.asarray(g_kl, dtype=np.float64)[..., None] * (lp - _log_rho(ref, temperature) - D[..., None])
        out = (inner - np.where(pi > 0, pi * q, 0.0)) / float(temperature)
    return np.where(bad_row[..., None], np.nan, out)
