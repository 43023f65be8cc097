"""float64 oracle of sampling from logits (include/beast_hip.h, beast_sample_rows).

For a row l[0..V), temperature tau, top_k = k, top_p = p and uniforms u_s in [0, 1):
    z = l / tau, zmax = max z, e_v = exp(z_v - zmax)
    top-k (1 <= k < V):  theta_k = the k-th largest value of l counting multiplicity,
                         K1 = {v : l_v >= theta_k}; k = 0 or k >= V: every bin
    top-p (0 < p < 1):   S1 = sum_{K1} e, theta_p = the largest value t among {l_v : v in K1} with
                         sum_{v in K1, l_v >= t} e_v >= p S1, kept = {v in K1 : l_v >= theta_p};
                         p = 1: kept = K1
    draw:                S2 = sum_kept e, C_v = sum_{w <= v, w in kept} e_w (ascending index),
                         tok_s = the lowest kept v with C_v > u_s S2, or the highest kept v with
                         e_v > 0 where rounding leaves none,
                         logprob_s = (z_tok - zmax) - log S2,  kept_count = |kept|
The thresholds compare the raw l; ties at either threshold stay whole.  Rows run along the last
axis; everything is vectorised over the leading ones.
"""
import numpy as np


def shifted(logits, temperature=1.0):
    """(z - zmax [..., V], e [..., V]) of logits [..., V]."""
    l = np.asarray(logits, dtype=np.float64)
    z = l / float(temperature)
    with np.errstate(invalid="ignore"):
        d = z - z.max(-1, keepdims=True)
        return d, np.exp(d)


def top_k_mask(logits, top_k=0):
    """K1 [..., V] (bool)."""
    l = np.asarray(logits, dtype=np.float64)
    V = l.shape[-1]
    if not 1 <= top_k < V:
        return np.ones(l.shape, dtype=bool)
    theta = -np.sort(-l, axis=-1)[..., top_k - 1:top_k]
    return l >= theta


def kept_mask(logits, temperature=1.0, top_k=0, top_p=1.0):
    """kept [..., V] (bool)."""
    l = np.asarray(logits, dtype=np.float64)
    k1 = top_k_mask(l, top_k)
    if top_p >= 1.0:
        return k1
    _, e = shifted(l, temperature)
    order = np.argsort(-l, axis=-1, kind="stable")
    ls = np.take_along_axis(l, order, -1)
    es = np.take_along_axis(e * k1, order, -1)
    ks = np.take_along_axis(k1, order, -1)
    cum = np.cumsum(es, axis=-1)
    s1 = cum[..., -1:]
    # the mass of {l >= ls_i}: the cumulative sum at the end of i's tie group
    last = np.concatenate([ls[..., :-1] != ls[..., 1:], np.ones(ls.shape[:-1] + (1,), dtype=bool)], -1)
    group = np.minimum.accumulate(np.where(last, cum, np.inf)[..., ::-1], axis=-1)[..., ::-1]
    ok = ks & (group >= float(top_p) * s1)
    first = np.argmax(ok, axis=-1)[..., None]                # descending order: the largest such value
    theta = np.take_along_axis(ls, first, -1)
    return k1 & (l >= theta)


def cdf(logits, temperature=1.0, kept=None):
    """(C [..., V], e restricted to kept [..., V]) with C the index-order inclusive prefix."""
    _, e = shifted(logits, temperature)
    if kept is not None:
        e = e * kept
    return np.cumsum(e, axis=-1), e


def draw(logits, uniforms, temperature=1.0, kept=None):
    """(tokens [S, ...] int64, logprob [S, ...]) for uniforms [S, ...] from the kept set given (default:
    every bin)."""
    d, _ = shifted(logits, temperature)
    C, e = cdf(logits, temperature, kept)
    u = np.asarray(uniforms, dtype=np.float64)
    V = C.shape[-1]
    s2 = C[..., -1]
    hit = (C[None] > (u * s2[None])[..., None]) & (e > 0)[None]
    tok = np.argmax(hit, axis=-1)
    highest = V - 1 - np.argmax((e > 0)[..., ::-1], axis=-1)
    tok = np.where(hit.any(-1), tok, highest[None]).astype(np.int64)
    dt = np.take_along_axis(np.broadcast_to(d, tok.shape + (V,)), tok[..., None], -1)[..., 0]
    with np.errstate(divide="ignore"):
        return tok, dt - np.log(s2)[None]


def sample(logits, uniforms, temperature=1.0, top_k=0, top_p=1.0):
    """(tokens [S, ...] int64, logprob [S, ...], kept_count [...] int64)."""
    kept = kept_mask(logits, temperature, top_k, top_p)
    tok, lp = draw(logits, uniforms, temperature, kept)
    return tok, lp, kept.sum(-1).astype(np.int64)


def probabilities(logits, temperature=1.0, top_k=0, top_p=1.0):
    """P [..., V]: the distribution the draws come from."""
    kept = kept_mask(logits, temperature, top_k, top_p)
    _, e = cdf(logits, temperature, kept)
    return e / e.sum(-1, keepdims=True)
