"""float64 oracle of the two-hot cross-entropy (include/beast_hip.h, beast_xent_rows / _bwd).

For a row l[0..V), a target position u = i + f (i <= V-2, f in [0, 1]) and label smoothing eps:
    m = max l, e = exp(l - m), s = sum e
    q_v    = (1-eps) [(1-f) (v == i) + f (v == i+1)] + eps / V
    loss   = log s + (1-eps) [(1-f) (m - l_i) + f (m - l_{i+1})] + eps sum_v (m - l_v) / V
    grad_v = g (e_v / s - q_v)
    amax   = the lowest v with l_v == m
A term whose weight is exactly 0 contributes exactly 0 (a select: a -inf logit under it does not
matter); under a positive weight a -inf logit gives +inf.  Which two bins carry the target is decided
in fp32, by a replica of the kernel's three roundings: everything after that is float64.  eps is
taken as the fp32 number the kernel receives.  An ignored row (kind IGNORED) has loss 0 and gradient
0, an out-of-range token (kind OUT_OF_RANGE) NaN in both.  Rows run along the last axis; everything
is vectorised over the leading ones.
"""
import numpy as np

TARGET, IGNORED, OUT_OF_RANGE = 0, 1, 2


def target_from_tokens(tokens, V, tok_offset=0, ignore_index=-100):
    """(i, f, kind) of int64 tokens [...]: u = t - tok_offset; a token equal to ignore_index as given
    is ignored, any other outside [tok_offset, tok_offset + V) is out of range."""
    raw = np.asarray(tokens, dtype=np.int64)
    t = raw - tok_offset
    kind = np.where(raw == ignore_index, IGNORED, np.where((t < 0) | (t >= V), OUT_OF_RANGE, TARGET))
    ok = kind == TARGET
    i = np.where(ok, np.minimum(t, V - 2), 0)
    f = np.where(ok, (t - i).astype(np.float64), 0.0)
    return i, f, kind


def position_fp32(x, V):
    """u = clamp(((x + 1) * 0.5) * (V-1), 0, V-1) with every operation rounded to fp32, in this order."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        u = ((x + np.float32(1.0)) * np.float32(0.5)) * np.float32(V - 1)
        return np.minimum(np.maximum(u, np.float32(0.0)), np.float32(V - 1)).astype(np.float32)


def target_from_coeffs(x, V):
    """(i, f, kind) of normalised coefficients [...]: NaN is ignored; f = u - i is exact in fp32."""
    x = np.asarray(x, dtype=np.float32)
    nan = np.isnan(x)
    u = np.where(nan, np.float32(0.0), position_fp32(np.where(nan, np.float32(0.0), x), V)).astype(np.float32)
    i = np.minimum(np.floor(u).astype(np.int64), V - 2)
    f = u.astype(np.float64) - i
    assert np.all(f.astype(np.float32).astype(np.float64) == f) and np.all((f >= 0) & (f <= 1))
    kind = np.where(nan, IGNORED, TARGET)
    return np.where(nan, 0, i), np.where(nan, 0.0, f), kind


def dense_target(i, f, V, eps=0.0):
    """q [..., V] of (i, f)."""
    eps = float(np.float32(eps))
    v = np.arange(V)
    i, f = np.asarray(i)[..., None], np.asarray(f, dtype=np.float64)[..., None]
    return (1.0 - eps) * ((1.0 - f) * (v == i) + f * (v == i + 1)) + eps / V


def rows(logits):
    """(m [...], s [...], amax [...] int64) of logits [..., V]."""
    l = np.asarray(logits, dtype=np.float64)
    m = l.max(-1)
    with np.errstate(invalid="ignore"):
        s = np.exp(l - m[..., None]).sum(-1)
    return m, s, np.argmax(l, axis=-1).astype(np.int64)


def loss(logits, i, f, kind, eps=0.0):
    """loss [...] of logits [..., V]."""
    l = np.asarray(logits, dtype=np.float64)
    V = l.shape[-1]
    eps = float(np.float32(eps))
    i, f = np.asarray(i, dtype=np.int64), np.asarray(f, dtype=np.float64)
    m, s, _ = rows(l)
    li = np.take_along_axis(l, i[..., None], -1)[..., 0]
    li1 = np.take_along_axis(l, i[..., None] + 1, -1)[..., 0]
    with np.errstate(invalid="ignore", over="ignore"):
        hot = np.where(1.0 - f != 0.0, (1.0 - f) * (m - li), 0.0) + np.where(f != 0.0, f * (m - li1), 0.0)
        out = np.log(s) + (1.0 - eps) * hot
        if eps > 0.0:
            out = out + eps * (m[..., None] - l).sum(-1) / V
    return np.where(kind == IGNORED, 0.0, np.where(kind == OUT_OF_RANGE, np.nan, out))


def grad(logits, i, f, kind, grad_loss, eps=0.0):
    """grad_logits [..., V] for the upstream gradient grad_loss [...]."""
    l = np.asarray(logits, dtype=np.float64)
    V = l.shape[-1]
    m, s, _ = rows(l)
    with np.errstate(invalid="ignore"):
        p = np.exp(l - m[..., None]) / s[..., None]
    g = np.asarray(grad_loss, dtype=np.float64)[..., None]
    out = g * (p - dense_target(i, f, V, eps))
    k = np.asarray(kind)[..., None]
    return np.where(k == IGNORED, 0.0, np.where(k == OUT_OF_RANGE, np.nan, out))
