"""Brute-force oracle of reconstruct_windows / beast_reconstruct_windows_f32: plain loops and numpy
float64, no op of the code under test.

A window is (start, end) in rows of a flat [R] buffer; its sample t < min(T, end - start) lies on row
start + t, later samples are edge padding and own no row.  Row r is the blend-weighted mean, over the
windows that own it in table order and whose blend weight there is not 0, of their samples."""
import numpy as np


def clamp_table(starts, ends, R):
    """The kernel's view of a table: start into [0, R - 1], end into [start + 1, R]."""
    s = np.clip(np.asarray(starts, dtype=np.int64), 0, R - 1)
    e = np.minimum(np.maximum(np.asarray(ends, dtype=np.int64), s + 1), R)
    return s, e


def contributors(starts, ends, T, R, blend):
    """Per row the list of (w, t) in table order: window w owns the row as sample t and blend[t] != 0."""
    out = [[] for _ in range(R)]
    for w, (s, e) in enumerate(zip(np.asarray(starts).tolist(), np.asarray(ends).tolist())):
        for t in range(min(T, e - s)):
            r = s + t
            if 0 <= r < R and blend[t] != 0:
                out[r].append((w, t))
    return out


def blend(y, starts, ends, blend_w, R, fill):
    """y [W, T, D] per-window values.  Returns float64 ``out`` [R, D], int32 ``coverage`` [R], float64
    ``weight`` [R], and per element the number of contributors ``C`` [R, D] and ``ymax`` = max_k |y_k|
    [R, D] (0 where C = 0): what the error bound of a C-term blend is stated in."""
    y = np.asarray(y, dtype=np.float64)
    W, T, D = y.shape
    bw = np.asarray(blend_w, dtype=np.float64)
    out = np.full((R, D), float(fill), dtype=np.float64)
    coverage = np.zeros(R, dtype=np.int32)
    weight = np.zeros(R, dtype=np.float64)
    C = np.zeros((R, D), dtype=np.int64)
    ymax = np.zeros((R, D), dtype=np.float64)
    for r, lst in enumerate(contributors(starts, ends, T, R, bw)):
        if not lst:
            continue
        num = np.zeros(D)
        den = 0.0
        for w, t in lst:
            num += bw[t] * y[w, t]
            den += bw[t]
            ymax[r] = np.maximum(ymax[r], np.abs(y[w, t]))
        out[r] = num / den
        coverage[r] = len(lst)
        weight[r] = den
        C[r] = len(lst)
    return out, coverage, weight, C, ymax


def blend_dense(y, starts, ends, blend_w, R, fill):
    """The same by a dense [R, W] weight matrix: M[r, w] = blend[r - start_w] where window w owns r."""
    y = np.asarray(y, dtype=np.float64)
    W, T, D = y.shape
    bw = np.asarray(blend_w, dtype=np.float64)
    s = np.asarray(starts, dtype=np.int64)
    n = np.minimum(T, np.asarray(ends, dtype=np.int64) - s)
    t = np.arange(R, dtype=np.int64)[:, None] - s[None, :]                 # [R, W]
    own = (t >= 0) & (t < n[None, :])
    tc = np.clip(t, 0, T - 1)
    M = np.where(own, bw[tc], 0.0)
    used = own & (M != 0)
    yy = y[np.arange(W)[None, :], tc]                                       # [R, W, D]
    num = np.einsum("rw,rwd->rd", np.where(used, M, 0.0), np.where(used[..., None], yy, 0.0))
    den = M.sum(1)
    cov = used.sum(1).astype(np.int32)
    out = np.where(cov[:, None] > 0, num / np.where(den == 0, 1.0, den)[:, None], float(fill))
    return out, cov, den
