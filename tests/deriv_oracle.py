"""Numpy oracle of the B-spline time derivatives (include/beast_hip.h, beast_bspline_basis_deriv_f32).

The definition, not the kernel's arithmetic: recursive Cox-de Boor on the project's knot vector,
the phase clipped to [0, 1] first, zero-denominator terms dropped, degree-0 spans [k_i, k_{i+1})
with the last non-degenerate one closed, one 1/tau per derivative order.  ``dtype`` is float64
for the oracle proper; float32 runs the same steps in single precision (the yardstick for the
second derivative's rounding error).
"""
from __future__ import annotations

import numpy as np

from beast_tokenizer_amd.bspline import knot_vector


def knots(degree: int, n_ctrl: int, dtype=np.float64) -> np.ndarray:
    """The project's clamped uniform knots (built in float32, as the reference builds them)."""
    return knot_vector(degree, n_ctrl).numpy().astype(dtype)


def _b(i, k, kv, u, last):
    if k == 0:
        hi = (u <= kv[i + 1]) if i == last else (u < kv[i + 1])
        return ((u >= kv[i]) & hi).astype(u.dtype)
    out = np.zeros_like(u)
    d1 = kv[i + k] - kv[i]
    if d1 != 0:
        out = out + (u - kv[i]) / d1 * _b(i, k - 1, kv, u, last)
    d2 = kv[i + k + 1] - kv[i + 1]
    if d2 != 0:
        out = out + (kv[i + k + 1] - u) / d2 * _b(i + 1, k - 1, kv, u, last)
    return out


def _db(i, k, r, kv, u, last):
    """d^r/du^r of B_{i,k}."""
    if r == 0:
        return _b(i, k, kv, u, last)
    if k < r:
        return np.zeros_like(u)
    out = np.zeros_like(u)
    d1 = kv[i + k] - kv[i]
    if d1 != 0:
        out = out + _db(i, k - 1, r - 1, kv, u, last) / d1
    d2 = kv[i + k + 1] - kv[i + 1]
    if d2 != 0:
        out = out - _db(i + 1, k - 1, r - 1, kv, u, last) / d2
    return u.dtype.type(k) * out


def phase(times, tau, delay=0.0, dtype=np.float64) -> np.ndarray:
    t = np.asarray(times).astype(dtype)
    return np.clip((t - dtype(delay)) / dtype(np.float32(tau)), dtype(0), dtype(1))


def deriv_basis(times, tau, degree: int, n_ctrl: int, order: int, delay=0.0, dtype=np.float64) -> np.ndarray:
    """[*times.shape, n_ctrl]: d^order/dt^order of B_{n,degree} at the clipped phase of ``times``
    (tau is taken through float32, as the tokenizer holds it)."""
    dtype = np.dtype(dtype).type
    kv = knots(degree, n_ctrl, dtype)
    u = phase(times, tau, delay, dtype)
    cols = [_db(i, degree, order, kv, u, n_ctrl - 1) for i in range(n_ctrl)]
    out = np.stack(cols, axis=-1)
    for _ in range(order):
        out = out / dtype(np.float32(tau))
    return out.astype(dtype)


def control_points(w, ic: int = 0, ec: int = 0, params_init=None, params_end=None) -> np.ndarray:
    """All C = N + ic + |ec| control points [..., C] of the joint spline from the fitted ones
    w [..., N] and the stored boundary control points (the extension of get_traj_pos; end
    order -1 repeats the last fitted point and subtracts params_end from the one before)."""
    parts = [w]
    if ic:
        parts.insert(0, np.asarray(params_init).astype(w.dtype))
    if ec == -1:
        ext = np.concatenate(parts + [w[..., -1:]], axis=-1)
        ext[..., -2] -= np.asarray(params_end).astype(w.dtype)[..., 0]
        return ext
    if ec:
        parts.append(np.asarray(params_end).astype(w.dtype))
    return np.concatenate(parts, axis=-1)


def trajectory(times, tau, degree: int, ctrl, order: int, init_pos=None, dtype=np.float64) -> np.ndarray:
    """[B, T, d]: the order-th derivative of the splines with control points ctrl [B, d, C] at
    times [T] or [B, T]; init_pos [B, d] is the constant offset of order 0."""
    dtype = np.dtype(dtype).type
    ctrl = np.asarray(ctrl).astype(dtype)
    basis = deriv_basis(times, tau, degree, ctrl.shape[-1], order, dtype=dtype)
    if basis.ndim == 2:
        out = np.einsum("tk,bdk->btd", basis, ctrl)
    else:
        out = np.einsum("btk,bdk->btd", basis, ctrl)
    if order == 0 and init_pos is not None:
        out = out + np.asarray(init_pos).astype(dtype)[:, None, :]
    return out.astype(dtype)


def rel_err(got, want) -> float:
    """max|got - want| / max|want|, the derivative tests' error measure; want must not be all zero."""
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / np.abs(want).max())
