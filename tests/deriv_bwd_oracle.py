"""Numpy oracle of beast_reconstruct_derivs_bwd_f32 (include/beast_hip.h): the definition in
float64, not the kernel's arithmetic.

    S[b][d][n]             = sum_o sum_t basis_o[kind(d)][t][n] * G_o[b][t][dof_dst[d]]
    grad_ntokens[b][n][d]  = (-1 <= x <= 1) ? S[b][d][n] * s[d][n] : 0
    s[d][n]                = 0.5f * (w_max - w_min) in float32, the derivative of denormalize_tensor

o runs over the gradients given (gripper DoFs, d >= n_joint: order 0 only, from the kind-1 slab);
with init_p, coefficient 0 of the joint DoFs gets 0 and its S goes to grad_init_p instead.  The
slabs of orders without a gradient are never touched, so they may hold NaN.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

EPS = 2.0 ** -24


class Backward(NamedTuple):
    grad_ntokens: np.ndarray             # [B, N, D] float64
    grad_init_p: Optional[np.ndarray]    # [B, width] float64, zero outside the named columns
    S: np.ndarray                        # [B, D, N] the unscaled, unmasked sums
    mag: np.ndarray                      # [B, D, N] sum_o sum_t |basis * G|
    scale: np.ndarray                    # [D, N] s, float32 values held in float64
    terms: int                           # K: products per sum for the joint DoFs


def scale(w_min, w_max) -> np.ndarray:
    lo, hi = np.asarray(w_min, dtype=np.float32), np.asarray(w_max, dtype=np.float32)
    return (np.float32(0.5) * (hi - lo)).astype(np.float64)


def backward(grads, basis, w_min, w_max, ntokens, dof_dst, n_joint, init_p_src=None, init_p_width=None) -> Backward:
    """grads: three entries (pos, vel, acc), each None or [B, T, num_dof_out]; basis [3, 2, T, N]
    or per row [B, 3, 2, T, N]; w_min / w_max [D, N]; ntokens [B, N, D]; dof_dst [D].
    init_p_src [>= n_joint] switches the init_p rule on; init_p_width asks for grad_init_p."""
    x = np.asarray(ntokens)
    B, N, D = x.shape
    basis = np.asarray(basis)
    per_row = basis.ndim == 5
    S = np.zeros((B, D, N))
    mag = np.zeros((B, D, N))
    for o, g in enumerate(grads):
        if g is None:
            continue
        g = np.asarray(g, dtype=np.float64)
        for d in range(D):
            kind = 0 if d < n_joint else 1
            if o and kind:
                continue
            ph = (basis[:, o, kind] if per_row else basis[o, kind]).astype(np.float64)   # [B, T, N] / [T, N]
            col = g[:, :, int(dof_dst[d])]                                               # [B, T]
            sub = "btn,bt->bn" if per_row else "tn,bt->bn"
            S[:, d, :] += np.einsum(sub, ph, col)
            mag[:, d, :] += np.einsum(sub, np.abs(ph), np.abs(col))
    s = scale(w_min, w_max).reshape(D, N)
    with np.errstate(invalid="ignore"):
        ok = (x >= -1) & (x <= 1)                                                        # NaN: False
    gx = np.where(ok.transpose(0, 2, 1), S * s[None], 0.0)                               # [B, D, N], a select
    gip = None
    if init_p_src is not None:
        gx[:, :n_joint, 0] = 0.0
        if init_p_width is not None:
            gip = np.zeros((B, init_p_width))
            for d in range(n_joint):
                gip[:, int(init_p_src[d])] = S[:, d, 0]
    terms = sum(g is not None for g in grads) * basis.shape[-2]
    return Backward(np.ascontiguousarray(gx.transpose(0, 2, 1)), gip, S, mag, s, terms)


def bound(r: Backward) -> np.ndarray:
    """[B, N, D]: the summation's own error bound, (K + 3) 2^-24 s sum|basis * G| -- any order of K
    fp32 products, plus the roundings of s and of the final scale."""
    return ((r.terms + 3) * EPS * r.scale[None] * r.mag).transpose(0, 2, 1)
