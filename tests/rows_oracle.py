"""Float64 oracle of the per-trajectory weighted ridge fit (include/beast_hip.h,
beast_encode_rows_f32; BEASTBsplineTokenizer.encode_at) -- TEST INFRASTRUCTURE ONLY.

The definition, not the kernel's arithmetic: per trajectory and DoF kind the fp32 basis of
``oracle.beast_oracle.basis`` at the trajectory's own times (bitwise the reference's
UniBSplineBasis.basis for [B, T] times), then G = Phi^T diag(w) Phi + reg I and
R = Phi^T diag(w) Y in float64, ``np.linalg.solve``, one rounding to fp32.  A weight of 0 skips
the sample: its time and values are replaced before anything is computed, so they may be NaN.

Also here: the seeded inputs that tests/golden/gen_rows_goldens.py and tests/test_gpu_rows.py share.
"""
from __future__ import annotations

import numpy as np

from oracle import beast_oracle as O

F32 = np.float32


def _rows(x, B, T, dtype):
    x = np.asarray(x, dtype=dtype)
    assert x.shape in ((T,), (B, T)), (x.shape, B, T)
    return np.broadcast_to(x, (B, T))


def fit(trajs, times, weights=None, *, tau, degree, num_basis, joint_indices, gripper_indices=(), reg=1e-9):
    """(params fp32 [B, D*N] in (d n) order, DoFs joint ++ gripper; cond(G) float64 [B, kinds]).

    trajs [B, T, Din]; times [T] or [B, T] (taken through fp32, as the kernel reads them); weights
    None, [T] or [B, T]; tau through fp32, as the tokenizer holds it."""
    trajs = np.asarray(trajs)
    B, T, _ = trajs.shape
    t = _rows(times, B, T, F32)
    w = np.ones((B, T)) if weights is None else _rows(weights, B, T, F32).astype(np.float64)
    keep = w != 0
    t = np.where(keep, t, F32(0))
    params, conds = [], []
    for idx, deg in ((list(joint_indices), degree), (list(gripper_indices), 0)):
        if not idx:
            continue
        phi = O.basis(t, F32(tau), deg, num_basis).astype(np.float64)           # [B, T, N]
        phi = np.where(keep[..., None], phi, 0.0)
        y = np.where(keep[..., None], trajs[..., idx].astype(np.float64), 0.0)
        G = np.einsum("btn,bt,btm->bnm", phi, w, phi) + reg * np.eye(num_basis)
        R = np.einsum("btn,bt,btd->bnd", phi, w, y)
        W = np.linalg.solve(G, R)                                               # [B, N, d]
        params.append(W.transpose(0, 2, 1).reshape(B, -1))
        conds.append(np.linalg.cond(G))
    return np.concatenate(params, axis=-1).astype(F32), np.stack(conds, axis=-1)


def tokens(params, w_min, w_max, vocab, num_dof, num_basis, offset=0):
    """The tokenizer's epilogue on fp32 params [B, (d n)]: clamp, continuous_to_discrete
    (beast/utils.py:4-17), (d n) -> (n d), + offset."""
    tok = O.continuous_to_discrete(O._clamp_t(params, w_min, w_max), w_min, w_max, vocab)
    B = tok.shape[0]
    return tok.reshape(B, num_dof, num_basis).transpose(0, 2, 1).reshape(B, -1) + offset


def parity_ok(got, ref, factor=1e-5):
    """The project's parity criterion (tests/test_gpu_parity.py): |got - ref| <= factor * max(1, |ref row|_inf)."""
    ref = np.asarray(ref, dtype=np.float64)
    scale = np.maximum(1.0, np.abs(ref).max(axis=1, keepdims=True))
    return np.abs(np.asarray(got, dtype=np.float64) - ref) <= factor * scale


def parity_err(got, ref):
    """max over the batch of |got - ref| / max(1, |ref row|_inf)."""
    ref = np.asarray(ref, dtype=np.float64)
    scale = np.maximum(1.0, np.abs(ref).max(axis=1, keepdims=True))
    return float((np.abs(np.asarray(got, dtype=np.float64) - ref) / scale).max()) if ref.size else 0.0


# ------------------------------------------------------------------ inputs --
def random_walk(B, T, D, seed, step=0.05, start=1.0):
    """Random-walk trajectories [B, T, D] fp32: a start in [-start, start] plus Gaussian steps."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-start, start, (B, 1, D)) + np.cumsum(rng.normal(0, step, (B, T, D)), axis=1)
    return x.astype(F32)


def jittered_times(B, T, duration, seed, jitter=0.4):
    """[B, T] fp32: the uniform grid over [0, duration], every stamp moved by up to +-jitter
    grid steps (sorted for jitter < 0.5; the ends leave [0, duration], where the phase clips)."""
    rng = np.random.default_rng(seed)
    grid = np.linspace(0.0, duration, T)
    dt = duration / max(T - 1, 1)
    return (grid[None, :] + rng.uniform(-jitter, jitter, (B, T)) * dt).astype(F32)


def census_inputs(B=128, T=50, D=7, seed=31):
    """(x, times, 0/1 weights) with each sample kept with probability 1/2: rows whose Gram
    matrices range from well conditioned to cond(G) >= 1e4 (a basis function left with hardly a
    sample), where an fp32 Gram or solve would lose cond * 6e-8."""
    rng = np.random.default_rng(seed + 2)
    w = (rng.random((B, T)) < 0.5).astype(F32)
    return random_walk(B, T, D, seed), jittered_times(B, T, 2 * np.pi, seed + 1), w


def keep_mask(B, T, n_keep, seed):
    """0/1 weights [B, T] fp32 with exactly n_keep ones per row."""
    rng = np.random.default_rng(seed)
    w = np.zeros((B, T), dtype=F32)
    for b in range(B):
        w[b, rng.choice(T, n_keep, replace=False)] = 1
    return w
