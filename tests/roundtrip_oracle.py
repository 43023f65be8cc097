"""float64 numpy oracle of ``beast_roundtrip_stats_f32`` and the tolerances its outputs are held to.

Everything is in DoF order (joint DoFs, then gripper DoFs), as the entry point's ``stats_out``:

    y        [B, T, D] fp32   the input samples, traj[..., dof_src]
    pos32    [B, T, D] fp32   what beast_reconstruct_f32 returns for encode's tokens (the yardstick)
    params32 [B, D, N] fp32   encode's unclamped, unquantised params
    phi32    [2, T, N] fp32   the basis of kind 0 (joint DoFs, d < n_joint) and kind 1 (gripper DoFs)
    w_min, w_max [D * N]      the bounds, (d n) order

``stats`` gives the float64 value of each statistic; ``tol_*`` the distance an fp32 evaluation in
any summation order may keep from it.  With u = 2^-24 (fp32 unit roundoff):

  * sum_t x_t over T terms in any order: |fl - exact| <= gamma_{T-1} sum|x_t| <= T u sum|x_t|; the
    bounds below grant twice that, T 2^-23 sum|x_t| (the terms e_t, e_t^2 are themselves fp32
    values: e_t exactly the subtraction both sides perform, e_t^2 with one more rounding, which
    the factor two covers);
  * max_t |e_t| involves no rounding: it is compared bitwise;
  * f_t = y_t - sum_n phi[t][n] p[n] evaluated in fp32 differs from its float64 value by at most
    eta_t = (N + 1) u sum_n |phi p| + u |f_t| (the dot-product bound in any order, fused or not,
    plus the subtraction's rounding), so f_t^2 moves by at most 2 |f_t| eta_t + eta_t^2.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24


def _kinds(D: int, n_joint: int) -> np.ndarray:
    return (np.arange(D) >= n_joint).astype(np.int64)


def fit_positions64(params32: np.ndarray, phi32: np.ndarray, n_joint: int):
    """(sum_n phi p, sum_n |phi p|) in float64, both [B, T, D]."""
    B, D, N = params32.shape
    p = params32.astype(np.float64)
    ph = phi32.astype(np.float64)[_kinds(D, n_joint)]           # [D, T, N]
    pos = np.einsum("dtn,bdn->btd", ph, p)
    mag = np.einsum("dtn,bdn->btd", np.abs(ph), np.abs(p))
    return pos, mag


def stats(y: np.ndarray, pos32: np.ndarray, params32: np.ndarray, phi32: np.ndarray, w_min: np.ndarray,
          w_max: np.ndarray, n_joint: int) -> dict:
    """The four statistics [B, D] in float64, the clip counts [D * N] and what the tolerances need."""
    assert y.dtype == np.float32 and pos32.dtype == np.float32 and params32.dtype == np.float32
    B, T, D = y.shape
    N = params32.shape[2]
    with np.errstate(invalid="ignore", over="ignore"):
        e = (y - pos32).astype(np.float64)                      # fl32(y - pos), exactly
        fit, mag = fit_positions64(params32, phi32, n_joint)
        f = y.astype(np.float64) - fit
        eta = (N + 1) * U * mag + U * np.abs(f)
        flat = params32.reshape(B, D * N)
        return {
            "sum_e": e.sum(axis=1), "sum_e2": (e * e).sum(axis=1), "max_abs": np.abs(y - pos32).max(axis=1),
            "sum_f2": (f * f).sum(axis=1),
            "sum_abs_e": np.abs(e).sum(axis=1),
            "f2_slack": (2 * np.abs(f) * eta + eta * eta).sum(axis=1),
            "clip_low": (flat < w_min[None, :]).sum(axis=0).astype(np.int64),
            "clip_high": (flat > w_max[None, :]).sum(axis=0).astype(np.int64),
            "T": T,
        }


def tol_sum_e(s: dict) -> np.ndarray:
    return s["T"] * 2.0 ** -23 * s["sum_abs_e"]


def tol_sum_e2(s: dict) -> np.ndarray:
    return s["T"] * 2.0 ** -23 * s["sum_e2"]


def tol_sum_f2(s: dict) -> np.ndarray:
    return s["f2_slack"] + s["T"] * 2.0 ** -23 * s["sum_f2"]


def assert_stats(got: np.ndarray, s: dict) -> None:
    """got [B, D, 4] fp32 against the oracle: the maximum bitwise, the sums within their tolerances;
    where the oracle's value is not finite the result must be the same non-finite value (NaN for NaN)."""
    assert got.dtype == np.float32 and got.shape == s["sum_e"].shape + (4,)
    want_mx = s["max_abs"]
    nan = np.isnan(want_mx)
    assert np.array_equal(np.isnan(got[..., 2]), nan)
    assert np.array_equal(got[..., 2][~nan].view(np.uint32), want_mx[~nan].view(np.uint32)), "max_abs is not bitwise"
    for i, key, tol in ((0, "sum_e", tol_sum_e(s)), (1, "sum_e2", tol_sum_e2(s)), (3, "sum_f2", tol_sum_f2(s))):
        want, g = s[key], got[..., i].astype(np.float64)
        fin = np.isfinite(want)
        with np.errstate(invalid="ignore"):
            err = np.abs(g - want)
            bad = fin & ~(err <= tol)
        assert not bad.any(), (key, float(np.nanmax(np.where(fin, err / np.maximum(tol, 1e-300), 0.0))))
        # a non-finite oracle value: the fp32 sum overflowed or met a NaN as well
        assert not np.isfinite(g[~fin]).any(), key
        both_inf = ~fin & np.isinf(want) & np.isinf(g)
        assert np.array_equal(np.sign(g[both_inf]), np.sign(want[both_inf])), key
