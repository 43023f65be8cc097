"""tests/roundtrip_oracle.py on the reference goldens (no GPU): its batch means are the means taken
directly from the reference's positions, its clip counts are the direct comparison, and a plain
fp32 numpy evaluation of the four statistics keeps within the tolerances the GPU kernel is held to."""
import numpy as np
import pytest

import roundtrip_oracle as R

F32 = np.float32


def _case(g):
    order = np.concatenate([g["joint_indices"], g["gripper_indices"]]).astype(np.int64)
    nj = len(g["joint_indices"])
    B, T, D = g["x"].shape
    N = g["phi_joint"].shape[1]
    phi = np.zeros((2, T, N), dtype=F32)
    phi[0] = g["phi_joint"]
    if "phi_grip" in g:
        phi[1] = g["phi_grip"]
    y = np.ascontiguousarray(g["x"][..., order])
    pos = np.ascontiguousarray(g["pos"][..., order])
    return y, pos, g["params"].reshape(B, D, N), phi, g["w_min"], g["w_max"], nj


@pytest.mark.parametrize("k", ["k1", "k2", "k3"])
def test_oracle_on_goldens(golden, k):
    g = golden[k]
    y, pos, params, phi, lo, hi, nj = _case(g)
    B, T, D = y.shape
    s = R.stats(y, pos, params, phi, lo, hi, nj)
    # the batch means are compute_reconstruction_error's, taken directly from the reference positions
    # (the reference subtracts in fp32; only the means are taken in float64 here)
    err = (g["x"] - g["pos"]).astype(np.float64)
    assert np.isclose(s["sum_e2"].sum() / (B * T * D), np.mean(err ** 2), rtol=1e-12, atol=0)
    assert np.isclose(s["sum_e"].sum() / (B * T * D), np.mean(err), rtol=1e-9, atol=1e-15)
    assert np.array_equal(s["max_abs"], np.abs(y - pos).max(axis=1))
    # quantisation only adds to the fit's error on these bounds (1 % / 99 % quantiles, V = 256)
    assert (s["sum_f2"] >= 0).all() and s["sum_f2"].sum() <= s["sum_e2"].sum()
    flat = g["params"]
    assert np.array_equal(s["clip_low"], (flat < lo).sum(0)) and np.array_equal(s["clip_high"], (flat > hi).sum(0))
    assert s["clip_low"].sum() > 0 and s["clip_high"].sum() > 0
    assert s["clip_low"].max() <= B and s["clip_low"].shape == (D * params.shape[2],)

    # a plain fp32 evaluation: sequential fp32 sums over t, an fp32 dot product over n
    e = y - pos
    got = np.zeros((B, D, 4), dtype=F32)
    fit = np.zeros_like(y)
    kinds = (np.arange(D) >= nj).astype(int)
    for n in range(params.shape[2]):
        fit += phi[kinds][:, :, n].T[None] * params[:, None, :, n]
    f = y - fit
    for t in range(T):
        got[..., 0] += e[:, t]
        got[..., 1] += e[:, t] * e[:, t]
        got[..., 2] = np.maximum(got[..., 2], np.abs(e[:, t]))
        got[..., 3] += f[:, t] * f[:, t]
    assert got.dtype == F32 and fit.dtype == F32
    R.assert_stats(got, s)
    # ... and the tolerances are tight enough to notice a wrong sample: one e_t off by 1e-3
    worse = got.copy()
    worse[0, 0, 0] += F32(1e-3)
    with pytest.raises(AssertionError):
        R.assert_stats(worse, s)
    worse = got.copy()
    worse[0, 0, 2] = np.nextafter(worse[0, 0, 2], F32(np.inf))
    with pytest.raises(AssertionError):
        R.assert_stats(worse, s)


def test_non_finite_samples():
    """A NaN sample makes its DoF's statistics NaN in the oracle, an inf sample infinite or NaN."""
    rng = np.random.default_rng(0)
    y = rng.normal(size=(3, 8, 2)).astype(F32)
    pos = (y + rng.normal(scale=1e-2, size=y.shape)).astype(F32)
    params = rng.normal(size=(3, 2, 4)).astype(F32)
    phi = np.abs(rng.normal(size=(2, 8, 4))).astype(F32)
    y[1, 3, 0] = np.nan
    y[2, 5, 1] = np.inf
    s = R.stats(y, pos, params, phi, np.full(8, -1, F32), np.full(8, 1, F32), 1)
    for key in ("sum_e", "sum_e2", "max_abs", "sum_f2"):
        assert np.isnan(s[key][1, 0]) and np.isinf(s[key][2, 1])
        fin = np.ones((3, 2), bool)
        fin[1, 0] = fin[2, 1] = False
        assert np.isfinite(s[key][fin]).all()
    got = np.stack([s["sum_e"], s["sum_e2"], s["max_abs"], s["sum_f2"]], axis=-1).astype(F32)
    R.assert_stats(got, s)
