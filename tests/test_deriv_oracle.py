"""The float64 derivative oracle (tests/deriv_oracle.py) against its goldens and its own
properties; no GPU.  The goldens (tests/golden/gen_deriv_goldens.py) were cross-checked against
scipy's BSpline.derivative and the reference's get_traj_vel when they were written."""
import numpy as np
import pytest

from conftest import load_json, load_npz
import deriv_oracle as O

TOL = load_json("deriv_tolerances.json")
CASES = sorted(TOL)
TWO_PI = float(np.float32(2 * np.pi))


def case_config(name):
    c = TOL[name]["config"]
    return dict(degree=c["degree"], N=c["N"], D=c["D"], grippers=sorted(c.get("grippers", [])),
                ic=c.get("ic", 0), ec=c.get("ec", 0), duration=c.get("duration", 2 * np.pi),
                init_p=bool(c.get("init_p")))


def decoded_params(g, cfg):
    """[B, D, N] fp32 params of the golden tokens (discrete_to_continuous, beast/utils.py:20-25)
    in the tokenizer's DoF order (joints, then grippers), init_p applied."""
    D, N = cfg["D"], cfg["N"]
    joint = [d for d in range(D) if d not in cfg["grippers"]]
    tok = g["tokens"].reshape(-1, N, D).transpose(0, 2, 1).astype(np.float32)      # (n d) -> [B, D, N]
    lo, hi = g["w_min"].reshape(D, N), g["w_max"].reshape(D, N)
    w = np.clip((tok / np.float32(255)) * (hi - lo) + lo, lo, hi).astype(np.float32)
    if "init_p" in g:
        w[:, : len(joint), 0] = g["init_p"][:, joint]
    return w, joint


@pytest.mark.parametrize("name", CASES)
def test_oracle_reproduces_goldens(name):
    g, cfg = load_npz(f"deriv_{name}.npz"), case_config(name)
    w, joint = decoded_params(g, cfg)
    dj = len(joint)
    ctrl = O.control_points(w[:, :dj].astype(np.float64), cfg["ic"], cfg["ec"], g.get("cond_params_init"),
                            g.get("cond_params_end"))
    for order in range(3):
        got = O.trajectory(g["times"], cfg["duration"], cfg["degree"], ctrl, order,
                           init_pos=g.get("cond_init_pos") if cfg["ic"] else None)
        want = g[f"oracle{order}"]
        assert want.dtype == np.float64
        np.testing.assert_allclose(got, want[..., joint], rtol=1e-13, atol=1e-13 * max(1.0, np.abs(want).max()))
        if order:
            assert not want[..., cfg["grippers"]].any()          # degree 0: derivatives are 0
    # the reference's own fp32 outputs sit at fp32 rounding distance from the oracle
    assert O.rel_err(g["ref_pos"], g["oracle0"]) <= 1e-5
    assert O.rel_err(g["ref_vel"], g["oracle1"]) == pytest.approx(TOL[name]["vel_ref_err"], rel=1e-9)


@pytest.mark.parametrize("degree,n_ctrl", [(1, 4), (2, 4), (3, 12), (4, 10), (4, 13), (8, 16)])
def test_first_derivative_matches_central_differences(degree, n_ctrl):
    """Order 1 against central differences of order 0 on a 4,001-point grid: the error of a
    central difference is h^2/6 max|f'''| (piecewise), and across a knot, where f''' jumps (or,
    for degree <= 2, a lower derivative does), it is bounded by h/2 (or 1/2) of that jump --
    so only points at least h from every knot are compared, with the O(h^2) bound."""
    tau = 4.0
    t = np.linspace(0.0, tau, 4001)
    h = t[1] - t[0]
    b0 = O.deriv_basis(t, tau, degree, n_ctrl, 0)
    b1 = O.deriv_basis(t, tau, degree, n_ctrl, 1)
    cd = (b0[2:] - b0[:-2]) / (2 * h)
    kv = np.unique(O.knots(degree, n_ctrl)) * tau
    away = np.abs(t[1:-1, None] - kv[None, :]).min(axis=1) > 1.5 * h
    assert away.sum() > 3000
    if degree >= 3:
        f3 = _db3_bound(degree, n_ctrl, tau)
    else:
        f3 = 0.0                                                  # piecewise degree <= 2: exact
    err = np.abs(cd - b1[1:-1])[away].max()
    assert err <= h * h / 6 * f3 * 1.01 + 1e-10, (err, h * h / 6 * f3)
    assert np.abs(b1).max() > 0


def _db3_bound(degree, n_ctrl, tau):
    """max over the basis functions of |d^3 B / dt^3|, from three applications of the derivative
    rule with |B| <= 1: each multiplies by at most 2 k / (smallest non-zero knot difference of
    that level) / tau."""
    kv = O.knots(degree, n_ctrl)
    bound = 1.0
    for k in (degree, degree - 1, degree - 2):
        d = kv[k:] - kv[:-k]
        bound *= 2 * k / d[d > 0].min() / tau
    return bound


@pytest.mark.parametrize("degree,n_ctrl", [(1, 2), (1, 4), (2, 4), (3, 12), (4, 10), (4, 16), (8, 16)])
def test_partition_of_unity_differentiates_to_zero(degree, n_ctrl):
    kv = np.unique(O.knots(degree, n_ctrl))
    t = np.concatenate([np.linspace(-0.3, 2.3, 257), kv * 2.0, [0.0, 2.0]])
    assert np.abs(O.deriv_basis(t, 2.0, degree, n_ctrl, 0).sum(-1) - 1).max() <= 1e-12
    for order in (1, 2):
        d = O.deriv_basis(t, 2.0, degree, n_ctrl, order)
        scale = max(1.0, np.abs(d).max())
        assert np.abs(d.sum(-1)).max() <= 1e-12 * scale, (order, np.abs(d.sum(-1)).max())


def test_order_above_degree_and_knot_rule():
    t = np.array([0.0, 0.5, 1.0, 1.5, 2.0])
    assert not O.deriv_basis(t, 2.0, 1, 4, 2).any()
    assert not O.deriv_basis(t, 2.0, 0, 4, 1).any()
    # degree 1, 3 control points: knots 0, 0, .5, 1, 1; the slope of B_0 is -2/tau on [0, .5) and 0
    # on [.5, 1]: at the knot the right-continuous value, at the end the last span's
    d = O.deriv_basis(np.array([0.0, 0.999, 1.0, 2.0]), 2.0, 1, 3, 1)
    np.testing.assert_allclose(d[:, 0], [-1.0, -1.0, 0.0, 0.0])
    np.testing.assert_allclose(d[:, 2], [0.0, 0.0, 1.0, 1.0])
    # outside [0, tau] the phase is clipped first
    np.testing.assert_array_equal(O.deriv_basis(np.array([-3.0, 7.0]), 2.0, 4, 10, 1),
                                  O.deriv_basis(np.array([0.0, 2.0]), 2.0, 4, 10, 1))


def test_float32_mode_is_single_precision():
    t = np.linspace(-0.1, 6.4, 77, dtype=np.float32)
    for order in range(3):
        a = O.deriv_basis(t, TWO_PI, 4, 10, order, dtype=np.float32)
        b = O.deriv_basis(t, TWO_PI, 4, 10, order)
        assert a.dtype == np.float32 and b.dtype == np.float64
        assert 0 < np.abs(a - b).max() <= 64 * 2.0 ** -24 * np.abs(b).max()
