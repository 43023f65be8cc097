"""The float64 oracle of the two-hot cross-entropy (tests/xent_oracle.py) against torch's float64
autograd of ``-(q * log_softmax(l)).sum(-1)`` with a target ``q`` built densely here, independently of
the oracle (torch fp32 ops for the position of a coefficient)."""
import numpy as np
import pytest
import torch

import xent_oracle as XO

IGNORE = -100
TOL = 1e-12


def dense_q(u, V, eps):
    """q [R, V] float64 from positions u [R] float64, built element by element."""
    eps = float(np.float32(eps))
    q = np.full((len(u), V), eps / V)
    for r, ur in enumerate(u):
        i = min(int(np.floor(ur)), V - 2)
        f = ur - i
        q[r, i] += (1.0 - eps) * (1.0 - f)
        q[r, i + 1] += (1.0 - eps) * f
    return q


def torch_reference(l, q, g):
    t = torch.tensor(l, dtype=torch.float64, requires_grad=True)
    out = -(torch.tensor(q) * torch.log_softmax(t, -1)).sum(-1)
    out.backward(torch.tensor(g))
    return out.detach().numpy(), t.grad.numpy()


def token_cases(V):
    """tokens: u = 0, u = V-1 (i = V-2, f = 1), an integer u inside, the ignored one, random ones"""
    gen = np.random.default_rng(V)
    return np.concatenate([[0, V - 1, V // 2, IGNORE], gen.integers(0, V, 6)]).astype(np.int64)


def coeff_cases(V):
    """coefficients: u = 0, u = V-1, an integer u, just outside [-1, 1] and far outside, NaN, random ones"""
    one = np.float32(1.0)
    k = (V - 1) // 2
    inside = np.float32(2.0 * k / (V - 1) - 1.0) if (V - 1) % 2 == 0 else np.float32(-1.0)    # x = 0: u = (V-1)/2
    gen = np.random.default_rng(V + 1)
    return np.concatenate([[-one, one, inside, np.nextafter(one, np.float32(2)), np.nextafter(-one, np.float32(-2)),
                            np.float32(1.5), np.float32(-1.5), np.float32(np.inf), np.float32(np.nan)],
                           gen.uniform(-1, 1, 6).astype(np.float32)]).astype(np.float32)


@pytest.mark.parametrize("kind", ["tokens", "coefficients"])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("V", [2, 3, 257])
def test_oracle_equals_torch_float64_autograd(V, eps, kind):
    gen = np.random.default_rng(7 * V + int(eps * 10))
    if kind == "tokens":
        t = token_cases(V)
        i, f, k = XO.target_from_tokens(t, V, ignore_index=IGNORE)
        keep = t != IGNORE
        u = t[keep].astype(np.float64)
        assert (i[1], f[1]) == (V - 2, 1.0) and (i[0], f[0]) == (0, 0.0)
    else:
        x = coeff_cases(V)
        i, f, k = XO.target_from_coeffs(x, V)
        keep = ~np.isnan(x)
        # the position with torch's fp32 arithmetic: an independent replica of the three roundings
        xt = torch.tensor(x[keep], dtype=torch.float32)
        ut = (((xt + 1.0) * 0.5) * float(V - 1)).clamp(0.0, float(V - 1))
        assert ut.dtype == torch.float32
        u = ut.double().numpy()
        assert (i[0], f[0]) == (0, 0.0) and (i[1], f[1]) == (V - 2, 1.0)          # x = -1, x = 1
        assert f[2] == 0.0 or V == 2                                              # an integer u
        assert (i[3], f[3]) == (V - 2, 1.0) and (i[4], f[4]) == (0, 0.0)          # just outside: clamped
        assert (i[7], f[7]) == (V - 2, 1.0)                                       # +inf: clamped
    assert np.array_equal(k == XO.IGNORED, ~keep) and not (k == XO.OUT_OF_RANGE).any()
    R = len(k)
    l = gen.standard_normal((R, V)) * 4.0
    g = gen.standard_normal(R)
    got_loss, got_grad = XO.loss(l, i, f, k, eps), XO.grad(l, i, f, k, g, eps)
    want_loss, want_grad = torch_reference(l[keep], dense_q(u, V, eps), g[keep])
    assert np.abs(got_loss[keep] - want_loss).max() <= TOL * max(1.0, np.abs(want_loss).max())
    assert np.abs(got_grad[keep] - want_grad).max() <= TOL * max(1.0, np.abs(want_grad).max())
    assert np.abs(XO.dense_target(i, f, V, eps)[keep] - dense_q(u, V, eps)).max() <= 1e-16
    # ignored rows: exactly 0, every gradient element
    assert (got_loss[~keep] == 0.0).all() and (got_grad[~keep] == 0.0).all() and (~keep).any()


def test_tokens_with_an_offset_and_out_of_range():
    V, off = 5, 1000
    t = np.array([off, off + V - 1, off - 1, off + V, 3, IGNORE], dtype=np.int64)
    i, f, k = XO.target_from_tokens(t, V, tok_offset=off, ignore_index=IGNORE)
    assert list(k) == [XO.TARGET, XO.TARGET, XO.OUT_OF_RANGE, XO.OUT_OF_RANGE, XO.OUT_OF_RANGE, XO.IGNORED]
    assert list(i[:2]) == [0, V - 2] and list(f[:2]) == [0.0, 1.0]
    l = np.random.default_rng(0).standard_normal((6, V))
    out, gr = XO.loss(l, i, f, k), XO.grad(l, i, f, k, np.ones(6))
    assert np.isfinite(out[:2]).all() and np.isnan(out[2:5]).all() and out[5] == 0.0
    assert np.isnan(gr[2:5]).all() and np.isfinite(gr[:2]).all() and (gr[5] == 0.0).all()
    # an ignore_index inside the token range is still ignored: the comparison is on the token as given
    assert XO.target_from_tokens(np.array([off + 2]), V, off, off + 2)[2][0] == XO.IGNORED


def test_zero_weights_are_selects():
    """-inf under a zero weight: finite loss, zero gradient there; under a positive weight (f > 0, or
    eps > 0): +inf loss."""
    V = 6
    l = np.array([0.5, -np.inf, 1.0, -0.25, -np.inf, 2.0])
    i, f, k = XO.target_from_tokens(np.array([0]), V)            # bins 0 and 1, f = 0: bin 1 has weight 0
    out = XO.loss(l[None], i, f, k, 0.0)
    assert np.isfinite(out[0]) and abs(out[0] - (np.log(np.exp(l - 2.0).sum()) + 1.5)) <= TOL
    gr = XO.grad(l[None], i, f, k, np.ones(1), 0.0)
    assert gr[0, 1] == 0.0 and gr[0, 4] == 0.0 and np.isfinite(gr).all()
    assert XO.loss(l[None], i, f, k, 0.1)[0] == np.inf           # smoothing puts weight on every bin
    i, f, k = XO.target_from_coeffs(np.array([-0.8], dtype=np.float32), V)     # u = 0.5: both bins weigh
    assert i[0] == 0 and 0.0 < f[0] < 1.0 and XO.loss(l[None], i, f, k, 0.0)[0] == np.inf
    i, f, k = XO.target_from_tokens(np.array([V - 1]), V)        # i = V-2 = 4 (-inf) with weight 1-f = 0
    assert (i[0], f[0]) == (4, 1.0) and np.isfinite(XO.loss(l[None], i, f, k, 0.0)[0])


def test_rows_and_argmax_ties():
    l = np.array([[1.0, 3.0, 3.0, -2.0], [0.0, 0.0, 0.0, 0.0]])
    m, s, amax = XO.rows(l)
    assert list(amax) == [1, 0] and list(m) == [3.0, 0.0] and s[1] == 4.0


def test_position_is_rounded_in_fp32_in_the_stated_order():
    """A coefficient where (x + 1) * 0.5 * (V-1) in float64 and the fp32 chain pick different f."""
    V = 257
    x = np.float32(0.3337)
    u32 = XO.position_fp32(x, V)
    assert u32.dtype == np.float32
    want = np.float32(np.float32(np.float32(x + np.float32(1)) * np.float32(0.5)) * np.float32(V - 1))
    assert u32 == want
    i, f, _ = XO.target_from_coeffs(x, V)
    assert i == int(np.floor(want)) and f == float(want) - i
