"""tests/logits_oracle.py against torch's float64 autograd of softmax(l / tau) . x (no GPU needed)."""
import numpy as np
import pytest
import torch

import logits_oracle as LO

VS = (2, 255, 256, 257, 1000)
TAUS = (0.7, 1.0, 2.5)


def rows(V, seed, n=6):
    """n rows of randn * 4; the last one is half -inf."""
    rng = np.random.default_rng(seed)
    l = rng.standard_normal((n, V)) * 4.0
    l[-1, rng.permutation(V)[: V // 2]] = -np.inf
    return l


@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("V", VS)
def test_oracle_agrees_with_torch_float64_autograd(V, tau):
    l = rows(V, seed=V)
    g = np.random.default_rng(V + 1).standard_normal(l.shape[0])
    t = torch.tensor(l, dtype=torch.float64, requires_grad=True)
    x = torch.tensor(LO.bins(V))
    mean_t = (torch.softmax(t / tau, -1) * x).sum(-1)
    mean_t.backward(torch.tensor(g))
    mean, amax, stats = LO.expect(l, tau)
    gl = LO.grad(l, g, tau)
    assert np.abs(mean - mean_t.detach().numpy()).max() <= 4e-15
    scale = np.abs(t.grad.numpy()).max()
    assert np.abs(gl - t.grad.numpy()).max() <= 4e-15 * max(scale, 1.0)
    # a -inf entry: probability and gradient exactly 0, everything else finite
    dead = np.isneginf(l)
    assert dead.any() and np.all(gl[dead] == 0.0) and np.all(np.isfinite(gl))
    assert np.all(np.isfinite(mean)) and np.all(np.abs(mean) <= 1.0)
    assert np.allclose(stats[:, 0], (l / tau).max(-1), rtol=0, atol=0)
    assert np.array_equal(amax, np.argmax(l, -1))


@pytest.mark.parametrize("V", VS)
def test_peaked_rows_give_the_bin_value(V):
    rng = np.random.default_rng(V)
    l = rng.standard_normal((9, V))
    hot = rng.integers(0, V, 9)
    hot[:2] = (0, V - 1)                                   # both ends of the range
    l[np.arange(9), hot] += 60.0
    mean, amax, _ = LO.expect(l, 1.0)
    assert np.array_equal(amax, hot)
    # the other bins hold at most V exp(-50) of the mass (|randn| < 5 here); 2^-50: float64 rounding
    assert np.abs(l).max() < 65.0
    assert np.abs(mean - LO.bins(V)[hot]).max() <= 2.0 ** -50 + 2 * V * np.exp(-50.0)
    assert mean[0] >= -1.0 and mean[1] <= 1.0


def test_argmax_takes_the_lowest_index_on_ties():
    l = np.zeros((3, 7))
    l[1, [2, 5]] = 1.0
    l[2, [6, 3]] = 2.0
    assert LO.expect(l)[1].tolist() == [0, 2, 3]
    assert LO.expect(l)[1].dtype == np.int64


def test_bins_span_the_normalised_range():
    for V in VS:
        x = LO.bins(V)
        assert x[0] == -1.0 and x[-1] == 1.0 and np.all(np.diff(x) > 0)
        assert np.allclose(x, -x[::-1], rtol=0, atol=1e-15)


def test_gradient_of_a_peaked_row_keeps_its_relative_accuracy():
    """p_0 = e^-37.6: the float64 mean rounds to x_1 = 1 and ``bins - mean`` would give bin 1 a zero
    gradient; measured from the maximum's bin both entries keep 2 p_0 g / tau, with opposite signs."""
    l, tau, g = np.array([[-1.2109375, 8.1875]]), 0.25, np.array([0.5])
    gl = LO.grad(l, g, tau)[0]
    p0 = np.exp((l[0, 0] - l[0, 1]) / tau)
    assert LO.expect(l, tau)[0][0] == 1.0
    assert gl[1] > 0 and gl[0] == -gl[1]
    assert abs(gl[1] - 2 * p0 * g[0] / tau) <= 1e-15 * gl[1]


def test_gradient_is_orthogonal_to_a_constant_shift():
    """softmax is shift-invariant: every row of grad_logits sums to 0."""
    l = rows(256, seed=1)
    gl = LO.grad(l, np.ones(l.shape[0]), 0.7)
    assert np.abs(gl.sum(-1)).max() <= 1e-15
