"""tests/score_oracle.py against torch's float64 composition and its autograd: ``masked_fill(-inf)``
-> ``log_softmax`` -> gather / entropy / KL on small rows, with and without a truncation, with -inf
logits, ignored tokens and tokens outside the kept set.  No GPU."""
import numpy as np
import pytest
import torch

import sample_oracle as SO
import score_oracle as SC

TOL = 1e-12


def rows(seed, lead=(4, 3), V=7, neg_inf=False):
    rng = np.random.default_rng(seed)
    l = rng.normal(size=lead + (V,)) * 3.0
    if neg_inf:
        l[..., 2] = -np.inf
        l[0, 0, 5] = -np.inf
    return l


def torch_all(l, ref, kept, tau, tok, part, g_lp, g_h, g_kl):
    """(logprob [S, ...], H, KL, grad) of torch's composition; the draws in ``part`` carry g_lp."""
    t = torch.tensor(l, requires_grad=True)
    keep = torch.tensor(kept)
    lp = torch.log_softmax((t / tau).masked_fill(~keep, -np.inf), -1)
    pi = lp.exp()
    safe = lp.masked_fill(lp == -np.inf, 0.0)
    H = -(pi * safe).sum(-1)
    lr = torch.log_softmax(torch.tensor(ref) / tau, -1)
    # pi == 0 terms are exactly 0; log rho == -inf under pi > 0 gives +inf
    KL = (pi * (safe - lr.masked_fill(pi == 0, 0.0))).sum(-1)
    S = tok.shape[0]
    idx = torch.tensor(tok)
    got = torch.stack([lp.gather(-1, idx[s][..., None])[..., 0] for s in range(S)])
    loss = (torch.where(torch.tensor(part), got, torch.zeros_like(got)) * torch.tensor(g_lp)).sum() \
        + (H * torch.tensor(g_h)).sum() + (KL * torch.tensor(g_kl)).sum()
    loss.backward()
    return got.detach().numpy(), H.detach().numpy(), KL.detach().numpy(), t.grad.numpy()


@pytest.mark.parametrize("tau", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("trunc", [(0, 1.0), (3, 1.0), (0, 0.7), (5, 0.5), (1, 1.0)])
@pytest.mark.parametrize("neg_inf", [False, True])
def test_values_and_gradient_match_torch_float64(tau, trunc, neg_inf):
    top_k, top_p = trunc
    l = rows(1, neg_inf=neg_inf)
    ref = rows(2)
    V, S, off = l.shape[-1], 3, 11
    kept = SO.kept_mask(l, tau, top_k, top_p)
    rng = np.random.default_rng(3)
    tok = rng.integers(0, V, size=(S,) + l.shape[:-1])
    tok[0, 0, 0] = int(np.argmax(l[0, 0]))                    # one token surely kept
    tokens = tok + off
    tokens[1, 1, 1] = SC.IGNORE
    tokens[2, 2, 2] = SC.IGNORE
    g_lp = rng.normal(size=tok.shape)
    g_h, g_kl = rng.normal(size=l.shape[:-1]), rng.normal(size=l.shape[:-1])

    want_lp, part = SC.logprob(l, kept, tokens, tau, off)
    if top_k or top_p < 1.0 or neg_inf:
        assert np.isneginf(want_lp).any(), "the case must hold a token outside the kept set"
    assert part.any() and not part[1, 1, 1] and not part[2, 2, 2]
    assert want_lp[1, 1, 1] == 0.0 and want_lp[2, 2, 2] == 0.0
    assert not part[np.isneginf(want_lp)].any()
    got_lp, got_h, got_kl, got_grad = torch_all(l, ref, kept, tau, tok, part, g_lp, g_h, g_kl)
    live = tokens != SC.IGNORE
    assert np.array_equal(np.isneginf(want_lp[live]), np.isneginf(got_lp[live]))
    fin = live & np.isfinite(want_lp)
    assert np.abs(want_lp[fin] - got_lp[fin]).max() <= TOL
    assert np.abs(SC.entropy(l, kept, tau) - got_h).max() <= TOL
    assert np.abs(SC.kl(l, ref, kept, tau) - got_kl).max() <= TOL
    want_grad = SC.grad(l, kept, tau, tokens, g_lp, g_h, g_kl, ref, off)
    assert np.isfinite(want_grad).all()
    assert np.abs(want_grad - got_grad).max() <= TOL
    assert not want_grad[~kept].any(), "outside the kept set the gradient is exactly 0"
    assert not want_grad[np.isneginf(l)].any(), "a -inf logit has gradient exactly 0"
    # each upstream gradient alone, too: the three parts add up
    parts = SC.grad(l, kept, tau, tokens, g_lp, None, None, None, off) \
        + SC.grad(l, kept, tau, None, None, g_h) + SC.grad(l, kept, tau, None, None, None, g_kl, ref)
    assert np.abs(parts - want_grad).max() <= TOL


def test_special_values():
    l = np.array([[0.0, 1.0, -np.inf, 2.0], [5.0, 5.0, 5.0, 5.0]])
    kept = np.array([[False, True, True, True], [True, True, True, True]])
    lp, pi = SC.log_pi(l, kept, 1.0)
    assert lp[0, 0] == -np.inf and lp[0, 2] == -np.inf and pi[0, 0] == 0.0 and pi[0, 2] == 0.0
    assert abs(pi[0].sum() - 1.0) <= TOL and np.abs(lp[1] + np.log(4.0)).max() <= TOL
    assert abs(SC.entropy(l, kept)[1] - np.log(4.0)) <= TOL
    # rho_v == 0 < pi_v: +inf; rho_v == 0 == pi_v: nothing
    ref = np.array([[0.0, 0.0, -np.inf, 0.0], [0.0, -np.inf, 0.0, 0.0]])
    d = SC.kl(l, ref, kept)
    assert np.isfinite(d[0]) and d[1] == np.inf
    # tokens: ignored, out of range on both sides, outside the kept set, on a -inf logit
    tokens = np.array([[10, SC.IGNORE], [14, 9], [12, 13]])
    got, part = SC.logprob(l, kept, tokens, 1.0, 10)
    assert got[0, 0] == -np.inf and got[0, 1] == 0.0 and np.isnan(got[1, 0]) and np.isnan(got[1, 1])
    assert got[2, 0] == -np.inf and abs(got[2, 1] + np.log(4.0)) <= TOL
    assert part.tolist() == [[False, False], [False, False], [False, True]]
    g = SC.grad(l, kept, 1.0, tokens, np.ones((3, 2)), tok_offset=10)
    assert np.isnan(g).all()                                    # both rows hold an out-of-range token
    # top_k = 1: one bin, logprob 0, H 0, no gradient from g_s
    one = np.array([[False, False, False, True]])
    got, _ = SC.logprob(l[:1], one, np.array([[3]]))
    assert got[0, 0] == 0.0 and SC.entropy(l[:1], one)[0] == 0.0
    assert not SC.grad(l[:1], one, 1.0, np.array([[3]]), np.ones((1, 1))).any()
