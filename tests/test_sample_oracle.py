"""tests/sample_oracle.py against a brute-force float64 torch composition written the way the warpers
are usually written -- sort descending, cumsum, mask, renormalise, index-order cumsum -- one row and
one tie group at a time, and the stratified-uniform property on the oracle alone."""
import numpy as np
import pytest
import torch

import sample_oracle as SO


def brute_row(l, us, tau, k, p):
    """(kept mask, tokens, logprobs) of one float64 row, group by group."""
    V = l.numel()
    prob = torch.softmax(l / tau, -1)
    vals, _ = torch.sort(l, descending=True, stable=True)
    keep = torch.ones(V, dtype=torch.bool)
    if 1 <= k < V:
        keep = l >= vals[k - 1]
    pk = torch.where(keep, prob, torch.zeros_like(prob))
    pk = pk / pk.sum()
    if p < 1.0:
        mass, chosen = 0.0, []
        for val in torch.unique(l[keep]).flip(0).tolist():           # distinct kept values, largest first
            chosen.append(val)
            mass = float(pk[l >= val].sum())
            if mass >= p:
                break
        keep = keep & (l >= chosen[-1])
    final = torch.where(keep, pk, torch.zeros_like(pk))
    final = final / final.sum()
    c = torch.cumsum(final, -1)
    toks, lps = [], []
    for u in us:
        hit = (c > u) & (final > 0)
        t = int(torch.nonzero(hit)[0]) if hit.any() else int(torch.nonzero(final > 0)[-1])
        toks.append(t)
        lps.append(float(torch.log(final[t])))
    return keep.numpy(), np.array(toks), np.array(lps), c.numpy()


def rows_for(V, seed):
    gen = torch.Generator().manual_seed(seed)
    l = torch.randn((6, V), generator=gen, dtype=torch.float64) * 4.0
    l[1] = torch.round(l[1])                                   # integers: many exact ties
    l[2] = torch.round(l[2] / 4.0)                             # a handful of distinct values
    l[3, torch.rand(V, generator=gen) < 0.5] = float("-inf")
    l[3, 0] = float("-inf")
    l[3, V - 1] = 1.0
    l[4] = 0.25                                                # one tie group
    l[5] = l[5].to(torch.bfloat16).double()
    return l


@pytest.mark.parametrize("V", [2, 3, 17, 256])
@pytest.mark.parametrize("tau", [0.25, 1.0, 3.0])
def test_oracle_equals_the_brute_force_composition(V, tau):
    l = rows_for(V, V)
    us = torch.rand((7, 6), generator=torch.Generator().manual_seed(V + 1), dtype=torch.float64).numpy()
    for k in sorted({0, 1, 2, V - 1, V, V + 5}):
        for p in (1e-6, 0.3, 0.9, 1.0):
            tok, lp, cnt = SO.sample(l.numpy(), us, tau, k, p)
            kept = SO.kept_mask(l.numpy(), tau, k, p)
            for r in range(6):
                bkeep, btok, blp, c = brute_row(l[r], us[:, r].tolist(), tau, k, p)
                assert np.array_equal(kept[r], bkeep), (V, tau, k, p, r)
                assert cnt[r] == bkeep.sum()
                edge = np.abs(c[None, :] - us[:, r][:, None]).min()
                assert edge > 1e-12, "a uniform sits on a CDF edge: choose another seed"
                assert np.array_equal(tok[:, r], btok), (V, tau, k, p, r)
                assert np.abs(lp[:, r] - blp).max() <= 1e-12 * max(1.0, np.abs(blp).max())


def test_named_consequences():
    l = np.array([[0.0, 3.0, 3.0, -np.inf, 1.0, 2.0, 2.0, -np.inf]])
    assert SO.kept_mask(l, 1.0, 1, 1.0)[0].tolist() == [False, True, True, False, False, False, False, False]
    assert SO.kept_mask(l, 1.0, 3, 1.0)[0].tolist() == [False, True, True, False, False, True, True, False]
    assert SO.kept_mask(l, 1.0, 7, 1.0)[0].sum() == 8          # the 7th largest is -inf: the tie keeps both
    assert SO.kept_mask(l, 1.0, 0, 1e-9)[0].tolist() == SO.kept_mask(l, 1.0, 1, 1.0)[0].tolist()
    assert SO.kept_mask(l, 1.0, 8, 1.0)[0].all() and SO.kept_mask(l, 1.0, 0, 1.0)[0].all()
    # u = 0: the lowest kept bin with mass; u just below 1: the highest; -inf is never drawn
    tok, lp, cnt = SO.sample(l, np.array([[0.0], [1.0 - 2.0 ** -53]]), 1.0, 0, 1.0)
    assert tok[:, 0].tolist() == [0, 6] and cnt[0] == 8
    p = SO.probabilities(l)
    assert np.allclose(np.exp(lp[:, 0]), p[0, [0, 6]], rtol=1e-14) and p[0, 3] == 0 and p[0, 7] == 0
    # the log-probability is that of the truncated, renormalised distribution
    tok, lp, cnt = SO.sample(l, np.array([[0.7]]), 2.0, 3, 1.0)
    assert cnt[0] == 4 and tok[0, 0] in (1, 2, 5, 6)
    assert abs(np.exp(lp[0, 0]) - SO.probabilities(l, 2.0, 3, 1.0)[0, tok[0, 0]]) <= 1e-15


@pytest.mark.parametrize("top_p", [1.0, 0.9])
def test_stratified_uniforms_hit_every_bin_within_one(top_p):
    """M identical rows, u_j = (j + 1/2) / M: an interval of length P_v holds M P_v +- 1 grid points."""
    M, V = 4096, 256
    l = (torch.randn(V, generator=torch.Generator().manual_seed(11), dtype=torch.float64) * 4.0).numpy()
    u = (np.arange(M) + 0.5) / M
    tok, _, cnt = SO.sample(np.broadcast_to(l, (M, V)), u[None], 1.0, 0, top_p)
    P = SO.probabilities(l[None], 1.0, 0, top_p)[0]
    counts = np.bincount(tok[0], minlength=V)
    assert np.abs(counts - M * P).max() <= 1.0
    assert (counts[P == 0] == 0).all() and (top_p == 1.0 or (P == 0).any())
