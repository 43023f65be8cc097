"""The float64 oracle of the reconstruct backward (tests/deriv_bwd_oracle.py) against
torch.autograd through a float64 CPU composition clamp -> denormalise -> einsum; no GPU."""
import itertools

import numpy as np
import pytest
import torch

import deriv_bwd_oracle as O

ORDER_SETS = [s for r in (1, 2, 3) for s in itertools.combinations((0, 1, 2), r)]


def make_inputs(B, T, D, nj, N, orders, *, ndo=None, per_row=False, seed=0):
    """Random fp32 inputs of one backward: the slabs of the orders without a gradient (and the
    gripper slabs of orders 1, 2) poisoned with NaN; ntokens in [-1.2, 1.2] with exact +-1, their
    outward neighbours and NaN planted; bounds on a 1/64 grid, so w_max - w_min is exact in fp32;
    dof_dst a random choice of D distinct columns of num_dof_out."""
    rng = np.random.default_rng([seed, B, T, D, N])
    f32 = np.float32
    ndo = ndo or D
    x = rng.uniform(-1.2, 1.2, size=(B, N, D)).astype(f32)
    flat = x.reshape(-1)
    special = [f32(1), f32(-1), np.nextafter(f32(1), f32(2)), np.nextafter(f32(-1), f32(-2)), f32(np.nan)]
    for i, v in zip(rng.permutation(flat.size)[:len(special)], special):
        flat[i] = v
    lo = (-rng.integers(8, 128, (D, N)) / 64).astype(f32)
    hi = (lo + rng.integers(8, 192, (D, N)) / 64).astype(f32)
    basis = rng.standard_normal(((B,) if per_row else ()) + (3, 2, T, N)).astype(f32)
    for o in range(3):
        if o not in orders:
            basis[..., o, :, :, :] = np.nan
        elif o:
            basis[..., o, 1, :, :] = np.nan
    grads = [rng.standard_normal((B, T, ndo)).astype(f32) if o in orders else None for o in range(3)]
    dst = rng.permutation(ndo)[:D].astype(np.int32)
    ip_src = rng.permutation(D + 3)[:D].astype(np.int32)
    return dict(x=x, lo=lo, hi=hi, basis=basis, grads=grads, dst=dst, ip_src=ip_src, nj=nj, ndo=ndo)


def autograd_reference(c, init_p=False):
    """d/dx (and d/d init_p) of sum_o <G_o, out_o> through clamp -> denormalise -> einsum in
    float64 on the CPU; NaN tokens are replaced by 2 (outside the clamp: gradient 0 either way)."""
    x = torch.from_numpy(np.nan_to_num(c["x"], nan=2.0).astype(np.float64)).requires_grad_()
    B, N, D = x.shape
    lo, hi = (torch.from_numpy(c[k].astype(np.float64)) for k in ("lo", "hi"))
    ip = torch.zeros((B, D + 3), dtype=torch.float64, requires_grad=True)
    w = ((x.clamp(-1, 1) + 1) / 2).permute(0, 2, 1) * (hi - lo) + lo                    # [B, D, N]
    if init_p:
        w0 = torch.cat([ip[:, torch.from_numpy(c["ip_src"][:c["nj"]].astype(np.int64))], w[:, c["nj"]:, 0]], dim=1)
        w = torch.cat([w0[:, :, None], w[:, :, 1:]], dim=2)
    basis = torch.from_numpy(np.nan_to_num(c["basis"], nan=0.0).astype(np.float64))
    loss = 0
    for o, g in enumerate(c["grads"]):
        if g is None:
            continue
        kinds = torch.tensor([0 if d < c["nj"] else 1 for d in range(D)])
        ph = basis[..., o, :, :, :][..., kinds, :, :]                                   # [(B,) D, T, N]
        out = torch.einsum("bdtn,bdn->btd" if ph.dim() == 4 else "dtn,bdn->btd", ph, w)
        if o:
            out = out * (kinds == 0)                                                    # gripper derivatives: 0
        full = torch.zeros((B, out.shape[1], c["ndo"]), dtype=torch.float64)
        full[:, :, torch.from_numpy(c["dst"].astype(np.int64))] = out
        loss = loss + (full * torch.from_numpy(g.astype(np.float64))).sum()
    gx, gip = torch.autograd.grad(loss, (x, ip), allow_unused=True)
    return gx.numpy(), (gip.numpy() if gip is not None else np.zeros((B, D + 3)))


@pytest.mark.parametrize("orders", ORDER_SETS)
@pytest.mark.parametrize("per_row", [False, True])
def test_oracle_matches_autograd(orders, per_row):
    c = make_inputs(5, 7, 6, 4, 5, orders, ndo=9, per_row=per_row)
    r = O.backward(c["grads"], c["basis"], c["lo"], c["hi"], c["x"], c["dst"], c["nj"])
    want, _ = autograd_reference(c)
    assert r.terms == len(orders) * 7
    np.testing.assert_allclose(r.grad_ntokens, want, rtol=1e-12, atol=1e-12)
    assert np.isfinite(r.grad_ntokens).all()            # the poisoned slabs were never read


def test_mask_is_inclusive_and_a_select():
    c = make_inputs(4, 3, 3, 2, 4, (0, 2))
    x = c["x"]
    x[0, 0, 0], x[0, 1, 0], x[0, 2, 0], x[0, 3, 0] = 1, -1, np.nextafter(np.float32(1), np.float32(2)), np.nan
    x[1, 0, 1] = np.nextafter(np.float32(-1), np.float32(-2))
    c["grads"][0][0, :, c["dst"][0]] = np.inf           # S[0][0][:] is not finite
    r = O.backward(c["grads"], c["basis"], c["lo"], c["hi"], x, c["dst"], c["nj"])
    assert not np.isfinite(r.S[0, 0]).any()
    assert not np.isfinite(r.grad_ntokens[0, :2, 0]).any()          # +-1 pass
    assert (r.grad_ntokens[0, 2:, 0] == 0).all() and r.grad_ntokens[1, 0, 1] == 0
    assert np.array_equal(r.scale, (0.5 * (c["hi"].astype(np.float64) - c["lo"])))


@pytest.mark.parametrize("nj", [0, 2, 4])
def test_init_p_rule(nj):
    c = make_inputs(3, 5, 4, nj, 3, (0, 1, 2), ndo=6)
    r = O.backward(c["grads"], c["basis"], c["lo"], c["hi"], c["x"], c["dst"], nj, init_p_src=c["ip_src"],
                   init_p_width=7)
    want, want_ip = autograd_reference(c, init_p=True)
    np.testing.assert_allclose(r.grad_ntokens, want, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(r.grad_init_p, want_ip, rtol=1e-12, atol=1e-12)
    assert (r.grad_ntokens[:, 0, :nj] == 0).all()
    untouched = sorted(set(range(7)) - set(c["ip_src"][:nj].tolist()))
    assert not r.grad_init_p[:, untouched].any()
    # without a grad_init_p request the token gradient is the same and nothing else is returned
    r2 = O.backward(c["grads"], c["basis"], c["lo"], c["hi"], c["x"], c["dst"], nj, init_p_src=c["ip_src"])
    assert r2.grad_init_p is None and np.array_equal(r2.grad_ntokens, r.grad_ntokens)


def test_unnamed_columns_contribute_nothing():
    c = make_inputs(3, 4, 3, 3, 4, (0, 1), ndo=8)
    r = O.backward(c["grads"], c["basis"], c["lo"], c["hi"], c["x"], c["dst"], c["nj"])
    unnamed = sorted(set(range(8)) - set(c["dst"].tolist()))
    for g in c["grads"]:
        if g is not None:
            g[:, :, unnamed] = np.nan
    r2 = O.backward(c["grads"], c["basis"], c["lo"], c["hi"], c["x"], c["dst"], c["nj"])
    assert np.array_equal(r.grad_ntokens, r2.grad_ntokens)
    assert np.array_equal(O.bound(r), O.bound(r2)) and O.bound(r).shape == r.grad_ntokens.shape
