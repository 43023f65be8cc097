"""The reconstruct backward on the GPU: beast_reconstruct_derivs_bwd_f32 and autograd through
reconstruct_traj_continuous / reconstruct_traj_continuous_derivs.

The oracle (tests/deriv_bwd_oracle.py) is fed the same fp32 slabs and gradients, upcast to
float64: the contraction is under test, the bases have their own tests.  The bound is the
accumulation's own, per element

    |got - want| <= (K + 3) 2^-24 s[k] sum_{o,t} |basis_o G_o|,    K = requested orders x T_out,

the standard bound of any summation order of K fp32 products plus the roundings of s and of the
final scale; masked elements must be exactly 0.
"""
import itertools

import numpy as np
import pytest
import torch

import deriv_bwd_oracle as O
from test_deriv_bwd_oracle import ORDER_SETS, make_inputs
from beast_tokenizer_amd import BEASTBsplineTokenizer, _lib
from beast_tokenizer_amd.synthetic import synth_trajectories

pytestmark = pytest.mark.gpu


def launch(dev, c, *, init_p=False, want_ip=True, misalign=False):
    """One launch on the inputs of make_inputs: (grad_ntokens [B, N, D], grad_init_p or None) as
    numpy.  The outputs start as NaN (grad_init_p as zeros, the caller's part of the contract), so
    an element the kernel skips shows."""
    B, N, D = c["x"].shape
    T = c["basis"].shape[-2]
    per_row = c["basis"].ndim == 5

    def dv(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    grads = [None, None, None]
    for o, g in enumerate(c["grads"]):
        if g is not None:
            buf = torch.zeros(g.size + 4, dtype=torch.float32, device=dev)
            grads[o] = buf[1:1 + g.size] if misalign else buf[:g.size]      # one float off 16-byte alignment
            grads[o].copy_(dv(g).reshape(-1))
    x, lo, hi, basis, dst, src = map(dv, (c["x"], c["lo"], c["hi"], c["basis"], c["dst"], c["ip_src"]))
    gx = torch.full((B, N, D), float("nan"), dtype=torch.float32, device=dev)
    gip = torch.zeros((B, D + 3), dtype=torch.float32, device=dev) if init_p and want_ip else None
    _lib.run("beast_reconstruct_derivs_bwd_f32", *map(_lib.ptr, grads), B, D, c["nj"], N, lo.data_ptr(),
             hi.data_ptr(), basis.data_ptr(), 3 * 2 * T * N if per_row else 0, T, dst.data_ptr(), c["ndo"],
             x.data_ptr(), src.data_ptr() if init_p else None, gx.data_ptr(), _lib.ptr(gip), D + 3, None)
    torch.cuda.synchronize()
    return gx.cpu().numpy(), None if gip is None else gip.cpu().numpy()


def check(dev, c, **kw):
    init_p = kw.get("init_p", False)
    got, got_ip = launch(dev, c, **kw)
    r = O.backward(c["grads"], c["basis"], c["lo"], c["hi"], c["x"], c["dst"], c["nj"],
                   init_p_src=c["ip_src"] if init_p else None,
                   init_p_width=c["x"].shape[2] + 3 if got_ip is not None else None)
    tol = O.bound(r)
    err = np.abs(got.astype(np.float64) - r.grad_ntokens)
    assert not np.isnan(got).any()
    assert (err <= tol).all(), (c["x"].shape, kw, float((err - tol).max()))
    assert not got[r.grad_ntokens == 0].any()                         # masked / overwritten: exact zeros
    if got_ip is not None:
        nj, src = c["nj"], c["ip_src"]
        tol_ip = (r.terms * O.EPS * r.mag[:, :nj, 0])
        assert (np.abs(got_ip[:, src[:nj]] - r.grad_init_p[:, src[:nj]]) <= tol_ip).all()
        untouched = sorted(set(range(got_ip.shape[1])) - set(src[:nj].tolist()))
        assert not got_ip[:, untouched].any()                         # gripper and unnamed columns stay 0
    return got, got_ip


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ------------------------------------------------------------------ raw entry point --
@pytest.mark.parametrize("D", [1, 14, 64])
@pytest.mark.parametrize("N", [1, 3, 5, 8, 10, 16])
def test_tile_and_vector_edges(N, D, gpu_device):
    """B around the tiles of 4 (and 16: tiles are capped at 256 / D trajectories), T_out 1, 7, 50
    (rows of 7 x D floats take the element loads where that is no multiple of four), every padding
    of N (N = 5 and 8 are the ends of KS = 2); the layouts cycle over no grippers / two / all, extra permuted output columns, per-row
    slabs, misaligned gradients and the order subsets, so each appears at several (B, T)."""
    layouts = itertools.cycle([dict(), dict(ndo=D + 5), dict(per_row=True), dict(misalign=True),
                               dict(ndo=D + 2, per_row=True, misalign=True)])
    joints = itertools.cycle([D, max(D - 2, 0), 0])
    sets = itertools.cycle(ORDER_SETS)
    for B in (1, 3, 4, 5, 16, 17, 37):
        for T in (1, 7, 50):
            kw = dict(next(layouts))
            misalign = kw.pop("misalign", False)
            check(gpu_device, make_inputs(B, T, D, next(joints), N, next(sets), **kw), misalign=misalign)


@pytest.mark.parametrize("orders", ORDER_SETS)
@pytest.mark.parametrize("per_row", [False, True])
def test_every_order_subset(orders, per_row, gpu_device):
    """Each single order, each pair and all three; the slabs of the other orders (and the gripper
    slabs of orders 1 and 2) hold NaN, which would reach the output if they were read."""
    check(gpu_device, make_inputs(17, 50, 14, 12, 10, orders, per_row=per_row))


@pytest.mark.parametrize("nj", [0, 12, 14])
@pytest.mark.parametrize("kw", [dict(ndo=19), dict(per_row=True), dict(misalign=True),
                                dict(ndo=17, per_row=True, misalign=True)])
def test_layouts(nj, kw, gpu_device):
    """num_dof_out > D with a permuted dof_dst, n_joint 0 / D - 2 / D, shared and per-row slabs,
    gradient pointers one float off 16-byte alignment (element loads)."""
    kw = dict(kw)
    misalign = kw.pop("misalign", False)
    check(gpu_device, make_inputs(37, 50, 14, nj, 10, (0, 1, 2), **kw), misalign=misalign)


@pytest.mark.parametrize("bulk", [False, True], ids=["small_tiles", "bulk_tiles"])
@pytest.mark.parametrize("per_row", [False, True], ids=["lds_slabs", "slabs_in_memory"])
@pytest.mark.parametrize("orders", [(1,), (0, 2), (0, 1, 2)], ids=["ns1", "ns2", "ns3"])
@pytest.mark.parametrize("N", [3, 5, 8, 10, 16])
def test_every_instantiation(N, orders, per_row, bulk, gpu_device):
    """k_reconstruct_derivs_bwd<KS, NS, LB, PF>: KS = ceil(N / 4) (both ends of KS = 2), NS
    gradients given, the slabs staged in LDS or read per row, and the small tiles (PF = 1) or, from
    two tiles of 16 per CU on, the bulk ones with two trajectories in flight (PF = 2); the last
    tile is partial in both.  Every product is launched here at the smallest payload."""
    B = 2 * 16 * cu_count() + 5 if bulk else 7
    check(gpu_device, make_inputs(B, 4, 2, 1, N, orders, ndo=3, per_row=per_row), init_p=True)


def test_bulk_variant_and_slabs_in_memory(gpu_device):
    """From two tiles of 16 per CU on, the launch takes tiles of 16 (full and a partial last one)
    with two trajectories in flight per thread; at 2 CUs + 1 tiles the resident workgroups get one
    tile each unless fewer than three fit a CU (tests/test_gpu_second_pass.py makes them stride).
    T_out 4096 puts the shared slabs in memory and cuts the time axis into many chunks."""
    B = 2 * 16 * cu_count() + 5
    check(gpu_device, make_inputs(B, 4, 2, 1, 3, (0, 1, 2)))
    check(gpu_device, make_inputs(B, 4, 2, 2, 3, (1,), per_row=True), misalign=True)
    check(gpu_device, make_inputs(2, 4096, 2, 2, 3, (0, 1, 2)))
    check(gpu_device, make_inputs(2, 4096, 2, 1, 3, (0, 2), ndo=3))


# ---------------------------------------------------------------------------- mask --
def test_mask(gpu_device):
    """x = +-1 pass; nextafter(+-1, +-2) and NaN give exactly 0, also where the upstream gradient
    holds inf (the sum is then inf or NaN: the mask must be a select, not a multiply)."""
    c = make_inputs(5, 7, 3, 2, 4, (0, 1, 2))
    x = c["x"]
    x[0, :, 0] = [1, -1, np.nextafter(np.float32(1), np.float32(2)), np.nan]
    x[1, :2, 1] = [np.nextafter(np.float32(-1), np.float32(-2)), -1]
    c["grads"][0][:2, :, c["dst"][0]] = np.inf
    c["grads"][1][:2, :, c["dst"][1]] = -np.inf
    got, _ = launch(gpu_device, c)
    assert not np.isfinite(got[0, :2, 0]).any()                       # passed: the non-finite sum arrives
    assert (got[0, 2:, 0] == 0).all() and got[1, 0, 1] == 0
    assert not np.isfinite(got[1, 1, 1])
    r = O.backward(c["grads"], c["basis"], c["lo"], c["hi"], x, c["dst"], c["nj"])
    fin = np.isfinite(r.grad_ntokens)
    assert (np.abs(got[fin] - r.grad_ntokens[fin]) <= O.bound(r)[fin]).all()
    assert not got[r.grad_ntokens == 0].any() and (r.grad_ntokens == 0).sum() >= 3


# -------------------------------------------------------------------------- init_p --
@pytest.mark.parametrize("nj,per_row", [(12, False), (14, True), (0, False)])
def test_init_p(nj, per_row, gpu_device):
    """Coefficient 0 of the joint DoFs gets 0; grad_init_p holds S[:, d, 0] at the named columns
    and 0 elsewhere (gripper columns untouched); a null grad_init_p changes nothing else."""
    c = make_inputs(37, 50, 14, nj, 10, (0, 1, 2), ndo=16, per_row=per_row)
    got, got_ip = check(gpu_device, c, init_p=True)
    assert not got[:, 0, :nj].any() and got_ip is not None
    got2, none = check(gpu_device, c, init_p=True, want_ip=False)
    assert none is None and np.array_equal(got, got2, equal_nan=True)


# --------------------------------------------------------------------- determinism --
def test_determinism_and_batch_independence(gpu_device):
    """Two calls agree bitwise; rows 0, 17 and 36 of a B = 37 launch are bitwise the rows run
    alone (other tile size, other workgroup); and bitwise the rows inside a bulk-variant batch."""
    for per_row in (False, True):
        c = make_inputs(37, 50, 14, 12, 10, (0, 1, 2), per_row=per_row)
        got, got_ip = launch(gpu_device, c, init_p=True)
        again, again_ip = launch(gpu_device, c, init_p=True)
        assert np.array_equal(got, again, equal_nan=True) and np.array_equal(got_ip, again_ip)
        for b in (0, 17, 36):
            one = dict(c, x=c["x"][b:b + 1], grads=[g[b:b + 1] for g in c["grads"]],
                       basis=c["basis"][b:b + 1] if per_row else c["basis"])
            g1, ip1 = launch(gpu_device, one, init_p=True)
            assert np.array_equal(g1[0], got[b], equal_nan=True) and np.array_equal(ip1[0], got_ip[b])
    # the same rows tiled into a batch large enough for the bulk variant (tiles of 16)
    c = make_inputs(37, 4, 2, 1, 3, (0, 1, 2))
    reps = -(-(2 * 16 * cu_count() + 5) // 37)
    big = dict(c, x=np.tile(c["x"], (reps, 1, 1)), grads=[np.tile(g, (reps, 1, 1)) for g in c["grads"]])
    small, _ = launch(gpu_device, c)
    bulk, _ = launch(gpu_device, big)
    assert np.array_equal(bulk.reshape(reps, 37, 3, 2), np.broadcast_to(small, (reps, 37, 3, 2)), equal_nan=True)


# ----------------------------------------------------------------------- tokenizer --
B_TOK, GRIPPERS = 37, [6, 13]


def make_tok(dev, **kw):
    tok = BEASTBsplineTokenizer(num_dof=14, num_basis=10, seq_len=50, gripper_zero_order=True,
                                gripper_indices=GRIPPERS, device=str(dev), **kw)
    rng = np.random.default_rng(11)
    lo = -rng.uniform(0.5, 2.0, 140).astype(np.float32)
    tok.w_min.copy_(torch.from_numpy(lo))
    tok.w_max.copy_(torch.from_numpy(lo + rng.uniform(0.5, 3.0, 140).astype(np.float32)))
    return tok


@pytest.fixture(scope="module")
def tok(gpu_device):
    return make_tok(gpu_device)


def params_for(dev, seed=3):
    """Normalised params [B, N*D] in [-1.1, 1.1]: a few coefficients sit outside the clamp."""
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand((B_TOK, 140), generator=g) * 2.2) - 1.1).to(dev)


def times_for(kind):
    if kind == "default":
        return None
    t = torch.linspace(-0.3, 7.0, 23)
    return t if kind == "shared" else t[None, :] + torch.linspace(0, 1, B_TOK)[:, None]


def slabs_of(tok, times, orders, positions_only):
    """The fp32 slabs the forward reads, as [3, 2, T, N] or [B, 3, 2, T, N] numpy."""
    p = tok._plan()
    if not positions_only:
        return tok._deriv_basis_for(times, B_TOK, p, orders)[0].cpu().numpy()
    phi = p.keep[0] if times is None else tok._basis_for(times, B_TOK, p)[0]
    phi = phi.cpu().numpy()                                           # [2, T, N] or [B, 2, T, N]
    out = np.full(phi.shape[:-3] + (3,) + phi.shape[-3:], np.nan, dtype=np.float32)
    out[..., 0, :, :, :] = phi
    return out


def f64_autograd(tok, x, slabs, orders, weights, init_p=None):
    """d/dx, d/d init_p of sum_o <weights_o, out_o> through clamp -> denormalise -> einsum in
    float64 on the CPU, with the fp32 slabs upcast."""
    D, N, nj = 14, 10, tok.joint_dof
    order = tok.joint_indices + tok.gripper_indices
    x = x.detach().cpu().double().requires_grad_()
    lo, hi = (b.detach().cpu().double().reshape(D, N) for b in (tok.w_min, tok.w_max))
    w = ((x.clamp(-1, 1) + 1) / 2).reshape(-1, N, D).permute(0, 2, 1) * (hi - lo) + lo      # [B, D, N]
    ip = None
    if init_p is not None:
        ip = init_p.detach().cpu().double().requires_grad_()
        w = torch.cat([torch.cat([ip[:, order[:nj]], w[:, nj:, 0]], dim=1)[:, :, None], w[:, :, 1:]], dim=2)
    sl = torch.from_numpy(np.nan_to_num(slabs, nan=0.0)).double()
    kinds = torch.tensor([0] * nj + [1] * (D - nj))
    loss = 0
    for o, wt in zip(orders, weights):
        ph = sl[..., o, :, :, :][..., kinds, :, :]
        out = torch.einsum("bdtn,bdn->btd" if ph.dim() == 4 else "dtn,bdn->btd", ph, w)
        if o:
            out = out * (kinds == 0)
        full = torch.zeros_like(out)
        full[:, :, order] = out
        loss = loss + (full * wt.detach().cpu().double()).sum()
    return torch.autograd.grad(loss, (x,) if ip is None else (x, ip))


def oracle(tok, x, slabs, orders, weights, init_p=False):
    """The oracle's result for this backward (gradients in the tokenizer's (n d) order)."""
    grads = [None, None, None]
    for o, wt in zip(orders, weights):
        grads[o] = wt.detach().cpu().numpy()
    dst = np.array(tok.joint_indices + tok.gripper_indices)
    return O.backward(grads, slabs, tok.w_min.cpu().numpy().reshape(14, 10), tok.w_max.cpu().numpy().reshape(14, 10),
                      x.detach().float().cpu().numpy().reshape(-1, 10, 14), dst, tok.joint_dof,
                      init_p_src=dst if init_p else None, init_p_width=14 if init_p else None)


def run_method(tok, x, times, orders, positions_only, **kw):
    if positions_only:
        return (tok.reconstruct_traj_continuous(x, times=times, **kw),)
    return tok.reconstruct_traj_continuous_derivs(x, times=times, orders=orders, **kw)


def assert_grad(tok, x, got, times, orders, positions_only, weights):
    slabs = slabs_of(tok, times, orders, positions_only)
    (want,) = f64_autograd(tok, x, slabs, orders, weights)
    tol = O.bound(oracle(tok, x, slabs, orders, weights)).reshape(B_TOK, 140)
    err = (got.detach().cpu().double().reshape(B_TOK, 140) - want.reshape(B_TOK, 140)).abs().numpy()
    assert (err <= tol).all(), float((err - tol).max())


@pytest.mark.parametrize("method", ["positions", "derivs_012", "derivs_20"])
@pytest.mark.parametrize("times_kind", ["default", "shared", "per_row"])
def test_tokenizer_backward_matches_f64_autograd(method, times_kind, tok, gpu_device):
    """Backward of a weighted sum of the outputs against the float64 composition, for the default
    grid, a [T] grid and per-row [B, T] grids."""
    orders = {"positions": (0,), "derivs_012": (0, 1, 2), "derivs_20": (2, 0)}[method]
    times = times_for(times_kind)
    x = params_for(gpu_device).requires_grad_()
    outs = run_method(tok, x, times, orders, method == "positions")
    assert all(o.grad_fn is not None and o.dtype is torch.float32 for o in outs)
    g = torch.Generator().manual_seed(5)
    weights = [torch.randn(o.shape, generator=g).to(gpu_device) for o in outs]
    sum((o * w).sum() for o, w in zip(outs, weights)).backward()
    assert x.grad.shape == x.shape and x.grad.device == x.device
    assert_grad(tok, x, x.grad, times, orders, method == "positions", weights)
    # an output left out of the loss arrives as None and is passed as a null pointer
    if len(outs) > 1:
        x2 = x.detach().clone().requires_grad_()
        outs2 = run_method(tok, x2, times, orders, False)
        (outs2[0] * weights[0]).sum().backward()
        assert_grad(tok, x2, x2.grad, times, orders[:1], False, weights[:1])


def test_sum_backward_shapes_and_dtypes(tok, gpu_device):
    """y.sum().backward() (a stride-0 gradient); a [B, N, D] leaf gets a [B, N, D] gradient; a
    bf16 leaf gets the fp32 gradient of its values rounded to bf16; a host leaf gets a host one."""
    x = params_for(gpu_device).requires_grad_()
    tok.reconstruct_traj_continuous(x).sum().backward()
    ones = [torch.ones((B_TOK, 50, 14), device=gpu_device)]
    assert_grad(tok, x, x.grad, None, (0,), True, ones)
    x3 = x.detach().reshape(B_TOK, 10, 14).clone().requires_grad_()
    pos, acc = tok.reconstruct_traj_continuous_derivs(x3, orders=(0, 2))
    (pos.sum() + acc.sum()).backward()
    assert x3.grad.shape == (B_TOK, 10, 14)
    assert_grad(tok, x, x3.grad, None, (0, 2), False, ones * 2)
    xb = x.detach().to(torch.bfloat16).requires_grad_()
    tok.reconstruct_traj_continuous(xb).sum().backward()
    xf = xb.detach().float().requires_grad_()
    tok.reconstruct_traj_continuous(xf).sum().backward()
    assert xb.grad.dtype is torch.bfloat16 and torch.equal(xb.grad, xf.grad.to(torch.bfloat16))
    xh = x.detach().cpu().requires_grad_()
    tok.reconstruct_traj_continuous(xh).sum().backward()
    assert xh.grad.device.type == "cpu" and torch.equal(xh.grad, x.grad.cpu())


def test_conditioned_tokenizer(gpu_device):
    """init_cond_order = 2 after an encode of the same batch: the boundary term does not depend
    on the params, and the backward runs over the effective slabs the forward used."""
    ctok = make_tok(gpu_device, init_cond_order=2)
    ctok.encode(torch.from_numpy(synth_trajectories(B_TOK, 50, 14, seed=4, gripper_indices=GRIPPERS)))
    x = params_for(gpu_device).requires_grad_()
    outs = ctok.reconstruct_traj_continuous_derivs(x, orders=(0, 1, 2))
    g = torch.Generator().manual_seed(6)
    weights = [torch.randn(o.shape, generator=g).to(gpu_device) for o in outs]
    sum((o * w).sum() for o, w in zip(outs, weights)).backward()
    assert_grad(ctok, x, x.grad, None, (0, 1, 2), False, weights)


def test_init_p_requires_grad(tok, gpu_device):
    x = params_for(gpu_device).requires_grad_()
    g = torch.Generator().manual_seed(7)
    init_p = torch.randn((B_TOK, 14), generator=g).to(gpu_device).requires_grad_()
    outs = tok.reconstruct_traj_continuous_derivs(x, orders=(0, 1, 2), init_p=init_p)
    weights = [torch.randn(o.shape, generator=g).to(gpu_device) for o in outs]
    sum((o * w).sum() for o, w in zip(outs, weights)).backward()
    slabs = slabs_of(tok, None, (0, 1, 2), False)
    want, want_ip = f64_autograd(tok, x, slabs, (0, 1, 2), weights, init_p=init_p)
    r = oracle(tok, x, slabs, (0, 1, 2), weights, init_p=True)
    assert ((x.grad.cpu().double() - want).abs().numpy() <= O.bound(r).reshape(B_TOK, 140)).all()
    nj = tok.joint_dof
    assert not x.grad.reshape(B_TOK, 10, 14)[:, 0, :nj].any()
    assert init_p.grad.shape == (B_TOK, 14) and not init_p.grad[:, GRIPPERS].any()
    tol_ip = np.zeros((B_TOK, 14))
    tol_ip[:, tok.joint_indices] = r.terms * O.EPS * r.mag[:, :nj, 0]      # K products, no scale
    assert (np.abs(init_p.grad.cpu().double().numpy() - want_ip.numpy()) <= tol_ip).all()
    # init_p alone requiring grad takes the differentiable path too
    ip2 = init_p.detach().clone().requires_grad_()
    tok.reconstruct_traj_continuous(x.detach(), init_p=ip2).sum().backward()
    assert ip2.grad is not None and not ip2.grad[:, GRIPPERS].any() and ip2.grad[:, :6].any()


def test_no_graph_without_requires_grad(tok, gpu_device):
    """Without requires_grad, and under no_grad with it, no graph is recorded and the outputs
    are bitwise the grad-enabled forward's."""
    x = params_for(gpu_device)
    xg = x.clone().requires_grad_()
    t = times_for("per_row")
    with_graph = (tok.reconstruct_traj_continuous(xg), *tok.reconstruct_traj_continuous_derivs(xg, times=t))
    assert all(o.grad_fn is not None for o in with_graph)
    plain = (tok.reconstruct_traj_continuous(x), *tok.reconstruct_traj_continuous_derivs(x, times=t))
    with torch.no_grad():
        muted = (tok.reconstruct_traj_continuous(xg), *tok.reconstruct_traj_continuous_derivs(xg, times=t))
    for a, b, c in zip(with_graph, plain, muted):
        assert b.grad_fn is None and c.grad_fn is None and not b.requires_grad and not c.requires_grad
        assert torch.equal(a, b) and torch.equal(a, c)


def test_sgd_on_a_trajectory_loss(tok, gpu_device):
    """The use case: 20 steps of gradient descent on the position MSE.  The map is linear inside
    the clamp and the step is 1 / L for L = 2 max(s)^2 / (B D) >= the Hessian's largest eigenvalue
    (each basis row sums to 1 and each column to at most T), so the loss falls at every step."""
    target = tok.reconstruct_traj_continuous(params_for(gpu_device, seed=9) * 0.4)
    x = torch.zeros((B_TOK, 140), device=gpu_device, requires_grad=True)
    s = 0.5 * (tok.w_max - tok.w_min).to(gpu_device)
    lr = float(B_TOK * 14 / (2 * s.max() ** 2))
    losses = []
    for _ in range(20):
        loss = ((tok.reconstruct_traj_continuous(x) - target) ** 2).mean()
        losses.append(loss.item())
        (g,) = torch.autograd.grad(loss, x)
        with torch.no_grad():
            x -= lr * g
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    assert x.detach().abs().max().item() < 1                                # it never left the clamp
