"""Velocity / acceleration reconstruction on the GPU: beast_bspline_basis_deriv_f32,
beast_reconstruct_derivs_f32 and the tokenizers' reconstruct_traj_derivs / _vel / _acc.

Tolerances.  Errors against the float64 oracle are max|got - oracle| / max|oracle| per case and
order.  Order 1 may be 4x the reference's own fp32 get_traj_vel error on the same inputs, order 2
4x the error of the oracle run in float32 (both recorded per case in
tests/golden/deriv_tolerances.json), never less than 16 * 2^-24: the kernel sums the same
<= degree + 1 non-zero products but forms the derivative-basis entry first instead of
differencing control points, one more rounding per term in another association.  Order 0 is
held to test_gpu_parity's reconstruct tolerance.  The raw launch-shape tests use random slabs
and the dot product's own bound, (N + 1) 2^-24 sum|basis * w|.
"""
import itertools

import numpy as np
import pytest
import torch

from conftest import load_json, load_npz
import deriv_oracle as O
from test_deriv_oracle import CASES, TOL, case_config
from beast_tokenizer_amd import BEASTBsplineBPETokenizer, BEASTBsplineTokenizer, _lib
from beast_tokenizer_amd.bspline import DeviceBasis, knot_vector
from beast_tokenizer_amd.synthetic import synth_trajectories

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
FLOOR = 16 * EPS
ORDER_SETS = [s for r in (1, 2, 3) for s in itertools.combinations((0, 1, 2), r)]


def bound(yardstick):
    return max(4 * yardstick, FLOOR)


def close_pos(a, b):
    """test_gpu_parity's reconstruct tolerance."""
    scale = np.maximum(1.0, np.abs(b).max(axis=(1, 2), keepdims=True))
    err = (np.abs(a - b) / scale).max()
    assert err <= 1e-5, err


def check_order(name, order, got, g):
    """One order of one golden case against the oracle, to the bound of the module docstring."""
    want = g[f"oracle{order}"]
    assert got.shape == want.shape and got.dtype == np.float32
    if order == 0:
        close_pos(got, g["ref_pos"])
        return
    if not want.any():
        assert not got.any(), (name, order)
        return
    err = O.rel_err(got, want)
    tol = bound(TOL[name]["vel_ref_err" if order == 1 else "acc_f32_err"])
    print(f"{name} order {order}: err {err:.3e} bound {tol:.3e}")
    assert err <= tol, (name, order, err, tol)


def make_tok(cfg, g, dev, cls=BEASTBsplineTokenizer, **kw):
    tok = cls(num_dof=cfg["D"], num_basis=cfg["N"], duration=cfg["duration"], seq_len=50, vocab_size=256,
              degree_p=cfg["degree"], gripper_zero_order=bool(cfg["grippers"]),
              gripper_indices=cfg["grippers"] or None, init_cond_order=cfg["ic"], end_cond_order=cfg["ec"],
              device=str(dev), **kw)
    tok.w_min.copy_(torch.from_numpy(g["w_min"]))
    tok.w_max.copy_(torch.from_numpy(g["w_max"]))
    return tok


# ------------------------------------------------------------------ basis kernel --
def basis_times(degree, n_ctrl, tau):
    kv = np.unique(knot_vector(degree, n_ctrl).numpy())
    rng = np.random.default_rng(degree * 100 + n_ctrl)
    u = np.concatenate([[-0.5, -1e-3], kv, (kv[1:] + kv[:-1]) / 2, rng.uniform(0, 1, 23), [1.001, 1.7]])
    return (u.astype(np.float32) * np.float32(tau)).astype(np.float32)


def run_basis(t, tau, degree, n_ctrl, order, entry="beast_bspline_basis_deriv_f32"):
    kv = knot_vector(degree, n_ctrl).to(t.device)
    out = torch.full((t.numel(), n_ctrl), float("nan"), dtype=torch.float32, device=t.device)
    args = [t.data_ptr(), t.numel(), tau, 0.0, kv.data_ptr(), kv.numel(), degree, n_ctrl]
    args += [out.data_ptr(), None] if order is None else [order, out.data_ptr(), None]
    _lib.run(entry, *args)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("degree,n_ctrl", [(d, n) for d in (0, 1, 2, 4) for n in (2, 4, 10, 16) if n >= d + 1])
def test_basis_deriv_kernel(degree, n_ctrl, gpu_device):
    """Order 0 is beast_bspline_basis_f32 bitwise; orders 1, 2 against the oracle at times below
    0, above tau, on the knots (tau a power of two, so the fp32 phase hits them exactly and the
    right-continuous rule decides) and between them; an order above the degree gives zeros."""
    for tau in (2.0, float(np.float32(2 * np.pi))):
        tn = basis_times(degree, n_ctrl, tau)
        if tau != 2.0:   # the fp32 and the float64 phase may fall on different sides of a knot
            kv = np.unique(knot_vector(degree, n_ctrl).numpy().astype(np.float64))
            tn = tn[np.abs(O.phase(tn, tau)[:, None] - kv[None, 1:-1]).min(axis=1, initial=1.0) > 1e-6]
        t = torch.from_numpy(tn).to(gpu_device)
        b0 = run_basis(t, tau, degree, n_ctrl, 0)
        assert np.array_equal(b0, run_basis(t, tau, degree, n_ctrl, None, "beast_bspline_basis_f32"))
        for order in (1, 2):
            got = run_basis(t, tau, degree, n_ctrl, order)
            want = O.deriv_basis(tn, tau, degree, n_ctrl, order)
            if order > degree:
                assert not want.any() and not got.any()
                continue
            yard = O.rel_err(O.deriv_basis(tn, tau, degree, n_ctrl, order, dtype=np.float32), want)
            err = O.rel_err(got, want)
            print(f"degree {degree} C {n_ctrl} tau {tau:.3f} order {order}: err {err:.3e} f32 oracle {yard:.3e}")
            assert err <= bound(yard), (degree, n_ctrl, tau, order, err, yard)


def test_device_basis_methods(gpu_device):
    """deriv_basis_at / full_deriv_basis_at mirror basis_at / full_basis_at; conditioned
    tokenizers take the fitted columns; the default grid's slabs are cached."""
    t = torch.linspace(-0.2, 6.5, 31, device=gpu_device)
    plain = DeviceBasis(10, 4, 2 * np.pi, True)
    assert torch.equal(plain.deriv_basis_at(t, 0), plain.basis_at(t))
    d1 = plain.deriv_basis_at(t.reshape(1, 31).expand(3, 31), 1)
    assert d1.shape == (2, 3, 31, 10) and not d1[1].any() and torch.equal(d1[0, 2], plain.deriv_basis_at(t, 1)[0])
    cond = DeviceBasis(10, 4, 2 * np.pi, False, init_cond_order=2, end_cond_order=-1)
    assert torch.equal(cond.full_deriv_basis_at(t, 0), cond.full_basis_at(t))
    full = cond.full_deriv_basis_at(t, 2)
    assert full.shape == (31, 13) and torch.equal(cond.deriv_basis_at(t, 2)[0], cond.effective(full))
    want = O.deriv_basis(t.cpu().numpy(), 2 * np.pi, 4, 13, 2)
    assert O.rel_err(full.cpu().numpy(), want) <= FLOOR
    slabs = plain.deriv_constants(t, 7)
    assert slabs.shape == (3, 2, 31, 10) and plain.deriv_constants(t, 7) is slabs
    assert torch.equal(slabs[0], plain.basis_at(t)) and torch.equal(slabs[2, 0], plain.deriv_basis_at(t, 2)[0])


# ------------------------------------------------------------------------ goldens --
@pytest.mark.parametrize("name", CASES)
def test_goldens(name, gpu_device):
    """Every golden case, orders (0, 1, 2) from one call: plain, init_p, grippers, the
    conditioned tokenizers after an encode of the golden trajectories, degree 1 and 2, and the
    grids with t < 0, t > duration and the exact knots."""
    g, cfg = load_npz(f"deriv_{name}.npz"), case_config(name)
    tok = make_tok(cfg, g, gpu_device)
    if cfg["ic"] or cfg["ec"]:
        _, pd = tok.encode(torch.from_numpy(g["x"]))
        for k in ("init_pos", "init_vel", "end_pos", "end_vel"):
            if pd[k] is not None:
                np.testing.assert_allclose(pd[k].cpu().numpy(), g["cond_" + k], rtol=1e-6, atol=1e-6)
    times = torch.from_numpy(g["times"]) if TOL[name]["config"].get("grid") else None
    kw = {"init_p": torch.from_numpy(g["init_p"])} if "init_p" in g else {}
    outs = tok.reconstruct_traj_derivs(torch.from_numpy(g["tokens"]), times=times, **kw)
    assert isinstance(outs, tuple) and len(outs) == 3
    for order, out in enumerate(outs):
        check_order(name, order, out.cpu().numpy(), g)
    # the requested order of the outputs is kept, and the conveniences are the single orders
    a2, a0 = tok.reconstruct_traj_derivs(torch.from_numpy(g["tokens"]), times=times, orders=(2, 0), **kw)
    assert torch.equal(a2, outs[2]) and torch.equal(a0, outs[0])
    assert torch.equal(tok.reconstruct_traj_vel(torch.from_numpy(g["tokens"]), times=times, **kw), outs[1])
    assert torch.equal(tok.reconstruct_traj_acc(torch.from_numpy(g["tokens"]), times, **kw), outs[2])
    close_pos(outs[0].cpu().numpy(), tok.reconstruct_traj(torch.from_numpy(g["tokens"]), times=times, **kw)
              .cpu().numpy())


# ------------------------------------------------------------------ launch shapes --
def raw_case(dev, B, T, D, nj, N, orders, *, ndo=None, offset=0, per_row=False, init_p=False, ntok=False,
             misalign=False, seed=0, vocab=256):
    """One beast_reconstruct_derivs_f32 launch on random tokens, bounds and slabs (the slabs of
    the orders not requested poisoned with NaN) against a float64 sum of the same products."""
    rng = np.random.default_rng([seed, B, T, D, N])
    ndo = ndo or D
    f32 = np.float32
    tok = rng.integers(0, vocab, size=(B, N, D)).astype(np.int64)
    nt = rng.uniform(-1.2, 1.2, size=(B, N, D)).astype(f32)
    lo = (-rng.uniform(0.5, 2.0, (D, N))).astype(f32)
    hi = (lo + rng.uniform(0.5, 3.0, (D, N)).astype(f32)).astype(f32)
    slabs = rng.standard_normal(((B,) if per_row else ()) + (3, 2, T, N)).astype(f32)
    for o in range(3):
        if o not in orders:
            slabs[..., o, :, :, :] = np.nan
    dst = rng.permutation(ndo)[:D].astype(np.int32)
    ip = rng.standard_normal((B, D + 3)).astype(f32)
    ip_src = rng.permutation(D + 3)[:D].astype(np.int32)
    # fp32 params exactly as the kernel forms them (beast/utils.py:20-25 / :38-44)
    if ntok:
        c = np.clip(nt, f32(-1), f32(1))
        w = ((c - f32(-1)) / f32(2)) * (hi.T - lo.T) + lo.T
    else:
        w = np.clip((tok.astype(f32) / f32(vocab - 1)) * (hi.T - lo.T) + lo.T, lo.T, hi.T)
    w = np.ascontiguousarray(w.astype(f32).transpose(0, 2, 1))                    # [B, D, N]
    if init_p:
        w[:, :nj, 0] = ip[:, ip_src[:nj]]
    want = np.zeros((3, B, T, ndo))
    mag = np.zeros((3, B, T, ndo))
    for o in orders:
        for d in range(D):
            kind = 0 if d < nj else 1
            if o and kind:
                continue
            ph = slabs[..., o, kind, :, :].astype(np.float64)                     # [T, N] or [B, T, N]
            wd = w[:, d, :].astype(np.float64)
            sub = "tn,bn->bt" if ph.ndim == 2 else "btn,bn->bt"
            want[o, :, :, dst[d]] = np.einsum(sub, ph, wd)
            mag[o, :, :, dst[d]] = np.einsum(sub, np.abs(ph), np.abs(wd))

    def dv(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_tok, d_nt, d_lo, d_hi, d_slabs, d_dst, d_ip, d_src = map(dv, (tok + offset, nt, lo, hi, slabs, dst, ip, ip_src))
    outs = [None, None, None]
    for o in orders:
        buf = torch.full((B * T * ndo + 1,), float("nan"), dtype=torch.float32, device=dev)
        outs[o] = buf[1:] if misalign else buf[:-1]
    _lib.run("beast_reconstruct_derivs_f32", None if ntok else d_tok.data_ptr(), B, D, nj, N, vocab, offset,
             d_lo.data_ptr(), d_hi.data_ptr(), d_slabs.data_ptr(), 3 * 2 * T * N if per_row else 0, T,
             d_dst.data_ptr(), ndo, d_ip.data_ptr() if init_p else None, D + 3, d_src.data_ptr() if init_p else None,
             *map(_lib.ptr, outs), d_nt.data_ptr() if ntok else None, None)
    torch.cuda.synchronize()
    for o in orders:
        got = outs[o].cpu().numpy().reshape(B, T, ndo).astype(np.float64)
        assert not np.isnan(got).any(), (orders, o)
        assert (np.abs(got - want[o]) <= (N + 1) * EPS * mag[o]).all(), (B, T, D, N, orders, o)
        assert not got[mag[o] == 0].any()         # unnamed columns and gripper derivatives: exact zeros


@pytest.mark.parametrize("D,nj", [(1, 1), (7, 7), (14, 12)])
@pytest.mark.parametrize("N", [2, 10, 16])
def test_launch_shapes(D, nj, N, gpu_device):
    """Tile edges (B 1, 15, 16, 17, 33 against the small batches' tiles of 4; test_large_shapes
    runs the 16-trajectory tiles), T_out 1, 2, 50, 51, one DoF up to 14 with two grippers,
    every 16-byte padding of N; each (B, T) takes another subset of the orders, so every single
    order and every pair runs with the other slabs poisoned."""
    sets = itertools.cycle(ORDER_SETS)
    for B in (1, 15, 16, 17, 33):
        for T in (1, 2, 50, 51):
            raw_case(gpu_device, B, T, D, nj, N, next(sets))


@pytest.mark.parametrize("orders", ORDER_SETS)
@pytest.mark.parametrize("per_row", [False, True])
def test_every_order_subset(orders, per_row, gpu_device):
    """Each single order, each pair and all three, shared and per-row [B, T] slabs; the null
    outputs' slabs hold NaN, which would reach an output if they were read."""
    raw_case(gpu_device, 17, 51, 14, 12, 10, orders, per_row=per_row)


@pytest.mark.parametrize("kw", [
    dict(ndo=19), dict(offset=31744), dict(ntok=True), dict(init_p=True), dict(misalign=True),
    dict(ndo=9, per_row=True, init_p=True, offset=1000, misalign=True),
    dict(vocab=70000), dict(ntok=True, init_p=True, per_row=True),
])
def test_launch_options(kw, gpu_device):
    """num_dof_out > D with the unnamed columns zero, a non-zero LLM offset, normalised tokens,
    init_p, outputs that are not 16-byte aligned, a vocabulary above 2^16."""
    raw_case(gpu_device, 33, 50, 7, 5, 10, (0, 1, 2), **kw)
    raw_case(gpu_device, 5, 3, 7, 7, 9, (1, 2), **kw)


def test_large_shapes(gpu_device):
    """Shared slabs too large for LDS are read from memory (T_out 700 at N 16); the envelope's
    corner D 64, N 16 and a wide output row still fit one tile's LDS; from two tiles of 16
    trajectories per CU on (B 20,000 covers up to 625 CUs) the bulk tile runs, here with full
    tiles, with a partial last one (20,011 = 1,250 * 16 + 11), and on per-row slabs.  At these
    payloads eight workgroups fit a CU, so from 157 CUs on every workgroup gets one tile only:
    the loop over tiles is tests/test_gpu_second_pass.py's."""
    raw_case(gpu_device, 20000, 5, 14, 12, 10, (0, 1, 2))
    raw_case(gpu_device, 20011, 3, 2, 2, 6, (1, 2), ndo=3)
    raw_case(gpu_device, 20011, 1, 2, 1, 16, (0, 1), per_row=True, init_p=True)
    raw_case(gpu_device, 3, 700, 4, 3, 16, (0, 1, 2))
    raw_case(gpu_device, 18, 5, 64, 60, 16, (0, 2))
    raw_case(gpu_device, 2, 4, 3, 3, 5, (1,), ndo=4096)
    raw_case(gpu_device, 2, 4096, 2, 2, 3, (0, 1))


@pytest.mark.parametrize("bulk", [False, True], ids=["tiles_of_4", "tiles_of_16"])
@pytest.mark.parametrize("per_row", [False, True], ids=["lds_slabs", "slabs_in_memory"])
@pytest.mark.parametrize("N", [3, 5, 8, 10, 16])
def test_every_instantiation(N, per_row, bulk, gpu_device):
    """k_reconstruct_derivs<KS, LB, TB>: KS = ceil(N / 4) (both ends of KS = 2), the slabs staged in
    LDS or read per row, tiles of 4 or -- from two tiles of 16 per CU on -- of 16; a partial last
    tile in both.  Every product is launched here at the smallest payload."""
    cus = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    raw_case(gpu_device, 2 * 16 * cus + 5 if bulk else 7, 3, 2, 1, N, (0, 1, 2), ndo=3, per_row=per_row, init_p=True)


# -------------------------------------------------------------------- equivalence --
@pytest.fixture(scope="module")
def grip_tok(gpu_device):
    g, cfg = load_npz("deriv_grip_d14.npz"), case_config("grip_d14")
    return make_tok(cfg, g, gpu_device), torch.from_numpy(synth_trajectories(37, 50, 14, seed=4, gripper_indices=[6, 13]))


def test_token_input_forms(grip_tok, gpu_device):
    """3-D, int32 and host token inputs go through _token_rows; an LLM offset is subtracted;
    [B, T] times equal to one grid take the shared path and give the same bits."""
    tok, x = grip_tok
    toks, _ = tok.encode(x)
    want = tok.reconstruct_traj_derivs(toks)
    for alt in (toks.reshape(37, 10, 14), toks.to(torch.int32), toks.cpu(), toks.reshape(37, 10, 14).to(torch.int32)):
        assert all(torch.equal(a, b) for a, b in zip(tok.reconstruct_traj_derivs(alt), want))
    with pytest.raises(ValueError, match="Token dimension"):
        tok.reconstruct_traj_derivs(toks[:, :-1])
    t = torch.linspace(-0.3, 7.0, 23)
    shared = tok.reconstruct_traj_derivs(toks, times=t)
    assert all(torch.equal(a, b) for a, b in zip(tok.reconstruct_traj_derivs(toks, times=t.expand(37, 23)), shared))
    # genuinely per-row times: row b is the shared-grid result of its own grid
    tb = t[None, :] + torch.linspace(0, 1, 37)[:, None]
    rows = tok.reconstruct_traj_derivs(toks, times=tb)
    for b in (0, 17, 36):
        one = tok.reconstruct_traj_derivs(toks[b:b + 1], times=tb[b])
        assert all(torch.equal(r[b], o[0]) for r, o in zip(rows, one))
    tok.set_llm_vocab_size(32000)
    try:
        llm, _ = tok.encode(x)
        assert torch.equal(llm, toks + (32000 - 256))
        assert all(torch.equal(a, b) for a, b in zip(tok.reconstruct_traj_derivs(llm), want))
        assert all(torch.equal(a, b) for a, b in
                   zip(tok.reconstruct_traj_derivs(toks, respect_llm_vocab_size=False), want))
    finally:
        tok.set_llm_vocab_size(None)
    assert tok.reconstruct_traj_vel(toks[:0]).shape == (0, 50, 14)


def test_single_orders_and_order_zero(grip_tok):
    tok, x = grip_tok
    toks, _ = tok.encode(x)
    pos, vel, acc = tok.reconstruct_traj_derivs(toks)
    assert torch.equal(tok.reconstruct_traj_derivs(toks, orders=(1,))[0], tok.reconstruct_traj_vel(toks))
    assert torch.equal(vel, tok.reconstruct_traj_vel(toks)) and torch.equal(acc, tok.reconstruct_traj_acc(toks))
    close_pos(pos.cpu().numpy(), tok.reconstruct_traj(toks).cpu().numpy())
    assert not vel[..., [6, 13]].any() and not acc[..., [6, 13]].any() and vel[..., :6].any()
    assert not pos.requires_grad and pos.grad_fn is None


def test_continuous_form_matches_token_form(grip_tok):
    """Normalised params that sit on bin centres decode to the tokens' params up to rounding:
    n = 2 tok / 255 - 1 (one fp32 rounding), then ((n + 1) / 2) (hi - lo) + lo against
    (tok / 255) (hi - lo) + lo -- the two differ by at most three roundings of 2^-24 in the
    normalised domain, times hi - lo <= 2 max|bound|, and two of the result: 8 * 2^-24
    max|bound| per coefficient.  Each form then rounds its dot product by at most
    (N + 1) 2^-24 sum|basis| max|bound|."""
    tok, x = grip_tok
    toks, _ = tok.encode(x)
    ntok, _ = tok.encode_continuous(x)
    assert ntok.shape == toks.shape
    centres = (toks.to(torch.float64) / 255 * 2 - 1).to(torch.float32)
    assert (centres - ntok).abs().max() <= 1 / 255 + 1e-6          # the same bins
    cont = tok.reconstruct_traj_continuous_derivs(centres)
    disc = tok.reconstruct_traj_derivs(toks)
    wmax = float(torch.maximum(tok.w_min.abs(), tok.w_max.abs()).max())
    slabs = tok._basis.deriv_constants(tok.times.to(torch.float32).reshape(-1), tok._times_version)
    for o in range(3):
        rowsum = slabs[o].abs().sum(-1).max(0).values              # [T], the larger of the two kinds
        tol = (8 + 2 * (10 + 1)) * EPS * rowsum * wmax
        assert ((cont[o] - disc[o]).abs() <= tol[None, :, None]).all(), o
    assert torch.equal(tok.reconstruct_traj_continuous_derivs(centres.reshape(37, 10, 14), orders=(1,))[0], cont[1])
    close_pos(cont[0].cpu().numpy(), tok.reconstruct_traj_continuous(centres).cpu().numpy())


# -------------------------------------------------------------- boundary property --
@pytest.mark.parametrize("ic,ec", [(2, 0), (0, 2), (2, 2)])
def test_boundary_velocity_is_the_encoded_condition(ic, ec, gpu_device):
    """Why the feature exists: with init_cond_order 2 the decoded velocity at times[0] is the
    init_vel that encode returned, with end_cond_order 2 the one at times[-1] is end_vel -- what
    the next chunk's conditioned encode is given.  To the order-1 tolerance."""
    g, cfg = load_npz("deriv_cond_d4_2_0.npz"), case_config("cond_d4_2_0")
    tok = make_tok(dict(cfg, ic=ic, ec=ec), g, gpu_device)
    toks, pd = tok.encode(torch.from_numpy(g["x"]))
    vel = tok.reconstruct_traj_vel(toks).cpu().numpy()
    tol = bound(TOL["cond_d4_2_0"]["vel_ref_err"])
    for on, idx, key in ((ic, 0, "init_vel"), (ec, -1, "end_vel")):
        if on:
            err = O.rel_err(vel[:, idx, :], pd[key].cpu().numpy())
            print(f"({ic}, {ec}) {key}: err {err:.3e} bound {tol:.3e}")
            assert err <= tol, (key, err, tol)


def test_condition_errors(gpu_device):
    """The errors of _add_conditions: no prior encode, another batch size."""
    g, cfg = load_npz("deriv_cond_d4_2_0.npz"), case_config("cond_d4_2_0")
    tok = make_tok(cfg, g, gpu_device)
    toks = torch.from_numpy(g["tokens"])
    with pytest.raises(RuntimeError, match="previous"):
        tok.reconstruct_traj_vel(toks)
    tok.encode(torch.from_numpy(g["x"]))
    with pytest.raises(RuntimeError, match="Sizes of tensors must match"):
        tok.reconstruct_traj_derivs(toks[:3])
    per_row = torch.from_numpy(g["times"])[None, :] + torch.arange(4)[:, None] * 0.01
    pos, vel = tok.reconstruct_traj_derivs(toks, times=per_row, orders=(0, 1))
    close_pos(pos.cpu().numpy(), tok.reconstruct_traj(toks, times=per_row).cpu().numpy())
    one = tok.reconstruct_traj_vel(toks, times=per_row[2].expand(4, 50))
    assert torch.equal(vel[2], one[2])


# -------------------------------------------------------------------------- BPE --
def test_bpe_tokenizer_delegates(gpu_device):
    """BEASTBsplineBPETokenizer's methods equal the base tokenizer's on the decoded bins."""
    g, cfg = load_npz("deriv_d4_n10_d7.npz"), case_config("d4_n10_d7")
    base = make_tok(cfg, g, gpu_device)
    bpe = make_tok(cfg, g, gpu_device, cls=BEASTBsplineBPETokenizer, bpe_vocab_size=400)
    bpe.fit_from_trajectories([torch.from_numpy(synth_trajectories(512, 50, 7, seed=21))], show_progress=False)
    x = torch.from_numpy(synth_trajectories(9, 50, 7, seed=22)).to(gpu_device)
    ids, _ = bpe.encode(x)
    bins = bpe.bpe_to_mp_tokens(ids)
    assert torch.equal(bins, base.encode(x)[0])
    t = torch.linspace(0, 6, 11)
    want = base.reconstruct_traj_derivs(bins, times=t, orders=(2, 1))
    got = bpe.reconstruct_traj_derivs(bins, times=t, orders=(2, 1))
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert torch.equal(bpe.reconstruct_traj_vel(bins, t), want[1])
    assert torch.equal(bpe.reconstruct_traj_acc(bins, times=t), want[0])
    assert torch.equal(bpe.reconstruct_traj_derivs(bins)[0], base.reconstruct_traj_derivs(bins)[0])
