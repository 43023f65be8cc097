"""The shared-grid codec after ``update_times``: every contract of DESIGN.md §Parity on time grids
other than linspace(0, 2 pi, T), against the float64 oracle built from that grid.

The grids are those of tests/golden/grid_consts.npz (squared, Chebyshev, reversed, overshooting both
ends, inner, first half, jittered).  Contracts, per configuration, grid and batch size (1, 5 and
16 CUs + 11, so the latency and the bulk kernels both run):
  1. constants: tok._basis.constants(...)[0] is bitwise oracle.basis; the plan's T is the grid's;
  2. params: |gpu - fit_exact| <= (Tp + 8) 2^-24 sum_t |P[n,t]| |y[t]| + 1e-30 with this grid's P;
  3. tokens: bit-equal to continuous_to_discrete(clamp(params_gpu)) on the kernel's own params;
  4. decode: bit-equal to the oracle's;
  5. positions: within 1e-5 max(1, |ref|_inf per trajectory) of float64 Phi @ decoded;
  6. a tokenizer left on the default grid and given ``times=grid`` returns the same bits (and, for
     reconstruct_traj, takes the same launch branch); orders 1 and 2 meet test_gpu_derivs' bound,
     max(4 yard, 16 * 2^-24) with yard the float32 run of deriv_oracle.trajectory;
  7. encode_at(x, grid per row) and encode(x) differ by at most the sum of their own bounds
     against fit_exact (2. and test_gpu_rows' 1e-5 max(1, |ref row|_inf));
  8. reconstruction_stats meets tests/roundtrip_oracle.py with this grid's Phi.
A sequential fp32 accumulation of the same products in numpy uses at most 0.31 of bound 2 (T = 13;
0.23 at the other shapes) and 0.10 of bound 5 on these configurations and grids, so a plain
restatement is well inside both; the kernels measured 0.24 and 0.13.

Then the conditioned tokenizers on such grids, staleness (one tokenizer switched between grids
against fresh ones, bitwise, under every kernel mode), and the constants cache, which must not grow
with the number of ``update_times`` calls.
"""
import numpy as np
import pytest
import torch

import deriv_oracle as DO
import roundtrip_oracle as R
from oracle import beast_oracle as O
from test_gpu_codec_dispatch import (_assert_close, _batch, _dn_to_nd, _make_tok, _positions_ref, _set_modes)
from test_gpu_constants import grid_names, load_grid_consts
from test_gpu_derivs import bound as deriv_bound
from test_gpu_roundtrip import _raw
from beast_tokenizer_amd import BEASTBsplineTokenizer, _lib
from beast_tokenizer_amd.synthetic import synth_trajectories

pytestmark = pytest.mark.gpu

F32 = np.float32
TAU = F32(2 * np.pi)
VOCAB = 256
CLAMP = 0.05
BATCHES = [1, 5, "16cu+11"]

# (degree, N, T, D, grippers)
K1G = (4, 10, 50, 7, (6,))
CONFIGS = [K1G, (3, 8, 33, 3, ()), (5, 16, 64, 2, ()), (4, 10, 13, 2, ())]
# at T = 13 the other grids push |P| to ~400: a plain fp32 reference already uses 0.8 of bound 5
GRIDS_T13 = ["default", "cheb", "reversed", "overshoot"]


def grids_of(cfg):
    return GRIDS_T13 if cfg[2] == 13 else [g for g in grid_names() if g != "unit_0_1"]


def grid_times(cfg, name):
    return load_grid_consts()[(cfg[0], cfg[1], cfg[2], name)]["times"]


_X, _REF = {}, {}


def _trajectories(cfg, B):
    degree, N, T, D, grip = cfg
    if (cfg, B) not in _X:
        x = synth_trajectories(B, T, D, seed=100 + T + D, gripper_indices=grip)
        x.setflags(write=False)
        _X[(cfg, B)] = x
    return _X[(cfg, B)]


def _ref(cfg, name, dev):
    """The float64 oracle of one configuration on one grid at the largest batch (the smaller ones
    are its first rows): x, the exact fit rounded once, the bound sums, bounds at the 5 % / 95 %
    quantiles of the exact fit, the layout and the two bases.  Shared and never modified."""
    if (cfg, name) not in _REF:
        degree, N, T, D, grip = cfg
        B = _batch("16cu+11", dev)
        x, t = _trajectories(cfg, B), grid_times(cfg, name)
        lay = O.Layout.make(D, list(grip) or None, bool(grip))
        exact, sums, phis = [], [], []
        for idx, deg in ((lay.joint_indices, degree), (lay.gripper_indices, 0)):
            phi = O.basis(t, TAU, deg, N)
            phis.append(phi)
            if idx:
                y = x[..., idx]
                exact.append(O.fit_exact(y, phi))
                sums.append(np.einsum("nt,btd->bdn", np.abs(O.projection_f64(phi)),
                                      np.abs(y.astype(np.float64))).reshape(B, -1))
        exact, sums = np.concatenate(exact, axis=-1), np.concatenate(sums, axis=-1)
        lo = np.quantile(exact, CLAMP, axis=0).astype(F32)
        hi = np.quantile(exact, 1 - CLAMP, axis=0).astype(F32)
        for a in (exact, sums, lo, hi, *phis):
            a.setflags(write=False)
        _REF[(cfg, name)] = dict(x=x, t=t, exact=exact, sums=sums, lo=lo, hi=hi, lay=lay, phi=phis)
    return _REF[(cfg, name)]


def _bits(a, b):
    """Bitwise equality of two tensors (NaN == NaN)."""
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return a.shape == b.shape and torch.equal(a, b)


def _cases():
    return [pytest.param(cfg, name, B, id=f"d{cfg[0]}n{cfg[1]}t{cfg[2]}-{name}-{B}")
            for cfg in CONFIGS for name in grids_of(cfg) for B in BATCHES]


WORST = {}


def _note(key, ratio):
    WORST[key] = max(WORST.get(key, 0.0), float(ratio))


@pytest.fixture(scope="module", autouse=True)
def worst_ratios():
    yield
    for key in sorted(WORST):
        print(f"worst ratio {key}: {WORST[key]:.3f}")


@pytest.mark.parametrize("cfg,name,B", _cases())
def test_codec_on_grid(cfg, name, B, gpu_device):
    dev = gpu_device
    degree, N, T, D, grip = cfg
    r = _ref(cfg, name, dev)
    B = _batch(B, dev)
    x, exact, sums, lo, hi, lay, t = r["x"][:B], r["exact"][:B], r["sums"][:B], r["lo"], r["hi"], r["lay"], r["t"]
    grid = torch.from_numpy(t.copy())
    _set_modes()
    tok = _make_tok(dev, D, N, T, VOCAB, degree, list(grip) or None, lo, hi)
    tok.update_times(grid)
    other = _make_tok(dev, D, N, T, VOCAB, degree, list(grip) or None, lo, hi)      # stays on the default grid
    xd = torch.tensor(x).to(dev)

    # 1. constants
    phi_gpu = tok._basis.constants(tok.times.to(dev, torch.float32).reshape(-1), tok._times_version)[0]
    assert tok._constants(dev)[0] is phi_gpu
    phi_np = phi_gpu.cpu().numpy()
    assert phi_np.shape == (2, T, N)
    assert np.array_equal(phi_np[0].view(np.uint32), r["phi"][0].view(np.uint32))
    if grip:
        assert np.array_equal(phi_np[1].view(np.uint32), r["phi"][1].view(np.uint32))
    else:
        assert not phi_np[1].any()
    assert tok._plan().T == T

    # 2. params  3. tokens
    tokens_t, pd = tok.encode(xd)
    params, tokens = pd["params"].cpu().numpy(), tokens_t.cpu().numpy()
    Tp = -(-T // 4) * 4
    pbound = (Tp + 8) * 2.0 ** -24 * sums + 1e-30
    perr = np.abs(params - exact)
    _note(f"params {name}", (perr / pbound).max())
    assert np.all(perr <= pbound), float((perr / pbound).max())
    want = _dn_to_nd(O.continuous_to_discrete(O._clamp_t(params, lo, hi), lo, hi, VOCAB), B, D, N)
    assert np.array_equal(tokens, want)
    if B > 100:
        assert (params < lo).any() and (params > hi).any() and want.min() == 0 and want.max() == VOCAB - 1

    # 4. decode  5. positions
    dec = tok.decode(tokens_t).cpu().numpy()
    want_dec = O.decode(tokens, lay, N, lo, hi, VOCAB)
    assert np.array_equal(dec.view(np.uint32), want_dec.view(np.uint32))
    w = want_dec.reshape(B, D, N)
    pos_t = tok.reconstruct_traj(tokens_t)
    branch = _lib.last_codec_launch()
    pos = pos_t.cpu().numpy()
    assert pos.shape == (B, T, D)
    want_pos = _positions_ref(w, lay, t, degree, N, lay.order, D)
    scale = np.maximum(1.0, np.abs(want_pos).max(axis=(1, 2), keepdims=True))
    _note(f"positions {name}", (np.abs(pos - want_pos) / scale).max() / 1e-5)
    _assert_close(pos, want_pos)

    # 6. one computation, two spellings
    pos_o = other.reconstruct_traj(tokens_t, times=grid)
    assert _lib.last_codec_launch() == branch, (branch, _lib.last_codec_launch())
    assert _bits(pos_o, pos_t)
    derivs = tok.reconstruct_traj_derivs(tokens_t)
    derivs_o = other.reconstruct_traj_derivs(tokens_t, times=grid)
    assert all(_bits(a, b) for a, b in zip(derivs, derivs_o))
    _assert_close(derivs[0].cpu().numpy(), want_pos)
    nj = len(lay.joint_indices)
    for order in (1, 2):
        got = derivs[order].cpu().numpy()
        assert not got[..., lay.gripper_indices].any()
        ctrl = w[:, :nj]
        want_d = DO.trajectory(t, TAU, degree, ctrl, order)
        yard = DO.rel_err(DO.trajectory(t, TAU, degree, ctrl, order, dtype=np.float32), want_d)
        err = DO.rel_err(got[..., lay.joint_indices], want_d)
        _note(f"derivative order {order} {name}", err / deriv_bound(yard))
        assert err <= deriv_bound(yard), (order, err, yard)

    # 7. two implementations of the fit
    p_at = tok.encode_at(xd, grid.to(dev).expand(B, T))[1]["params"].cpu().numpy()
    rows_bound = 1e-5 * np.maximum(1.0, np.abs(exact).max(axis=1, keepdims=True))
    assert np.all(np.abs(p_at - exact) <= rows_bound)
    assert np.all(np.abs(p_at - params) <= pbound + rows_bound)

    # 8. round-trip statistics
    order_cols = torch.tensor(lay.order, device=dev)
    y = xd[..., order_cols].contiguous().cpu().numpy()
    pos_dof = pos_t[..., order_cols].contiguous().cpu().numpy()
    phi32 = np.stack([r["phi"][0], r["phi"][1] if grip else np.zeros_like(r["phi"][1])])
    s = R.stats(y, pos_dof, params.reshape(B, D, N), phi32, lo, hi, nj)
    stats, tk, clip = _raw(tok, xd.data_ptr(), B, xd.stride(), xd.shape[2])
    assert torch.equal(tk, tokens_t)
    R.assert_stats(stats.cpu().numpy(), s)
    c = clip.cpu().numpy().astype(np.int64)
    assert np.array_equal(c[0], s["clip_low"]) and np.array_equal(c[1], s["clip_high"])
    rs = tok.reconstruction_stats(xd, return_tokens=True)
    inv_t = 1.0 / T
    assert torch.equal(rs.tokens, tokens_t)
    assert _bits(rs.mse, tok._scatter_cols(stats[..., 1] * inv_t))
    assert _bits(rs.mean_err, tok._scatter_cols(stats[..., 0] * inv_t))
    assert _bits(rs.max_abs, tok._scatter_cols(stats[..., 2]))
    assert _bits(rs.mse_fit, tok._scatter_cols(stats[..., 3] * inv_t))
    assert np.array_equal(rs.clip_low.cpu().numpy().reshape(-1), s["clip_low"])
    assert np.array_equal(rs.clip_high.cpu().numpy().reshape(-1), s["clip_high"])


# ----------------------------------------------------------------------- conditioned --
COND = [(1, 0), (2, -1), (2, 2), (0, 1)]
COND_GRIDS = ["squared", "jitter", "cheb", "reversed", "overshoot"]
COND_CFG = (4, 10, 50, 3, ())


def _cond_tok(dev, ic, ec, lo, hi, T=50, D=3):
    tok = BEASTBsplineTokenizer(num_dof=D, num_basis=10, seq_len=T, vocab_size=VOCAB, degree_p=4,
                                init_cond_order=ic, end_cond_order=ec, device=str(dev))
    tok.load_state_dict({"w_min": lo.tolist(), "w_max": hi.tolist()})
    return tok


@pytest.mark.parametrize("name", COND_GRIDS)
@pytest.mark.parametrize("ic,ec", COND)
def test_conditioned_on_grid(ic, ec, name, gpu_device):
    """test_prop_conditioned_encode_reconstruct's contracts (1e-5 max(1, |want|_inf)) after
    update_times: dt = t[1] - t[0] of the new grid (negative on ``reversed``, small on ``squared``)
    enters the boundary control points and the conditioned projection."""
    dev = gpu_device
    degree, N, T, D, _ = COND_CFG
    B = 37
    x, t = _trajectories(COND_CFG, B), grid_times(COND_CFG, name)
    want_p, st = O.cond_fit(x, t, TAU, degree, N, ic, ec)
    lo = np.quantile(want_p, CLAMP, axis=0).astype(F32)
    hi = np.quantile(want_p, 1 - CLAMP, axis=0).astype(F32)
    _set_modes()
    tok = _cond_tok(dev, ic, ec, lo, hi)
    tok.update_times(torch.from_numpy(t.copy()))
    tokens_t, pd = tok.encode(torch.tensor(x).to(dev))
    got = pd["params"].cpu().numpy()
    scale = np.maximum(1.0, np.abs(want_p).max(axis=1, keepdims=True))
    _note(f"conditioned params {name}", (np.abs(got - want_p) / scale).max() / 1e-5)
    assert np.all(np.abs(got - want_p) <= 1e-5 * scale), float((np.abs(got - want_p) / scale).max())
    want_t = _dn_to_nd(O.continuous_to_discrete(O._clamp_t(got, lo, hi), lo, hi, VOCAB), B, D, N)
    assert np.array_equal(tokens_t.cpu().numpy(), want_t)
    assert (got < lo).any() and (got > hi).any()
    pos = tok.reconstruct_traj(tokens_t).cpu().numpy()
    dec = O.decode(want_t, O.Layout.make(D, None, False), N, lo, hi, VOCAB).reshape(B, D, N)
    full = O.cond_full_basis(t, TAU, degree, N, ic, ec)
    ref = O.cond_reconstruct_joint(dec, full, st, ic, ec)
    rscale = np.maximum(1.0, np.abs(ref).max(axis=(1, 2), keepdims=True))
    _note(f"conditioned positions {name}", (np.abs(pos - ref) / rscale).max() / 1e-5)
    assert np.max(np.abs(pos - ref) / rscale) <= 1e-5


# ------------------------------------------------------------------------- staleness --
def _everything(tok, xd, conditioned):
    """Every result that reads a per-grid constant, as a flat list of tensors."""
    tokens, pd = tok.encode(xd)
    out = [tokens, pd["params"]]
    if conditioned:
        out += [v for v in pd.values() if v is not None and v is not pd["params"]]
        out += [tok._cond_state[k] for k in ("params_init", "params_end") if tok._cond_state[k] is not None]
    out.append(tok.reconstruct_traj(tokens))                  # the host fast path, where there is one
    out.append(tok.reconstruct_traj(tokens, init_p=None))     # never the fast path
    out += list(tok.reconstruct_traj_derivs(tokens))
    rs = tok.reconstruction_stats(xd, return_tokens=True)
    out += [v for v in (rs.mse, rs.mean_err, rs.max_abs, rs.mse_fit, rs.clip_low, rs.clip_high, rs.tokens)
            if v is not None]
    return out


@pytest.mark.parametrize("conditioned", [False, True], ids=["plain", "conditioned"])
def test_no_stale_constants_after_update_times(conditioned, kernel_mode, gpu_device):
    """default -> squared -> default at T = 50, then 50 -> 33 -> 50: after every switch the one
    tokenizer gives the bits of a tokenizer freshly constructed on that grid, and trajectories of
    the previous T are refused with the shape error."""
    dev = gpu_device
    degree, N, D = 4, 10, 7
    grip = () if conditioned else (6,)
    cfg50, cfg33 = (degree, N, 50, D, grip), (degree, N, 33, D, grip)
    ref = _ref(K1G, "default", dev)
    lo, hi = ref["lo"], ref["hi"]                      # the same bounds for every grid and both tokenizers

    def make(T):
        if conditioned:
            return _cond_tok(dev, 2, -1, lo, hi, T=T, D=D)
        return _make_tok(dev, D, N, T, VOCAB, degree, list(grip), lo, hi)
    xs = {T: torch.tensor(_trajectories(c, 37)).to(dev) for T, c in ((50, cfg50), (33, cfg33))}
    t50 = load_grid_consts()[(4, 10, 50, "squared")]["times"]
    t33 = load_grid_consts()[(3, 8, 33, "cheb")]["times"]
    tok = make(50)
    steps = [(50, None), (50, t50), (50, "default"), (33, t33), (50, "default")]
    prev_T = None
    for T, g in steps:
        fresh = make(T)
        if isinstance(g, str):
            tok.update_times(torch.linspace(0, 2 * torch.pi, T))
        elif g is not None:
            tok.update_times(torch.from_numpy(g.copy()))
            fresh.update_times(torch.from_numpy(g.copy()))
        got, want = _everything(tok, xs[T], conditioned), _everything(fresh, xs[T], conditioned)
        assert len(got) == len(want)
        for i, (a, b) in enumerate(zip(got, want)):
            assert _bits(a, b), (T, None if g is None else "grid", i)
        if prev_T is not None and prev_T != T:
            with pytest.raises(AssertionError, match="does not match"):
                tok.encode(xs[prev_T])
            with pytest.raises(AssertionError, match="does not match"):
                tok.reconstruction_stats(xs[prev_T])
        prev_T = T


# ----------------------------------------------------------------------------- cache --
def test_constants_cache_does_not_grow(gpu_device):
    """40 rounds of update_times + encode + reconstruct_traj_derivs keep one grid's constants alive:
    the cache holds no more entries and the device no more live bytes after round 40 than after
    round 2 (memory_allocated counts live tensors, not the allocator's pool)."""
    dev = gpu_device
    ref = _ref(K1G, "squared", dev)
    _set_modes()
    tok = _make_tok(dev, 7, 10, 50, VOCAB, 4, [6], ref["lo"], ref["hi"])
    xd = torch.tensor(ref["x"][:37]).to(dev)
    grid = torch.from_numpy(ref["t"].copy()).to(dev)
    seen = {}
    tokens = derivs = None
    for rnd in range(1, 41):
        tok.update_times(grid.clone())
        tokens, _ = tok.encode(xd)
        derivs = tok.reconstruct_traj_derivs(tokens)
        if rnd in (2, 40):
            torch.cuda.synchronize(dev)
            seen[rnd] = (len(tok._basis._cache), torch.cuda.memory_allocated(dev))
    print("cache entries, live bytes after rounds 2 and 40:", seen)
    assert derivs is not None and seen[40][0] <= seen[2][0] == 2
    assert seen[40][1] == seen[2][1]
