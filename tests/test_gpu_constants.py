"""The two kernels every fused codec kernel takes its constants from (csrc/fit.hip), by themselves:
k_basis / k_basis_deriv at every compiled degree, and k_projection against the exact projection.

Fixture: tests/golden/grid_consts.npz (tests/golden/gen_grid_goldens.py) -- per (degree, N, T, grid)
the fp32 grid, Phi, the projection P* = (Phi^T Phi + 1e-9 I)^-1 Phi^T from 60-digit arithmetic and
the error of two float64 eliminations against it.

Contracts:
  * basis: bitwise the reference's fp32 recursion (oracle.beast_oracle.basis) at degree 0..8;
  * derivative basis, degree 3 and 5..8: test_gpu_derivs' rule, err <= max(4 yard, 16 * 2^-24) with
    yard the fp32 run of the float64 oracle;
  * projection: max|P_gpu - P*| / max|P*| <= 8 max(yard_solve, yard_gj, N 2^-52).  Two correct
    float64 eliminations differ from each other by up to 7x on these systems (the near-dependent
    ones, T <= N and degree 8 on an inner grid, reach 2.8e-8), so the kernel may be 8x the worse of
    the two; N 2^-52 is the floor where both are exact (degree 0).  Padding rows and columns are
    exact zeros, nothing is written past 16 * Tp doubles, and two runs give the same bits.
"""
import numpy as np
import pytest
import torch

from conftest import load_npz
import deriv_oracle as DO
from oracle import beast_oracle as O
from test_gpu_derivs import basis_times, bound, run_basis
from beast_tokenizer_amd import _lib
from beast_tokenizer_amd.bspline import knot_vector

F32 = np.float32
TAU = float(F32(2 * np.pi))
REG = 1e-9
SENTINEL = -7777.0

_CONSTS = {}


def load_grid_consts():
    """{(degree, N, T, grid name): dict(times [T], phi [T, N], proj [N, T], yard_solve, yard_gj)} in
    the generator's order; shared among the tests and never modified."""
    if not _CONSTS:
        z = load_npz("grid_consts.npz")
        names = [str(s) for s in z["grid_names"]]
        t0 = e0 = 0
        for (degree, N, T, g), (ys, yg) in zip(z["cases"].tolist(), z["yard"].tolist()):
            c = dict(times=z["times"][t0:t0 + T], phi=z["phi"][e0:e0 + T * N].reshape(T, N),
                     proj=z["proj"][e0:e0 + N * T].reshape(N, T), yard_solve=ys, yard_gj=yg)
            for a in (c["times"], c["phi"], c["proj"]):
                a.setflags(write=False)
            _CONSTS[(degree, N, T, names[g])] = c
            t0, e0 = t0 + T, e0 + T * N
        assert t0 == z["times"].size and e0 == z["phi"].size == z["proj"].size
    return _CONSTS


def grid_names():
    return list(dict.fromkeys(k[3] for k in load_grid_consts()))


def shapes():
    return list(dict.fromkeys(k[:3] for k in load_grid_consts()))


def fixture_times():
    """Every grid of the fixture once (each name at each T), concatenated."""
    seen = {}
    for (_, _, T, name), c in load_grid_consts().items():
        seen.setdefault((name, T), c["times"])
    return np.concatenate(list(seen.values()))


# ------------------------------------------------------------------------- fixture --
def test_fixture_is_the_oracle_s():
    """Without a GPU: the stored Phi is oracle.beast_oracle.basis of the stored grid, the default
    grid is linspace(0, 1, T) * fp32(2 pi), and P* solves its own normal equations to float64 rounding."""
    consts = load_grid_consts()
    assert len(consts) == 10 * 9 + 4 and len(grid_names()) == 9
    for (degree, N, T, name), c in consts.items():
        assert c["times"].dtype == F32 and c["phi"].dtype == F32 and c["proj"].dtype == np.float64
        assert np.array_equal(c["phi"], O.basis(c["times"], F32(TAU), degree, N)), (degree, N, T, name)
        if name == "default":
            assert np.array_equal(c["times"], (np.linspace(0, 1, T) * TAU).astype(F32))
        p = c["phi"].astype(np.float64)
        G = p.T @ p + REG * np.eye(N)
        res = np.abs(G @ c["proj"] - p.T).max()
        assert res <= 64 * N * 2.0 ** -52 * np.abs(G).max() * np.abs(c["proj"]).max(), (degree, N, T, name, res)


# --------------------------------------------------------------------------- basis --
DEGREE_NCTRL = [(d, n) for d in range(9) for n in sorted({d + 1, d + 2, 10, 16}) if n >= d + 1]


@pytest.mark.gpu
@pytest.mark.parametrize("degree,n_ctrl", DEGREE_NCTRL)
def test_basis_bitwise_every_degree(degree, n_ctrl, gpu_device):
    """All nine instantiations of k_basis, n_ctrl = degree + 1 (no interior knot), degree + 2, 10
    and 16: bitwise the reference's recursion below 0, above tau, on every knot (tau = 2, so the fp32
    phase hits them), between them, and on every grid of the fixture at tau = fp32(2 pi)."""
    for tau, tn in ((2.0, basis_times(degree, n_ctrl, 2.0)), (TAU, fixture_times())):
        got = run_basis(torch.from_numpy(tn).to(gpu_device), tau, degree, n_ctrl, None, "beast_bspline_basis_f32")
        want = O.basis(tn, F32(tau), degree, n_ctrl)
        diff = got.view(np.uint32) != want.view(np.uint32)
        assert not diff.any(), (degree, n_ctrl, tau, int(diff.sum()), float(np.abs(got - want).max()))


@pytest.mark.gpu
@pytest.mark.parametrize("degree,n_ctrl", [(d, n) for d, n in DEGREE_NCTRL if d in (3, 5, 6, 7, 8)])
def test_basis_deriv_remaining_degrees(degree, n_ctrl, gpu_device):
    """Orders 1 and 2 of the degrees test_gpu_derivs leaves out, by its rule and with its exclusion
    of tau = 2 pi times whose fp32 and float64 phase fall on different sides of a knot."""
    for tau in (2.0, TAU):
        tn = basis_times(degree, n_ctrl, tau)
        if tau != 2.0:
            kv = np.unique(knot_vector(degree, n_ctrl).numpy().astype(np.float64))
            tn = tn[np.abs(DO.phase(tn, tau)[:, None] - kv[None, 1:-1]).min(axis=1, initial=1.0) > 1e-6]
        t = torch.from_numpy(tn).to(gpu_device)
        assert np.array_equal(run_basis(t, tau, degree, n_ctrl, 0),
                              run_basis(t, tau, degree, n_ctrl, None, "beast_bspline_basis_f32"))
        for order in (1, 2):
            got = run_basis(t, tau, degree, n_ctrl, order)
            want = DO.deriv_basis(tn, tau, degree, n_ctrl, order)
            yard = DO.rel_err(DO.deriv_basis(tn, tau, degree, n_ctrl, order, dtype=np.float32), want)
            err = DO.rel_err(got, want)
            print(f"degree {degree} C {n_ctrl} tau {tau:.3f} order {order}: err {err:.3e} f32 oracle {yard:.3e} "
                  f"ratio {err / bound(yard):.3f}")
            assert err <= bound(yard), (degree, n_ctrl, tau, order, err, yard)


# ---------------------------------------------------------------------- projection --
def run_projection(phi, dev):
    """One beast_bspline_projection_f64 call into a sentinel-filled buffer of 16 Tp + 8 doubles."""
    T, N = phi.shape
    Tp = (T + 3) // 4 * 4
    d_phi = torch.tensor(phi).to(dev)
    buf = torch.full((16 * Tp + 8,), SENTINEL, dtype=torch.float64, device=dev)
    _lib.run("beast_bspline_projection_f64", d_phi.data_ptr(), T, N, REG, buf.data_ptr(), None)
    torch.cuda.synchronize()
    return buf.cpu().numpy(), Tp


def projection_bound(c, N):
    return 8 * max(c["yard_solve"], c["yard_gj"], N * 2.0 ** -52)


@pytest.mark.gpu
@pytest.mark.parametrize("degree,N,T", shapes())
def test_projection_against_the_exact_one(degree, N, T, gpu_device):
    """N = 1 and 16, T = 1, T = N, T < N (the regulariser decides), T = 257 (more steps than
    threads), grids that leave basis columns empty (first_half, unit_0_1)."""
    worst = (-1.0, "")
    for (d, n, t, name), c in load_grid_consts().items():
        if (d, n, t) != (degree, N, T):
            continue
        buf, Tp = run_projection(c["phi"], gpu_device)
        again, _ = run_projection(c["phi"], gpu_device)
        assert np.array_equal(buf.view(np.uint64), again.view(np.uint64)), name     # one workgroup, no atomics
        assert np.all(buf[16 * Tp:] == SENTINEL), name
        P = buf[:16 * Tp].reshape(16, Tp)
        assert not P[N:].any() and not P[:, T:].any(), name
        exact = c["proj"]
        err = float(np.abs(P[:N, :T] - exact).max() / np.abs(exact).max())
        tol = projection_bound(c, N)
        print(f"degree {degree} N {N} T {T} {name}: err {err:.3e} yard_solve {c['yard_solve']:.3e} "
              f"yard_gj {c['yard_gj']:.3e} err/bound {err / tol:.3f}")
        worst = max(worst, (err / tol, name))
        assert err <= tol, (degree, N, T, name, err, c["yard_solve"], c["yard_gj"])
    print(f"degree {degree} N {N} T {T}: worst err/bound {worst[0]:.3f} ({worst[1]})")
    assert worst[1]
