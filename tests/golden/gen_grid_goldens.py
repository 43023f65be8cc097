"""Writes tests/golden/grid_consts.npz: the spline constants on time grids other than the default.

CPU only; needs mpmath (the tests read the file and never import mpmath).  Run from the repository
root:  python tests/golden/gen_grid_goldens.py   -- the output is the same bytes every time.

Per case (degree, N, T, grid):
  * the fp32 time grid [T];
  * Phi = oracle.beast_oracle.basis(grid, fp32(2 pi), degree, N), fp32 [T, N];
  * P* = (Phi^T Phi + 1e-9 I)^-1 Phi^T from that Phi at 60 decimal digits, rounded once to
    float64, [N, T];
  * two float64 yardsticks, max|P - P*| / max|P*| of
      yard_solve  oracle.beast_oracle.projection_f64 (np.linalg.solve),
      yard_gj     a plain numpy float64 Gauss-Jordan with partial pivoting on [G | I]
                  (a restatement of the method, not of the kernel's code).

Layout of the file (one array per kind of data, the cases concatenated, so that the zip holds six
entries and not four hundred):
  grid_names [9] str; cases [C, 4] int32 = (degree, N, T, index into grid_names), in the order of
  ``all_cases()``; times fp32 [sum T]; phi fp32 [sum T N]; proj float64 [sum N T]; yard float64
  [C, 2] = (yard_solve, yard_gj).  tests/test_gpu_constants.py:load_grid_consts slices it.
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import beast_oracle as O  # noqa: E402

F32 = np.float32
TAU = float(np.float32(2 * np.pi))
REG = 1e-9

GRIDS = {
    "default": lambda lin, T: lin * TAU,
    "squared": lambda lin, T: lin ** 2 * TAU,
    "cheb": lambda lin, T: (0.5 - 0.5 * np.cos(np.pi * lin)) * TAU,
    "reversed": lambda lin, T: lin[::-1] * TAU,
    "overshoot": lambda lin, T: (1.3 * lin - 0.15) * TAU,
    "inner_10_90": lambda lin, T: (0.1 + 0.8 * lin) * TAU,
    "first_half": lambda lin, T: 0.5 * lin * TAU,
    "unit_0_1": lambda lin, T: lin,
    "jitter": lambda lin, T: np.sort(np.random.default_rng(7).uniform(0, 1, T)) * TAU,
}
GRID_NAMES = list(GRIDS)

EVERY_GRID = [(4, 10, 50), (3, 8, 33), (4, 10, 13), (4, 10, 10), (4, 10, 9), (5, 16, 64), (8, 16, 50), (0, 10, 50),
              (1, 4, 7), (4, 5, 128)]
DEFAULT_ONLY = [(0, 1, 1), (0, 1, 5), (4, 5, 257), (2, 16, 16)]


def grid(name, T):
    lin = np.linspace(0, 1, T)
    return np.ascontiguousarray(GRIDS[name](lin, T)).astype(F32)


def all_cases():
    return [(d, n, t, g) for (d, n, t) in EVERY_GRID for g in GRID_NAMES] + \
           [(d, n, t, "default") for (d, n, t) in DEFAULT_ONLY]


def exact_projection(phi):
    """(Phi^T Phi + reg I)^-1 Phi^T at 60 digits from the fp32 Phi, rounded once to float64."""
    import mpmath as mp
    mp.mp.dps = 60
    T, N = phi.shape
    A = mp.matrix([[mp.mpf(float(v)) for v in row] for row in phi])          # exact: fp32 values
    G = A.T * A
    for i in range(N):
        G[i, i] += mp.mpf(REG)                                                # the double 1e-9, exactly
    P = mp.inverse(G) * A.T
    return np.array([[float(P[i, j]) for j in range(T)] for i in range(N)], dtype=np.float64)


def gauss_jordan_projection(phi, reg=REG):
    """float64 Gauss-Jordan with partial pivoting on [G | I], then Ginv Phi^T."""
    p = phi.astype(np.float64)
    N = p.shape[1]
    A = np.concatenate([p.T @ p + reg * np.eye(N), np.eye(N)], axis=1)
    for k in range(N):
        piv = k + int(np.argmax(np.abs(A[k:, k])))
        if piv != k:
            A[[k, piv]] = A[[piv, k]]
        A[k] = A[k] / A[k, k]
        for r in range(N):
            if r != k:
                A[r] = A[r] - A[r, k] * A[k]
    return A[:, N:] @ p.T


def rel(P, exact):
    return float(np.abs(P - exact).max() / np.abs(exact).max())


def write_npz(path, arrays):
    """np.savez_compressed with fixed zip timestamps: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for key, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(a), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    cases, times, phis, projs, yards = [], [], [], [], []
    for degree, N, T, name in all_cases():
        t = grid(name, T)
        phi = O.basis(t, F32(TAU), degree, N)
        exact = exact_projection(phi)
        ys, yg = rel(O.projection_f64(phi, REG), exact), rel(gauss_jordan_projection(phi), exact)
        G = phi.astype(np.float64).T @ phi.astype(np.float64) + REG * np.eye(N)
        print(f"degree {degree} N {N:2d} T {T:3d} {name:12s} cond {np.linalg.cond(G):9.3e} max|P*| "
              f"{np.abs(exact).max():9.3e} yard_solve {ys:9.3e} yard_gj {yg:9.3e}")
        cases.append((degree, N, T, GRID_NAMES.index(name)))
        times.append(t)
        phis.append(phi.reshape(-1))
        projs.append(exact.reshape(-1))
        yards.append((ys, yg))
    out = os.path.join(HERE, "grid_consts.npz")
    write_npz(out, {
        "grid_names": np.array(GRID_NAMES), "cases": np.array(cases, dtype=np.int32),
        "times": np.concatenate(times), "phi": np.concatenate(phis), "proj": np.concatenate(projs),
        "yard": np.array(yards, dtype=np.float64)})
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
