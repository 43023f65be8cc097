"""Generate tests/golden/rows_*.npz and rows_tolerances.json (per-trajectory time grids).

Needs the reference checkout, which the test machines do not have:
``BEAST_REFERENCE=<reference root> python tests/golden/gen_rows_goldens.py``.  From it comes
``mp_pytorch`` (MPFactory.init_mp, UniformBSpline.learn_mp_params_from_trajs, mp/uni_bspline.py:
471-602), imported as tests/golden/gen_goldens.py imports it, and called with ``times`` that
differ from row to row.  Outputs are data only.

Per case: the inputs (random-walk trajectories, times jittered by +-0.4 grid steps, weights where
the case has them) and the reference's fp32 params in the tokenizer's (d n) order, joint DoFs
then gripper DoFs.  The reference has no sample weights: the 0/1-weight case records the
reference run on the compacted [B, T_kept, D] trajectories and times, the same least-squares
problem.  rows_tolerances.json holds, per case, the configuration and ``ref_err``: the
reference's own error against tests/rows_oracle.py, max |ref - oracle| / max(1, |oracle row|_inf).
The generator asserts ref_err <= 5e-6, half the project's parity criterion of 1e-5, so a GPU
result within 5e-6 of the oracle is within 1e-5 of the reference.
"""
from __future__ import annotations

import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ["BEAST_REFERENCE"]
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REF, "MP_lite_PyTorch"))
sys.path.insert(0, REF)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from mp_pytorch.mp import MPFactory  # noqa: E402

import rows_oracle as R  # noqa: E402

B = 8
TWO_PI = float(2 * torch.pi)
REF_BUDGET = 5e-6

CASES = {
    "n10_d7": dict(degree=4, N=10, T=50, D=7),
    "n10_d14_grip": dict(degree=4, N=10, T=50, D=14, grippers=[6, 13]),
    "n4_t10_deg3": dict(degree=3, N=4, T=10, D=3, duration=4.0),
    "n16_t50": dict(degree=4, N=16, T=50, D=7),
    # the reference's fp32 LU error grows with cond(G): 45 of 50 samples and |y| <~ 1 keep it in budget
    "mask_keep45": dict(degree=4, N=10, T=50, D=7, keep=45, start=0.5),
}


def make_mp(dof, N, degree, duration):
    return MPFactory.init_mp(mp_type="uni_bspline", device="cpu", num_dof=dof, tau=duration,
                             mp_args=dict(num_basis=N, degree_p=degree, init_condition_order=0,
                                          end_condition_order=0, dt=0.01))


def reference_fit(x, times, joint, grip, N, degree, duration):
    xt, tt = torch.from_numpy(x), torch.from_numpy(times)
    w = make_mp(len(joint), N, degree, duration).learn_mp_params_from_trajs(tt, xt[..., joint])["params"]
    if grip:
        wg = make_mp(len(grip), N, 0, duration).learn_mp_params_from_trajs(tt, xt[..., grip])["params"]
        w = torch.cat([w, wg], dim=-1)
    return w.numpy()


def run_case(name, cfg, seed):
    degree, N, T, D = cfg["degree"], cfg["N"], cfg["T"], cfg["D"]
    duration = cfg.get("duration", TWO_PI)
    grip = sorted(cfg.get("grippers", []))
    joint = [d for d in range(D) if d not in grip]
    x = R.random_walk(B, T, D, seed, start=cfg.get("start", 1.0))
    times = R.jittered_times(B, T, duration, seed + 1)
    out = {"x": x, "times": times}
    weights = None
    if "keep" in cfg:
        weights = R.keep_mask(B, T, cfg["keep"], seed + 2)
        out["weights"] = weights
        sel = np.stack([np.flatnonzero(weights[b]) for b in range(B)])            # [B, keep], sorted
        xc = np.take_along_axis(x, sel[..., None], axis=1)
        tc = np.take_along_axis(times, sel, axis=1)
        ref = reference_fit(xc, tc, joint, grip, N, degree, duration)
    else:
        ref = reference_fit(x, times, joint, grip, N, degree, duration)
    want, cond = R.fit(x, times, weights, tau=np.float32(duration), degree=degree, num_basis=N,
                       joint_indices=joint, gripper_indices=grip)
    assert ref.dtype == np.float32 and ref.shape == want.shape
    err = R.parity_err(ref, want)
    assert err <= REF_BUDGET, (name, err)
    out["ref_params"] = ref
    np.savez_compressed(os.path.join(HERE, f"rows_{name}.npz"), **out)
    tol = {"config": cfg, "ref_err": err, "max_cond": float(cond.max()), "max_abs_param": float(np.abs(want).max())}
    print(name, tol)
    return tol


if __name__ == "__main__":
    torch.set_num_threads(4)
    tols = {name: run_case(name, cfg, 100 + 10 * i) for i, (name, cfg) in enumerate(CASES.items())}
    with open(os.path.join(HERE, "rows_tolerances.json"), "w") as f:
        json.dump(tols, f, indent=1, sort_keys=True)
