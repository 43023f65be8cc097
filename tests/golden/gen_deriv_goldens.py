"""Generate tests/golden/deriv_*.npz and deriv_tolerances.json (velocity / acceleration goldens).

Needs the reference checkout, which the test machines do not have:
``BEAST_REFERENCE=<reference root> python tests/golden/gen_deriv_goldens.py``.  From it come
``mp_pytorch`` (MPFactory.init_mp, UniformBSpline.learn_mp_params_from_trajs / update_inputs /
get_traj_pos / get_traj_vel) and ``beast.utils`` (continuous_to_discrete /
discrete_to_continuous), imported as tests/golden/gen_goldens.py imports them; the tokenizer's
glue (DoF split, (d n) -> (n d)) is restated here.  scipy.interpolate.BSpline cross-checks the
oracle.  Outputs are data only.

Per case: the inputs (trajectories, tokens, bounds, times, init_p, the stored condition
tensors), the reference's fp32 get_traj_pos / get_traj_vel, and tests/deriv_oracle.py's float64
orders 0, 1, 2.  get_traj_acc is NOT recorded: it is not the second derivative (tau (p-1)/p
times it on uniform knot spans).  Gripper DoFs (degree 0) have velocity 0 by definition; the reference recurses
without end there, so its columns are written as 0.

Before writing, the generator asserts that the oracle equals scipy's BSpline.derivative to 1e-12
(relative, away from interior knots) and that it equals the reference's velocity to the
yardstick of deriv_tolerances.json: per case the reference's own fp32 velocity error
(``vel_ref_err``) and the error of the oracle run in float32 for order 2 (``acc_f32_err``), both
max|x - oracle_f64| / max|oracle_f64|.  The GPU tests hold the kernel to 4x these, floor 16 * 2^-24.
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
from scipy.interpolate import BSpline  # noqa: E402
from mp_pytorch.mp import MPFactory  # noqa: E402
from beast.utils import continuous_to_discrete, discrete_to_continuous  # noqa: E402

import deriv_oracle as O  # noqa: E402
from beast_tokenizer_amd.synthetic import synth_trajectories  # noqa: E402

B, VOCAB, SEQ = 4, 256, 50
TWO_PI = float(2 * torch.pi)


def knot_grid(degree, n_ctrl, tau):
    """Times below 0, above tau, on every knot (exactly, in fp32, when tau is a power of two)
    and between the knots."""
    kv = np.unique(O.knots(degree, n_ctrl, np.float32))
    mid = (kv[1:] + kv[:-1]) / 2
    u = np.concatenate([[-0.25, -0.01], kv, mid, [1.01, 1.5]]).astype(np.float32)
    rng = np.random.default_rng(3)
    return (rng.permutation(u) * np.float32(tau)).astype(np.float32)


CASES = {
    "d4_n10_d7": dict(degree=4, N=10, D=7),
    "init_p": dict(degree=4, N=10, D=7, init_p=True),
    "grip_d14": dict(degree=4, N=10, D=14, grippers=[6, 13]),
    "cond_d3_1_1": dict(degree=3, N=10, D=7, ic=1, ec=1),
    "cond_d4_2_0": dict(degree=4, N=10, D=7, ic=2, ec=0),
    "cond_d4_2_m1": dict(degree=4, N=10, D=7, ic=2, ec=-1),
    "d1_n4": dict(degree=1, N=4, D=3, duration=4.0, grid=True),
    "d2_n4": dict(degree=2, N=4, D=3, duration=4.0, grid=True),
    "d4_grid": dict(degree=4, N=10, D=7, grid=True),
}


def scipy_check(degree, n_ctrl, tau, times):
    """oracle basis == scipy's, orders 0..2, away from interior knots."""
    kv = O.knots(degree, n_ctrl)
    u = O.phase(times, tau)
    keep = ~np.isin(u, kv[(kv > 0) & (kv < 1)])
    for order in range(3):
        got = O.deriv_basis(times, tau, degree, n_ctrl, order)[keep]
        if order > degree:
            assert not got.any()
            continue
        spl = BSpline(kv, np.eye(n_ctrl), degree)
        want = (spl.derivative(order) if order else spl)(u[keep]) / float(np.float32(tau)) ** order
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (degree, n_ctrl, order)


def make_mp(dj, N, degree, duration, ic=0, ec=0):
    return MPFactory.init_mp(mp_type="uni_bspline", device="cpu", num_dof=dj, tau=duration,
                             mp_args=dict(num_basis=N, degree_p=degree, init_condition_order=ic,
                                          end_condition_order=ec, dt=0.01))


def run_case(name, cfg):
    degree, N, D = cfg["degree"], cfg["N"], cfg["D"]
    duration, ic, ec = cfg.get("duration", TWO_PI), cfg.get("ic", 0), cfg.get("ec", 0)
    grip = sorted(cfg.get("grippers", []))
    joint = [d for d in range(D) if d not in grip]
    dj = len(joint)
    mp = make_mp(dj, N, degree, duration, ic, ec)
    gmp = make_mp(len(grip), N, 0, duration) if grip else None
    grid = torch.linspace(0, duration, SEQ)

    def fit(x):
        xt = torch.from_numpy(x)
        t = grid.expand(x.shape[0], SEQ)
        w = mp.learn_mp_params_from_trajs(t, xt[..., joint])["params"]
        if gmp is not None:
            w = torch.cat([w, gmp.learn_mp_params_from_trajs(t, xt[..., grip])["params"]], dim=-1)
        return w

    # bounds: 1 % / 99 % quantiles of a larger batch's params, as fit_parameters takes them
    wfit = fit(synth_trajectories(256, SEQ, D, seed=1, gripper_indices=grip)).numpy()
    w_min = torch.from_numpy(np.quantile(wfit, 0.01, 0).astype(np.float32))
    w_max = torch.from_numpy(np.quantile(wfit, 0.99, 0).astype(np.float32))
    x = synth_trajectories(B, SEQ, D, seed=11, gripper_indices=grip)
    params = fit(x)                         # the MP object now holds this batch's conditions
    tok_dn = continuous_to_discrete(torch.clamp(params, min=w_min, max=w_max), min_val=w_min, max_val=w_max,
                                    num_bins=VOCAB)
    tokens = tok_dn.reshape(B, D, N).permute(0, 2, 1).reshape(B, N * D)          # (d n) -> (n d)
    dec = discrete_to_continuous(tok_dn, min_val=w_min, max_val=w_max, num_bins=VOCAB).reshape(B, D, N).clone()
    init_p = None
    if cfg.get("init_p"):
        init_p = torch.from_numpy(x[:, 0, :] + np.float32(0.05))
        dec[:, :dj, 0] = init_p[:, joint]                                          # reference :505-510
    times = torch.from_numpy(knot_grid(degree, N + ic + abs(ec), duration)) if cfg.get("grid") else grid
    T = times.numel()
    tb = times.expand(B, T)

    mp.update_inputs(times=tb, params=dec[:, :dj].reshape(B, -1))
    ref_pos, ref_vel = torch.zeros(B, T, D), torch.zeros(B, T, D)
    ref_pos[..., joint] = mp.get_traj_pos()
    ref_vel[..., joint] = mp.get_traj_vel()
    if gmp is not None:
        gmp.update_inputs(times=tb, params=dec[:, dj:].reshape(B, -1))
        ref_pos[..., grip] = gmp.get_traj_pos()

    cond = {k: getattr(mp, k) for k in ("init_pos", "init_vel", "end_pos", "end_vel", "params_init", "params_end")}
    cond = {k: v.numpy() for k, v in cond.items() if v is not None and (ic or ec)}
    if "end_pos" in cond and "init_pos" in cond:      # encode returns the absolute end position
        cond["end_pos"] = cond["end_pos"] + cond["init_pos"]
    decn, tn = dec.numpy(), times.numpy()
    ctrl = O.control_points(decn[:, :dj].astype(np.float64), ic, ec, cond.get("params_init"), cond.get("params_end"))
    scipy_check(degree, ctrl.shape[-1], duration, tn)
    out = {"x": x, "tokens": tokens.numpy(), "w_min": w_min.numpy(), "w_max": w_max.numpy(), "times": tn,
           "ref_pos": ref_pos.numpy(), "ref_vel": ref_vel.numpy()}
    if init_p is not None:
        out["init_p"] = init_p.numpy()
    out.update({"cond_" + k: v for k, v in cond.items()})
    f32 = {}
    for order in range(3):
        for dt, dst in ((np.float64, out), (np.float32, f32)):
            o = np.zeros((B, T, D), dtype=dt)
            o[..., joint] = O.trajectory(tn, duration, degree, ctrl, order,
                                         init_pos=cond.get("init_pos") if ic else None, dtype=dt)
            if order == 0 and grip:
                o[..., grip] = O.trajectory(tn, duration, 0, decn[:, dj:], 0, dtype=dt)
            dst[f"oracle{order}"] = o
    tol = {"config": {k: v for k, v in cfg.items()}, "vel_ref_err": None, "acc_f32_err": None,
           "pos_ref_err": O.rel_err(out["ref_pos"], out["oracle0"])}
    assert tol["pos_ref_err"] <= 1e-5, (name, tol)
    if degree >= 1:
        tol["vel_ref_err"] = O.rel_err(out["ref_vel"], out["oracle1"])
        assert tol["vel_ref_err"] <= 64 * 2.0 ** -24, (name, tol)    # the oracle IS the reference's velocity
    if degree >= 2:
        tol["acc_f32_err"] = O.rel_err(f32["oracle2"], out["oracle2"])
    np.savez_compressed(os.path.join(HERE, f"deriv_{name}.npz"), **out)
    print(name, tol)
    return tol


if __name__ == "__main__":
    torch.set_num_threads(4)
    tols = {name: run_case(name, cfg) for name, cfg in CASES.items()}
    with open(os.path.join(HERE, "deriv_tolerances.json"), "w") as f:
        json.dump(tols, f, indent=1, sort_keys=True)
