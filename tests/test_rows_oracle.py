"""The float64 per-trajectory fit oracle (tests/rows_oracle.py) against the reference goldens
(tests/golden/gen_rows_goldens.py: learn_mp_params_from_trajs run on row-wise different times)
and against its own properties; no GPU."""
import numpy as np
import pytest

from conftest import load_json, load_npz
from oracle import beast_oracle as O
import rows_oracle as R

TOL = load_json("rows_tolerances.json")
CASES = sorted(TOL)
REF_BUDGET = 5e-6          # the generator's bound on the reference's own error: half of 1e-5


def case_config(name):
    c = TOL[name]["config"]
    grip = sorted(c.get("grippers", []))
    return dict(degree=c["degree"], N=c["N"], T=c["T"], D=c["D"], grippers=grip,
                joint=[d for d in range(c["D"]) if d not in grip], duration=c.get("duration", 2 * np.pi))


def oracle_fit(g, cfg):
    return R.fit(g["x"], g["times"], g.get("weights"), tau=np.float32(cfg["duration"]), degree=cfg["degree"],
                 num_basis=cfg["N"], joint_indices=cfg["joint"], gripper_indices=cfg["grippers"])


def test_every_golden_case_is_there():
    cfgs = [case_config(n) for n in CASES]
    assert any(c["N"] == 10 and c["D"] == 7 and c["degree"] == 4 and c["T"] == 50 for c in cfgs)
    assert any(c["D"] == 14 and c["grippers"] == [6, 13] for c in cfgs)
    assert any(c["N"] == 4 and c["T"] == 10 and c["degree"] == 3 and c["duration"] == 4.0 for c in cfgs)
    assert any(c["N"] == 16 and c["T"] == 50 for c in cfgs)
    assert any("keep" in TOL[n]["config"] for n in CASES)


@pytest.mark.parametrize("name", CASES)
def test_oracle_reproduces_reference_goldens(name):
    g, cfg = load_npz(f"rows_{name}.npz"), case_config(name)
    want, cond = oracle_fit(g, cfg)
    ref = g["ref_params"]
    assert ref.dtype == np.float32 and ref.shape == want.shape == (len(g["x"]), cfg["D"] * cfg["N"])
    # rows really differ in their times
    assert g["times"].shape == g["x"].shape[:2] and np.ptp(g["times"], axis=0).min() > 0
    err = R.parity_err(ref, want)
    assert err <= REF_BUDGET, err
    assert err == pytest.approx(TOL[name]["ref_err"], rel=1e-6, abs=1e-9)
    assert cond.max() == pytest.approx(TOL[name]["max_cond"], rel=1e-6)
    if "weights" in g:       # 0/1 weights with the same number of samples in every row
        keep = TOL[name]["config"]["keep"]
        assert set(np.unique(g["weights"])) == {0.0, 1.0} and (g["weights"].sum(axis=1) == keep).all()


@pytest.mark.parametrize("D,grippers", [(7, []), (14, [6, 13])])
def test_unit_weights_on_the_shared_grid_equal_fit_exact(D, grippers):
    """On the tokenizer's own grid, repeated per row, with unit weights the per-row problem is the
    shared one: the oracle equals beast_oracle.fit_exact up to float64 rounding of two solves."""
    duration, T, N = 2 * np.pi, 50, 10
    joint = [d for d in range(D) if d not in grippers]
    x = R.random_walk(6, T, D, seed=5)
    t = O.times_grid(duration, T)
    got, _ = R.fit(x, np.tile(t, (6, 1)), np.ones((6, T), np.float32), tau=np.float32(duration), degree=4,
                   num_basis=N, joint_indices=joint, gripper_indices=grippers)
    want = O.fit_exact(x[..., joint], O.basis(t, np.float32(duration), 4, N))
    if grippers:
        want = np.concatenate([want, O.fit_exact(x[..., grippers], O.basis(t, np.float32(duration), 0, N))], axis=-1)
    # both are float64 fits rounded once: equal except where the float64 difference straddles an fp32 tie
    assert np.abs(got.astype(np.float64) - want).max() <= 2.0 ** -23 * max(1.0, np.abs(want).max())
    assert (got != want).mean() <= 0.01
    got1, _ = R.fit(x, t, None, tau=np.float32(duration), degree=4, num_basis=N, joint_indices=joint,
                    gripper_indices=grippers)
    assert np.array_equal(got1, got)            # [T] times and weights=None are the same problem


def test_zero_weight_skips_the_sample_and_scales_cancel():
    x = R.random_walk(4, 30, 3, seed=9)
    t = R.jittered_times(4, 30, 2.0, seed=10)
    w = R.keep_mask(4, 30, 20, seed=11)
    kw = dict(tau=np.float32(2.0), degree=3, num_basis=6, joint_indices=[0, 1, 2])
    base, cond = R.fit(x, t, w, **kw)
    xn, tn = x.copy(), t.copy()
    xn[w == 0] = np.nan
    tn[w == 0] = np.nan
    got, _ = R.fit(xn, tn, w, **kw)
    assert np.array_equal(got, base) and np.isfinite(base).all()
    # the compacted problem is the same problem
    sel = np.stack([np.flatnonzero(w[b]) for b in range(4)])
    comp, _ = R.fit(np.take_along_axis(x, sel[..., None], 1), np.take_along_axis(t, sel, 1), None, **kw)
    assert np.abs(comp.astype(np.float64) - base).max() <= 1e-6
    # no weight at all: G = reg I, R = 0
    zero, zc = R.fit(x, t, np.zeros_like(w), **kw)
    assert not zero.any() and np.allclose(zc, 1.0)
    assert cond.shape == (4, 1)


def test_float64_census_has_both_condition_groups():
    """The draw tests/test_gpu_rows.py uses to show that float64 is really used: 128 rows, about
    half the samples kept, at least 16 rows with cond(G) <= 1e3 and 4 with 1e4 <= cond <= 1e6."""
    x, t, w = R.census_inputs()
    _, cond = R.fit(x, t, w, tau=np.float32(2 * np.pi), degree=4, num_basis=10, joint_indices=list(range(7)))
    cond = cond[:, 0]
    assert (cond <= 1e3).sum() >= 16 and ((cond >= 1e4) & (cond <= 1e6)).sum() >= 4, \
        ((cond <= 1e3).sum(), ((cond >= 1e4) & (cond <= 1e6)).sum())


def test_tokens_are_the_tokenizer_s_epilogue():
    rng = np.random.default_rng(2)
    D, N = 3, 4
    p = rng.normal(0, 1, (5, D * N)).astype(np.float32)
    lo, hi = np.full(D * N, -1, np.float32), np.full(D * N, 1, np.float32)
    tok = R.tokens(p, lo, hi, 256, D, N, offset=1000)
    want = O.continuous_to_discrete(np.clip(p, lo, hi), lo, hi, 256).reshape(5, D, N).transpose(0, 2, 1).reshape(5, -1)
    assert np.array_equal(tok, want + 1000) and tok.min() >= 1000 and tok.max() <= 1255
