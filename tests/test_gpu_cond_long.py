"""Boundary conditions past the resident envelope: the conditioned projection P' on the streamed encode
kernels and k_cond_add_long (csrc/cond.hip), against the float64 oracle (oracle/beast_oracle.py cond_*)
under the parity contract of the streamed shapes: 1e-5 relative to the per-trajectory maximum."""
import numpy as np
import pytest
import torch

from conftest import load_json
from beast_tokenizer_amd import BEASTBsplineTokenizer, _lib
from beast_tokenizer_amd.synthetic import synth_trajectories
from oracle import beast_oracle as O

pytestmark = pytest.mark.gpu

F32, TAU, VOCAB, B = np.float32, np.float32(2 * np.pi), 256, 9
ORDERS = [(1, 0), (2, 0), (0, 1), (0, -1), (2, 2), (1, -1)]
SHAPES = [(257, 10), (300, 24), (64, 17)]   # first T past the envelope, both past, first N past


def _tok(dev, T, N, D, grip, ic, ec):
    return BEASTBsplineTokenizer(num_dof=D, num_basis=N, seq_len=T, vocab_size=VOCAB, gripper_zero_order=bool(grip),
                                 gripper_indices=grip, init_cond_order=ic, end_cond_order=ec, device=str(dev))


def _close(got, want, axes):
    want = np.asarray(want, dtype=np.float64)
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want).max(axis=axes, keepdims=True))
    print(f"max relative error {err.max():.3e}")
    assert err.max() <= 1e-5, float(err.max())


@pytest.mark.parametrize("D,grip", [(7, None), (14, [6, 13])], ids=["d7", "d14_grip"])
@pytest.mark.parametrize("T,N", SHAPES)
@pytest.mark.parametrize("ic,ec", ORDERS)
def test_encode_reconstruct_match_the_oracle(ic, ec, T, N, D, grip, gpu_device):
    x = synth_trajectories(B, T, D, seed=100 + T + D, gripper_indices=grip or ())
    t, lay = O.times_grid(2 * np.pi, T), O.Layout.make(D, grip, bool(grip))
    nj, phi_g = len(lay.joint_indices), O.basis(t, TAU, 0, N)
    want_p, st = O.cond_fit(x[..., lay.joint_indices], t, TAU, 4, N, ic, ec)
    if grip:
        want_p = np.concatenate([want_p, O.fit_exact(x[..., lay.gripper_indices], phi_g)], axis=-1)
    lo, hi = (np.quantile(want_p, q, axis=0).astype(F32) + F32(s) for q, s in ((0.05, -1e-3), (0.95, 1e-3)))
    tok = _tok(gpu_device, T, N, D, grip, ic, ec)
    tok.load_state_dict({"w_min": lo.tolist(), "w_max": hi.tolist()})
    tokens, pd = tok.encode(torch.from_numpy(x).to(gpu_device))
    _close(pd["params"].cpu().numpy(), want_p, 1)
    for key in ("init_pos", "init_vel", "end_pos", "end_vel"):
        assert (pd[key] is None) == (st[key] is None), key
        if st[key] is not None:
            _close(pd[key].cpu().numpy(), st[key], 1)
    dec = O.decode(tokens.cpu().numpy(), lay, N, lo, hi, VOCAB).reshape(B, D, N)
    ref = np.empty((B, T, D))
    ref[..., lay.joint_indices] = O.cond_reconstruct_joint(dec[:, :nj], O.cond_full_basis(t, TAU, 4, N, ic, ec), st, ic, ec)
    if grip:
        ref[..., lay.gripper_indices] = np.einsum("tn,bdn->btd", phi_g.astype(np.float64), dec[:, nj:].astype(np.float64))
    _close(tok.reconstruct_traj(tokens).cpu().numpy(), ref, (1, 2))


@pytest.mark.parametrize("D,joints", [(14, [0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12]), (7, list(range(7)))], ids=["d14", "d7"])
@pytest.mark.parametrize("nb", [1, 9])
@pytest.mark.parametrize("ic,ec", [(2, 2), (1, -1)])
def test_cond_add_kernels_give_the_same_bits(ic, ec, nb, D, joints, gpu_device):
    """beast_cond_add_f32 at T = 256 (k_cond_add) and T = 272 (k_cond_add_long) on the same rows: the same bits
    for t < 256, gripper columns untouched.  D = 7: chunks start off a 16-byte boundary, so the scalar ends run."""
    dev, C, dj = gpu_device, 20, len(joints)
    g = torch.Generator(device=dev).manual_seed(7)
    full, pos, p_init, p_end, ip = (torch.randn(s, device=dev, generator=g) for s in (
        (272, C), (nb, 272, D), (nb, dj, ic), (nb, dj, abs(ec)), (nb, dj)))
    jidx, out = torch.tensor(joints, dtype=torch.int32, device=dev), {}
    for T in (256, 272):
        out[T] = pos[:, :T].clone()
        _lib.run("beast_cond_add_f32", out[T].data_ptr(), nb, T, D, jidx.data_ptr(), dj, full.data_ptr(), 0, C, ic, ec,
                 p_init.data_ptr(), p_end.data_ptr(), ip.data_ptr(), _lib.stream_of(dev))
    grip = [d for d in range(D) if d not in joints]
    assert torch.equal(out[256], out[272][:, :256]) and torch.equal(out[272][..., grip], pos[..., grip])


@pytest.mark.parametrize("ic,ec", [(2, 2), (1, -1)])
def test_old_envelope_projection_is_the_dense_one(ic, ec, gpu_device, tmp_path):
    """constants()'s P' is bitwise P_eff (I - Dfit^T) by T unit trajectories; tokens survive a save / load."""
    T, N, D, dev = 50, 10, 7, gpu_device
    tok = _tok(dev, T, N, D, None, ic, ec)
    b, times = tok._basis, tok.times.to(dev, torch.float32).reshape(-1)
    phi, got, _ = tok._constants(dev)
    want = torch.zeros_like(got)                  # P_eff: the ridge projection of the N fitted columns
    _lib.run("beast_bspline_projection_f64", phi[0].data_ptr(), T, N, b.reg, want[0].data_ptr(), _lib.stream_of(dev))
    eye = torch.eye(T, dtype=torch.float64, device=dev)[:, :, None]
    pi, _, _, _, p_init, p_end = b.fixed_ctrl(eye, (times[1] - times[0]).to(torch.float64))
    d = b.fixed_term(b.full_basis_at(times).to(torch.float64), p_init, p_end, pi, fit=True)[..., 0]
    want[0, :, :T] = want[0, :, :T] - want[0, :, :T] @ d.T
    assert torch.equal(got, want)
    x = torch.from_numpy(synth_trajectories(B, T, D, seed=3)).to(dev)
    tok.update_weights_bounds(x)
    tok.save_pretrained(tmp_path)
    assert torch.equal(BEASTBsplineTokenizer.from_pretrained(tmp_path, device=str(dev)).encode(x)[0], tok.encode(x)[0])


def test_long_horizon_api(gpu_device):
    """List-mode fit_parameters over four batches of 16: P' reaches the list kernel, the bounds are the
    quantiles of the per-batch params, bitwise.  The composed reconstruction_stats returns."""
    T, N, D, dev = 300, 24, 14, gpu_device
    tok = _tok(dev, T, N, D, [6, 13], 2, 2)
    x = torch.from_numpy(synth_trajectories(64, T, D, seed=11, gripper_indices=[6, 13])).to(dev)
    batches = [x[i:i + 16].clone() for i in range(0, 64, 16)]
    assert tok._listable(batches[0], [])
    tok.fit_parameters([{"actions": b} for b in batches], verbose=False)
    params = np.concatenate([tok.encode_continuous(b)[1]["params"].cpu().numpy() for b in batches])
    for q, got in ((0.01, tok.w_min), (0.99, tok.w_max)):
        assert np.array_equal(got.cpu().numpy(), np.quantile(params, F32(q), axis=0).astype(F32))
    stats = tok.reconstruction_stats(x[:B])
    assert stats.mse_fit is None and stats.mse.shape == (B, D) and bool(torch.isfinite(stats.mse).all())


def test_chunk_continuity_at_a_long_horizon(gpu_device):
    """To test_boundary_velocity_is_the_encoded_condition's tolerance: the reconstruction's first sample is the
    encoded init_pos, and the reconstructed spline's velocity there (the derivative basis at times[0] on its
    control points: the stored fixed ones, then the decoded params) is the encoded init_vel."""
    T, N, D, dev = 300, 24, 7, gpu_device
    tol = max(4 * load_json("deriv_tolerances.json")["cond_d4_2_0"]["vel_ref_err"], 16 * 2.0 ** -24)
    tok = _tok(dev, T, N, D, None, 2, 0)
    x = torch.from_numpy(synth_trajectories(B, T, D, seed=5)).to(dev)
    tok.update_weights_bounds(x)
    tokens, pd = tok.encode(x)
    pos = tok.reconstruct_traj(tokens).double()
    ctrl = torch.cat([tok._cond_state["params_init"], tok.decode(tokens).reshape(B, D, N)], dim=-1).double()
    dfull = tok._basis.full_deriv_basis_at(tok.times.to(dev).reshape(-1)[:1], 1).double()
    for got, want in ((pos[:, 0], pd["init_pos"].double()), (ctrl @ dfull[0], pd["init_vel"].double())):
        err = float((got - want).abs().max() / want.abs().max())
        print(f"err {err:.3e} bound {tol:.3e}")
        assert err <= tol, (err, tol)
