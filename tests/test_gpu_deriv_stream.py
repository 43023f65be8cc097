"""k_reconstruct_derivs_stream: shared order slabs too large for the resident kernel's LDS, streamed in
chunks of RC = beast_reconstruct_derivs_stream_rows() output rows.

Every case is placed on RC (T_out = RC + 1, 2 RC or 3 RC - 1: one full and one 1-row chunk, two full
chunks, an odd count with a partial last one) and checks
  1. every element against the float64 product of the same fp32 slabs (DeviceBasis.deriv_basis_at) and
     the decoded fp32 params, to the dot product's own bound (N + 1) 2^-24 sum_n |basis w|
     (test_gpu_derivs' bound for raw launches); columns whose bound is 0 are exact zeros;
  2. the first 40 rows bitwise against a launch on times[:40], which the resident kernel serves.
The shapes pair (N, D, n_joint) with the order sets so that RC + 1 leaves the resident path and
3 RC - 1 stays inside T_out <= 4096: a single order at N <= 10 would give RC > 1365."""
import pytest
import torch

from beast_tokenizer_amd import BEASTBsplineTokenizer, _lib

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
SHAPES = {   # N, D, gripper columns, orders
    "n10": (10, 7, (), (0, 1, 2)),                       # NP 12 > N: the padding columns' DMA lanes
    "n16_pos_acc": (16, 14, (6, 13), (0, 2)),            # NP == N: 16-byte DMA units; the kind-1 slab
    "n16_vel": (16, 14, (6, 13), (1,)),                  # gripper DoFs: zeros, no kind-1 slab staged
    "n5": (5, 3, (), (0, 1, 2)),
}
T_OUT = {"rc+1": lambda rc: rc + 1, "2rc": lambda rc: 2 * rc, "3rc-1": lambda rc: 3 * rc - 1}
CASES = [(s, t, B, "") for s in SHAPES for t in T_OUT for B in (1, 5)]
# B from the CU count, so that the tiles alone fill the GPU: a workgroup walks whole time axes, chunk by
# chunk through both buffers, and then a second tile (of 16 trajectories; of 4 in the smallest such batch)
CASES += [("n5", "rc+1", 16, "second_tile"), ("n5", "3rc-1", 4, "second_tile"),
          ("n16_pos_acc", "3rc-1", 4, "second_tile"), ("n10", "rc+1", 4, "second_tile"), ("n10", "2rc", 5, "init_p"),
          ("n16_pos_acc", "3rc-1", 5, "ctypes")]         # num_dof_out > D, outputs 4 bytes off 16


def launch(tok, tokens, t, orders, init_p, dst, ndo, raw):
    """The requested orders [B, T, ndo] and the launch's grid; raw: through ctypes into outputs that start
    4 bytes past a 16-byte boundary (element stores), else through the tokenizer."""
    if not raw:
        outs = tok.reconstruct_traj_derivs(tokens, times=t, orders=orders, init_p=init_p)
        return outs, _lib.last_launch_grid()
    p, B = tok._plan(), tokens.shape[0]
    slabs, _, T = tok._deriv_basis_for(t, B, p, orders)
    bufs = [torch.full((B * T * ndo + 1,), float("nan"), device=t.device)[1:] if o in orders else None for o in range(3)]
    _lib.run("beast_reconstruct_derivs_f32", tokens.data_ptr(), B, tok.num_dof, tok.joint_dof, tok.num_basis, 256, 0,
             p.p_wmn, p.p_wmx, slabs.data_ptr(), 0, T, dst.data_ptr(), ndo, None, 0, None, *map(_lib.ptr, bufs),
             None, None)
    return [bufs[o].reshape(B, T, ndo) for o in orders], _lib.last_launch_grid()


@pytest.mark.parametrize("shape,t_sel,B,opt", CASES, ids=["-".join(map(str, c)).rstrip("-") for c in CASES])
def test_streamed_derivs(shape, t_sel, B, opt, gpu_device):
    dev = gpu_device
    N, D, grip, orders = SHAPES[shape]
    nj, mask = D - len(grip), sum(1 << o for o in orders)
    raw = opt == "ctypes"
    ndo = D + 3 if raw else D
    rc = _lib.load().beast_reconstruct_derivs_stream_rows(4096, D, nj, N, ndo, mask)
    T = T_OUT[t_sel](rc)
    assert rc > 0 and T <= 4096 and _lib.load().beast_reconstruct_derivs_stream_rows(T, D, nj, N, ndo, mask) == rc
    assert _lib.load().beast_reconstruct_derivs_stream_rows(40, D, nj, N, ndo, mask) == 0
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    if opt == "second_tile":                             # two tiles per CU and a partial one
        tile = B
        B = tile * 2 * cus + 1
    tok = BEASTBsplineTokenizer(num_dof=D, num_basis=N, seq_len=50, vocab_size=256, degree_p=4,
                                gripper_zero_order=bool(grip), gripper_indices=list(grip) or None, device=str(dev))
    gen = torch.Generator().manual_seed(N * 100 + T + B)
    tok.w_min.copy_(-torch.rand(tok.w_min.shape, generator=gen) - 0.5)
    tok.w_max.copy_(torch.rand(tok.w_max.shape, generator=gen) + 0.5)
    tokens = torch.randint(0, 256, (B, N * D), generator=gen).to(dev)
    init_p = torch.randn((B, D), generator=gen).to(dev) if opt == "init_p" else None
    t = torch.linspace(0, float(tok.duration), T, device=dev)
    cols = tok.joint_indices + tok.gripper_indices       # output column of DoF d
    if raw:
        cols = torch.randperm(ndo, generator=gen)[:D].tolist()
    dst = torch.tensor(cols, dtype=torch.int32, device=dev)

    outs, grid = launch(tok, tokens, t, orders, init_p, dst, ndo, raw)
    if opt == "second_tile":                             # one workgroup per CU at the full LDS budget
        assert 0 < grid and 2 * grid <= -(-B // tile), f"grid {grid} for {-(-B // tile)} tiles proves no second tile"
    elif B == 1:
        assert grid > 1, "one trajectory must be split over time"
    head, _ = launch(tok, tokens, t[:40], orders, init_p, dst, ndo, raw)

    w = tok.decode(tokens).reshape(B, D, N).double()
    if init_p is not None:
        w[:, :nj, 0] = init_p[:, tok.joint_indices].double()
    for o, got, first in zip(orders, outs, head):
        want = torch.zeros((B, T, ndo), dtype=torch.float64, device=dev)
        mag = torch.zeros_like(want)
        slab = tok._basis.deriv_basis_at(t, o).double()  # [kinds, T, N]
        for d in range(D):
            kind = int(d >= nj)
            if not (o and kind):                         # gripper DoFs: derivatives 0
                want[:, :, cols[d]] = torch.einsum("tn,bn->bt", slab[kind], w[:, d])
                mag[:, :, cols[d]] = torch.einsum("tn,bn->bt", slab[kind].abs(), w[:, d].abs())
        err, tol = (got.double() - want).abs(), (N + 1) * EPS * mag
        print(f"{shape} {t_sel} B {B} {opt} order {o}: RC {rc} T_out {T} grid {grid} "
              f"worst err / bound {float((err / tol.clamp_min(1e-300)).max()):.3f}")
        assert not torch.isnan(got).any() and (err <= tol).all(), (o, float((err - tol).max()))
        assert not got[mag == 0].any()
        assert torch.equal(got[:, :40], first), o
