"""k_encode_stream_list (csrc/codec_stream.h): beast_encode_list_f32 beyond N = 16 or T = 256.

Params against the float64 fit within the params bar, 1e-5 * max(1, row inf-norm), and -- the chunk
being beast_encode_f32's, so the order of summation too -- bitwise those of per-batch calls.  Shapes
are the smallest that reach each branch: the first T and the first N past the resident envelope, both
row tiles of P, both kinds, whole chunks plus a tail off the 4-grid, 16-byte and 4-byte DMA units
(T * row_elems odd; a table entry 4 bytes off), and a workgroup's second and third tile."""
import numpy as np
import pytest
import torch

from beast_tokenizer_amd import BEASTBsplineTokenizer, _lib
from beast_tokenizer_amd.synthetic import synth_trajectories
from oracle import beast_oracle as O

pytestmark = pytest.mark.gpu

TAU, ROWS, NB = np.float32(2 * np.pi), 8, 3   # 3 batches of 8 rows


def _tok(dev, D, N, T, grip):
    return BEASTBsplineTokenizer(num_dof=D, num_basis=N, seq_len=T, gripper_zero_order=bool(grip),
                                 gripper_indices=grip, device=str(dev))


def _encode_list(tok, batches):
    p, (B, T, Din) = tok._plan(), batches[0].shape
    table = torch.tensor([b.data_ptr() for b in batches], dtype=torch.int64, device=p.dev)
    out = torch.full((len(batches) * B, tok.num_dof * tok.num_basis), float("nan"), device=p.dev)
    _lib.run("beast_encode_list_f32", table.data_ptr(), len(batches), B, T, Din, tok.num_dof, tok.joint_dof, p.p_src,
             p.p_proj, tok.num_basis, out.data_ptr(), _lib.raw_stream(p.idx))
    m = _lib.last_codec_launch()
    assert m.family == "encode_dyn" and not m.staged and m.fast and m.waves == 4, m
    return out, m.tile


# (id, T or a function of the chunk TC, N, D, gripper DoFs, floats the middle batch lies off a 16-byte boundary)
CASES = [
    ("t257_n10_odd", 257, 10, 7, None, 0),               # T * row_elems odd: 4-byte DMA units, a one-sample tail
    ("t64_n17_grip", 64, 17, 14, [5, 9], 0),             # the second row tile of P, both kinds, whole chunks only
    ("t300_n24", 300, 24, 7, None, 0),                   # 16-byte units, five chunks: the buffers swap roles per tile
    ("2tc+3_n32", lambda tc: 2 * tc + 3, 32, 14, None, 0),   # both row tiles full, a tail off the 4-grid
    ("t300_n24_unaligned", 300, 24, 7, None, 1),         # one table entry 4 bytes off: that tile alone takes 4-byte units
]


@pytest.mark.parametrize("T,N,D,grip,off", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_encode_list_stream(T, N, D, grip, off, gpu_device):
    dev, nj = gpu_device, D - len(grip or ())
    if callable(T):
        T = T(_lib.load().beast_encode_stream_chunk(4096, D, D, nj, N, 1))
    x = synth_trajectories(NB * ROWS, T, D, seed=200 + T + N, gripper_indices=grip or ())
    t, lay = O.times_grid(2 * np.pi, T), O.Layout.make(D, grip, bool(grip))
    exact = np.concatenate([O.fit_exact(x[..., idx], O.basis(t, TAU, deg, N))
                            for idx, deg in ((lay.joint_indices, 4), (lay.gripper_indices, 0)) if idx], axis=-1)
    tok, per = _tok(dev, D, N, T, grip), ROWS * T * D
    # every batch at its exact size in a NaN-filled buffer: NaN follows each batch's last sample
    flat = torch.full((NB * (per + 4) + 4,), float("nan"), device=dev)
    starts = [i * (per + 4) + (off if i == 1 else 0) for i in range(NB)]
    batches = [flat[s:s + per].view(ROWS, T, D) for s in starts]
    assert [b.data_ptr() % 16 for b in batches] == [0, 4 * off, 0]
    for i, b in enumerate(batches):
        b.copy_(torch.from_numpy(x[i * ROWS:(i + 1) * ROWS]))
    got, _ = _encode_list(tok, batches)
    err = np.abs(got.cpu().numpy() - exact) / np.maximum(1.0, np.abs(exact).max(axis=1, keepdims=True))
    print(f"T={T} N={N} D={D}: max params error / bar = {err.max() / 1e-5:.3f}")
    assert err.max() <= 1e-5
    assert torch.equal(got, torch.cat([tok.compute_weights(b) for b in batches]))
    # NaN right behind a trajectory's last sample (every odd trajectory, and what follows the batch)
    for b in batches:
        b[1::2] = float("nan")
    alt, _ = _encode_list(tok, batches)
    assert torch.equal(alt[0::2], got[0::2]) and bool(torch.isnan(alt[1::2]).all())


def test_encode_list_stream_second_tile(gpu_device):
    """More than twice as many tiles as the grid: every workgroup carries its chunk pipeline over tile
    changes (21 chunks per tile, an odd number, so the two buffers swap roles) and into a new batch,
    with every CU full -- the regime in which a chunk read before another wave's DMA had landed showed
    (a few rows in ten thousand; never in a launch of three tiles)."""
    dev, T, N, D = gpu_device, 1000, 10, 14              # 16-byte DMA units, 20 whole chunks of 48 and a tail
    tok = _tok(dev, D, N, T, None)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    rows = 8 * -(-(12 * cus + 1) // NB)                  # 48 KB of LDS: at most 6 workgroups per CU in the grid
    base = torch.from_numpy(synth_trajectories(64, T, D, seed=9)).to(dev)
    batches = [base.roll(i + 1, 0).repeat(-(-rows // 64), 1, 1)[:rows].contiguous() for i in range(NB)]
    got, tile = _encode_list(tok, batches)
    assert 2 * _lib.last_launch_grid() <= NB * rows // tile
    for i in (0, NB - 1):
        assert torch.equal(got[i * rows:(i + 1) * rows], tok.compute_weights(batches[i]))


def test_fit_parameters_long_shape_takes_list_mode(gpu_device, monkeypatch):
    from beast_tokenizer_amd.bpe_train import no_reduce
    from beast_tokenizer_amd.quantile import column_quantiles
    dev, D, N, T = gpu_device, 7, 24, 300
    tok = _tok(dev, D, N, T, None)
    x = torch.from_numpy(synth_trajectories(76, T, D, seed=5)).to(dev)
    # a ragged batch first (per batch, as before), then four that group into one list launch
    loader = [{"actions": x[:12].clone()}] + [{"actions": x[i:i + 16].clone()} for i in range(12, 76, 16)]
    want = column_quantiles([tok.compute_weights(b["actions"]) for b in loader], [0.01, 0.99], no_reduce)
    calls, run = [], _lib.run
    monkeypatch.setattr(_lib, "run", lambda name, *a: (calls.append(name), run(name, *a))[1])
    tok.fit_parameters(loader, verbose=False)
    assert calls.count("beast_encode_list_f32") == 1
    m = _lib.last_codec_launch()
    assert m.family == "encode_dyn" and not m.staged, m
    assert torch.equal(tok.w_min, want[0].to(tok.w_min.device)) and torch.equal(tok.w_max, want[1].to(tok.w_max.device))
