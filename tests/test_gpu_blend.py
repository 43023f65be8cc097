"""GPU tests of reconstruct_windows / beast_reconstruct_windows_f32 (csrc/blend.hip): the tokens of a
window table blended back into the frames of a flat buffer.

The per-window values are always ``tok.reconstruct_traj(tokens)`` (existing code, not under test) and
the expected frames the float64 blend of those values by tests/blend_oracle.py (plain loops).  T 50,
N 10, D 7 with one gripper DoF (two basis kinds) and the episode lengths of the windows tests
(R = 310) unless a test says otherwise; bounds are wide and random, so decoded values are normal floats."""
import numpy as np
import pytest
import torch

import blend_oracle as BO
import windows_oracle as WO

pytestmark = pytest.mark.gpu

from beast_tokenizer_amd import BEASTBsplineBPETokenizer, BEASTBsplineTokenizer, _lib  # noqa: E402

T, N, D = 50, 10, 7
EPS = 2.0 ** -24
OFF = WO.offsets_of(WO.episode_lengths(T))
R = OFF[-1]
CW = min(16, max(1, 48 * 1024 // (N * D * 12)))          # windows per chunk: csrc/blend.hip, blend_chunk


def make_tok(dev, grip=True, cls=BEASTBsplineTokenizer, num_dof=D, **kw):
    tok = cls(num_dof=num_dof, num_basis=N, seq_len=T, gripper_indices=[num_dof - 1] if grip else None,
              gripper_zero_order=grip, device=str(dev), **kw)
    g = torch.Generator().manual_seed(3)
    tok.w_min.copy_(-1.0 - torch.rand(tok.w_min.shape, generator=g))
    tok.w_max.copy_(1.0 + torch.rand(tok.w_max.shape, generator=g))
    return tok


def table(tok, stride, pad, off=OFF):
    s, e, _ = tok.window_index(off, stride=stride, pad=pad)
    return s, e


def random_tokens(W, dev, seed, per=N * D):
    return torch.randint(0, 256, (W, per), generator=torch.Generator().manual_seed(seed)).to(dev)


def weights(tok, kind):
    return {"uniform": lambda: tok.blend_weights(), "exp": lambda: tok.blend_weights("exp", m=0.1),
            "first": lambda: tok.blend_weights("first", horizon=8)}[kind]()


def check_against_oracle(out, info, y, s, e, bw, n_rows, fill, rows=None):
    """out [R, D] within (2 C + 2) 2^-24 max_k |y_k| of the float64 blend of y: a C-term fma chain and
    a C-term sum are each within gamma_C = C u / (1 - C u) of their exact values relative to
    sum |b_k y_k| <= den max|y| and to den, one division adds u, and (1 + gamma_C)(1 + u) /
    (1 - gamma_C) - 1 <= (2 C + 2) u for C u << 1, with u = 2^-24.  coverage equal; weight within C u den."""
    want, cov, wt, C, ymax = BO.blend(y, np.asarray(s), np.asarray(e), bw.cpu().numpy(), n_rows, fill)
    got = out.cpu().numpy().astype(np.float64)
    gcov, gwt = info["coverage"].cpu().numpy(), info["weight"].cpu().numpy().astype(np.float64)
    sel = slice(None) if rows is None else rows
    assert info["coverage"].dtype is torch.int32 and np.array_equal(gcov[sel], cov[sel])
    covered = (C > 0)[sel]
    err = np.abs(got[sel] - want[sel])
    bound = (2 * C[sel] + 2) * EPS * ymax[sel]
    assert np.isfinite(want[sel][covered]).all()
    worst = float((err[covered] / np.maximum(bound[covered], 1e-300)).max()) if covered.any() else 0.0
    print(f"worst error / bound {worst:.3f}, max contributors {int(C[sel].max())}")
    assert (err[covered] <= bound[covered]).all(), worst
    if np.isnan(fill):
        assert np.isnan(got[sel][~covered]).all()
    else:
        assert (got[sel][~covered] == np.float32(fill)).all()
    assert (np.abs(gwt[sel] - wt[sel]) <= cov[sel] * EPS * wt[sel]).all() and (gwt[sel][cov[sel] == 0] == 0).all()
    return cov


@pytest.mark.parametrize("blend", ["uniform", "exp", "first"])
@pytest.mark.parametrize("pad", ["edge", "valid"])
@pytest.mark.parametrize("stride", ["1", "3", "T", "T+5"])
def test_blend_equals_the_oracle_of_reconstructed_windows(gpu_device, stride, pad, blend):
    tok = make_tok(gpu_device)
    s, e = table(tok, {"1": 1, "3": 3, "T": T, "T+5": T + 5}[stride], pad)
    tokens = random_tokens(len(s), gpu_device, 11)
    y = tok.reconstruct_traj(tokens).cpu().numpy()
    bw = weights(tok, blend)
    for fill, tables in ((float("nan"), (s, e)), (-3.5, (s.to(gpu_device), e.to(gpu_device)))):
        out, info = tok.reconstruct_windows(tokens, *tables, R, blend=bw, fill=fill, return_tile_counts=True)
        assert out.shape == (R, D) and out.dtype is torch.float32 and info["weight"].shape == (R,)
        cov = check_against_oracle(out, info, y, s, e, bw, R, fill)
        assert int(info["tile_counts"][0]) >= 1
    if stride == "T+5":
        assert (cov == 0).sum() >= 5
    if stride == "1" and pad == "edge" and blend != "first":
        assert cov.max() == T
    # the LLM offset is taken off, blend by name
    if blend == "uniform":
        tok.set_llm_vocab_size(1000)
        out2, _ = tok.reconstruct_windows(tokens + (1000 - tok.vocab_size), s, e, R, fill=-3.5)
        assert torch.equal(out2, out)
        assert torch.equal(tok.reconstruct_windows(tokens, s, e, R, fill=-3.5, respect_llm_vocab_size=False)[0], out)


def test_a_single_contributor_is_reconstruct_traj_bitwise(gpu_device):
    """Stride T, uniform blend: fmaf(1, y, 0) / 1 is exact, so every covered frame is reconstruct_traj's
    sample bit for bit -- from tokens and from normalised params."""
    tok = make_tok(gpu_device)
    s, e = table(tok, T, "edge")
    W = len(s)
    tokens = random_tokens(W, gpu_device, 12)
    params = (torch.rand((W, N * D), generator=torch.Generator().manual_seed(13)) * 2.2 - 1.1).to(gpu_device)
    for y, (out, info) in ((tok.reconstruct_traj(tokens), tok.reconstruct_windows(tokens, s, e, R)),
                           (tok.reconstruct_traj_continuous(params),
                            tok.reconstruct_windows_continuous(params, s, e, R))):
        cov = info["coverage"].cpu()
        assert int(cov.max()) == 1 and int((cov == 0).sum()) == 0      # stride T, edge: every frame once
        want = torch.full((R, D), float("nan"), device=gpu_device)
        for w, (a, b) in enumerate(zip(s.tolist(), e.tolist())):
            n = min(T, b - a)
            want[a:a + n] = y[w, :n]
        assert torch.equal(out, want)
        assert torch.equal(info["weight"], torch.ones(R, device=gpu_device))


def test_zero_weight_samples_are_skipped(gpu_device):
    """A window whose params are NaN, blend "first" with horizon 1: only the window's first frame is NaN;
    every other frame is what it is without the NaN (a zero weight skips, it does not multiply)."""
    tok = make_tok(gpu_device)
    s, e = table(tok, 1, "edge")
    W = len(s)
    params = (torch.rand((W, N * D), generator=torch.Generator().manual_seed(14)) * 2 - 1).to(gpu_device)
    w0 = int(np.searchsorted(s.numpy(), OFF[6] + 20))
    bad = params.clone()
    bad[w0] = float("nan")
    bw = tok.blend_weights("first", horizon=1)
    clean, _ = tok.reconstruct_windows_continuous(params, s, e, R, blend=bw)
    out, info = tok.reconstruct_windows_continuous(bad, s, e, R, blend=bw)
    r = int(s[w0])
    assert bool(torch.isnan(out[r]).all()) and bool(torch.isfinite(clean).all())
    keep = torch.ones(R, dtype=torch.bool, device=gpu_device)
    keep[r] = False
    assert torch.equal(out[keep], clean[keep])
    assert torch.equal(info["coverage"], torch.ones(R, dtype=torch.int32, device=gpu_device))
    # with every weight on, the NaN reaches all the frames the window owns and no other
    out_u, _ = tok.reconstruct_windows_continuous(bad, s, e, R)
    nan_rows = torch.isnan(out_u).any(1).cpu().numpy()
    assert np.array_equal(np.nonzero(nan_rows)[0], np.arange(r, r + min(T, int(e[w0]) - r)))


def test_duplicate_starts_exceed_one_chunk(gpu_device):
    """3 C_w + 1 windows on one start: a row's candidates span four chunks and are summed in table order."""
    tok = make_tok(gpu_device)
    s, e = table(tok, 3, "edge")
    w0 = int(np.searchsorted(s.numpy(), OFF[6] + 30))
    rep = 3 * CW
    s2 = torch.cat([s[:w0], s[w0].repeat(rep), s[w0:]])
    e2 = torch.cat([e[:w0], e[w0].repeat(rep), e[w0:]])
    assert bool((s2[1:] >= s2[:-1]).all()) and int((s2 == s[w0]).sum()) == 3 * CW + 1
    tokens = random_tokens(len(s2), gpu_device, 15)           # every copy has its own tokens
    y = tok.reconstruct_traj(tokens).cpu().numpy()
    for kind in ("uniform", "exp"):
        bw = weights(tok, kind)
        out, info = tok.reconstruct_windows(tokens, s2, e2, R, blend=bw, return_tile_counts=True)
        cov = check_against_oracle(out, info, y, s2, e2, bw, R, float("nan"))
        assert cov.max() >= 3 * CW + 1
        counts = info["tile_counts"].cpu()
        assert int(counts[1]) > 0 and int(counts[0]) >= -(-(3 * CW + 1) // CW)


def test_rows_are_independent_of_the_rest_of_the_table(gpu_device):
    """The long episode alone, its table moved to row 0 and R its own length: the same bits as its rows in
    the call over the whole buffer; and the whole call twice."""
    tok = make_tok(gpu_device)
    s, e = table(tok, 1, "edge")
    tokens = random_tokens(len(s), gpu_device, 16)
    bw = weights(tok, "exp")
    full, info = tok.reconstruct_windows(tokens, s, e, R, blend=bw)
    again, info2 = tok.reconstruct_windows(tokens, s.to(gpu_device), e.to(gpu_device), R, blend=bw)
    assert torch.equal(full, again) and torch.equal(info["weight"], info2["weight"])
    assert torch.equal(info["coverage"], info2["coverage"])
    for ep in (6, 5, 3):
        a, b = OFF[ep], OFF[ep + 1]
        m = (s >= a) & (s < b)
        sub, sinfo = tok.reconstruct_windows(tokens[m.to(gpu_device)], s[m] - a, e[m] - a, b - a, blend=bw)
        assert torch.equal(sub, full[a:b]) and torch.equal(sinfo["weight"], info["weight"][a:b])
        assert torch.equal(sinfo["coverage"], info["coverage"][a:b])
    # a sub-range of the long episode's rows: the windows that can own them, in a buffer cut off behind them
    a, b = OFF[6], OFF[6] + 77
    m = (s >= a) & (s < b)
    sub, _ = tok.reconstruct_windows(tokens[m.to(gpu_device)], s[m] - a, torch.clamp(e[m] - a, max=b - a), b - a, blend=bw)
    # rows whose contributors all start inside [a, b) and end where they end in the whole table
    assert torch.equal(sub, full[a:b])


@pytest.mark.parametrize("which", ["out-of-range", "unsorted"])
def test_bad_device_tables_are_clamped(gpu_device, which):
    """Device tables are not read back: a table wrong by a margin (start < 0, end > R, end <= start) is
    seen through the kernel's clamps, an unsorted one loses windows -- wrong numbers, never a fault.
    The contributors of every row are a subset of the clamped table's."""
    tok = make_tok(gpu_device)
    s, e = table(tok, 3, "edge")
    M = 8
    bad_s, bad_e = s.clone(), e.clone()
    bad_s[s < M] -= M                                  # start < 0
    bad_e[e == R] += M                                 # end > R
    bad_e[:3] = bad_s[:3]                              # an empty window: end is raised to start + 1
    assert int((bad_s < 0).sum()) >= 2 and int((bad_e > R).sum()) >= 2
    if which == "unsorted":
        perm = torch.randperm(len(s), generator=torch.Generator().manual_seed(4))
        bad_s, bad_e = bad_s[perm], bad_e[perm]
    tokens = random_tokens(len(s), gpu_device, 17)
    with pytest.raises(ValueError, match="out of range"):
        tok.reconstruct_windows(tokens, bad_s, bad_e, R)           # a host table is checked instead
    out, info = tok.reconstruct_windows(tokens, bad_s.to(gpu_device), bad_e.to(gpu_device), R)
    assert out.shape == (R, D) and info["coverage"].shape == (R,) and info["weight"].shape == (R,)
    cs, ce = BO.clamp_table(bad_s.numpy(), bad_e.numpy(), R)
    bw = np.ones(T)
    true_cov = np.array([len(c) for c in BO.contributors(cs, ce, T, R, bw)])
    got = info["coverage"].cpu().numpy()
    assert (got >= 0).all() and (got <= true_cov).all()
    if which == "out-of-range":
        # the search runs on the clamped starts, which stay sorted: nothing is lost, and the frames are
        # those of the host-clamped table
        assert np.array_equal(got, true_cov)
        want, _ = tok.reconstruct_windows(tokens, torch.from_numpy(cs), torch.from_numpy(ce), R)
        assert torch.equal(out, want) and bool(torch.isfinite(out[torch.from_numpy(true_cov > 0)]).all())


def test_every_workgroup_takes_a_second_tile(gpu_device):
    """The launch has at most 16 workgroups per compute unit (the launch layer's grid: 2 x at most 8
    resident ones) and a tile is 64 rows, so 32 tiles per CU and a partial one make every workgroup walk
    two tiles or more -- it restages its token image, rewrites its window table and W image and
    re-uses the staged constants.  Bitwise equal to the same entry point on each episode alone
    (2 tiles per CU: one per workgroup), and the oracle on sampled rows."""
    tok = make_tok(gpu_device)
    cus = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    tile, ep_len = 64, 64 * 2 * cus
    off = [ep_len * i for i in range(17)] + [16 * ep_len + 17]
    n_rows = off[-1]
    ntiles = -(-n_rows // tile)
    s = torch.arange(n_rows, dtype=torch.int64, device=gpu_device)          # stride 1, edge
    e = torch.full_like(s, off[-1])
    for a, b in zip(off[:-1], off[1:]):
        e[a:b] = b
    tokens = torch.randint(0, 256, (n_rows, N * D), device=gpu_device)
    bw = weights(tok, "exp")
    for _ in range(2):                                   # cold and warm caches
        out, info = tok.reconstruct_windows(tokens, s, e, n_rows, blend=bw, return_tile_counts=True)
        grid = _lib.last_launch_grid()
        assert 0 < grid and 2 * grid <= ntiles, f"grid {grid} for {ntiles} tiles: no second tile for every workgroup"
    assert n_rows % tile == 17
    for a, b in zip(off[:-1], off[1:]):
        sub, sinfo = tok.reconstruct_windows(tokens[a:b], s[a:b] - a, e[a:b] - a, b - a, blend=bw)
        assert _lib.last_launch_grid() == -(-(b - a) // tile), "a slice's grid is its tile count"
        assert torch.equal(sub, out[a:b]) and torch.equal(sinfo["coverage"], info["coverage"][a:b])
        assert torch.equal(sinfo["weight"], info["weight"][a:b])
    # the oracle on the first tile, a tile of a later pass, the partial last tile and every 4,099th row
    rows = np.unique(np.concatenate([np.arange(tile), np.arange((grid + 1) * tile, (grid + 2) * tile),
                                     np.arange((ntiles - 1) * tile, n_rows), np.arange(0, n_rows, 4099)]))
    sh, eh = s.cpu().numpy(), e.cpu().numpy()
    need = np.unique(np.concatenate([np.arange(max(r - T + 1, 0), r + 1) for r in rows]))
    y = tok.reconstruct_traj(tokens[torch.from_numpy(need).to(gpu_device)]).cpu().numpy()
    check_against_oracle(out, info, y, sh[need], eh[need], bw, n_rows, float("nan"), rows=rows)


# ------------------------------------------------------------------------------- smaller cases --
def test_no_windows(gpu_device):
    tok = make_tok(gpu_device)
    z = torch.zeros(0, dtype=torch.int64)
    out, info = tok.reconstruct_windows(torch.zeros((0, N * D), dtype=torch.int64), z, z, 130, fill=2.5,
                                        return_tile_counts=True)
    assert out.shape == (130, D) and bool((out == 2.5).all())
    assert not info["coverage"].any() and not info["weight"].any() and info["tile_counts"].tolist() == [0, 0]
    out, _ = tok.reconstruct_windows_continuous(torch.zeros((0, N * D)), z.to(gpu_device), z.to(gpu_device), 3)
    assert out.shape == (3, D) and bool(torch.isnan(out).all())
    assert tok.reconstruct_windows(torch.zeros((0, N * D), dtype=torch.int64), z, z, 0)[0].shape == (0, D)


def test_one_basis_kind(gpu_device):
    tok = make_tok(gpu_device, grip=False)
    s, e = table(tok, 3, "edge")
    tokens = random_tokens(len(s), gpu_device, 18)
    y = tok.reconstruct_traj(tokens).cpu().numpy()
    bw = weights(tok, "exp")
    out, info = tok.reconstruct_windows(tokens, s, e, R, blend=bw)
    check_against_oracle(out, info, y, s, e, bw, R, float("nan"))


@pytest.mark.parametrize("dof,nb,seq_len,grip", [(5, 8, 37, None), (20, 10, 50, [3, 11]), (24, 7, 50, [0]),
                                                 (33, 10, 20, None), (64, 16, 37, [0, 63])])
def test_other_shapes(gpu_device, dof, nb, seq_len, grip):
    """The kernel's other instantiations: 8 and 16 (row, DoF) elements per thread (D above 16 and above
    32), each with num_basis 10 (compile-time chain) and another (runtime chain; odd N 7 too); chunks
    of fewer than 16 windows (D 64 x N 16: 4); other K-step counts of reconstruct_traj's chain (N 7,
    8: 2, N 16: 4); and a shape whose reconstruct_traj leaves the matrix cores for the per-row kernel
    (D 64, T 37: n ascending).  Single contributors are bitwise reconstruct_traj's."""
    tok = BEASTBsplineTokenizer(num_dof=dof, num_basis=nb, seq_len=seq_len, gripper_indices=grip,
                                gripper_zero_order=grip is not None, device=str(gpu_device))
    g = torch.Generator().manual_seed(5)
    tok.w_min.copy_(-1.0 - torch.rand(tok.w_min.shape, generator=g))
    tok.w_max.copy_(1.0 + torch.rand(tok.w_max.shape, generator=g))
    off = WO.offsets_of(WO.episode_lengths(seq_len))
    n_rows = off[-1]
    for stride in (3, seq_len):
        s, e = table(tok, stride, "edge", off)
        tokens = random_tokens(len(s), gpu_device, 20 + stride, per=nb * dof)
        y = tok.reconstruct_traj(tokens)
        bw = tok.blend_weights("exp", m=0.2) if stride == 3 else tok.blend_weights()
        out, info = tok.reconstruct_windows(tokens, s, e, n_rows, blend=bw, return_tile_counts=True)
        check_against_oracle(out, info, y.cpu().numpy(), s, e, bw, n_rows, float("nan"))
        if stride == seq_len:
            for w, (a, b) in enumerate(zip(s.tolist(), e.tolist())):
                n = min(seq_len, b - a)
                assert torch.equal(out[a:a + n], y[w, :n])
        else:
            assert int(info["tile_counts"][1]) > 0


def raw_blend(tok, dev, tokens, s, e, n_rows, bw, dst, ndo, out_sr, fill):
    """beast_reconstruct_windows_f32 itself, into a poisoned [n_rows, out_sr] buffer."""
    p = tok._plan()
    buf = torch.full((n_rows, out_sr), 777.0, device=dev)
    cov = torch.full((n_rows,), -1, dtype=torch.int32, device=dev)
    wt = torch.full((n_rows,), -1.0, device=dev)
    sd, ed = s.to(dev), e.to(dev)
    _lib.run("beast_reconstruct_windows_f32", tokens.data_ptr(), None, len(s), tok.num_dof, tok.joint_dof, N,
             tok.vocab_size, 0, p.p_wmn, p.p_wmx, p.p_phi, T, sd.data_ptr(), ed.data_ptr(), n_rows, bw.data_ptr(), fill,
             dst.data_ptr(), ndo, buf.data_ptr(), out_sr, cov.data_ptr(), wt.data_ptr(), None, _lib.stream_of(dev))
    return buf, {"coverage": cov, "weight": wt}


@pytest.mark.parametrize("ndo,out_sr", [(D, D + 5), (D + 4, D + 4), (D + 4, D + 9), (600, 600)])
def test_unnamed_columns_and_row_strides_through_the_c_abi(gpu_device, ndo, out_sr):
    """num_dof_out > D: the columns dof_dst does not name are zeros; out_sr > num_dof_out: the floats
    between two rows are left alone.  600 columns: the tile's image exceeds its LDS budget and the
    kernel stores straight to memory.  The per-window values are beast_reconstruct_f32's at the same
    num_dof_out."""
    tok = make_tok(gpu_device)
    p = tok._plan()
    s, e = table(tok, 3, "edge")
    W = len(s)
    tokens = random_tokens(W, gpu_device, 19)
    dst = torch.tensor([3, 0, ndo - 1, 1, 5, 2, 6] if ndo > D else [3, 0, 4, 1, 5, 2, 6], dtype=torch.int32,
                       device=gpu_device)
    pos = torch.empty((W, T, ndo), device=gpu_device)
    _lib.run("beast_reconstruct_f32", tokens.data_ptr(), W, D, tok.joint_dof, N, tok.vocab_size, 0, p.p_wmn, p.p_wmx,
             p.p_phi, 0, T, dst.data_ptr(), ndo, None, 0, None, None, pos.data_ptr(), None, _lib.stream_of(gpu_device))
    bw = weights(tok, "uniform")
    buf, info = raw_blend(tok, gpu_device, tokens, s, e, R, bw, dst, ndo, out_sr, -2.0)
    named = dst.long()
    check_against_oracle(buf[:, named], info, pos[:, :, named].cpu().numpy(), s, e, bw, R, -2.0)
    unnamed = torch.ones(ndo, dtype=torch.bool, device=gpu_device)
    unnamed[named] = False
    assert bool((buf[:, :ndo][:, unnamed] == 0).all())
    assert bool((buf[:, ndo:] == 777.0).all())


def test_bpe_tokenizer_blends_its_own_ids(gpu_device):
    tok = make_tok(gpu_device, cls=BEASTBsplineBPETokenizer, bpe_vocab_size=400)
    s, e = table(tok, 3, "edge")
    rng = np.random.default_rng(7)
    frames = np.cumsum(rng.normal(0, 0.08, (R, D)), 0).astype(np.float32)
    g = torch.from_numpy(WO.gather_windows(frames, s.numpy(), e.numpy(), T))
    tok.fit_from_trajectories([g], show_progress=False)
    ids, _, mp = tok.encode_windows(torch.from_numpy(frames).to(gpu_device), s, e, return_mp_tokens=True)
    got, info = tok.reconstruct_windows(ids, s, e, R, blend="exp")
    want, winfo = BEASTBsplineTokenizer.reconstruct_windows(tok, mp, s, e, R, blend="exp", respect_llm_vocab_size=False)
    assert torch.equal(got, want) and torch.equal(info["coverage"], winfo["coverage"])
    assert bool(torch.isfinite(got).all())
