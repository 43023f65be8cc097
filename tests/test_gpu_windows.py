"""GPU tests of encode_windows / beast_encode_windows_f32 (csrc/windows.hip): encoding the windows of
a flat episode buffer is, bit for bit, ``encode`` of the gathered windows -- tokens and params -- on
either of the kernel's per-tile paths (one staged segment shared by the tile's windows, or a gather
window by window), at every alignment and stride, and with tables the kernel has to clamp.

The expected value is always ``tok.encode(gather_windows(...))`` (tests/windows_oracle.py builds the
windows with plain loops) on the same tokenizer.  The buffers hold a few hundred frames, but for the
two properties that need more: both paths on one table (4,000 frames, so that a shuffled tile's span
exceeds its image) and workgroups that walk several tiles (40,001 windows)."""
import numpy as np
import pytest
import torch

import windows_oracle as WO

pytestmark = pytest.mark.gpu

from beast_tokenizer_amd import BEASTBsplineBPETokenizer, BEASTBsplineTokenizer, _lib  # noqa: E402

# name -> (constructor arguments, columns of the frame buffer)
SHAPES = {
    "d7": (dict(num_dof=7, num_basis=10, seq_len=50), 7),
    # two kinds, gripper columns in the middle (dof_src is a permutation), rows wider than num_dof
    "d14-grippers-16-columns": (dict(num_dof=14, num_basis=10, seq_len=50, gripper_indices=[5, 9],
                                     gripper_zero_order=True), 16),
    "t37-d5-n8": (dict(num_dof=5, num_basis=8, seq_len=37), 5),       # T is no multiple of 4
}


def make_tok(dev, name, cls=BEASTBsplineTokenizer, wide_bounds=True, **kw):
    args, cols = SHAPES[name]
    tok = cls(device=str(dev), **args, **kw)
    if wide_bounds:                       # so that the tokens spread over the bins and some params clamp
        tok.w_min.fill_(-1.5)
        tok.w_max.fill_(1.5)
    return tok, cols, args["seq_len"]


def random_frames(R, cols, seed):
    """A smooth walk plus noise, O(1): neighbouring windows differ, the fit is well inside fp32."""
    rng = np.random.default_rng(seed)
    x = np.cumsum(rng.normal(0, 0.08, (R, cols)), 0) + rng.normal(0, 0.02, (R, cols))
    return np.ascontiguousarray((x - x.mean(0)).astype(np.float32))


def table(tok, off, stride, pad):
    """window_index, with an odd number of windows: no tile width (8, 4, 2) divides it."""
    s, e, _ = tok.window_index(off, stride=stride, pad=pad)
    if len(s) % 2 == 0:
        s, e = s[:-1], e[:-1]
    assert len(s) % 2 == 1
    return s, e


def expected(tok, frames_np, starts, ends, T, dev, **kw):
    g = WO.gather_windows(frames_np, np.asarray(starts), np.asarray(ends), T)
    return tok.encode(torch.from_numpy(g).to(dev), **kw)


def assert_same(got, want):
    assert got[0].dtype is torch.int64 and got[0].shape == want[0].shape
    assert torch.equal(got[0], want[0]), "tokens differ"
    assert torch.equal(got[1]["params"], want[1]["params"]), "params differ"


CASES = {}


def case(name, seed=7):
    """(frames, offsets) of the shape's episode buffer, built once per session."""
    if name not in CASES:
        _, cols = SHAPES[name]
        off = WO.offsets_of(WO.episode_lengths(SHAPES[name][0]["seq_len"]))
        CASES[name] = (random_frames(off[-1], cols, seed), off)
    return CASES[name]


@pytest.mark.parametrize("pad", ["edge", "valid"])
@pytest.mark.parametrize("stride", ["1", "3", "T", "T+5"])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_windows_equal_encode_of_the_gathered_windows(gpu_device, name, stride, pad):
    tok, cols, T = make_tok(gpu_device, name)
    frames, off = case(name)
    s, e = table(tok, off, {"1": 1, "3": 3, "T": T, "T+5": T + 5}[stride], pad)
    want = expected(tok, frames, s, e, T, gpu_device)
    fd = torch.from_numpy(frames).to(gpu_device)
    got = tok.encode_windows(fd, s, e, return_tile_counts=True)
    assert_same(got, want)
    info = got[1]
    assert info["valid"].dtype is torch.int32
    assert torch.equal(info["valid"].cpu(), torch.clamp(e - s, max=T).to(torch.int32))
    W = len(s)
    assert int(info["tile_counts"].sum()) == -(-W // 8)              # every tile counted once
    # device tables, the LLM offset, params only through the continuous form
    tok.set_llm_vocab_size(1000)
    got_d = tok.encode_windows(fd, s.to(gpu_device), e.to(gpu_device))
    assert torch.equal(got_d[0], want[0] + (1000 - tok.vocab_size)) and torch.equal(got_d[1]["params"], want[1]["params"])
    assert torch.equal(tok.encode_windows(fd, s, e, respect_llm_vocab_size=False)[0], want[0])


def test_episode_boundaries_fall_inside_tiles():
    """What the table test relies on: at stride 1 several 8-window tiles hold windows of two or more
    episodes, and W is odd."""
    tok = BEASTBsplineTokenizer(num_dof=7, num_basis=10, seq_len=50, device="cpu")
    _, off = case("d7")
    s, e, ep = tok.window_index(off)
    tiles = [set(ep[i:i + 8].tolist()) for i in range(0, len(ep), 8)]
    assert sum(len(t) > 1 for t in tiles) >= 3 and max(len(t) for t in tiles) >= 3


@pytest.mark.parametrize("view", ["row-offset", "row-strided", "last-stride-2"])
def test_alignment_and_strides(gpu_device, view):
    """D = 7 rows are 28 bytes: ``frames[1:]`` starts 28 bytes into the allocation and no tile's
    segment is 16-byte aligned; a row-strided view has sr > row_elems; a last-stride-2 view is copied."""
    tok, _, T = make_tok(gpu_device, "d7")
    _, off = case("d7")
    R = off[-1]
    if view == "row-offset":
        big = torch.from_numpy(random_frames(R + 1, 7, 11)).to(gpu_device)
        fr = big[1:]
        assert fr.data_ptr() % 16 == 12 and fr.is_contiguous()
    elif view == "row-strided":
        big = torch.from_numpy(random_frames(R, 12, 12)).to(gpu_device)
        fr = big[:, 2:9]
        assert fr.stride() == (12, 1)
    else:
        big = torch.from_numpy(random_frames(R, 14, 13)).to(gpu_device)
        fr = big[:, ::2]
        assert fr.stride() == (14, 2)
    for stride in (1, T + 5):
        s, e = table(tok, off, stride, "edge")
        got = tok.encode_windows(fr, s, e, return_tile_counts=True)
        assert_same(got, expected(tok, fr.cpu().numpy(), s, e, T, gpu_device))
        assert int(got[1]["tile_counts"][0]) > 0       # the shared-segment path ran on this view


def test_both_paths_are_seen_and_agree(gpu_device):
    """A dense stride-1 table over one long episode shares a segment in every tile; the same table
    shuffled gathers (4,000 frames: a tile's 8 random starts hardly ever lie within 8 T = 400 rows), and
    its outputs are the dense run's rows, permuted."""
    tok, cols, T = make_tok(gpu_device, "d7")
    R = 4000
    frames = random_frames(R, cols, 21)
    fd = torch.from_numpy(frames).to(gpu_device)
    s, e, _ = tok.window_index([0, R])
    assert len(s) == R
    dense = tok.encode_windows(fd, s, e, return_tile_counts=True)
    counts = dense[1]["tile_counts"].cpu()
    assert counts[0] > 0 and counts[1] == 0
    assert_same(dense, expected(tok, frames, s, e, T, gpu_device))
    perm = torch.randperm(R, generator=torch.Generator().manual_seed(5))
    shuffled = tok.encode_windows(fd, s[perm], e[perm], return_tile_counts=True)
    c2 = shuffled[1]["tile_counts"].cpu()
    assert c2[1] > 0 and c2.sum() == counts.sum()
    pd = perm.to(gpu_device)
    assert torch.equal(shuffled[0], dense[0][pd]) and torch.equal(shuffled[1]["params"], dense[1]["params"][pd])
    assert torch.equal(shuffled[1]["valid"], dense[1]["valid"][pd])


@pytest.mark.parametrize("shuffled", [False, True])
def test_more_tiles_than_workgroups(gpu_device, shuffled):
    """The launch has at most 16 workgroups per compute unit (the launch layer's grid: 2 x at most 8
    resident ones), so 32 tiles per CU and one window (never fewer than 40,001 windows) make every
    workgroup of the grid walk two tiles or more: it stages the next image over the last one,
    rewrites the window table and re-uses the params image and the quantiser constants.  The grid
    read back after each launch is at most half the tiles.  With 28-byte rows the staged segment's
    phase inside 16 bytes changes from tile to tile too."""
    tok, cols, T = make_tok(gpu_device, "d7")
    R = max(40001, 8 * 32 * torch.cuda.get_device_properties(gpu_device).multi_processor_count + 1)
    ntiles = -(-R // 8)
    frames = random_frames(R, cols, 41)
    s, e, _ = tok.window_index([0, 7000, R])
    if shuffled:
        perm = torch.randperm(R, generator=torch.Generator().manual_seed(8))
        s, e = s[perm], e[perm]
    g = torch.from_numpy(WO.gather_windows_indexed(frames, s.numpy(), e.numpy(), T)).to(gpu_device)
    want = tok.encode(g)
    fd = torch.from_numpy(frames).to(gpu_device)
    for _ in range(3):                                  # cold and warm caches
        got = tok.encode_windows(fd, s, e, return_tile_counts=True)
        grid = _lib.last_launch_grid()
        assert 0 < grid and 2 * grid <= ntiles, f"grid {grid} for {ntiles} tiles: no second tile for every workgroup"
        assert_same(got, want)
    counts = got[1]["tile_counts"]
    assert int(counts.sum()) == ntiles and int(counts[1 if shuffled else 0]) >= ntiles - 20


# T, D, columns, windows per tile: 8 T rows of the image exceed 32 KB, so the launch takes tiles of 4,
# 2 and -- one trajectory alone above 32 KB: gather only, sized by the whole LDS layout -- 1 window
SMALL_TILES = [(100, 14, 14, 4), (200, 14, 16, 2), (256, 64, 64, 1)]


@pytest.mark.parametrize("T,D,cols,tbt", SMALL_TILES)
def test_tiles_of_fewer_than_eight_windows(gpu_device, T, D, cols, tbt):
    """The corners of the envelope (T <= 256, D <= 64): both paths on tiles of 4, 2 and 1 windows."""
    tok = BEASTBsplineTokenizer(num_dof=D, num_basis=10, seq_len=T, device=str(gpu_device))
    tok.w_min.fill_(-1.5)
    tok.w_max.fill_(1.5)
    off = WO.offsets_of([1, T - 1, T + 1, 2 * T + 7] * 3)
    R = off[-1]
    frames = random_frames(R, cols, 51)
    fd = torch.from_numpy(frames).to(gpu_device)
    s, e = table(tok, off, 7, "edge")
    W = len(s)
    want = tok.encode(torch.from_numpy(WO.gather_windows_indexed(frames, s.numpy(), e.numpy(), T)).to(gpu_device))
    dense = tok.encode_windows(fd, s, e, return_tile_counts=True)
    assert_same(dense, want)
    c = dense[1]["tile_counts"]
    assert int(c.sum()) == -(-W // tbt)
    assert (int(c[0]) > 0) == (tbt > 1)                 # one trajectory above 32 KB is never staged as a segment
    perm = torch.randperm(W, generator=torch.Generator().manual_seed(9))
    shuffled = tok.encode_windows(fd, s[perm], e[perm], return_tile_counts=True)
    assert torch.equal(shuffled[0], want[0][perm.to(gpu_device)])
    assert torch.equal(shuffled[1]["params"], want[1]["params"][perm.to(gpu_device)])
    assert int(shuffled[1]["tile_counts"][1]) > 0 and int(shuffled[1]["tile_counts"].sum()) == -(-W // tbt)


def raw_windows(tok, frames, R, sr, sd, row_elems, s, e, dof_src, dev):
    """beast_encode_windows_f32 itself: (tokens, params, tile counts)."""
    T, D, N = int(tok.times.numel()), tok.num_dof, tok.num_basis
    p = tok._plan()
    W = len(s)
    sd_, ed_ = s.to(dev), e.to(dev)
    params = torch.empty((W, D * N), device=dev)
    tokens = torch.empty((W, N * D), dtype=torch.int64, device=dev)
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    _lib.run("beast_encode_windows_f32", frames.data_ptr(), R, sr, sd, row_elems, sd_.data_ptr(), ed_.data_ptr(), W, T,
             D, tok.joint_dof, dof_src.data_ptr(), p.p_proj, N, p.p_wmn, p.p_wmx, tok.vocab_size, 0,
             params.data_ptr(), tokens.data_ptr(), counts.data_ptr(), _lib.stream_of(dev))
    return tokens, params, counts


def test_element_strides_through_the_c_abi(gpu_device):
    """sd = 2 (every second float of 14-float rows) is reachable only through the C-ABI, where it is
    gathered whatever the table; the result is that of the contiguous copy of the same view."""
    tok, _, T = make_tok(gpu_device, "d7")
    _, off = case("d7")
    R = off[-1]
    big = torch.from_numpy(random_frames(R, 14, 61)).to(gpu_device)
    src, _ = tok._dof_maps(gpu_device)
    s, e = table(tok, off, 1, "edge")
    tokens, params, counts = raw_windows(tok, big, R, 14, 2, 7, s, e, src, gpu_device)
    assert counts.tolist() == [0, -(-len(s) // 8)]
    want = expected(tok, big[:, ::2].cpu().numpy(), s, e, T, gpu_device)
    assert torch.equal(tokens, want[0]) and torch.equal(params, want[1]["params"])


def test_out_of_range_columns_are_clamped_on_both_paths(gpu_device):
    """A dof_src entry outside [0, row_elems) (the C-ABI accepts any table) reads the row's first or
    last column, on a tile that shares a segment as on one that gathers."""
    tok, cols, T = make_tok(gpu_device, "d7")
    R = 4000
    frames = random_frames(R, cols, 71)
    fd = torch.from_numpy(frames).to(gpu_device)
    s, e, _ = tok.window_index([0, R], stride=5)
    bad = torch.tensor([0, -3, 2, 99, 4, 7, 6], dtype=torch.int32, device=gpu_device)
    good = torch.tensor([0, 0, 2, 6, 4, 6, 6], dtype=torch.int32, device=gpu_device)
    perm = torch.randperm(len(s), generator=torch.Generator().manual_seed(10))
    for ss, ee, path in ((s, e, 0), (s[perm], e[perm], 1)):
        got = raw_windows(tok, fd, R, cols, 1, cols, ss, ee, bad, gpu_device)
        want = raw_windows(tok, fd, R, cols, 1, cols, ss, ee, good, gpu_device)
        assert int(got[2][path]) > 0 and torch.equal(got[2], want[2])
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    want = tok.encode(torch.from_numpy(WO.gather_windows_indexed(frames[:, good.cpu().numpy()], s.numpy(), e.numpy(), T))
                      .to(gpu_device))
    dense = raw_windows(tok, fd, R, cols, 1, cols, s, e, bad, gpu_device)
    assert torch.equal(dense[0], want[0]) and torch.equal(dense[1], want[1]["params"])


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_scattered_starts_are_gathered(gpu_device, name):
    """The episode buffer four times over (more rows than the 8 T a tile's image holds) and a shuffled
    table: tiles gather window by window, here from rows that lie apart in memory (sr > row_elems)."""
    tok, cols, T = make_tok(gpu_device, name)
    off = WO.offsets_of(WO.episode_lengths(T) * 4)
    R = off[-1]
    assert R > 3 * 8 * T
    big = torch.from_numpy(random_frames(R, cols + 3, 31)).to(gpu_device)
    fr = big[:, 1:1 + cols]
    s, e = table(tok, off, 3, "edge")
    perm = torch.randperm(len(s), generator=torch.Generator().manual_seed(6))
    s, e = s[perm], e[perm]
    got = tok.encode_windows(fr, s, e, return_tile_counts=True)
    assert int(got[1]["tile_counts"][1]) > 0
    assert_same(got, expected(tok, fr.cpu().numpy(), s, e, T, gpu_device))


@pytest.mark.parametrize("which", ["short-windows", "stride-T+5-valid", "stride-1-valid"])
def test_rows_no_window_reads_may_be_nan(gpu_device, which):
    """The gaps of a table that skips rows hold NaN: a read past a window's ``end`` (or before its
    start) that a clamp bug folds into the fit shows as a NaN or as a wrong number.  The short
    windows (10 rows each, 12 apart, so T - 10 samples repeat the last row) share segments in which
    the gap rows ARE staged -- and must not be used."""
    tok, cols, T = make_tok(gpu_device, "d7")
    frames, off = case("d7")
    frames = frames.copy()
    R = off[-1]
    if which == "short-windows":
        s = torch.arange(0, R - 10, 12, dtype=torch.int64)
        e = s + 10
    else:
        s, e = table(tok, off, T + 5 if which == "stride-T+5-valid" else 1, "valid")
    read = np.zeros(R, dtype=bool)
    for a, b in zip(s.tolist(), e.tolist()):
        read[a:min(a + T, b)] = True
    assert (~read).sum() >= 20
    frames[~read] = np.nan
    want = expected(tok, frames, s, e, T, gpu_device)
    got = tok.encode_windows(torch.from_numpy(frames).to(gpu_device), s, e, return_tile_counts=True)
    assert bool(torch.isfinite(got[1]["params"]).all()) and bool(torch.isfinite(want[1]["params"]).all())
    assert_same(got, want)
    if which == "short-windows":
        assert int(got[1]["tile_counts"][0]) > 0 and int(got[1]["valid"].max()) == 10


@pytest.mark.parametrize("name", ["d7", "d14-grippers-16-columns"])
def test_bad_device_tables_are_clamped_into_the_buffer(gpu_device, name):
    """Without any way to fault: ``frames`` is the middle of a larger allocation whose margins hold NaN,
    and the device tables are wrong by at most the margin (start < 0, end > R).  The result is that of
    the host-clamped table -- start into [0, R - 1], end into [start + 1, R] -- and finite."""
    tok, cols, T = make_tok(gpu_device, name)
    frames, off = case(name)
    R, M = off[-1], 8
    big = torch.full((R + 2 * M, cols), float("nan"), device=gpu_device)
    big[M:M + R] = torch.from_numpy(frames).to(gpu_device)
    fr = big[M:M + R]
    s, e = table(tok, off, 3, "edge")
    bad_s, bad_e = s.clone(), e.clone()
    bad_s[s < M] -= M                                  # start < 0
    bad_e[e == R] += M                                 # end > R
    bad_e[:3] = bad_s[:3]                              # an empty window: end is raised to start + 1
    assert int((bad_s < 0).sum()) >= 2 and int((bad_e > R).sum()) >= 2
    cs = bad_s.clamp(0, R - 1)
    ce = torch.minimum(torch.maximum(bad_e, cs + 1), torch.tensor(R))
    with pytest.raises(ValueError, match="out of range"):
        tok.encode_windows(fr, bad_s, bad_e)           # a host table is checked instead
    got = tok.encode_windows(fr, bad_s.to(gpu_device), bad_e.to(gpu_device))
    assert bool(torch.isfinite(got[1]["params"]).all())
    assert_same(got, tok.encode_windows(fr, cs, ce))
    assert_same(got, expected(tok, frames, cs, ce, T, gpu_device))


def test_update_bounds_widens_as_encode_does(gpu_device):
    tok_a, cols, T = make_tok(gpu_device, "d14-grippers-16-columns", wide_bounds=False)
    tok_b, _, _ = make_tok(gpu_device, "d14-grippers-16-columns", wide_bounds=False)
    frames, off = case("d14-grippers-16-columns")
    s, e = table(tok_a, off, 3, "edge")
    before = tok_a.w_min.clone()
    got = tok_a.encode_windows(torch.from_numpy(frames).to(gpu_device), s, e, update_bounds=True)
    want = expected(tok_b, frames, s, e, T, gpu_device, update_bounds=True)
    assert_same(got, want)
    assert torch.equal(tok_a.w_min, tok_b.w_min) and torch.equal(tok_a.w_max, tok_b.w_max)
    assert not torch.equal(tok_a.w_min, before)        # the bounds did move


def test_encode_continuous_windows(gpu_device):
    tok, cols, T = make_tok(gpu_device, "t37-d5-n8")
    frames, off = case("t37-d5-n8")
    s, e = table(tok, off, 3, "edge")
    g = torch.from_numpy(WO.gather_windows(frames, s.numpy(), e.numpy(), T)).to(gpu_device)
    want = tok.encode_continuous(g)
    got = tok.encode_continuous_windows(torch.from_numpy(frames).to(gpu_device), s, e)
    assert got[0].dtype is torch.float32 and torch.equal(got[0], want[0])
    assert torch.equal(got[1]["params"], want[1]["params"])
    assert torch.equal(got[1]["valid"].cpu(), torch.clamp(e - s, max=T).to(torch.int32))


def test_fit_parameters_windows(gpu_device):
    """Several chunks (64 windows each, a ragged last one) give the bounds of fit_parameters over a
    loader of the gathered chunks."""
    tok_a, cols, T = make_tok(gpu_device, "d7", wide_bounds=False)
    tok_b, _, _ = make_tok(gpu_device, "d7", wide_bounds=False)
    frames, off = case("d7")
    s, e = table(tok_a, off, 1, "edge")
    assert len(s) > 4 * 64 and len(s) % 64
    tok_a.fit_parameters_windows(torch.from_numpy(frames).to(gpu_device), s, e, chunk_windows=64)
    g = torch.from_numpy(WO.gather_windows(frames, s.numpy(), e.numpy(), T)).to(gpu_device)
    tok_b.fit_parameters([{"actions": g[i:i + 64]} for i in range(0, len(s), 64)], verbose=False)
    assert torch.equal(tok_a.w_min, tok_b.w_min) and torch.equal(tok_a.w_max, tok_b.w_max)
    assert float((tok_a.w_max - tok_a.w_min).min()) > 0 and not torch.equal(tok_a.w_min, torch.full_like(tok_a.w_min, -0.02))


def test_bpe_tokenizer_encodes_the_same_ids(gpu_device):
    tok, cols, T = make_tok(gpu_device, "d7", cls=BEASTBsplineBPETokenizer, bpe_vocab_size=400)
    frames, off = case("d7")
    fd = torch.from_numpy(frames).to(gpu_device)
    s, e = table(tok, off, 3, "edge")
    g = torch.from_numpy(WO.gather_windows(frames, s.numpy(), e.numpy(), T))
    tok.fit_from_trajectories([g], show_progress=False)
    ids, pd, mp = tok.encode_windows(fd, s, e, return_mp_tokens=True)
    want_ids, want_pd, want_mp = tok.encode(g.to(gpu_device), return_mp_tokens=True)
    assert ids == want_ids and len(ids) == len(s)
    assert torch.equal(mp, want_mp) and torch.equal(pd["params"], want_pd["params"])
    assert tok.encode_windows(fd, s, e, return_tensors=True)[0].to_lists() == ids
