"""window_index against the brute-force table of tests/windows_oracle.py, LeRobot's clamp rule
written out, and the window counts' closed forms.  No GPU."""
import numpy as np
import pytest
import torch

import windows_oracle as WO
from beast_tokenizer_amd import BEASTBsplineTokenizer

T = 50
STRIDES = [1, 3, T, T + 5]
PADS = ["edge", "valid"]


def tok(seq_len=T):
    return BEASTBsplineTokenizer(num_dof=7, num_basis=10, seq_len=seq_len, device="cpu")


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("seq_len", [T, 37])
def test_window_index_equals_the_loops(seq_len, stride, pad):
    stride = stride if seq_len == T else {T: seq_len, T + 5: seq_len + 5}.get(stride, stride)
    off = WO.offsets_of(WO.episode_lengths(seq_len))
    want = WO.window_index_loops(off, seq_len, stride, pad)
    for table in (off, torch.tensor(off), np.asarray(off)):
        got = tok(seq_len).window_index(table, stride=stride, pad=pad)
        assert len(got) == 3
        for g, w in zip(got, want):
            assert g.dtype is torch.int64 and g.device.type == "cpu"
            assert np.array_equal(g.numpy(), w)


@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("pad", PADS)
def test_counts_match_the_closed_forms(stride, pad):
    lengths = WO.episode_lengths(T)
    _, _, episode = tok().window_index(WO.offsets_of(lengths), stride=stride, pad=pad)
    got = np.bincount(episode.numpy(), minlength=len(lengths))
    for n, L in zip(got, lengths):
        if pad == "edge":
            assert n == -(-L // stride)                       # ceil(L / stride)
        else:
            assert n == (0 if L < T else (L - T) // stride + 1)


@pytest.mark.parametrize("stride", STRIDES)
def test_edge_padding_is_lerobots_clamp_rule(stride):
    """LeRobot's dataset: the sample at frame i of an episode [ep_start, ep_end) with delta indices
    0 .. T-1 reads frames max(ep_start, min(ep_end - 1, i + delta)) and marks i + delta >= ep_end as
    padding."""
    off = WO.offsets_of(WO.episode_lengths(T))
    frames = np.arange(off[-1], dtype=np.int64)[:, None]          # a frame's value is its row
    starts, ends, episode = (x.numpy() for x in tok().window_index(off, stride=stride, pad="edge"))
    rows = WO.gather_windows(frames, starts, ends, T)[:, :, 0]
    w = 0
    for e in range(len(off) - 1):
        ep_start, ep_end = off[e], off[e + 1]
        for i in range(ep_start, ep_end, stride):
            query = [max(ep_start, min(ep_end - 1, i + delta)) for delta in range(T)]
            is_pad = [(i + delta < ep_start) | (i + delta >= ep_end) for delta in range(T)]
            assert (starts[w], ends[w], episode[w]) == (i, ep_end, e)
            assert rows[w].tolist() == query
            assert T - sum(is_pad) == min(T, ends[w] - starts[w])
            w += 1
    assert w == len(starts)


def test_valid_windows_never_pad():
    off = WO.offsets_of(WO.episode_lengths(T))
    starts, ends, _ = tok().window_index(off, stride=3, pad="valid")
    assert len(starts) and bool((starts + T <= ends).all())


def test_empty_tables_and_bad_arguments():
    for off in ([0], [5], [0, 0, 0]):
        got = tok().window_index(off)
        assert all(g.shape == (0,) and g.dtype is torch.int64 for g in got)
    t = tok()
    for bad in ([], [0, 5, 3], [-1, 4], [0.0, 4.0], [[0, 4]]):
        with pytest.raises(ValueError, match="episode_offsets"):
            t.window_index(bad)
    with pytest.raises(ValueError, match="stride"):
        t.window_index([0, 4], stride=0)
    with pytest.raises(ValueError, match="pad"):
        t.window_index([0, 4], pad="zero")


def test_the_indexed_gather_is_the_loops():
    off = WO.offsets_of(WO.episode_lengths(T))
    frames = np.random.default_rng(0).normal(size=(off[-1], 3)).astype(np.float32)
    for stride, pad in ((1, "edge"), (3, "edge"), (T + 5, "valid")):
        s, e, _ = WO.window_index_loops(off, T, stride, pad)
        assert np.array_equal(WO.gather_windows_indexed(frames, s, e, T), WO.gather_windows(frames, s, e, T))
