"""Brute-force oracle of the window tables and of the windows themselves: plain loops and numpy,
no torch op of the code under test.

A window is (start, end) in rows of a flat [R, D] frame buffer; its sample t is row
min(start + t, end - 1)."""
import numpy as np


def episode_lengths(T):
    """The episode lengths every windows test concatenates: empty, shorter than, equal to and longer
    than a window, and one of several windows with a ragged tail."""
    return [0, 1, 2, T - 1, T, T + 1, 3 * T + 7]


def offsets_of(lengths):
    off = [0]
    for n in lengths:
        off.append(off[-1] + n)
    return off


def window_index_loops(offsets, T, stride, pad):
    """(starts, ends, episode) as int64 arrays, one Python loop iteration per window."""
    starts, ends, episode = [], [], []
    for e in range(len(offsets) - 1):
        lo, hi = offsets[e], offsets[e + 1]
        s = lo
        while s < hi:
            if pad == "edge" or s + T <= hi:
                starts.append(s)
                ends.append(hi)
                episode.append(e)
            s += stride
    return (np.asarray(starts, dtype=np.int64), np.asarray(ends, dtype=np.int64), np.asarray(episode, dtype=np.int64))


def gather_windows(frames, starts, ends, T):
    """[W, T, D]: window w's sample t is frames[min(starts[w] + t, ends[w] - 1)]."""
    frames = np.asarray(frames)
    out = np.empty((len(starts), T) + frames.shape[1:], dtype=frames.dtype)
    for w, (s, e) in enumerate(zip(starts, ends)):
        for t in range(T):
            out[w, t] = frames[min(int(s) + t, int(e) - 1)]
    return out


def gather_windows_indexed(frames, starts, ends, T):
    """gather_windows by one numpy index (for tables of many thousand windows; test_windows_oracle.py
    holds it to the loops)."""
    starts, ends = np.asarray(starts, dtype=np.int64), np.asarray(ends, dtype=np.int64)
    idx = np.minimum(starts[:, None] + np.arange(T, dtype=np.int64)[None, :], ends[:, None] - 1)
    return np.asarray(frames)[idx]
