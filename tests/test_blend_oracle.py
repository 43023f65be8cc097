"""The yardstick of the blend tests and the index logic of the blend kernel, on a machine without a GPU:

* tests/blend_oracle.py (loops) against a second, independent formulation (a dense [R, W] matrix);
* ``blend_weights("exp")`` against ACT's normalised ``exp(-m i)``;
* csrc/blend_index.h, through the host-only exports ``beast_blend_candidates_host`` and
  ``beast_blend_member_host``, against brute force -- on sorted tables and on garbage: whatever a table
  holds, 0 <= a <= b <= W (the searches index nothing else), and on every table with non-decreasing
  starts no contributor of a row of [r0, r1) lies outside [a, b);
* the same header in a stand-alone program under the host compiler's sanitizers
  (tests/host/blend_index_check.cpp), where a table read outside [0, W) aborts."""
import ctypes as C

import numpy as np
import pytest
import torch

import blend_oracle as BO
import windows_oracle as WO
from beast_tokenizer_amd import BEASTBsplineTokenizer, _lib

T = 50


def tok_cpu(**kw):
    return BEASTBsplineTokenizer(num_dof=7, num_basis=10, seq_len=T, device="cpu", **kw)


@pytest.mark.parametrize("stride", [1, 3, T, T + 5])
@pytest.mark.parametrize("pad", ["edge", "valid"])
@pytest.mark.parametrize("kind", ["uniform", "exp", "first"])
def test_the_loops_agree_with_the_dense_matrix(stride, pad, kind):
    tok = tok_cpu()
    off = WO.offsets_of(WO.episode_lengths(T))
    R = off[-1]
    s, e, _ = WO.window_index_loops(off, T, stride, pad)
    bw = tok.blend_weights(kind, m=0.1, horizon=8).numpy()
    rng = np.random.default_rng(stride)
    y = rng.normal(size=(len(s), T, 3))
    out, cov, wt, Cn, ymax = BO.blend(y, s, e, bw, R, -7.0)
    out2, cov2, wt2 = BO.blend_dense(y, s, e, bw, R, -7.0)
    assert np.array_equal(cov, cov2) and np.array_equal(Cn[:, 0], cov)
    np.testing.assert_allclose(wt, wt2, rtol=1e-13, atol=0)
    np.testing.assert_allclose(out, out2, rtol=1e-12, atol=1e-13)
    assert (out[cov == 0] == -7.0).all() and (ymax[cov == 0] == 0).all()
    if stride == T + 5:
        assert (cov == 0).sum() >= 5
    if stride == 1 and pad == "edge" and kind != "first":
        assert cov.max() == T and cov.min() == 1          # an interior frame of the long episode; a 1-frame episode
    if kind == "first" and stride == 1 and pad == "edge":
        assert cov.max() == 8


def test_nan_in_a_zero_weight_sample_is_skipped_by_the_oracle():
    y = np.zeros((2, 4, 1))
    y[0, 2] = np.nan
    bw = np.array([1.0, 1.0, 0.0, 0.0])
    out, cov, _, _, _ = BO.blend(y, [0, 1], [4, 5], bw, 5, np.nan)
    assert np.isfinite(out[:3]).all() and cov.tolist() == [1, 2, 1, 0, 0] and np.isnan(out[3:]).all()


def test_exp_weights_are_acts_temporal_ensembling():
    """A stride-1 table: frame r's contributors are the chunks started at r - T + 1 .. r, oldest first.
    ACT weights them exp(-m i), i = 0 the oldest, normalised; so does blend_weights("exp") after the
    kernel's division -- on an interior frame and 3 frames into an episode (4 contributors)."""
    m = 0.1
    tok = tok_cpu()
    bw = tok.blend_weights("exp", m=m)
    assert bw.dtype is torch.float32 and bw.shape == (T,) and bw.device.type == "cpu"
    bw = bw.double().numpy()
    off = [0, 3 * T]
    s, e, _ = WO.window_index_loops(off, T, 1, "edge")
    con = BO.contributors(s, e, T, off[-1], bw)
    for r, k in ((2 * T, T), (3, 4)):
        ws = [w for w, _ in con[r]]
        assert ws == sorted(ws) and len(ws) == k and ws[0] == max(0, r - T + 1)
        ours = np.array([bw[t] for _, t in con[r]])
        act = np.exp(-m * np.arange(k))                   # i = 0: the oldest prediction
        np.testing.assert_allclose(ours / ours.sum(), act / act.sum(), rtol=2e-6)
    assert torch.equal(tok.blend_weights(), torch.ones(T))
    assert tok.blend_weights("first", horizon=8).tolist() == [1.0] * 8 + [0.0] * (T - 8)
    for bad in (dict(kind="first"), dict(kind="first", horizon=0), dict(kind="first", horizon=T + 1), dict(kind="x")):
        with pytest.raises(ValueError):
            tok.blend_weights(**bad)


# ----------------------------------------------------------------- csrc/blend_index.h on the host --
def candidates(s, e, R, Tn, r0, r1):
    s = np.ascontiguousarray(s, dtype=np.int64)
    e = np.ascontiguousarray(e, dtype=np.int64)
    a, b = C.c_int64(-1), C.c_int64(-1)
    rc = _lib.load().beast_blend_candidates_host(s.ctypes.data, e.ctypes.data, len(s), R, Tn, r0, r1,
                                                 C.byref(a), C.byref(b))
    assert rc == _lib.BEAST_OK, _lib.load().beast_last_error()
    return a.value, b.value


def member_loops(s, e, R, Tn, r):
    """blend_member, restated: the clamps of windows.hip, then start <= r < start + rows."""
    cs = min(max(s, 0), R - 1)
    ce = min(max(e, cs + 1), R)
    rows = min(Tn, ce - cs)
    return r - cs if cs <= r < cs + rows else -1


def sorted_tables():
    off = WO.offsets_of(WO.episode_lengths(T))
    out = {}
    for stride in (1, 3, T, T + 5):
        s, e, _ = WO.window_index_loops(off, T, stride, "edge")
        out[f"stride{stride}"] = (s, e, off[-1])
    s, e, _ = WO.window_index_loops(off, T, 1, "edge")
    dup = np.sort(np.concatenate([s, np.repeat(s[100:103], 40)]))          # duplicate-heavy
    ends = np.array([e[np.searchsorted(s, v)] for v in dup])
    out["duplicates"] = (dup, ends, off[-1])
    out["one-window"] = (np.array([5]), np.array([9]), 20)
    out["empty"] = (np.zeros(0, np.int64), np.zeros(0, np.int64), 20)
    # sorted, but out of range at both ends: the clamp keeps it sorted
    out["sorted-out-of-range"] = (np.array([-1 << 40, -5, 0, 7, 7, 30, 1 << 40]),
                                  np.array([3, 2, 60, 7, 1 << 41, 31, -9]), 40)
    return out


def garbage_tables():
    rng = np.random.default_rng(5)
    out = {}
    out["shuffled"] = (rng.permutation(300), rng.permutation(300) + 10, 310)
    out["negative-and-huge"] = (rng.integers(-1 << 41, 1 << 41, 257), rng.integers(-1 << 41, 1 << 41, 257), 310)
    out["end-before-start"] = (np.arange(100)[::-1].copy(), np.arange(100)[::-1] - 5, 100)
    out["int64-extremes"] = (np.array([np.iinfo(np.int64).max, np.iinfo(np.int64).min, 0, 3]),
                             np.array([np.iinfo(np.int64).min, np.iinfo(np.int64).max, -1, 2]), 17)
    return out


def row_ranges(R, rng):
    fixed = [(0, 0), (0, R), (R, R), (0, min(64, R)), (max(R - 1, 0), R)] + \
        [(r, min(r + 64, R)) for r in range(0, R, 64)]
    rnd = []
    for _ in range(40):
        r0 = int(rng.integers(0, R + 1))
        rnd.append((r0, int(rng.integers(r0, R + 1))))
    return fixed + rnd


@pytest.mark.parametrize("name", sorted(sorted_tables()))
def test_candidates_hold_every_contributor_of_a_sorted_table(name):
    s, e, R = sorted_tables()[name]
    W = len(s)
    lib = _lib.load()
    rng = np.random.default_rng(1)
    for Tn in (T, 1, 7):
        own = np.array([[member_loops(int(s[w]), int(e[w]), R, Tn, r) for w in range(W)] for r in range(R)]
                       ).reshape(R, W)
        for w in range(0, W, 7):                              # blend_member itself, against its restatement
            for r in range(0, R, 5):
                assert lib.beast_blend_member_host(int(s[w]), int(e[w]), R, Tn, r) == own[r, w]
        cs = np.clip(s, 0, R - 1)
        for r0, r1 in row_ranges(R, rng):
            a, b = candidates(s, e, R, Tn, r0, r1)
            assert 0 <= a <= b <= W
            # the definition, by brute force over the clamped starts
            assert a == int((cs <= r0 - Tn).sum()) and b == int((cs < r1).sum()) if r1 > r0 else True
            ws = np.nonzero((own[r0:r1] >= 0).any(0))[0]
            assert all(a <= w < b for w in ws), (name, Tn, r0, r1, a, b, ws)


@pytest.mark.parametrize("name", sorted(garbage_tables()))
def test_candidates_of_a_garbage_table_stay_inside_it(name):
    s, e, R = garbage_tables()[name]
    W = len(s)
    rng = np.random.default_rng(2)
    lib = _lib.load()
    for Tn in (T, 1, 256):
        for r0, r1 in row_ranges(R, rng):
            a, b = candidates(s, e, R, Tn, r0, r1)
            assert 0 <= a <= b <= W, (name, Tn, r0, r1, a, b)
        for w in range(W):                                    # a member's sample index lies in [0, T)
            for r in (0, R // 2, R - 1):
                t = lib.beast_blend_member_host(int(s[w]), int(e[w]), R, Tn, r)
                assert t == member_loops(int(s[w]), int(e[w]), R, Tn, r) and -1 <= t < Tn


def test_index_header_under_the_host_sanitizers(tmp_path):
    """csrc/blend_index.h in a stand-alone program (tests/host/blend_index_check.cpp) built with the host
    compiler's address and undefined-behaviour sanitizers: the tables are heap arrays of exactly W
    entries, so a read outside [0, W) -- the one way this index logic could fault on a GPU -- aborts."""
    import os
    import shutil
    import subprocess
    from conftest import REPO
    cxx = os.environ.get("CXX") or shutil.which("g++")
    assert cxx, "the host C++ compiler (g++) is needed, as for the oracle"
    exe = str(tmp_path / "blend_index_check")
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", os.path.join(REPO, "beast_tokenizer_amd", "csrc"),
                        os.path.join(REPO, "tests", "host", "blend_index_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-4000:]   # -Wall clean
    for seed in (1, 2):
        r = subprocess.run([exe, str(seed), "300"], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.startswith("ok 300 "), (r.returncode, r.stdout[-500:], r.stderr[-3000:])


def test_host_export_checks_its_arguments():
    lib = _lib.load()
    s = np.zeros(3, np.int64)
    a, b = C.c_int64(), C.c_int64()
    ok = lambda *x: lib.beast_blend_candidates_host(*x)   # noqa: E731
    assert ok(s.ctypes.data, s.ctypes.data, 3, 10, 5, 0, 10, C.byref(a), C.byref(b)) == _lib.BEAST_OK
    assert ok(None, None, 0, 10, 5, 0, 10, C.byref(a), C.byref(b)) == _lib.BEAST_OK and (a.value, b.value) == (0, 0)
    assert ok(s.ctypes.data, s.ctypes.data, 3, 0, 5, 0, 0, C.byref(a), C.byref(b)) == _lib.BEAST_OK
    assert (a.value, b.value) == (0, 0)                       # R == 0: no row, no candidate
    for bad in ((None, s.ctypes.data, 3, 10, 5, 0, 10, C.byref(a), C.byref(b)),
                (s.ctypes.data, s.ctypes.data, 3, 10, 5, 0, 10, None, C.byref(b)),
                (s.ctypes.data, s.ctypes.data, -1, 10, 5, 0, 10, C.byref(a), C.byref(b)),
                (s.ctypes.data, s.ctypes.data, 3, 10, 0, 0, 10, C.byref(a), C.byref(b)),
                (s.ctypes.data, s.ctypes.data, 3, 10, 5, 4, 3, C.byref(a), C.byref(b)),
                (s.ctypes.data, s.ctypes.data, 3, 10, 5, 0, 11, C.byref(a), C.byref(b)),
                (s.ctypes.data, s.ctypes.data, 3, 10, 5, -1, 3, C.byref(a), C.byref(b))):
        assert ok(*bad) == _lib.BEAST_E_INVALID
        assert b"beast_blend_candidates_host" in lib.beast_last_error()
