"""The BPE training kernels (csrc/bpe_setup.hip, csrc/bpe_loop.hip) one operation at a time.

Every test calls one C-ABI entry point and compares, exactly, with a plain reference of that one
operation: numpy, ``tests/cpu_ops.py:NumpyBpeOps`` or ``tests/bpe_ops_oracle.py``.  Every output
and every workspace is the payload of a sentinel-filled allocation of exactly the size the header
(or the ``*_workspace_bytes`` query) gives, and the guard elements on both sides must be intact
afterwards.  Launch branches and second trips of the grid-stride loops are proved through
``_lib.last_launch_grid()``; where gridDim.x cannot tell two kernel forms apart, the test restates
the host formula that chooses.  The last part runs the product's host-driven loop with the GPU
and the numpy ops in lockstep (``CheckedOps``), so a mismatch names the merge and the kernel.
"""
import numpy as np
import pytest
import torch

import bpe_ops_oracle as BO
from beast_tokenizer_amd import _lib
from beast_tokenizer_amd.bpe_train import GpuBpeOps, build_alphabet, fixed_rows_to_device, train_bpe
from cpu_ops import NumpyBpeOps

pytestmark = pytest.mark.gpu

GUARD = 64          # guard elements on either side of a payload
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
SENTINEL = {torch.uint8: 0xA5, torch.int16: 0x5AA5, torch.int32: 0x5AA5A55A, torch.int64: 0x5AA5A55A5AA5A55A}


def cdiv(a, b):
    return -(-a // b)


def cu_count(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


class Guarded:
    """``n`` elements between two guards of GUARD sentinel elements.  ``init`` None fills the
    payload with the sentinel too (an output the kernel must write), else with that value or array."""

    def __init__(self, n, dtype, dev, init=None):
        self.n, self.s = int(n), SENTINEL[dtype]
        self.full = torch.full((self.n + 2 * GUARD,), self.s, dtype=dtype, device=dev)
        self.t = self.full[GUARD:GUARD + self.n]
        if init is not None and self.n:
            if isinstance(init, np.ndarray):
                self.t.copy_(torch.from_numpy(np.ascontiguousarray(init)).view(dtype).reshape(-1))
            else:
                self.t.fill_(init)
        self.ptr = self.full.data_ptr() + GUARD * self.full.element_size()   # valid for n == 0 too

    def np(self):
        """The payload on the host, after checking both guards."""
        h = self.full.cpu().numpy()
        assert (h[:GUARD] == self.s).all(), "the guard before the buffer was written"
        assert (h[GUARD + self.n:] == self.s).all(), "the guard after the buffer was written"
        return h[GUARD:GUARD + self.n].copy()


def dv(a, dev):
    """A host array on the device; never empty, so its pointer is never null."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a if a.size else np.zeros(1, dtype=a.dtype)).to(dev)


class Inputs:
    """Host arrays copied to the device for one call: ``ins(a)`` is the device pointer, and the
    tensors live as long as ``ins`` does (a temporary would hand its block to the next copy)."""

    def __init__(self, dev):
        self.dev, self.kept = dev, []

    def __call__(self, a):
        self.kept.append(dv(a, self.dev))
        return self.kept[-1].data_ptr()


def stream(dev):
    return _lib.stream_of(dev)


def grid_is(want, what):
    g = _lib.last_launch_grid()
    assert g == want, f"{what}: gridDim.x {g}, expected {want}"


# ------------------------------------------------------------- beast_exclusive_scan_i64 --
def run_scan(x, dev):
    ins = Inputs(dev)
    n = x.size
    ws = Guarded(_lib.load().beast_scan_workspace_bytes(n), torch.uint8, dev)
    out = Guarded(n + 1, torch.int64, dev)
    _lib.run("beast_exclusive_scan_i64", ins(x), out.ptr, n, ws.ptr, stream(dev))
    torch.cuda.synchronize()
    ws.np()
    return out.np()


@pytest.mark.parametrize("n", [0, 1, 2, 1023, 1024, 1025, 2500, 1024 ** 2 - 1, 1024 ** 2, 1024 ** 2 + 1])
def test_scan_matches_cumsum(n, gpu_device):
    """A tile is 1,024 elements: one level up to 1,024, two up to 1,024^2 (k_scan_add once), three
    above (k_scan_add on the tile sums as well).  Values below 2^40: the sums cross 32 bits."""
    x = np.random.default_rng(n).integers(0, 2 ** 40, size=n, dtype=np.int64)
    got = run_scan(x, gpu_device)
    want = np.concatenate([[0], np.cumsum(x)]).astype(np.int64)
    assert np.array_equal(got, want)
    assert got[n] == int(x.sum())


def test_scan_negative_values(gpu_device):
    x = np.random.default_rng(1).integers(-2 ** 40, 2 ** 40, size=2500, dtype=np.int64)
    assert (x < 0).any()
    assert np.array_equal(run_scan(x, gpu_device), np.concatenate([[0], np.cumsum(x)]))


# --------------------------------------------------------------------- beast_i64_minmax --
@pytest.mark.parametrize("last", ["min_last", "max_last"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, BO.N_MINMAX_BIG])
def test_minmax_extremes_at_the_end(n, last, gpu_device):
    """INT64_MIN / INT64_MAX at the last index (the other one just before it, from n = 2).  At
    n = 2048 * 256 + 1 the grid is capped at 2,048 workgroups of 256, so the last index is read
    only by workgroup 0's second trip; both orders put each extreme there once."""
    ins = Inputs(gpu_device)
    x = np.random.default_rng(n).integers(-2 ** 62, 2 ** 62, size=n, dtype=np.int64)
    lo_hi = (I64_MIN, I64_MAX) if last == "min_last" else (I64_MAX, I64_MIN)
    x[n - 1] = lo_hi[0]
    if n >= 2:
        x[n - 2] = lo_hi[1]
    out = Guarded(2, torch.int64, gpu_device)
    _lib.run("beast_i64_minmax", ins(x), n, out.ptr, stream(gpu_device))
    torch.cuda.synchronize()
    grid_is(min(cdiv(n, 256), 2048), "k_minmax")
    if n == BO.N_MINMAX_BIG:
        assert _lib.last_launch_grid() == 2048 and 2048 * 256 == n - 1
    assert out.np().tolist() == [int(x.min()), int(x.max())]


# ---------------------------------------------------------------- beast_bpe_cp_presence --
def run_presence(tok, n, mn, n_cp, dev):
    ins = Inputs(dev)
    pr = Guarded(n_cp, torch.uint8, dev)
    _lib.run("beast_bpe_cp_presence", ins(tok), n, mn, pr.ptr, n_cp, stream(dev))
    torch.cuda.synchronize()
    return pr.np()


def test_presence_empty_is_zeros(gpu_device):
    assert not run_presence(np.zeros(1, dtype=np.int64), 0, -5, 300, gpu_device).any()


def test_presence_ignores_tokens_outside_the_range(gpu_device):
    """Tokens below min_tok or from min_tok + n_cp on set nothing (the guards on either side of
    the n_cp bytes stay intact, checked by Guarded.np)."""
    mn, n_cp = -5, 300
    rng = np.random.default_rng(3)
    tok = np.concatenate([rng.integers(mn, mn + n_cp, 900)[rng.random(900) < 0.5],
                          [mn - 1, mn - 2, mn - GUARD, mn + n_cp, mn + n_cp + 1, mn + n_cp + GUARD - 1,
                           I64_MIN, 2 ** 62, mn + 2 ** 32, mn - 2 ** 32, mn + 2 ** 32 + 3]]).astype(np.int64)
    rng.shuffle(tok)
    want = np.zeros(n_cp, dtype=np.uint8)
    inside = tok[(tok >= mn) & (tok < mn + n_cp)]
    want[inside - mn] = 1
    assert 0 < want.sum() < n_cp
    assert np.array_equal(run_presence(tok, tok.size, mn, n_cp, gpu_device), want)


def test_presence_second_trip(gpu_device):
    """n = 2048 * 256 + 1: the grid is capped at 2,048 workgroups of 256, and one code point occurs
    only at the last index, which workgroup 0 reads on its second trip."""
    n, mn, n_cp = BO.N_MINMAX_BIG, 7, 41
    tok = np.random.default_rng(4).integers(mn, mn + n_cp - 1, size=n, dtype=np.int64)
    tok[n - 1] = mn + n_cp - 1
    got = run_presence(tok, n, mn, n_cp, gpu_device)
    grid_is(2048, "k_presence")
    assert got.all() and got.size == n_cp


# ---------------------------------------------------------------- beast_bpe_count_pairs --
# n_sym -> the form and the row groups the host formula of beast_bpe_count_pairs selects:
#   R = min(n_sym, 160 KiB / (4 n_sym)) rows of n_sym uint32 fit the LDS budget, groups = ceil(n_sym / R);
#   groups <= 16: k_count_pairs_lds on a (gx, groups) grid, else k_count_pairs (global atomics).
#   202: 202^2 * 4 = 163,216 bytes is the last square to fit 163,840; 203: R = 201, a last group of 2 rows;
#   800: R = 51, 16 groups; 810: R = 50, 17 groups.
COUNT_FORMS = {1: ("lds", 1), 2: ("lds", 1), 202: ("lds", 1), 203: ("lds", 2), 800: ("lds", 16), 810: ("global", 17)}


def count_pairs_launch(n_sym, n_words, cus):
    """(form, row groups, gridDim.x): beast_bpe_count_pairs' host formula restated."""
    budget = 160 * 1024
    R = min(n_sym, budget // (4 * n_sym))
    groups = cdiv(n_sym, R) if R else 0
    chunks = cdiv(n_words, 256)
    if R and groups <= 16:
        per_cu = max(1, budget // (R * n_sym * 4))
        return "lds", groups, max(1, min(cus * per_cu // groups, chunks))
    return "global", groups, max(1, min(chunks, 8192))


def check_count_pairs(n_sym, n_words, with_counts, dev):
    ins = Inputs(dev)
    Vt = n_sym + 37                       # the table's row stride is not n_sym
    tpl, idx = BO.count_words(n_sym, n_words)
    sym, ws, wl = BO.layout_np(tpl, idx)
    wc = np.random.default_rng(n_words).integers(1, 1000, n_words).astype(np.int32) if with_counts else None
    table = Guarded(Vt * Vt, torch.int32, dev, init=0)
    _lib.run("beast_bpe_count_pairs", ins(sym), ins(ws), ins(wl),
             ins(wc) if with_counts else None, n_words, table.ptr, Vt, n_sym, stream(dev))
    torch.cuda.synchronize()
    form, groups, gx = count_pairs_launch(n_sym, n_words, cu_count(dev))
    assert (form, groups) == COUNT_FORMS[n_sym]
    if n_words:
        grid_is(gx, f"count_pairs {form}")
    got = table.np().reshape(Vt, Vt)
    want = BO.count_pairs_layout(sym, ws, wl, wc, Vt)
    assert want.max() < 2 ** 31
    assert np.array_equal(got, want.astype(np.int32))
    assert not got[n_sym:].any() and not got[:, n_sym:].any()
    if n_words > 8:
        assert got[n_sym - 1, n_sym - 1] > 0
    return form, gx


@pytest.mark.parametrize("with_counts", [False, True], ids=["wcount_null", "wcount"])
@pytest.mark.parametrize("n_words", [0, 1, 255, 256, 257])
@pytest.mark.parametrize("n_sym", list(COUNT_FORMS))
def test_count_pairs_small(n_sym, n_words, with_counts, gpu_device):
    """The form COUNT_FORMS names for n_sym (the host formula above): at these word counts both
    forms launch ceil(n_words / 256) workgroups in x, so the form is the formula's, not a measured one;
    test_count_pairs_above_the_grid_cap tells them apart by gridDim.x."""
    check_count_pairs(n_sym, n_words, with_counts, gpu_device)


@pytest.mark.parametrize("n_sym", [202, 203, 800, 810])
def test_count_pairs_above_the_grid_cap(n_sym, gpu_device):
    """More 256-word chunks than the form that runs launches workgroups, so workgroups take a second
    chunk.  LDS form (202: 1 row group, 203: 2, 800: 16): one workgroup a CU fits the 160 KiB, so
    gridDim.x is capped at CUs / groups, and n_words = 256 * (2 * cap) + 1 makes 2 * cap + 1 chunks;
    the global form would launch one workgroup per chunk there.  Global form (810: 17 groups):
    capped at 8,192 workgroups, n_words = 8192 * 256 + 1; the LDS formula would give CUs / 17.
    (n_sym 1 and 2 keep tens of thousands of workgroups a CU resident: no input reaches that cap.)"""
    cus = cu_count(gpu_device)
    form, groups = COUNT_FORMS[n_sym]
    n_words = BO.N_SIG_BIG if form == "global" else 256 * 2 * (cus // groups) + 1
    got_form, gx = check_count_pairs(n_sym, n_words, True, gpu_device)
    chunks = cdiv(n_words, 256)
    assert got_form == form and gx < chunks
    other = min(chunks, 8192) if form == "lds" else max(1, cus // groups)
    assert gx != other                       # gridDim.x (asserted in check_count_pairs) names the form


# ------------------------------------------------------------ beast_bpe_word_signatures --
def run_signatures(tpl, idx, dev):
    ins = Inputs(dev)
    sym, ws, wl = BO.layout_np(tpl, idx)
    sig = Guarded(idx.size, torch.int64, dev)
    _lib.run("beast_bpe_word_signatures", ins(sym), ins(ws), ins(wl),
             idx.size, sig.ptr, stream(dev))
    torch.cuda.synchronize()
    return sig.np()


def test_word_signatures_match_sig_of(gpu_device):
    """Words of 0, 1, 2, 48, 49 and 300 symbols, ids up to 65,534."""
    tpl = BO.sig_templates()
    assert [len(w) for w in tpl[:6]] == [0, 1, 2, 48, 49, 300] and max(map(max, tpl[1:6])) == 65534
    got = run_signatures(tpl, np.arange(len(tpl)), gpu_device)
    grid_is(1, "k_word_sig")
    assert got.tolist() == BO.sigs_i64(tpl).tolist()
    assert got[0] == 0


def test_word_signatures_second_trip(gpu_device):
    """n_words = 8192 * 256 + 1 words drawn from 64 templates: the grid is capped at 8,192
    workgroups of 256, and the last word (49 symbols) is workgroup 0's second trip."""
    tpl = BO.sig_templates()
    idx = BO.big_sig_index(len(tpl))
    got = run_signatures(tpl, idx, gpu_device)
    grid_is(8192, "k_word_sig")
    assert np.array_equal(got, BO.sigs_i64(tpl)[idx])


# ------------------------------------------------------ dedup, repack, compact (setup) --
def word_pool():
    """The distinct words, written down: lengths 0 and 1 (dedup drops them), 2, 254, 255, 256, 300,
    words that differ in their last symbol only, a prefix of another word, repeated symbols."""
    def run(L, mul, add=0):
        return [(mul * j + add) % 500 for j in range(L)]
    pool = [[], [7], [8], [1, 2], [1, 3], [2, 1], [0, 0], [0, 0, 0], [1, 2, 3], [1, 2, 3, 4], [1, 2, 3, 4, 5],
            [499, 0, 499], [9] * 17, [9] * 18]
    pool += [run(L, 7) for L in (254, 255, 256, 300)] + [run(L, 11, 3) for L in (254, 255, 256, 300)]
    pool += [run(255, 7)[:-1] + [123], run(256, 7)[:-1] + [124], run(33, 13), run(64, 17), run(5, 3), run(6, 3)]
    assert len({tuple(w) for w in pool}) == len(pool)
    return pool


def pool_occurrences(n_words):
    """idx[w]: which pool word occurrence w is; multiplicities differ per word."""
    P = len(word_pool())
    return (np.arange(n_words) * 7 + (np.arange(n_words) // 11) % 5) % P


def packed_layout(words):
    """Words tiling the symbol array without padding, as the pre-tokeniser emits them."""
    lens = np.array([len(w) for w in words], dtype=np.int64)
    ws = np.concatenate([[0], np.cumsum(lens)])
    sym = np.array([s for w in words for s in w], dtype=np.uint16)
    return sym, ws[:-1].astype(np.int32), lens.astype(np.int32)


@pytest.mark.parametrize("n_words", [0, 1, 2047, 2048, 2049])
def test_dedup_words_match_counter(n_words, gpu_device):
    ins = Inputs(gpu_device)
    from collections import Counter
    dev, pool = gpu_device, word_pool()
    words = [pool[i] for i in pool_occurrences(n_words)]
    if n_words == 1:
        words = [pool[3]]
    sym, ws, wl = packed_layout(words)
    lib = _lib.load()
    wsp = Guarded(lib.beast_bpe_dedup_workspace_bytes(n_words), torch.uint8, dev)
    ow, ol, oc = (Guarded(n_words, torch.int32, dev) for _ in range(3))
    on = Guarded(1, torch.int64, dev)
    _lib.run("beast_bpe_dedup_words", ins(sym), ins(ws), ins(wl), n_words,
             wsp.ptr, wsp.n, ow.ptr, ol.ptr, oc.ptr, on.ptr, stream(dev))
    torch.cuda.synchronize()
    wsp.np()
    want = Counter(tuple(w) for w in words if len(w) >= 2)
    nu = int(on.np()[0])
    assert nu == len(want)
    s, l, c = ow.np()[:nu], ol.np()[:nu], oc.np()[:nu]
    got = [(tuple(sym[a:a + k].tolist()), int(m)) for a, k, m in zip(s, l, c)]
    assert len(dict(got)) == nu and dict(got) == dict(want)


@pytest.mark.parametrize("with_counts", [False, True], ids=["wcount_null", "wcount"])
@pytest.mark.parametrize("n_words", [0, 1, 2047, 2048, 2049])
def test_repack_words_layout(n_words, with_counts, gpu_device):
    """k_len_scatter takes 2,048 words a workgroup (RP_WPB).  The output is ordered by bucket
    min(L, 255) -- 255, 256 and 300 share the last one -- and unordered inside a bucket: the
    (word, count) multisets are compared per bucket.  Spans are 4-aligned, contiguous and
    zero-padded (out_sym starts as the sentinel), *out_nsym is the padded total."""
    ins = Inputs(gpu_device)
    dev, pool = gpu_device, word_pool()
    words = [pool[i] for i in pool_occurrences(n_words)]
    if n_words == 1:
        words = [pool[-1]]                                   # 6 symbols: two of padding
    sym, ws, wl = packed_layout(words)
    wc = (np.arange(n_words) % 1000 + 1).astype(np.int32) if with_counts else None
    total = int(((wl.astype(np.int64) + 3) // 4 * 4).sum())
    lib = _lib.load()
    wsp = Guarded(lib.beast_bpe_repack_workspace_bytes(n_words), torch.uint8, dev)
    osym = Guarded(total, torch.int16, dev)
    ow, ol, oc = (Guarded(n_words, torch.int32, dev) for _ in range(3))
    on = Guarded(1, torch.int64, dev)
    _lib.run("beast_bpe_repack_words", ins(sym), ins(ws), ins(wl),
             ins(wc) if with_counts else None, n_words, wsp.ptr, wsp.n, osym.ptr, ow.ptr, ol.ptr,
             oc.ptr, on.ptr, stream(dev))
    torch.cuda.synchronize()
    wsp.np()
    assert int(on.np()[0]) == total
    s2, st, ln, ct = osym.np().view(np.uint16), ow.np().astype(np.int64), ol.np().astype(np.int64), oc.np()
    span = (ln + 3) // 4 * 4
    assert np.array_equal(st, np.concatenate([[0], np.cumsum(span)])[:-1])            # 4-aligned, contiguous
    bucket = np.minimum(ln, 255)
    assert np.all(np.diff(bucket) >= 0)
    live = np.zeros(total, dtype=bool)
    for a, k in zip(st, ln):
        live[a:a + k] = True
    assert not s2[~live].any()                                                        # the padding is zero
    cnt = wc if with_counts else np.ones(n_words, dtype=np.int32)                     # wcount NULL means 1
    got = sorted((min(int(k), 255), tuple(s2[a:a + k].tolist()), int(m)) for a, k, m in zip(st, ln, ct))
    want = sorted((min(len(w), 255), tuple(w), int(m)) for w, m in zip(words, cnt))
    assert got == want
    if n_words >= 2047:
        assert {254, 255} <= set(bucket.tolist()) and {255, 256, 300} <= set(ln[bucket == 255].tolist())


@pytest.mark.parametrize("with_counts", [False, True], ids=["wcount_null", "wcount"])
@pytest.mark.parametrize("n_words", [0, 63, 64, 65, BO.N_COMPACT_BIG])
def test_compact_words_keeps_mergeable(n_words, with_counts, gpu_device):
    """Every third length is below 2 (0 and 1 in turn).  The order of the kept words is
    unspecified: sorted (start, length, count) triples are compared.  n = 16384 * 256 + 5 exceeds
    the cap of 16,384 workgroups of 256, so workgroups 0 .. 4 take a second trip."""
    ins = Inputs(gpu_device)
    dev = gpu_device
    ws, wl, wc = BO.compact_inputs(n_words)
    ow, ol, oc = (Guarded(n_words, torch.int32, dev) for _ in range(3))
    on = Guarded(1, torch.int64, dev)
    _lib.run("beast_bpe_compact_words", ins(ws), ins(wl),
             ins(wc) if with_counts else None, n_words, ow.ptr, ol.ptr, oc.ptr, on.ptr, stream(dev))
    torch.cuda.synchronize()
    if n_words:
        grid_is(min(cdiv(n_words, 256), 16384), "k_compact_words")
    keep = wl >= 2
    m = int(on.np()[0])
    assert m == int(keep.sum()) and (n_words < 3 or 0 < m < n_words)
    cnt = wc if with_counts else np.ones(n_words, dtype=np.int32)
    got = np.sort(BO.compact_key(ow.np()[:m], ol.np()[:m], oc.np()[:m]))
    assert np.array_equal(got, np.sort(BO.compact_key(ws[keep], wl[keep], cnt[keep])))


# --------------------------------------------------------------------- beast_bpe_argmax --
def argmax_ws(Vt, dev):
    return Guarded(_lib.load().beast_bpe_argmax_workspace_bytes(Vt), torch.uint8, dev, init=0)


def ws_slots(ws):
    return ws.np()[16:32].view(np.uint64).tolist()       # u64 words 2 and 3 (the bytes need not be a multiple of 8)


def key_of(count, x, y, Vt):
    return (count << 32) | (0xFFFFFFFF - (x * Vt + y))


def argmax_table(Vt, vcur, scenario):
    """(table uint32 [Vt, Vt], expected key).  Every table but the empty one also holds, where
    they fit: cells >= 2^31 (negative as int32: never candidates) inside the searched block, and
    counts above the maximum at x >= vcur and at y >= vcur (outside it)."""
    rng = np.random.default_rng([Vt, vcur])
    t = np.zeros((Vt, Vt), dtype=np.uint32)
    if scenario == "empty":
        return t, 0
    M = 1000
    if scenario != "single":
        bg = rng.integers(0, vcur, (min(4 * vcur, 4000), 2))
        t[bg[:, 0], bg[:, 1]] = rng.integers(1, M, bg.shape[0])
    hi = vcur - 1
    far = hi if hi < 2048 else 2048 + (hi - 2048) // 2 + 1      # a column of the second 2,048 stretch
    if scenario == "single":
        cells = [(hi, hi)]                                       # the last cell searched
    elif scenario == "tie_rows":                                 # rows of different 16-row workgroups
        cells = [(hi, 0), (hi // 2, hi), (min(17, hi), min(3, hi))]
    elif scenario == "tie_in_row":
        cells = [(hi, far), (hi, hi // 2), (hi, hi)]
    else:
        raise ValueError(scenario)
    for x, y in cells:
        t[x, y] = M
    neg = rng.integers(0, vcur, (min(vcur, 64), 2))
    keep = np.array([tuple(c) not in cells for c in neg.tolist()], dtype=bool)
    t[neg[keep, 0], neg[keep, 1]] = rng.choice(np.array([0x80000000, 0x80000001, 0xFFFFFFFF], dtype=np.uint32),
                                               int(np.sum(keep)))
    if vcur < Vt:
        t[vcur:, :] = M + 5
        t[:, vcur:] = M + 7
    x, y = min(cells)
    return t, key_of(M, x, y, Vt)


def argmax_vcurs(Vt):
    return [1, Vt] + ([Vt - 2] if Vt - 2 > 2048 else [])


@pytest.mark.parametrize("scenario", ["empty", "single", "tie_rows", "tie_in_row"])
@pytest.mark.parametrize("Vt,vcur", [(Vt, v) for Vt in (5, 64, 67, 2048, 2052, 4101) for v in argmax_vcurs(Vt)])
def test_argmax_matches_numpy(Vt, vcur, scenario, gpu_device):
    """rank_row reads 16 bytes a lane where Vt % 4 == 0 (64, 2048, 2052) and element by element
    otherwise (5, 67, 4101) and at a row's tail (vcur = Vt - 2); columns from 2,048 on are its
    second stretch (2052, 4101).  Ties go to the smallest (x, y).  Two calls on one fresh
    zero-filled workspace: results alternate between ws[2] and ws[3], and each call zeroes the
    other slot; the second call answers from the per-row cache."""
    dev = gpu_device
    t, want = argmax_table(Vt, vcur, scenario)
    assert want == NumpyBpeOps().argmax(torch.from_numpy(t.view(np.int32).reshape(-1)), Vt, vcur)
    td = dv(t.reshape(-1).view(np.int32), dev)
    ws = argmax_ws(Vt, dev)
    for call in range(3):
        _lib.run("beast_bpe_argmax", td.data_ptr(), Vt, vcur, ws.ptr, call, stream(dev))
        torch.cuda.synchronize()
        grid_is(cdiv(vcur, 16), "k_apply_argmax")
        slots = ws_slots(ws)
        assert slots[call & 1] == want, (call, slots, want)
        assert slots[1 - (call & 1)] == 0, (call, slots)


# ---------------------------------------------------------------------- beast_bpe_merge --
MERGE_VT = 600
FILL = BO.FILL                               # symbols that are neither a, b nor nid


def find_sig_only_word(a, b, rng):
    """A word whose signature has every bit of sig_need(a, b) but that holds no adjacent (a, b):
    both symbols apart, and other pairs that happen to set the pair's two bits."""
    need = BO.sig_need(a, b)
    for _ in range(20000):
        w = rng.integers(20, 400, 30).tolist()
        w[3], w[17] = a, b
        if a == b:
            w[18] = 19
        if BO.sig_of(w) & need == need and (a, b) not in zip(w, w[1:]):
            return w
    raise AssertionError("no word with the signature of (a, b) and without the pair")


def merge_words(a, b, nid, rng):
    """The word list of the merge tests, written down around the pair (a, b)."""
    def filler(L):
        return [FILL[(3 * j + L) % len(FILL)] for j in range(L)]

    def with_pair(L, at):
        w = filler(L)
        w[at], w[at + 1] = a, b
        return w
    words = [[], [a], [a, b], [b, a], [a, 11, b], [b, 11, a, 12]]                    # absent, both symbols present
    for L in (2, 3, 4, 5, 47, 48, 49, 50, 300):                                      # 48: the last register word
        words += [with_pair(L, 0), with_pair(L, L - 2)]
        if L >= 5:
            words.append(with_pair(L, 3))                                            # straddles an 8-byte unit
            words.append(filler(L))                                                  # no pair at all
        if L >= 47:                                                                  # several, and at both ends
            w = with_pair(L, 0)
            w[L - 2], w[L - 1] = a, b
            w[7], w[8] = a, b
            w[20], w[21], w[22], w[23] = a, b, a, b
            words.append(w)
    words += [[a, b, a, b, a, b], [11, a, b, a, b, a, b, 12], [a, b, nid], [nid, a, b], [nid, a, b, nid, a, b, a]]
    if a == b:
        words += [[a] * 3, [a] * 4, [a] * 5, [12] + [a] * 7 + [13], [a] * 48, [a] * 49, [a] * 300, [11, a, 12, a]]
    else:
        words += [[a, a, b, b], [b, a, b, a], [a, a, a, b], [a, b, b, b], [a, 13, b] * 16]
    # neighbours of every token length (tlen below: FILL[k] has length 1 + k % 3)
    for s in FILL:
        words += [[s, a, b, s], [s, a, b], [a, b, s], [s, s, a, b, a, b, s]]
    words.append(find_sig_only_word(a, b, rng))
    return words


def merge_tlen(a, b):
    tlen = np.ones(MERGE_VT, dtype=np.int32)
    for k, s in enumerate(FILL):
        tlen[s] = 1 + k % 3
    return tlen


def run_merge(d, wc, a, b, nid, tlen, max_len, Vt, lds_min, dev):
    """One beast_bpe_merge on guarded copies of the words dict d: (deltas [4, Vt], sym, wlen, sig)."""
    ins = Inputs(dev)
    n = d["n_words"]
    sym = Guarded(d["n_syms_padded"], torch.int16, dev, init=d["sym"][:d["n_syms_padded"]].numpy())
    wl = Guarded(n, torch.int32, dev, init=d["wlen"][:n].numpy())
    sig = Guarded(n, torch.int64, dev, init=d["sig"][:n].numpy())
    deltas = Guarded(4 * Vt, torch.int32, dev, init=0)
    td = Guarded(Vt, torch.int32, dev, init=tlen)
    lib = _lib.load()
    assert lib.beast_set_option(_lib.OPT_MERGE_LDS_MIN, lds_min) == 0
    try:
        _lib.run("beast_bpe_merge", sym.ptr, ins(d["wstart"][:n].numpy()), wl.ptr,
                 None if wc is None else ins(wc), n, a, b, nid, td.ptr, max_len, deltas.ptr, Vt, sig.ptr,
                 1, stream(dev))
        torch.cuda.synchronize()
        grid = _lib.last_launch_grid()
    finally:
        lib.beast_set_option(_lib.OPT_MERGE_LDS_MIN, 4096)
    assert np.array_equal(td.np(), tlen)
    return deltas.np().reshape(4, Vt), sym.np().view(np.uint16), wl.np(), sig.np(), grid


@pytest.mark.parametrize("counts", ["wcount", "wcount_null"])
@pytest.mark.parametrize("max_len", [3, 4, 2 ** 31 - 1])
@pytest.mark.parametrize("lds_min", [0, 1 << 30], ids=["lds_deltas", "global_deltas"])
@pytest.mark.parametrize("pair", ["a_b", "a_a"])
def test_merge_matches_numpy(pair, lds_min, max_len, counts, gpu_device):
    """k_merge<true> (pair_count 1 >= threshold 0: deltas summed in LDS, 4 * Vt * 4 <= 64 KiB) and
    k_merge<false> (threshold 2^30: global atomics); which one runs is the host's choice from
    OPT_MERGE_LDS_MIN alone (both launch one workgroup here).  Words of up to 48 symbols merge in
    registers, longer ones in global memory.  Token lengths: a, b 1 (the new token 2), neighbours
    1, 2 or 3, so at max_token_length 3 every '+' is blocked, at 4 those next to a neighbour of
    length 1 pass and those next to the merge's own new token (2 + 2) do not, at 2^31 - 1 all pass."""
    dev = gpu_device
    a, b, nid = (5, 9, 77) if pair == "a_b" else (5, 5, 77)
    rng = np.random.default_rng(8)
    words = merge_words(a, b, nid, rng)
    n = len(words)
    wc = rng.integers(1, 50, n)
    wc[::9] = 2 ** 20
    wc[1::9] = 2 ** 20 - 1
    cnt = wc.tolist() if counts == "wcount" else [1] * n
    tlen = merge_tlen(a, b)
    d = BO.lists_to_words(words, cnt, "cpu")
    ref = NumpyBpeOps()
    ref.new_state(MERGE_VT, tlen)
    merged = [list(w) for w in words]
    want = ref.merge({"words": merged, "counts": cnt}, a, b, nid, max_len, MERGE_VT).numpy().reshape(4, MERGE_VT)
    got, sym, wl, sig, grid = run_merge(d, wc.astype(np.int32) if counts == "wcount" else None, a, b, nid, tlen,
                                        max_len, MERGE_VT, lds_min, dev)
    assert grid == 1
    assert np.array_equal(got, want)
    # the '+' rows: blocked and allowed as the docstring says
    plus = int(want[1].sum()) + int(want[3].sum())
    assert (plus == 0) == (max_len == 3) and want[0].sum() < 0 and want[2].sum() < 0
    if max_len == 4:
        assert want[1, FILL[0]] > 0 and want[3, FILL[0]] > 0 and want[1, FILL[1]] == 0 and want[3, FILL[1]] == 0
        assert want[1, nid] == 0 and want[0, nid] < 0
    if max_len == 2 ** 31 - 1:
        assert want[1, nid] > 0 and want[1, FILL[2]] > 0 and want[3, FILL[2]] > 0
    ws = d["wstart"].numpy()
    assert wl.tolist() == [len(w) for w in merged]
    assert [sym[s:s + k].tolist() for s, k in zip(ws, wl)] == merged
    assert sig.tolist() == BO.sigs_i64(merged).tolist()              # rewritten or untouched
    assert merged[-1] == words[-1] and sum(len(w) for w in merged) < sum(len(w) for w in words)


@pytest.mark.parametrize("lds_min", [0, 1 << 30], ids=["lds_deltas", "global_deltas"])
def test_merge_beyond_the_resident_grid(lds_min, gpu_device):
    """n_words = 2048 * 1100 + 300 words, each holding the pair, drawn from 64 templates: a
    workgroup scans 2,048 words a round (8 chunks of 256) and the grid is the resident one, so
    2048 * gridDim.x < n_words proves a second round -- and with every word a candidate, more
    than the 2,048 entries of the LDS candidate list per workgroup (the threads merge the overflow
    themselves).  The expected changes are merge_templates' (linear in the counts)."""
    dev = gpu_device
    a, b, nid, Vt, max_len = 5, 9, 77, MERGE_VT, 4
    tpl = BO.big_merge_templates(a, b)
    n = BO.N_MERGE_BIG
    idx, wc = BO.big_merge_index()
    sym0, ws, wl0 = BO.layout_np(tpl, idx)
    tlen = merge_tlen(a, b)
    tsig = BO.sigs_i64(tpl)
    d = {"sym": torch.from_numpy(sym0.view(np.int16)), "wstart": torch.from_numpy(ws), "wlen": torch.from_numpy(wl0),
         "sig": torch.from_numpy(tsig[idx]), "n_words": n, "n_syms_padded": sym0.size}
    mult = np.bincount(idx, weights=wc, minlength=len(tpl)).astype(np.int64)
    want, merged = BO.merge_templates(tpl, mult, a, b, nid, max_len, Vt, tlen)
    got, sym, wl, sig, grid = run_merge(d, wc, a, b, nid, tlen, max_len, Vt, lds_min, dev)
    assert 0 < grid and 2048 * grid < n, f"grid {grid}: no workgroup scans a second round of {n} words"
    assert np.array_equal(got, want.astype(np.int32))
    mlen = np.array([len(w) for w in merged], dtype=np.int32)
    assert np.array_equal(wl, mlen[idx])
    msym, mws, mwl = BO.layout_np(merged, idx)
    assert np.array_equal(BO.live_symbols(sym, ws, wl), BO.live_symbols(msym, mws, mwl))
    assert np.array_equal(sig, BO.sigs_i64(merged)[idx])


# --------------------------------------------------------------- beast_bpe_apply_argmax --
APPLY_CASES = {
    # name: (a, b, nid, vcur) as offsets into Vt where negative
    "one_workgroup": (16, 18, 21, 0),            # rows 16 .. 31
    "three_workgroups": (3, 40, -1, 0),
    "a_equals_b": (35, 35, -1, 0),
    "nid_equals_b": (3, 40, 40, 0),
    "reused_id": (50, 3, 20, 0),                 # nid < vcur and in another workgroup than a, b
    "nid_is_the_new_row": (3, 40, -5, -4),       # vcur < Vt: nid = vcur - 1, rows beyond not searched
}


@pytest.mark.parametrize("case", list(APPLY_CASES))
@pytest.mark.parametrize("Vt", [67, 2052])
def test_apply_argmax_matches_numpy(Vt, case, gpu_device):
    """beast_bpe_argmax fills the per-row cache (call 0), then beast_bpe_apply_argmax (call 1) adds
    sparse random deltas: rows whose cells did not change answer from the cache, the others are
    ranked again.  Table exact, the deltas consumed all zero, table[a][b] == 0, tlen[nid], the key."""
    dev = gpu_device
    a, b, nid, vcur = (v + Vt if v < 0 else v for v in APPLY_CASES[case])
    vcur = vcur or Vt
    rng = np.random.default_rng([Vt, a, b, nid])
    t = rng.integers(0, 1000, (Vt, Vt)).astype(np.uint32)
    t[rng.random((Vt, Vt)) < 0.5] = 0
    t[a, b] = 5000                                                   # the pair being merged: the maximum
    dl = rng.integers(-1200, 1200, (4, Vt)).astype(np.int32)
    dl[rng.random((4, Vt)) < 0.7] = 0
    rows = max(vcur, a + 1, b + 1, nid + 1)
    dl[:2, rows:] = 0                                                # symbols that do not exist yet
    tlen = rng.integers(1, 9, Vt).astype(np.int32)
    ref = NumpyBpeOps()
    ref.new_state(Vt, tlen)
    rt = torch.from_numpy(t.view(np.int32).reshape(-1).copy())
    key0 = ref.argmax(rt, Vt, vcur)
    key1 = ref.apply_argmax(rt, torch.from_numpy(dl.reshape(-1).copy()), Vt, vcur, a, b, nid)
    assert key0 == key_of(5000, a, b, Vt) and key1 != key0
    table = Guarded(Vt * Vt, torch.int32, dev, init=t.reshape(-1).view(np.int32))
    deltas = Guarded(4 * Vt, torch.int32, dev, init=dl.reshape(-1))
    td = Guarded(Vt, torch.int32, dev, init=tlen)
    ws = argmax_ws(Vt, dev)
    _lib.run("beast_bpe_argmax", table.ptr, Vt, vcur, ws.ptr, 0, stream(dev))
    _lib.run("beast_bpe_apply_argmax", table.ptr, deltas.ptr, Vt, vcur, a, b, nid, td.ptr, ws.ptr, 1, stream(dev))
    torch.cuda.synchronize()
    grid_is(cdiv(rows, 16), "k_apply_argmax")
    assert ws_slots(ws) == [0, key1]
    got = table.np().reshape(Vt, Vt)
    assert np.array_equal(got, rt.numpy().reshape(Vt, Vt))
    assert got[a, b] == 0
    assert not deltas.np().any()
    want_tlen = tlen.copy()
    want_tlen[nid] = tlen[a] + tlen[b]
    assert np.array_equal(td.np(), want_tlen) and np.array_equal(ref.tlen, want_tlen)
    # the cache was used: some row < vcur had no change at all, some did
    changed = (dl[0, :vcur] != 0) | (dl[1, :vcur] != 0)
    changed[[x for x in (a, b, nid) if x < vcur]] = True
    assert changed.any() and not changed.all()


# ------------------------------------------------------------ the host-driven loop in lockstep --
class CheckedOps(GpuBpeOps):
    """GpuBpeOps with a NumpyBpeOps beside it: count_pairs, argmax, merge, apply_argmax and compact
    run both and compare after every call -- the key, the deltas, every word with its length,
    signature and count, the table, tlen -- so a mismatch names the merge and the first kernel
    that went wrong.  Above Vt 2,048 the table is compared in full every 25th merge and in rows
    a, b, nid and columns a, nid at every merge."""

    def __init__(self, device):
        super().__init__(device)
        self.ref = NumpyBpeOps()
        self.n_merges = 0
        self.reused = []
        self.compactions = 0

    def _fail(self, op, what):
        raise AssertionError(f"merge {self.n_merges}: {op}: {what} differs from NumpyBpeOps")

    def _adopt_words(self, words):
        """The device words become the reference's lists (after count_pairs' input and after a
        compaction, whose order is unspecified)."""
        self.rwords = BO.words_to_lists(words)
        self.rsig = BO.sigs_i64(self.rwords["words"])

    def _check_words(self, op, words):
        n = words["n_words"]
        ref = self.rwords
        if n != len(ref["words"]):
            self._fail(op, "n_words")
        wl = words["wlen"].cpu().numpy()[:n]
        if wl.tolist() != [len(w) for w in ref["words"]]:
            self._fail(op, "wlen")
        sym = words["sym"].cpu().numpy().view(np.uint16)
        flat = np.fromiter((s for w in ref["words"] for s in w), dtype=np.uint16)
        if not np.array_equal(BO.live_symbols(sym, words["wstart"].cpu().numpy()[:n], wl), flat):
            self._fail(op, "symbols")
        if words["wcount"].cpu().numpy()[:n].tolist() != ref["counts"]:
            self._fail(op, "wcount")
        if not np.array_equal(words["sig"].cpu().numpy()[:n], self.rsig):
            self._fail(op, "sig")

    def _check_table(self, op, table, cells=None):
        Vt = self.Vt
        rt = self.rtable.numpy().reshape(Vt, Vt)
        if cells is None or Vt <= 2048 or self.n_merges % 25 == 0:
            if not np.array_equal(table.cpu().numpy().reshape(Vt, Vt), rt):
                self._fail(op, "the table")
            return
        a, b, nid = cells
        tv = table.view(Vt, Vt)
        for r in (a, b, nid):
            if not np.array_equal(tv[r].cpu().numpy(), rt[r]):
                self._fail(op, f"table row {r}")
        for c in (a, nid):
            if not np.array_equal(tv[:, c].cpu().numpy(), rt[:, c]):
                self._fail(op, f"table column {c}")

    def count_pairs(self, words, Vt, n_sym=0):
        table = super().count_pairs(words, Vt, n_sym)
        self.Vt = Vt
        self._adopt_words(words)
        self._check_words("pretok_dedup", words)          # the signatures the setup made
        self.rtable = self.ref.count_pairs(self.rwords, Vt, n_sym)
        self._check_table("count_pairs", table)
        return table

    def new_state(self, Vt, tlen):
        super().new_state(Vt, tlen)
        self.ref.new_state(Vt, tlen)

    def argmax(self, table, Vt, vcur):
        key = super().argmax(table, Vt, vcur)
        if key != self.ref.argmax(self.rtable, Vt, vcur):
            self._fail("argmax", "the key")
        return key

    def merge(self, words, a, b, nid, max_len, Vt, count=1 << 62):
        deltas = super().merge(words, a, b, nid, max_len, Vt, count)
        ref = self.rwords
        has_a = [i for i, w in enumerate(ref["words"]) if a in w]     # the others cannot change
        sub = {"words": [ref["words"][i] for i in has_a], "counts": [ref["counts"][i] for i in has_a]}
        before = [len(w) for w in sub["words"]]
        rd = self.ref.merge(sub, a, b, nid, max_len, Vt)
        for i, w, k in zip(has_a, sub["words"], before):
            if len(w) != k:
                self.rsig[i] = BO.sigs_i64([w])[0]
        if not np.array_equal(deltas.cpu().numpy(), rd.numpy()):
            self._fail("merge", "the deltas")
        self._check_words("merge", words)
        self.rdeltas = rd
        return deltas

    def apply_argmax(self, table, deltas, Vt, vcur, a, b, nid, reused):
        key = super().apply_argmax(table, deltas, Vt, vcur, a, b, nid, reused)
        rkey = self.ref.apply_argmax(self.rtable, self.rdeltas, Vt, vcur, a, b, nid)
        self.n_merges += 1
        self.reused.append(bool(reused))
        self._check_table("apply_argmax", table, (a, b, nid))
        if deltas.any().item():
            self._fail("apply_argmax", "the consumed deltas (not zero)")
        if not np.array_equal(self._tlen.cpu().numpy(), self.ref.tlen.astype(np.int32)):
            self._fail("apply_argmax", "tlen")
        if key != rkey:
            self._fail("apply_argmax", "the key")
        return key

    def compact(self, words):
        out = super().compact(words)
        want = self.ref.compact(self.rwords)
        self.compactions += 1
        got = BO.words_to_lists(out)
        if sorted(zip(map(tuple, got["words"]), got["counts"])) != \
                sorted(zip(map(tuple, want["words"]), want["counts"])):
            self._fail("compact", "the kept words")
        self._adopt_words(out)
        self._check_words("compact", out)                 # the signatures compact made afresh
        return out


LOCKSTEP_MERGES = 150


def lockstep_corpus(span):
    """300 rows x 60 tokens: 12 common symbols spread over ``span`` token values, and a few others."""
    rng = np.random.default_rng(span)
    common = np.sort(rng.choice(span, 12, replace=False))
    common[0], common[-1] = 0, span - 1
    arr = common[rng.integers(0, 12, size=(300, 60))]
    rare = rng.random((300, 60)) < 0.03
    arr[rare] = rng.integers(0, span, int(rare.sum()))
    return arr.astype(np.int64) + 5


def lockstep_special(arr, span):
    """span 40: a special token spelled like the corpus' first merge (found by a one-merge
    training on the numpy ops), so that merge finds its string in the vocabulary and re-uses the
    special token's id (HF looks the new string up before it appends one)."""
    if span != 40:
        return []
    flat, off = torch.from_numpy(arr.reshape(-1)), torch.arange(0, arr.size + 1, arr.shape[1])
    n_base = lockstep_vocab(arr, 0, [])[1]
    first = train_bpe(flat, off, n_base + 1, ops=NumpyBpeOps(), device_loop=False, min_frequency=1).merges[0]
    return [first[0] + first[1]]


def lockstep_vocab(arr, rem, special):
    """A vocab_size 150 merges above the corpus' alphabet, rounded up so that Vt % 4 == rem."""
    n_cp = int(arr.max() - arr.min()) + 1
    present = np.zeros(n_cp, dtype=bool)
    present[np.unique(arr) - arr.min()] = True
    n_base = len(build_alphabet(present, [chr(i) for i in range(n_cp)], special)[0])
    v = n_base + LOCKSTEP_MERGES
    return v + (rem - v) % 4, n_base


LOCKSTEP = [(span, mtl, mf, lds, ce, 0) for span in (40, 2100) for mtl in (4, 10000) for mf in (1, 3)
            for lds in (0, 1 << 30) for ce in (0, 7)] + [(40, 10000, 1, 0, 0, 3), (2100, 10000, 1, 1 << 30, 7, 1)]


@pytest.mark.parametrize("span,max_token_length,min_frequency,lds_min,compact_every,rem", LOCKSTEP)
def test_host_loop_in_lockstep(span, max_token_length, min_frequency, lds_min, compact_every, rem, gpu_device):
    """train_bpe's host-driven loop on CheckedOps: up to 150 merges (the vocabulary room), or
    until the stop rule (min_frequency 3, or no pair left under max_token_length 4).  span 2100
    makes Vt > 2,048 (rank_row's second stretch); rem is Vt % 4 (0: its 16-byte loads).  Every
    span-40 case re-uses an id (lockstep_special), asserted at the end."""
    dev = gpu_device
    arr = lockstep_corpus(span)
    special = lockstep_special(arr, span)
    vocab, n_base = lockstep_vocab(arr, rem, special)
    flat, off = fixed_rows_to_device(torch.from_numpy(arr).to(dev))
    ops = CheckedOps(dev)
    lib = _lib.load()
    assert lib.beast_set_option(_lib.OPT_MERGE_LDS_MIN, lds_min) == 0
    try:
        res = train_bpe(flat, off, vocab, ops=ops, device_loop=False, max_token_length=max_token_length,
                        min_frequency=min_frequency, compact_every=compact_every, special_tokens=special)
    finally:
        lib.beast_set_option(_lib.OPT_MERGE_LDS_MIN, 4096)
    assert res.stats["loop"] == "host" and res.stats["Vt"] == vocab and vocab % 4 == rem
    assert (vocab > 2048) == (span == 2100)
    assert ops.n_merges == len(res.merges) > 20
    full = len(res.vocab) == vocab
    assert full or min_frequency == 3 or max_token_length == 4            # else the stop rule ended it
    assert ops.n_merges >= LOCKSTEP_MERGES or not full
    if compact_every:
        assert ops.compactions >= ops.n_merges // compact_every - 1 > 0
    if special:
        assert any(ops.reused), "no merge of this case re-used an id"
