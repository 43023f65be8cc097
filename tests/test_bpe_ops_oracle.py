"""CPU tests of tests/bpe_ops_oracle.py: the references the GPU tests of the BPE training kernels
(tests/test_gpu_bpe_ops.py) compare with are themselves compared with NumpyBpeOps' plain loops,
and timed at the sizes those tests use above the kernels' grid caps."""
import time

import numpy as np

import bpe_ops_oracle as BO
from cpu_ops import NumpyBpeOps

# A reference takes about a second on the machine this was written on; the bound leaves room for
# a slower or busier host without letting a reference grow to where a GPU test would crawl.
REFERENCE_SECONDS = 5.0


def random_words(rng, n, n_sym, max_len=12):
    return [rng.integers(0, n_sym, int(L)).tolist() for L in rng.integers(0, max_len + 1, n)]


def test_signature_has_no_false_negatives():
    """sig_of(word) holds every bit of sig_need(a, b) for every adjacent pair of the word: a
    filter on it never drops a word that holds the pair."""
    rng = np.random.default_rng(0)
    for n_sym in (3, 300, 65535):
        for w in random_words(rng, 300, n_sym, 40):
            g = BO.sig_of(w)
            assert 0 <= g < 2 ** 64
            for a, b in zip(w, w[1:]):
                need = BO.sig_need(a, b)
                assert g & need == need, (w, a, b)


def test_signature_bits():
    """csrc/bpe_common.h with BPE_SIG_PAIRS = 1: two symbol bits in the low 32, two pair bits in
    the high 32 (fewer where they coincide), products wrapping at 2^32."""
    assert BO.sig_of([]) == 0
    assert BO.sig_sym(0) == 1 and BO.sig_pair(0, 0) == 1 << 32
    for x in (1, 31, 32, 255, 65534):
        s = BO.sig_sym(x)
        assert s < 2 ** 32 and s & (1 << (x & 31)) and s & (1 << (((x * 0x9E3779B1) % 2 ** 32) >> 27))
        assert 1 <= bin(s).count("1") <= 2
        p = BO.sig_pair(x, 65534 - x)
        assert p >= 2 ** 32 and 1 <= bin(p).count("1") <= 2
    assert BO.sig_pair(65534, 3) != BO.sig_pair(3, 65534)
    assert BO.sig_of([7]) == BO.sig_sym(7)
    assert BO.sig_of([7, 9, 7]) == BO.sig_sym(7) | BO.sig_sym(9) | BO.sig_pair(7, 9) | BO.sig_pair(9, 7)
    assert BO.sigs_i64([[7, 9], []]).view(np.uint64).tolist() == [BO.sig_of([7, 9]), 0]


def test_count_pairs_np_equals_numpy_ops():
    rng = np.random.default_rng(1)
    for n_sym, n in ((1, 9), (2, 40), (50, 700)):
        words = random_words(rng, n, n_sym) + [[], [n_sym - 1], [n_sym - 1] * 3]
        counts = rng.integers(1, 1000, len(words)).tolist()
        Vt = n_sym + 37
        want = NumpyBpeOps().count_pairs({"words": words, "counts": counts}, Vt).numpy().reshape(Vt, Vt)
        assert np.array_equal(BO.count_pairs_np(words, counts, Vt), want)
        ones = NumpyBpeOps().count_pairs({"words": words, "counts": [1] * len(words)}, Vt).numpy().reshape(Vt, Vt)
        assert np.array_equal(BO.count_pairs_np(words, None, Vt), ones)
    assert not BO.count_pairs_np([], [], 5).any()


def test_merge_templates_equals_merge_of_the_expanded_list():
    rng = np.random.default_rng(2)
    Vt, a, nid = 40, 3, 30
    tlen = rng.integers(1, 4, Vt)
    for b in (5, 3):
        templates = random_words(rng, 20, 8, 14) + [[a, b], [a, b, a, b, a], [6, a, b, 7], [a] * 5, [nid, a, b]]
        idx = rng.integers(0, len(templates), 3000)
        counts = rng.integers(1, 9, idx.size)
        mult = np.bincount(idx, weights=counts, minlength=len(templates)).astype(np.int64)
        for max_len in (3, 4, 2 ** 31 - 1):
            got, merged = BO.merge_templates(templates, mult, a, b, nid, max_len, Vt, tlen)
            ops = NumpyBpeOps()
            ops.new_state(Vt, tlen)
            expanded = [list(templates[i]) for i in idx]
            want = ops.merge({"words": expanded, "counts": counts.tolist()}, a, b, nid, max_len, Vt)
            assert np.array_equal(got, want.numpy().reshape(4, Vt))
            assert expanded == [merged[i] for i in idx]
            assert any(m != t for m, t in zip(merged, templates)) and got.any()


def test_layout_round_trip():
    """lists -> device layout -> lists is the identity; spans start at multiples of 4 symbols, are
    contiguous and zero-padded; the signatures are sig_of's."""
    rng = np.random.default_rng(3)
    words = random_words(rng, 200, 65535, 9) + [[], [1], [65534] * 4, list(range(300))]
    counts = rng.integers(1, 2 ** 20, len(words)).tolist()
    d = BO.lists_to_words(words, counts, "cpu")
    back = BO.words_to_lists(d)
    assert back["words"] == words and back["counts"] == counts and back["n_words"] == len(words)
    ws, wl = d["wstart"].numpy().astype(np.int64), d["wlen"].numpy().astype(np.int64)
    sym = d["sym"].numpy().view(np.uint16)
    assert not (ws % 4).any() and ws[0] == 0
    span = (wl + 3) // 4 * 4
    assert np.array_equal(ws[1:], (ws + span)[:-1]) and d["n_syms_padded"] == ws[-1] + span[-1]
    live = np.zeros(sym.size, dtype=bool)
    for a, k in zip(ws, wl):
        live[a:a + k] = True
    assert not sym[~live].any()
    assert d["sig"].numpy().view(np.uint64).tolist() == [BO.sig_of(w) for w in words]
    assert np.array_equal(BO.live_symbols(sym, ws, wl), np.array([s for w in words for s in w], dtype=np.uint16))
    none = BO.lists_to_words(words, None, "cpu")
    assert none["wcount"] is None and BO.words_to_lists(none)["counts"] == [1] * len(words)
    empty = BO.lists_to_words([], [], "cpu")
    assert empty["n_words"] == 0 and BO.words_to_lists(empty)["words"] == []
    # the same layout from templates and an index
    idx = rng.integers(0, len(words), 500)
    s2, w2, l2 = BO.layout_np(words, idx)
    d2 = BO.lists_to_words([words[i] for i in idx], None, "cpu")
    assert np.array_equal(s2, d2["sym"].numpy().view(np.uint16)) and np.array_equal(w2, d2["wstart"].numpy())
    assert np.array_equal(l2, d2["wlen"].numpy())


def timed(what, fn):
    t0 = time.perf_counter()
    out = fn()
    dt = time.perf_counter() - t0
    print(f"[reference] {what}: {dt:.2f} s")
    assert dt < REFERENCE_SECONDS, f"{what}: the reference took {dt:.1f} s"
    return out


def test_references_are_quick_at_the_sizes_above_the_grid_caps():
    """Every size the GPU tests run above a grid cap (named in bpe_ops_oracle) with the reference
    of that test, timed one by one."""
    rng = np.random.default_rng(4)
    x = rng.integers(0, 2 ** 40, BO.SCAN_TILE ** 2 + 1, dtype=np.int64)
    timed("scan, 1024^2 + 1", lambda: np.concatenate([[0], np.cumsum(x)]))
    y = rng.integers(-2 ** 62, 2 ** 62, BO.N_MINMAX_BIG, dtype=np.int64)
    timed("minmax, 2048 * 256 + 1", lambda: (y.min(), y.max()))
    timed("presence, 2048 * 256 + 1", lambda: np.bincount((y & 63), minlength=64) > 0)
    # the argmax at the largest table of the GPU tests
    import torch
    big = rng.integers(0, 1000, 4101 * 4101).astype(np.int32)
    timed("argmax, Vt 4101", lambda: NumpyBpeOps().argmax(torch.from_numpy(big), 4101, 4101))
    # signatures at 8192 * 256 + 1 words of 64 templates
    tpl = BO.sig_templates()
    idx = BO.big_sig_index(len(tpl))
    assert len(tpl) == 64 and idx.size == BO.N_SIG_BIG
    timed("layout, 8192 * 256 + 1 words", lambda: BO.layout_np(tpl, idx))
    timed("signatures, 8192 * 256 + 1 words", lambda: BO.sigs_i64(tpl)[idx])
    # pair counts at 8192 * 256 + 1 words over 810 symbols (the global-atomics form's cap)
    ctpl, cidx = BO.count_words(810, BO.N_SIG_BIG)
    sym, ws, wl = timed("layout, count_pairs words", lambda: BO.layout_np(ctpl, cidx))
    wc = rng.integers(1, 1000, cidx.size)
    table = timed("count_pairs, 8192 * 256 + 1 words", lambda: BO.count_pairs_layout(sym, ws, wl, wc, 847))
    assert table.sum() == int((np.maximum(wl.astype(np.int64) - 1, 0) * wc).sum())
    # compaction at 16384 * 256 + 5 words
    cs, cl, cc = BO.compact_inputs(BO.N_COMPACT_BIG)
    timed("compact, 16384 * 256 + 5 words", lambda: np.sort(BO.compact_key(cs[cl >= 2], cl[cl >= 2], cc[cl >= 2])))
    # the merge at 2048 * 1100 + 300 words of 64 templates that all hold the pair
    a, b, nid, Vt = 5, 9, 77, 600
    mt = BO.big_merge_templates(a, b)
    assert len(mt) == 64 and all((a, b) in zip(w, w[1:]) for w in mt)
    midx, mwc = BO.big_merge_index()
    timed("layout, 2048 * 1100 + 300 words", lambda: BO.layout_np(mt, midx))
    mult = np.bincount(midx, weights=mwc, minlength=len(mt)).astype(np.int64)
    ones = np.ones(Vt, dtype=np.int64)
    d, merged = timed("merge_templates", lambda: BO.merge_templates(mt, mult, a, b, nid, 4, Vt, ones))
    assert d[0].sum() < 0 or d[2].sum() < 0
    m2, w2, l2 = BO.layout_np(merged, midx)
    timed("live symbols, 2048 * 1100 + 300 words", lambda: BO.live_symbols(m2, w2, l2))
