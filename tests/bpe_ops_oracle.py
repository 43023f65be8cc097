"""Plain references for the BPE training kernels taken one operation at a time (no GPU).

``tests/cpu_ops.py:NumpyBpeOps`` is the reference of the driver's ops; what is here is what it
lacks for a comparison with single launches of csrc/bpe_setup.hip and csrc/bpe_loop.hip:

* the words' 64-bit Bloom signature, restated from csrc/bpe_common.h (``BPE_SIG_PAIRS = 1``);
* the device word layout (``sym`` uint16 kept in int16 tensors, ``wstart`` / ``wlen`` / ``wcount``
  int32, every span starting at a multiple of 4 symbols and zero-padded to 4) to and from
  ``NumpyBpeOps``' lists;
* references for inputs of millions of words: a vectorised pair count, and a merge of a few
  template words weighted by how often each occurs.

The sizes the GPU tests use that exceed a grid cap are named here, so the CPU tests can time the
references at exactly those sizes.
"""
import numpy as np
import torch

from cpu_ops import NumpyBpeOps

M32 = 0xFFFFFFFF

# ---- sizes above the grid caps (blocks_for(n, per_block, cap) in the C-ABI entry points)
SCAN_TILE = 1024                        # k_scan_tiles; a recursion level more above 1024 and 1024^2
N_MINMAX_BIG = 2048 * 256 + 1           # k_minmax, k_presence: 2,048 workgroups of 256
N_SIG_BIG = 8192 * 256 + 1              # k_word_sig, k_count_pairs: 8,192 workgroups of 256
N_COMPACT_BIG = 16384 * 256 + 5         # k_compact_words: 16,384 workgroups of 256
N_MERGE_BIG = 2048 * 1100 + 300         # k_merge: 2,048 words a workgroup on the resident grid


# ------------------------------------------------------------------- signatures --
def sig_sym(x):
    x = int(x) & M32
    return (1 << (x & 31)) | (1 << (((x * 0x9E3779B1) & M32) >> 27))


def sig_pair(a, b):
    q = (((((int(a) & M32) * 0x9E3779B1) & M32) + (int(b) & M32)) & M32) * 0x85EBCA6B & M32
    return (1 << (32 + (q >> 27))) | (1 << (32 + ((q >> 22) & 31)))


def sig_need(a, b):
    """The bits a word holding the adjacent pair (a, b) has set."""
    return sig_sym(a) | sig_sym(b) | sig_pair(a, b)


def sig_of(word):
    g, prev = 0, None
    for y in word:
        g |= sig_sym(y)
        if prev is not None:
            g |= sig_pair(prev, y)
        prev = y
    return g


def sigs_i64(words):
    """sig_of per word as the int64 bit patterns a torch tensor holds."""
    return np.array([sig_of(w) for w in words], dtype=np.uint64).view(np.int64) if len(words) else \
        np.zeros(0, dtype=np.int64)


# ----------------------------------------------------------------------- layout --
def layout_np(templates, idx=None):
    """(sym uint16, wstart int32, wlen int32) of the words templates[idx[0]], templates[idx[1]], ...
    (all templates in order when idx is None) in the layout of beast_bpe_repack_words: spans in
    order, each a multiple of 4 symbols, padded with zeros."""
    T = len(templates)
    lens = np.array([len(w) for w in templates], dtype=np.int64)
    pad = (lens + 3) // 4 * 4
    tsym = np.zeros((max(T, 1), max(int(pad.max()) if T else 0, 4)), dtype=np.uint16)
    for i, w in enumerate(templates):
        tsym[i, :len(w)] = w
    idx = np.arange(T, dtype=np.int64) if idx is None else np.asarray(idx, dtype=np.int64)
    span = pad[idx] if idx.size else np.zeros(0, dtype=np.int64)
    ws = np.concatenate([[0], np.cumsum(span)]).astype(np.int64)
    wid = np.repeat(np.arange(idx.size), span)
    pos = np.arange(int(ws[-1])) - ws[:-1][wid]
    sym = tsym[idx[wid], pos] if idx.size else np.zeros(0, dtype=np.uint16)
    assert ws[-1] < 2 ** 31
    return sym, ws[:-1].astype(np.int32), (lens[idx] if idx.size else lens[:0]).astype(np.int32)


def live_symbols(sym, wstart, wlen):
    """The symbols of every word's live prefix sym[wstart : wstart + wlen], concatenated."""
    wlen = np.asarray(wlen, dtype=np.int64)
    ws = np.asarray(wstart, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(wlen)])
    wid = np.repeat(np.arange(wlen.size), wlen)
    return sym[ws[wid] + (np.arange(int(off[-1])) - off[:-1][wid])]


def lists_to_words(words, counts, device):
    """NumpyBpeOps' lists as the dict GpuBpeOps' merge loop reads (torch tensors on ``device``);
    ``counts`` None leaves wcount out (the kernels then count every word once).  Arrays are never
    empty (a pointer must not be null): n_words says how much of them counts."""
    sym, ws, wl = layout_np(words)
    n = len(words)

    def t(a, dtype, fill=0):
        a = np.ascontiguousarray(a, dtype=dtype)
        return torch.from_numpy(a if a.size else np.full(1, fill, dtype=dtype)).to(device)
    d = {"sym": t(sym.view(np.int16), np.int16), "wstart": t(ws, np.int32), "wlen": t(wl, np.int32),
         "wcount": None if counts is None else t(np.asarray(counts, dtype=np.int64), np.int32),
         "sig": t(sigs_i64(words), np.int64), "n_words": n, "n_syms_padded": int(sym.size)}
    return d


def words_to_lists(d):
    """The dict of the device layout as NumpyBpeOps' {"words": [[ids]], "counts": [...]}."""
    n = d["n_words"]
    sym = d["sym"].cpu().numpy().view(np.uint16)
    ws = d["wstart"].cpu().numpy()[:n].astype(np.int64)
    wl = d["wlen"].cpu().numpy()[:n].astype(np.int64)
    wc = d.get("wcount")
    counts = [1] * n if wc is None else [int(c) for c in wc.cpu().numpy()[:n]]
    return {"words": [sym[a:a + k].tolist() for a, k in zip(ws, wl)], "counts": counts, "n_words": n}


# ------------------------------------------------------------------- references --
def count_pairs_layout(sym, wstart, wlen, wcount, Vt):
    """[Vt, Vt] int64 pair counts of words in the device layout (wcount None: every word once)."""
    wl = np.asarray(wlen, dtype=np.int64)
    npairs = np.maximum(wl - 1, 0)
    off = np.concatenate([[0], np.cumsum(npairs)])
    wid = np.repeat(np.arange(wl.size), npairs)
    at = np.asarray(wstart, dtype=np.int64)[wid] + (np.arange(int(off[-1])) - off[:-1][wid])
    x, y = sym[at].astype(np.int64), sym[at + 1].astype(np.int64)
    w = np.ones(at.size, dtype=np.int64) if wcount is None else np.asarray(wcount, dtype=np.int64)[wid]
    table = np.zeros(Vt * Vt, dtype=np.int64)
    np.add.at(table, x * Vt + y, w)
    return table.reshape(Vt, Vt)


def count_pairs_np(words, counts, Vt):
    """NumpyBpeOps.count_pairs, vectorised: [Vt, Vt] int64."""
    sym, ws, wl = layout_np(words)
    return count_pairs_layout(sym, ws, wl, None if counts is None else np.asarray(counts, dtype=np.int64), Vt)


def merge_templates(templates, mult, a, b, nid, max_len, Vt, tlen):
    """NumpyBpeOps.merge of (a, b) -> nid on the template words alone, template t counted mult[t]
    times: the pair-count changes [4, Vt] int64 of any word list drawn from the templates whose
    counts sum to mult per template (the changes are linear in the counts), and the merged
    templates.  The cost is that of len(templates) words."""
    assert len(templates) <= 64 and len(mult) == len(templates)
    ops = NumpyBpeOps()
    ops.new_state(Vt, np.asarray(tlen))
    merged = [list(w) for w in templates]
    d = ops.merge({"words": merged, "counts": [int(m) for m in mult]}, a, b, nid, max_len, Vt)
    return d.numpy().reshape(4, Vt).astype(np.int64), merged


# ------------------------------------------------- inputs shared with the CPU timing test --
FILL = [11, 12, 13, 14, 15, 16, 17, 18]   # symbols of the merge tests that are neither a, b nor the new id


def count_words(n_sym, n_words):
    """(templates, idx): words of length 0, 1, 2 and longer over ids < n_sym, self-pairs (x, x)
    and the largest id among them; word w is templates[idx[w]]."""
    rng = np.random.default_rng([5, n_sym])
    top = n_sym - 1
    tpl = [[], [top], [0], [top, top], [0, top], [top, 0], [top, top, top], [0, 0, 0, 0, 0]]
    for L in (2, 2, 3, 3, 4, 5, 7, 9, 12):
        tpl += [rng.integers(0, n_sym, L).tolist() for _ in range(4)]
    idx = rng.integers(0, len(tpl), n_words)
    idx[:min(n_words, len(tpl))] = np.arange(min(n_words, len(tpl)))
    if n_words:
        idx[-1] = 3                       # the last word: a self-pair of the largest id
    return tpl, idx


def sig_templates():
    """64 words: of 0, 1, 2, 48, 49 and 300 symbols with ids up to 65,534, then short ones."""
    rng = np.random.default_rng(6)
    tpl = [[], [65534], [65534, 0], rng.integers(0, 65535, 48).tolist(), rng.integers(0, 65535, 49).tolist(),
           rng.integers(0, 65535, 300).tolist()]
    tpl += [rng.integers(0, 65535, L).tolist() for L in rng.integers(0, 7, 58)]
    return tpl


def big_sig_index(n_templates):
    """N_SIG_BIG words: short templates, every 997th one of the first six, the last of 49 symbols."""
    idx = np.random.default_rng(7).integers(6, n_templates, N_SIG_BIG)
    idx[::997] = np.arange(idx[::997].size) % 6
    idx[-1] = 4
    return idx


def big_merge_templates(a, b):
    """64 template words that all hold (a, b): short ones, and words of 48, 49 and 50 symbols."""
    rng = np.random.default_rng(10)
    tpl = []
    for t in range(61):
        L = 2 + t % 6
        w = [FILL[int(k)] for k in rng.integers(0, len(FILL), L)]
        at = int(rng.integers(0, L - 1))
        w[at], w[at + 1] = a, b
        if t % 7 == 0 and L >= 4:
            w[L - 2], w[L - 1] = a, b
        tpl.append(w)
    for L in (48, 49, 50):
        w = [FILL[int(k)] for k in rng.integers(0, len(FILL), L)]
        w[3], w[4], w[L - 2], w[L - 1] = a, b, a, b
        tpl.append(w)
    return tpl


def big_merge_index():
    """(idx, wcount) of N_MERGE_BIG words over big_merge_templates: every 997th a long one."""
    rng = np.random.default_rng(11)
    idx = rng.integers(0, 61, N_MERGE_BIG)
    idx[::997] = 61 + np.arange(idx[::997].size) % 3
    return idx, rng.integers(1, 4, N_MERGE_BIG).astype(np.int32)


def compact_inputs(n_words):
    """(wstart, wlen, wcount) int32: every third length below 2 (0 and 1 in turn)."""
    i = np.arange(n_words, dtype=np.int64)
    wl = (2 + (i * 7) % 300).astype(np.int32)
    wl[::3] = (i[::3] // 3) % 2
    return (4 * i).astype(np.int32), wl, (1 + i % 1000).astype(np.int32)


def compact_key(ws, wl, wc):
    """One sortable int64 per (start < 2^31, length < 2^12, count < 2^20) triple."""
    return (ws.astype(np.int64) << 32) | (wl.astype(np.int64) << 20) | wc.astype(np.int64)
