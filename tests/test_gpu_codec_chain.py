"""The latency-regime per-trajectory kernels (k_encode_v / k_reconstruct_v) against the runtime-shape
kernels (k_encode / k_reconstruct, ``BEAST_OPT_GENERIC_KERNELS = 1``), bitwise.

k_encode_v quantises three slots per lane (rows n = 3 and n = 7 move to other lanes) from bounds it
loads into registers before its tile barrier; k_reconstruct_v does the same for its bounds, DoF map
and basis operands.  Nothing derived from the bounds may outlive a launch, and every slot class
(n in {0, 3, 4, 7, 8, 9} x d in {0, 13}, and the gripper DoFs) must meet every kind of bound, a value
on either side of a rounding tie (the exact fallback), and tokens outside the dequantise LUT.

Floats are compared as int32 views, so NaNs compare.  Every case asserts through
``_lib.last_codec_launch()`` that the per-trajectory latency family really ran.  The float64-oracle
tolerances of both kernel families are test_gpu_codec_dispatch.py's and test_gpu_parity.py's.
"""
import numpy as np
import pytest
import torch

from beast_tokenizer_amd import BEASTBsplineTokenizer, _lib
from beast_tokenizer_amd.synthetic import synth_trajectories
from oracle import beast_oracle as O

pytestmark = pytest.mark.gpu

F32 = np.float32
T, N, D, V = 50, 10, 14, 256
BATCHES = (1, 15, 16, 17, 33)       # a partial tile, one tile, a tile plus one, two tiles plus one
GRIPS = {14: None, 12: [12, 13]}    # joint_dof -> gripper DoFs: the two specialised instantiations
SLOT_N = (0, 3, 4, 7, 8, 9)         # rows of every quantiser slot class (3 and 7 are the moved ones)
ENC_LAT = dict(family="encode_v", tile=16, waves=16, latency=True)
REC_LAT = dict(family="reconstruct_v", tile=16, waves=16, ks=3, latency=True)
INT64_MIN = -2 ** 63
NKINDS = 7                          # kinds of special bounds, _special_bounds


def _slot_columns(jd):
    """(d n) columns of the slot classes: n in SLOT_N x d in {0, 13}, and DoF 12 with grippers."""
    ds = (0, 13) if jd == 14 else (0, 12, 13)
    return [d * N + n for d in ds for n in SLOT_N]


def _set_generic(v):
    lib = _lib.load()
    assert lib.beast_set_option(_lib.OPT_GENERIC_KERNELS, int(v)) == 0
    assert lib.beast_set_option(_lib.OPT_BLOCK_WAVES, 0) == 0


def _ran(fields):
    m = _lib.last_codec_launch()
    got = {k: getattr(m, k) for k in fields}
    assert got == fields, f"launch took another branch: {m}"


def _bits(t):
    a = t.detach().cpu().numpy()
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(a, b, what):
    a, b = _bits(a), _bits(b)
    bad = np.argwhere(a != b)
    assert bad.size == 0, f"{what}: {len(bad)} elements differ, first at {bad[0].tolist()}"


_DATA = {}


def _data(jd):
    """(x [33, T, D], ordinary w_min, w_max): shared among the cases, never modified."""
    if jd not in _DATA:
        x = synth_trajectories(max(BATCHES), T, D, seed=700 + jd, gripper_indices=GRIPS[jd] or ())
        t = O.times_grid(2 * np.pi, T)
        lay = O.Layout.make(D, GRIPS[jd], bool(GRIPS[jd]))
        fit = [O.fit_exact(x[..., idx], O.basis(t, F32(2 * np.pi), deg, N))
               for idx, deg in ((lay.joint_indices, 4), (lay.gripper_indices, 0)) if idx]
        p = np.concatenate(fit, axis=-1)
        lo, hi = np.quantile(p, 0.1, axis=0).astype(F32), np.quantile(p, 0.9, axis=0).astype(F32)
        hi = np.maximum(hi, lo + F32(1e-3)).astype(F32)
        for a in (x, lo, hi):
            a.setflags(write=False)
        _DATA[jd] = (x, lo, hi)
    return _DATA[jd]


def _tok(jd, lo, hi, llm=None):
    grip = GRIPS[jd]
    tok = BEASTBsplineTokenizer(num_dof=D, num_basis=N, seq_len=T, vocab_size=V, degree_p=4,
                                gripper_zero_order=bool(grip), gripper_indices=grip, device="cuda:0",
                                llm_vocab_size=llm)
    _set_bounds(tok, lo, hi)
    assert tok.joint_dof == jd
    return tok


def _set_bounds(tok, lo, hi):
    """In place: the tokenizer's plan, and the pointers it holds, stay as they are."""
    tok.w_min.copy_(torch.from_numpy(np.ascontiguousarray(lo)).to(tok.w_min.device))
    tok.w_max.copy_(torch.from_numpy(np.ascontiguousarray(hi)).to(tok.w_max.device))


def _special_bounds(jd, lo, hi, rot):
    """Bounds with the slot-class columns made special; column i of the list gets kind (i + rot) % 7,
    so NKINDS rotations put every kind into every slot class."""
    lo, hi = lo.copy(), hi.copy()
    for i, c in enumerate(_slot_columns(jd)):
        kind = (i + rot) % NKINDS
        if kind == 0:
            hi[c] = lo[c] + F32(1e-9) * max(F32(1), abs(lo[c]))   # hi - lo < 1e-8 (or 0)
        elif kind == 1:
            lo[c], hi[c] = hi[c], lo[c]                           # lo > hi
        elif kind == 2:
            lo[c] = np.nan
        elif kind == 3:
            hi[c] = np.nan
        elif kind == 4:
            lo[c], hi[c] = -np.inf, np.inf
        elif kind == 5:
            hi[c] = np.inf
        else:
            lo[c] = -np.inf
    tiny = [c for i, c in enumerate(_slot_columns(jd)) if (i + rot) % NKINDS == 0]
    assert np.all(hi[tiny] - lo[tiny] < 1e-8)
    return lo, hi


def _encode_both(tok, x):
    """(tokens, params) of the per-trajectory kernel and of the runtime-shape kernel."""
    try:
        _set_generic(0)
        t1, d1 = tok.encode(x)
        _ran(ENC_LAT)
        _set_generic(1)
        t0, d0 = tok.encode(x)
        assert _lib.last_codec_launch().family == "encode_dyn"
    finally:
        _set_generic(0)
    return (t1, d1["params"]), (t0, d0["params"])


def _rec_both(tok, tokens, **kw):
    try:
        _set_generic(0)
        p1 = tok.reconstruct_traj(tokens, **kw)
        _ran(REC_LAT)
        _set_generic(1)
        p0 = tok.reconstruct_traj(tokens, **kw)
        assert _lib.last_codec_launch().family == "reconstruct_mfma"
    finally:
        _set_generic(0)
    return p1, p0


# ------------------------------------------------------------------------------------- encode --
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("jd", (14, 12))
def test_encode_bounds(jd, B):
    """Ordinary bounds, then every kind of special bound in every slot class."""
    x, lo, hi = _data(jd)
    xd = torch.from_numpy(x[:B]).cuda()
    tok = _tok(jd, lo, hi)
    (t1, p1), (t0, p0) = _encode_both(tok, xd)
    _same(t1, t0, "tokens, ordinary bounds")
    _same(p1, p0, "params, ordinary bounds")
    for rot in range(NKINDS):
        _set_bounds(tok, *_special_bounds(jd, lo, hi, rot))
        (t1, p1), (t0, p0) = _encode_both(tok, xd)
        _same(t1, t0, f"tokens, special bounds rotation {rot}")
        _same(p1, p0, f"params, special bounds rotation {rot}")
    nd = t1.cpu().numpy().reshape(B, N, D)
    assert (nd == INT64_MIN).any(), "NaN bounds must give the NaN token somewhere"


@pytest.mark.parametrize("llm", (None, 32000))
@pytest.mark.parametrize("jd", (14, 12))
def test_encode_ties(jd, llm):
    """Params a few ulps either side of a .5 rounding boundary in every slot class: the exact
    fallback decides, in the moved lanes too.  Column c ties trajectory c % B at bin k = c % 32:
    lo = p - (k + 0.5) / (V - 1) * (hi - lo) in float64, rounded to f32, then nudged by -1, 0 or +1 ulp.
    The range hi - lo is a power of two >= 4 max |p| of the column, so rounding lo and hi to f32 moves
    the units by about 255 * 2^-24 * 0.4 = 6e-6 and the f32 chain's own rounding at units <= 32 by a few
    32 * 2^-24 = 2e-6: both well inside the window of 2^-20 * (V - 1) = 2.4e-4."""
    B = 17
    x, lo0, hi0 = _data(jd)
    xd = torch.from_numpy(x[:B]).cuda()
    tok = _tok(jd, lo0, hi0, llm)
    _set_generic(0)
    p = tok.encode(xd)[1]["params"].cpu().numpy()            # the fit, once
    s = 2.0 ** np.ceil(np.log2(np.maximum(4 * np.abs(p).max(axis=0).astype(np.float64), 2.0 ** -6)))
    cols = np.arange(D * N)
    k = cols % 32
    pc = p[cols % B, cols].astype(np.float64)
    lo = (pc - (k + 0.5) / (V - 1) * s).astype(F32)
    nudge = cols % 3
    lo = np.where(nudge == 0, np.nextafter(lo, F32(-np.inf)), np.where(nudge == 2, np.nextafter(lo, F32(np.inf)), lo))
    lo = lo.astype(F32)
    hi = (lo.astype(np.float64) + s).astype(F32)
    units = O.normalized_units(p, lo, hi, V)
    frac = np.abs(units - np.floor(units) - F32(0.5))
    window = 2.0 ** -20 * (V - 1)
    for c in _slot_columns(jd):
        print(f"column d={c // N} n={c % N}: min |frac - .5| = {frac[:, c].min():.3e} (window {window:.3e})")
    for c in _slot_columns(jd):
        assert frac[:, c].min() < window, f"no tie inside the window in column d={c // N} n={c % N}"
    _set_bounds(tok, lo, hi)
    (t1, p1), (t0, p0) = _encode_both(tok, xd)
    _same(t1, t0, "tokens at rounding ties")
    _same(p1, p0, "params at rounding ties")
    off = 0 if llm is None else llm - V
    assert int(t1.min()) >= off and int(t1.max()) < off + V


@pytest.mark.parametrize("jd", (14, 12))
def test_encode_inplace_bounds_update(jd):
    """Bounds updated in place between two launches: the second launch uses the new ones."""
    B = 33
    x, lo, hi = _data(jd)
    xd = torch.from_numpy(x[:B]).cuda()
    tok = _tok(jd, lo, hi)
    _set_generic(0)
    first = tok.encode(xd)[0].clone()
    _ran(ENC_LAT)
    tok.w_min.mul_(0.5)
    tok.w_max.copy_(torch.from_numpy(hi * F32(0.75) + F32(0.01)).to(tok.w_max.device))
    (t1, p1), (t0, p0) = _encode_both(tok, xd)
    _same(t1, t0, "tokens after the in-place update")
    _same(p1, p0, "params after the in-place update")
    assert not torch.equal(first, t1), "the new bounds must change the tokens"


# -------------------------------------------------------------------------------- reconstruct --
def _tokens(jd, B, off, wild):
    """Tokens [B, N * D] in (n d) order: in range; with `wild`, every slot-class column of some
    trajectories holds a negative token, one >= V, or INT64_MIN."""
    rng = np.random.default_rng(900 + jd + B)
    t = rng.integers(0, V, size=(B, N, D), dtype=np.int64) + off
    if wild:
        for i, c in enumerate(_slot_columns(jd)):
            d, n = c // N, c % N
            t[i % B, n, d] = (-1 - i, V + i, INT64_MIN, off - 1, off + V, 2 ** 40)[i % 6]
    return torch.from_numpy(t.reshape(B, N * D)).cuda()


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("jd", (14, 12))
def test_reconstruct_tokens(jd, B):
    """In-range tokens and tokens outside [0, lut_n), with and without the LLM offset and init_p."""
    _, lo, hi = _data(jd)
    init_p = torch.from_numpy(np.random.default_rng(B).standard_normal((B, D)).astype(F32)).cuda()
    for llm in (None, 32000):
        tok = _tok(jd, lo, hi, llm)
        off = 0 if llm is None else llm - V
        for wild in (False, True):
            tk = _tokens(jd, B, off, wild)
            for kw in ({}, {"init_p": init_p}):
                p1, p0 = _rec_both(tok, tk, **kw)
                _same(p1, p0, f"positions, llm={llm} wild={wild} init_p={bool(kw)}")


@pytest.mark.parametrize("B", (1, 17))
@pytest.mark.parametrize("jd", (14, 12))
def test_reconstruct_bounds(jd, B):
    """Every kind of special bound in every slot class, tokens in and out of range, init_p."""
    _, lo, hi = _data(jd)
    tok = _tok(jd, lo, hi)
    init_p = torch.from_numpy(np.random.default_rng(B).standard_normal((B, D)).astype(F32)).cuda()
    for rot in range(NKINDS):
        _set_bounds(tok, *_special_bounds(jd, lo, hi, rot))
        for wild in (False, True):
            tk = _tokens(jd, B, 0, wild)
            for kw in ({}, {"init_p": init_p}):
                p1, p0 = _rec_both(tok, tk, **kw)
                _same(p1, p0, f"positions, rotation {rot} wild={wild} init_p={bool(kw)}")
    assert p1.isnan().any(), "NaN bounds must give NaN positions somewhere"


@pytest.mark.parametrize("jd", (14, 12))
def test_reconstruct_inplace_bounds_update(jd):
    B = 33
    _, lo, hi = _data(jd)
    tok = _tok(jd, lo, hi)
    tk = _tokens(jd, B, 0, False)
    _set_generic(0)
    first = tok.reconstruct_traj(tk).clone()
    _ran(REC_LAT)
    tok.w_min.mul_(0.5)
    tok.w_max.copy_(torch.from_numpy(hi * F32(0.75) + F32(0.01)).to(tok.w_max.device))
    p1, p0 = _rec_both(tok, tk)
    _same(p1, p0, "positions after the in-place update")
    assert not torch.equal(first, p1), "the new bounds must change the positions"
