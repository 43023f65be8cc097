"""k_encode_v (one wave per trajectory; in its 16-wave form the bounds, the quantiser scales, the DoF
columns and the lane-only LDS offsets come from a table that one wave builds in front of the tile
barrier) against the tile-walking k_encode, bitwise, and against the oracle.

The comparison kernel is the specialised k_encode, forced with BEAST_OPT_BLOCK_WAVES 7 and 4: it
still stages the bounds by DMA and computes its scales per column.  Params and tokens must be the same
bits.  Against the oracle the project's existing bars hold (test_gpu_codec_dispatch.py):
  * params: |gpu - fit_exact| <= (Tp + 8) * 2^-24 * sum_t |P[n,t]| |y[t]| + 1e-30;
  * tokens: bit-equal to continuous_to_discrete(clamp(params_gpu)) on the kernel's own params.

Every launch is checked through BEAST_OPT_LAST_CODEC_LAUNCH to be the kernel it is meant to be.
"""
import numpy as np
import pytest
import torch

from beast_tokenizer_amd import BEASTBsplineTokenizer, _lib
from beast_tokenizer_amd.synthetic import synth_trajectories
from oracle import beast_oracle as O

pytestmark = pytest.mark.gpu

F32 = np.float32
TAU = F32(2 * np.pi)
T, N, D = 50, 10, 14
DN = D * N
BATCHES = (1, 15, 16, 17, 33)       # one live wave, the last wave missing, a full tile, one past, two tiles and one
GRIPS = {14: None, 12: [12, 13]}    # joint_dof -> gripper DoFs: one basis kind, two
INT64_MIN = -2 ** 63
OFF = 32000 - 256
PERM = [5, 0, 13, 2, 9, 7, 1, 12, 3, 11, 4, 10, 6, 8]   # a dof_src without fixed structure (a permutation)
V_LAT = dict(family="encode_v", tile=16, waves=16, latency=True)
V_BULK = dict(family="encode_v", tile=8, waves=8, latency=False)
DEV = "cuda:0"


def _spec(waves):
    return dict(family="encode_spec", tile=8, waves=waves)


def _set_waves(w):
    lib = _lib.load()
    assert lib.beast_set_option(_lib.OPT_GENERIC_KERNELS, 0) == 0
    assert lib.beast_set_option(_lib.OPT_BLOCK_WAVES, w) == 0


def _ran(fields):
    m = _lib.last_codec_launch()
    got = {k: getattr(m, k) for k in fields}
    assert got == fields, f"launch took another branch: {m}"


def _same(a, b, what):
    a = a.detach().cpu().numpy().reshape(-1)
    b = b.detach().cpu().numpy().reshape(-1)
    a, b = a.view(np.int32), b.view(np.int32)
    bad = np.argwhere(a != b)
    assert bad.size == 0, f"{what}: {len(bad)} words differ, first at {bad[0].tolist()}"


def _dev(a, dtype=None):
    return torch.from_numpy(np.array(a, order="C")).to(DEV, dtype=dtype)   # a copy: the shared references are read-only


_TOK = {}


def _tok(jd):
    """The tokenizer whose plan supplies the projection and the DoF order; shared, never modified."""
    if jd not in _TOK:
        grip = GRIPS[jd]
        tok = BEASTBsplineTokenizer(num_dof=D, num_basis=N, seq_len=T, vocab_size=256, degree_p=4,
                                    gripper_zero_order=bool(grip), gripper_indices=grip, device=DEV)
        assert tok.joint_dof == jd
        _TOK[jd] = (tok, O.Layout.make(D, grip, bool(grip)))
    return _TOK[jd]


_REF = {}


def _ref(jd, B, src):
    """(x [B,T,D], the float64 fit rounded once [B, D*N] of DoF i <- column src[i], the bound's sums,
    bounds at the 5 % / 95 % quantiles of that fit); shared, never modified."""
    key = (jd, B, tuple(src))
    if key not in _REF:
        x = synth_trajectories(max(B, 64), T, D, seed=300 + jd, gripper_indices=GRIPS[jd] or ())[:B]
        t = O.times_grid(2 * np.pi, T)
        exact, sums = [], []
        for idx, deg in ((list(src[:jd]), 4), (list(src[jd:]), 0)):
            if idx:
                phi = O.basis(t, TAU, deg, N)
                y = x[..., idx]
                exact.append(O.fit_exact(y, phi))
                sums.append(np.einsum("nt,btd->bdn", np.abs(O.projection_f64(phi)),
                                      np.abs(y.astype(np.float64))).reshape(B, -1))
        exact, sums = np.concatenate(exact, axis=-1), np.concatenate(sums, axis=-1)
        big = _ref(jd, 64, src)[1] if B < 64 else exact      # bounds from 64 trajectories, whatever B
        lo = np.quantile(big, 0.05, axis=0).astype(F32)
        hi = np.maximum(np.quantile(big, 0.95, axis=0).astype(F32), lo + F32(1e-3))
        for a in (x, exact, sums, lo, hi):
            a.setflags(write=False)
        _REF[key] = (x, exact, sums, lo, hi)
    return _REF[key]


def _c_enc(jd, x_t, vocab, off, lo_t, hi_t, src_t, want_tokens=True, params=None, tokens=None):
    """beast_encode_f32 with the caller's own bounds, vocabulary, offset and DoF map: (params, tokens)."""
    tok, _ = _tok(jd)
    p = tok._plan()
    B = x_t.shape[0]
    if params is None:
        params = torch.full((B, DN), float("nan"), device=DEV)
    if tokens is None and want_tokens:
        tokens = torch.full((B, DN), -7777, dtype=torch.int64, device=DEV)
    rc = _lib.load().beast_encode_f32(
        x_t.data_ptr(), B, T, x_t.stride(0), x_t.stride(1), x_t.stride(2), D, D, jd, src_t.data_ptr(), p.p_proj, N,
        _lib.ptr(lo_t) if want_tokens else None, _lib.ptr(hi_t) if want_tokens else None, vocab, off,
        params.data_ptr(), _lib.ptr(tokens) if want_tokens else None, _lib.raw_stream(p.idx))
    _lib.check(rc, "beast_encode_f32")
    return params, tokens


def _three(jd, x_t, vocab, off, lo_t, hi_t, src_t, what, first=V_LAT, want_tokens=True):
    """Params and tokens of k_encode_v, checked bitwise against the 7- and the 4-wave k_encode."""
    try:
        _set_waves(0)
        pv, tv = _c_enc(jd, x_t, vocab, off, lo_t, hi_t, src_t, want_tokens)
        _ran(first)
        for w in (7, 4):
            _set_waves(w)
            pw, tw = _c_enc(jd, x_t, vocab, off, lo_t, hi_t, src_t, want_tokens)
            _ran(_spec(w))
            torch.cuda.synchronize()
            _same(pv, pw, f"{what}: params of k_encode_v against the {w}-wave k_encode")
            if want_tokens:
                _same(tv, tw, f"{what}: tokens of k_encode_v against the {w}-wave k_encode")
    finally:
        _set_waves(0)
    return pv.cpu().numpy(), (tv.cpu().numpy() if want_tokens else None)


def _want_tokens(params, lo, hi, vocab, off, B):
    """The oracle's quantiser on the kernel's own params, (n d) order, offset added with int64 wrap."""
    with np.errstate(all="ignore"):
        w = O.continuous_to_discrete(O._clamp_t(params, lo, hi), lo, hi, vocab)
    w = w.reshape(B, D, N).transpose(0, 2, 1).reshape(B, DN).astype(np.int64)
    return (w.view(np.uint64) + np.uint64(off)).view(np.int64) if off else w


def _params_ok(params, exact, sums):
    bound = (52 + 8) * 2.0 ** -24 * sums + 1e-30
    assert np.all(np.abs(params - exact) <= bound), float(np.max(np.abs(params - exact) / bound))


def _src(jd, perm):
    _, lay = _tok(jd)
    return list(PERM) if perm else list(lay.order)


def _bulk_B():
    return 16 * torch.cuda.get_device_properties(0).multi_processor_count + 11


@pytest.mark.parametrize("B", BATCHES + ("bulk",))
@pytest.mark.parametrize("jd", (14, 12))
def test_batches_maps_offsets(jd, B):
    """Every workgroup shape (and the 8-wave bulk form) x identity / permuted dof_src x LLM offset."""
    first = V_BULK if B == "bulk" else V_LAT
    B = _bulk_B() if B == "bulk" else B
    for perm in (False, True):
        src = _src(jd, perm)
        x, exact, sums, lo, hi = _ref(jd, B, src)
        x_t, lo_t, hi_t = _dev(x), _dev(lo), _dev(hi)
        src_t = torch.tensor(src, dtype=torch.int32, device=DEV)
        for off in (0, OFF):
            params, tokens = _three(jd, x_t, 256, off, lo_t, hi_t, src_t, f"B={B} perm={perm} off={off}", first)
            _params_ok(params, exact, sums)
            assert np.array_equal(tokens, _want_tokens(params, lo, hi, 256, off, B))
            if B >= 16:
                assert (params < lo).any() and (params > hi).any()      # both clamp sides


@pytest.mark.parametrize("vocab", (2, 256, 4096))
@pytest.mark.parametrize("jd", (14, 12))
def test_vocabularies(jd, vocab):
    B = 33
    src = _src(jd, True)
    x, exact, sums, lo, hi = _ref(jd, B, src)
    src_t = torch.tensor(src, dtype=torch.int32, device=DEV)
    params, tokens = _three(jd, _dev(x), vocab, 0, _dev(lo), _dev(hi), src_t, f"vocab={vocab}")
    want = _want_tokens(params, lo, hi, vocab, 0, B)
    assert np.array_equal(tokens, want)
    assert want.min() == 0 and want.max() == vocab - 1


@pytest.mark.parametrize("jd", (14, 12))
def test_degenerate_bounds(jd):
    """Single columns with hi - lo < 1e-8 (both signs of zero width included), inverted bounds, inf and NaN
    bounds; the columns beside them keep the oracle's bins."""
    B = 33
    src = _src(jd, False)
    x, exact, sums, lo0, hi0 = _ref(jd, B, src)
    lo, hi = lo0.copy(), hi0.copy()
    hi[3] = lo[3] + F32(1e-9)                  # narrower than the 1e-8 floor
    hi[17] = lo[17]                            # zero width
    lo[29], hi[29] = hi0[29], lo0[29]          # inverted
    hi[44] = F32(np.inf)
    lo[58] = F32(-np.inf)
    lo[71], hi[71] = F32(-np.inf), F32(np.inf)
    nan_cols = [86, 99, 139]
    lo[86] = F32(np.nan)
    hi[99] = F32(np.nan)
    lo[139], hi[139] = F32(np.nan), F32(np.nan)
    src_t = torch.tensor(src, dtype=torch.int32, device=DEV)
    for off in (0, OFF):
        params, tokens = _three(jd, _dev(x), 256, off, _dev(lo), _dev(hi), src_t, f"degenerate bounds, off={off}")
        _params_ok(params, exact, sums)
        want = _want_tokens(params, lo, hi, 256, off, B).reshape(B, N, D)
        for c in nan_cols:                     # NaN bounds: clamp gives NaN, .to(int64) gives INT64_MIN (+ offset, wrapped)
            want[:, c % N, c // N] = INT64_MIN + off
        assert np.array_equal(tokens.reshape(B, N, D), want)


@pytest.mark.parametrize("vocab", (256, 4096))
@pytest.mark.parametrize("jd", (14, 12))
def test_rounding_boundaries_in_one_trajectory(jd, vocab):
    """Every column's bounds are placed so that one trajectory's param lies within 2^-20 (V - 1) of a rounding
    boundary (j + 0.5) / (V - 1), on either side of it: that trajectory's lanes take the exactly-rounded
    chain, the other trajectories of its tile must keep their bins."""
    B, planted = 33, 21
    src = _src(jd, False)
    x, exact, sums, lo0, hi0 = _ref(jd, B, src)
    src_t = torch.tensor(src, dtype=torch.int32, device=DEV)
    x_t = _dev(x)
    params0, _ = _three(jd, x_t, vocab, 0, _dev(lo0), _dev(hi0), src_t, "before planting")
    p = params0[planted].astype(np.float64)
    s = (hi0 - lo0).astype(np.float64)
    jb = (np.arange(DN) * 37) % (vocab - 1)                                   # the boundary j + 0.5 of each column
    eps = np.where(np.arange(DN) % 2 == 0, 1, -1) * 2.0 ** -22 * (np.arange(DN) % 3)   # 0 or a quarter of the window
    lo = (p - (jb + 0.5 + eps * (vocab - 1)) * s / (vocab - 1)).astype(F32)
    hi = (lo.astype(np.float64) + s).astype(F32)
    va = (p - lo) / (hi.astype(np.float64) - lo) * (vocab - 1)
    assert np.all(np.abs(va - np.floor(va) - 0.5) < 2.0 ** -20 * (vocab - 1)), "the planted params are near boundaries"
    params, tokens = _three(jd, x_t, vocab, 0, _dev(lo), _dev(hi), src_t, f"planted, vocab={vocab}")
    assert np.array_equal(params, params0)
    assert np.array_equal(tokens, _want_tokens(params, lo, hi, vocab, 0, B))


@pytest.mark.parametrize("jd", (14, 12))
def test_nan_inf_samples_in_one_trajectory(jd):
    """A NaN sample in one trajectory and an inf sample in another of the same tile: their own tokens are the
    k_encode's, every other trajectory's params and bins do not move."""
    B = 33
    src = _src(jd, True)
    x, exact, sums, lo, hi = _ref(jd, B, src)
    src_t = torch.tensor(src, dtype=torch.int32, device=DEV)
    lo_t, hi_t = _dev(lo), _dev(hi)
    params0, tokens0 = _three(jd, _dev(x), 256, OFF, lo_t, hi_t, src_t, "clean")
    xb = x.copy()
    xb[5, 17, 3] = np.nan
    xb[9, 40, 11] = np.inf
    xb[20, 0, 0] = -np.inf
    params, tokens = _three(jd, _dev(xb), 256, OFF, lo_t, hi_t, src_t, "NaN / inf samples")
    clean = np.array([b for b in range(B) if b not in (5, 9, 20)])
    assert np.array_equal(params[clean], params0[clean]) and np.array_equal(tokens[clean], tokens0[clean])
    assert not np.isfinite(params[[5, 9, 20]]).all(axis=1).any()
    nan = np.isnan(params).reshape(B, D, N).transpose(0, 2, 1).reshape(B, DN)
    assert nan[5].any() and np.all(tokens[nan] == INT64_MIN + OFF)


@pytest.mark.parametrize("jd", (14, 12))
def test_params_only_with_null_bounds(jd):
    """The compute_weights path: tokens_out, w_min and w_max are null; the params are the full call's."""
    B = 33
    src = _src(jd, True)
    x, exact, sums, lo, hi = _ref(jd, B, src)
    src_t = torch.tensor(src, dtype=torch.int32, device=DEV)
    x_t = _dev(x)
    full, _ = _three(jd, x_t, 256, 0, _dev(lo), _dev(hi), src_t, "full call")
    only, none = _three(jd, x_t, 256, 0, None, None, src_t, "params only", want_tokens=False)
    assert none is None and np.array_equal(only, full)
    _params_ok(only, exact, sums)
    tok, _ = _tok(jd)
    w = tok.compute_weights(x_t)
    _ran(V_LAT)
    ident, _ = _three(jd, x_t, 256, 0, None, None, torch.tensor(_src(jd, False), dtype=torch.int32, device=DEV),
                      "params only, identity map", want_tokens=False)
    assert np.array_equal(w.reshape(B, DN).cpu().numpy(), ident)


@pytest.mark.parametrize("jd", (14, 12))
def test_inplace_bounds_and_map_update(jd):
    """w_min / w_max and dof_src updated in place between two calls on one stream, with no synchronisation in
    between: the second call sees the new values (nothing derived from them outlives a launch)."""
    B = 33
    src, src2 = _src(jd, False), _src(jd, True)
    x, _, _, lo, hi = _ref(jd, B, src)
    lo2, hi2 = (lo * F32(0.5)).astype(F32), (hi * F32(0.75) + F32(0.01)).astype(F32)
    x_t = _dev(x)
    lo_t, hi_t, src_t = _dev(lo), _dev(hi), torch.tensor(src, dtype=torch.int32, device=DEV)
    lo2_t, hi2_t, src2_t = _dev(lo2), _dev(hi2), torch.tensor(src2, dtype=torch.int32, device=DEV)
    _set_waves(0)
    outs = [(torch.empty((B, DN), device=DEV), torch.empty((B, DN), dtype=torch.int64, device=DEV)) for _ in range(3)]
    torch.cuda.synchronize()
    _c_enc(jd, x_t, 256, 0, lo_t, hi_t, src_t, params=outs[0][0], tokens=outs[0][1])
    _ran(V_LAT)
    lo_t.copy_(lo2_t)
    hi_t.copy_(hi2_t)
    _c_enc(jd, x_t, 256, 0, lo_t, hi_t, src_t, params=outs[1][0], tokens=outs[1][1])
    src_t.copy_(src2_t)
    _c_enc(jd, x_t, 256, 0, lo_t, hi_t, src_t, params=outs[2][0], tokens=outs[2][1])
    torch.cuda.synchronize()
    got = [(p.cpu().numpy(), t.cpu().numpy()) for p, t in outs]
    assert np.array_equal(got[0][0], got[1][0]) and not np.array_equal(got[0][1], got[1][1])
    assert not np.array_equal(got[1][0], got[2][0])
    for (pg, tg), (l, h, s) in zip(got, ((lo, hi, src), (lo2, hi2, src), (lo2, hi2, src2))):
        pw, tw = _three(jd, x_t, 256, 0, _dev(l), _dev(h), torch.tensor(s, dtype=torch.int32, device=DEV), "fresh")
        assert np.array_equal(pg, pw) and np.array_equal(tg, tw)
        assert np.array_equal(tg, _want_tokens(pg, l, h, 256, 0, B))


@pytest.mark.parametrize("shift", ((1, 0), (0, 1), (1, 1)))
def test_unaligned_outputs_take_k_encode(shift):
    """Params 4 bytes or tokens 8 bytes past a 16-byte boundary: the launch is k_encode's, the values are
    k_encode_v's, and nothing is written outside the outputs."""
    jd, B = 14, 33
    src = _src(jd, False)
    x, _, _, lo, hi = _ref(jd, B, src)
    x_t, lo_t, hi_t = _dev(x), _dev(lo), _dev(hi)
    src_t = torch.tensor(src, dtype=torch.int32, device=DEV)
    params0, tokens0 = _three(jd, x_t, 256, OFF, lo_t, hi_t, src_t, "aligned")
    ps, ts = shift
    pbuf = torch.full((B * DN + 8,), -7777.0, device=DEV)
    tbuf = torch.full((B * DN + 8,), -7777, dtype=torch.int64, device=DEV)
    pv, tv = pbuf[ps:ps + B * DN].view(B, DN), tbuf[ts:ts + B * DN].view(B, DN)
    assert pv.data_ptr() % 16 == 4 * ps and tv.data_ptr() % 16 == 8 * ts
    _set_waves(0)
    _c_enc(jd, x_t, 256, OFF, lo_t, hi_t, src_t, params=pv, tokens=tv)
    _ran(dict(family="encode_spec", tile=8))
    torch.cuda.synchronize()
    assert np.array_equal(pv.cpu().numpy(), params0) and np.array_equal(tv.cpu().numpy(), tokens0)
    for buf, s in ((pbuf, ps), (tbuf, ts)):
        assert bool((torch.cat([buf[:s], buf[s + B * DN:]]) == -7777).all())
