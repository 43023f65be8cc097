"""``beast_roundtrip_stats_f32`` / ``reconstruction_stats`` against the existing path.

The yardstick is never the kernel under test: ``tokens_ref, params_ref = encode(x)`` with the bounds
fixed, ``pos_ref = reconstruct_traj(tokens_ref)``, and tests/roundtrip_oracle.py turns those into the
float64 statistics and their tolerances (the maximum is compared bitwise, which pins the fused
kernel's positions to ``reconstruct_traj``'s to the bit; the clip counts and tokens are exact).
Every raw call starts from NaN-filled statistics and -1-filled tokens, so an element the kernel
leaves unwritten fails.
"""
import numpy as np
import pytest
import torch

import roundtrip_oracle as R
from beast_tokenizer_amd import BEASTBsplineBPETokenizer, BEASTBsplineTokenizer, _lib
from beast_tokenizer_amd.synthetic import synth_trajectories
from conftest import CONFIGS

pytestmark = pytest.mark.gpu

F32 = np.float32
NREF = 64          # trajectories the bounds of a shape are taken from

K2 = dict(T=50, N=10, D=14, grip=None)
K3 = dict(T=50, N=10, D=14, grip=(6, 13))
K1 = dict(T=50, N=10, D=7, grip=None)
SMALL = dict(T=13, N=5, D=3, grip=(1,))
LIMIT = dict(T=256, N=16, D=64, grip=(10, 20, 40, 63))


def _set_generic(v):
    assert _lib.load().beast_set_option(_lib.OPT_GENERIC_KERNELS, v) == 0


_SETUP = {}


def _setup(dev, T, N, D, grip, vocab=256):
    """(tokenizer with bounds at the 10 % / 90 % quantiles of the fit of NREF synthetic trajectories,
    those trajectories on the device), shared among the tests and never modified."""
    key = (T, N, D, grip, vocab)
    if key not in _SETUP:
        tok = BEASTBsplineTokenizer(num_dof=D, num_basis=N, seq_len=T, vocab_size=vocab, gripper_zero_order=bool(grip),
                                    gripper_indices=list(grip) if grip else None, device=str(dev))
        x = synth_trajectories(NREF, T, D, seed=7 + T + D, gripper_indices=grip or ())
        # every trajectory at its own amplitude: the gripper DoFs' +-1 steps alone give params of two
        # values, which no quantile bound clips
        x = torch.from_numpy(x * np.linspace(0.5, 1.5, NREF, dtype=F32)[:, None, None]).to(dev)
        params = tok.compute_weights(x).cpu().numpy()
        lo = np.quantile(params, 0.1, axis=0).astype(F32)
        hi = np.quantile(params, 0.9, axis=0).astype(F32)
        tok.load_state_dict({"w_min": lo.tolist(), "w_max": hi.tolist()})
        _SETUP[key] = (tok, x)
    return _SETUP[key]


def _batch(x64, B):
    """B trajectories from the NREF reference ones (repeated, each repeat scaled differently)."""
    if B <= x64.shape[0]:
        return x64[:B].contiguous()
    reps = -(-B // x64.shape[0])
    x = x64.repeat(reps, 1, 1)[:B]
    scale = torch.linspace(0.5, 1.5, B, device=x.device)[:, None, None]
    return (x * scale).contiguous()


def _raw(tok, ptr, B, strides, row_elems, *, tokens=True, clip=True, offset=0, stats_shift=0, clip_buf=None):
    """One beast_roundtrip_stats_f32 call on NaN / -1 filled outputs: (stats, tokens, clip counts)."""
    p = tok._plan()
    D, N = tok.num_dof, tok.num_basis
    sbuf = torch.full((B * D * 4 + 4,), float("nan"), device=p.dev)
    stats = sbuf[stats_shift:stats_shift + B * D * 4].view(B, D, 4)
    tk = torch.full((B, N * D), -1, dtype=torch.int64, device=p.dev) if tokens else None
    if clip and clip_buf is None:
        clip_buf = torch.zeros((2, D * N), dtype=torch.int32, device=p.dev)
    rc = _lib.load().beast_roundtrip_stats_f32(ptr, B, p.T, strides[0], strides[1], strides[2], row_elems, D,
                                               tok.joint_dof, p.p_src, p.p_proj, p.p_phi, N, p.p_wmn, p.p_wmx,
                                               tok.vocab_size, offset, _lib.ptr(tk), stats.data_ptr(),
                                               _lib.ptr(clip_buf) if clip else None, _lib.raw_stream(p.idx))
    _lib.check(rc, "beast_roundtrip_stats_f32")
    if stats_shift:
        assert bool(torch.isnan(sbuf[:stats_shift]).all()) and bool(torch.isnan(sbuf[stats_shift + B * D * 4:]).all())
    return stats, tk, clip_buf


def _reference(tok, x):
    """The existing path on contiguous x [B, T, Din]: tokens, and the oracle's statistics."""
    dev = x.device
    order = tok.joint_indices + tok.gripper_indices
    B, T = x.shape[:2]
    D, N = tok.num_dof, tok.num_basis
    tokens_ref, pd = tok.encode(x, respect_llm_vocab_size=False)
    pos_ref = tok.reconstruct_traj(tokens_ref) if tok.llm_vocab_size is None else \
        tok._reconstruct(tokens_ref, None, None, None, False, tok._plan())
    cols = torch.tensor(order, device=dev)
    y = x[..., cols].contiguous()
    pos = pos_ref[..., cols].contiguous()
    E = y - pos                                                   # torch fp32
    phi = tok._constants(dev)[0]
    s = R.stats(y.cpu().numpy(), pos.cpu().numpy(), pd["params"].reshape(B, D, N).cpu().numpy(), phi.cpu().numpy(),
                tok.w_min.cpu().numpy(), tok.w_max.cpu().numpy(), tok.joint_dof)
    return tokens_ref, E, s


def _check(tok, x, stats, tokens, clip, *, offset=0, ref=None):
    tokens_ref, E, s = ref if ref is not None else _reference(tok, x)
    if tokens is not None:
        assert torch.equal(tokens, tokens_ref + offset)
    # max_abs bitwise against torch's fp32 subtract / abs / amax (NaN where torch has NaN)
    want = E.abs().amax(dim=1)
    got = stats[..., 2]
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan)
    assert torch.equal(got[~nan].view(torch.int32), want[~nan].view(torch.int32))
    R.assert_stats(stats.cpu().numpy(), s)
    if clip is not None:
        c = clip.cpu().numpy().astype(np.int64)
        assert np.array_equal(c[0], s["clip_low"]) and np.array_equal(c[1], s["clip_high"])
    return tokens_ref, E, s


def _same(a, b):
    """bitwise equality of two result triples (NaN == NaN)."""
    for u, v in zip(a, b):
        assert (u is None) == (v is None)
        if u is not None:
            u, v = u.contiguous(), v.contiguous()
            assert torch.equal(u.view(torch.int32) if u.dtype == torch.float32 else u,
                               v.view(torch.int32) if v.dtype == torch.float32 else v)


# ------------------------------------------------------------------------------- launch shapes --
@pytest.mark.parametrize("shape", [K2, K3, K1], ids=["k2", "k3", "k1"])
@pytest.mark.parametrize("B", [1, 7, 8, 9, 16, 17, 33])
def test_tile_edges(shape, B, gpu_device):
    tok, x64 = _setup(gpu_device, **shape)
    x = _batch(x64, B)
    _set_generic(0)
    spec = _raw(tok, x.data_ptr(), B, x.stride(), x.shape[2])
    ref = _check(tok, x, *spec)
    again = _raw(tok, x.data_ptr(), B, x.stride(), x.shape[2])
    _same(spec, again)                                  # run-to-run identical
    try:
        _set_generic(1)
        gen = _raw(tok, x.data_ptr(), B, x.stride(), x.shape[2])
    finally:
        _set_generic(0)
    _same(spec, gen)                                    # the two instantiations agree to the bit
    _check(tok, x, *gen, ref=ref)


def test_bounds_clip_both_sides_on_every_column(gpu_device):
    """Bounds at the 10 % / 90 % quantiles of the very batch: every column clips on both sides; a
    second call adds to the counts."""
    tok, x = _setup(gpu_device, **K3)
    B = x.shape[0]
    stats, tokens, clip = _raw(tok, x.data_ptr(), B, x.stride(), x.shape[2])
    _, _, s = _check(tok, x, stats, tokens, clip)
    assert s["clip_low"].min() > 0 and s["clip_high"].min() > 0
    _raw(tok, x.data_ptr(), B, x.stride(), x.shape[2], clip_buf=clip)
    c = clip.cpu().numpy().astype(np.int64)
    assert np.array_equal(c[0], 2 * s["clip_low"]) and np.array_equal(c[1], 2 * s["clip_high"])


@pytest.mark.parametrize("shape,B,tile", [(K2, 20001, 8), (K1, 40001, 16), (K3, 20001, 8)],
                         ids=["k2_20001", "k1_40001", "k3_20001"])
def test_many_tiles(shape, B, tile, gpu_device):
    """More tiles than the capped grid has workgroups (8-trajectory tiles at the default shape,
    16-trajectory tiles at D = 7; the launch layer's grid is at most 2 x 8 workgroups per CU), so a
    workgroup walks several tiles and flushes its clip counts once; one trajectory in the last tile.
    B is the least batch for that, never below the parameter (enough up to 78 CUs): 32 tiles per CU
    and one trajectory, and the grid read back after the launch is at most half the tiles."""
    tok, x64 = _setup(gpu_device, **shape)
    cus = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    B = max(B, tile * 32 * cus + 1)
    x = _batch(x64, B)
    out = _raw(tok, x.data_ptr(), B, x.stride(), x.shape[2])
    grid, ntiles = _lib.last_launch_grid(), -(-B // tile)
    assert 0 < grid and 2 * grid <= ntiles, f"grid {grid} for {ntiles} tiles: no workgroup is shown to walk two"
    _check(tok, x, *out)


@pytest.mark.parametrize("shape,B,generic", [(SMALL, 19, 0), (K2, 19, 1), (LIMIT, 3, 0)],
                         ids=["13x5x3", "default_forced_generic", "256x16x64"])
def test_runtime_shapes(shape, B, generic, gpu_device):
    tok, x64 = _setup(gpu_device, **shape)
    x = _batch(x64, B)
    try:
        _set_generic(generic)
        out = _raw(tok, x.data_ptr(), B, x.stride(), x.shape[2])
    finally:
        _set_generic(0)
    _check(tok, x, *out)


@pytest.mark.parametrize("shape", [K3, SMALL], ids=["k3", "13x5x3"])
@pytest.mark.parametrize("layout", ["wide_slice", "transposed", "base4", "stats4", "clip4"])
def test_strided_inputs(shape, layout, gpu_device):
    """Layout variants of one computation equal the contiguous, aligned result bitwise."""
    dev = gpu_device
    tok, x64 = _setup(dev, **shape)
    B = 19
    x = _batch(x64, B)
    T, D = x.shape[1:]
    base = _raw(tok, x.data_ptr(), B, x.stride(), D)
    _check(tok, x, *base)
    shift, clip_buf = 0, None
    if layout == "wide_slice":
        big = torch.full((B, T, D + 2), float("nan"), device=dev)
        big[..., :D] = x
        v = big[..., :D]
        ptr, strides, keep = v.data_ptr(), v.stride(), big
    elif layout == "transposed":
        keep = x.transpose(1, 2).contiguous()              # [B, D, T] storage
        ptr, strides = keep.data_ptr(), (D * T, 1, T)
    elif layout == "base4":
        keep = torch.full((B * T * D + 4,), float("nan"), device=dev)
        v = keep[1:1 + B * T * D].view(B, T, D)
        v.copy_(x)
        assert v.data_ptr() % 16 == 4
        ptr, strides = v.data_ptr(), v.stride()
    elif layout == "stats4":                               # stats_out 4 bytes past a 16-byte boundary
        ptr, strides, keep, shift = x.data_ptr(), x.stride(), x, 1
    else:                                                  # clip_counts 4 bytes past an 8-byte boundary
        ptr, strides, keep = x.data_ptr(), x.stride(), x
        cbuf = torch.zeros((2 * D * tok.num_basis + 2,), dtype=torch.int32, device=dev)
        clip_buf = cbuf[1:-1].view(2, -1)
        assert clip_buf.data_ptr() % 8 == 4
    out = _raw(tok, ptr, B, strides, D, stats_shift=shift, clip_buf=clip_buf)
    if clip_buf is not None:
        assert int(cbuf[0]) == 0 and int(cbuf[-1]) == 0
    _same(base, out)


@pytest.mark.parametrize("vocab", [2, 256, 5000])
def test_vocab_sizes(vocab, gpu_device):
    """Below and above the 4,096-entry dequantise table of the reconstruct kernels."""
    tok, x64 = _setup(gpu_device, **K2, vocab=vocab)
    x = _batch(x64, 17)
    _check(tok, x, *_raw(tok, x.data_ptr(), 17, x.stride(), x.shape[2]))


def test_token_offset_and_nullable_outputs(gpu_device):
    tok, x64 = _setup(gpu_device, **K3)
    x = _batch(x64, 33)
    full = _raw(tok, x.data_ptr(), 33, x.stride(), x.shape[2])
    ref = _check(tok, x, *full)
    # the LLM offset as encode applies it
    llm = BEASTBsplineTokenizer(num_dof=14, gripper_zero_order=True, gripper_indices=[6, 13], device=str(gpu_device),
                                llm_vocab_size=256 + 31744)
    llm.load_state_dict({"w_min": tok.w_min.tolist(), "w_max": tok.w_max.tolist()})
    want, _ = llm.encode(x)
    off = _raw(tok, x.data_ptr(), 33, x.stride(), x.shape[2], offset=31744)
    assert torch.equal(off[1], want) and int(want.min()) >= 31744
    _same((full[0], full[2]), (off[0], off[2]))
    _check(tok, x, *off, offset=31744, ref=ref)
    for kw in (dict(tokens=False), dict(clip=False), dict(tokens=False, clip=False)):
        part = _raw(tok, x.data_ptr(), 33, x.stride(), x.shape[2], **kw)
        _same((full[0],), (part[0],))
        if part[1] is not None:
            _same((full[1],), (part[1],))
        if kw.get("clip", True):
            _same((full[2],), (part[2],))


def test_degenerate_bounds(gpu_device):
    """w_min == w_max on one column: the quantiser's scale clamp and a zero dequantise range."""
    dev = gpu_device
    src, x64 = _setup(dev, **K2)
    tok = BEASTBsplineTokenizer(num_dof=14, device=str(dev))
    lo, hi = src.w_min.clone(), src.w_max.clone()
    hi[23] = lo[23]
    tok.load_state_dict({"w_min": lo.tolist(), "w_max": hi.tolist()})
    x = _batch(x64, 17)
    for generic in (0, 1):
        try:
            _set_generic(generic)
            out = _raw(tok, x.data_ptr(), 17, x.stride(), x.shape[2])
        finally:
            _set_generic(0)
        _check(tok, x, *out)


@pytest.mark.parametrize("generic", [0, 1], ids=["specialised", "generic"])
def test_non_finite_samples(generic, gpu_device):
    """One NaN and one +inf sample reach all four statistics of their (b, d) and nothing else."""
    tok, x64 = _setup(gpu_device, **K3)
    clean = _batch(x64, 9)
    x = clean.clone()
    order = tok.joint_indices + tok.gripper_indices
    (bn, dn), (bi, di) = (2, 3), (5, 12)                       # a joint DoF, a gripper DoF
    x[bn, 7, order[dn]] = float("nan")
    x[bi, 11, order[di]] = float("inf")
    try:
        _set_generic(generic)
        stats, tokens, clip = _raw(tok, x.data_ptr(), 9, x.stride(), x.shape[2])
        base = _raw(tok, clean.data_ptr(), 9, clean.stride(), clean.shape[2])
    finally:
        _set_generic(0)
    _check(tok, x, stats, tokens, clip)
    assert bool(torch.isnan(stats[bn, dn]).all())
    assert not bool(torch.isfinite(stats[bi, di]).any())
    mask = torch.ones((9, 14), dtype=torch.bool, device=x.device)
    mask[bn, dn] = mask[bi, di] = False
    assert bool(torch.isfinite(stats[mask]).all())
    assert torch.equal(stats[mask], base[0][mask])             # the other DoFs do not notice


# -------------------------------------------------------------------------------- Python level --
def _golden_tok(cls, k, golden, dev, **kw):
    g = golden[k]
    tok = cls(**CONFIGS[k], device=str(dev), **kw)
    tok.load_state_dict({"w_min": g["w_min"].tolist(), "w_max": g["w_max"].tolist()})
    return tok, torch.from_numpy(g["x"]).to(dev)


def _composed(tok, x):
    tokens, pd = tok.encode(x)
    err = x - tok.reconstruct_traj(tokens)
    return tokens, pd["params"], err


@pytest.mark.parametrize("k", ["k1", "k2", "k3"])
@pytest.mark.parametrize("cls", [BEASTBsplineTokenizer, BEASTBsplineBPETokenizer], ids=["mp", "bpe"])
def test_reconstruction_stats_on_goldens(cls, k, golden, gpu_device):
    tok, x = _golden_tok(cls, k, golden, gpu_device)
    # the yardstick is always the plain tokenizer: the BPE class (untrained here) inherits the two
    # methods unchanged and returns the same MP tokens, while its own encode gives BPE ids
    plain, _ = _golden_tok(BEASTBsplineTokenizer, k, golden, gpu_device)
    D, N = tok.num_dof, tok.num_basis
    r = tok.reconstruction_stats(x, return_tokens=True)
    tokens, params, err = _composed(plain, x)
    l2, l1 = plain.compute_reconstruction_error(x)
    for got, want in ((r.l2, l2), (r.l1, l1)):
        assert abs(float(got) - float(want)) <= 1e-6 * max(1.0, abs(float(want)))
    # per output column (k3: the gripper columns 6 and 13 are DoFs 12 and 13 of the kernel)
    assert r.mse.shape == (x.shape[0], D) and r.mse.dtype == torch.float32
    assert torch.equal(r.max_abs, err.abs().amax(dim=1))
    torch.testing.assert_close(r.mse, (err * err).mean(dim=1), rtol=1e-5, atol=1e-12)
    torch.testing.assert_close(r.mean_err, err.mean(dim=1), rtol=1e-4, atol=1e-7)
    assert bool((r.mse_fit >= 0).all()) and float(r.mse_fit.mean()) <= float(r.mse.mean())
    assert torch.equal(r.tokens, tokens)
    assert r.clip_low.dtype == torch.int64 and r.clip_low.shape == (D, N)
    assert torch.equal(r.clip_low, (params < tok.w_min).sum(0).reshape(D, N))
    assert torch.equal(r.clip_high, (params > tok.w_max).sum(0).reshape(D, N))
    assert tok.reconstruction_stats(x).tokens is None
    # one [T, D] trajectory, float64 input, a strided view
    one = tok.reconstruction_stats(x[3].double())
    assert torch.equal(one.mse, r.mse[3:4]) and torch.equal(one.max_abs, r.max_abs[3:4])
    wide = torch.zeros((x.shape[0], x.shape[1], D + 3), device=x.device)
    wide[..., :D] = x
    assert torch.equal(tok.reconstruction_stats(wide).mse, r.mse)


def test_llm_offset_tokens(golden, gpu_device):
    tok, x = _golden_tok(BEASTBsplineTokenizer, "k3", golden, gpu_device, llm_vocab_size=32000)
    want, _ = tok.encode(x)
    assert torch.equal(tok.reconstruction_stats(x, return_tokens=True).tokens, want)
    mp, _ = tok.encode(x, respect_llm_vocab_size=False)
    r = tok.reconstruction_stats(x, return_tokens=True, respect_llm_vocab_size=False)
    assert torch.equal(r.tokens, mp) and torch.equal(want, mp + 32000 - 256)


def test_conditioned_tokenizer_takes_the_composed_path(golden, gpu_device):
    g = golden["k2"]
    tok = BEASTBsplineTokenizer(num_dof=14, init_cond_order=2, device=str(gpu_device))
    x = torch.from_numpy(g["x"]).to(gpu_device)
    lo, hi = torch.quantile(tok.compute_weights(x), torch.tensor([0.1, 0.9], device=x.device), dim=0)
    tok.load_state_dict({"w_min": lo.tolist(), "w_max": hi.tolist()})
    r = tok.reconstruction_stats(x, return_tokens=True)
    assert r.mse_fit is None
    tokens, params, err = _composed(tok, x)
    assert torch.equal(r.tokens, tokens)
    assert torch.equal(r.mse, (err * err).mean(dim=1)) and torch.equal(r.mean_err, err.mean(dim=1))
    assert torch.equal(r.max_abs, err.abs().amax(dim=1))
    assert torch.equal(r.clip_low, (params < tok.w_min).sum(0).reshape(14, -1)) and int(r.clip_low.sum()) > 0
    assert tok._cond_state["B"] == x.shape[0]                 # conditions stored as encode stores them
    ev = tok.evaluate_reconstruction([x[:40], x[40:]])
    assert ev["mse_fit"] is None and ev["num_samples"] == 64


def test_evaluate_reconstruction(golden, gpu_device):
    tok, x = _golden_tok(BEASTBsplineTokenizer, "k3", golden, gpu_device)
    batches = [x[:24], {"actions": x[24:48]}, x[48:61]]      # ragged last batch
    ev = tok.evaluate_reconstruction(batches)
    r = tok.reconstruction_stats(x[:61])
    assert ev["num_samples"] == 61
    assert torch.equal(ev["clip_low"], r.clip_low) and torch.equal(ev["clip_high"], r.clip_high)
    assert torch.equal(ev["clip_low_rate"], r.clip_low.double() / 61)
    for key, want in (("mse", r.mse), ("mean_err", r.mean_err), ("mse_fit", r.mse_fit)):
        assert ev[key].dtype == torch.float64 and ev[key].shape == (14,)
        torch.testing.assert_close(ev[key], want.double().sum(0) / 61, rtol=1e-12, atol=0)
    assert torch.equal(ev["max_abs"], r.max_abs.double().amax(0))
    # max_samples counts batches, as fit_parameters does
    two = tok.evaluate_reconstruction(batches, max_samples=2)
    assert two["num_samples"] == 48
    assert torch.equal(two["clip_high"], tok.reconstruction_stats(x[:48]).clip_high)
    with pytest.raises(KeyError):
        tok.evaluate_reconstruction([{"observations": x}])
