"""GPU parity of the HIP path against the reference goldens and the CPU oracle.

Contracts:
  * basis, quantiser, dequantiser, quantiles, BPE vocab/merges: bit-exact;
  * params: |gpu - ref| <= 1e-5 * max(1, |ref row|_inf) (the reference's own fp32
    LU error is ~2e-6 of that scale); vs the float64 oracle fit: within the fp32
    fma-chain bound (T + 8) * 2^-24 * sum_t |P[n,t] y[t]|;
  * tokens end-to-end: equal to the reference except where the exact fit's
    normalised value lies within TIE_TOL = 5e-4 of a .5 rounding tie (counted; observed
    at most 4.0e-4 over the 7e7 tokens of the K5 corpus, 2.0e-4 at B = 4,096);
  * positions: |gpu - ref| <= 1e-5 * max(1, |ref|_inf per trajectory).
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import CONFIGS, GOLDEN, load_json, load_npz

pytestmark = pytest.mark.gpu

from beast_tokenizer_amd import BEASTBsplineBPETokenizer, BEASTBsplineTokenizer, FIGBPE  # noqa: E402
from beast_tokenizer_amd.synthetic import synth_trajectories  # noqa: E402
from oracle import beast_oracle as O  # noqa: E402

sys.path.insert(0, GOLDEN)
from kat_inputs import quantile_inputs  # noqa: E402

TIE_TOL = 5e-4   # observed max 4.0e-4 (K5 census, tests/golden/k5_bpe.json), 2.0e-4 at K2/K3


def make_tok(name, g, dev, cls=BEASTBsplineTokenizer, **kw):
    tok = cls(device=str(dev), **CONFIGS[name], **kw)
    tok.load_state_dict({"w_min": g["w_min"].tolist(), "w_max": g["w_max"].tolist()})
    return tok


def phis(g):
    pj = g["phi_joint"]
    return pj, g.get("phi_grip", pj)


def check_token_flips(tok_gpu, tok_ref, x, g, name, max_flips):
    """Every token that differs from the reference must sit on a rounding tie of the exact fit."""
    lay = O.Layout.make(CONFIGS[name]["num_dof"], CONFIGS[name]["gripper_indices"],
                        CONFIGS[name]["gripper_zero_order"])
    pj, pg = phis(g)
    p_exact = O.fit_exact(x[..., lay.joint_indices], pj)
    if lay.gripper_indices:
        p_exact = np.concatenate([p_exact, O.fit_exact(x[..., lay.gripper_indices], pg)], axis=-1)
    units = O.normalized_units(p_exact, g["w_min"], g["w_max"], 256)
    B, N, D = x.shape[0], 10, lay.num_dof
    units = units.reshape(B, D, N).transpose(0, 2, 1).reshape(B, N * D)
    diff = tok_gpu != tok_ref
    nflip = int(diff.sum())
    assert nflip <= max_flips, f"{nflip} token flips vs reference"
    if nflip:
        frac = np.abs(units[diff] - np.floor(units[diff]) - 0.5)
        assert frac.max() < TIE_TOL, f"non-tie flip: distance to .5 = {frac.max()}"
        assert np.abs(tok_gpu[diff] - tok_ref[diff]).max() == 1
    return nflip


@pytest.mark.parametrize("name", list(CONFIGS))
def test_basis_bitexact(name, golden, gpu_device):
    g = golden[name]
    tok = make_tok(name, g, gpu_device)
    phi, proj, proj32 = tok._constants(gpu_device)
    assert np.array_equal(phi[0].cpu().numpy(), g["phi_joint"])
    assert np.array_equal(proj32.cpu().numpy(), proj.cpu().numpy().astype(np.float32))
    if "phi_grip" in g:
        assert np.array_equal(phi[1].cpu().numpy(), g["phi_grip"])
    P = O.projection_f64(g["phi_joint"])
    pp = proj[0].cpu().numpy()
    assert pp.shape == (16, 52) and not pp[10:].any() and not pp[:, 50:].any()
    assert np.allclose(pp[:10, :50], P, rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_encode_params_and_tokens(name, golden, gpu_device, kernel_mode):
    g = golden[name]
    tok = make_tok(name, g, gpu_device)
    x = g["x"]
    tokens, pd = tok.encode(torch.from_numpy(x))
    params = pd["params"].cpu().numpy()
    ref = g["params"]
    scale = np.maximum(1.0, np.abs(ref).max(axis=1, keepdims=True))
    assert np.all(np.abs(params - ref) <= 1e-5 * scale), np.abs(params - ref).max()
    # vs the float64 oracle: correctly rounded up to the f64 accumulation
    lay = O.Layout.make(CONFIGS[name]["num_dof"], CONFIGS[name]["gripper_indices"],
                        CONFIGS[name]["gripper_zero_order"])
    pj, pg = phis(g)
    ex = O.fit_exact(x[..., lay.joint_indices], pj)
    if lay.gripper_indices:
        ex = np.concatenate([ex, O.fit_exact(x[..., lay.gripper_indices], pg)], axis=-1)
    # fp32 MFMA fit (fp32 P, k-ordered fma chain over T): |err| <= (T + 8) * 2^-24 * sum_t |P y|
    S = []
    for idx, ph in ((lay.joint_indices, pj), (lay.gripper_indices, pg)):
        if idx:
            P = np.abs(O.projection_f64(ph))                               # [N, T]
            S.append(np.einsum('nt,btd->bdn', P, np.abs(x[..., idx].astype(np.float64))).reshape(len(x), -1))
    S = np.concatenate(S, axis=-1)
    assert np.all(np.abs(params - ex) <= (50 + 8) * 2.0 ** -24 * S + 1e-30)
    # quantiser given identical params: bit-exact
    t = tokens.cpu().numpy()
    want = O.continuous_to_discrete(O._clamp_t(params, g["w_min"], g["w_max"]), g["w_min"], g["w_max"], 256)
    B, D, N = params.shape[0], lay.num_dof, 10
    assert np.array_equal(t, want.reshape(B, D, N).transpose(0, 2, 1).reshape(B, N * D))
    assert tokens.dtype == torch.int64 and tokens.shape == (64, N * D)
    check_token_flips(t, g["tokens"], x, g, name, max_flips=3)
    for k in ("init_pos", "init_vel", "end_pos", "end_vel"):
        assert pd[k] is None


@pytest.mark.parametrize("name", list(CONFIGS))
def test_quantize_bitexact_on_reference_params(name, golden, gpu_device):
    g = golden[name]
    tok = make_tok(name, g, gpu_device)
    p = torch.from_numpy(g["params"]).to(gpu_device)
    out = tok._quantize(p, 0, gpu_device, mode=0).cpu().numpy()
    assert np.array_equal(out, g["tokens"])
    out = tok._quantize(p, 32000 - 256, gpu_device, mode=0).cpu().numpy()
    assert np.array_equal(out, g["tokens_llm"])


@pytest.mark.parametrize("V", [256, 1024, 4096])
def test_quantize_nonfinite_matches_reference(V, gpu_device):
    """k_quantize on NaN / +-inf params and degenerate / inverted / NaN / infinite bounds equals
    the reference's own tokens (tests/golden/nonfinite_tokens.npz: torch's NaN -> int64 cast)."""
    g = load_npz("nonfinite_tokens.npz")
    D, N = 4, 6   # 24 (d n) columns
    tok = BEASTBsplineTokenizer(num_dof=D, num_basis=N, seq_len=50, vocab_size=V, device=str(gpu_device))
    tok.load_state_dict({"w_min": g[f"v{V}_w_min"].tolist(), "w_max": g[f"v{V}_w_max"].tolist()})
    p = torch.from_numpy(g[f"v{V}_params"]).to(gpu_device)
    out = tok._quantize(p, 0, gpu_device, mode=0).cpu().numpy()
    want = g[f"v{V}_tokens"].reshape(-1, D, N).transpose(0, 2, 1).reshape(-1, N * D)
    assert np.array_equal(out, want)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_decode_bitexact(name, golden, gpu_device, kernel_mode):
    g = golden[name]
    tok = make_tok(name, g, gpu_device)
    dec = tok.decode(torch.from_numpy(g["tokens"])).cpu().numpy()
    assert np.array_equal(dec, g["decoded"])
    tok.set_llm_vocab_size(32000)
    dec2 = tok.decode(torch.from_numpy(g["tokens_llm"])).cpu().numpy()
    assert np.array_equal(dec2, g["decoded"])
    # [B, N, D] input form
    dec3 = tok.decode(torch.from_numpy(g["tokens_llm"]).reshape(64, 10, -1)).cpu().numpy()
    assert np.array_equal(dec3, g["decoded"])


def _close_pos(a, b):
    scale = np.maximum(1.0, np.abs(b).max(axis=(1, 2), keepdims=True))
    err = np.abs(a - b) / scale
    assert err.max() <= 1e-5, err.max()
    return float((a == b).mean())


@pytest.mark.parametrize("name", list(CONFIGS))
def test_reconstruct(name, golden, gpu_device, kernel_mode):
    g = golden[name]
    tok = make_tok(name, g, gpu_device)
    toks = torch.from_numpy(g["tokens"])
    pos = tok.reconstruct_traj(toks).cpu().numpy()
    assert pos.shape == g["pos"].shape and pos.dtype == np.float32
    _close_pos(pos, g["pos"])
    pos_ip = tok.reconstruct_traj(toks, init_p=torch.from_numpy(g["init_p"])).cpu().numpy()
    _close_pos(pos_ip, g["pos_init_p"])
    t80 = torch.from_numpy(g["times80"])
    pos80 = tok.reconstruct_traj(toks, times=t80.expand(64, 80)).cpu().numpy()
    _close_pos(pos80, g["pos_t80"])
    pos80b = tok.reconstruct_traj(toks, times=t80).cpu().numpy()
    assert np.array_equal(pos80, pos80b)


@pytest.mark.parametrize("name", ["k2", "k3"])
def test_reconstruct_per_row_times(name, golden, gpu_device):
    """Different time grid per trajectory -> per-row basis path; vs fp64 numpy."""
    g = golden[name]
    tok = make_tok(name, g, gpu_device)
    toks = torch.from_numpy(g["tokens"][:16])
    rng = np.random.default_rng(5)
    times = np.sort(rng.uniform(0, 2 * np.pi, size=(16, 33)), axis=1).astype(np.float32)
    pos = tok.reconstruct_traj(toks, times=torch.from_numpy(times)).cpu().numpy()
    lay = O.Layout.make(CONFIGS[name]["num_dof"], CONFIGS[name]["gripper_indices"],
                        CONFIGS[name]["gripper_zero_order"])
    params = O.decode(g["tokens"][:16], lay, 10, g["w_min"], g["w_max"], 256).reshape(16, lay.num_dof, 10)
    want = np.zeros_like(pos)
    for b in range(16):
        pj = O.basis(times[b], np.float32(2 * np.pi), 4, 10)
        pg = O.basis(times[b], np.float32(2 * np.pi), 0, 10)
        for i, d in enumerate(lay.order):
            ph = pj if i < len(lay.joint_indices) else pg
            want[b, :, d] = ph.astype(np.float64) @ params[b, i].astype(np.float64)
    _close_pos(pos, want)


@pytest.mark.parametrize("name", ["k2", "k3"])
def test_flip_census_4096(name, gpu_device, kernel_mode):
    """Full BASELINE size: tokens vs the reference's, every flip a rounding tie."""
    z = load_npz(f"tokens4096_{name}.npz")
    gi = CONFIGS[name]["gripper_indices"] or []
    x = synth_trajectories(4096, 50, 14, seed=0, gripper_indices=gi)
    assert hashlib.sha256(x.tobytes()).digest() == z["x_sha256"].tobytes(), "synthetic generator drifted"
    g = dict(load_npz(f"bspline_{name}.npz"))
    g["w_min"], g["w_max"] = z["w_min"], z["w_max"]
    tok = make_tok(name, g, gpu_device)
    tokens, _ = tok.encode(torch.from_numpy(x))
    # observed: 21 flips of 573,440 tokens at K2 (bench token census); about twice that is the bar
    n = check_token_flips(tokens.cpu().numpy(), z["tokens"].astype(np.int64), x, g, name, max_flips=45)
    print(f"{name}: {n} tie flips of {tokens.numel()} tokens")


@pytest.mark.parametrize("name", list(CONFIGS))
def test_specialised_kernels_equal_generic(name, gpu_device):
    """The shape-specialised encode / reconstruct kernels (both workgroup widths) compute
    exactly what the runtime-shape kernels compute (same operation order): bitwise-equal.  At
    1,000 trajectories the per-trajectory kernels run their latency variants; 16 per CU plus 11 is
    a bulk launch (8-wave encode tiles, write-back stores, a partial last tile)."""
    from conftest import set_kernel_mode
    gi = CONFIGS[name]["gripper_indices"] or []
    g = dict(load_npz(f"bspline_{name}.npz"))
    tok = make_tok(name, g, gpu_device)
    cus = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    for B in (1000, 16 * cus + 11):
        x = torch.from_numpy(synth_trajectories(B, 50, CONFIGS[name]["num_dof"], seed=3, gripper_indices=gi))
        outs = []
        for mode in ("generic", "specialised_w4", "specialised_w7", "specialised_w8", "specialised"):
            set_kernel_mode(mode)
            try:
                t, pd = tok.encode(x)
                pos = tok.reconstruct_traj(t)
                outs.append((t.cpu().numpy(), pd["params"].cpu().numpy(), pos.cpu().numpy()))
            finally:
                set_kernel_mode("specialised")
        for other in outs[1:]:
            for a, b in zip(outs[0], other):
                assert np.array_equal(a, b)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_host_fastpath_equals_python_path(name, gpu_device):
    """The C++ host fast path (csrc/fastpath.cpp) is built, in use, and returns exactly what
    the Python/ctypes path returns; inputs it does not take fall through to that path."""
    gi = CONFIGS[name]["gripper_indices"] or []
    g = dict(load_npz(f"bspline_{name}.npz"))
    tok = make_tok(name, g, gpu_device, llm_vocab_size=32000)
    p = tok._plan()
    assert p.fast is not None and p.fast_enc is not None, "fast path not built / not loaded"
    x = torch.from_numpy(synth_trajectories(777, 50, CONFIGS[name]["num_dof"], seed=4, gripper_indices=gi))
    xd = x.to(gpu_device)
    t1, d1 = tok.encode(xd)
    r1 = tok.reconstruct_traj(t1)
    saved = (p.fast, p.fast_enc, p.fast_rec)
    p.fast = p.fast_enc = p.fast_rec = None          # the Python / ctypes path
    try:
        t2, d2 = tok.encode(xd)
        r2 = tok.reconstruct_traj(t2)
    finally:
        p.fast, p.fast_enc, p.fast_rec = saved
    assert torch.equal(t1, t2) and torch.equal(d1["params"], d2["params"]) and torch.equal(r1, r2)
    assert list(d1) == list(d2) and all(d1[k] is None for k in d1 if k != "params")   # same dict as the reference
    # the fastcall entry points are ordered on a non-default current stream: the ordering probe of
    # tests/stream_order.py (stale input, a delay, poison-free fresh outputs, no host synchronisation)
    from stream_order import Case, assert_ordered
    xb = torch.empty_like(xd)

    def chain(_handle):
        t6, d6 = tok.encode(xb)
        return [t6, d6["params"], tok.reconstruct_traj(t6)]
    rep = assert_ordered(Case(f"fastpath[{name}]", ("fast_encode", "fast_reconstruct"),
                              [(xb, xd, xd.flip(0).contiguous())], chain), gpu_device, api=True)
    assert torch.equal(rep.snapshot[0], t1) and torch.equal(rep.snapshot[1], d1["params"])
    assert torch.equal(rep.snapshot[2], r1)
    # fall-through cases: host input, strided input, 3-D int32 tokens
    t3, _ = tok.encode(x)
    assert torch.equal(t3, t1)
    t4, _ = tok.encode(torch.cat([xd, xd], dim=2)[..., : xd.shape[2]])
    assert torch.equal(t4, t1)
    r5 = tok.reconstruct_traj(t1.reshape(777, 10, -1).to(torch.int32))
    assert torch.equal(r5, r1)


@pytest.mark.parametrize("vocab", [256, 1024, 4096])
def test_encode_quantiser_exact_near_ties(vocab, gpu_device, kernel_mode):
    """The encode kernel's in-lane quantiser (reciprocal fast path + exact fallback) must
    equal continuous_to_discrete on its own params bit for bit.  Trajectories are built
    as y = Phi w with w on or next to rounding ties (k + 0.5) of the bins, plus NaN /
    inf / degenerate-range / inverted-bound / NaN-bound columns."""
    rng = np.random.default_rng(vocab)
    B, T, D, N = 2048, 50, 7, 10
    tok = BEASTBsplineTokenizer(num_dof=D, num_basis=N, seq_len=T, vocab_size=vocab, device=str(gpu_device))
    lo = rng.uniform(-2, 0, size=D * N).astype(np.float32)
    hi = (lo + rng.uniform(0.5, 3, size=D * N)).astype(np.float32)
    hi[3] = lo[3]                                   # degenerate range: scale clamps to 1e-8
    hi[5] = lo[5] - 0.7                             # inverted bounds: every bin is 0
    hi[12] = np.nan                                 # NaN bound: clamp gives NaN
    tok.load_state_dict({"w_min": lo.tolist(), "w_max": hi.tolist()})
    # targets on ties: u * (vocab - 1) = k + 0.5 (+ a few ulps either way)
    k = rng.integers(0, vocab - 1, size=(B, D * N))
    u = (k + 0.5 + rng.choice([0, 1e-7, -1e-7, 3e-6, -3e-6], size=k.shape)) / (vocab - 1)
    w = (lo + u * (hi - lo)).astype(np.float64)                     # [B, (d n)]
    phi = O.basis(O.times_grid(2 * np.pi, T), np.float32(2 * np.pi), 4, N).astype(np.float64)   # [T, N]
    y = np.einsum("tn,bdn->btd", phi, w.reshape(B, D, N)).astype(np.float32)
    y[5, 7, 2] = np.nan                             # NaN params for DoF 2 of trajectory 5
    y[9, :, 4] = np.inf                             # inf / NaN params for DoF 4 of trajectory 9
    tokens, pd = tok.encode(torch.from_numpy(y))
    params = pd["params"].cpu().numpy()
    want = O.continuous_to_discrete(O._clamp_t(params, lo, hi), lo, hi, vocab)
    want = want.reshape(B, D, N).transpose(0, 2, 1).reshape(B, N * D)
    assert np.array_equal(tokens.cpu().numpy(), want)
    near = np.abs(O.normalized_units(params, lo, hi, vocab) % 1.0 - 0.5) < 1e-4
    assert near.sum() > B   # the fast path's fallback really was exercised


@pytest.mark.parametrize("name", ["k2", "k3"])
def test_roundtrip_properties(name, golden, gpu_device):
    """Size-independent properties at B=4096: decode(encode) within one bin, reconstruct(tokens) == Phi.decode."""
    g = golden[name]
    tok = make_tok(name, g, gpu_device)
    x = synth_trajectories(4096, 50, 14, seed=11, gripper_indices=CONFIGS[name]["gripper_indices"] or [])
    tokens, pd = tok.encode(torch.from_numpy(x).to(gpu_device))
    dec = tok.decode(tokens)
    clamped = torch.clamp(pd["params"], min=tok.w_min, max=tok.w_max)
    binw = (tok.w_max - tok.w_min) / 255
    slack = 4e-7 * torch.maximum(tok.w_min.abs(), tok.w_max.abs())   # three fp32 roundings in dequantise
    assert torch.all((dec - clamped).abs() <= 0.5 * binw * (1 + 1e-5) + slack + 1e-7)
    # idempotence: re-encoding the decoded params' quantisation gives the same tokens
    again = tok._quantize(dec, 0, gpu_device, 0)
    assert torch.equal(again, tokens)
    assert int(tokens.min()) >= 0 and int(tokens.max()) <= 255


@pytest.mark.parametrize("name", list(CONFIGS))
def test_update_bounds(name, golden, gpu_device):
    g = golden[name]
    tok = make_tok(name, g, gpu_device)
    x = torch.from_numpy(g["x"]) * 3.0
    wmin0, wmax0 = tok.w_min.clone(), tok.w_max.clone()
    tokens, pd = tok.encode(x, update_bounds=True)
    p = pd["params"].cpu().numpy()
    bmin, bmax = p.min(0), p.max(0)
    wmn, wmx = wmin0.cpu().numpy(), wmax0.cpu().numpy()
    exp_min = np.where(bmin < (wmn - np.float32(1e-4)), bmin, wmn)
    exp_max = np.where(bmax > (wmx + np.float32(1e-4)), bmax, wmx)
    assert np.array_equal(tok.w_min.cpu().numpy(), exp_min)
    assert np.array_equal(tok.w_max.cpu().numpy(), exp_max)
    want = O.continuous_to_discrete(O._clamp_t(p, exp_min, exp_max), exp_min, exp_max, 256)
    B, D = p.shape[0], CONFIGS[name]["num_dof"]
    assert np.array_equal(tokens.cpu().numpy(), want.reshape(B, D, 10).transpose(0, 2, 1).reshape(B, -1))


def _identity_reduce(t, op):
    """A one-rank stand-in for an all-reduce: column_quantiles then takes the multi-rank radix
    (11/7/7/7-bit digits, small histogram slices)."""
    return None


@pytest.mark.parametrize("reduce", [None, _identity_reduce], ids=["radix11", "radix7"])
def test_quantile_kat(gpu_device, reduce):
    from beast_tokenizer_amd.quantile import column_quantiles, no_reduce
    reduce = reduce or no_reduce
    z = load_npz("quantile_kat.npz")
    for k, x in quantile_inputs().items():
        q = column_quantiles(torch.from_numpy(x).to(gpu_device), [0.01, 0.99], reduce).cpu().numpy()
        assert np.array_equal(q[0], z[k + "_lo"].astype(np.float32)), k
        assert np.array_equal(q[1], z[k + "_hi"].astype(np.float32)), k
    # row blocks read in place (fit_parameters' per-batch params) == one matrix
    for k, x in quantile_inputs().items():
        if x.shape[0] < 10:
            continue
        cuts = [0, 3, x.shape[0] // 2, x.shape[0] // 2, x.shape[0]]
        blocks = [torch.from_numpy(x[a:b]).to(gpu_device) for a, b in zip(cuts[:-1], cuts[1:])]
        q = column_quantiles(blocks, [0.01, 0.99], reduce).cpu().numpy()
        assert np.array_equal(q[0], z[k + "_lo"].astype(np.float32)), k
        assert np.array_equal(q[1], z[k + "_hi"].astype(np.float32)), k
    xn = quantile_inputs()["n101"].copy()
    xn[7, 3] = np.nan
    q = column_quantiles(torch.from_numpy(xn).to(gpu_device), [0.01, 0.99], reduce).cpu().numpy()
    ref = np.quantile(xn, [0.01, 0.99], axis=0)
    assert np.array_equal(np.isnan(q), np.isnan(ref)) and np.isnan(q[:, 3]).all()
    assert np.array_equal(q[~np.isnan(q)], ref[~np.isnan(ref)].astype(np.float32))


@pytest.mark.parametrize("name", list(CONFIGS))
def test_fit_parameters(name, golden, gpu_device):
    g = golden[name]
    tok = make_tok(name, g, gpu_device)
    gi = CONFIGS[name]["gripper_indices"] or []
    D = CONFIGS[name]["num_dof"]
    loader = [{"actions": torch.from_numpy(synth_trajectories(1024, 50, D, seed=1, gripper_indices=gi,
                                                              start=1024 * i))} for i in range(8)]
    tok.fit_parameters(loader, verbose=False)
    allp = torch.cat([tok.compute_weights(b["actions"]) for b in loader]).cpu().numpy()
    lo, hi = O.quantile_bounds(allp)
    assert np.array_equal(tok.w_min.cpu().numpy(), lo)
    assert np.array_equal(tok.w_max.cpu().numpy(), hi)
    bounds = load_json(f"bounds_{name}.json")
    assert np.allclose(tok.w_min.cpu().numpy(), bounds["w_min"], rtol=1e-4, atol=1e-4)
    assert np.allclose(tok.w_max.cpu().numpy(), bounds["w_max"], rtol=1e-4, atol=1e-4)
    with pytest.raises(KeyError):
        tok.fit_parameters([{"obs": 1}], verbose=False)
    with pytest.raises(RuntimeError):
        tok.fit_parameters([], verbose=False)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_fit_parameters_grouped_launch(name, golden, gpu_device):
    """Device-resident batches are fitted in groups by beast_encode_list_f32: params bitwise
    those of per-batch compute_weights, bounds those of the oracle's quantiles; batches that
    cannot join a group (host tensors, B % 8 != 0, another shape) interleave correctly."""
    g = golden[name]
    tok = make_tok(name, g, gpu_device)
    gi = CONFIGS[name]["gripper_indices"] or []
    D = CONFIGS[name]["num_dof"]
    xs = [torch.from_numpy(synth_trajectories(n, 50, D, seed=3, gripper_indices=gi, start=4096 * i))
          for i, n in enumerate([1024, 1024, 1024, 512, 1020, 1024, 1024, 1024, 1024, 8])]
    loader = [{"actions": x.to(gpu_device)} for x in xs]
    loader[5]["actions"] = xs[5]                     # a host batch in the middle of a group
    tok._FIT_GROUP_ROWS = 2048                        # several groups, and a group of one
    ptrs = [x.data_ptr() for x in (b["actions"] for b in loader)]
    listable = (50 * D) % 4 == 0                       # whole 16-byte rows (not D = 7)
    assert tok._listable(loader[0]["actions"], []) == listable and not tok._listable(loader[4]["actions"], [])
    if listable:
        grouped = tok._fit_list([b["actions"] for b in loader[6:9]])
        single = torch.cat([tok.compute_weights(b["actions"]) for b in loader[6:9]])
        assert torch.equal(grouped, single)
    tok.fit_parameters(loader, verbose=False)
    assert ptrs == [b["actions"].data_ptr() for b in loader]
    allp = torch.cat([tok.compute_weights(b["actions"]) for b in loader]).cpu().numpy()
    lo, hi = O.quantile_bounds(allp)
    assert np.array_equal(tok.w_min.cpu().numpy(), lo)
    assert np.array_equal(tok.w_max.cpu().numpy(), hi)
    tok.fit_parameters(loader, max_samples=3, verbose=False)   # stops mid-group
    lo3, hi3 = O.quantile_bounds(allp[:3072])
    assert np.array_equal(tok.w_min.cpu().numpy(), lo3) and np.array_equal(tok.w_max.cpu().numpy(), hi3)


def test_encode_continuous_and_back(golden, gpu_device):
    g = golden["k3"]
    tok = make_tok("k3", g, gpu_device)
    ct, pd = tok.encode_continuous(torch.from_numpy(g["x"]))
    p = pd["params"].cpu().numpy()
    wmn, wmx = g["w_min"], g["w_max"]
    c = O._clamp_t(p, wmn, wmx)
    want = (((c - wmn) / np.maximum(wmx - wmn, np.float32(1e-8))).astype(np.float32) * np.float32(2)
            + np.float32(-1)).astype(np.float32)
    B = p.shape[0]
    assert np.array_equal(ct.cpu().numpy(), want.reshape(B, 14, 10).transpose(0, 2, 1).reshape(B, -1))
    pos = tok.reconstruct_traj_continuous(ct).cpu().numpy()
    # expected: denormalise (evident intent of beast/utils.py:38-44) then Phi . W in float64
    c = np.clip(ct.cpu().numpy(), -1, 1).reshape(B, 10, 14).transpose(0, 2, 1).reshape(B, -1)
    w = (((c + np.float32(1)) / np.float32(2)).astype(np.float32) * (wmx - wmn) + wmn).astype(np.float32)
    lay = O.Layout.make(14, [6, 13], True)
    pj, pg = phis(g)
    want = np.zeros_like(pos)
    for i, d in enumerate(lay.order):
        ph = pj if i < len(lay.joint_indices) else pg
        want[:, :, d] = w.reshape(B, 14, 10)[:, i].astype(np.float64) @ ph.T.astype(np.float64)
    _close_pos(pos, want)


# ------------------------------------------------------------------ BPE ----
BPE_CASES = sorted(load_json("bpe_hf.json").keys()) if os.path.exists(os.path.join(GOLDEN, "bpe_hf.json")) else []


@pytest.fixture(scope="module")
def bpe_golden():
    return load_json("bpe_hf.json"), load_npz("bpe_corpora.npz")


@pytest.mark.parametrize("case", BPE_CASES)
def test_bpe_train_matches_hf(case, bpe_golden, gpu_device):
    ref, corpora = bpe_golden
    cname, vs = case.split("/")
    arr = corpora[cname]
    fig = FIGBPE(vocab_size=int(vs), show_progress=False, device=gpu_device)
    st = fig.fit_from_sequences(list(arr))
    r = ref[case]
    assert st.min_token == r["min_token"] and st.max_token == r["max_token"]
    res = fig.last_result
    assert res.vocab == r["vocab"]
    assert [list(m) for m in res.merges] == r["merges"]
    # the wrapped HF object behaves like the HF-trained one
    text = "".join(map(chr, (arr[0] - r["min_token"]).astype(int)))
    ids = st.tokenizer.encode(text, add_special_tokens=False).ids
    assert st.tokenizer.decode(ids) == text


@pytest.mark.parametrize("case", ["skew/2048", "rand256/700", "traj_k3/2048"])
def test_bpe_host_loop_and_compaction_match_hf(case, bpe_golden, gpu_device):
    """The host-driven loop (one merge per call: the fallback for vocabularies above 4,096 and on a
    string-hash collision), with and without periodic compaction of the words that cannot merge
    any more, gives HF's merges."""
    from beast_tokenizer_amd.bpe_train import fixed_rows_to_device, train_bpe
    ref, corpora = bpe_golden
    cname, vs = case.split("/")
    flat, off = fixed_rows_to_device(torch.from_numpy(corpora[cname].astype(np.int64)).to(gpu_device))
    for compact in (0, 3):
        res = train_bpe(flat, off, int(vs), device_loop=False, compact_every=compact)
        assert res.stats["loop"] == "host"
        assert res.vocab == ref[case]["vocab"]
        assert [list(m) for m in res.merges] == ref[case]["merges"]


@pytest.mark.parametrize("lds_min", [0, 1 << 30])
@pytest.mark.parametrize("case", ["skew/2048", "traj_k3/2048"])
def test_bpe_delta_paths_match_hf(case, lds_min, bpe_golden, gpu_device):
    """The merge kernels' pair-count changes summed in LDS first for every merge (threshold 0) and
    by global atomics for every merge (threshold 2^30) both give HF's merges (default: LDS from
    4,096), in the batched device loop and the host-driven loop."""
    from beast_tokenizer_amd import _lib
    from beast_tokenizer_amd.bpe_train import fixed_rows_to_device, train_bpe
    ref, corpora = bpe_golden
    cname, vs = case.split("/")
    flat, off = fixed_rows_to_device(torch.from_numpy(corpora[cname].astype(np.int64)).to(gpu_device))
    lib = _lib.load()
    assert lib.beast_set_option(_lib.OPT_MERGE_LDS_MIN, lds_min) == 0
    try:
        res = train_bpe(flat, off, int(vs))
        res2 = train_bpe(flat, off, int(vs), device_loop=False)
    finally:
        lib.beast_set_option(_lib.OPT_MERGE_LDS_MIN, 4096)
    for r in (res, res2):
        assert r.vocab == ref[case]["vocab"]
        assert [list(m) for m in r.merges] == ref[case]["merges"]


def test_bpe_pretok_words_match_hf(gpu_device):
    from beast_tokenizer_amd.bpe_train import GpuBpeOps, build_alphabet, sequences_to_device
    from beast_tokenizer_amd.pretok import bytes_to_unicode, class_lut
    samples = [s for s, _ in load_json("pretok.json")["samples"] if s]
    pieces = [p for _, ps in load_json("pretok.json")["samples"] for p in ps]
    seqs = [np.array([ord(c) for c in s], dtype=np.int64) for s in samples]
    tokens, off = sequences_to_device(seqs, gpu_device)
    K = int(tokens.max())
    present = np.zeros(K + 1, dtype=bool)
    present[np.concatenate(seqs)] = True
    id2str, _, byte2id = build_alphabet(present, [chr(i) for i in range(K + 1)], [])
    ops = GpuBpeOps(gpu_device)
    w = ops.pretokenize(tokens, off, 0, class_lut(K + 1), byte2id)
    sym = w["sym"].cpu().numpy().view(np.uint16)
    ws, wl = w["wstart"].cpu().numpy(), w["wlen"].cpu().numpy()
    got = ["".join(id2str[s] for s in sym[a:a + n]) for a, n in zip(ws[: w["n_words"]], wl[: w["n_words"]])]
    assert got == pieces


def test_bpe_pretok_ragged_rows_match_oracle(gpu_device):
    """Wave-per-sequence pre-tokeniser on ragged rows: empty, one code point, rows at and past
    the LDS row bound (512: lane 0 falls back to the serial walk), contractions, blank runs,
    2-byte code points -- words and byte symbols equal the regex oracle's (bpe_oracle.pretokenize)."""
    from beast_tokenizer_amd.bpe_train import GpuBpeOps, build_alphabet
    from beast_tokenizer_amd.pretok import class_lut
    from cpu_ops import NumpyBpeOps
    rng = np.random.default_rng(5)
    # letters, digits, blanks, apostrophe + contraction letters, punctuation, Latin-1 letters
    alphabet = np.array([ord(c) for c in "ab z09 '  \t\nstrevmld!?,."] + [0xA0, 0xC4, 0xE9, 0xB5, 0xD7, 0x85])
    lens = [0, 1, 2, 3, 63, 64, 65, 140, 511, 512, 513, 777, 140, 0, 2000] + list(rng.integers(0, 300, 40))
    seqs = [alphabet[rng.integers(0, alphabet.size, n)].astype(np.int64) + 7 for n in lens]
    tokens = torch.from_numpy(np.concatenate(seqs)).to(gpu_device)
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).to(gpu_device)
    K = int(alphabet.max()) + 1
    present = np.zeros(K, dtype=bool)
    present[alphabet] = True
    _, _, byte2id = build_alphabet(present, [chr(i) for i in range(K)], [])
    w = GpuBpeOps(gpu_device).pretokenize(tokens, off, 7, class_lut(K), byte2id)
    sym = w["sym"].cpu().numpy().view(np.uint16)
    ws, wl = w["wstart"].cpu().numpy(), w["wlen"].cpu().numpy()
    got = [sym[a:a + n].tolist() for a, n in zip(ws[: w["n_words"]], wl[: w["n_words"]])]
    want = NumpyBpeOps().pretokenize(tokens.cpu(), off.cpu(), 7, class_lut(K), byte2id)
    assert w["n_syms"] == want["n_syms"]
    assert got == want["words"]
    # the words tile the symbol array in order
    assert ws[0] == 0 and np.all(ws[1: w["n_words"]] == (ws + wl)[: w["n_words"] - 1])


def test_bpe_dedup_table_overflow_retries(gpu_device):
    """Round 4 sizes the dedup table for a quarter of the word occurrences.  A corpus whose words
    are nearly all distinct overflows it: the kernel flags it (*out_n = -1) and GpuBpeOps.dedup
    retries with a 4x table -- the distinct words x counts stay a Counter's."""
    from collections import Counter
    from beast_tokenizer_amd.bpe_train import GpuBpeOps, build_alphabet, fixed_rows_to_device
    from beast_tokenizer_amd.pretok import class_lut
    rng = np.random.default_rng(12)
    # rows of distinct 3-letter words separated by a space: almost every occurrence is new
    letters = np.r_[65:91, 97:123]
    R, W = 4000, 12
    arr = np.full((R, W * 4), 32, dtype=np.int64)
    for k in range(3):
        arr[:, k::4] = letters[rng.integers(0, len(letters), size=(R, W))]
    flat, off = fixed_rows_to_device(torch.from_numpy(arr).to(gpu_device))
    present = np.zeros(128, dtype=bool)
    present[np.unique(arr)] = True
    _, _, byte2id = build_alphabet(present, [chr(i) for i in range(128)], [])
    ops = GpuBpeOps(gpu_device)
    w = ops.pretokenize(flat, off, 0, class_lut(128), byte2id)

    def words_of(d):
        sym = d["sym"].cpu().numpy().view(np.uint16)
        ws, wl = d["wstart"].cpu().numpy(), d["wlen"].cpu().numpy()
        return [tuple(sym[a:a + n]) for a, n in zip(ws[: d["n_words"]], wl[: d["n_words"]])]
    want = Counter(x for x in words_of(w) if len(x) >= 2)
    assert len(want) > w["n_words"] // 4          # more distinct words than the first table holds
    u = ops.dedup(w)
    got = dict(zip(words_of(u), u["wcount"].cpu().numpy()[: u["n_words"]].tolist()))
    assert got == dict(want)
    # the C-ABI's never-full size (include/beast_hip.h): one call, *out_n the distinct count
    from beast_tokenizer_amd import _lib
    lib, n = _lib.load(), w["n_words"]
    small, safe = lib.beast_bpe_dedup_workspace_bytes(n), lib.beast_bpe_dedup_workspace_bytes_safe(n)
    assert safe > small
    outs = [torch.empty(n, dtype=torch.int32, device=gpu_device) for _ in range(3)]
    on = torch.empty(1, dtype=torch.int64, device=gpu_device)
    for nbytes, ok in ((small, False), (safe, True)):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=gpu_device)
        _lib.run("beast_bpe_dedup_words", w["sym"].data_ptr(), w["wstart"].data_ptr(), w["wlen"].data_ptr(), n,
                 ws.data_ptr(), ws.numel(), *[o.data_ptr() for o in outs], on.data_ptr(), ops.stream)
        torch.cuda.synchronize()
        assert (int(on.item()) == len(want)) == ok and (int(on.item()) == -1) == (not ok)


def test_bpe_dedup_and_compact_match_counter(gpu_device):
    """Distinct words x counts equal a Counter over the pre-tokenised words (>= 2 symbols);
    compaction keeps exactly the words that can still merge."""
    from collections import Counter
    from beast_tokenizer_amd.bpe_train import GpuBpeOps, build_alphabet, fixed_rows_to_device
    from beast_tokenizer_amd.pretok import class_lut
    rng = np.random.default_rng(11)
    base = rng.integers(0, 300, size=9)
    arr = base[rng.integers(0, 9, size=(3000, 40))]
    arr[::7] = rng.integers(0, 300, size=(arr[::7].shape[0], 40))
    flat, off = fixed_rows_to_device(torch.from_numpy(arr.astype(np.int64)).to(gpu_device))
    present = np.zeros(300, dtype=bool)
    present[np.unique(arr)] = True
    _, _, byte2id = build_alphabet(present, [chr(i) for i in range(300)], [])
    ops = GpuBpeOps(gpu_device)
    w = ops.pretokenize(flat, off, 0, class_lut(300), byte2id)

    def words_of(d):
        sym = d["sym"].cpu().numpy().view(np.uint16)
        ws, wl = d["wstart"].cpu().numpy(), d["wlen"].cpu().numpy()
        return [tuple(sym[a:a + n]) for a, n in zip(ws[: d["n_words"]], wl[: d["n_words"]])]
    want = Counter(x for x in words_of(w) if len(x) >= 2)
    u = ops.dedup(w)
    got = dict(zip(words_of(u), u["wcount"].cpu().numpy()[: u["n_words"]].tolist()))
    assert len(got) == u["n_words"] == len(want)
    assert got == dict(want)
    lens = u["wlen"].cpu().numpy()[: u["n_words"]]
    assert np.all(np.diff(np.minimum(lens, 255)) >= 0)                     # length-ordered
    ws = u["wstart"].cpu().numpy()[: u["n_words"]]
    assert np.array_equal(ws[1:], ws[:-1] + (lens[:-1] + 3) // 4 * 4)       # contiguous 4-symbol-aligned spans
    assert u["n_syms_distinct"] == int(lens.sum()) and u["n_syms_padded"] == int(((lens + 3) // 4 * 4).sum())
    # shorten some words to length 1 / 0 and compact
    wl = u["wlen"].clone()
    wl[::3] = 1
    wl[1::5] = 0
    u2 = dict(u, wlen=wl)
    c = ops.compact(u2)
    keep = [(a, n, k) for a, n, k in zip(u["wstart"].cpu().tolist(), wl.cpu().tolist(), u["wcount"].cpu().tolist())
            if n >= 2]
    got_c = sorted(zip(c["wstart"].cpu().tolist()[: c["n_words"]], c["wlen"].cpu().tolist()[: c["n_words"]],
                       c["wcount"].cpu().tolist()[: c["n_words"]]))
    assert got_c == sorted(keep)


@pytest.mark.parametrize("mode", ["plain", "tag3", "overflow", "mixed_utf8", "long_rows"])
def test_bpe_pretok_dedup_equals_two_pass(gpu_device, mode):
    """The one-pass setup (k_pretok_dedup + the table compaction + repack from code points) gives
    exactly the two-pass pipeline's distinct words x counts, in the same layout (length order,
    4-symbol spans), and the same word / symbol totals: with forced 3-bit hash tags (every tag
    collides; the code-point compare keeps words apart), with a table too small for the words (the
    retry), over code points of 1-3 UTF-8 bytes, and over ragged rows of which some take the
    512-code-point kernel (257..512 code points)."""
    from collections import Counter
    from beast_tokenizer_amd import _lib
    from beast_tokenizer_amd.bpe_train import GpuBpeOps, build_alphabet, fixed_rows_to_device, sequences_to_device
    from beast_tokenizer_amd.pretok import class_lut
    rng = np.random.default_rng(23)
    hi = 3000 if mode == "mixed_utf8" else 300
    base = rng.integers(0, hi, size=9)
    arr = base[rng.integers(0, 9, size=(4000, 60))]
    arr[::7] = rng.integers(0, hi, size=(arr[::7].shape[0], 60))
    arr[::11, ::5] = 32   # spaces: more, shorter words
    if mode == "long_rows":
        seqs = [base[rng.integers(0, 9, size=n)] for n in rng.choice([40, 256, 257, 300, 512], size=900)]
        for q in seqs[::5]:
            q[::6] = 32
        arr = np.concatenate(seqs)
        flat, off = sequences_to_device([q.astype(np.int64) + 17 for q in seqs], gpu_device)
    else:
        flat, off = fixed_rows_to_device(torch.from_numpy(arr.astype(np.int64) + 17).to(gpu_device))
    present = np.zeros(hi, dtype=bool)
    present[np.unique(arr)] = True
    _, _, byte2id = build_alphabet(present, [chr(i) for i in range(hi)], [])
    ops = GpuBpeOps(gpu_device)
    lut = class_lut(hi)

    def counted(d):
        sym = d["sym"].cpu().numpy().view(np.uint16)
        ws, wl = d["wstart"].cpu().numpy(), d["wlen"].cpu().numpy()
        wc = d["wcount"].cpu().numpy()
        return {tuple(sym[a:a + n]): int(c) for a, n, c in zip(ws[: d["n_words"]], wl[: d["n_words"]],
                                                                wc[: d["n_words"]])}
    w = ops.pretokenize(flat, off, 17, lut, byte2id)
    want = counted(ops.dedup(w))
    lib = _lib.load()
    saved = lib.beast_bpe_pretok_dedup_workspace_bytes
    try:
        if mode == "tag3":
            lib.beast_set_option(_lib.OPT_BPE_DEDUP_KEY_BITS, 3)
        if mode == "overflow":   # 2,048 slots for thousands of distinct words: the kernel flags it, ops retries
            ops_lib = _lib.load()
            ops_lib.beast_bpe_pretok_dedup_workspace_bytes = lambda n: saved(5 * 2048)   # a 2,048-slot table
        res = ops.pretok_dedup(flat, off, 17, lut, byte2id)
    finally:
        lib.beast_set_option(_lib.OPT_BPE_DEDUP_KEY_BITS, 64)
        lib.beast_bpe_pretok_dedup_workspace_bytes = saved
    assert res is not None
    u, nw, ns = res
    assert (nw, ns) == (w["n_words"], w["n_syms"])
    if mode == "overflow":
        assert u["n_words"] > 2048 * 0.5
    got = counted(u)
    assert len(got) == u["n_words"] == len(want) and got == want
    lens = u["wlen"].cpu().numpy()[: u["n_words"]]
    assert np.all(np.diff(np.minimum(lens, 255)) >= 0)
    ws = u["wstart"].cpu().numpy()[: u["n_words"]]
    assert np.array_equal(ws[1:], ws[:-1] + (lens[:-1] + 3) // 4 * 4)
    assert u["n_syms_distinct"] == int(lens.sum()) and u["n_syms_padded"] == int(((lens + 3) // 4 * 4).sum())


def test_bpe_pretok_dedup_declines_long_rows(gpu_device):
    """A row over 512 code points is not the one-pass kernel's: it reports it and train_bpe runs the
    two-pass pipeline (HF's merges either way, tests/golden ragged corpora)."""
    from beast_tokenizer_amd.bpe_train import GpuBpeOps, build_alphabet, sequences_to_device
    from beast_tokenizer_amd.pretok import class_lut
    rng = np.random.default_rng(3)
    seqs = [rng.integers(0, 200, size=n) for n in (40, 700, 90)]
    flat, off = sequences_to_device(seqs, gpu_device)
    present = np.zeros(200, dtype=bool)
    present[np.unique(np.concatenate(seqs))] = True
    _, _, byte2id = build_alphabet(present, [chr(i) for i in range(200)], [])
    assert GpuBpeOps(gpu_device).pretok_dedup(flat, off, 0, class_lut(200), byte2id) is None


def test_bpe_tokenizer_end_to_end(gpu_device):
    g = load_npz("bspline_k2.npz")
    tok = make_tok("k2", g, gpu_device, cls=BEASTBsplineBPETokenizer, bpe_vocab_size=512)
    batches = [{"actions": torch.from_numpy(synth_trajectories(512, 50, 14, seed=4, start=512 * i))}
               for i in range(4)]
    st = tok.fit_from_trajectories(batches, show_progress=False, max_sequences=1800)
    assert tok.bpe_tokenizer is not None and st.max_token <= 255
    x = torch.from_numpy(synth_trajectories(32, 50, 14, seed=9))
    bpe_ids, params, mp = tok.encode(x, return_mp_tokens=True)
    # bins >= 128 are 2 UTF-8 bytes, so a row is at most 2*140 BPE ids
    assert len(bpe_ids) == 32 and all(len(r) <= 280 for r in bpe_ids)
    back = tok.bpe_to_mp_tokens(bpe_ids)
    assert torch.equal(back.cpu(), mp.cpu())
    assert torch.equal(tok.decode(bpe_ids), BEASTBsplineTokenizer.decode(tok, mp))
    # the tensor form: same ids, padded with PAD_ID, decodes as given (pads skipped, as HF skips them)
    from beast_tokenizer_amd import BpeIds
    from beast_tokenizer_amd.bpe_codec import PAD_ID
    blk, params2 = tok.encode(x, return_tensors=True)
    assert isinstance(blk, BpeIds) and blk.ids.device.type == "cuda" and params2.keys() == params.keys()
    assert blk.to_lists() == bpe_ids
    assert blk.lengths.tolist() == [len(r) for r in bpe_ids]
    assert int(blk.ids.shape[1]) == max(len(r) for r in bpe_ids)
    assert bool((blk.ids[torch.arange(blk.ids.shape[1], device=blk.ids.device)[None, :] >= blk.lengths[:, None]]
                 == PAD_ID).all())
    assert torch.equal(tok.bpe_to_mp_tokens(blk).cpu(), mp.cpu())
    assert torch.equal(tok.bpe_to_mp_tokens(blk.ids).cpu(), mp.cpu())
    assert torch.equal(tok.decode(blk), BEASTBsplineTokenizer.decode(tok, mp))
    assert tok._require_bpe().decode([blk.ids[0, 0].item(), PAD_ID], skip_special_tokens=True) == \
        tok._require_bpe().decode([blk.ids[0, 0].item()], skip_special_tokens=True)   # HF skips the pad id too
    with pytest.raises(ValueError):   # out-of-range bins: the same error as the list form
        tok._discrete_to_bpe(torch.full((2, 140), -5, dtype=torch.int64, device=gpu_device), as_tensors=True)
    # HF-trained reference on the same bins gives the same merges
    from tokenizers import ByteLevelBPETokenizer
    from tokenizers.trainers import BpeTrainer
    rows = torch.cat([tok.encode_to_mp_tokens(b["actions"])[0] for b in batches])[:1800].cpu().numpy()
    lo, hi = int(rows.min()), int(rows.max())
    bpe = ByteLevelBPETokenizer()
    tr = BpeTrainer(vocab_size=512, min_frequency=2, show_progress=False, special_tokens=[],
                    initial_alphabet=[chr(i) for i in range(hi - lo + 1)], max_token_length=10000)
    bpe._tokenizer.train_from_iterator(["".join(map(chr, r - lo)) for r in rows], trainer=tr)
    model = json.loads(bpe._tokenizer.to_str())["model"]
    assert tok._last_bpe_result.vocab == model["vocab"]
    assert [list(m) for m in tok._last_bpe_result.merges] == model["merges"]


# -------------------------------------------- init / end conditions (§8f rank 4) ----
COND = load_npz("conditions.npz")
COND_CASES = sorted({k.rsplit("_", 1)[0] for k in COND if k.endswith("_params")})


@pytest.mark.parametrize("case", COND_CASES)
def test_conditions_match_reference(case, gpu_device):
    """init_cond_order / end_cond_order != 0: params within 1e-5 of the reference, its
    conditions, tokens up to rounding ties, and reconstruct (which reuses the last fit's
    conditions, as the reference's MP object does) within 1e-5 -- default and custom times."""
    name, ic, ec = case.split("_")
    ic, ec = int(ic), int(ec)
    nd, g = (7, []) if name == "k1" else (14, [6, 13])
    x = torch.from_numpy(synth_trajectories(32, 50, nd, seed=5, gripper_indices=g)).to(gpu_device)
    tok = BEASTBsplineTokenizer(num_dof=nd, gripper_zero_order=bool(g), gripper_indices=g or None,
                                init_cond_order=ic, end_cond_order=ec, device=str(gpu_device))
    tok.w_min.copy_(torch.from_numpy(COND[case + "_w_min"]))
    tok.w_max.copy_(torch.from_numpy(COND[case + "_w_max"]))
    with pytest.raises(RuntimeError):
        tok.reconstruct_traj(torch.from_numpy(COND[case + "_tokens"]))   # no fit yet: no conditions
    tokens, pd = tok.encode(x)
    ref = COND[case + "_params"]
    got = pd["params"].cpu().numpy()
    scale = np.maximum(1.0, np.abs(ref).max(axis=1, keepdims=True))
    assert np.all(np.abs(got - ref) <= 1e-5 * scale)
    for c in ("init_pos", "init_vel", "end_pos", "end_vel"):
        if case + "_" + c in COND:
            np.testing.assert_allclose(pd[c].cpu().numpy(), COND[case + "_" + c], rtol=1e-6, atol=1e-6)
        else:
            assert pd[c] is None
    rt = COND[case + "_tokens"]
    diff = tokens.cpu().numpy() - rt
    assert np.abs(diff).max() <= 1 and (diff != 0).sum() <= 3          # rounding ties only
    pos = tok.reconstruct_traj(torch.from_numpy(rt).to(gpu_device)).cpu().numpy()
    rp = COND[case + "_pos"]
    assert np.abs(pos - rp).max() <= 1e-5 * max(1.0, np.abs(rp).max())
    t30 = torch.linspace(0, 2 * torch.pi, 30).to(gpu_device).repeat(32, 1)
    pos30 = tok.reconstruct_traj(torch.from_numpy(rt).to(gpu_device), times=t30).cpu().numpy()
    rp30 = COND[case + "_pos_t30"]
    assert np.abs(pos30 - rp30).max() <= 1e-5 * max(1.0, np.abs(rp30).max())
    with pytest.raises(RuntimeError):
        tok.reconstruct_traj(torch.from_numpy(rt[:5]).to(gpu_device))    # conditions fitted on 32 rows


@pytest.mark.parametrize("ic,ec", [(1, 0), (2, 0), (0, 1), (0, 2), (0, -1), (1, 1), (2, 2), (2, -1), (1, -1)])
def test_condition_kernels_match_torch_restatement(ic, ec, gpu_device):
    """csrc/cond.hip (k_cond_fixed, k_cond_add) against bspline.DeviceBasis.fixed_ctrl /
    fixed_term -- the reference's ATen op sequence in fp32 (uni_bspline_basis.py:192-301,
    uni_bspline.py:126-166): every condition output and the reconstruct term, shared and
    per-row time grids, gripper DoFs left untouched."""
    from beast_tokenizer_amd import _lib
    g = [6, 13]
    x = torch.from_numpy(synth_trajectories(32, 50, 14, seed=7, gripper_indices=g)).to(gpu_device)
    tok = BEASTBsplineTokenizer(num_dof=14, gripper_zero_order=True, gripper_indices=g, init_cond_order=ic,
                                end_cond_order=ec, device=str(gpu_device))
    tok.encode(x)
    st, b = tok._cond_state, tok._basis
    t = tok.times.to(gpu_device, torch.float32).reshape(-1)
    want = b.fixed_ctrl(x[..., tok.joint_indices], t[1] - t[0])
    names = ("init_pos", "init_vel", "end_pos", "end_vel", "params_init", "params_end")
    for name, w in zip(names, want):
        if w is None:
            assert st[name] is None, name
        else:
            np.testing.assert_allclose(st[name].cpu().numpy(), w.cpu().numpy(), rtol=1e-6, atol=1e-7, err_msg=name)
    jidx = torch.tensor(tok.joint_indices, dtype=torch.int32, device=gpu_device)
    for times in (t, torch.linspace(0, 1, 30, device=gpu_device).repeat(32, 1) * torch.rand(32, 1, device=gpu_device)):
        full = b.full_basis_at(times).contiguous()
        T = full.shape[-2]
        pos = torch.zeros((32, T, 14), dtype=torch.float32, device=gpu_device)
        _lib.run("beast_cond_add_f32", pos.data_ptr(), 32, T, 14, jidx.data_ptr(), jidx.numel(), full.data_ptr(),
                 0 if full.dim() == 2 else T * full.shape[-1], b.n_ctrl, ic, ec, _lib.ptr(st["params_init"]),
                 _lib.ptr(st["params_end"]), _lib.ptr(st["init_pos"]), _lib.stream_of(gpu_device))
        ref = b.fixed_term(full, st["params_init"], st["params_end"], st["init_pos"], fit=False)
        got = pos.cpu().numpy()
        np.testing.assert_allclose(got[..., tok.joint_indices], ref.cpu().numpy(), rtol=1e-6, atol=1e-6)
        assert not got[..., g].any()


@pytest.mark.parametrize("loop", ["batch"])
@pytest.mark.parametrize("case", ["traj_k2/2048", "skew/700", "wide3000/2048", "repeat700/300", "runs/2048"])
def test_bpe_device_loop_matches_hf(case, loop, bpe_golden, gpu_device):
    """The device-driven merge loop (merges decided on the GPU, ids by string hash, replayed and
    verified on the host) gives HF's vocab and merges; so does its collision fallback (forced
    here with a degenerate hash multiplier, so that different strings collide)."""
    from beast_tokenizer_amd.bpe_train import GpuBpeOps, fixed_rows_to_device, train_bpe
    ref, corpora = bpe_golden
    cname, vs = case.split("/")
    flat, off = fixed_rows_to_device(torch.from_numpy(corpora[cname].astype(np.int64)).to(gpu_device))
    ops = GpuBpeOps(gpu_device)
    ops._loop_kind = loop
    res = train_bpe(flat, off, int(vs), ops=ops)
    assert res.stats.get("device_loop") is True and res.stats.get("loop") == loop
    assert res.vocab == ref[case]["vocab"]
    assert [list(m) for m in res.merges] == ref[case]["merges"]

    class Degenerate(GpuBpeOps):
        LOOP_P = 0          # h(string) = its last byte: distinct strings collide -> host fallback
    dg = Degenerate(gpu_device)
    dg._loop_kind = loop
    res2 = train_bpe(flat, off, int(vs), ops=dg)
    assert res2.vocab == ref[case]["vocab"]
    assert [list(m) for m in res2.merges] == ref[case]["merges"]


@pytest.mark.parametrize("loop", ["batch2", "batch4", "batch"])
@pytest.mark.parametrize("case", ["skew/300", "skew/2048", "traj_k2/700", "traj_k3/2048", "rand256/2048",
                                  "repeat700/700", "repeat700/2048", "runs/300", "runs/700"])
def test_bpe_batched_loop_matches_hf(case, loop, bpe_golden, gpu_device):
    """Several merges per pass (csrc/bpe.hip k_merge_batch: the top pairs in HF order while they
    are symbol-disjoint, no id re-use after the first, no taken row's second-best above the next)
    give exactly HF's sequential merges -- with batches of 2, 4 and 8, on corpora with id re-use
    (repeat700), self-pair runs (runs), the min_frequency stop (repeat700/2048) and wide alphabets."""
    from beast_tokenizer_amd.bpe_train import GpuBpeOps, fixed_rows_to_device, train_bpe
    ref, corpora = bpe_golden
    cname, vs = case.split("/")
    flat, off = fixed_rows_to_device(torch.from_numpy(corpora[cname].astype(np.int64)).to(gpu_device))
    ops = GpuBpeOps(gpu_device)
    ops._loop_kind = loop
    res = train_bpe(flat, off, int(vs), ops=ops)
    assert res.stats.get("device_loop") is True and res.stats.get("loop") == loop
    assert [list(m) for m in res.merges] == ref[case]["merges"]
    assert res.vocab == ref[case]["vocab"]


@pytest.mark.parametrize("loop", ["batch", "host"])
@pytest.mark.parametrize("special,max_len,min_freq", [
    ((), 10000, 2), (("<pad>", "<eos>"), 10000, 2), ((), 3, 2), ((), 10000, 5), (("<s>",), 2, 3), ((), 4, 7)])
def test_train_options_match_live_hf(special, max_len, min_freq, loop, gpu_device):
    """HF's BpeTrainer options through the device loops against HF itself, live: special tokens
    (ids first, never in words), max_token_length (the batched loop's length lookups, with new
    tokens of the same batch as neighbours), min_frequency (a stop inside a batch)."""
    from tokenizers import ByteLevelBPETokenizer
    from tokenizers.trainers import BpeTrainer
    from beast_tokenizer_amd.bpe_train import GpuBpeOps, fixed_rows_to_device, train_bpe
    rng = np.random.default_rng(len(special) * 100 + max_len + min_freq)
    base = rng.integers(0, 300, size=9)
    arr = base[rng.integers(0, 9, size=(600, 48))]
    arr[::7] = rng.integers(0, 300, size=(arr[::7].shape[0], 48))
    lo, hi = int(arr.min()), int(arr.max())
    bpe = ByteLevelBPETokenizer()
    tr = BpeTrainer(vocab_size=1500, min_frequency=min_freq, show_progress=False, special_tokens=list(special),
                    initial_alphabet=[chr(i) for i in range(hi - lo + 1)], max_token_length=max_len)
    bpe._tokenizer.train_from_iterator(["".join(map(chr, r - lo)) for r in arr], trainer=tr)
    m = json.loads(bpe._tokenizer.to_str())["model"]
    flat, off = fixed_rows_to_device(torch.from_numpy(arr.astype(np.int64)).to(gpu_device))
    ops = GpuBpeOps(gpu_device)
    res = train_bpe(flat, off, 1500, min_frequency=min_freq, special_tokens=special, max_token_length=max_len,
                    ops=ops, device_loop=loop != "host")
    assert res.stats.get("loop") == loop
    assert [list(x) for x in res.merges] == [list(x) for x in m["merges"]]
    assert res.vocab == m["vocab"]
