"""GPU tests of encode_at / beast_encode_rows_f32: the per-trajectory weighted ridge fit on row-wise
different time stamps (csrc/fit_rows.hip) against the float64 oracle (tests/rows_oracle.py) and the
reference goldens (tests/golden/gen_rows_goldens.py).

Parity criterion: the project's own (tests/test_gpu_parity.py), |gpu - ref| <= 1e-5 * max(1, |ref row|_inf).
The kernel accumulates and solves in float64 and rounds once, so against the oracle it is expected
to differ by an fp32 rounding of a float64 difference of about cond(G) * 1e-16.
"""
import numpy as np
import pytest
import torch

from conftest import load_json, load_npz

pytestmark = pytest.mark.gpu

from beast_tokenizer_amd import BEASTBsplineBPETokenizer, BEASTBsplineTokenizer  # noqa: E402
from oracle import beast_oracle as O  # noqa: E402
import rows_oracle as R  # noqa: E402

TWO_PI = 2 * np.pi
TOL = load_json("rows_tolerances.json")


def make_tok(dev, D, N, degree, grippers=(), duration=TWO_PI, cls=BEASTBsplineTokenizer, **kw):
    return cls(num_dof=D, num_basis=N, degree_p=degree, duration=duration, gripper_indices=list(grippers) or None,
               gripper_zero_order=bool(grippers), device=str(dev), **kw)


def oracle_for(tok, x, times, weights=None):
    return R.fit(x, times, weights, tau=np.float32(tok.duration), degree=tok.degree_p, num_basis=tok.num_basis,
                 joint_indices=tok.joint_indices, gripper_indices=tok.gripper_indices)


def dev_t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def assert_parity(got, ref, what=""):
    ok = R.parity_ok(got, ref)
    assert ok.all(), (what, R.parity_err(got, ref))


# B, T, N, degree, D, grippers: T a multiple of 4 or not and the cap of 256; N = degree + 1, 10, 16;
# every degree the dispatch has a k_fit_rows<K> for (0 .. 8), each at N = degree + 1 and N = 16 from
# degree 2 on; D = 1, 7, 14 with two grippers, 17 (a second 16-column tile), 64; B = 1, 3, 67 (a
# ragged last workgroup of 4 waves), 1,025 (two kinds: 2,050 items, one per wave -- a wave takes a
# second item only above 32 items per CU, which tests/test_gpu_second_pass.py arranges)
SHAPES = [
    (3, 2, 2, 1, 1, ()),
    (67, 7, 4, 3, 7, ()),
    (1025, 50, 10, 4, 14, (6, 13)),
    (3, 256, 16, 4, 17, ()),
    (67, 50, 10, 0, 7, ()),
    (1, 50, 5, 4, 64, (3, 40)),
    (1025, 50, 16, 3, 1, ()),
    (5, 11, 3, 2, 3, ()), (5, 50, 16, 2, 2, (1,)),
    (5, 19, 6, 5, 3, ()), (5, 50, 16, 5, 2, (1,)),
    (5, 23, 7, 6, 3, ()), (5, 50, 16, 6, 2, (1,)),
    (5, 26, 8, 7, 3, ()), (5, 50, 16, 7, 2, (1,)),
    (5, 29, 9, 8, 3, ()), (5, 50, 16, 8, 2, (1,)),
]


@pytest.mark.parametrize("B,T,N,degree,D,grippers", SHAPES)
def test_params_match_the_oracle(gpu_device, B, T, N, degree, D, grippers):
    """Random-walk inputs, jittered times, real-valued weights in [0.25, 4]."""
    tok = make_tok(gpu_device, D, N, degree, grippers)
    seed = 1000 + B + T + N + D
    x, t = R.random_walk(B, T, D, seed), R.jittered_times(B, T, TWO_PI, seed + 1)
    w = np.random.default_rng(seed + 2).uniform(0.25, 4.0, (B, T)).astype(np.float32)
    want, cond = oracle_for(tok, x, t, w)
    tokens, pd = tok.encode_at(dev_t(x, gpu_device), dev_t(t, gpu_device), dev_t(w, gpu_device))
    params = pd["params"].cpu().numpy()
    print("err vs oracle", R.parity_err(params, want), "max cond", cond.max())
    assert params.shape == (B, D * N) and params.dtype == np.float32
    assert tokens.shape == (B, N * D) and tokens.dtype == torch.int64
    assert_parity(params, want)
    # float64 throughout: an fp32 rounding of the oracle's float64 value, or its neighbour
    assert np.abs(params.astype(np.float64) - want).max() <= 2.0 ** -22 * max(1.0, np.abs(want).max())


def test_views_shared_times_and_no_weights(gpu_device):
    """Non-contiguous input (sliced last dimension, transposed batch), times [T] (times_sb = 0),
    weights None and [T]: the same results as contiguous [B, T] arguments."""
    B, T, D, N = 67, 50, 7, 10
    tok = make_tok(gpu_device, D, N, 4)
    x = R.random_walk(B, T, D, 77)
    t1 = R.jittered_times(1, T, TWO_PI, 78)[0]
    w1 = np.random.default_rng(79).uniform(0.25, 4.0, T).astype(np.float32)
    want, _ = oracle_for(tok, x, t1, None)
    xd, td = dev_t(x, gpu_device), dev_t(t1, gpu_device)
    base = tok.encode_at(xd, td)[1]["params"]
    assert_parity(base.cpu().numpy(), want)
    wide = torch.zeros((B, T, D + 5), device=gpu_device)
    wide[..., :D] = xd
    sliced = wide[..., :D]                                         # row stride D + 5
    tb = xd.permute(1, 0, 2).contiguous().permute(1, 0, 2)         # stored [T, B, D]
    col = xd.permute(2, 0, 1).contiguous().permute(1, 2, 0)        # stored [D, B, T]: last stride != 1
    assert not sliced.is_contiguous() and not tb.is_contiguous() and col.stride(2) != 1
    for v in (sliced, tb, col):
        assert torch.equal(tok.encode_at(v, td)[1]["params"], base)
    # [B, T] copies, an expanded view (stride 0) and a strided view of the times
    tt = td.expand(B, T)
    t2 = torch.stack([td, td], dim=-1)[..., 0].expand(B, T)        # element stride 2
    for tv in (tt, tt.contiguous(), t2):
        assert torch.equal(tok.encode_at(xd, tv)[1]["params"], base)
    assert torch.equal(tok.encode_at(xd, td, torch.ones(T, device=gpu_device))[1]["params"], base)
    ww, _ = oracle_for(tok, x, t1, w1)
    got = tok.encode_at(xd, td, dev_t(w1, gpu_device))[1]["params"]
    assert_parity(got.cpu().numpy(), ww)
    assert torch.equal(tok.encode_at(xd, tt, dev_t(w1, gpu_device).expand(B, T).contiguous())[1]["params"], got)
    # host tensors move to the tokenizer's device, as in encode
    assert torch.equal(tok.encode_at(torch.from_numpy(x), torch.from_numpy(t1))[1]["params"], base)
    # an empty batch
    tk, pd = tok.encode_at(xd[:0], td)
    assert tk.shape == (0, N * D) and pd["params"].shape == (0, D * N)


@pytest.mark.parametrize("name", sorted(TOL))
def test_params_match_the_reference_goldens(gpu_device, name):
    """The reference's learn_mp_params_from_trajs on row-wise different times (for the 0/1-weight
    case: on the compacted trajectories), same criterion.  Budget: the GPU's error against the
    oracle plus the reference's recorded own error (<= 5e-6, rows_tolerances.json)."""
    g, c = load_npz(f"rows_{name}.npz"), TOL[name]["config"]
    tok = make_tok(gpu_device, c["D"], c["N"], c["degree"], c.get("grippers", ()), c.get("duration", TWO_PI))
    _, pd = tok.encode_at(dev_t(g["x"], gpu_device), dev_t(g["times"], gpu_device), dev_t(g.get("weights"), gpu_device))
    params = pd["params"].cpu().numpy()
    want, _ = oracle_for(tok, g["x"], g["times"], g.get("weights"))
    print("err vs oracle", R.parity_err(params, want), "vs reference", R.parity_err(params, g["ref_params"]),
          "reference's own", TOL[name]["ref_err"])
    assert_parity(params, want, "oracle")
    assert_parity(params, g["ref_params"], "reference")


def test_float64_is_really_used(gpu_device):
    """0/1 weights keeping about half of 50 samples: rows are grouped by the oracle's own cond(G).
    Both the well-conditioned rows and those with 1e4 <= cond <= 1e6 meet the criterion; an fp32
    Gram or solve would miss it by cond * 6e-8 in the second group.  Rows above 1e6 are not asserted."""
    tok = make_tok(gpu_device, 7, 10, 4)
    x, t, w = R.census_inputs()
    want, cond = oracle_for(tok, x, t, w)
    cond = cond[:, 0]
    easy, hard = cond <= 1e3, (cond >= 1e4) & (cond <= 1e6)
    assert easy.sum() >= 16 and hard.sum() >= 4, (easy.sum(), hard.sum())
    _, pd = tok.encode_at(dev_t(x, gpu_device), dev_t(t, gpu_device), dev_t(w, gpu_device))
    params = pd["params"].cpu().numpy()
    print("easy rows", easy.sum(), R.parity_err(params[easy], want[easy]), "hard rows", hard.sum(),
          R.parity_err(params[hard], want[hard]), "max cond asserted", cond[hard].max())
    assert_parity(params[easy], want[easy], "cond <= 1e3")
    assert_parity(params[hard], want[hard], "1e4 <= cond <= 1e6")
    assert np.isfinite(params).all()


def fitted_tok(dev, D=14, grippers=(6, 13), cls=BEASTBsplineTokenizer, **kw):
    """A tokenizer whose bounds are the 1 % / 99 % quantiles of random-walk params (so that some
    params are clamped), with the inputs."""
    tok = make_tok(dev, D, 10, 4, grippers, cls=cls, **kw)
    x = R.random_walk(256, 50, D, 41)
    lay_p, _ = oracle_for(tok, x, O.times_grid(TWO_PI, 50))
    lo, hi = np.quantile(lay_p, 0.01, 0).astype(np.float32), np.quantile(lay_p, 0.99, 0).astype(np.float32)
    tok.load_state_dict({"w_min": lo.tolist(), "w_max": hi.tolist()})
    return tok, x, lo, hi


def test_tokens_are_the_quantiser_s(gpu_device):
    """Tokens are bitwise beast_quantize_f32 of the kernel's own params, with and without the LLM
    offset; encode_continuous_at is bitwise _quantize(mode=1) of the same params; update_bounds
    widens the bounds first, as encode does."""
    tok, x, lo, hi = fitted_tok(gpu_device)
    B, T, D, N = 256, 50, 14, 10
    t = R.jittered_times(B, T, TWO_PI, 42)
    w = np.random.default_rng(43).uniform(0.25, 4.0, (B, T)).astype(np.float32)
    xd, td, wd = dev_t(x, gpu_device), dev_t(t, gpu_device), dev_t(w, gpu_device)
    tokens, pd = tok.encode_at(xd, td, wd)
    params = pd["params"]
    assert torch.equal(tokens, tok._quantize(params, 0, gpu_device, 0))
    assert np.array_equal(tokens.cpu().numpy(), R.tokens(params.cpu().numpy(), lo, hi, 256, D, N))
    assert int(tokens.min()) == 0 and int(tokens.max()) == 255          # both clamps were exercised
    tok.set_llm_vocab_size(32000)
    t_llm, pd2 = tok.encode_at(xd, td, wd)
    assert torch.equal(pd2["params"], params)
    assert torch.equal(t_llm, tokens + (32000 - 256)) and torch.equal(t_llm, tok._quantize(params, 32000 - 256, gpu_device, 0))
    assert torch.equal(tok.encode_at(xd, td, wd, respect_llm_vocab_size=False)[0], tokens)
    tok.set_llm_vocab_size(None)
    cont, pd3 = tok.encode_continuous_at(xd, td, wd)
    assert torch.equal(pd3["params"], params) and torch.equal(cont, tok._quantize(params, 0, gpu_device, 1))
    assert cont.dtype == torch.float32 and float(cont.min()) == -1.0 and float(cont.max()) == 1.0
    # update_bounds: fit, widen by the batch extremes, then quantise with the new bounds
    tk, pd4 = tok.encode_at(xd * 3, td, wd, update_bounds=True)
    p4 = pd4["params"].cpu().numpy()
    nlo, nhi = O.update_bounds_per_batch(lo, hi, p4)
    assert np.array_equal(tok.w_min.cpu().numpy(), nlo) and np.array_equal(tok.w_max.cpu().numpy(), nhi)
    assert not np.array_equal(nlo, lo)
    assert np.array_equal(tk.cpu().numpy(), R.tokens(p4, nlo, nhi, 256, D, N))


def test_consistent_with_the_shared_grid_encode(gpu_device):
    """On tok.times repeated per row with unit weights, encode_at's params are within the criterion
    of encode's, and tokens differ only where the oracle's normalised value lies within 1e-3 of a
    .5 tie (at most 1 % of the entries)."""
    tok, x, lo, hi = fitted_tok(gpu_device)
    B, T, D, N = 256, 50, 14, 10
    xd = dev_t(x, gpu_device)
    tok_s, pd_s = tok.encode(xd)
    times = tok.times.reshape(1, -1).expand(B, T).contiguous()
    tok_r, pd_r = tok.encode_at(xd, times, torch.ones((B, T), device=gpu_device))
    assert_parity(pd_r["params"].cpu().numpy(), pd_s["params"].cpu().numpy())
    want, _ = oracle_for(tok, x, O.times_grid(TWO_PI, T))
    units = O.normalized_units(want, lo, hi, 256).reshape(B, D, N).transpose(0, 2, 1).reshape(B, N * D)
    near_tie = np.abs(units - np.floor(units) - 0.5) < 1e-3
    assert near_tie.mean() <= 0.01, near_tie.mean()
    diff = (tok_r != tok_s).cpu().numpy()
    print("token differences", int(diff.sum()), "entries near a tie", int(near_tie.sum()))
    assert not (diff & ~near_tie).any()


def test_missing_frames(gpu_device):
    """NaN in traj and times at zero-weight samples changes nothing, bit for bit; a row without any
    weight gives params exactly 0 and finite tokens; rows of a batch are independent."""
    tok, _, lo, hi = fitted_tok(gpu_device)
    B, T, D = 67, 50, 14
    x, t = R.random_walk(B, T, D, 51), R.jittered_times(B, T, TWO_PI, 52)
    w = (np.random.default_rng(53).random((B, T)) < 0.7).astype(np.float32)
    w[:10, 40:] = 0                    # short tails: the last basis functions see no sample
    w[5] = 0                           # a row with no sample at all
    w[6, 1:] = 0                       # a row with one sample
    xn, tn = x.copy(), t.copy()
    xn[w == 0] = np.nan
    tn[w == 0] = np.inf
    tn[7][w[7] == 0] = np.nan
    wd = dev_t(w, gpu_device)
    tk, pd = tok.encode_at(dev_t(x, gpu_device), dev_t(t, gpu_device), wd)
    tkn, pdn = tok.encode_at(dev_t(xn, gpu_device), dev_t(tn, gpu_device), wd)
    assert torch.equal(pd["params"], pdn["params"]) and torch.equal(tk, tkn)
    params = pd["params"].cpu().numpy()
    assert np.isfinite(params).all()
    assert not params[5].any()
    assert np.array_equal(tk[5].cpu().numpy(), R.tokens(np.zeros((1, D * 10), np.float32), lo, hi, 256, D, 10)[0])
    assert int(tk.min()) >= 0 and int(tk.max()) <= 255
    want, cond = oracle_for(tok, xn, tn, w)
    ok = (cond <= 1e6).all(axis=1)
    assert ok.sum() >= B // 2
    assert_parity(params[ok], want[ok])
    # permuting the batch permutes the outputs bitwise
    perm = torch.from_numpy(np.random.default_rng(54).permutation(B)).to(gpu_device)
    tkp, pdp = tok.encode_at(dev_t(xn, gpu_device)[perm], dev_t(tn, gpu_device)[perm], wd[perm])
    assert torch.equal(pdp["params"], pd["params"][perm]) and torch.equal(tkp, tk[perm])


def test_round_trip_on_its_own_time_stamps(gpu_device):
    """reconstruct_traj(encode_at(y, times)[0], times=times) on splines sampled at jittered times:
    the basis functions are a partition of unity, so the position error is at most the largest
    per-coefficient quantisation error of the DoF (the bound of test_roundtrip_properties: half a
    bin, (1 + 1e-5), plus three fp32 roundings of the dequantiser), plus the fit's and the
    reconstruction's own rounding, 2e-5 * max(1, |y|)."""
    B, T, D, N = 67, 50, 7, 10
    tok = make_tok(gpu_device, D, N, 4)
    tok.load_state_dict({"w_min": [-1.0] * (D * N), "w_max": [1.0] * (D * N)})
    rng = np.random.default_rng(61)
    wtrue = rng.uniform(-0.95, 0.95, (B, D, N))
    t = R.jittered_times(B, T, TWO_PI, 62)
    phi = O.basis(t, np.float32(TWO_PI), 4, N).astype(np.float64)                # [B, T, N]
    y = np.einsum("btn,bdn->btd", phi, wtrue).astype(np.float32)
    td = dev_t(t, gpu_device)
    tokens, pd = tok.encode_at(dev_t(y, gpu_device), td)
    assert np.abs(pd["params"].cpu().numpy().reshape(B, D, N) - wtrue).max() <= 1e-5
    pos = tok.reconstruct_traj(tokens, times=td).cpu().numpy()
    binw = 2.0 / 255
    bound = 0.5 * binw * (1 + 1e-5) + 4e-7 + 1e-7 + 2e-5 * max(1.0, np.abs(y).max())
    err = np.abs(pos - y).max()
    print("round trip max error", err, "bound", bound)
    assert pos.shape == y.shape and err <= bound
    assert err > 1e-4                                                              # it did quantise


def test_bpe_tokenizer_encodes_the_same_mp_tokens(gpu_device):
    tok, x, _, _ = fitted_tok(gpu_device, D=7, grippers=(), cls=BEASTBsplineBPETokenizer, bpe_vocab_size=400)
    tok.fit_from_trajectories([torch.from_numpy(x)], show_progress=False)
    B, T = 9, 37                                                                   # T is not seq_len
    y, t = R.random_walk(B, T, 7, 71), R.jittered_times(B, T, TWO_PI, 72)
    w = np.random.default_rng(73).uniform(0.25, 4.0, (B, T)).astype(np.float32)
    yd, td, wd = dev_t(y, gpu_device), dev_t(t, gpu_device), dev_t(w, gpu_device)
    ids, pd, mp = tok.encode_at(yd, td, wd, return_mp_tokens=True)
    base_mp, base_pd = BEASTBsplineTokenizer.encode_at(tok, yd, td, wd, respect_llm_vocab_size=False)
    assert torch.equal(mp, base_mp) and torch.equal(pd["params"], base_pd["params"])
    assert ids == tok._discrete_to_bpe(mp) and len(ids) == B
    block = tok.encode_at(yd, td, wd, return_tensors=True)[0]
    assert block.to_lists() == ids
    assert torch.equal(tok.bpe_to_mp_tokens(ids), mp)
