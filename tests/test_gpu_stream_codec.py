"""k_encode_stream and k_reconstruct_wide (csrc/codec_stream.h) against the float64 oracle, by the
yardsticks of tests/test_gpu_codec_dispatch.py: params within (Tp + 8) * 2^-24 * sum_t |P||y| of the
float64 fit (a Tp-term fp32 chain), tokens the quantiser of the kernel's own params, decode bitwise,
positions within 1e-5 * max(1, |ref|) of float64 basis @ params (a B-spline row has at most
degree + 1 non-zero entries summing to 1, so the bar holds at N = 32); alone, strided or misaligned
give the same bits.  Shapes sit on the chunk boundaries the library's queries report; a batch is one
trajectory more than the kernel's tile, allocated at its exact size."""
import numpy as np
import pytest
import torch

from beast_tokenizer_amd import BEASTBsplineTokenizer, _lib
from beast_tokenizer_amd.synthetic import synth_trajectories
from oracle import beast_oracle as O

pytestmark = pytest.mark.gpu

F32, TAU, VOCAB = np.float32, np.float32(2 * np.pi), 256
NREF = 9   # trajectories of a reference: one more than the widest tile


def _tok(dev, D, N, T, grip, lo, hi):
    tok = BEASTBsplineTokenizer(num_dof=D, num_basis=N, seq_len=T, vocab_size=VOCAB, gripper_zero_order=bool(grip),
                                gripper_indices=grip, device=str(dev))
    tok.load_state_dict({"w_min": lo.tolist(), "w_max": hi.tolist()})
    return tok


def _enc_ref(T, D, N, grip):
    """(x [NREF,T,D], float64 fit rounded once, bound sums, w_min, w_max at the 5 % / 95 % quantiles)."""
    x = synth_trajectories(NREF, T, D, seed=100 + T + D, gripper_indices=grip or ())
    t, lay = O.times_grid(2 * np.pi, T), O.Layout.make(D, grip, bool(grip))
    exact, sums = [], []
    for idx, deg in ((lay.joint_indices, 4), (lay.gripper_indices, 0)):
        if idx:
            phi = O.basis(t, TAU, deg, N)
            exact.append(O.fit_exact(x[..., idx], phi))
            sums.append(np.einsum("nt,btd->bdn", np.abs(O.projection_f64(phi)),
                                  np.abs(x[..., idx].astype(np.float64))).reshape(NREF, -1))
    exact, sums = np.concatenate(exact, axis=-1), np.concatenate(sums, axis=-1)
    return x, exact, sums, np.quantile(exact, 0.05, axis=0).astype(F32), np.quantile(exact, 0.95, axis=0).astype(F32)


def _mark(family, fast=None, **fields):
    m = _lib.last_codec_launch()
    assert m.family == family and m.waves == 4 and (fast is None or m.fast == fast), m
    assert all(getattr(m, k) == v for k, v in fields.items()), m
    return m.tile


# (id, T or a function of the chunk TC, N, D, gripper DoFs)
ENCODE = [
    ("t50_n17", 50, 17, 14, None),                        # the second row tile with one live row
    ("t64_n32_d5", 64, 32, 5, None),                      # both row tiles full
    ("t257_n10", 257, 10, 14, None),                      # the first T past the resident envelope; 4-byte DMA units
    ("tc+1_n17", lambda tc: tc + 1, 17, 14, None),        # one sample in the second chunk
    ("2tc+3_n20_grip", lambda tc: 2 * tc + 3, 20, 14, [5, 9]),   # a buffer swap, a tail off the 4-grid, both kinds
]


@pytest.mark.parametrize("T,N,D,grip", [r[1:] for r in ENCODE], ids=[r[0] for r in ENCODE])
def test_encode_stream(T, N, D, grip, gpu_device):
    dev, lib = gpu_device, _lib.load()
    tc = lib.beast_encode_stream_chunk(4096, D, D, D - len(grip or ()), N, 1)
    second_chunk = callable(T) and T(0) == 1
    T = T(tc) if callable(T) else T
    assert tc > 0 and tc % 4 == 0 and T >= 2 * N          # well-conditioned ridge systems
    x, exact, sums, lo, hi = _enc_ref(T, D, N, grip)
    tok, DN = _tok(dev, D, N, T, grip, lo, hi), D * N
    xd = torch.from_numpy(x).to(dev)
    t1, pd1 = tok.encode(xd[:1].clone())                  # alone: the tile width is known after a launch
    B = _mark("encode_dyn", True, staged=False) + 1
    t0, pd0 = tok.encode(xd[:B].clone())                  # exact-size allocation: nothing follows the last trajectory
    assert B <= NREF and _mark("encode_dyn", True, staged=False) == B - 1
    params0, tokens0 = pd0["params"].cpu().numpy(), t0.cpu().numpy()
    assert torch.equal(pd1["params"][0], pd0["params"][0]) and torch.equal(t1[0], t0[0])
    # values: the float64 fit, the quantiser on the kernel's own params, both clamp sides hit
    bound = (-(-T // 4) * 4 + 8) * 2.0 ** -24 * sums[:B] + 1e-30
    assert np.all(np.abs(params0 - exact[:B]) <= bound), float(np.max(np.abs(params0 - exact[:B]) / bound))
    assert (params0 < lo).any() and (params0 > hi).any()
    want = O.continuous_to_discrete(O._clamp_t(params0, lo, hi), lo, hi, VOCAB)
    want = want.reshape(B, D, N).transpose(0, 2, 1).reshape(B, DN)
    assert np.array_equal(tokens0, want) and want.min() == 0 and want.max() == VOCAB - 1
    # a strided view of a wider, longer buffer (gathered, the same chunk): the same bits.  Its rows of D + 2
    # floats read in place by DMA take another chunk, so another order of summation: the bound
    big = torch.full((B, T + 4, D + 2), float("nan"), device=dev)
    big[:, :T, :D] = xd[:B]
    t2, pd2 = tok.encode(big[:, :T, :D])
    assert _mark("encode_dyn", False, staged=False) and torch.equal(pd2["params"], pd0["params"]) and torch.equal(t2, t0)
    wide = tok.encode(big[:, :T].contiguous())[1]["params"].cpu().numpy()
    assert _mark("encode_dyn", True, staged=False) and np.all(np.abs(wide - exact[:B]) <= bound)
    # misaligned outputs (params 4, tokens 8 bytes past a 16-byte boundary): the same bits, guards intact
    pbuf = torch.full((B * DN + 8,), -7777.0, device=dev)
    tbuf = torch.full((B * DN + 8,), -7777, dtype=torch.int64, device=dev)
    pv, tv, p = pbuf[1:1 + B * DN].view(B, DN), tbuf[1:1 + B * DN].view(B, DN), tok._plan()
    assert pv.data_ptr() % 16 == 4 and tv.data_ptr() % 16 == 8
    _lib.check(lib.beast_encode_f32(xd.data_ptr(), B, T, T * D, D, 1, D, D, tok.joint_dof, p.p_src, p.p_proj, N, p.p_wmn,
                                    p.p_wmx, VOCAB, 0, pv.data_ptr(), tv.data_ptr(), _lib.raw_stream(p.idx)))
    assert torch.equal(pv, pd0["params"]) and torch.equal(tv, t0)
    assert all(bool((g == -7777).all()) for g in (pbuf[:1], pbuf[1 + B * DN:], tbuf[:1], tbuf[1 + B * DN:]))
    if second_chunk:   # NaN after a trajectory's last sample is never read into its sums
        xn = xd[:B].clone()
        xn[1] = float("nan")
        pn = tok.encode(xn)[1]["params"][0]
        assert bool(torch.isfinite(pn).all()) and torch.equal(pn, pd0["params"][0])


def test_encode_stream_second_pass(gpu_device):
    """A workgroup's second and third tile: more than twice as many tiles as the grid holds."""
    dev, T, N, D = gpu_device, 257, 10, 2
    tok = _tok(dev, D, N, T, None, np.full(D * N, -1.0, F32), np.full(D * N, 1.0, F32))
    base = torch.from_numpy(synth_trajectories(64, T, D, seed=7)).to(dev)
    tok.encode(base[:1].clone())
    tile = _mark("encode_dyn", staged=False)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    tok.encode(base.repeat(tile * 16 * cus // 64 + 1, 1, 1))    # enough tiles to fill any grid
    B = tile * 2 * _lib.last_launch_grid() + 3
    x = base.repeat(-(-B // 64), 1, 1)[:B].contiguous()
    tokens, pd = tok.encode(x)
    assert 2 * _lib.last_launch_grid() <= -(-B // tile)
    t_last, pd_last = tok.encode(x[-3:].clone())
    assert torch.equal(pd["params"][-3:], pd_last["params"]) and torch.equal(tokens[-3:], t_last)


# (id, N, T_out as a function of the row chunk RC, gripper DoFs, variant)
RECONSTRUCT = [(f"n{N}_{name}", N, f, None, "") for N in (17, 32)
               for name, f in (("t5", lambda rc: 5), ("rc+1", lambda rc: rc + 1), ("2rc+3", lambda rc: 2 * rc + 3))]
RECONSTRUCT += [
    ("scatter_grip", 20, lambda rc: rc + 1, [5, 9], "scatter"),   # permuted dof_dst into D + 3 columns
    ("init_p", 17, lambda rc: rc + 1, [5, 9], "init_p"),
    ("ntokens", 24, lambda rc: rc + 1, None, "ntokens"),
    ("llm_offset", 17, lambda rc: 5, None, "offset"),
]


@pytest.mark.parametrize("N,T,grip,variant", [r[1:] for r in RECONSTRUCT], ids=[r[0] for r in RECONSTRUCT])
def test_reconstruct_wide(N, T, grip, variant, gpu_device):
    dev, lib, D = gpu_device, _lib.load(), 14
    lay = O.Layout.make(D, grip, bool(grip))
    dst, ndo = ([16, 0, 3, 8, 1, 5, 12, 2, 15, 10, 7, 13, 4, 9], D + 3) if variant == "scatter" else (lay.order, D)
    rc = lib.beast_reconstruct_stream_rows(50, D, D - len(grip or ()), N, ndo)
    assert rc > 0 and rc % 4 == 0
    T, off = T(rc), 1000 if variant == "offset" else 0
    rng = np.random.default_rng(N * 100 + T)
    lo = rng.uniform(-3, 1, size=D * N).astype(F32)
    hi = (lo + rng.uniform(0.1, 4, size=D * N)).astype(F32)
    tokens = rng.integers(0, VOCAB, size=(NREF, N * D)).astype(np.int64)
    tokens[0, :4] = (0, VOCAB - 1, VOCAB + 7, -1)          # the vocabulary's ends and tokens outside it
    nt = rng.uniform(-1.2, 1.2, size=(NREF, N * D)).astype(F32)
    init_p = rng.uniform(-2, 2, size=(NREF, 2 * D)).astype(F32)
    tok = _tok(dev, D, N, 64, grip, lo, hi)
    times = np.linspace(0, 2 * np.pi, T).astype(F32)
    tokens_t, nt_t, ip_t = (torch.from_numpy(a).to(dev) for a in (tokens + off, nt, init_p))
    dst_t, p = torch.tensor(dst, dtype=torch.int32, device=dev), tok._plan()
    phi, p_phi, basis_sb, _ = tok._basis_for(torch.from_numpy(times), NREF, p)   # a shared 1-D grid

    def run(B):
        pos = torch.full((B, T, ndo), float("nan"), device=dev)
        ip = ip_t.data_ptr() if variant == "init_p" else None
        _lib.check(lib.beast_reconstruct_f32(
            tokens_t.data_ptr(), B, D, tok.joint_dof, N, VOCAB, off, p.p_wmn, p.p_wmx, p_phi, basis_sb, T,
            dst_t.data_ptr(), ndo, ip, 2 * D, p.p_dst if ip else None, None, pos.data_ptr(),
            nt_t.data_ptr() if variant == "ntokens" else None, _lib.raw_stream(p.idx)))
        return pos

    # decode: params_out only, bitwise the host's discrete_to_continuous
    want_dec = O.decode(tokens, lay, N, lo, hi, VOCAB)
    assert np.array_equal(tok.decode(tokens_t - off).cpu().numpy(), want_dec) and _mark("reconstruct_mfma", ks=0)
    alone = run(1)
    B = _mark("reconstruct_mfma", ks=0, staged=True) + 1
    pos_t = run(B)
    assert B <= NREF and _mark("reconstruct_mfma", ks=0, staged=True) == B - 1 and torch.equal(alone[0], pos_t[0])
    pos, w = pos_t.cpu().numpy(), want_dec[:B].reshape(B, D, N).astype(np.float64)
    if variant == "ntokens":   # denormalize_tensor's intent (beast/utils.py:38-44)
        u = (np.clip(nt[:B].astype(np.float64), -1, 1).reshape(B, N, D).transpose(0, 2, 1) + 1) / 2
        w = u * (hi.astype(np.float64) - lo).reshape(D, N) + lo.reshape(D, N)
    if variant == "init_p":   # coefficient 0 of the joint DoFs <- init_p[:, the DoF's column]
        w[:, :len(lay.joint_indices), 0] = init_p[:B][:, lay.joint_indices]
    want = np.zeros((B, T, ndo))
    pj, pg = (O.basis(times, TAU, deg, N).astype(np.float64) for deg in (4, 0))
    for i in range(D):
        want[:, :, dst[i]] = np.einsum("tn,bn->bt", pj if i < len(lay.joint_indices) else pg, w[:, i])
    err = np.abs(pos - want) / np.maximum(1.0, np.abs(want).max(axis=(1, 2), keepdims=True))
    assert err.max() <= 1e-5, float(err.max())
    assert not pos[:, :, sorted(set(range(ndo)) - set(dst))].any()


def test_api_round_trip(gpu_device, tmp_path):
    dev, D, N, T = gpu_device, 7, 24, 300
    tok = BEASTBsplineTokenizer(num_dof=D, num_basis=N, seq_len=T, device=str(dev))
    x = synth_trajectories(64, T, D, seed=3)
    tok.fit_parameters([{"actions": torch.from_numpy(x[i:i + 16])} for i in range(0, 64, 16)], verbose=False)
    xd = torch.from_numpy(x).to(dev)
    tokens, pd = tok.encode(xd)
    pos = tok.reconstruct_traj(tokens, times=tok.times).cpu().numpy().astype(np.float64)
    # the quantiser's property, in float64 from the bounds: a coefficient moves by its clamp plus at most a bin
    phi = O.basis(O.times_grid(2 * np.pi, T), TAU, 4, N).astype(np.float64)
    params = pd["params"].cpu().numpy().astype(np.float64).reshape(64, D, N)
    lo, hi = (b.cpu().numpy().astype(np.float64).reshape(D, N) for b in (tok.w_min, tok.w_max))
    moved = np.abs(np.clip(params, lo, hi) - params) + (hi - lo) / (VOCAB - 1)
    allowed = np.abs(np.einsum("tn,bdn->btd", phi, params) - x) + np.einsum("tn,bdn->btd", phi, moved) + 1e-5
    assert np.all(np.abs(pos - x) <= allowed)
    tok.save_pretrained(tmp_path)
    assert torch.equal(BEASTBsplineTokenizer.from_pretrained(tmp_path, device=str(dev)).encode(xd)[0], tokens)
    with pytest.raises(NotImplementedError):
        tok.encode_at(xd, tok.times)
