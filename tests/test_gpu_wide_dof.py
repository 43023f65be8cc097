"""k_encode_dof and k_reconstruct_dof (csrc/codec_wide_dof.h, 65 <= D <= 256) against the float64
oracle, by the yardsticks of tests/test_gpu_stream_codec.py: params within (T + 8) * 2^-24 * sum_t |P||y|
of the float64 fit (a T-term fp32 chain), tokens bitwise the quantiser of the kernel's own params,
decode bitwise, positions within 1e-5 * max(1, |ref|) of float64 basis @ params.  The DoF counts sit
one past the old limit, on a second block of 64 after one of 65, on a block that holds both kinds, and
at the largest shape (three blocks); the lengths on and off the chunk the library reports."""
import functools

import numpy as np
import pytest
import torch

from beast_tokenizer_amd import BEASTBsplineTokenizer, _lib
from beast_tokenizer_amd.synthetic import synth_trajectories
from oracle import beast_oracle as O

pytestmark = pytest.mark.gpu

F32, TAU, VOCAB, B = np.float32, np.float32(2 * np.pi), 256, 3
DOFS = [(65, ()), (129, ()), (130, (3, 40, 77, 100, 129)), (256, (6, 255))]
# (id, T or a function of the encode chunk, N)
SHAPES = [("t50_n10", 50, 10), ("6tc+21_n10", lambda tc: 6 * tc + 21, 10), ("2tc_n10", lambda tc: 2 * tc, 10),
          ("t50_n17", 50, 17)]
shapes = pytest.mark.parametrize("T,N", [s[1:] for s in SHAPES], ids=[s[0] for s in SHAPES])
dofs = pytest.mark.parametrize("D,grip", DOFS, ids=[f"d{d}_g{len(g)}" for d, g in DOFS])


def _tok(dev, D, N, T, grip, lo=None, hi=None):
    tok = BEASTBsplineTokenizer(num_dof=D, num_basis=N, seq_len=T, vocab_size=VOCAB, gripper_zero_order=bool(grip),
                                gripper_indices=list(grip), device=str(dev))
    if lo is not None:
        tok.load_state_dict({"w_min": lo.tolist(), "w_max": hi.tolist()})
    return tok


@functools.lru_cache(maxsize=None)
def _enc_ref(T, D, N, grip):
    """(x [B,T,D], float64 fit rounded once, bound sums, w_min, w_max inside the fit's range)."""
    x = synth_trajectories(B, T, D, seed=T + D, gripper_indices=grip)
    t, lay = O.times_grid(2 * np.pi, T), O.Layout.make(D, list(grip), bool(grip))
    exact, sums = [], []
    for idx, deg in ((lay.joint_indices, 4), (lay.gripper_indices, 0)):
        if idx:
            phi = O.basis(t, TAU, deg, N)
            exact.append(O.fit_exact(x[..., idx], phi))
            sums.append(np.einsum("nt,btd->bdn", np.abs(O.projection_f64(phi)),
                                  np.abs(x[..., idx].astype(np.float64))).reshape(B, -1))
    exact, sums = np.concatenate(exact, axis=-1), np.concatenate(sums, axis=-1)
    return x, exact, sums, np.quantile(exact, 0.2, axis=0).astype(F32), np.quantile(exact, 0.8, axis=0).astype(F32)


def _chunk(D, grip, N):
    tc = _lib.load().beast_encode_stream_chunk(50, D, D, D - len(grip), N, 1)
    assert tc > 0 and tc % 4 == 0
    return tc


def _mark(family, **fields):
    m = _lib.last_codec_launch()
    assert m.family == family and m.waves == 4 and m.tile == 1, m
    assert all(getattr(m, k) == v for k, v in fields.items()), m


@dofs
@shapes
def test_encode(T, N, D, grip, gpu_device):
    dev, lib = gpu_device, _lib.load()
    T = T(_chunk(D, grip, N)) if callable(T) else T
    x, exact, sums, lo, hi = _enc_ref(T, D, N, grip)
    tok, DN, xd = _tok(dev, D, N, T, grip, lo, hi), D * N, torch.from_numpy(x).to(dev)
    t0, pd0 = tok.encode(xd)
    _mark("encode_dyn", staged=False, fast=True)
    params0 = pd0["params"].cpu().numpy()
    bound = (T + 8) * 2.0 ** -24 * sums + 1e-30
    assert np.all(np.abs(params0 - exact) <= bound), float(np.max(np.abs(params0 - exact) / bound))
    assert torch.equal(t0, tok._quantize(pd0["params"], 0, dev, mode=0)) and (params0 < lo).any() and (params0 > hi).any()
    # alone, and as a strided view of a longer, wider NaN-filled buffer: the same bits
    t1, pd1 = tok.encode(xd[2:].clone())
    assert torch.equal(pd1["params"][0], pd0["params"][2]) and torch.equal(t1[0], t0[2])
    big = torch.full((B, T + 4, D + 2), float("nan"), device=dev)
    big[:, :T, :D] = xd
    t2, pd2 = tok.encode(big[:, :T, :D])
    assert torch.equal(pd2["params"], pd0["params"]) and torch.equal(t2, t0)
    # the gather path: the DoFs permuted over a wider last dim, element stride 2, outputs 4 / 8 bytes
    # past a 16-byte boundary with guards around them
    perm = np.random.default_rng(D).permutation(D + 3)[:D]
    order = tok.joint_indices + tok.gripper_indices
    wide = torch.full((B, T, 2 * (D + 3)), float("nan"), device=dev)
    wide[:, :, 2 * torch.from_numpy(perm).to(dev)] = xd[:, :, order]
    src = torch.from_numpy(perm.astype(np.int32)).to(dev)
    pbuf = torch.full((B * DN + 8,), -7777.0, device=dev)
    tbuf = torch.full((B * DN + 8,), -7777, dtype=torch.int64, device=dev)
    pv, tv, p = pbuf[1:1 + B * DN].view(B, DN), tbuf[1:1 + B * DN].view(B, DN), tok._plan()
    _lib.check(lib.beast_encode_f32(wide.data_ptr(), B, T, wide.stride(0), wide.stride(1), 2, D + 3, D, tok.joint_dof,
                                    src.data_ptr(), p.p_proj, N, p.p_wmn, p.p_wmx, VOCAB, 0, pv.data_ptr(),
                                    tv.data_ptr(), _lib.raw_stream(p.idx)))
    _mark("encode_dyn", staged=False, fast=False)
    assert torch.equal(pv, pd0["params"]) and torch.equal(tv, t0)
    assert all(bool((g == -7777).all()) for g in (pbuf[:1], pbuf[1 + B * DN:], tbuf[:1], tbuf[1 + B * DN:]))


def test_second_item_and_list(gpu_device):
    """More items than the grid holds (a workgroup walks on to a second one), on both kernels; the
    list form and fit_parameters' grouped launches give the per-batch bits."""
    dev, D, T, N = gpu_device, 129, 50, 10
    tok = _tok(dev, D, N, T, ())
    base = torch.from_numpy(synth_trajectories(64, T, D, seed=7)).to(dev)
    loader = [{"actions": base[i:i + 16].clone()} for i in range(0, 64, 16)]
    per_batch = [tok.compute_weights(b["actions"]) for b in loader]
    assert torch.equal(tok._fit_list([b["actions"] for b in loader]), torch.cat(per_batch))
    from beast_tokenizer_amd.bpe_train import no_reduce
    from beast_tokenizer_amd.quantile import column_quantiles
    tok.fit_parameters(loader, verbose=False)
    want = column_quantiles(per_batch, [0.01, 0.99], no_reduce)
    assert torch.equal(tok.w_min, want[0].to(tok.w_min.device)) and torch.equal(tok.w_max, want[1].to(tok.w_max.device))
    tok.encode(base.repeat(64, 1, 1))                       # 8192 items: enough to fill any grid
    Bn = _lib.last_launch_grid() + 3                        # two blocks a trajectory: twice the grid, and a tail
    x = base.repeat(-(-Bn // 64), 1, 1)[:Bn].contiguous()
    tokens, pd = tok.encode(x)
    assert _lib.last_launch_grid() < 2 * Bn
    t_last, pd_last = tok.encode(x[-3:].clone())
    assert torch.equal(pd["params"][-3:], pd_last["params"]) and torch.equal(tokens[-3:], t_last)
    pos = tok.reconstruct_traj(tokens)
    assert _lib.last_launch_grid() < 2 * Bn and torch.equal(pos[-3:], tok.reconstruct_traj(t_last))


@dofs
@pytest.mark.parametrize("N,T,variant", [(10, lambda rc: 50, ""), (10, lambda rc: 2 * rc + 3, "scatter"),
                                         (17, lambda rc: rc + 1, "init_p"), (32, lambda rc: rc, "ntokens")],
                         ids=["n10_t50", "n10_2rc+3_scatter", "n17_rc+1_init_p", "n32_rc_ntokens"])
def test_reconstruct(N, T, variant, D, grip, gpu_device):
    dev, lib = gpu_device, _lib.load()
    lay = O.Layout.make(D, list(grip), bool(grip))
    rng = np.random.default_rng(N * 1000 + D)
    ndo = D + 3 if variant == "scatter" else D
    dst = list(rng.permutation(ndo)[:D]) if variant == "scatter" else lay.order
    rc = lib.beast_reconstruct_stream_rows(50, D, D - len(grip), N, ndo)
    assert rc > 0 and rc % 16 == 0
    T = T(rc)
    lo = rng.uniform(-3, 1, size=D * N).astype(F32)
    hi = (lo + rng.uniform(0.1, 4, size=D * N)).astype(F32)
    tokens = rng.integers(0, VOCAB, size=(B, N * D)).astype(np.int64)
    tokens[0, :4] = (0, VOCAB - 1, VOCAB + 7, -1)          # the vocabulary's ends and tokens outside it
    nt = rng.uniform(-1.2, 1.2, size=(B, N * D)).astype(F32)
    init_p = rng.uniform(-2, 2, size=(B, 2 * D)).astype(F32)
    tok = _tok(dev, D, N, 64, grip, lo, hi)
    times = np.linspace(0, 2 * np.pi, T).astype(F32)
    tokens_t, nt_t, ip_t = (torch.from_numpy(a).to(dev) for a in (tokens, nt, init_p))
    dst_t, p = torch.tensor(dst, dtype=torch.int32, device=dev), tok._plan()
    phi, p_phi, basis_sb, _ = tok._basis_for(torch.from_numpy(times), B, p)   # a shared 1-D grid

    def run(nb):
        pos = torch.full((nb, T, ndo), float("nan"), device=dev)
        ip = ip_t.data_ptr() if variant == "init_p" else None
        _lib.check(lib.beast_reconstruct_f32(
            tokens_t.data_ptr(), nb, D, tok.joint_dof, N, VOCAB, 0, p.p_wmn, p.p_wmx, p_phi, basis_sb, T,
            dst_t.data_ptr(), ndo, ip, 2 * D, p.p_dst if ip else None, None, pos.data_ptr(),
            nt_t.data_ptr() if variant == "ntokens" else None, _lib.raw_stream(p.idx)))
        _mark("reconstruct_mfma", ks=0, staged=True)
        return pos

    want_dec = O.decode(tokens, lay, N, lo, hi, VOCAB)
    assert np.array_equal(tok.decode(tokens_t).cpu().numpy(), want_dec)
    _mark("reconstruct_mfma", ks=0)
    pos_t = run(B)
    assert torch.equal(run(B), pos_t) and torch.equal(run(1)[0], pos_t[0])
    pos, w = pos_t.cpu().numpy(), want_dec.reshape(B, D, N).astype(np.float64)
    if variant == "ntokens":   # denormalize_tensor's intent (beast/utils.py:38-44)
        u = (np.clip(nt.astype(np.float64), -1, 1).reshape(B, N, D).transpose(0, 2, 1) + 1) / 2
        w = u * (hi.astype(np.float64) - lo).reshape(D, N) + lo.reshape(D, N)
    if variant == "init_p":   # coefficient 0 of the joint DoFs <- init_p[:, the DoF's column]
        w[:, :len(lay.joint_indices), 0] = init_p[:, lay.joint_indices]
    want = np.zeros((B, T, ndo))
    pj, pg = (O.basis(times, TAU, deg, N).astype(np.float64) for deg in (4, 0))
    for i in range(D):
        want[:, :, dst[i]] = np.einsum("tn,bn->bt", pj if i < len(lay.joint_indices) else pg, w[:, i])
    err = np.abs(pos - want) / np.maximum(1.0, np.abs(want).max(axis=(1, 2), keepdims=True))
    assert err.max() <= 1e-5, float(err.max())
    assert not pos[:, :, sorted(set(range(ndo)) - set(dst))].any()


def test_api_round_trip(gpu_device, tmp_path):
    dev, D, N, T = gpu_device, 73, 10, 50   # a humanoid: 29 body joints and two hands of 22
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
    cont = tok.reconstruct_traj_continuous(tok.encode_continuous(xd)[0]).cpu().numpy()   # clamped, not quantised
    assert np.all(np.abs(cont - x) <= allowed)
    tok.save_pretrained(tmp_path)
    assert torch.equal(BEASTBsplineTokenizer.from_pretrained(tmp_path, device=str(dev)).encode(xd)[0], tokens)
    with pytest.raises(NotImplementedError, match="num_dof <= 64"):
        tok.reconstruct_traj(tokens, times=tok.times.expand(64, T) + torch.arange(64, device=dev)[:, None] * 1e-3)
