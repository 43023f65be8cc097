"""The second pass of every persistent kernel.

The hot kernels cap their grid at what the chip keeps resident and walk tiles (or rows) in a loop,
re-using an LDS image, constants staged once and tables filled before the loop.  The other test
files reach that loop's second iteration on small devices only; here every batch is sized from the
device's CU count and the kernel's documented cap so that EVERY workgroup (or wave) takes at least
two tiles (items, rows) and the last tile is partial, and the test proves it: right after the
launch it reads ``BEAST_OPT_LAST_LAUNCH_GRID`` and asserts grid <= tiles / 2.  A test that cannot
prove its second pass fails.

Every test compares twice:
  1. bitwise, every output element, with the same entry point called on slices small enough that
     each slice's grid equals its tile count (asserted through the same option), cut at tile
     boundaries: the kernels compute rows independently, so a first-pass result is the reference
     of a later pass;
  2. with the float64 oracle of the kernel's own test file, to that file's tolerance.

Rows of different character (all-zero weights, tokens at both clamp ends and outside the
vocabulary, zero and huge init_p rows, amplitudes that clamp) are drawn per row from a seeded
generator, so the passes of one workgroup differ and a stale image would show.
"""
import numpy as np
import pytest
import torch

from conftest import load_json
from beast_tokenizer_amd import _lib
from beast_tokenizer_amd.bpe_codec import GpuBpeModel, ids_as_i32, rows_from_sequences
from beast_tokenizer_amd.synthetic import synth_trajectories
from oracle import beast_oracle as O
from oracle import bpe_oracle
import deriv_bwd_oracle as DB
import rows_oracle as R
from test_deriv_bwd_oracle import make_inputs
from test_gpu_codec_dispatch import (_assert_close, _c_encode, _dn_to_nd, _expect, _make_tok, _place, _positions_ref,
                                     _set_modes)
from test_gpu_deriv_bwd import launch as bwd_launch
from test_gpu_rows import make_tok as rows_tok, oracle_for as rows_oracle_for

pytestmark = pytest.mark.gpu

F32 = np.float32
EPS = 2.0 ** -24
TWO_PI = 2 * np.pi


def cu_count(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def cdiv(a, b):
    return -(-a // b)


def strided(ntiles, what):
    """The launch just made got at most half as many workgroups as it had tiles: each walked two or more."""
    g = _lib.last_launch_grid()
    assert 0 < g and 2 * g <= ntiles, f"{what}: grid {g} for {ntiles} tiles proves no second pass"
    return g


def one_pass(ntiles, what):
    g = _lib.last_launch_grid()
    assert g == ntiles, f"{what}: a slice of {ntiles} tiles got {g} workgroups"


def cuts(B, step):
    return [(a, min(a + step, B)) for a in range(0, B, step)]


def report(what, dev, **kw):
    print(f"[second pass] {what}: CUs {cu_count(dev)} " + " ".join(f"{k} {v}" for k, v in kw.items()))


def sample_rows(B, tile, grid, stride=61):
    """Rows for an oracle too slow for the batch: the whole first tile, a whole tile of a later pass
    (tile grid + 1: workgroup 1's second), the partial last tile, and every stride-th row."""
    first = np.arange(min(tile, B))
    later = np.arange((grid + 1) * tile, min((grid + 2) * tile, B))
    last = np.arange((cdiv(B, tile) - 1) * tile, B)
    assert later.size == tile and 0 < last.size < tile
    return np.unique(np.concatenate([first, later, last, np.arange(0, B, stride)]))


def dv(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------------------- k_fit_rows --
@pytest.mark.parametrize("grippers", [(), (2,)], ids=["one_kind", "two_kinds"])
def test_fit_rows_second_item(grippers, gpu_device):
    """k_fit_rows: min(ceil(items / 4), 8 CUs) workgroups of 4 waves, an item per wave and pass.
    Items >= 64 CUs + 3, so every wave fits two or more; T = 10 is no multiple of the 4-step chunk;
    [B, T] weights with whole rows of zeros (params exactly 0, NaN inputs never read) and rows that
    lose one sample (NaN there) between full rows; rows of 40x amplitude clamp at both ends."""
    dev = gpu_device
    cus, nk = cu_count(dev), 2 if grippers else 1
    B = cdiv(64 * cus, nk) + 3
    items = B * nk
    T, D, N, degree = 10, 3, 4, 3
    tok = rows_tok(dev, D, N, degree, grippers)
    rng = np.random.default_rng(7 + nk)
    x, t = R.random_walk(B, T, D, 5), R.jittered_times(B, T, TWO_PI, 6)
    w = rng.uniform(0.25, 4.0, (B, T)).astype(F32)
    kind = rng.integers(0, 4, B)
    w[kind == 1] = 0
    lost = np.flatnonzero(kind == 2)
    w[lost, rng.integers(0, T, lost.size)] = 0
    x[kind == 3] *= 40
    x[w == 0] = np.nan
    t[w == 0] = np.nan
    want, cond = rows_oracle_for(tok, x, t, w)
    assert cond.max() <= 1e6, cond.max()                 # every row is held to the criterion
    plain = want[kind == 0]
    lo, hi = np.quantile(plain, 0.05, 0).astype(F32), np.quantile(plain, 0.95, 0).astype(F32)
    tok.load_state_dict({"w_min": lo.tolist(), "w_max": hi.tolist()})
    xd, td, wd = dv(x, dev), dv(t, dev), dv(w, dev)
    tokens, pd = tok.encode_at(xd, td, wd)
    grid = strided(cdiv(items, 4), "k_fit_rows")
    assert items % 4 != 0
    # 1. slices of 16 CUs items: 4 CUs workgroups, an item per wave
    parts = []
    for a, b in cuts(B, 16 * cus // nk):
        tk, p = tok.encode_at(xd[a:b], td[a:b], wd[a:b])
        one_pass(cdiv((b - a) * nk, 4), "k_fit_rows slice")
        parts.append((tk, p["params"]))
    assert torch.equal(tokens, torch.cat([p[0] for p in parts]))
    assert torch.equal(pd["params"], torch.cat([p[1] for p in parts]))
    # 2. the float64 oracle, every row; the quantiser on the kernel's own params
    params = pd["params"].cpu().numpy()
    assert R.parity_ok(params, want).all(), R.parity_err(params, want)
    assert not params[kind == 1].any() and np.isfinite(params).all()
    tk = tokens.cpu().numpy()
    assert np.array_equal(tk, R.tokens(params, lo, hi, 256, D, N))
    assert tk.min() == 0 and tk.max() == 255
    report(f"k_fit_rows kinds {nk}", dev, B=B, items=items, grid=grid, err=f"{R.parity_err(params, want):.3e}",
           tol="1e-5")


# --------------------------------------------------------------------- k_reconstruct_derivs --
def derivs_inputs(B, T, D, nj, N, ndo, per_row, seed, vocab=256):
    """Random tokens, bounds, slabs and init_p of one beast_reconstruct_derivs_f32 call; per row one
    of: random tokens, all 0, all vocab - 1, tokens outside the vocabulary; init_p rows of zeros
    and of 1e3 x among the plain ones."""
    rng = np.random.default_rng([seed, B, T, D, N])
    tok = rng.integers(0, vocab, size=(B, N, D)).astype(np.int64)
    kind = rng.integers(0, 4, B)
    tok[kind == 1] = 0
    tok[kind == 2] = vocab - 1
    tok[kind == 3] = rng.choice(np.array([-3, -1, vocab, vocab + 7, 0, vocab - 1]), size=((kind == 3).sum(), N, D))
    lo = (-rng.uniform(0.5, 2.0, (D, N))).astype(F32)
    hi = (lo + rng.uniform(0.5, 3.0, (D, N)).astype(F32)).astype(F32)
    slabs = rng.standard_normal(((B,) if per_row else ()) + (3, 2, T, N)).astype(F32)
    ip = rng.standard_normal((B, D + 3)).astype(F32)
    ip[kind == 1] = 0
    ip[kind == 2] *= F32(1e3)
    return dict(tok=tok, lo=lo, hi=hi, slabs=slabs, ip=ip, dst=rng.permutation(ndo)[:D].astype(np.int32),
                ip_src=rng.permutation(D + 3)[:D].astype(np.int32), B=B, T=T, D=D, nj=nj, N=N, ndo=ndo,
                per_row=per_row, vocab=vocab)


def derivs_oracle(c):
    """(want, mag) [3, B, T, ndo] float64: the sum of the same products, and of their magnitudes;
    the fp32 params formed op by op as the kernel forms them (beast/utils.py:20-25), init_p on."""
    B, T, D, nj, N, ndo, vocab = (c[k] for k in ("B", "T", "D", "nj", "N", "ndo", "vocab"))
    lo, hi = c["lo"], c["hi"]
    w = np.clip(((c["tok"].astype(F32) / F32(vocab - 1)) * (hi.T - lo.T)).astype(F32) + lo.T, lo.T, hi.T)
    w = np.ascontiguousarray(w.astype(F32).transpose(0, 2, 1))                    # [B, D, N]
    w[:, :nj, 0] = c["ip"][:, c["ip_src"][:nj]]
    want, mag = np.zeros((3, B, T, ndo)), np.zeros((3, B, T, ndo))
    for o in range(3):
        for d in range(D):
            kd = 0 if d < nj else 1
            if o and kd:
                continue
            ph = c["slabs"][..., o, kd, :, :].astype(np.float64)
            wd = w[:, d, :].astype(np.float64)
            sub = "tn,bn->bt" if ph.ndim == 2 else "btn,bn->bt"
            want[o, :, :, c["dst"][d]] = np.einsum(sub, ph, wd)
            mag[o, :, :, c["dst"][d]] = np.einsum(sub, np.abs(ph), np.abs(wd))
    return want, mag


def derivs_run(c, d, a, b):
    """beast_reconstruct_derivs_f32 on rows [a, b) of the device copies d: three [b - a, T, ndo] outputs."""
    T, D, N, ndo = c["T"], c["D"], c["N"], c["ndo"]
    outs = [torch.full((b - a, T, ndo), float("nan"), dtype=torch.float32, device=d["tok"].device) for _ in range(3)]
    sb = 3 * 2 * T * N if c["per_row"] else 0
    basis = d["slabs"][a:b] if c["per_row"] else d["slabs"]
    _lib.run("beast_reconstruct_derivs_f32", d["tok"][a:b].data_ptr(), b - a, D, c["nj"], N, c["vocab"], 0,
             d["lo"].data_ptr(), d["hi"].data_ptr(), basis.data_ptr(), sb, T, d["dst"].data_ptr(), ndo,
             d["ip"][a:b].data_ptr(), D + 3, d["ip_src"].data_ptr(), *(o.data_ptr() for o in outs), None, None)
    return outs


def derivs_check(dev, c, tile, slice_rows, what):
    cus, B = cu_count(dev), c["B"]
    d = {k: dv(c[k], dev) for k in ("tok", "lo", "hi", "slabs", "ip", "dst", "ip_src")}
    full = derivs_run(c, d, 0, B)
    ntiles = cdiv(B, tile)
    grid = strided(ntiles, what)
    assert B % tile != 0
    parts = []
    for a, b in cuts(B, slice_rows):
        parts.append(derivs_run(c, d, a, b))
        one_pass(cdiv(b - a, 16 if cdiv(b - a, 16) >= 2 * cus else 4), what + " slice")
    want, mag = derivs_oracle(c)
    worst = 0.0
    for o in range(3):
        assert torch.equal(full[o], torch.cat([p[o] for p in parts])), o
        got = full[o].cpu().numpy().astype(np.float64)
        assert not np.isnan(got).any()
        err, tol = np.abs(got - want[o]), (c["N"] + 1) * EPS * mag[o]
        assert (err <= tol).all(), (what, o, float((err - tol).max()))
        assert not got[mag[o] == 0].any()
        worst = max(worst, float((err[tol > 0] / tol[tol > 0]).max()))
    report(what, dev, B=B, tiles=ntiles, grid=grid, worst_err_over_bound=f"{worst:.3f}", bound="(N+1) 2^-24 sum|basis w|")


@pytest.mark.parametrize("per_row", [False, True], ids=["lds_slabs", "per_row_slabs"])
def test_derivs_bulk_tiles_stride(per_row, gpu_device):
    """k_reconstruct_derivs, tiles of 16 on at most 8 workgroups per CU: 16 CUs + 1 tiles, 5 rows in
    the last; rows of T * ndo = 9 floats (element stores).  Slices of 4 CUs tiles stay bulk."""
    cus = cu_count(gpu_device)
    c = derivs_inputs(16 * 16 * cus + 5, 3, 2, 1, 5, 3, per_row, seed=11)
    derivs_check(gpu_device, c, 16, 16 * 4 * cus, f"k_reconstruct_derivs bulk per_row={per_row}")


def test_derivs_latency_tiles_stride(gpu_device):
    """The 4-trajectory tile strides only when fewer than 8 workgroups fit a CU: T_out 170 at N 13
    stages 4 * 170 * 16 floats of slabs (42.5 KB: at most 3 workgroups per CU), and B = 32 CUs - 17
    is the largest batch of the latency regime with a partial last tile: 8 CUs - 4 tiles on at
    most 3 CUs workgroups.  init_p on, num_dof_out 4 > D 3."""
    cus = cu_count(gpu_device)
    c = derivs_inputs(32 * cus - 17, 170, 3, 2, 13, 4, False, seed=12)
    derivs_check(gpu_device, c, 4, 4 * cus, "k_reconstruct_derivs latency")


# ----------------------------------------------------------------- k_reconstruct_derivs_bwd --
def bwd_inputs(B, T, D, nj, N, ndo, per_row):
    """make_inputs, then per row one of: as drawn, every x outside the clamp (an all-masked row:
    exact zeros), every x exactly +-1, NaN in half the row."""
    c = make_inputs(B, T, D, nj, N, (0, 1, 2), ndo=ndo, per_row=per_row, seed=3)
    rng = np.random.default_rng([B, T, D, N])
    kind = rng.integers(0, 4, B)
    x = c["x"]
    x[kind == 1] = F32(1.5)
    x[kind == 2] = np.where(rng.random(((kind == 2).sum(), N, D)) < 0.5, F32(1), F32(-1))
    half = x[kind == 3]
    half[:, ::2] = np.nan
    x[kind == 3] = half
    return c, kind


def bwd_check(dev, c, kind, tile, slice_rows, what):
    B, D, nj = c["x"].shape[0], c["x"].shape[2], c["nj"]
    per_row = c["basis"].ndim == 5
    got, got_ip = bwd_launch(dev, c, init_p=True)
    ntiles = cdiv(B, tile)
    grid = strided(ntiles, what)
    assert B % tile != 0
    parts = []
    for a, b in cuts(B, slice_rows):
        one = dict(c, x=c["x"][a:b], grads=[g[a:b] for g in c["grads"]], basis=c["basis"][a:b] if per_row else c["basis"])
        parts.append(bwd_launch(dev, one, init_p=True))
        one_pass(cdiv(b - a, tile if b - a >= slice_rows else 4), what + " slice")
    assert np.array_equal(got, np.concatenate([p[0] for p in parts]), equal_nan=True)
    assert np.array_equal(got_ip, np.concatenate([p[1] for p in parts]))
    r = DB.backward(c["grads"], c["basis"], c["lo"], c["hi"], c["x"], c["dst"], nj, init_p_src=c["ip_src"],
                    init_p_width=D + 3)
    tol = DB.bound(r)
    err = np.abs(got.astype(np.float64) - r.grad_ntokens)
    assert not np.isnan(got).any()
    assert (err <= tol).all(), (what, float((err - tol).max()))
    assert not got[r.grad_ntokens == 0].any() and not got[kind == 1].any()
    src = c["ip_src"]
    tol_ip = r.terms * DB.EPS * r.mag[:, :nj, 0]
    assert (np.abs(got_ip[:, src[:nj]] - r.grad_init_p[:, src[:nj]]) <= tol_ip).all()
    assert got_ip[kind == 1][:, src[:nj]].any()          # a masked row still feeds grad_init_p
    worst = float((err[tol > 0] / tol[tol > 0]).max())
    report(what, dev, B=B, tiles=ntiles, grid=grid, worst_err_over_bound=f"{worst:.3f}",
           bound="(K+3) 2^-24 s sum|basis G|")


@pytest.mark.parametrize("per_row", [False, True], ids=["lds_slabs", "per_row_slabs"])
def test_derivs_bwd_bulk_tiles_stride(per_row, gpu_device):
    """k_reconstruct_derivs_bwd, tiles of 16 on at most 8 workgroups per CU (fewer where registers
    say so): 16 CUs + 1 tiles, 5 rows in the last.  Slices of 2 CUs tiles are the smallest bulk ones."""
    cus = cu_count(gpu_device)
    c, kind = bwd_inputs(16 * 16 * cus + 5, 3, 2, 1, 5, 3, per_row)
    bwd_check(gpu_device, c, kind, 16, 16 * 2 * cus, f"k_reconstruct_derivs_bwd bulk per_row={per_row}")


def test_derivs_bwd_latency_tiles_stride(gpu_device):
    """The 4-trajectory tile with 42.5 KB of staged slabs beside the 24 KB gradient chunk: at most 2
    workgroups per CU for 8 CUs - 4 tiles (B = 32 CUs - 17).  The chunk holds 128 of the 170 time
    steps, so every tile also walks two chunks."""
    cus = cu_count(gpu_device)
    c, kind = bwd_inputs(32 * cus - 17, 170, 3, 2, 13, 4, False)
    bwd_check(gpu_device, c, kind, 4, 4 * cus, "k_reconstruct_derivs_bwd latency")


# --------------------------------------------------------------------------------- k_encode --
RT_ENC = dict(T=8, D=3, N=4, degree=3)            # T * D = 24: the contiguous rows take the DMA path
ENC_CASES = {
    # name: (shape, layout, forced waves, trajectories per CU that double the cap, expected launch)
    "dma": (RT_ENC, "contig", 0, 8 * 32, dict(family="encode_dyn", tile=8, waves=4, fast=True)),
    "gather": (RT_ENC, "col_slice", 0, 8 * 32, dict(family="encode_dyn", tile=8, waves=4, fast=False)),
    # the 14-DoF images leave room for 4 workgroups of 4 waves per CU (cap 8 CUs), 2 of 7 waves
    "spec_4_waves": (dict(T=50, D=14, N=10, grip=[6, 13]), "contig", 4, 8 * 16,
                     dict(family="encode_spec", tile=8, waves=4, fast=True)),
    "spec_4_waves_k2": (dict(T=50, D=14, N=10), "contig", 4, 8 * 16, dict(family="encode_spec", tile=8, waves=4, fast=True)),
    "spec_7_waves": (dict(T=50, D=14, N=10), "contig", 7, 8 * 16, dict(family="encode_spec", tile=8, waves=7, fast=True)),
}
_ENC = {}


def enc_ref(name, dev):
    """(x, amplitude kind per row, lo, hi, layout, B) of a case, shared by its two output variants."""
    if name not in _ENC:
        shape, _, _, per_cu, _ = ENC_CASES[name]
        T, D, grip = shape["T"], shape["D"], shape.get("grip")
        B = per_cu * cu_count(dev) + 3
        base = synth_trajectories(1024, T, D, seed=100 + T + D, gripper_indices=grip or ())
        rng = np.random.default_rng(T * D)
        kind = rng.integers(0, 4, B)
        scale = np.array([1, 0, 25, 0.3], dtype=F32)[kind]               # plain, all zero, clamping, small
        x = base[rng.integers(0, 1024, B)] * scale[:, None, None]
        lay = O.Layout.make(D, grip, bool(grip))
        ex = enc_exact(base, lay, shape)[0]
        lo, hi = np.quantile(ex, 0.05, axis=0).astype(F32), np.quantile(ex, 0.95, axis=0).astype(F32)
        _ENC[name] = (x, kind, lo, hi, lay, B)
    return _ENC[name]


def enc_exact(x, lay, shape):
    """test_gpu_codec_dispatch's reference: the float64 fit rounded once and its bound sums."""
    t = O.times_grid(2 * np.pi, shape["T"])
    exact, sums = [], []
    for idx, deg in ((lay.joint_indices, shape.get("degree", 4)), (lay.gripper_indices, 0)):
        if idx:
            phi = O.basis(t, F32(2 * np.pi), deg, shape["N"])
            y = x[..., idx]
            exact.append(O.fit_exact(y, phi))
            sums.append(np.einsum("nt,btd->bdn", np.abs(O.projection_f64(phi)), np.abs(y.astype(np.float64)))
                        .reshape(len(x), -1))
    return np.concatenate(exact, axis=-1), np.concatenate(sums, axis=-1)


@pytest.mark.parametrize("outputs", ["tokens_and_params", "tokens_only"])
@pytest.mark.parametrize("name", list(ENC_CASES))
def test_encode_second_tile(name, outputs, gpu_device):
    """k_encode walks tiles of 8 on at most 2 x (workgroups per CU by LDS, <= 8) x CUs workgroups.
    The batch is twice that cap in tiles plus 3 trajectories; rows are plain, all zero, 25x (both
    clamps) or 0.3x.  Slices of 2 CUs tiles never reach the cap."""
    dev = gpu_device
    shape, layout, waves, _, expect = ENC_CASES[name]
    T, D, N = shape["T"], shape["D"], shape["N"]
    x, kind, lo, hi, lay, B = enc_ref(name, dev)
    cus, DN = cu_count(dev), D * N
    tok = _make_tok(dev, D, N, T, 256, shape.get("degree", 4), shape.get("grip"), lo, hi)
    view, ptr, strides, row_elems, keep = _place(x, layout, dev)
    both = outputs == "tokens_and_params"

    def run(a, b, want_params):
        params = torch.full((b - a, DN), float("nan"), device=dev) if want_params else None
        tokens = torch.full((b - a, DN), -7777, dtype=torch.int64, device=dev)
        _c_encode(tok, view[a:b].data_ptr(), b - a, T, strides, row_elems, params, tokens)
        _expect(**expect)
        return params, tokens

    _set_modes(waves=waves)
    try:
        params, tokens = run(0, B, both)
        grid = strided(cdiv(B, 8), f"k_encode {name}")
        assert B % 8 != 0
        parts = []
        for a, b in cuts(B, 8 * 2 * cus):
            parts.append(run(a, b, both))
            one_pass(cdiv(b - a, 8), f"k_encode {name} slice")
        if not both:                                     # the params these tokens quantise
            params = run(0, B, True)[0]
    finally:
        _set_modes()
    assert torch.equal(tokens, torch.cat([p[1] for p in parts]))
    if both:
        assert torch.equal(params, torch.cat([p[0] for p in parts]))
    # the float64 fit on a sample of whole tiles; the quantiser on the kernel's own params, every row
    rows = sample_rows(B, 8, grid)
    exact, sums = enc_exact(x[rows], lay, shape)
    pn, tn = params.cpu().numpy(), tokens.cpu().numpy()
    bound = (cdiv(T, 4) * 4 + 8) * EPS * sums + 1e-30
    err = np.abs(pn[rows] - exact)
    assert np.all(err <= bound), float(np.max(err / bound))
    assert not pn[kind == 1].any()
    assert (pn < lo).any() and (pn > hi).any()
    want = _dn_to_nd(O.continuous_to_discrete(O._clamp_t(pn, lo, hi), lo, hi, 256), B, D, N)
    assert np.array_equal(tn, want) and want.min() == 0 and want.max() == 255
    report(f"k_encode {name} {outputs}", dev, B=B, tiles=cdiv(B, 8), grid=grid,
           worst_err_over_bound=f"{float(np.max(err / bound)):.3f}", bound="(Tp+8) 2^-24 sum|P||y|", oracle_rows=rows.size)


# ------------------------------------------------------- k_reconstruct, k_reconstruct_rows --
REC_CASES = {
    # name: (D, N, T_out, degree, grippers, dof_dst, num_dof_out, per-row times, forced waves,
    #        trajectories per CU that double the cap, expected launch)
    "regs_basis": (3, 5, 9, 3, None, [3, 0, 2], 4, False, 0, 8 * 32,
                   dict(family="reconstruct_mfma", tile=8, waves=4, ks=2, basis_regs=True)),
    "lds_basis": (3, 5, 65, 3, None, [3, 0, 2], 4, False, 0, 8 * 32,
                  dict(family="reconstruct_mfma", tile=8, waves=4, ks=2, basis_regs=False)),
    # the 14-DoF images: 44 KB and more, at most 3 workgroups per CU (cap 6 CUs)
    "spec_4_waves": (14, 10, 50, 4, [6, 13], None, 14, False, 4, 8 * 16,
                     dict(family="reconstruct_spec", tile=8, waves=4, ks=3, basis_regs=True)),
    "spec_4_waves_k2": (14, 10, 50, 4, None, None, 14, False, 4, 8 * 16,
                        dict(family="reconstruct_spec", tile=8, waves=4, ks=3, basis_regs=True)),
    "spec_7_waves": (14, 10, 50, 4, None, None, 14, False, 7, 8 * 16,
                     dict(family="reconstruct_spec", tile=8, waves=7, ks=3, basis_regs=True)),
    "rows_per_row_times": (3, 5, 5, 3, [1], [3, 0, 2], 4, True, 0, 8 * 32,
                           dict(family="reconstruct_rows", tile=8, waves=4, ks=0)),
}


@pytest.mark.parametrize("name", list(REC_CASES))
def test_reconstruct_second_tile(name, gpu_device):
    """k_reconstruct / k_reconstruct_rows walk tiles of 8 under the same cap as k_encode.  Positions
    and params_out from one launch, init_p on (rows of zeros and of 1e3 x), token rows of all 0, all
    vocab - 1 and outside the vocabulary among random ones; the runtime shapes scatter 3 DoFs
    into 4 output columns."""
    dev = gpu_device
    D, N, T, degree, grip, dst, ndo, per_row, waves, per_cu, expect = REC_CASES[name]
    cus, vocab = cu_count(dev), 256
    B = per_cu * cus + 3
    rng = np.random.default_rng(D * 1000 + N * 10 + T)
    lo = rng.uniform(-3, 1, size=D * N).astype(F32)
    hi = (lo + rng.uniform(0.1, 4, size=D * N)).astype(F32)
    tokens = rng.integers(0, vocab, size=(B, N * D)).astype(np.int64)
    kind = rng.integers(0, 4, B)
    tokens[kind == 1] = 0
    tokens[kind == 2] = vocab - 1
    tokens[kind == 3] = rng.choice(np.array([-3, -1, vocab, vocab + 7, 0, vocab - 1]), size=((kind == 3).sum(), N * D))
    init_p = rng.uniform(-2, 2, size=(B, 2 * D)).astype(F32)
    init_p[kind == 1] = 0
    init_p[kind == 2] *= F32(1e3)
    lay = O.Layout.make(D, grip, bool(grip))
    dst = dst or lay.order
    tok = _make_tok(dev, D, N, 50, vocab, degree, grip, lo, hi)
    if per_row:
        times = np.sort(rng.uniform(0, 2 * np.pi, size=(B, T)), axis=1).astype(F32)
    else:
        times = O.times_grid(2 * np.pi, T) if T == 50 else np.linspace(0, 2 * np.pi, T).astype(F32)
    p = tok._plan()
    phi, p_phi, basis_sb, Tn = tok._basis_for(torch.from_numpy(times), B, p)
    assert Tn == T and (basis_sb != 0) == per_row
    tk_d, ip_d = dv(tokens, dev), dv(init_p, dev)
    dst_t = torch.tensor(dst, dtype=torch.int32, device=dev)
    lib = _lib.load()

    def run(a, b):
        pos = torch.full((b - a, T, ndo), float("nan"), device=dev)
        par = torch.full((b - a, D * N), float("nan"), device=dev)
        rc = lib.beast_reconstruct_f32(tk_d[a:b].data_ptr(), b - a, D, tok.joint_dof, N, vocab, 0, p.p_wmn, p.p_wmx,
                                       p_phi + 4 * a * basis_sb, basis_sb, T, dst_t.data_ptr(), ndo,
                                       ip_d[a:b].data_ptr(), 2 * D, p.p_dst, par.data_ptr(), pos.data_ptr(), None,
                                       _lib.raw_stream(p.idx))
        _lib.check(rc, "beast_reconstruct_f32")
        _expect(**expect)
        return pos, par

    _set_modes(waves=waves)
    try:
        pos, par = run(0, B)
        grid = strided(cdiv(B, 8), f"reconstruct {name}")
        assert B % 8 != 0
        parts = []
        for a, b in cuts(B, 8 * 2 * cus):
            parts.append(run(a, b))
            one_pass(cdiv(b - a, 8), f"reconstruct {name} slice")
    finally:
        _set_modes()
    assert torch.equal(pos, torch.cat([q[0] for q in parts])) and torch.equal(par, torch.cat([q[1] for q in parts]))
    want_dec = O.decode(tokens, lay, N, lo, hi, vocab)
    assert np.array_equal(par.cpu().numpy(), want_dec)                   # params_out: the plain decode, bit for bit
    rows = sample_rows(B, 8, grid, stride=31)
    w = want_dec.reshape(B, D, N)[rows].copy()
    for i, col in enumerate(lay.joint_indices):
        w[:, i, 0] = init_p[rows, col]
    got = pos.cpu().numpy()
    ref = _positions_ref(w, lay, times[rows] if per_row else times, degree, N, dst, ndo)
    _assert_close(got[rows], ref)
    unnamed = sorted(set(range(ndo)) - set(dst))
    assert not got[:, :, unnamed].any() and not np.isnan(got).any()
    scale = np.maximum(1.0, np.abs(ref).max(axis=(1, 2), keepdims=True))
    report(f"reconstruct {name}", dev, B=B, tiles=cdiv(B, 8), grid=grid,
           err=f"{float((np.abs(got[rows] - ref) / scale).max()):.3e}", tol="1e-5", oracle_rows=rows.size)


# ------------------------------------------------------------------------------- k_quantize --
@pytest.mark.parametrize("mode", [0, 1], ids=["tokens", "normalised"])
def test_quantize_second_pass(mode, gpu_device):
    """k_quantize: at most 4,096 workgroups of 256 elements.  B * 15 elements fill 8,204 blocks (the
    last one 77 elements), so every thread takes two or three; the oracle quantiser bit for bit."""
    dev = gpu_device
    D, N, B = 3, 5, 140003
    tok = _make_tok(dev, D, N, 50, 256, 4, None, np.full(D * N, -1, F32), np.full(D * N, 1, F32))
    rng = np.random.default_rng(mode)
    lo = rng.uniform(-3, 1, size=D * N).astype(F32)
    hi = (lo + rng.uniform(0.1, 4, size=D * N)).astype(F32)
    tok.load_state_dict({"w_min": lo.tolist(), "w_max": hi.tolist()})
    p = rng.uniform(-4, 6, size=(B, D * N)).astype(F32)
    kind = rng.integers(0, 4, B)
    p[kind == 1] = lo                                                    # both clamp ends, exactly
    p[kind == 2] = hi
    p[kind == 3] *= F32(100)
    pd_ = dv(p, dev)
    out = tok._quantize(pd_, 0, dev, mode)
    total = B * D * N
    grid = strided(cdiv(total, 256), "k_quantize")
    assert grid == 4096 and total % 256 != 0
    parts = []
    for a, b in cuts(B, 4096 * 256 // (2 * D * N)):
        parts.append(tok._quantize(pd_[a:b], 0, dev, mode))
        one_pass(cdiv((b - a) * D * N, 256), "k_quantize slice")
    assert torch.equal(out, torch.cat(parts))
    c = O._clamp_t(p, lo, hi)
    if mode == 0:
        want = O.continuous_to_discrete(c, lo, hi, 256)
    else:   # normalize_tensor (beast/utils.py:29-35) in fp32, op by op
        want = (((c - lo) / np.maximum(hi - lo, F32(1e-8))).astype(F32) * F32(2) + F32(-1)).astype(F32)
    assert np.array_equal(out.cpu().numpy(), _dn_to_nd(want, B, D, N))
    report(f"k_quantize mode {mode}", dev, B=B, tiles=cdiv(total, 256), grid=grid, err="bit-exact")


# ------------------------------------------------------------- k_bpe_encode, k_bpe_decode --
CODEC = load_json("bpe_codec.json")
HF = load_json("bpe_hf.json")


def test_bpe_rows_second_pass(gpu_device):
    """k_bpe_encode (per-row mode): a wave per row, at most 16 waves per workgroup and 2 such
    workgroups per CU; k_bpe_decode: 4 waves on at most 4 workgroups per CU.  64 CUs + 7 ragged
    rows (empty, one symbol, up to 60) of a golden model give every wave of either kernel two
    rows or more; the ids of the encode are what the decode reads."""
    from tokenizers import ByteLevelBPETokenizer
    from beast_tokenizer_amd.bpe_codec import set_encode_path
    dev = gpu_device
    cus = cu_count(dev)
    ref = HF[CODEC["traj_k2/2048"]["model"]["ref"]]
    hf = ByteLevelBPETokenizer(vocab=ref["vocab"], merges=[tuple(m) for m in ref["merges"]])
    model = GpuBpeModel(hf, dev)
    oracle = bpe_oracle.BpeModel(ref["vocab"], ref["merges"])
    pool = [np.asarray(cps, dtype=np.int64) for cps, _ in CODEC["traj_k2/2048"]["encode"] if len(cps) >= 60]
    rng = np.random.default_rng(9)
    n_rows = 64 * cus + 7
    lens = rng.integers(2, 61, n_rows)
    kind = rng.integers(0, 4, n_rows)
    lens[kind == 1] = 0
    lens[kind == 2] = 1
    src = rng.integers(0, len(pool), n_rows)
    rows = [pool[s][o:o + n] for s, o, n in zip(src, rng.integers(0, 60, n_rows) % (60 - lens + 1), lens)]
    flat, off, width = rows_from_sequences(rows, dev)
    off_h = off.cpu().numpy()
    assert width == 60
    set_encode_path("rows")
    try:
        ids, elens, status = model.encode_rows(flat, off, width, 0, None)
        # 16 waves per workgroup at most, so grid * 16 bounds the rows of one pass
        grid_e = _lib.last_launch_grid()
        assert 0 < grid_e and 2 * 16 * grid_e <= n_rows, f"k_bpe_encode: grid {grid_e} for {n_rows} rows"
        assert not status.any()
        # rows this short leave the LDS to 16 rows a workgroup: a launch of 16 rows is one workgroup
        one = model.encode_rows(flat[:off_h[16]], off[:17], width, 0, None)
        one_pass(1, "k_bpe_encode, 16 rows")
        parts = []
        for a, b in cuts(n_rows, 16 * cus):
            parts.append(model.encode_rows(flat[off_h[a]:off_h[b]], off[a:b + 1] - off_h[a], width, 0, None))
            one_pass(cdiv(b - a, 16), "k_bpe_encode slice")
    finally:
        set_encode_path("auto")
    ids_h, lens_h = ids.cpu().numpy(), elens.cpu().numpy()
    pi, pl = np.concatenate([q[0].cpu().numpy() for q in parts]), np.concatenate([q[1].cpu().numpy() for q in parts])
    assert np.array_equal(lens_h, pl) and np.array_equal(one[1].cpu().numpy(), lens_h[:16])
    valid = np.arange(ids_h.shape[1])[None, :] < lens_h[:, None]
    assert np.array_equal(np.where(valid, ids_h, -1), np.where(valid, pi, -1))
    got = [ids_h[i, :lens_h[i]].tolist() for i in range(n_rows)]
    sample = sample_rows(n_rows, 16, grid_e, stride=37)
    for i in sample:
        assert got[i] == oracle.encode("".join(map(chr, rows[i]))), i
    # ---- decode: the ids just made, ragged; L = 60 code points
    seqs = [ids_as_i32(np.asarray(g, dtype=np.int64)).reshape(-1) for g in got]
    dflat, doff, _ = rows_from_sequences(seqs, dev, dtype=np.int32)
    doff_h = doff.cpu().numpy()
    out, counts, dstat = model.decode_rows(dflat, doff, 60, 0)
    grid_d = strided(cdiv(n_rows, 4), "k_bpe_decode")
    assert n_rows % 4 != 0 and grid_d <= 4 * cus
    dparts = []
    for a, b in cuts(n_rows, 8 * cus):
        dparts.append(model.decode_rows(dflat[doff_h[a]:doff_h[b]], doff[a:b + 1] - doff_h[a], 60, 0))
        one_pass(cdiv(b - a, 4), "k_bpe_decode slice")
    out_h, cnt_h = out.cpu().numpy(), counts.cpu().numpy()
    assert np.array_equal(cnt_h, np.concatenate([q[1].cpu().numpy() for q in dparts])) and not dstat.any()
    po = np.concatenate([q[0].cpu().numpy() for q in dparts])
    valid = np.arange(60)[None, :] < cnt_h[:, None]
    assert np.array_equal(np.where(valid, out_h, -1), np.where(valid, po, -1))
    assert np.array_equal(cnt_h, lens)
    for i in range(n_rows):                                              # the round trip, every row
        assert np.array_equal(out_h[i, :cnt_h[i]], rows[i]), i
    for i in sample:
        assert [ord(ch) for ch in oracle.decode(got[i])] == out_h[i, :cnt_h[i]].tolist(), i
    report("k_bpe_encode / k_bpe_decode", dev, rows=n_rows, grid_encode=grid_e, grid_decode=grid_d,
           err="bit-exact", oracle_rows=sample.size)
