"""Every encode / reconstruct launch branch of csrc/codec.hip against the float64 oracle.

``launch_encode`` / ``launch_reconstruct`` (csrc/codec.hip; the kernels themselves are in
csrc/codec_encode.h and csrc/codec_reconstruct.h, the launch path in csrc/launch.h) choose among about twenty kernel instantiations by batch
size against the CU count, contiguity, 16-byte alignment of inputs and outputs, T * row_elems, N,
T_out, the LDS footprint and whether the basis is shared.  Each row of the two tables below names a
shape, the way to reach one branch and the fields of ``BEAST_OPT_LAST_CODEC_LAUNCH`` that branch
must report; the row fails if the launch took another branch (a threshold moved, a partitioned
card) as well as if the values are wrong.

Contracts (the project's existing ones):
  * params: |gpu - fit_exact| <= (Tp + 8) * 2^-24 * sum_t |P[n,t]| |y[t]| + 1e-30, Tp = round_up(T, 4);
  * tokens: bit-equal to continuous_to_discrete(clamp(params_gpu)) on the kernel's own params;
  * decode: bit-equal to the oracle's decode;
  * positions: <= 1e-5 * max(1, |ref|_inf per trajectory) of the float64 basis @ decoded params;
  * layout variants of one computation (misaligned outputs, strided inputs, C-ABI against the
    Python API) are bitwise equal to the aligned, contiguous result.
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
CLAMP = 0.05          # bounds at the 5 % / 95 % quantiles of the exact fit: params clamp on both sides


def _batch(B, dev):
    """Batch sizes relative to the latency / bulk threshold of the per-trajectory kernels."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    return {"16cu+11": 16 * cus + 11, "16cu": 16 * cus}.get(B, B)


def _dn_to_nd(t, B, D, N):
    return t.reshape(B, D, N).transpose(0, 2, 1).reshape(B, N * D)


def _expect(**fields):
    m = _lib.last_codec_launch()
    got = {k: getattr(m, k) for k in fields}
    assert got == fields, f"launch took another branch: {m}"


def _set_modes(generic=0, waves=0):
    lib = _lib.load()
    assert lib.beast_set_option(_lib.OPT_GENERIC_KERNELS, generic) == 0
    assert lib.beast_set_option(_lib.OPT_BLOCK_WAVES, waves) == 0


def _make_tok(dev, D, N, T, vocab, degree, grip, lo, hi):
    tok = BEASTBsplineTokenizer(num_dof=D, num_basis=N, seq_len=T, vocab_size=vocab, degree_p=degree,
                                gripper_zero_order=bool(grip), gripper_indices=grip, device=str(dev))
    tok.load_state_dict({"w_min": lo.tolist(), "w_max": hi.tolist()})
    return tok


def _shifted(dev, rows, cols, dtype, shift):
    """A [rows, cols] output whose first element lies `shift` elements past a 16-byte boundary,
    inside a sentinel-filled buffer: (buffer, view)."""
    buf = torch.full((rows * cols + 8,), -7777, dtype=dtype, device=dev)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[shift:shift + rows * cols].view(rows, cols)


def _guards_intact(buf, shift, n):
    g = torch.cat([buf[:shift], buf[shift + n:]]).cpu().numpy()
    return bool(np.all(g == -7777))


# ------------------------------------------------------------------------------------- encode --
_ENC_REF = {}


def _enc_ref(T, D, N, B, degree, grip):
    """(x [B,T,D], float64 fit rounded once [B, D*N], bound sums, w_min, w_max, layout), shared."""
    key = (T, D, N, B, degree, tuple(grip or ()))
    if key not in _ENC_REF:
        x = synth_trajectories(B, T, D, seed=100 + T + D, gripper_indices=grip or ())
        t = O.times_grid(2 * np.pi, T)
        lay = O.Layout.make(D, grip, bool(grip))
        exact, sums = [], []
        for idx, deg in ((lay.joint_indices, degree), (lay.gripper_indices, 0)):
            if idx:
                phi = O.basis(t, TAU, deg, N)
                y = x[..., idx]
                exact.append(O.fit_exact(y, phi))
                sums.append(np.einsum("nt,btd->bdn", np.abs(O.projection_f64(phi)),
                                      np.abs(y.astype(np.float64))).reshape(B, -1))
        exact, sums = np.concatenate(exact, axis=-1), np.concatenate(sums, axis=-1)
        lo = np.quantile(exact, CLAMP, axis=0).astype(F32)
        hi = np.quantile(exact, 1 - CLAMP, axis=0).astype(F32)
        for a in (exact, sums, lo, hi):   # shared among the rows: never modified
            a.setflags(write=False)
        _ENC_REF[key] = (x, exact, sums, lo, hi, lay)
    return _ENC_REF[key]


def _place(x, layout, dev):
    """The trajectories in device memory under `layout`: (tensor view [B,T,Din] or None, pointer,
    (sb, st, sd), row_elems, keepalive).  Memory the view does not cover holds NaN."""
    B, T, D = x.shape
    xd = torch.from_numpy(x).to(dev)
    nan = float("nan")
    if layout == "contig":
        v = xd
    elif layout == "col_slice":        # rows of D + 1 floats, the last column sliced off
        big = torch.full((B, T, D + 1), nan, device=dev)
        big[..., :D] = xd
        v = big[..., :D]
    elif layout == "time_slice":       # trajectories of T + 3 steps, the tail sliced off
        big = torch.full((B, T + 3, D), nan, device=dev)
        big[:, :T] = xd
        v = big[:, :T]
    elif layout == "base4":            # contiguous rows, the base pointer 4 bytes past a 16-byte boundary
        big = torch.full((B * T * D + 4,), nan, device=dev)
        v = big[1:1 + B * T * D].view(B, T, D)
        v.copy_(xd)
        assert v.data_ptr() % 16 == 4
    elif layout == "wide":             # rows of D + 2 floats, read in place (row_elems > D)
        v = torch.full((B, T, D + 2), nan, device=dev)
        v[..., :D] = xd
    elif layout == "dt":               # [B, D, T] storage: element stride T between the DoFs
        big = xd.transpose(1, 2).contiguous()
        return None, big.data_ptr(), (D * T, 1, T), D, big
    else:
        raise KeyError(layout)
    return v, v.data_ptr(), v.stride(), v.shape[2], v


def _c_encode(tok, ptr, B, T, strides, row_elems, params, tokens):
    p = tok._plan()
    rc = _lib.load().beast_encode_f32(ptr, B, T, strides[0], strides[1], strides[2], row_elems, tok.num_dof,
                                      tok.joint_dof, p.p_src, p.p_proj, tok.num_basis, p.p_wmn, p.p_wmx,
                                      tok.vocab_size, 0, _lib.ptr(params), _lib.ptr(tokens), _lib.raw_stream(p.idx))
    _lib.check(rc, "beast_encode_f32")


V_LAT = dict(family="encode_v", tile=16, waves=16, fast=True, staged=True, latency=True)
V_BULK = dict(family="encode_v", tile=8, waves=8, fast=True, staged=True, latency=False)
SPEC7 = dict(family="encode_spec", tile=8, waves=7, fast=True, latency=True)


def _dyn(tile, fast):
    return dict(family="encode_dyn", tile=tile, waves=4, fast=fast, latency=False)


K2 = dict(T=50, D=14, N=10)
K3 = dict(T=50, D=14, N=10, grip=[6, 13])
K1 = dict(T=50, D=7, N=10)
RT = dict(T=24, D=8, N=12, B=19)             # a runtime shape with T >= 2 N
GATHER = dict(D=8, N=8, B=19, grip=[0, 5])   # gripper DoFs gathered from the middle of the row

# (id, shape, input layout, call, expected launch).  call: "api" tok.encode; "cabi" both outputs
# aligned; "p4" / "t8" / "p4t8" params_out 4 bytes / tokens_out 8 bytes past a 16-byte boundary;
# "tokens" / "params" only that output requested.
ENCODE_ROWS = [
    # k_encode_v: bulk (8-wave tiles, write-back stores; the last tile holds 3 of 8) and latency
    # (16-wave tiles; exactly at the threshold, and one full tile + 1 trajectory)
    ("v_bulk_k2", dict(K2, B="16cu+11"), "contig", "api", V_BULK),
    ("v_bulk_k3", dict(K3, B="16cu+11"), "contig", "api", V_BULK),
    ("v_lat_k2_16cu", dict(K2, B="16cu"), "contig", "api", V_LAT),
    ("v_lat_k3_16cu", dict(K3, B="16cu"), "contig", "api", V_LAT),
    ("v_lat_k2_17", dict(K2, B=17), "contig", "api", V_LAT),
    ("v_lat_k3_17", dict(K3, B=17), "contig", "api", V_LAT),
    # misaligned outputs leave k_encode_v for the specialised k_encode (its scalar store loops).
    # T * D = 350 is no multiple of 4 at D = 7, so that shape never takes the DMA path: its
    # specialised instantiation is unreachable and the runtime-shape gather runs instead.
    ("spec_k2_p4t8", dict(K2, B=37), "contig", "p4t8", SPEC7),
    ("spec_k2_p4", dict(K2, B=37), "contig", "p4", SPEC7),
    ("spec_k2_t8", dict(K2, B=37), "contig", "t8", SPEC7),
    ("spec_k3_p4t8", dict(K3, B=37), "contig", "p4t8", SPEC7),
    ("spec_k3_p4", dict(K3, B=37), "contig", "p4", SPEC7),
    ("spec_k3_t8", dict(K3, B=37), "contig", "t8", SPEC7),
    ("k1_p4t8", dict(K1, B=37), "contig", "p4t8", _dyn(8, False)),
    ("k1_p4", dict(K1, B=37), "contig", "p4", _dyn(8, False)),
    ("k1_t8", dict(K1, B=37), "contig", "t8", _dyn(8, False)),
    # runtime shape, contiguous DMA path: tiles of 8 / 4 / 2 / 1 trajectories (32 KB of rows)
    ("fast8_20x8", dict(T=20, D=8, N=12, B=19), "contig", "api", _dyn(8, True)),
    ("fast8_24x8", dict(RT), "contig", "api", _dyn(8, True)),
    ("fast4_64x24", dict(T=64, D=24, N=12, B=19), "contig", "api", _dyn(4, True)),
    ("fast2_96x32", dict(T=96, D=32, N=12, B=19), "contig", "api", _dyn(2, True)),
    ("fast1_128x48", dict(T=128, D=48, N=12, B=19), "contig", "api", _dyn(1, True)),
    ("fast1_256x32", dict(T=256, D=32, N=12, B=19), "contig", "api", _dyn(1, True)),
    ("fast8_p4t8", dict(RT), "contig", "p4t8", _dyn(8, True)),
    # runtime shape, strided gather: (a) T * D % 4 != 0, contiguous and with a column sliced off
    ("strided_9x3", dict(T=9, D=3, N=4, B=19, degree=3), "contig", "api", _dyn(8, False)),
    ("strided_9x3_cols", dict(T=9, D=3, N=4, B=19, degree=3), "col_slice", "api", _dyn(8, False)),
    ("strided_k1", dict(K1, B=19), "contig", "api", _dyn(8, False)),
    ("strided_k1_cols", dict(K1, B=19), "col_slice", "api", _dyn(8, False)),
    # (b) base pointer + 4 bytes  (c) row slice, time slice  (d) element stride between the DoFs
    ("strided_base4_k2", dict(K2, B=37), "base4", "api", _dyn(8, False)),
    ("strided_base4_rt", dict(RT), "base4", "api", _dyn(8, False)),
    ("strided_cols_k3", dict(K3, B=37), "col_slice", "api", _dyn(8, False)),
    ("strided_cols_rt", dict(RT), "col_slice", "api", _dyn(8, False)),
    ("strided_time_k2", dict(K2, B=37), "time_slice", "api", _dyn(8, False)),
    ("strided_time_rt", dict(RT), "time_slice", "api", _dyn(8, False)),
    ("strided_dt_k2", dict(K2, B=37), "dt", "cabi", _dyn(8, False)),
    ("strided_dt_rt", dict(RT), "dt", "cabi", _dyn(8, False)),
    ("strided_dt_rt_p4t8", dict(RT), "dt", "p4t8", _dyn(8, False)),
    # (e) rows wider than D with the gripper DoFs gathered from columns 0 and 5: DMA and gather
    ("wide_fast", dict(GATHER, T=20), "wide", "api", _dyn(8, True)),
    ("wide_strided", dict(GATHER, T=21), "wide", "api", _dyn(8, False)),
    # the header's limits: one trajectory above 32 KB is gathered a trajectory per tile; a
    # strided [B, 200, 24] takes the largest tile whose LDS layout fits
    ("limit_256x64", dict(T=256, D=64, N=16, B=9), "contig", "api", _dyn(1, False)),
    ("limit_200x24_cols", dict(T=200, D=24, N=16, B=9), "col_slice", "api", _dyn(4, False)),
    ("limit_256x48_cols", dict(T=256, D=48, N=16, B=9), "col_slice", "api", _dyn(2, False)),
    # nullable outputs
    ("tokens_only_v", dict(K2, B=37), "contig", "tokens", V_LAT),
    ("params_only_v", dict(K2, B=37), "contig", "params", V_LAT),
    ("tokens_only_rt", dict(RT), "contig", "tokens", _dyn(8, True)),
    ("params_only_rt", dict(RT), "contig", "params", _dyn(8, True)),
    ("tokens_only_strided", dict(RT), "dt", "tokens", _dyn(8, False)),
    # spline degree
    ("degree3", dict(T=40, D=5, N=8, B=19, degree=3), "contig", "api", _dyn(8, True)),
    ("degree5", dict(T=40, D=5, N=8, B=19, degree=5), "contig", "api", _dyn(8, True)),
]


@pytest.mark.parametrize("shape,layout,call,expect", [r[1:] for r in ENCODE_ROWS], ids=[r[0] for r in ENCODE_ROWS])
def test_encode_dispatch(shape, layout, call, expect, gpu_device):
    dev = gpu_device
    T, D, N = shape["T"], shape["D"], shape["N"]
    degree, grip, vocab = shape.get("degree", 4), shape.get("grip"), shape.get("vocab", 256)
    B = _batch(shape["B"], dev)
    assert T >= 2 * N or (T, N) == (20, 12)       # well-conditioned ridge systems
    x, exact, sums, lo, hi, lay = _enc_ref(T, D, N, B, degree, grip)
    tok = _make_tok(dev, D, N, T, vocab, degree, grip, lo, hi)
    DN = D * N
    _set_modes()
    try:
        # the aligned, contiguous result through the Python API: every variant must equal it bitwise
        t0, pd0 = tok.encode(torch.from_numpy(x).to(dev))
        base = _lib.last_codec_launch()
        params0, tokens0 = pd0["params"].cpu().numpy(), t0.cpu().numpy()
        view, ptr, strides, row_elems, keep = _place(x, layout, dev)
        if call == "api":
            t1, pd1 = tok.encode(view)
            _expect(**expect)
            params, tokens = pd1["params"].cpu().numpy(), t1.cpu().numpy()
        else:
            ps, ts = (1 if "p4" in call else 0), (1 if "t8" in call else 0)
            pbuf, pv = _shifted(dev, B, DN, torch.float32, ps)
            tbuf, tv = _shifted(dev, B, DN, torch.int64, ts)
            assert pv.data_ptr() % 16 == 4 * ps and tv.data_ptr() % 16 == 8 * ts
            _c_encode(tok, ptr, B, T, strides, row_elems, None if call == "tokens" else pv,
                      None if call == "params" else tv)
            _expect(**expect)
            params = None if call == "tokens" else pv.cpu().numpy()
            tokens = None if call == "params" else tv.cpu().numpy()
            assert _guards_intact(pbuf, ps, B * DN) and _guards_intact(tbuf, ts, B * DN)
            if call == "tokens":
                assert bool((pbuf == -7777).all())
            if call == "params":
                assert bool((tbuf == -7777).all())
    finally:
        _set_modes()
    assert base.family in ("encode_v", "encode_dyn") and base.raw != 0
    # values: the float64 fit, the quantiser on the kernel's own params, both clamp sides hit
    Tp = -(-T // 4) * 4
    bound = (Tp + 8) * 2.0 ** -24 * sums + 1e-30
    assert np.all(np.abs(params0 - exact) <= bound), float(np.max(np.abs(params0 - exact) / bound))
    assert (params0 < lo).any() and (params0 > hi).any()
    want = _dn_to_nd(O.continuous_to_discrete(O._clamp_t(params0, lo, hi), lo, hi, vocab), B, D, N)
    assert np.array_equal(tokens0, want)
    assert want.min() == 0 and want.max() == vocab - 1
    if params is not None:
        assert np.all(np.abs(params - exact) <= bound)
        assert np.array_equal(params, params0)
    if tokens is not None:
        assert np.array_equal(tokens, tokens0)


# -------------------------------------------------------------------------------- reconstruct --
def _rec_inputs(D, N, B, vocab, grip, seed):
    rng = np.random.default_rng(seed)
    lo = rng.uniform(-3, 1, size=D * N).astype(F32)
    hi = (lo + rng.uniform(0.1, 4, size=D * N)).astype(F32)
    tokens = rng.integers(0, vocab, size=(B, N * D)).astype(np.int64)
    flat = tokens.reshape(-1)
    # the vocabulary's ends, and tokens outside it (the dequantiser's division path, clamped)
    flat[:6] = (0, vocab - 1, vocab, vocab + 7, -1, -3)
    return tokens, lo, hi, O.Layout.make(D, grip, bool(grip)), rng


def _basis64(times, degree, N):
    return O.basis(times, TAU, degree, N).astype(np.float64)


def _positions_ref(w, lay, times, degree, N, dst, ndo):
    """float64 basis @ params: w [B, D, N] (d n) in the DoF order of the layout -> [B, T, ndo]."""
    B = w.shape[0]
    pj, pg = _basis64(times, degree, N), _basis64(times, 0, N)
    want = np.zeros((B, times.shape[-1], ndo))
    for i in range(lay.num_dof):
        ph = pj if i < len(lay.joint_indices) else pg
        want[:, :, dst[i]] = np.einsum("btn,bn->bt" if ph.ndim == 3 else "tn,bn->bt", ph, w[:, i].astype(np.float64))
    return want


def _assert_close(pos, want):
    scale = np.maximum(1.0, np.abs(want).max(axis=(1, 2), keepdims=True))
    err = np.abs(pos - want) / scale
    assert err.max() <= 1e-5, float(err.max())


def _c_reconstruct(tok, B, T_out, basis_ptr, basis_sb, dst, ndo, pos, tokens=None, ntokens=None, init_p=None,
                   init_p_sb=0):
    p = tok._plan()
    rc = _lib.load().beast_reconstruct_f32(
        _lib.ptr(tokens), B, tok.num_dof, tok.joint_dof, tok.num_basis, tok.vocab_size, 0, p.p_wmn, p.p_wmx,
        basis_ptr, basis_sb, T_out, dst.data_ptr(), ndo, _lib.ptr(init_p), init_p_sb,
        None if init_p is None else p.p_dst, None, pos.data_ptr(), _lib.ptr(ntokens), _lib.raw_stream(p.idx))
    _lib.check(rc, "beast_reconstruct_f32")


RV_LAT = dict(family="reconstruct_v", tile=16, waves=16, ks=3, basis_regs=True, staged=True, latency=True)
RV_BULK = dict(RV_LAT, latency=False)
RSPEC7 = dict(family="reconstruct_spec", tile=8, waves=7, ks=3, basis_regs=True, staged=True, latency=True)


def _mfma(ks, regs):
    return dict(family="reconstruct_mfma", tile=8, waves=4, ks=ks, basis_regs=regs, staged=True, latency=False)


def _rows(staged):
    return dict(family="reconstruct_rows", tile=8, waves=4, ks=0, basis_regs=False, staged=staged)


RK2 = dict(D=14, N=10, T=50)
RK3 = dict(D=14, N=10, T=50, grip=[6, 13])
SMALL = dict(D=5, B=19)

# (id, shape, call, expected launch).  shape: T output steps; grid "default" (the tokenizer's own
# time grid), "shared" (one explicit grid) or "rows" (one grid per trajectory); waves = forced
# BEAST_OPT_BLOCK_WAVES.  call: "api" reconstruct_traj; "ntokens" reconstruct_traj_continuous;
# "pos4" C-ABI, pos_out 4 bytes past a 16-byte boundary; "scatter" C-ABI, 6 DoFs into 9 output
# columns; "init_p" C-ABI, init_p rows of stride 2 * num_dof.
RECONSTRUCT_ROWS = [
    # k_reconstruct_v: bulk (write-back stores; forced, 11 trajectories in the last tile), latency
    ("v_bulk_k2", dict(RK2, B="16cu+11", waves=8), "api", RV_BULK),
    ("v_bulk_k3", dict(RK3, B="16cu+11", waves=8), "api", RV_BULK),
    ("v_lat_k2_17", dict(RK2, B=17), "api", RV_LAT),
    ("v_lat_k3_17", dict(RK3, B=17), "api", RV_LAT),
    ("v_lat_k2_16cu", dict(RK2, B="16cu"), "api", RV_LAT),
    ("v_lat_k3_16cu", dict(RK3, B="16cu"), "api", RV_LAT),
    ("v_lat_k2_vocab8192", dict(RK2, B=17, vocab=8192), "api", RV_LAT),
    # misaligned pos_out leaves k_reconstruct_v for the specialised k_reconstruct's scalar stores
    ("spec_k2_pos4", dict(RK2, B=37), "pos4", RSPEC7),
    ("spec_k3_pos4", dict(RK3, B=37), "pos4", RSPEC7),
    # runtime-shape MFMA kernel: KS = 1..4, basis operands in registers (T_out <= 64) ...
    ("ks1_regs", dict(SMALL, N=4, T=33, degree=3), "api", _mfma(1, True)),
    ("ks2_regs", dict(SMALL, N=8, T=33), "api", _mfma(2, True)),
    ("ks3_regs", dict(SMALL, N=12, T=33), "api", _mfma(3, True)),
    ("ks4_regs", dict(SMALL, N=16, T=33), "api", _mfma(4, True)),
    # ... and in LDS
    ("ks1_lds_65", dict(SMALL, N=4, T=65, degree=3), "api", _mfma(1, False)),
    ("ks2_lds_65", dict(SMALL, N=8, T=65), "api", _mfma(2, False)),
    ("ks3_lds_65", dict(SMALL, N=12, T=65), "api", _mfma(3, False)),
    ("ks4_lds_65", dict(SMALL, N=16, T=65), "api", _mfma(4, False)),
    ("ks1_lds_130", dict(SMALL, N=4, T=130, degree=3, grid="shared"), "api", _mfma(1, False)),
    ("ks2_lds_130", dict(SMALL, N=8, T=130, grid="shared"), "api", _mfma(2, False)),
    ("ks3_lds_130", dict(SMALL, N=12, T=130, grid="shared"), "api", _mfma(3, False)),
    ("ks4_lds_130", dict(SMALL, N=16, T=130, grid="shared"), "api", _mfma(4, False)),
    ("ks2_regs_pos4", dict(SMALL, N=8, T=33), "pos4", _mfma(2, True)),
    ("ks2_regs_pos4_vec", dict(D=8, N=8, T=32, B=19), "pos4", _mfma(2, True)),   # aligned: 16-byte stores
    ("ks2_regs_vocab8192", dict(SMALL, N=8, T=33, vocab=8192), "api", _mfma(2, True)),
    # rows kernel from a shared basis (the MFMA tile's LDS image is too large): staged through
    # LDS at 150 points, stored directly at 200 and 500; and from per-row grids
    ("rows_shared_150", dict(D=14, N=10, T=150, B=11, grid="shared"), "api", _rows(True)),
    ("rows_shared_200", dict(D=14, N=10, T=200, B=11, grid="shared"), "api", _rows(False)),
    ("rows_shared_200_k3", dict(D=14, N=10, T=200, B=11, grid="shared", grip=[6, 13]), "api", _rows(False)),
    ("rows_shared_500", dict(D=14, N=10, T=500, B=11, grid="shared"), "api", _rows(False)),
    ("rows_shared_500_pos4", dict(D=14, N=10, T=500, B=11, grid="shared"), "pos4", _rows(False)),
    ("rows_per_row_130", dict(D=14, N=10, T=130, B=11, grid="rows"), "api", _rows(True)),
    ("rows_per_row_130_k3", dict(D=14, N=10, T=130, B=11, grid="rows", grip=[6, 13]), "api", _rows(True)),
    ("rows_vocab8192", dict(SMALL, N=8, T=33, grid="rows", vocab=8192), "api", _rows(True)),
    # num_dof_out > D with a scattering dof_dst: the columns it does not name are zeros
    ("scatter_regs", dict(D=6, N=10, T=50, B=19), "scatter", _mfma(3, True)),
    ("scatter_lds", dict(D=6, N=10, T=130, B=19, grid="shared"), "scatter", _mfma(3, False)),
    ("scatter_rows", dict(D=6, N=10, T=50, B=19, grid="rows"), "scatter", _rows(True)),
    # init_p rows of stride 2 * num_dof
    ("init_p_mfma", dict(SMALL, N=8, T=33), "init_p", _mfma(2, True)),
    ("init_p_mfma_k3", dict(D=14, N=12, T=33, B=19, grip=[6, 13]), "init_p", _mfma(3, True)),
    ("init_p_rows", dict(SMALL, N=8, T=33, grid="rows"), "init_p", _rows(True)),
    # normalised fp32 tokens
    ("ntokens_ks4", dict(SMALL, N=16, T=33), "ntokens", _mfma(4, True)),
    ("ntokens_k2", dict(RK2, B=17), "ntokens", RSPEC7),
    ("ntokens_rows", dict(SMALL, N=16, T=33, grid="rows"), "ntokens", _rows(True)),
]

SCATTER_DST, SCATTER_NDO = [7, 0, 3, 8, 1, 5], 9


@pytest.mark.parametrize("shape,call,expect", [r[1:] for r in RECONSTRUCT_ROWS],
                         ids=[r[0] for r in RECONSTRUCT_ROWS])
def test_reconstruct_dispatch(shape, call, expect, gpu_device):
    dev = gpu_device
    D, N, T = shape["D"], shape["N"], shape["T"]
    degree, grip, vocab, grid = shape.get("degree", 4), shape.get("grip"), shape.get("vocab", 256), \
        shape.get("grid", "default")
    B = _batch(shape["B"], dev)
    tokens, lo, hi, lay, rng = _rec_inputs(D, N, B, vocab, grip, seed=D * 1000 + N * 10 + T)
    tok = _make_tok(dev, D, N, T if grid == "default" else 50, vocab, degree, grip, lo, hi)
    if grid == "default":
        times, times_t = O.times_grid(2 * np.pi, T), None
    elif grid == "shared":
        times = np.linspace(0, 2 * np.pi, T).astype(F32)
        times_t = torch.from_numpy(times)
    else:
        times = np.sort(rng.uniform(0, 2 * np.pi, size=(B, T)), axis=1).astype(F32)
        times_t = torch.from_numpy(times)
    tokens_t = torch.from_numpy(tokens).to(dev)
    dst, ndo = lay.order, D
    init_p = None
    _set_modes(waves=shape.get("waves", 0))
    try:
        # decode: the rows kernel without positions, bit for bit
        dec = tok.decode(tokens_t).cpu().numpy()
        _expect(family="reconstruct_rows", tile=8)
        if call == "api":
            pos = tok.reconstruct_traj(tokens_t, times=times_t)
            _expect(**expect)
        elif call == "ntokens":
            nt = rng.uniform(-1.2, 1.2, size=(B, N * D)).astype(F32)
            pos = tok.reconstruct_traj_continuous(torch.from_numpy(nt).to(dev), times=times_t)
            _expect(**expect)
        else:
            p = tok._plan()
            phi, p_phi, basis_sb, Tn = tok._basis_for(times_t, B, p)
            assert Tn == T
            dst_t = torch.tensor(lay.order, dtype=torch.int32, device=dev)
            shift = 0
            if call == "pos4":
                aligned = tok.reconstruct_traj(tokens_t, times=times_t)
                shift = 1
            elif call == "scatter":
                dst, ndo = SCATTER_DST, SCATTER_NDO
                dst_t = torch.tensor(dst, dtype=torch.int32, device=dev)
            elif call == "init_p":
                init_p = rng.uniform(-2, 2, size=(B, 2 * D)).astype(F32)
            buf = torch.full((B * T * ndo + 8,), float("nan"), device=dev)
            pos = buf[shift:shift + B * T * ndo].view(B, T, ndo)
            assert pos.data_ptr() % 16 == 4 * shift
            ip = None if init_p is None else torch.from_numpy(init_p).to(dev)
            _c_reconstruct(tok, B, T, p_phi, basis_sb, dst_t, ndo, pos, tokens=tokens_t, init_p=ip,
                           init_p_sb=2 * D)
            _expect(**expect)
            guard = torch.cat([buf[:shift], buf[shift + B * T * ndo:]])
            assert bool(torch.isnan(guard).all())
            if call == "pos4":
                assert torch.equal(pos, aligned)
    finally:
        _set_modes()
    pos = pos.cpu().numpy()
    assert pos.shape == (B, T, ndo) and pos.dtype == np.float32
    want_dec = O.decode(tokens, lay, N, lo, hi, vocab)
    assert np.array_equal(dec, want_dec)
    if call == "ntokens":   # denormalize_tensor's intent (beast/utils.py:38-44), fp32 op by op
        c = np.clip(nt, F32(-1), F32(1)).reshape(B, N, D).transpose(0, 2, 1).reshape(B, D * N)
        u = ((c - F32(-1)) / F32(2)).astype(F32)
        w = ((u * (hi - lo)).astype(F32) + lo).astype(F32).reshape(B, D, N)
    else:
        w = want_dec.reshape(B, D, N).copy()
    if init_p is not None:   # coefficient 0 of the joint DoFs <- init_p[:, the DoF's column]
        for i, col in enumerate(lay.joint_indices):
            w[:, i, 0] = init_p[:, col]
    _assert_close(pos, _positions_ref(w, lay, times, degree, N, dst, ndo))
    unnamed = sorted(set(range(ndo)) - set(dst))
    assert call != "scatter" or unnamed == [2, 4, 6]
    assert not pos[:, :, unnamed].any()
