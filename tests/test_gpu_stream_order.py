"""Every entry point is ordered on the stream it is given (include/beast_hip.h: "every call is
stream-ordered on `stream`"; INTEGRATION.md: the Python API behaves "like any torch op").

tests/stream_order.py holds the probe: stale inputs everywhere, then on a fresh side stream a
delay, a poison fill of every output and workspace, the copy of the good inputs, the call and a
snapshot -- with no host synchronisation -- and the snapshot must equal what the null stream
computed from the good inputs.  A kernel, memset or copy issued on any other stream ran while the
delay was still running (``busy``) and shows as stale or poisoned output.  The side stream is one
that demonstrably runs beside the null stream: streams that share a hardware queue execute in
submission order, and late in a long test process a new stream often shares the null stream's.

Two canaries guard the probe itself: a torch copy issued on the null stream, and two library
calls (a kernel, an internal memset) handed the null stream, must all be REPORTED as mis-ordered.
If the first is not, every test of every stream-order module fails (the ``canary`` fixture of
tests/stream_order.py, computed once per process).  After a HIP error in any of those modules no
later stream-order test starts GPU work (``stops_after_a_fault``).

Section A calls the C-ABI with the side stream's handle while torch's current stream is the null
stream; section B calls the Python API under ``torch.cuda.stream(s)``; section C builds the cached
constants on one stream behind a delay and uses them at once from two others.

The ``extern "C"`` functions that take a ``void* stream`` and are not probed in one of the six
sibling modules (tests/test_stream_order_accounting.py checks the lists of all seven against
include/beast_hip.h):

probed
    beast_bspline_basis_f32  beast_bspline_basis_deriv_f32  beast_bspline_projection_f64
    beast_encode_f32  beast_encode_list_f32  beast_quantize_f32  beast_encode_rows_f32
    beast_reconstruct_f32  beast_reconstruct_derivs_f32  beast_reconstruct_derivs_bwd_f32
    beast_roundtrip_stats_f32  beast_cond_fixed_f32  beast_cond_add_f32  beast_colminmax_f32
    beast_quantile_prepare  beast_quantile_prepare_segments  beast_quantile_hist
    beast_quantile_select  beast_quantile_finalize  beast_quantile_f32
    beast_i64_minmax  beast_bpe_cp_presence  beast_bpe_pretok_count  beast_exclusive_scan_i64
    beast_bpe_pretok_emit  beast_bpe_count_pairs  beast_bpe_word_signatures  beast_bpe_dedup_words
    beast_bpe_pretok_dedup  beast_bpe_pretok_dedup_repack  beast_bpe_repack_words
    beast_bpe_compact_words  beast_bpe_argmax  beast_bpe_merge  beast_bpe_apply_argmax
    beast_bpe_loop_init  beast_bpe_loop_batch  beast_bpe_mergemap_build  beast_bpe_encode_rows
    beast_bpe_encode_rows_words  beast_bpe_decode_rows

probed in the weaker form (the call synchronises the host inside, so the stream cannot be busy
when it returns: stale input and poison only)
    beast_bpe_train

not probed
    beast_comm_allreduce  beast_comm_allgather  beast_comm_allgatherv  beast_bpe_train_comm
    -- every collective synchronises the caller's stream and meets the other ranks in host memory
    or in RCCL, from one host thread per rank: host threads and the RCCL side of comm.hip are
    outside this module (tests/test_comm_virtual.py, tests/test_gpu_collectives.py drive them).
"""
import ctypes
import json

import numpy as np
import pytest
import torch

import deriv_bwd_oracle as BO
import roundtrip_oracle
import rows_oracle as RO
import stream_order as SO
from conftest import CONFIGS, load_json, load_npz
from stream_order import CASES, Case, api, canary, capi, probe, stops_after_a_fault  # noqa: F401 (canary: autouse)
from test_deriv_bwd_oracle import make_inputs

pytestmark = pytest.mark.gpu

from beast_tokenizer_amd import BEASTBsplineBPETokenizer, BEASTBsplineTokenizer, _lib  # noqa: E402
from beast_tokenizer_amd.bspline import knot_vector  # noqa: E402
from beast_tokenizer_amd.synthetic import synth_trajectories  # noqa: E402
from oracle import beast_oracle as O  # noqa: E402

F32 = np.float32
EPS = 2.0 ** -24

PROBED = """
    beast_bspline_basis_f32 beast_bspline_basis_deriv_f32 beast_bspline_projection_f64
    beast_encode_f32 beast_encode_list_f32 beast_quantize_f32 beast_encode_rows_f32
    beast_reconstruct_f32 beast_reconstruct_derivs_f32 beast_reconstruct_derivs_bwd_f32
    beast_roundtrip_stats_f32 beast_cond_fixed_f32 beast_cond_add_f32 beast_colminmax_f32
    beast_quantile_prepare beast_quantile_prepare_segments beast_quantile_hist
    beast_quantile_select beast_quantile_finalize beast_quantile_f32
    beast_i64_minmax beast_bpe_cp_presence beast_bpe_pretok_count beast_exclusive_scan_i64
    beast_bpe_pretok_emit beast_bpe_count_pairs beast_bpe_word_signatures beast_bpe_dedup_words
    beast_bpe_pretok_dedup beast_bpe_pretok_dedup_repack beast_bpe_repack_words
    beast_bpe_compact_words beast_bpe_argmax beast_bpe_merge beast_bpe_apply_argmax
    beast_bpe_loop_init beast_bpe_loop_batch beast_bpe_mergemap_build beast_bpe_encode_rows
    beast_bpe_encode_rows_words beast_bpe_decode_rows
""".split()
# these synchronise the host inside (csrc/bpe_train_api.hip reads the word counts, the loop state and
# the merge log back): the probe runs without the ``busy`` assertion, its weaker form
SYNCHRONOUS = ["beast_bpe_train"]
NOT_PROBED = {
    "beast_comm_allreduce": "a collective: synchronises the stream and meets the other ranks (host threads, RCCL)",
    "beast_comm_allgather": "a collective: synchronises the stream and meets the other ranks (host threads, RCCL)",
    "beast_comm_allgatherv": "a collective: synchronises the stream and meets the other ranks (host threads, RCCL)",
    "beast_bpe_train_comm": "beast_bpe_train plus collectives, one host thread per rank; comm == NULL is beast_bpe_train",
}


def dv(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def npy(t):
    return t.detach().cpu().numpy()


def buf_like(t):
    return torch.empty_like(t)


def flip_rows(t):
    """Stale floats / ids: the rows in reverse order (every value stays a valid one)."""
    return t.flip(0).contiguous()


def run(name, *args):
    _lib.run(name, *args)


# ------------------------------------------------------------------------ canary --
def test_canary_reports_a_mismatch(canary):
    """The mis-ordered copy ran while the delay was still running (busy) and the snapshot is not the
    expected copy of the good input: it is the poison the side stream wrote afterwards."""
    assert canary.busy
    assert canary.mismatch == [0]
    assert not SO.bits_equal(canary.snapshot[0], canary.expected[0])
    assert bool(torch.isnan(canary.snapshot[0]).all())


@pytest.mark.parametrize("cid", ["quantize[mode0-tokens]", "bspline_basis_deriv[order2-above-degree-memset]"])
@stops_after_a_fault
def test_probe_sees_an_entry_point_on_the_wrong_stream(cid, gpu_device):
    """The same canary through the library: a kernel (k_quantize) and an internal memset (the
    order > degree branch of beast_bspline_basis_deriv_f32) handed the NULL stream while the probe
    drives the side stream.  The kernel reads the stale input, the memset is overwritten by the
    poison: both must be reported, or a wrong stream inside the library would go unseen too."""
    case = CASES[cid][2](gpu_device)
    inner = case.call
    case.call = lambda _handle: inner(None)
    r = probe(case, gpu_device)
    assert r.busy and r.mismatch, (cid, r.busy, r.mismatch)


# ================================================================= A. codec (k3 shapes) ==
_CTX = {}


def codec(dev):
    """The k3 tokenizer (T 50, D 14 = 12 joints + 2 grippers, N 10) with the golden bounds, its
    launch plan and the goldens' bases; shared and never modified."""
    if "codec" not in _CTX:
        g = load_npz("bspline_k3.npz")
        tok = BEASTBsplineTokenizer(device=str(dev), **CONFIGS["k3"])
        tok.load_state_dict({"w_min": g["w_min"].tolist(), "w_max": g["w_max"].tolist()})
        p = tok._plan()
        torch.cuda.synchronize(dev)
        _CTX["codec"] = (tok, p, g, O.Layout.make(14, [6, 13], True))
    return _CTX["codec"]


def trajectories(B, dev, seed=3):
    return dv(synth_trajectories(B, 50, 14, seed=seed, gripper_indices=[6, 13]), dev)


def check_params(x, params, g, lay):
    """test_gpu_parity's bound against the float64 fit: (T + 8) 2^-24 sum_t |P y|."""
    pj, pg = g["phi_joint"], g["phi_grip"]
    ex = np.concatenate([O.fit_exact(x[..., lay.joint_indices], pj), O.fit_exact(x[..., lay.gripper_indices], pg)], -1)
    S = []
    for idx, ph in ((lay.joint_indices, pj), (lay.gripper_indices, pg)):
        P = np.abs(O.projection_f64(ph))
        S.append(np.einsum("nt,btd->bdn", P, np.abs(x[..., idx].astype(np.float64))).reshape(len(x), -1))
    assert np.all(np.abs(params - ex) <= (50 + 8) * EPS * np.concatenate(S, -1) + 1e-30)


def check_tokens(params, tokens, g):
    want = O.continuous_to_discrete(O._clamp_t(params, g["w_min"], g["w_max"]), g["w_min"], g["w_max"], 256)
    B = params.shape[0]
    assert np.array_equal(tokens, want.reshape(B, 14, 10).transpose(0, 2, 1).reshape(B, 140))


def encode_case(dev, B, latency):
    tok, p, g, lay = codec(dev)
    good = trajectories(B, dev)
    x = buf_like(good)
    params = torch.empty((B, 140), dtype=torch.float32, device=dev)
    tokens = torch.empty((B, 140), dtype=torch.int64, device=dev)

    def call(h):
        run("beast_encode_f32", x.data_ptr(), B, 50, *x.stride(), 14, 14, tok.joint_dof, p.p_src, p.p_proj, 10,
            p.p_wmn, p.p_wmx, 256, 0, params.data_ptr(), tokens.data_ptr(), h)
        assert _lib.last_codec_launch().latency is latency
        return [params, tokens]

    def check(exp):
        check_params(npy(good), npy(exp[0]), g, lay)
        check_tokens(npy(exp[0]), npy(exp[1]), g)
    return Case(f"encode[B{B}]", ("beast_encode_f32",), [(x, good, flip_rows(good))], call, scratch=[params, tokens],
                check_expected=check)


@capi("encode[B17-latency]", "beast_encode_f32")
def _(dev):
    return encode_case(dev, 17, True)


@capi("encode[B20011-bulk]", "beast_encode_f32")
def _(dev):
    return encode_case(dev, 20011, False)


def encode_list_case(dev, rows):
    tok, p, g, lay = codec(dev)
    goods = [trajectories(rows, dev, seed=5), trajectories(rows, dev, seed=6)]
    xs = [buf_like(t) for t in goods]
    table = torch.tensor([t.data_ptr() for t in xs], dtype=torch.int64).to(dev)   # the pointer table is never stale
    params = torch.empty((2 * rows, 140), dtype=torch.float32, device=dev)

    def call(h):
        run("beast_encode_list_f32", table.data_ptr(), 2, rows, 50, 14, 14, tok.joint_dof, p.p_src, p.p_proj, 10,
            params.data_ptr(), h)
        return [params]

    def check(exp):
        check_params(np.concatenate([npy(t) for t in goods]), npy(exp[0]), g, lay)
    return Case(f"encode_list[2x{rows}]", ("beast_encode_list_f32",),
                [(x, t, flip_rows(t)) for x, t in zip(xs, goods)], call, scratch=[params], check_expected=check)


@capi("encode_list[2x24-latency]", "beast_encode_list_f32")
def _(dev):
    return encode_list_case(dev, 24)


@capi("encode_list[2x10008-bulk]", "beast_encode_list_f32")
def _(dev):
    return encode_list_case(dev, 10008)


def reconstruct_case(dev, B, latency):
    tok, p, g, lay = codec(dev)
    good = dv(np.random.default_rng(B).integers(0, 256, size=(B, 140)), dev)
    t = buf_like(good)
    params = torch.empty((B, 140), dtype=torch.float32, device=dev)
    pos = torch.empty((B, 50, 14), dtype=torch.float32, device=dev)

    def call(h):
        run("beast_reconstruct_f32", t.data_ptr(), B, 14, tok.joint_dof, 10, 256, 0, p.p_wmn, p.p_wmx, p.p_phi, 0, 50,
            p.p_dst, 14, None, 0, None, params.data_ptr(), pos.data_ptr(), None, h)
        assert _lib.last_codec_launch().latency is latency
        return [params, pos]

    def check(exp):
        tk = npy(good)
        assert np.array_equal(npy(exp[0]), O.decode(tk, lay, 10, g["w_min"], g["w_max"], 256))
        want = O.reconstruct(tk, g["phi_joint"], g["phi_grip"], lay, g["w_min"], g["w_max"], 256)
        scale = np.maximum(1.0, np.abs(want).max(axis=(1, 2), keepdims=True))
        assert (np.abs(npy(exp[1]) - want) / scale).max() <= 1e-5
    return Case(f"reconstruct[B{B}]", ("beast_reconstruct_f32",), [(t, good, flip_rows(good))], call,
                scratch=[params, pos], check_expected=check)


@capi("reconstruct[B17-latency]", "beast_reconstruct_f32")
def _(dev):
    return reconstruct_case(dev, 17, True)


@capi("reconstruct[B20011-bulk]", "beast_reconstruct_f32")
def _(dev):
    return reconstruct_case(dev, 20011, False)


def roundtrip_case(dev, B):
    from test_gpu_roundtrip import _check
    tok, p, g, lay = codec(dev)
    good = trajectories(B, dev, seed=9)
    x = buf_like(good)
    tokens = torch.empty((B, 140), dtype=torch.int64, device=dev)
    stats = torch.empty((B, 14, 4), dtype=torch.float32, device=dev)
    clip = torch.empty((2, 140), dtype=torch.int32, device=dev)

    def call(h):
        run("beast_roundtrip_stats_f32", x.data_ptr(), B, 50, *x.stride(), 14, 14, tok.joint_dof, p.p_src, p.p_proj,
            p.p_phi, 10, p.p_wmn, p.p_wmx, 256, 0, tokens.data_ptr(), stats.data_ptr(), clip.data_ptr(), h)
        return [tokens, stats, clip]
    return Case(f"roundtrip_stats[B{B}]", ("beast_roundtrip_stats_f32",), [(x, good, flip_rows(good))], call,
                scratch=[tokens, stats, clip], setup=clip.zero_,        # clip_counts: "the caller zero-fills"
                check_expected=lambda exp: _check(tok, good, exp[1], exp[0], exp[2]))


@capi("roundtrip_stats[B17-latency]", "beast_roundtrip_stats_f32")
def _(dev):
    return roundtrip_case(dev, 17)


@capi("roundtrip_stats[B20011-bulk]", "beast_roundtrip_stats_f32")
def _(dev):
    return roundtrip_case(dev, 20011)


# ---- derivatives: the inputs of tests/test_deriv_bwd_oracle.make_inputs (random slabs, bounds, dof_dst)
def deriv_inputs(B, per_row):
    c = make_inputs(B, 50, 14, 12, 10, (0, 1, 2), ndo=17, per_row=per_row, seed=3)
    return c


def derivs_case(dev, B, per_row):
    c = deriv_inputs(B, per_row)
    T, N, D, nj, ndo = 50, 10, 14, c["nj"], c["ndo"]
    xg = np.nan_to_num(c["x"], nan=0.5)                   # the forward reads every ntoken: no NaN planted
    good = dv(xg, dev)
    x = buf_like(good)
    lo, hi, basis, dst = (dv(c[k], dev) for k in ("lo", "hi", "basis", "dst"))
    outs = [torch.empty((B, T, ndo), dtype=torch.float32, device=dev) for _ in range(3)]

    def call(h):
        run("beast_reconstruct_derivs_f32", None, B, D, nj, N, 256, 0, lo.data_ptr(), hi.data_ptr(), basis.data_ptr(),
            3 * 2 * T * N if per_row else 0, T, dst.data_ptr(), ndo, None, 0, None, *[o.data_ptr() for o in outs],
            x.data_ptr(), h)
        return outs

    def check(exp):
        """test_gpu_derivs.raw_case's yardstick: the float64 sum of the same products, within the dot
        product's bound (N + 1) 2^-24 sum |basis w|; unnamed columns and gripper derivatives 0."""
        cl = np.clip(xg, F32(-1), F32(1))
        w = ((cl - F32(-1)) / F32(2)) * (c["hi"].T - c["lo"].T) + c["lo"].T
        w = np.ascontiguousarray(w.astype(F32).transpose(0, 2, 1))
        for o in range(3):
            want, mag = np.zeros((B, T, ndo)), np.zeros((B, T, ndo))
            for d in range(D):
                kind = 0 if d < nj else 1
                if o and kind:
                    continue
                ph = c["basis"][..., o, kind, :, :].astype(np.float64)
                sub = "tn,bn->bt" if ph.ndim == 2 else "btn,bn->bt"
                want[:, :, c["dst"][d]] = np.einsum(sub, ph, w[:, d].astype(np.float64))
                mag[:, :, c["dst"][d]] = np.einsum(sub, np.abs(ph), np.abs(w[:, d].astype(np.float64)))
            got = npy(exp[o]).astype(np.float64)
            assert not np.isnan(got).any()
            assert (np.abs(got - want) <= (N + 1) * EPS * mag).all(), o
            assert not got[mag == 0].any()
    return Case(f"reconstruct_derivs[B{B}]", ("beast_reconstruct_derivs_f32",), [(x, good, flip_rows(good))], call,
                scratch=outs, check_expected=check)


@capi("reconstruct_derivs[B17-shared-slabs]", "beast_reconstruct_derivs_f32")
def _(dev):
    return derivs_case(dev, 17, False)


@capi("reconstruct_derivs[B5-per-row-slabs]", "beast_reconstruct_derivs_f32")
def _(dev):
    return derivs_case(dev, 5, True)


def derivs_bwd_case(dev, B, per_row):
    c = deriv_inputs(B, per_row)
    T, N, D, nj, ndo = 50, 10, 14, c["nj"], c["ndo"]
    gx_good = dv(c["x"], dev)
    grads_good = [dv(g, dev) for g in c["grads"]]
    x, grads = buf_like(gx_good), [buf_like(g) for g in grads_good]
    lo, hi, basis, dst, src = (dv(c[k], dev) for k in ("lo", "hi", "basis", "dst", "ip_src"))
    gnt = torch.empty((B, N, D), dtype=torch.float32, device=dev)
    gip = torch.empty((B, D + 3), dtype=torch.float32, device=dev)

    def call(h):
        run("beast_reconstruct_derivs_bwd_f32", *[g.data_ptr() for g in grads], B, D, nj, N, lo.data_ptr(),
            hi.data_ptr(), basis.data_ptr(), 3 * 2 * T * N if per_row else 0, T, dst.data_ptr(), ndo, x.data_ptr(),
            src.data_ptr(), gnt.data_ptr(), gip.data_ptr(), D + 3, h)
        return [gnt, gip]

    def check(exp):
        """tests/test_gpu_deriv_bwd.check: the float64 oracle and the accumulation's own bound."""
        got, got_ip = npy(exp[0]), npy(exp[1])
        r = BO.backward(c["grads"], c["basis"], c["lo"], c["hi"], c["x"], c["dst"], nj, init_p_src=c["ip_src"],
                        init_p_width=D + 3)
        assert not np.isnan(got).any()
        assert (np.abs(got.astype(np.float64) - r.grad_ntokens) <= BO.bound(r)).all()
        assert not got[r.grad_ntokens == 0].any()
        s = c["ip_src"]
        assert (np.abs(got_ip[:, s[:nj]] - r.grad_init_p[:, s[:nj]]) <= r.terms * BO.EPS * r.mag[:, :nj, 0]).all()
        assert not got_ip[:, sorted(set(range(D + 3)) - set(s[:nj].tolist()))].any()
    # grad_init_p is "zero-filled by the caller" (include/beast_hip.h): poisoned, then zeroed on the stream
    return Case(f"reconstruct_derivs_bwd[B{B}]", ("beast_reconstruct_derivs_bwd_f32",),
                [(x, gx_good, flip_rows(gx_good))] + [(b, g, flip_rows(g)) for b, g in zip(grads, grads_good)], call,
                scratch=[gnt, gip], setup=gip.zero_, check_expected=check)


@capi("reconstruct_derivs_bwd[B17-shared-slabs-grad_init_p]", "beast_reconstruct_derivs_bwd_f32")
def _(dev):
    return derivs_bwd_case(dev, 17, False)


@capi("reconstruct_derivs_bwd[B5-per-row-slabs-grad_init_p]", "beast_reconstruct_derivs_bwd_f32")
def _(dev):
    return derivs_bwd_case(dev, 5, True)


@capi("encode_rows[B5-T9-times-weights]", "beast_encode_rows_f32")
def _(dev):
    B, T, D, N, deg = 5, 9, 7, 4, 3
    tok = BEASTBsplineTokenizer(num_dof=D, num_basis=N, degree_p=deg, device=str(dev))
    tok.load_state_dict({"w_min": [-3.0] * (D * N), "w_max": [3.0] * (D * N)})
    xg, tg = RO.random_walk(B, T, D, 41), RO.jittered_times(B, T, 2 * np.pi, 42)
    wg = np.random.default_rng(43).uniform(0.25, 4.0, (B, T)).astype(F32)
    goods = [dv(a, dev) for a in (xg, tg, wg)]
    x, t, w = (buf_like(a) for a in goods)
    basis = tok._basis
    kj = basis.knots(dev, 0)
    src, _ = tok._dof_maps(dev)
    wmn, wmx = tok._bounds(dev)
    params = torch.empty((B, D * N), dtype=torch.float32, device=dev)
    tokens = torch.empty((B, N * D), dtype=torch.int64, device=dev)

    def call(h):
        run("beast_encode_rows_f32", x.data_ptr(), B, T, *x.stride(), D, D, src.data_ptr(), t.data_ptr(), T,
            w.data_ptr(), T, basis.tau, basis.delay, kj.data_ptr(), kj.numel(), None, 0, deg, N, basis.reg,
            wmn.data_ptr(), wmx.data_ptr(), 256, 0, params.data_ptr(), tokens.data_ptr(), h)
        return [params, tokens]

    def check(exp):
        want, _ = RO.fit(xg, tg, wg, tau=F32(tok.duration), degree=deg, num_basis=N, joint_indices=tok.joint_indices,
                         gripper_indices=[])
        assert RO.parity_ok(npy(exp[0]), want).all(), RO.parity_err(npy(exp[0]), want)
        assert np.array_equal(npy(exp[1]), RO.tokens(npy(exp[0]), npy(wmn), npy(wmx), 256, D, N))
    return Case("encode_rows", ("beast_encode_rows_f32",), [(b, a, flip_rows(a)) for b, a in zip((x, t, w), goods)],
                call, scratch=[params, tokens], check_expected=check)


def cond_case(dev, ic, ec, which):
    """beast_cond_fixed_f32 / beast_cond_add_f32 at B 5 against bspline.DeviceBasis.fixed_ctrl /
    fixed_term, the torch restatement tests/test_gpu_parity.py holds them to."""
    B, T, D = 5, 50, 14
    g = [6, 13]
    tok = BEASTBsplineTokenizer(num_dof=D, gripper_zero_order=True, gripper_indices=g, init_cond_order=ic,
                                end_cond_order=ec, device=str(dev))
    b = tok._basis
    good = dv(synth_trajectories(B, T, D, seed=7, gripper_indices=g), dev)
    jidx, times, kv = tok._cond_consts(dev)
    dj = jidx.numel()

    def out(*shape):
        return torch.empty(shape, dtype=torch.float32, device=dev)
    ip, iv, p_init = (out(B, dj), out(B, dj), out(B, dj, ic)) if ic else (None, None, None)
    ep, ev, p_end = (out(B, dj), out(B, dj), out(B, dj, abs(ec))) if ec else (None, None, None)
    six = (ip, iv, ep, ev, p_init, p_end)
    want = b.fixed_ctrl(good[..., tok.joint_indices], times[1] - times[0])
    torch.cuda.synchronize(dev)
    if which == "fixed":
        x = buf_like(good)

        def call(h):
            run("beast_cond_fixed_f32", x.data_ptr(), B, T, *x.stride(), jidx.data_ptr(), dj, times.data_ptr(),
                kv.data_ptr(), b.degrees[0], b.n_ctrl, float(b.tau), ic, ec, *map(_lib.ptr, six), h)
            return [t for t in six if t is not None]

        def check(exp):
            for got, w in zip(exp, [w for w in want if w is not None]):
                np.testing.assert_allclose(npy(got), npy(w), rtol=1e-6, atol=1e-7)
        return Case(f"cond_fixed[ic{ic}-ec{ec}]", ("beast_cond_fixed_f32",), [(x, good, flip_rows(good))], call,
                    scratch=[t for t in six if t is not None], check_expected=check)
    # cond_add: pos += the fixed control points' term; pos and the conditions are its inputs
    w_ip, _, _, _, w_pi, w_pe = want
    full = b.full_basis_at(times).contiguous()
    pos_good = torch.zeros((B, T, D), dtype=torch.float32, device=dev)     # as test_condition_kernels_match_torch_restatement
    pos = buf_like(pos_good)
    conds = [(torch.empty_like(w.contiguous()), w.contiguous(), flip_rows(w)) for w in (w_pi, w_pe, w_ip)
             if w is not None]
    bufs = iter(c[0] for c in conds)
    b_pi = next(bufs) if w_pi is not None else None
    b_pe = next(bufs) if w_pe is not None else None
    b_ip = next(bufs) if w_ip is not None else None
    torch.cuda.synchronize(dev)

    def call(h):
        run("beast_cond_add_f32", pos.data_ptr(), B, T, D, jidx.data_ptr(), dj, full.data_ptr(), 0, b.n_ctrl, ic, ec,
            _lib.ptr(b_pi), _lib.ptr(b_pe), _lib.ptr(b_ip), h)
        return [pos]

    def check(exp):
        ref = b.fixed_term(full, w_pi, w_pe, w_ip, fit=False)
        got = npy(exp[0])
        np.testing.assert_allclose(got[..., tok.joint_indices], npy(ref), rtol=1e-6, atol=1e-6)
        assert not got[..., g].any()
    return Case(f"cond_add[ic{ic}-ec{ec}]", ("beast_cond_add_f32",), [(pos, pos_good, torch.ones_like(pos_good))] + conds,
                call, check_expected=check)


for _ic, _ec in ((2, 2), (0, -1)):
    capi(f"cond_fixed[ic{_ic}-ec{_ec}-B5]", "beast_cond_fixed_f32")(
        lambda dev, ic=_ic, ec=_ec: cond_case(dev, ic, ec, "fixed"))
    capi(f"cond_add[ic{_ic}-ec{_ec}-B5]", "beast_cond_add_f32")(
        lambda dev, ic=_ic, ec=_ec: cond_case(dev, ic, ec, "add"))


# ====================================================================== A. fit and quantise ==
def basis_case(dev, entry, order, degree, branch):
    N, tau = 10, float(F32(2 * np.pi))
    tg = np.sort(np.random.default_rng(5).uniform(-0.3, 6.6, 333)).astype(F32)       # two workgroups
    good = dv(tg, dev)
    t = buf_like(good)
    kv = knot_vector(degree, N).to(dev)
    outb = torch.empty((333, N), dtype=torch.float32, device=dev)

    def call(h):
        args = [t.data_ptr(), 333, tau, 0.0, kv.data_ptr(), kv.numel(), degree, N]
        run(entry, *args, *([outb.data_ptr(), h] if order is None else [order, outb.data_ptr(), h]))
        return [outb]

    def check(exp):
        got = npy(exp[0])
        if not order:
            assert np.array_equal(got, O.basis(tg, F32(tau), degree, N))        # bit-exact (test_basis_bitexact)
        elif order > degree:
            assert not got.any()
        else:
            import deriv_oracle as DO
            want = DO.deriv_basis(tg, tau, degree, N, order)
            yard = DO.rel_err(DO.deriv_basis(tg, tau, degree, N, order, dtype=F32), want)
            assert DO.rel_err(got, want) <= max(4 * yard, 16 * EPS)             # test_gpu_derivs.bound
    case = Case(f"{entry}[{branch}]", (entry,), [(t, good, flip_rows(good))], call, scratch=[outb], check_expected=check)
    if order is not None and order > degree:
        case.inputs = []          # the memset branch reads nothing: only the poison can show it
    return case


capi("bspline_basis[degree4]", "beast_bspline_basis_f32")(
    lambda dev: basis_case(dev, "beast_bspline_basis_f32", None, 4, "degree4"))
capi("bspline_basis_deriv[order0-basis-kernel]", "beast_bspline_basis_deriv_f32")(
    lambda dev: basis_case(dev, "beast_bspline_basis_deriv_f32", 0, 4, "order0"))
capi("bspline_basis_deriv[order1-kernel]", "beast_bspline_basis_deriv_f32")(
    lambda dev: basis_case(dev, "beast_bspline_basis_deriv_f32", 1, 4, "order1"))
capi("bspline_basis_deriv[order2-above-degree-memset]", "beast_bspline_basis_deriv_f32")(
    lambda dev: basis_case(dev, "beast_bspline_basis_deriv_f32", 2, 1, "order2>degree1"))


@capi("bspline_projection_f64[asynchronous-one-workgroup]", "beast_bspline_projection_f64")
def _(dev):
    tok, p, g, lay = codec(dev)
    good = dv(g["phi_joint"], dev)                       # [50][10]
    stale = good.flip(1).contiguous()                    # the basis functions in reverse order: as well conditioned
    phi = buf_like(good)
    proj = torch.empty((16, 52), dtype=torch.float64, device=dev)

    def call(h):
        run("beast_bspline_projection_f64", phi.data_ptr(), 50, 10, 1e-9, proj.data_ptr(), h)
        return [proj]

    def check(exp):
        pp = npy(exp[0])
        assert not pp[10:].any() and not pp[:, 50:].any()
        assert np.allclose(pp[:10, :50], O.projection_f64(g["phi_joint"]), rtol=1e-12, atol=1e-13)   # test_basis_bitexact
    return Case("projection", ("beast_bspline_projection_f64",), [(phi, good, stale)], call, scratch=[proj],
                check_expected=check)


def quantize_case(dev, mode):
    tok, p, g, lay = codec(dev)
    B = 300                                               # 42,000 elements: more than one workgroup
    good = dv(g["params"][np.arange(B) % len(g["params"])] * np.linspace(0.5, 1.5, B, dtype=F32)[:, None], dev)
    x = buf_like(good)
    outb = torch.empty((B, 140), dtype=torch.int64 if mode == 0 else torch.float32, device=dev)

    def call(h):
        run("beast_quantize_f32", x.data_ptr(), B, 14, 10, p.p_wmn, p.p_wmx, 256, 0, mode,
            outb.data_ptr() if mode == 0 else None, outb.data_ptr() if mode == 1 else None, h)
        return [outb]

    def check(exp):
        pr = npy(good)
        if mode == 0:
            check_tokens(pr, npy(exp[0]), g)
        else:   # normalize_tensor (beast/utils.py:29-35) of the clamped params, (d n) -> (n d)
            lo, hi = g["w_min"], g["w_max"]
            n = (O._clamp_t(pr, lo, hi) - lo) / np.maximum(hi - lo, F32(1e-8)) * 2 - 1
            want = n.reshape(B, 14, 10).transpose(0, 2, 1).reshape(B, 140)
            assert np.abs(npy(exp[0]) - want).max() <= 4 * 2.0 ** -23
    return Case(f"quantize[mode{mode}]", ("beast_quantize_f32",), [(x, good, flip_rows(good))], call, scratch=[outb],
                check_expected=check)


capi("quantize[mode0-tokens]", "beast_quantize_f32")(lambda dev: quantize_case(dev, 0))
capi("quantize[mode1-normalised]", "beast_quantize_f32")(lambda dev: quantize_case(dev, 1))


@capi("colminmax[300x3-partial-and-final]", "beast_colminmax_f32")
def _(dev):
    xg = np.random.default_rng(8).standard_normal((300, 3)).astype(F32)
    good = dv(xg, dev)
    x = buf_like(good)
    lib = _lib.load()
    ws = torch.empty(lib.beast_colminmax_workspace_bytes(300, 3), dtype=torch.uint8, device=dev)
    mn, mx = (torch.empty(3, dtype=torch.float32, device=dev) for _ in range(2))

    def call(h):
        run("beast_colminmax_f32", x.data_ptr(), 300, 3, 3, mn.data_ptr(), mx.data_ptr(), ws.data_ptr(), ws.numel(), h)
        return [mn, mx]

    def check(exp):
        assert np.array_equal(npy(exp[0]), xg.min(0)) and np.array_equal(npy(exp[1]), xg.max(0))
    return Case("colminmax", ("beast_colminmax_f32",), [(x, good, (good * 0.5).contiguous())], call,
                scratch=[mn, mx, ws], check_expected=check)


# ============================================================================ A. quantiles ==
def quantile_case(dev, form, radix):
    rows, cols, qs = 300, 3, [0.01, 0.99]
    xg = np.random.default_rng(radix).standard_normal((rows, cols)).astype(F32)
    good = dv(xg, dev)
    stale = (good * 0.5 + 1).contiguous()
    x = buf_like(good)
    lib = _lib.load()
    ws = torch.empty(lib.beast_quantile_workspace_bytes(rows, cols, 2), dtype=torch.uint8, device=dev)
    outb = torch.empty((2, cols), dtype=torch.float32, device=dev)
    qh = (ctypes.c_float * 2)(*qs)
    qp = ctypes.cast(qh, ctypes.c_void_p)             # host_q is read on the host, inside the call
    seg = None
    if form == "segments":    # {ptr, first_row, row_stride} of two row blocks of the one buffer: never stale
        seg = dv(np.array([x.data_ptr(), 0, cols, x[200:].data_ptr(), 200, cols], dtype=np.uint64).view(np.int64), dev)

    def call(h, _keep=qh):
        if form == "f32":
            run("beast_quantile_f32", x.data_ptr(), rows, cols, cols, 2, qp, outb.data_ptr(), ws.data_ptr(),
                ws.numel(), h)
            return [outb]
        if form == "segments":
            run("beast_quantile_prepare_segments", seg.data_ptr(), 2, 200, rows, cols, rows, 2, qp, ws.data_ptr(),
                ws.numel(), h)
        else:
            run("beast_quantile_prepare", x.data_ptr(), rows, cols, cols, rows, 2, qp, ws.data_ptr(), ws.numel(), h)
        for ps in range(lib.beast_quantile_passes(radix)):
            run("beast_quantile_hist", ps, rows, cols, 2, radix, ws.data_ptr(), h)
            run("beast_quantile_select", ps, cols, 2, radix, ws.data_ptr(), h)
        run("beast_quantile_finalize", cols, 2, ws.data_ptr(), outb.data_ptr(), h)
        return [outb]

    def check(exp):   # exact: numpy 'linear' quantiles in float32 (test_prop_column_quantiles_equal_numpy)
        assert np.array_equal(npy(exp[0]), np.stack([np.quantile(xg, F32(q), axis=0) for q in qs]).astype(F32))
    return Case(f"quantile[{form}-radix{radix}]", QUANTILE_ENTRIES[form], [(x, good, stale)], call, scratch=[ws, outb],
                check_expected=check)


QUANTILE_ENTRIES = {
    "f32": ("beast_quantile_f32",),
    "segments": ("beast_quantile_prepare_segments", "beast_quantile_hist", "beast_quantile_select",
                 "beast_quantile_finalize"),
    "chain": ("beast_quantile_prepare", "beast_quantile_hist", "beast_quantile_select", "beast_quantile_finalize"),
}
for _form, _radix in (("chain", 11), ("chain", 7), ("segments", 11), ("segments", 7), ("f32", 11)):
    capi(f"quantile[{_form}-radix{_radix}-300x3]", *QUANTILE_ENTRIES[_form])(
        lambda dev, form=_form, radix=_radix: quantile_case(dev, form, radix))


# ============================================================================ A. BPE codec ==
def bpe_model(dev):
    """The smallest trained model of tests/golden/bpe_codec.json (runs/300: 240 merges) and 40 of its
    rows cut to ragged lengths; the yardstick is HF itself on the same rows."""
    if "bpe_model" not in _CTX:
        from test_gpu_bpe_codec import CODEC, hf_tokenizer
        from beast_tokenizer_amd.bpe_codec import GpuBpeModel, rows_from_sequences
        spec = CODEC["runs/300"]
        hf = hf_tokenizer(spec)
        model = GpuBpeModel(hf, dev)
        lens = [60, 37, 1, 13, 59, 2, 44, 8]
        rows = [np.asarray(cps[:lens[i % 8]], dtype=np.int64) for i, (cps, _) in enumerate(spec["encode"][:40])]
        want = [hf.encode("".join(map(chr, r)), add_special_tokens=False).ids for r in rows]
        flat, off, width = rows_from_sequences(rows, dev)
        torch.cuda.synchronize(dev)
        _CTX["bpe_model"] = (model, hf, spec, rows, want, flat, off, width)
    return _CTX["bpe_model"]


def ragged(ids, lens):
    ids, lens = npy(ids), npy(lens)
    return [ids[i, :lens[i]].tolist() for i in range(len(lens))]


def bpe_encode_case(dev, entry):
    model, hf, spec, rows, want, flat, off, width = bpe_model(dev)
    R = len(rows)
    tok = buf_like(flat)
    ids = torch.empty((R, width), dtype=torch.int32, device=dev)
    st = torch.empty((2, R), dtype=torch.int32, device=dev)
    m = model
    built = entry == "beast_bpe_mergemap_build"
    if built:   # the merges in rank order, and a map of this case's own
        mdl = json.loads(hf._tokenizer.to_str())["model"]
        vocab = mdl["vocab"]
        pairs = [mm.split(" ", 1) if isinstance(mm, str) else mm for mm in mdl["merges"]]
        abn = np.array([[vocab[a] for a, b in pairs], [vocab[b] for a, b in pairs], [vocab[a + b] for a, b in pairs]],
                       dtype=np.int32)
        mg_good = dv(abn, dev)
        mg = buf_like(mg_good)
        mapb = torch.empty_like(m.map)

    def call(h):
        mp = m.map
        if built:
            run("beast_bpe_mergemap_build", mg[0].data_ptr(), mg[1].data_ptr(), mg[2].data_ptr(), m.n_merges,
                mapb.data_ptr(), mapb.numel(), h)
            mp = mapb
        if entry == "beast_bpe_encode_rows_words":
            run(entry, tok.data_ptr(), off.data_ptr(), R, 0, -1, m.lut.data_ptr(), m.lut.numel(), m.byte2id.data_ptr(),
                m.wordmap.data_ptr(), m.wordmap_log2b, m.unk_id, m.fuse_unk, width, width, ids.data_ptr(), width,
                st[0].data_ptr(), st[1].data_ptr(), h)
        else:
            run("beast_bpe_encode_rows", tok.data_ptr(), off.data_ptr(), R, 0, -1, m.lut.data_ptr(), m.lut.numel(),
                m.byte2id.data_ptr(), mp.data_ptr(), m.n_merges, m.spec_cps.data_ptr(), m.spec_len.data_ptr(),
                m.spec_id.data_ptr(), m.n_spec, m.unk_id, m.fuse_unk, width, width, ids.data_ptr(), width,
                st[0].data_ptr(), st[1].data_ptr(), h)
        return [ids, st]

    def canon(res):   # the ids past a row's length are not written
        idt, stt = res
        mask = torch.arange(width, device=idt.device)[None, :] < stt[0][:, None]
        return [torch.where(mask, idt, torch.full_like(idt, -1)), stt]

    def check(exp):
        assert not npy(exp[1])[1].any()
        assert ragged(exp[0], exp[1][0]) == want
    inputs = [(tok, flat, flat.flip(0).contiguous())]
    scratch = [ids, st]
    if built:
        inputs.append((mg, mg_good, mg_good.flip(1).contiguous()))     # the merges in reverse rank order
        scratch.append(mapb)
    return Case(entry, (entry,) + (("beast_bpe_encode_rows",) if built else ()), inputs, call, scratch=scratch,
                canon=canon, check_expected=check)


capi("bpe_encode_rows[runs300-40-ragged-rows]", "beast_bpe_encode_rows")(
    lambda dev: bpe_encode_case(dev, "beast_bpe_encode_rows"))
capi("bpe_encode_rows_words[runs300-40-ragged-rows]", "beast_bpe_encode_rows_words")(
    lambda dev: bpe_encode_case(dev, "beast_bpe_encode_rows_words"))
capi("bpe_mergemap_build[240-merges-then-encode_rows]", "beast_bpe_mergemap_build", "beast_bpe_encode_rows")(
    lambda dev: bpe_encode_case(dev, "beast_bpe_mergemap_build"))


@capi("bpe_mergemap_build[no-merges-clear-only]", "beast_bpe_mergemap_build")
def _(dev):
    lib = _lib.load()
    mapb = torch.empty(int(lib.beast_bpe_mergemap_bytes(0)), dtype=torch.uint8, device=dev)
    cap = 1 << lib.beast_bpe_mergemap_log2cap(0)

    def call(h):
        run("beast_bpe_mergemap_build", None, None, None, 0, mapb.data_ptr(), mapb.numel(), h)
        return [mapb[:8 * cap]]               # the key / value slots k_mergemap_clear writes
    return Case("mergemap_clear", ("beast_bpe_mergemap_build",), [], call, scratch=[mapb])


@capi("bpe_decode_rows[runs300-40-ragged-rows]", "beast_bpe_decode_rows")
def _(dev):
    from beast_tokenizer_amd.bpe_codec import ids_as_i32, rows_from_sequences
    model, hf, spec = bpe_model(dev)[:3]
    dec = spec["decode"][:40]
    seqs = [ids_as_i32(np.asarray(ids, dtype=np.int64)).reshape(-1) for ids, _ in dec]
    want = [cps for _, cps in dec]
    flat, off, _ = rows_from_sequences(seqs, dev, dtype=np.int32)
    R, L = len(seqs), max(len(w) for w in want) + 1
    idb = buf_like(flat)
    outb = torch.empty((R, L), dtype=torch.int64, device=dev)
    st = torch.empty((2, R), dtype=torch.int32, device=dev)
    m = model

    def call(h):
        run("beast_bpe_decode_rows", idb.data_ptr(), off.data_ptr(), R, m.tok_off.data_ptr(), m.tok_bytes.data_ptr(),
            m.tok_skip.data_ptr(), m.n_vocab, m.decode_unk_id, 0, L, outb.data_ptr(), st[0].data_ptr(),
            st[1].data_ptr(), h)
        return [outb, st]

    def canon(res):
        o, s = res
        mask = torch.arange(L, device=o.device)[None, :] < s[0][:, None]
        return [torch.where(mask, o, torch.full_like(o, -1)), s]

    def check(exp):   # the HF golden
        assert npy(exp[1])[0].tolist() == [len(w) for w in want]
        assert ragged(exp[0], exp[1][0]) == want
    return Case("bpe_decode_rows", ("beast_bpe_decode_rows",), [(idb, flat, flat.flip(0).contiguous())], call,
                scratch=[outb, st], canon=canon, check_expected=check)


# ============================================================================ A. BPE setup ==
def bpe_setup(dev):
    """A few hundred synthetic rows (as test_bpe_dedup_and_compact_match_counter builds them, plus
    spaces for more words) taken through every setup stage once, synchronously, on the null stream:
    each case below gets complete inputs for its one entry point.

    Stale contents keep every structure: the stale tokens swap neighbouring code points of one
    pre-tokeniser class and one UTF-8 length (a bijection, no apostrophe in the corpus, so the words
    have the same extents and the same number of distinct ones); the stale symbols are the ids
    mirrored inside the alphabet, at the words' positions only."""
    if "bpe" in _CTX:
        return _CTX["bpe"]
    from beast_tokenizer_amd.bpe_train import GpuBpeOps, build_alphabet, fixed_rows_to_device
    from beast_tokenizer_amd.pretok import class_lut
    rng = np.random.default_rng(11)
    base = rng.integers(0, 300, size=9)
    arr = base[rng.integers(0, 9, size=(300, 40))]
    arr[::7] = rng.integers(0, 300, size=(arr[::7].shape[0], 40))
    arr[::3, ::5] = 32
    arr[arr == 39] = 40
    lut = class_lut(300)
    ulen = np.where(np.arange(300) < 128, 1, 2)
    swap = np.arange(300)
    for v in range(0, 298, 2):
        if lut[v] == lut[v + 1] and ulen[v] == ulen[v + 1] and 39 not in (v, v + 1):
            swap[v], swap[v + 1] = v + 1, v
    arr_stale = swap[arr]
    present = np.zeros(300, dtype=bool)
    present[np.unique(arr)] = True
    present[np.unique(arr_stale)] = True
    id2str, str2id, byte2id = build_alphabet(present, [chr(i) for i in range(300)], [])
    flat, off = fixed_rows_to_device(dv(arr.astype(np.int64), dev))
    flat_stale, _ = fixed_rows_to_device(dv(arr_stale.astype(np.int64), dev))
    ops = GpuBpeOps(dev)
    w = ops.pretokenize(flat, off, 0, lut, byte2id)
    ws_ = ops.pretokenize(flat_stale, off, 0, lut, byte2id)
    assert w["n_words"] == ws_["n_words"] and torch.equal(w["wstart"], ws_["wstart"]) \
        and torch.equal(w["wlen"], ws_["wlen"]), "the stale corpus must keep the words' extents"
    u = ops.dedup(w)                                  # distinct words, repacked, with signatures
    assert ops.dedup(ws_)["n_words"] == u["n_words"], "the stale corpus must have as many distinct words"
    n_tok = len(id2str)

    def mirrored(sym, wstart, wlen, n):
        """the ids mirrored inside [0, n_tok) at the words' positions; the padding stays"""
        s = npy(sym).astype(np.int64)
        mask = np.zeros(s.shape, dtype=bool)
        for a, k in zip(npy(wstart)[:n].tolist(), npy(wlen)[:n].tolist()):
            mask[a:a + k] = True
        return dv(np.where(mask, n_tok - 1 - s, s).astype(np.int16), dev)
    lut_d, b2i = ops._upload_luts(lut, byte2id)
    torch.cuda.synchronize(dev)
    _CTX["bpe"] = dict(arr=arr, arr_stale=arr_stale, lut=lut, lut_d=lut_d, b2i=b2i, byte2id=byte2id, id2str=id2str,
                       flat=flat, flat_stale=flat_stale, off=off, ops=ops, w=w, u=u, n_tok=n_tok, mirrored=mirrored,
                       S=arr.shape[0])
    return _CTX["bpe"]


def words_of(sym, wstart, wlen, n):
    s, a, k = npy(sym).view(np.uint16), npy(wstart), npy(wlen)
    return [tuple(s[a[i]:a[i] + k[i]].tolist()) for i in range(n)]


def word_table(words, counts, extra=()):
    """An order-free form of (word, count) lists: sorted, padded, as one int64 tensor."""
    rows = sorted((len(w),) + tuple(w) + (int(c),) for w, c in zip(words, counts))
    width = max((len(r) for r in rows), default=1)
    flat = [v for r in rows for v in r + (-1,) * (width - len(r))]
    return torch.tensor(list(extra) + flat, dtype=torch.int64)


@capi("i64_minmax[12000-tokens]", "beast_i64_minmax")
def _(dev):
    c = bpe_setup(dev)
    tok, out2 = buf_like(c["flat"]), torch.empty(2, dtype=torch.int64, device=dev)

    def call(h):
        run("beast_i64_minmax", tok.data_ptr(), tok.numel(), out2.data_ptr(), h)
        return [out2]

    def check(exp):
        assert npy(exp[0]).tolist() == [int(c["arr"].min()), int(c["arr"].max())]
    return Case("i64_minmax", ("beast_i64_minmax",), [(tok, c["flat"], c["flat"] + 1000)], call, scratch=[out2],
                check_expected=check)


def presence_case(dev, n):
    c = bpe_setup(dev)
    tok, pr = buf_like(c["flat"]), torch.empty(300, dtype=torch.uint8, device=dev)

    def call(h):
        run("beast_bpe_cp_presence", tok.data_ptr(), n, 0, pr.data_ptr(), 300, h)
        return [pr]

    def check(exp):
        want = np.zeros(300, dtype=np.uint8)
        if n:
            want[np.unique(c["arr"])] = 1
        assert np.array_equal(npy(exp[0]), want)
    # stale: the lower half of the range only (the swapped corpus has the same code points present)
    return Case(f"cp_presence[n{n}]", ("beast_bpe_cp_presence",), [(tok, c["flat"], c["flat"] % 150)] if n else [],
                call, scratch=[pr], check_expected=check)


capi("bpe_cp_presence[memset-then-kernel]", "beast_bpe_cp_presence")(lambda dev: presence_case(dev, 12000))
capi("bpe_cp_presence[n0-memset-only]", "beast_bpe_cp_presence")(lambda dev: presence_case(dev, 0))


@capi("bpe_pretok_count[300-rows]", "beast_bpe_pretok_count")
def _(dev):
    c = bpe_setup(dev)
    S = c["S"]
    tok = buf_like(c["flat"])
    wps, sps = (torch.empty(S, dtype=torch.int64, device=dev) for _ in range(2))
    stale = c["flat"].reshape(S, -1).flip(0).reshape(-1).contiguous()      # the rows in reverse order

    def call(h):
        run("beast_bpe_pretok_count", tok.data_ptr(), c["off"].data_ptr(), S, 0, c["lut_d"].data_ptr(), c["lut_d"].numel(),
            wps.data_ptr(), sps.data_ptr(), h)
        return [wps, sps]

    def check(exp):   # the emit pass' totals, and the UTF-8 bytes of every row
        assert int(exp[0].sum()) == c["w"]["n_words"] and int(exp[1].sum()) == c["w"]["n_syms"]
        assert np.array_equal(npy(exp[1]), np.where(c["arr"] < 128, 1, 2).sum(1))
    return Case("pretok_count", ("beast_bpe_pretok_count",), [(tok, c["flat"], stale)], call, scratch=[wps, sps],
                check_expected=check)


@capi("exclusive_scan_i64[n2500-two-levels]", "beast_exclusive_scan_i64")
def _(dev):
    n = 2500                                              # three tiles of 1,024: a second scan level
    xg = np.random.default_rng(2).integers(0, 50, size=n)
    good = dv(xg, dev)
    x, outb = buf_like(good), torch.empty(n + 1, dtype=torch.int64, device=dev)
    ws = torch.empty(_lib.load().beast_scan_workspace_bytes(n), dtype=torch.uint8, device=dev)

    def call(h):
        run("beast_exclusive_scan_i64", x.data_ptr(), outb.data_ptr(), n, ws.data_ptr(), h)
        return [outb]
    return Case("exclusive_scan", ("beast_exclusive_scan_i64",), [(x, good, flip_rows(good))], call, scratch=[outb, ws],
                check_expected=lambda e: np.testing.assert_array_equal(npy(e[0]), np.concatenate([[0], np.cumsum(xg)])))


@capi("bpe_pretok_emit[300-rows]", "beast_bpe_pretok_emit")
def _(dev):
    c = bpe_setup(dev)
    S, w = c["S"], c["w"]
    tok = buf_like(c["flat"])
    wps, sps = (torch.empty(S, dtype=torch.int64, device=dev) for _ in range(2))
    run("beast_bpe_pretok_count", c["flat"].data_ptr(), c["off"].data_ptr(), S, 0, c["lut_d"].data_ptr(), c["lut_d"].numel(),
        wps.data_ptr(), sps.data_ptr(), None)
    z = torch.zeros(1, dtype=torch.int64, device=dev)
    woff, soff = torch.cat([z, wps.cumsum(0)]), torch.cat([z, sps.cumsum(0)])     # offset tables: never stale
    torch.cuda.synchronize(dev)
    sym, ws_, wl = buf_like(w["sym"]), buf_like(w["wstart"]), buf_like(w["wlen"])

    def call(h):
        run("beast_bpe_pretok_emit", tok.data_ptr(), c["off"].data_ptr(), S, 0, c["lut_d"].data_ptr(), c["lut_d"].numel(),
            woff.data_ptr(), soff.data_ptr(), c["b2i"].data_ptr(), sym.data_ptr(), ws_.data_ptr(), wl.data_ptr(), h)
        return [sym, ws_, wl]

    def check(exp):   # the symbols are the rows' UTF-8 bytes through byte2id
        want = np.concatenate([c["byte2id"][list("".join(map(chr, r)).encode("utf-8"))] for r in c["arr"]])
        assert np.array_equal(npy(exp[0]).view(np.uint16)[:w["n_syms"]], want.astype(np.uint16))
        assert int(npy(exp[2])[:w["n_words"]].sum()) == w["n_syms"]
    return Case("pretok_emit", ("beast_bpe_pretok_emit",), [(tok, c["flat"], c["flat_stale"])], call,
                scratch=[sym, ws_, wl], check_expected=check)


def pair_counts(words, counts, V):
    t = np.zeros((V, V), dtype=np.int64)
    for w, k in zip(words, counts):
        for a, b in zip(w[:-1], w[1:]):
            t[a, b] += k
    return t


def count_pairs_case(dev, Vt, n_sym, branch):
    c = bpe_setup(dev)
    u = c["u"]
    n = u["n_words"]
    good = u["sym"]
    stale = c["mirrored"](good, u["wstart"], u["wlen"], n)
    sym = buf_like(good)
    table = torch.empty(Vt * Vt, dtype=torch.int32, device=dev)

    def call(h):
        run("beast_bpe_count_pairs", sym.data_ptr(), u["wstart"].data_ptr(), u["wlen"].data_ptr(),
            u["wcount"].data_ptr(), n, table.data_ptr(), Vt, n_sym, h)
        return [table]

    def check(exp):
        want = pair_counts(words_of(good, u["wstart"], u["wlen"], n), npy(u["wcount"])[:n].tolist(), Vt)
        assert np.array_equal(npy(exp[0]).reshape(Vt, Vt), want)
    # the table is "+=": the caller zero-fills it
    return Case(f"count_pairs[{branch}]", ("beast_bpe_count_pairs",), [(sym, good, stale)], call, scratch=[table],
                setup=table.zero_, check_expected=check)


@capi("bpe_count_pairs[n_sym-small-LDS-kernel]", "beast_bpe_count_pairs")
def _(dev):
    n_tok = bpe_setup(dev)["n_tok"]
    assert (n_tok + min(n_tok, 160 * 1024 // (4 * n_tok)) - 1) // min(n_tok, 160 * 1024 // (4 * n_tok)) <= 16
    return count_pairs_case(dev, n_tok, n_tok, "lds")


@capi("bpe_count_pairs[n_sym-1000-global-kernel]", "beast_bpe_count_pairs")
def _(dev):
    assert (1000 + 40 - 1) // 40 > 16                     # 25 row groups of 40: past the LDS kernel's 16
    return count_pairs_case(dev, 1000, 1000, "global")


@capi("bpe_word_signatures[distinct-words]", "beast_bpe_word_signatures")
def _(dev):
    c = bpe_setup(dev)
    u = c["u"]
    n = u["n_words"]
    sym, sig = buf_like(u["sym"]), torch.empty(n, dtype=torch.int64, device=dev)

    def call(h):
        run("beast_bpe_word_signatures", sym.data_ptr(), u["wstart"].data_ptr(), u["wlen"].data_ptr(), n,
            sig.data_ptr(), h)
        return [sig]

    def check(exp):   # GpuBpeOps._loop_words computed the same signatures for the merge loop (pinned to HF's merges)
        assert torch.equal(exp[0], u["sig"][:n])
    return Case("word_signatures", ("beast_bpe_word_signatures",),
                [(sym, u["sym"], c["mirrored"](u["sym"], u["wstart"], u["wlen"], n))], call, scratch=[sig],
                check_expected=check)


@capi("bpe_dedup_words[memsets-insert-gather]", "beast_bpe_dedup_words")
def _(dev):
    from collections import Counter
    c = bpe_setup(dev)
    w = c["w"]
    n = w["n_words"]
    good = w["sym"]
    sym = buf_like(good)
    ws = torch.empty(_lib.load().beast_bpe_dedup_workspace_bytes_safe(n), dtype=torch.uint8, device=dev)
    ow, ol, oc = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    on = torch.empty(1, dtype=torch.int64, device=dev)

    def call(h):
        run("beast_bpe_dedup_words", sym.data_ptr(), w["wstart"].data_ptr(), w["wlen"].data_ptr(), n, ws.data_ptr(),
            ws.numel(), ow.data_ptr(), ol.data_ptr(), oc.data_ptr(), on.data_ptr(), h)
        return [ow, ol, oc, on]

    def canon(res):   # the output order is unspecified: the distinct words by content, with their counts
        k = int(res[3])
        assert 0 <= k <= n
        return [word_table(words_of(sym, res[0], res[1], k), npy(res[2])[:k].tolist(), extra=(k,))]

    def check(exp):
        want = Counter(x for x in words_of(good, w["wstart"], w["wlen"], n) if len(x) >= 2)
        assert SO.bits_equal(exp[0], word_table(list(want), list(want.values()), extra=(len(want),)))
    return Case("dedup_words", ("beast_bpe_dedup_words",),
                [(sym, good, c["mirrored"](good, w["wstart"], w["wlen"], n))], call, scratch=[ws, ow, ol, oc, on],
                canon=canon, check_expected=check)


def repack_case(dev, empty):
    c = bpe_setup(dev)
    w, u = c["w"], c["u"]
    n = 0 if empty else u["n_words"]
    lib = _lib.load()
    good = u["sym"]
    sym = buf_like(good)
    cnt_good = u["wcount"]
    cnt = buf_like(cnt_good)
    ws = torch.empty(lib.beast_bpe_repack_workspace_bytes(n), dtype=torch.uint8, device=dev)
    sym2 = torch.empty(good.numel() + 3 * max(n, 1), dtype=torch.int16, device=dev)
    w2, l2, c2 = (torch.empty(max(n, 1), dtype=torch.int32, device=dev) for _ in range(3))
    on = torch.empty(1, dtype=torch.int64, device=dev)

    def call(h):
        run("beast_bpe_repack_words", sym.data_ptr(), u["wstart"].data_ptr(), u["wlen"].data_ptr(), cnt.data_ptr(), n,
            ws.data_ptr(), ws.numel(), sym2.data_ptr(), w2.data_ptr(), l2.data_ptr(), c2.data_ptr(), on.data_ptr(), h)
        return [on] if empty else [sym2, w2, l2, c2, on]

    def canon(res):   # the order inside a length bucket is unspecified
        if empty:
            return res
        return [word_table(words_of(res[0], res[1], res[2], n), npy(res[3])[:n].tolist(), extra=(int(res[4]),))]

    def check(exp):
        if empty:
            assert int(exp[0]) == 0
            return
        lens = npy(u["wlen"])[:n].astype(np.int64)
        want = word_table(words_of(good, u["wstart"], u["wlen"], n), npy(cnt_good)[:n].tolist(),
                          extra=(int(((lens + 3) // 4 * 4).sum()),))
        assert SO.bits_equal(exp[0], want)
    inputs = [] if empty else [(sym, good, c["mirrored"](good, u["wstart"], u["wlen"], n)), (cnt, cnt_good, cnt_good + 1)]
    return Case(f"repack_words[n{n}]", ("beast_bpe_repack_words",), inputs, call,
                scratch=[ws, on] if empty else [ws, sym2, w2, l2, c2, on], canon=canon, check_expected=check)


capi("bpe_repack_words[memset-six-kernels]", "beast_bpe_repack_words")(lambda dev: repack_case(dev, False))
capi("bpe_repack_words[n0-two-memsets]", "beast_bpe_repack_words")(lambda dev: repack_case(dev, True))


def compact_case(dev, empty):
    c = bpe_setup(dev)
    u = c["u"]
    n = 0 if empty else u["n_words"]
    wl = u["wlen"].clone()
    wl[::3] = 1
    wl[1::5] = 0
    cnt_good = u["wcount"]
    cnt = buf_like(cnt_good)
    ow, ol, oc = (torch.empty(max(n, 1), dtype=torch.int32, device=dev) for _ in range(3))
    on = torch.empty(1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)

    def call(h):
        run("beast_bpe_compact_words", u["wstart"].data_ptr(), wl.data_ptr(), cnt.data_ptr(), n, ow.data_ptr(),
            ol.data_ptr(), oc.data_ptr(), on.data_ptr(), h)
        return [on] if empty else [ow, ol, oc, on]

    def canon(res):   # "order unspecified"
        if empty:
            return res
        k = int(res[3])
        assert 0 <= k <= n
        rows = sorted(zip(npy(res[0])[:k].tolist(), npy(res[1])[:k].tolist(), npy(res[2])[:k].tolist()))
        return [torch.tensor([k] + [v for r in rows for v in r], dtype=torch.int64)]

    def check(exp):
        if empty:
            assert int(exp[0]) == 0
            return
        keep = sorted((a, k, q) for a, k, q in zip(npy(u["wstart"])[:n].tolist(), npy(wl)[:n].tolist(),
                                                   npy(cnt_good)[:n].tolist()) if k >= 2)
        assert exp[0].tolist() == [len(keep)] + [v for r in keep for v in r]
    return Case(f"compact_words[n{n}]", ("beast_bpe_compact_words",), [] if empty else [(cnt, cnt_good, cnt_good + 1)],
                call, scratch=[on] if empty else [ow, ol, oc, on], canon=canon, check_expected=check)


capi("bpe_compact_words[memset-then-kernel]", "beast_bpe_compact_words")(lambda dev: compact_case(dev, False))
capi("bpe_compact_words[n0-memset-only]", "beast_bpe_compact_words")(lambda dev: compact_case(dev, True))


@capi("bpe_pretok_dedup+repack[two-memsets-256-and-512-kernels-compact-copy-then-repack]",
      "beast_bpe_pretok_dedup", "beast_bpe_pretok_dedup_repack")
def _(dev):
    """The one-pass setup as beast_bpe_train chains it.  The <256> and <512> kernels are both
    launched whatever the rows hold (the host does not branch on it), so one sequence covers them.
    n_distinct is the good corpus' (the stale one has as many: its code points are a bijection)."""
    from collections import Counter
    c = bpe_setup(dev)
    S, u = c["S"], c["u"]
    nu = u["n_words"]
    lib = _lib.load()
    tok = buf_like(c["flat"])
    ws = torch.empty(lib.beast_bpe_pretok_dedup_workspace_bytes(tok.numel()), dtype=torch.uint8, device=dev)
    info = torch.empty(4, dtype=torch.int64, device=dev)
    rws = torch.empty(lib.beast_bpe_repack_workspace_bytes(nu) + 8 * (nu + 1), dtype=torch.uint8, device=dev)
    sym2 = torch.empty(c["w"]["n_syms"] + 3 * nu, dtype=torch.int16, device=dev)
    w2, l2, c2 = (torch.empty(nu, dtype=torch.int32, device=dev) for _ in range(3))
    on = torch.empty(1, dtype=torch.int64, device=dev)

    def call(h):
        run("beast_bpe_pretok_dedup", tok.data_ptr(), c["off"].data_ptr(), S, 0, c["lut_d"].data_ptr(), c["lut_d"].numel(),
            ws.data_ptr(), ws.numel(), info.data_ptr(), h)
        run("beast_bpe_pretok_dedup_repack", tok.data_ptr(), 0, c["b2i"].data_ptr(), ws.data_ptr(), ws.numel(), nu,
            rws.data_ptr(), rws.numel(), sym2.data_ptr(), w2.data_ptr(), l2.data_ptr(), c2.data_ptr(), on.data_ptr(), h)
        return [info, sym2, w2, l2, c2, on]

    def canon(res):
        assert res[0].tolist()[0] == nu and res[0].tolist()[3] == 0
        return [res[0], word_table(words_of(res[1], res[2], res[3], nu), npy(res[4])[:nu].tolist(), extra=(int(res[5]),))]

    def check(exp):   # the two-pass pipeline's distinct words x counts (test_bpe_pretok_dedup_equals_two_pass)
        assert exp[0].tolist() == [nu, c["w"]["n_words"], c["w"]["n_syms"], 0]
        lens = npy(u["wlen"])[:nu].astype(np.int64)
        want = word_table(words_of(u["sym"], u["wstart"], u["wlen"], nu), npy(u["wcount"])[:nu].tolist(),
                          extra=(int(((lens + 3) // 4 * 4).sum()),))
        assert SO.bits_equal(exp[1], want)
        assert len(Counter(words_of(u["sym"], u["wstart"], u["wlen"], nu))) == nu
    return Case("pretok_dedup+repack", ("beast_bpe_pretok_dedup", "beast_bpe_pretok_dedup_repack"),
                [(tok, c["flat"], c["flat_stale"])], call, scratch=[ws, info, rws, sym2, w2, l2, c2, on], canon=canon,
                check_expected=check)


@capi("bpe_pretok_dedup+repack[n0-memsets-and-info-copy-only]", "beast_bpe_pretok_dedup", "beast_bpe_pretok_dedup_repack")
def _(dev):
    """No sequences, no distinct words: two memsets and the device-to-device copy of the info block,
    then the repack's two memsets; no kernel runs and nothing is read."""
    c = bpe_setup(dev)
    lib = _lib.load()
    ws = torch.empty(lib.beast_bpe_pretok_dedup_workspace_bytes(0), dtype=torch.uint8, device=dev)
    info = torch.empty(4, dtype=torch.int64, device=dev)
    rws = torch.empty(lib.beast_bpe_repack_workspace_bytes(0) + 8, dtype=torch.uint8, device=dev)
    one16 = torch.empty(4, dtype=torch.int16, device=dev)
    w2, l2, c2 = (torch.empty(1, dtype=torch.int32, device=dev) for _ in range(3))
    on = torch.empty(1, dtype=torch.int64, device=dev)

    def call(h):
        run("beast_bpe_pretok_dedup", c["flat"].data_ptr(), c["off"].data_ptr(), 0, 0, c["lut_d"].data_ptr(),
            c["lut_d"].numel(), ws.data_ptr(), ws.numel(), info.data_ptr(), h)
        run("beast_bpe_pretok_dedup_repack", c["flat"].data_ptr(), 0, c["b2i"].data_ptr(), ws.data_ptr(), ws.numel(), 0,
            rws.data_ptr(), rws.numel(), one16.data_ptr(), w2.data_ptr(), l2.data_ptr(), c2.data_ptr(), on.data_ptr(), h)
        return [info, on]

    def check(exp):
        assert exp[0].tolist() == [0, 0, 0, 0] and int(exp[1]) == 0
    return Case("pretok_dedup+repack[n0]", ("beast_bpe_pretok_dedup", "beast_bpe_pretok_dedup_repack"), [], call,
                scratch=[ws, info, rws, on], check_expected=check)


# ============================================================================= A. BPE loop ==
def bpe_loop(dev):
    """The pair table, token lengths and hashes of the distinct words above (Vt 512)."""
    if "loop" in _CTX:
        return _CTX["loop"]
    from beast_tokenizer_amd.bpe_train import token_hashes
    c = bpe_setup(dev)
    u, n_tok = c["u"], c["n_tok"]
    Vt = 512
    assert n_tok < Vt - 40
    n = u["n_words"]
    words = words_of(u["sym"], u["wstart"], u["wlen"], n)
    counts = npy(u["wcount"])[:n].tolist()
    table = pair_counts(words, counts, Vt)
    stale_sym = c["mirrored"](u["sym"], u["wstart"], u["wlen"], n)
    table_stale = pair_counts(words_of(stale_sym, u["wstart"], u["wlen"], n), counts, Vt)
    flat = table.reshape(-1)
    best = int(np.flatnonzero(flat == flat.max())[0])                # HF's tie rule: the smallest (a, b)
    tlen = np.zeros(Vt, dtype=np.int32)
    tlen[:n_tok] = [len(s) for s in c["id2str"]]
    hp = np.stack(token_hashes(c["id2str"])).view(np.int64)
    _CTX["loop"] = dict(Vt=Vt, n=n, table=dv(table.astype(np.int32).reshape(-1), dev),
                        table_stale=dv(table_stale.astype(np.int32).reshape(-1), dev), stale_sym=stale_sym,
                        a=best // Vt, b=best % Vt, count=int(flat.max()), tlen=dv(tlen, dev), hp=dv(hp, dev),
                        max_tlen=int(max(len(s) for s in c["id2str"])), np_table=table)
    torch.cuda.synchronize(dev)
    return _CTX["loop"]


def argws_of(dev, Vt):
    return torch.empty((_lib.load().beast_bpe_argmax_workspace_bytes(Vt) + 7) // 8, dtype=torch.int64, device=dev)


@capi("bpe_argmax[call0]", "beast_bpe_argmax")
def _(dev):
    c, L = bpe_setup(dev), bpe_loop(dev)
    Vt = L["Vt"]
    table, argws = buf_like(L["table"]), argws_of(dev, Vt)

    def call(h):
        run("beast_bpe_argmax", table.data_ptr(), Vt, c["n_tok"], argws.data_ptr(), 0, h)
        return [argws[2:3]]

    def check(exp):
        key = int(exp[0]) & 0xFFFFFFFFFFFFFFFF
        assert key >> 32 == L["count"] and 0xFFFFFFFF - (key & 0xFFFFFFFF) == L["a"] * Vt + L["b"]
    # ws: "zero-filled once before call 0" by the caller
    return Case("argmax", ("beast_bpe_argmax",), [(table, L["table"], L["table_stale"])], call, scratch=[argws],
                setup=argws.zero_, check_expected=check)


def merge_case(dev, pair_count, branch):
    c, L = bpe_setup(dev), bpe_loop(dev)
    u, Vt, n = c["u"], L["Vt"], L["n"]
    a, b, nid = L["a"], L["b"], c["n_tok"]
    sym, wl, sig = buf_like(u["sym"]), buf_like(u["wlen"]), buf_like(u["sig"])
    deltas = torch.empty(4 * Vt, dtype=torch.int32, device=dev)
    stale_sig = torch.empty_like(u["sig"])
    run("beast_bpe_word_signatures", L["stale_sym"].data_ptr(), u["wstart"].data_ptr(), u["wlen"].data_ptr(), n,
        stale_sig.data_ptr(), None)
    torch.cuda.synchronize(dev)

    def call(h):
        run("beast_bpe_merge", sym.data_ptr(), u["wstart"].data_ptr(), wl.data_ptr(), u["wcount"].data_ptr(), n, a, b,
            nid, L["tlen"].data_ptr(), 10000, deltas.data_ptr(), Vt, sig.data_ptr(), pair_count, h)
        return [sym, wl, deltas]

    def check(exp):   # HF Word::merge on the host: the words after the merge, and the pair-count changes
        before = words_of(u["sym"], u["wstart"], u["wlen"], n)
        after = []
        for w in before:
            o, i = [], 0
            while i < len(w):
                if i + 1 < len(w) and w[i] == a and w[i + 1] == b:
                    o.append(nid)
                    i += 2
                else:
                    o.append(w[i])
                    i += 1
            after.append(tuple(o))
        assert words_of(exp[0], u["wstart"], exp[1], n) == after
        counts = npy(u["wcount"])[:n].tolist()
        diff = pair_counts(after, counts, Vt) - pair_counts(before, counts, Vt)
        diff[a, b] = 0                                     # the merged pair itself is retired by apply_argmax
        d = npy(exp[2]).reshape(4, Vt).astype(np.int64)
        got = np.zeros((Vt, Vt), dtype=np.int64)
        got[:, a] += d[0]
        got[:, nid] += d[1]
        got[b, :] += d[2]
        got[nid, :] += d[3]
        assert np.array_equal(got, diff)
    # sym, wlen and sig are rewritten in place: inputs that are restored before every call; deltas "+="
    return Case(f"merge[{branch}]", ("beast_bpe_merge",),
                [(sym, u["sym"], L["stale_sym"]), (wl, u["wlen"], u["wlen"]), (sig, u["sig"], stale_sig)], call,
                scratch=[deltas], setup=deltas.zero_, check_expected=check)


@capi("bpe_merge[LDS-privatised-deltas]", "beast_bpe_merge")
def _(dev):
    assert _lib.load().beast_get_option(_lib.OPT_MERGE_LDS_MIN) <= 1 << 40
    return merge_case(dev, 1 << 40, "lds")


@capi("bpe_merge[direct-delta-atomics]", "beast_bpe_merge")
def _(dev):
    assert _lib.load().beast_get_option(_lib.OPT_MERGE_LDS_MIN) > 1
    return merge_case(dev, 1, "direct")


@capi("bpe_argmax+apply_argmax[call0-then-call1]", "beast_bpe_argmax", "beast_bpe_apply_argmax")
def _(dev):
    """apply_argmax continues argmax's workspace (it rescans only the rows it changed), so the two run
    as the chain the host-driven loop issues: argmax (call 0), then apply + argmax (call 1) with the
    deltas of one merge."""
    c, L = bpe_setup(dev), bpe_loop(dev)
    u, Vt, n = c["u"], L["Vt"], L["n"]
    a, b, nid = L["a"], L["b"], c["n_tok"]
    m = merge_case(dev, 1, "for-apply")
    for buf, good, _ in m.inputs:
        buf.copy_(good)
    m.setup()
    d_good = m.call(None)[2].clone()
    torch.cuda.synchronize(dev)
    table, deltas, tlen, argws = buf_like(L["table"]), buf_like(d_good), buf_like(L["tlen"]), argws_of(dev, Vt)

    def call(h):
        run("beast_bpe_argmax", table.data_ptr(), Vt, nid, argws.data_ptr(), 0, h)
        run("beast_bpe_apply_argmax", table.data_ptr(), deltas.data_ptr(), Vt, nid + 1, a, b, nid, tlen.data_ptr(),
            argws.data_ptr(), 1, h)
        return [table, deltas, tlen, argws[2:4]]

    def check(exp):
        d = npy(d_good).reshape(4, Vt).astype(np.int64)
        want = L["np_table"].copy()
        want[:, a] += d[0]
        want[:, nid] += d[1]
        want[b, :] += d[2]
        want[nid, :] += d[3]
        want[a, b] = 0
        assert np.array_equal(npy(exp[0]).reshape(Vt, Vt), want)
        assert not npy(exp[1]).any()                                       # consumed deltas are zeroed
        assert int(exp[2][nid]) == int(L["tlen"][a]) + int(L["tlen"][b])
        key = int(exp[3][1]) & 0xFFFFFFFFFFFFFFFF                          # call 1's slot
        flat = want.reshape(-1)
        assert key >> 32 == flat.max() and 0xFFFFFFFF - (key & 0xFFFFFFFF) == int(np.flatnonzero(flat == flat.max())[0])
    return Case("argmax+apply_argmax", ("beast_bpe_argmax", "beast_bpe_apply_argmax"),
                [(table, L["table"], L["table_stale"]), (deltas, d_good, torch.zeros_like(d_good)),
                 (tlen, L["tlen"], L["tlen"])], call, scratch=[argws], setup=argws.zero_, check_expected=check)


def loop_batch_case(dev, sharded):
    """beast_bpe_loop_init, then the batched loop: INIT + 3 passes (merge and apply launches), or the
    sharded form's sequence INIT / NO_APPLY / NO_MERGE with the deltas buffer between the two."""
    c, L = bpe_setup(dev), bpe_loop(dev)
    u, Vt, n, n_tok = c["u"], L["Vt"], L["n"], c["n_tok"]
    lib = _lib.load()
    vocab, max_merges = n_tok + 24, 64
    nb, bb = lib.beast_bpe_loop_workspace_bytes(Vt, max_merges), lib.beast_bpe_batch_workspace_bytes(Vt)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    bws = torch.empty(bb, dtype=torch.uint8, device=dev)
    argws = argws_of(dev, Vt)
    deltas = torch.empty(lib.beast_bpe_batch_delta_count(Vt), dtype=torch.int32, device=dev) if sharded else None
    st_p, log_p = ctypes.c_void_p(), ctypes.c_void_p()
    run("beast_bpe_loop_state", ws.data_ptr(), Vt, max_merges, ctypes.byref(st_p), ctypes.byref(log_p))
    st_off, log_off = st_p.value - ws.data_ptr(), log_p.value - ws.data_ptr()
    state = ws[st_off:st_off + 12].view(torch.int32)                  # active, vcur, n_merges
    log = ws[log_off:log_off + 16 * max_merges].view(torch.int32)
    stale_sig = torch.empty_like(u["sig"])
    run("beast_bpe_word_signatures", L["stale_sym"].data_ptr(), u["wstart"].data_ptr(), u["wlen"].data_ptr(), n,
        stale_sig.data_ptr(), None)
    torch.cuda.synchronize(dev)
    sym, wl, sig = buf_like(u["sym"]), buf_like(u["wlen"]), buf_like(u["sig"])
    table, tlen = buf_like(L["table"]), buf_like(L["tlen"])

    def batch(steps, flags, h):
        run("beast_bpe_loop_batch", ws.data_ptr(), Vt, max_merges, steps, 8, flags, sym.data_ptr(),
            u["wstart"].data_ptr(), wl.data_ptr(), u["wcount"].data_ptr(), n, tlen.data_ptr(), 10000, sig.data_ptr(),
            table.data_ptr(), argws.data_ptr(), bws.data_ptr(), bb, vocab, _lib.ptr(deltas), None, h)

    def call(h):
        run("beast_bpe_loop_init", ws.data_ptr(), nb, Vt, max_merges, n_tok, vocab, 2, L["hp"][0].data_ptr(),
            L["hp"][1].data_ptr(), tlen.data_ptr(), L["max_tlen"], h)
        if sharded:
            batch(0, _lib.BPE_BATCH_INIT, h)
            for _ in range(2):
                batch(1, _lib.BPE_BATCH_NO_APPLY, h)
                batch(1, _lib.BPE_BATCH_NO_MERGE, h)
        else:
            batch(3, _lib.BPE_BATCH_INIT, h)
        return [state, log, table, wl]

    def setup():   # "argws: zero-filled"; deltas "zero-filled once"
        argws.zero_()
        if deltas is not None:
            deltas.zero_()

    def check(exp):   # the first merge is the table's argmax, a new id; every logged merge is in HF's form
        nm = int(exp[0][_lib.BPE_STATE_NMERGES])
        lg = npy(exp[1]).reshape(-1, 4)[:nm]
        assert nm >= 1 and lg[0].tolist() == [L["a"], L["b"], n_tok, 0]
        assert int(exp[0][_lib.BPE_STATE_VCUR]) == n_tok + int((lg[:, 3] == 0).sum())
    return Case(f"loop_batch[{'sharded' if sharded else 'single'}]", ("beast_bpe_loop_init", "beast_bpe_loop_batch"),
                [(sym, u["sym"], L["stale_sym"]), (wl, u["wlen"], u["wlen"]), (sig, u["sig"], stale_sig),
                 (table, L["table"], L["table_stale"]), (tlen, L["tlen"], L["tlen"])], call,
                scratch=[ws, bws, argws] + ([deltas] if sharded else []), setup=setup, check_expected=check)


capi("bpe_loop_init+loop_batch[INIT-memset-then-3-passes]", "beast_bpe_loop_init", "beast_bpe_loop_batch")(
    lambda dev: loop_batch_case(dev, False))
capi("bpe_loop_init+loop_batch[sharded-INIT-NO_APPLY-NO_MERGE-deltas]", "beast_bpe_loop_init", "beast_bpe_loop_batch")(
    lambda dev: loop_batch_case(dev, True))


@capi("bpe_train[rand256/700-synchronous-weaker-form]", "beast_bpe_train")
def _(dev):
    """WEAKER FORM: beast_bpe_train synchronises the stream inside (it reads counts, the loop state and
    the merge log back), so the stream cannot be busy when it returns and ``busy`` is not asserted;
    the stale input and the poison still show work issued on another stream."""
    from beast_tokenizer_amd.bpe_train import fixed_rows_to_device, train_bpe_capi
    ref = load_json("bpe_hf.json")["rand256/700"]
    arr = load_npz("bpe_corpora.npz")["rand256"].astype(np.int64)
    good, off = fixed_rows_to_device(dv(arr, dev))
    stale = good.reshape(arr.shape).flip(1).reshape(-1).contiguous()      # every row backwards: same range
    tok = buf_like(good)
    saved = _lib.stream_of

    def call(h):
        _lib.stream_of = lambda device: h            # train_bpe_capi marshals the call; the handle is ours
        try:
            res = train_bpe_capi(tok, off, 700)
        finally:
            _lib.stream_of = saved
        ids = [res.vocab[a] for m in res.merges for a in m]
        return [torch.tensor([res.min_token, res.max_token, len(res.vocab)] + ids, dtype=torch.int64, device=dev)]

    def canon(res):   # the merge lists of the good and the stale corpus may differ in length
        outb = torch.full((3 + 2 * 700,), -1, dtype=torch.int64)
        outb[:res[0].numel()] = res[0].cpu()
        return [outb]

    def check(exp):
        got = exp[0].tolist()
        want = [ref["vocab"][a] for m in ref["merges"] for a in m]
        assert got[:3] == [ref["min_token"], ref["max_token"], len(ref["vocab"])] and got[3:3 + len(want)] == want
    return Case("bpe_train", ("beast_bpe_train",), [(tok, good, stale)], call, canon=canon, check_expected=check,
                synchronous=True)


@pytest.mark.parametrize("cid", SO.ids(CASES, __name__))
def test_capi_is_ordered_on_the_given_stream(cid, gpu_device):
    SO.check_capi(cid, gpu_device)


# ================================================================== B. the Python API ==
def api_tok(dev, cls=BEASTBsplineTokenizer, **kw):
    g = load_npz("bspline_k3.npz")
    tok = cls(device=str(dev), **CONFIGS["k3"], **kw)
    tok.load_state_dict({"w_min": g["w_min"].tolist(), "w_max": g["w_max"].tolist()})
    return tok, g


def api_case(name, x_good, x_stale, fn, check=None, equal=SO.bits_equal):
    x = buf_like(x_good)
    return Case(name, (name,), [(x, x_good, x_stale)], lambda h: fn(x), check_expected=check, equal=equal)


def encode_api(dev, fast):
    tok, g = api_tok(dev)
    p = tok._plan()
    assert p.fast is not None and p.fast_enc is not None, "fast path not built / not loaded"
    if not fast:
        p.fast = p.fast_enc = p.fast_rec = None          # the Python / ctypes path, as
        # test_host_fastpath_equals_python_path toggles it
    good = trajectories(17, dev)
    lay = O.Layout.make(14, [6, 13], True)

    def fn(x):
        t, d = tok.encode(x)
        return [t, d["params"]]

    def check(exp):
        check_params(npy(good), npy(exp[1]), g, lay)
        check_tokens(npy(exp[1]), npy(exp[0]), g)
    return api_case(f"encode[{'fastpath' if fast else 'ctypes'}]", good, flip_rows(good), fn, check)


api("encode[fastpath]")(lambda dev: encode_api(dev, True))
api("encode[ctypes]")(lambda dev: encode_api(dev, False))


@api("encode_continuous")
def _(dev):
    tok, g = api_tok(dev)
    good = trajectories(17, dev)

    def check(exp):
        check_params(npy(good), npy(exp[1]), g, O.Layout.make(14, [6, 13], True))
        lo, hi = g["w_min"], g["w_max"]
        n = (O._clamp_t(npy(exp[1]), lo, hi) - lo) / np.maximum(hi - lo, F32(1e-8)) * 2 - 1
        assert np.abs(npy(exp[0]) - n.reshape(17, 14, 10).transpose(0, 2, 1).reshape(17, 140)).max() <= 4 * 2.0 ** -23
    return api_case("encode_continuous", good, flip_rows(good),
                    lambda x: (lambda r: [r[0], r[1]["params"]])(tok.encode_continuous(x)), check)


def tokens17(dev):
    return dv(np.random.default_rng(17).integers(0, 256, size=(17, 140)), dev)


def pos_check(g, good):
    lay = O.Layout.make(14, [6, 13], True)

    def check(exp):
        want = O.reconstruct(npy(good), g["phi_joint"], g["phi_grip"], lay, g["w_min"], g["w_max"], 256)
        scale = np.maximum(1.0, np.abs(want).max(axis=(1, 2), keepdims=True))
        assert (np.abs(npy(exp[0]) - want) / scale).max() <= 1e-5
    return check


def reconstruct_api(dev, fast):
    tok, g = api_tok(dev)
    p = tok._plan()
    if not fast:
        p.fast = p.fast_enc = p.fast_rec = None
    good = tokens17(dev)
    return api_case(f"reconstruct_traj[{'fastpath' if fast else 'ctypes'}]", good, flip_rows(good),
                    lambda t: [tok.reconstruct_traj(t)], pos_check(g, good))


api("reconstruct_traj[fastpath]")(lambda dev: reconstruct_api(dev, True))
api("reconstruct_traj[ctypes]")(lambda dev: reconstruct_api(dev, False))


@api("reconstruct_traj_continuous[backward]")
def _(dev):
    """Forward and ``.backward()``: the backward launch asks for the current stream when autograd
    runs it (on the forward's stream), so the gradient is part of the probed sequence."""
    tok, g = api_tok(dev)
    good = (torch.rand((17, 140), device=dev, generator=torch.Generator(dev).manual_seed(3)) * 2.2 - 1.1).contiguous()
    gup = torch.randn((17, 50, 14), device=dev, generator=torch.Generator(dev).manual_seed(4))

    def fn(x):
        xr = x.detach().clone().requires_grad_()
        pos = tok.reconstruct_traj_continuous(xr)
        pos.backward(gup)
        return [pos.detach(), xr.grad]

    def check(exp):   # the oracle of tests/deriv_bwd_oracle.py on the plan's own slabs
        phi = npy(tok._constants(dev)[0])
        basis = np.zeros((3, 2, 50, 10), dtype=F32)
        basis[0] = phi
        lo, hi = g["w_min"].reshape(14, 10), g["w_max"].reshape(14, 10)
        dst = np.array(tok.joint_indices + tok.gripper_indices, dtype=np.int32)
        r = BO.backward([npy(gup), None, None], basis, lo, hi, npy(good).reshape(17, 10, 14), dst, tok.joint_dof)
        assert (np.abs(npy(exp[1]).reshape(17, 10, 14).astype(np.float64) - r.grad_ntokens) <= BO.bound(r)).all()
    return api_case("reconstruct_traj_continuous", good, flip_rows(good), fn, check)


@api("reconstruct_traj_derivs")
def _(dev):
    tok, g = api_tok(dev)
    good = tokens17(dev)
    base = pos_check(g, good)

    def check(exp):
        base(exp)
        assert not npy(exp[1])[..., [6, 13]].any() and npy(exp[1])[..., :6].any()    # gripper velocities are 0
    return api_case("reconstruct_traj_derivs", good, flip_rows(good), lambda t: list(tok.reconstruct_traj_derivs(t)),
                    check)


@api("encode_at")
def _(dev):
    tok = BEASTBsplineTokenizer(num_dof=7, num_basis=4, degree_p=3, device=str(dev))
    tok.load_state_dict({"w_min": [-3.0] * 28, "w_max": [3.0] * 28})
    B, T = 17, 9
    xg, tg = RO.random_walk(B, T, 7, 41), RO.jittered_times(B, T, 2 * np.pi, 42)
    wg = np.random.default_rng(43).uniform(0.25, 4.0, (B, T)).astype(F32)
    good = dv(xg, dev)
    td, wd = dv(tg, dev), dv(wg, dev)

    def fn(x):
        t, d = tok.encode_at(x, td, wd)
        return [t, d["params"]]

    def check(exp):
        want, _ = RO.fit(xg, tg, wg, tau=F32(tok.duration), degree=3, num_basis=4, joint_indices=tok.joint_indices,
                         gripper_indices=[])
        assert RO.parity_ok(npy(exp[1]), want).all()
        assert np.array_equal(npy(exp[0]), RO.tokens(npy(exp[1]), npy(tok.w_min), npy(tok.w_max), 256, 7, 4))
    return api_case("encode_at", good, flip_rows(good), fn, check)


@api("reconstruction_stats")
def _(dev):
    from test_gpu_roundtrip import _reference
    tok, g = api_tok(dev)
    good = trajectories(17, dev, seed=9)

    def fn(x):
        r = tok.reconstruction_stats(x, return_tokens=True)
        return [r.tokens, r.mse, r.mean_err, r.max_abs, r.mse_fit, r.clip_low, r.clip_high]

    def check(exp):   # tokens, maximum and clip counts exactly; the means within the oracle's bounds on the sums
        tokens_ref, E, s = _reference(tok, good)
        assert torch.equal(exp[0], tokens_ref)
        order = tok.joint_indices + tok.gripper_indices
        assert torch.equal(exp[3][:, order], E.abs().amax(dim=1))
        assert np.array_equal(npy(exp[5]).reshape(-1), s["clip_low"]) and np.array_equal(npy(exp[6]).reshape(-1), s["clip_high"])
        raw = np.stack([npy(exp[2]) * 50, npy(exp[1]) * 50, npy(exp[3]), npy(exp[4]) * 50], -1)[:, order]
        for k, tol in ((0, roundtrip_oracle.tol_sum_e(s)), (1, roundtrip_oracle.tol_sum_e2(s)),
                       (3, roundtrip_oracle.tol_sum_f2(s))):
            want = s[("sum_e", "sum_e2", None, "sum_f2")[k]]
            assert (np.abs(raw[..., k] - want) <= tol * (1 + 1e-6) + 2.0 ** -22 * np.abs(want)).all(), k
    return api_case("reconstruction_stats", good, flip_rows(good), fn, check)


@api("update_weights_bounds")
def _(dev):
    tok, g = api_tok(dev)
    good = trajectories(17, dev, seed=12)

    def fn(x):
        tok.update_weights_bounds(x)
        return [tok.w_min, tok.w_max]

    def check(exp):
        pr = npy(tok.compute_weights(good))
        assert np.array_equal(npy(exp[0]), pr.min(0)) and np.array_equal(npy(exp[1]), pr.max(0))
    return api_case("update_weights_bounds", good, (good * 0.5).contiguous(), fn, check)


@api("fit_parameters[quantile-path]")
def _(dev):
    tok, g = api_tok(dev)
    good = trajectories(48, dev, seed=13)

    def fn(x):
        tok.fit_parameters([{"actions": x[:24]}, {"actions": x[24:]}], verbose=False)
        return [tok.w_min, tok.w_max]

    def check(exp):
        pr = npy(tok.compute_weights(good))
        q = np.stack([np.quantile(pr, F32(v), axis=0) for v in (0.01, 0.99)]).astype(F32)
        assert np.array_equal(npy(exp[0]), q[0]) and np.array_equal(npy(exp[1]), q[1])
    return api_case("fit_parameters", good, (good * 0.5).contiguous(), fn, check)


@api("conditioned[ic2-ec2]")
def _(dev):
    tok = BEASTBsplineTokenizer(device=str(dev), init_cond_order=2, end_cond_order=2, **CONFIGS["k3"])
    good = trajectories(17, dev, seed=14)
    tok.update_weights_bounds(good)
    torch.cuda.synchronize(dev)

    def fn(x):
        t, d = tok.encode(x)
        return [t, d["params"], d["init_vel"], d["end_vel"], tok.reconstruct_traj(t)]

    def check(exp):   # test_prop_conditioned_encode_reconstruct's yardstick on the joint DoFs
        xj = npy(good)[..., tok.joint_indices]
        want_p, st_ = O.cond_fit(xj, O.times_grid(2 * np.pi, 50), F32(2 * np.pi), 4, 10, 2, 2)
        got = npy(exp[1])[:, :want_p.shape[1]]
        scale = np.maximum(1.0, np.abs(want_p).max(axis=1, keepdims=True))
        assert np.all(np.abs(got - want_p) <= 1e-5 * scale)
    return api_case("conditioned", good, flip_rows(good), fn, check)


def bpe_tokenizer(dev):
    """A BEASTBsplineBPETokenizer (k3) whose BPE model was trained on the bins of 256 trajectories."""
    if "bpe_tok" not in _CTX:
        tok, g = api_tok(dev, cls=BEASTBsplineBPETokenizer, bpe_vocab_size=400)
        tok.fit_from_trajectories([trajectories(256, dev, seed=21)], show_progress=False)
        tok._gpu_bpe()
        torch.cuda.synchronize(dev)
        _CTX["bpe_tok"] = (tok, g)
    return _CTX["bpe_tok"]


def hf_ids(tok, bins):
    """HF itself, row by row, as the reference does (beast_bspline_bpe_tokenizer.py:175-198)."""
    return [tok.bpe_tokenizer.encode("".join(chr(int(v) - tok.bpe_min_token) for v in row), add_special_tokens=False).ids
            for row in npy(bins)]


@api("bpe_tokenizer.encode[synchronous-weaker-form]")
def _(dev):
    """WEAKER FORM: the method reads the row status back (a host synchronisation of the current
    stream), so ``busy`` cannot hold; stale input and the returned ids still show mis-ordered work."""
    tok, g = bpe_tokenizer(dev)
    good = trajectories(17, dev, seed=22)

    def fn(x):
        ids, params, bins = tok.encode(x, return_tensors=True, return_mp_tokens=True)
        block = torch.full((17, 280), -1, dtype=torch.int64, device=dev)   # the id block is as wide as its longest row
        block[:, :ids.ids.shape[1]] = ids.ids
        return [block, ids.lengths, params["params"], bins]

    def check(exp):
        check_tokens(npy(exp[2]), npy(exp[3]), g)
        assert ragged(exp[0], exp[1]) == hf_ids(tok, exp[3])
    c = api_case("bpe_tokenizer.encode", good, flip_rows(good), fn, check)
    c.synchronous = True
    return c


@api("bpe_tokenizer.decode[synchronous-weaker-form]")
def _(dev):
    """WEAKER FORM (decode_checked reads the counts and status back); ids -> bins -> params."""
    tok, g = bpe_tokenizer(dev)
    lay = O.Layout.make(14, [6, 13], True)

    def ids_of(x):
        r = tok.encode(x, return_tensors=True)[0]
        block = torch.full((17, 280), 0xFFFFFFFF, dtype=torch.int64, device=dev)      # PAD_ID: skipped by decode
        block[:, :r.ids.shape[1]] = r.ids
        return block
    good_x = trajectories(17, dev, seed=22)
    good, stale = ids_of(good_x), ids_of(trajectories(17, dev, seed=23))
    bins = BEASTBsplineTokenizer.encode(tok, good_x, respect_llm_vocab_size=False)[0]
    torch.cuda.synchronize(dev)

    def check(exp):
        assert torch.equal(exp[0], bins)
        assert np.array_equal(npy(exp[1]), O.decode(npy(bins), lay, 10, g["w_min"], g["w_max"], 256))
    c = api_case("bpe_tokenizer.decode", good, stale, lambda t: [tok.bpe_to_mp_tokens(t), tok.decode(t)], check)
    c.synchronous = True
    return c


def train_case(dev, early_ops):
    """GpuBpeOps-driven training (bpe_train.train_bpe) on rand256/700, whose golden merges exist.
    WEAKER FORM: the driver reads sizes and the loop state back.  ``early_ops``: the ops object is
    constructed before the stream changes, as a long-lived trainer's would be."""
    from beast_tokenizer_amd.bpe_train import GpuBpeOps, fixed_rows_to_device, train_bpe
    ref = load_json("bpe_hf.json")["rand256/700"]
    arr = load_npz("bpe_corpora.npz")["rand256"].astype(np.int64)
    good, off = fixed_rows_to_device(dv(arr, dev))
    stale = good.reshape(arr.shape).flip(1).reshape(-1).contiguous()      # every row backwards: the same range
    ops = GpuBpeOps(dev) if early_ops else None

    def fn(x):
        res = train_bpe(x, off, 700, ops=ops)
        ids = [res.vocab[a] for m in res.merges for a in m]
        outb = torch.full((3 + 2 * 700,), -1, dtype=torch.int64)
        outb[:3 + len(ids)] = torch.tensor([res.min_token, res.max_token, len(res.vocab)] + ids)
        return [outb.to(dev)]

    def check(exp):
        got = exp[0].tolist()
        want = [ref["vocab"][a] for m in ref["merges"] for a in m]
        assert got[:3] == [ref["min_token"], ref["max_token"], len(ref["vocab"])] and got[3:3 + len(want)] == want
    c = api_case(f"train_bpe[{'ops-from-before' if early_ops else 'fresh-ops'}]", good, stale, fn, check)
    c.synchronous = True
    return c


api("train_bpe[GpuBpeOps-rand256/700-synchronous-weaker-form]")(lambda dev: train_case(dev, False))
api("train_bpe[GpuBpeOps-constructed-on-the-null-stream-synchronous-weaker-form]")(lambda dev: train_case(dev, True))


@api("column_quantiles[GpuQuantileOps-constructed-on-the-null-stream]")
def _(dev):
    """quantile.column_quantiles with an ops object made before the stream changed: its launches
    must follow the current stream, not the one of construction."""
    from beast_tokenizer_amd.quantile import GpuQuantileOps, column_quantiles
    xg = np.random.default_rng(4).standard_normal((300, 3)).astype(F32)
    good = dv(xg, dev)
    ops = GpuQuantileOps(dev)

    def check(exp):
        assert np.array_equal(npy(exp[0]), np.stack([np.quantile(xg, F32(q), axis=0) for q in (0.01, 0.99)]).astype(F32))
    return api_case("column_quantiles", good, (good * 0.5 + 1).contiguous(),
                    lambda x: [column_quantiles(x, [0.01, 0.99], ops=ops)], check)


@pytest.mark.parametrize("cid", SO.ids(SO.API_CASES, __name__))
def test_python_api_is_ordered_on_the_current_stream(cid, gpu_device):
    SO.check_api(cid, gpu_device)


# ===================================================== C. constants built on another stream ==
def on_three_streams(dev, first, again, expected_of):
    """``first()`` runs on a side stream s1 behind a delay, so every constant it caches is built
    behind that delay; at once ``again()`` runs on the null stream and on a second side stream s2
    with inputs that are complete.  Both must return ``expected_of()``'s value (computed last, on the
    null stream, fully synchronised, with its own fresh object)."""
    s1 = SO.side_stream(dev)                                     # a delay on s1 holds up neither the null stream
    s2 = SO.side_stream(dev, beside=[torch.cuda.default_stream(dev)])
    for _ in range(16):                                          # ... nor s2 (they must not share a hardware queue)
        if SO.runs_beside(s1, s2, dev):
            break
        s2 = SO.side_stream(dev)
    else:
        pytest.fail("no second side stream runs beside the first")
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(s1):
        SO.sleep_ms(30.0, dev)
        r1 = first()
    r0 = again()
    with torch.cuda.stream(s2):
        r2 = again()
    s2.synchronize()
    torch.cuda.default_stream(dev).synchronize()
    got0, got2 = [t.clone() for t in r0], [t.clone() for t in r2]
    s1.synchronize()
    torch.cuda.synchronize(dev)
    want = expected_of()
    torch.cuda.synchronize(dev)
    for name, got in (("s1", r1), ("null stream", got0), ("s2", got2)):
        for i, (a, b) in enumerate(zip(want, got)):
            assert SO.bits_equal(a, b), f"result {i} on {name} differs: a cached constant was used before it was built"


@stops_after_a_fault
def test_plan_constants_built_on_another_stream(gpu_device, canary):
    """_Plan.keep (Phi, the fp32 projection, the DoF maps, the bounds) and DeviceBasis._cache."""
    dev = gpu_device
    x, t = trajectories(17, dev), tokens17(dev)
    tok, g = api_tok(dev)

    def use(tk):
        return lambda: [tk.encode(x)[0], tk.encode(x)[1]["params"], tk.reconstruct_traj(t),
                        tk.reconstruct_traj_derivs(t)[1]]
    torch.cuda.synchronize(dev)
    on_three_streams(dev, use(tok), use(tok), use(api_tok(dev)[0]))


@stops_after_a_fault
def test_plan_rebuilt_after_update_times_on_another_stream(gpu_device, canary):
    """The sharpest form: everything that needs a host-to-device copy (knot vectors, DoF maps) is
    cached already, then ``update_times`` invalidates the plan, so the rebuild on s1 is kernels
    only -- Phi, the float64 projection, its fp32 image and the derivative slabs are all still
    behind the delay when the null stream and s2 ask for them.  (A first build waits for its own
    copies from host memory, which hides the race most of the time.)"""
    dev = gpu_device
    x, t = trajectories(17, dev), tokens17(dev)
    tok, g = api_tok(dev)

    def use(tk):
        return lambda: [tk.encode(x)[0], tk.encode(x)[1]["params"], tk.reconstruct_traj(t),
                        tk.reconstruct_traj_derivs(t)[1]]
    use(tok)()
    torch.cuda.synchronize(dev)
    tok.update_times(tok.times.clone())              # the same grid as a new tensor: every plan is stale
    torch.cuda.synchronize(dev)
    on_three_streams(dev, use(tok), use(tok), use(api_tok(dev)[0]))


@stops_after_a_fault
def test_times_override_built_on_another_stream(gpu_device, canary):
    """A per-row ``times`` override (_basis_for / _deriv_basis_for): the per-call bases are built
    and used on the calling stream, over knot vectors and a plan cached by the first call."""
    dev = gpu_device
    t = tokens17(dev)
    times = dv(np.sort(np.random.default_rng(5).uniform(0, 2 * np.pi, size=(17, 33)), axis=1).astype(F32), dev)
    tok, g = api_tok(dev)

    def use(tk):
        return lambda: [tk.reconstruct_traj(t, times=times), tk.reconstruct_traj_derivs(t, times=times)[2]]
    torch.cuda.synchronize(dev)
    on_three_streams(dev, use(tok), use(tok), use(api_tok(dev)[0]))


@stops_after_a_fault
def test_conditioned_caches_built_on_another_stream(gpu_device, canary):
    """_cond_cache, _full_basis and _full_deriv of a conditioned tokenizer."""
    dev = gpu_device
    x = trajectories(17, dev, seed=14)

    def make():
        tk = BEASTBsplineTokenizer(device=str(dev), init_cond_order=2, end_cond_order=2, **CONFIGS["k3"])
        tk.load_state_dict({"w_min": [-2.0] * 140, "w_max": [2.0] * 140})
        return tk

    def use(tk):
        def f():
            tks, d = tk.encode(x)
            return [tks, d["params"], d["init_vel"], tk.reconstruct_traj(tks), tk.reconstruct_traj_derivs(tks)[1]]
        return f
    tok = make()
    torch.cuda.synchronize(dev)
    on_three_streams(dev, use(tok), use(tok), use(make()))


@stops_after_a_fault
def test_bpe_model_built_on_another_stream(gpu_device, canary):
    """GpuBpeModel: the merge map (built by beast_bpe_mergemap_build), byte2id, lut and wordmap."""
    from beast_tokenizer_amd.bpe_codec import GpuBpeModel
    dev = gpu_device
    _, hf, spec, rows, want, flat, off, width = bpe_model(dev)
    box = {}

    def first():
        box["m"] = GpuBpeModel(hf, dev)
        return encode_with(box["m"])

    def encode_with(m):
        out = []
        for fn in (m._encode_rows_words, m._encode_rows_kernel):
            ids, lens, status = fn(flat, off, width, 0, None)
            mask = torch.arange(ids.shape[1], device=dev)[None, :] < lens[:, None]
            out += [torch.where(mask, ids, torch.full_like(ids, -1)), lens, status]
        return out
    on_three_streams(dev, first, lambda: encode_with(box["m"]), lambda: encode_with(GpuBpeModel(hf, dev)))
    res = encode_with(box["m"])
    assert ragged(res[0], res[1]) == want and ragged(res[3], res[4]) == want
