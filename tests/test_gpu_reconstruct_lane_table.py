"""k_reconstruct_v (one wave per trajectory; lane table built once per workgroup, quotient without the
dequantise LUT) against the tile-walking k_reconstruct, bitwise, and against the oracle.

k_reconstruct_v takes the inverse DoF map, the A-operand addresses and the kind mask of every lane
from a table that one wave of the workgroup writes in front of the tile barrier, maps its dequantise
slots to (n d) without a division (d = lane % 16, n = lane / 16 + 4 u) and computes t / (V - 1) as
beast::exact_quotient (csrc/common.h) for 0 <= t < 4096 and V <= 4096, by IEEE division otherwise.
The comparison kernel is the specialised k_reconstruct, forced with BEAST_OPT_BLOCK_WAVES 7 and 4: it
still reads the LUT and divides.  Positions must be the same bits, and within the project's bar
(1e-5 * max(1, |ref|_inf) per trajectory, test_gpu_codec_dispatch.py) of the float64 basis product of
the oracle's float32 discrete_to_continuous.

Every launch is checked through BEAST_OPT_LAST_CODEC_LAUNCH to be the kernel it is meant to be.
"""
import numpy as np
import pytest
import torch

from beast_tokenizer_amd import BEASTBsplineTokenizer, _lib
from oracle import beast_oracle as O

pytestmark = pytest.mark.gpu

F32 = np.float32
TAU = F32(2 * np.pi)
T, N, D, V = 50, 10, 14, 256
BATCHES = (1, 15, 16, 17, 33)       # one live wave, the last wave missing, a full tile, one past, two tiles and one
GRIPS = {14: None, 12: [12, 13]}    # joint_dof -> gripper DoFs: one basis kind, two (mask path, gripper columns)
INT64_MIN = -2 ** 63
WILD = (-1, 256, 4095, 4096, 2 ** 24 + 1, INT64_MIN)
REC_V = dict(family="reconstruct_v", tile=16, waves=16, ks=3, latency=True)
PERM = [5, 0, 13, 2, 9, 7, 1, 12, 3, 11, 4, 10, 6, 8]   # a dof_dst without fixed structure (a permutation)


def _spec(waves):
    return dict(family="reconstruct_spec", tile=8, waves=waves, ks=3)


def _set_waves(w):
    lib = _lib.load()
    assert lib.beast_set_option(_lib.OPT_GENERIC_KERNELS, 0) == 0
    assert lib.beast_set_option(_lib.OPT_BLOCK_WAVES, w) == 0


def _ran(fields):
    m = _lib.last_codec_launch()
    got = {k: getattr(m, k) for k in fields}
    assert got == fields, f"launch took another branch: {m}"


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def _same(a, b, what):
    a, b = _bits(a), _bits(b)
    bad = np.argwhere(a != b)
    assert bad.size == 0, f"{what}: {len(bad)} elements differ, first at {bad[0].tolist()}"


_TOK = {}


def _tok(jd):
    """The tokenizer whose plan supplies the basis [2][T][N] and the DoF order; shared, never modified."""
    if jd not in _TOK:
        grip = GRIPS[jd]
        tok = BEASTBsplineTokenizer(num_dof=D, num_basis=N, seq_len=T, vocab_size=V, degree_p=4,
                                    gripper_zero_order=bool(grip), gripper_indices=grip, device="cuda:0")
        assert tok.joint_dof == jd
        _TOK[jd] = (tok, O.Layout.make(D, grip, bool(grip)))
    return _TOK[jd]


def _bounds(seed):
    rng = np.random.default_rng(seed)
    lo = rng.uniform(-3, 1, size=D * N).astype(F32)
    hi = (lo + rng.uniform(0.1, 4, size=D * N)).astype(F32)
    return lo, hi


def _c_rec(jd, tokens, vocab, off, lo_t, hi_t, dst_t, init_p=None):
    """beast_reconstruct_f32 with the caller's own bounds, vocabulary, offset and DoF map."""
    tok, lay = _tok(jd)
    p = tok._plan()
    B = tokens.shape[0]
    pos = torch.full((B, T, D), float("nan"), device="cuda:0")
    src = torch.tensor(lay.order, dtype=torch.int32, device="cuda:0")
    rc = _lib.load().beast_reconstruct_f32(
        tokens.data_ptr(), B, D, jd, N, vocab, off, lo_t.data_ptr(), hi_t.data_ptr(), p.p_phi, 0, T,
        dst_t.data_ptr(), D, _lib.ptr(init_p), 0 if init_p is None else init_p.stride(0),
        None if init_p is None else src.data_ptr(), None, pos.data_ptr(), None, _lib.raw_stream(p.idx))
    _lib.check(rc, "beast_reconstruct_f32")
    torch.cuda.synchronize()
    return pos


def _three(jd, tokens, vocab, off, lo_t, hi_t, dst_t, init_p, what):
    """Positions of k_reconstruct_v, checked bitwise against the 7- and the 4-wave k_reconstruct."""
    try:
        _set_waves(0)
        pv = _c_rec(jd, tokens, vocab, off, lo_t, hi_t, dst_t, init_p)
        _ran(REC_V)
        for w in (7, 4):
            _set_waves(w)
            pw = _c_rec(jd, tokens, vocab, off, lo_t, hi_t, dst_t, init_p)
            _ran(_spec(w))
            _same(pv, pw, f"{what}: k_reconstruct_v against the {w}-wave k_reconstruct")
    finally:
        _set_waves(0)
    return pv


def _oracle(jd, tokens, vocab, off, lo, hi, dst, init_p=None):
    """float64 basis @ the oracle's float32 discrete_to_continuous, [B, T, D] with column dst[i] <- DoF i."""
    _, lay = _tok(jd)
    B = tokens.shape[0]
    w = O.decode(tokens, lay, N, lo, hi, vocab, offset=off).reshape(B, D, N).copy()
    if init_p is not None:
        for i, col in enumerate(lay.joint_indices):
            w[:, i, 0] = init_p[:, col]
    times = O.times_grid(2 * np.pi, T)
    pj, pg = O.basis(times, TAU, 4, N).astype(np.float64), O.basis(times, TAU, 0, N).astype(np.float64)
    want = np.zeros((B, T, D))
    for i in range(D):
        want[:, :, dst[i]] = np.einsum("tn,bn->bt", pj if i < jd else pg, w[:, i].astype(np.float64))
    return want


def _close(pos, want):
    pos = pos.cpu().numpy()
    scale = np.maximum(1.0, np.abs(want).max(axis=(1, 2), keepdims=True))
    err = np.abs(pos - want) / scale
    assert err.max() <= 1e-5, float(err.max())


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0", dtype=dtype)


def _tokens(B, vocab, off, seed, wild=True):
    """[B, N, D] tokens in [0, vocab) + off; with `wild`, WILD (before the offset) walks over the slots of
    each trajectory so that every (n d) class of slot meets one in some case."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, vocab, size=(B, N, D), dtype=np.int64)
    if wild:
        for b in range(B):
            for i, wv in enumerate(WILD):
                e = (b * 17 + i * 23 + seed) % (N * D)
                t[b, e // D, e % D] = wv
    return (t + np.int64(off)) if off else t     # int64 wraps for INT64_MIN, as on the device


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("jd", (14, 12))
def test_batches_maps_offsets(jd, B):
    """Every workgroup shape x identity / permuted dof_dst x LLM offset x init_p, wild tokens included."""
    lo, hi = _bounds(100 + jd)
    lo_t, hi_t = _dev(lo), _dev(hi)
    _, lay = _tok(jd)
    ip = np.random.default_rng(B).standard_normal((B, D)).astype(F32)
    ip_t = _dev(ip)
    for dst in (lay.order, PERM):
        dst_t = torch.tensor(dst, dtype=torch.int32, device="cuda:0")
        for off in (0, 32000 - V):
            t = _tokens(B, V, off, seed=B + jd)
            tk = _dev(t.reshape(B, N * D))
            for init in (None, ip):
                what = f"B={B} dst={'perm' if dst is PERM else 'order'} off={off} init_p={init is not None}"
                pv = _three(jd, tk, V, off, lo_t, hi_t, dst_t, None if init is None else ip_t, what)
                _close(pv, _oracle(jd, t.reshape(B, N * D), V, off, lo, hi, dst, init))


@pytest.mark.parametrize("jd", (14, 12))
def test_every_bin_everywhere(jd):
    """Every bin 0..255 in every (n, d) position (256 trajectories; position e of trajectory b holds bin
    (b + 37 e) % 256), identity and permuted DoF map."""
    B = 256
    lo, hi = _bounds(200 + jd)
    lo_t, hi_t = _dev(lo), _dev(hi)
    _, lay = _tok(jd)
    t = ((np.arange(B)[:, None] + 37 * np.arange(N * D)[None, :]) % 256).astype(np.int64)
    assert all(len(set(t[:, e])) == 256 for e in range(N * D))
    tk = _dev(t)
    for dst in (lay.order, PERM):
        dst_t = torch.tensor(dst, dtype=torch.int32, device="cuda:0")
        pv = _three(jd, tk, V, 0, lo_t, hi_t, dst_t, None, f"every bin, dst={'perm' if dst is PERM else 'order'}")
        _close(pv, _oracle(jd, t, V, 0, lo, hi, dst))


@pytest.mark.parametrize("vocab", (2, 3, 4096, 4097))
@pytest.mark.parametrize("jd", (14, 12))
def test_vocab_through_the_c_abi(jd, vocab):
    """The C-ABI with its own bounds and vocabulary: 2 and 3 (r = 1, 0.5), 4096 (the largest without the
    division) and 4097 (every token divides); in-range tokens over the whole vocabulary, and WILD."""
    B = 17
    lo, hi = _bounds(300 + jd + vocab)
    lo_t, hi_t = _dev(lo), _dev(hi)
    dst_t = torch.tensor(PERM, dtype=torch.int32, device="cuda:0")
    t = _tokens(B, vocab, 0, seed=vocab)
    t[0, :, 0] = vocab - 1                      # the top bin, every n
    t[0, :, 1] = np.arange(N) % vocab
    tk = _dev(t.reshape(B, N * D))
    pv = _three(jd, tk, vocab, 0, lo_t, hi_t, dst_t, None, f"vocab={vocab}")
    _close(pv, _oracle(jd, t.reshape(B, N * D), vocab, 0, lo, hi, PERM))


@pytest.mark.parametrize("jd", (14, 12))
def test_api_token_shapes_and_init_p(jd):
    """Tokens as [B, N*D] and as [B, N, D] through reconstruct_traj, with a nonzero LLM offset; a call
    with init_p gives the general path's positions."""
    B = 33
    grip = GRIPS[jd]
    lo, hi = _bounds(400 + jd)
    tok = BEASTBsplineTokenizer(num_dof=D, num_basis=N, seq_len=T, vocab_size=V, degree_p=4,
                                gripper_zero_order=bool(grip), gripper_indices=grip, device="cuda:0",
                                llm_vocab_size=32000)
    tok.w_min.copy_(_dev(lo))
    tok.w_max.copy_(_dev(hi))
    off = 32000 - V
    t = _tokens(B, V, off, seed=jd, wild=True)
    ip = _dev(np.random.default_rng(jd).standard_normal((B, D)).astype(F32))
    try:
        _set_waves(0)
        p2 = tok.reconstruct_traj(_dev(t.reshape(B, N * D)))
        _ran(REC_V)
        p3 = tok.reconstruct_traj(_dev(t))
        _ran(REC_V)
        _same(p2, p3, "[B, N*D] against [B, N, D]")
        pi = tok.reconstruct_traj(_dev(t), init_p=ip)
        _ran(REC_V)
        _set_waves(7)
        q2 = tok.reconstruct_traj(_dev(t.reshape(B, N * D)))
        _ran(_spec(7))
        qi = tok.reconstruct_traj(_dev(t), init_p=ip)
        _ran(_spec(7))
    finally:
        _set_waves(0)
    _same(p2, q2, "API positions against the 7-wave k_reconstruct")
    _same(pi, qi, "API positions with init_p against the 7-wave k_reconstruct")
    assert not torch.equal(p2, pi), "init_p must change the positions"
    _, lay = _tok(jd)
    _close(p2, _oracle(jd, t.reshape(B, N * D), V, off, lo, hi, lay.order))


@pytest.mark.parametrize("jd", (14, 12))
def test_inplace_bounds_and_map_update(jd):
    """w_min / w_max and dof_dst updated in place between two calls change the second call's output:
    nothing derived from them outlives a launch."""
    B = 33
    lo, hi = _bounds(500 + jd)
    lo_t, hi_t = _dev(lo), _dev(hi)
    _, lay = _tok(jd)
    dst_t = torch.tensor(lay.order, dtype=torch.int32, device="cuda:0")
    t = _tokens(B, V, 0, seed=5 + jd, wild=False)
    tk = _dev(t.reshape(B, N * D))
    first = _three(jd, tk, V, 0, lo_t, hi_t, dst_t, None, "before the update")
    lo2, hi2 = (lo * F32(0.5)).astype(F32), (hi * F32(0.75) + F32(0.01)).astype(F32)
    lo_t.copy_(_dev(lo2))
    hi_t.copy_(_dev(hi2))
    second = _three(jd, tk, V, 0, lo_t, hi_t, dst_t, None, "after the bounds update")
    assert not torch.equal(first, second), "the new bounds must change the positions"
    _close(second, _oracle(jd, t.reshape(B, N * D), V, 0, lo2, hi2, lay.order))
    dst_t.copy_(torch.tensor(PERM, dtype=torch.int32, device="cuda:0"))
    third = _three(jd, tk, V, 0, lo_t, hi_t, dst_t, None, "after the DoF-map update")
    assert not torch.equal(second, third), "the new DoF map must change the positions"
    _close(third, _oracle(jd, t.reshape(B, N * D), V, 0, lo2, hi2, PERM))
