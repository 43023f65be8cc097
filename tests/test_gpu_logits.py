"""beast_logits_expect / beast_logits_expect_bwd and the tokenizer's logits methods on the GPU,
against the float64 oracle (tests/logits_oracle.py).

Tolerances are measured, not fixed in advance (the rule and the floor of tests/test_gpu_derivs.py):
    forward   max |mean - oracle|                         (mean's range is [-1, 1])
    backward  max |grad - oracle| / max |oracle|          per case
each bounded by 4x the error of torch's own fp32 composition ``(softmax(l / tau) * x).sum(-1)`` (and
its autograd) evaluated on the CPU on the same inputs, with a floor of 16 * 2^-24.  A half / bf16
``grad_logits`` additionally gets one ulp of its type at the oracle's value.  Every test prints what
it measured.
"""
import numpy as np
import pytest
import torch

import logits_oracle as LO
from beast_tokenizer_amd import BEASTBsplineBPETokenizer, BEASTBsplineTokenizer, _lib

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
FLOOR = 16 * EPS
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
MANT = {torch.float32: 23, torch.float16: 10, torch.bfloat16: 7}
MIN_EXP = {torch.float32: -126, torch.float16: -14, torch.bfloat16: -126}


def bound(yardstick):
    return max(4 * yardstick, FLOOR)


def ulp(dtype, x):
    """One unit in the last place of ``dtype`` at |x| (float64 array)."""
    e = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** MIN_EXP[dtype])))
    return 2.0 ** (e - MANT[dtype])


def bits(t):
    return t.contiguous().view(torch.uint8) if t.dtype != torch.uint8 else t


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def f64(t):
    return t.detach().to("cpu", torch.float64).numpy()


# ------------------------------------------------------------------ raw entry points --
def fwd(l, tau=1.0, off=0, mean=True, amax=True, stats=True):
    """beast_logits_expect on a [B, K, V] view; returns (mean, amax, stats), poisoned first."""
    B, K, V = l.shape
    dev = l.device
    m = torch.full((B, K), float("nan"), device=dev) if mean else None
    a = torch.full((B, K), -7, dtype=torch.int64, device=dev) if amax else None
    s = torch.full((B, K, 2), float("nan"), device=dev) if stats else None
    _lib.run("beast_logits_expect", l.data_ptr(), _lib.LOGITS_DTYPES[l.dtype], B, K, V, l.stride(0), l.stride(1),
             tau, off, _lib.ptr(m), _lib.ptr(a), _lib.ptr(s), _lib.stream_of(dev))
    return m, a, s


def bwd(l, tau, mean, stats, g, out=None):
    """beast_logits_expect_bwd into ``out`` (a [B, K, V] view; default: a fresh NaN-filled tensor)."""
    B, K, V = l.shape
    if out is None:
        out = torch.full((B, K, V), float("nan"), dtype=l.dtype, device=l.device)
    _lib.run("beast_logits_expect_bwd", l.data_ptr(), _lib.LOGITS_DTYPES[l.dtype], B, K, V, l.stride(0), l.stride(1),
             tau, mean.data_ptr(), stats.data_ptr(), g.data_ptr(), out.data_ptr(), out.stride(0), out.stride(1),
             _lib.stream_of(l.device))
    return out


def torch_fp32_errors(l64, g64, tau, want_mean, want_grad):
    """The yardstick: torch's fp32 composition and its autograd on the CPU, on the same inputs."""
    t = torch.tensor(l64, dtype=torch.float32, requires_grad=True)
    x = torch.tensor(LO.bins(l64.shape[-1]), dtype=torch.float32)
    m = (torch.softmax(t / tau, -1) * x).sum(-1)
    m.backward(torch.tensor(g64, dtype=torch.float32))
    e_f = float(np.abs(m.detach().numpy().astype(np.float64) - want_mean).max())
    e_b = float(np.abs(t.grad.numpy().astype(np.float64) - want_grad).max() / np.abs(want_grad).max())
    return e_f, e_b


def check_against_oracle(l, tau, tag, dev):
    """Forward and backward of the [B, K, V] device tensor ``l`` against the oracle; returns the
    measured (forward, backward) errors and their bounds."""
    l64 = f64(l)
    g = torch.randn(l.shape[:2], generator=torch.Generator().manual_seed(l.shape[-1]), dtype=torch.float32)
    want_mean, want_amax, want_stats = LO.expect(l64, tau)
    want_grad = LO.grad(l64, g.numpy().astype(np.float64), tau)
    y_f, y_b = torch_fp32_errors(l64, g.numpy().astype(np.float64), tau, want_mean, want_grad)
    mean, amax, stats = fwd(l, tau)
    grad = bwd(l, tau, mean, stats, g.to(dev))
    torch.cuda.synchronize(dev)
    e_f = float(np.abs(f64(mean) - want_mean).max())
    diff = np.abs(f64(grad) - want_grad)
    scale = np.abs(want_grad).max()
    slack = ulp(l.dtype, want_grad) if l.dtype != torch.float32 else 0.0
    e_b = float(np.maximum(diff - slack, 0.0).max() / scale)
    print(f"{tag} tau {tau}: forward {e_f:.3e} (bound {bound(y_f):.3e})  backward {e_b:.3e} (bound {bound(y_b):.3e})")
    assert np.array_equal(amax.cpu().numpy(), want_amax), tag
    assert float(f64(mean).min()) >= -1.0 and float(f64(mean).max()) <= 1.0
    # stats: zmax is one product of two fp32 numbers; s is relative to the ROUNDED zmax, so it is
    # zmax + log s (the log-sum-exp) that compares with the oracle's
    st = f64(stats)
    assert np.all(np.abs(st[..., 0] - want_stats[..., 0]) <= 4 * EPS * np.abs(want_stats[..., 0]) + 1e-30)
    lse, want_lse = st[..., 0] + np.log(st[..., 1]), want_stats[..., 0] + np.log(want_stats[..., 1])
    assert np.all(np.abs(lse - want_lse) <= 4 * EPS * np.abs(want_stats[..., 0]) + 64 * EPS)
    assert e_f <= bound(y_f), (tag, tau, e_f, bound(y_f))
    assert e_b <= bound(y_b), (tag, tau, e_b, bound(y_b))
    return e_f, e_b


def randn4(shape, dtype, dev, seed, scale=4.0):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=gen, dtype=torch.float32) * scale).to(dtype).to(dev)


@pytest.mark.parametrize("BK", [(1, 1), (3, 7), (2, 140), (37, 140)], ids=lambda bk: f"B{bk[0]}K{bk[1]}")
@pytest.mark.parametrize("V", [2, 3, 255, 256, 257, 1000, 4097])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_forward_and_backward_against_the_oracle(dtype, V, BK, gpu_device):
    """V 2, 3: one lane partly filled; 255 / 256 / 257 (fp32): a partial chunk, a chunk exactly
    full, one element past a chunk; 1000: several chunks in registers; 4097: the online form."""
    l = randn4((*BK, V), DTYPES[dtype], gpu_device, seed=V * 1000 + BK[0])
    for tau in (0.25, 1.0, 3.0):
        check_against_oracle(l, tau, f"{dtype} V{V} B{BK[0]} K{BK[1]}", gpu_device)


@pytest.mark.parametrize("V", [1025, 2048])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_three_and_four_chunks_of_the_16_bit_types(dtype, V, gpu_device):
    """A 16-bit chunk is 512 logits, so the V list above reaches one chunk (up to 257), two (1000)
    and the online form (4097) for fp16 / bf16, never the three- and four-chunk in-register
    instantiation: V 1025 (one element in the third chunk) and 2048 (four full chunks)."""
    l = randn4((3, 7, V), DTYPES[dtype], gpu_device, seed=V)
    for tau in (0.25, 1.0, 3.0):
        check_against_oracle(l, tau, f"{dtype} V{V} B3 K7", gpu_device)


def test_grid_stride_over_four_times_the_resident_rows(gpu_device):
    """At least four times as many rows as either launch keeps resident (the library says how many):
    every workgroup walks several groups of rows.  A row's outputs do not depend on the batch, so
    the launch over everything is compared bitwise with launches that fit the resident grid --
    every 17th batch element, the first and the last ones -- and the sample goes against the oracle."""
    lib = _lib.load()
    code = _lib.LOGITS_DTYPES[torch.bfloat16]
    resident = max(lib.beast_logits_resident_rows(code, 256, b, _lib.stream_of(gpu_device)) for b in (0, 1))
    assert resident > 0
    K = 140
    B = -(-4 * resident // K)
    assert B * K >= 4 * resident
    print(f"grid stride: {B * K} rows over {resident} resident")
    l = randn4((B, K, 256), torch.bfloat16, gpu_device, seed=5)
    g = torch.randn((B, K), device=gpu_device)
    mean, amax, stats = fwd(l, 1.0)
    grad = bwd(l, 1.0, mean, stats, g)
    sample = l[::17].contiguous()
    assert sample.shape[0] * K <= resident
    check_against_oracle(sample, 1.0, "grid stride sample", gpu_device)
    for sl in (slice(None, None, 17), slice(0, 3), slice(B - 3, B)):
        part, gp = l[sl].contiguous(), g[sl].contiguous()
        m1, a1, s1 = fwd(part, 1.0)
        assert same_bits(m1, mean[sl]) and same_bits(a1, amax[sl]) and same_bits(s1, stats[sl])
        assert same_bits(bwd(part, 1.0, m1, s1, gp), grad[sl])


# ---------------------------------------------------------------- strides, alignment --
@pytest.mark.parametrize("start", [13, 48])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_strided_slices_equal_the_contiguous_tensor_bitwise(dtype, start, gpu_device):
    """A 252-wide slice of a [B, K, 300] tensor from element 13 (no row is 16-byte aligned) and from
    48 (every fp32 row is; with 2-byte elements the 600-byte row stride alternates): the outputs,
    and a gradient written into such a slice, equal those of the same values in a contiguous tensor
    bit for bit, and nothing around the gradient's slice is touched."""
    dt, V = DTYPES[dtype], 252
    full = randn4((5, 9, 300), dt, gpu_device, seed=start)
    view = full[..., start:start + V]
    assert view.stride() == (9 * 300, 300, 1) and view.data_ptr() == full.data_ptr() + start * full.element_size()
    aligned = {(view[b, k].data_ptr() % 16 == 0) for b in range(5) for k in range(9)}
    assert aligned == ({False} if start == 13 else {True} if dt is torch.float32 else {True, False})
    flat = view.contiguous()
    assert flat.data_ptr() % 16 == 0
    g = torch.randn((5, 9), device=gpu_device)
    for tau in (0.5, 2.0):
        want = fwd(flat, tau, off=100)
        got = fwd(view, tau, off=100)
        assert all(same_bits(a, b) for a, b in zip(got, want))
        want_grad = bwd(flat, tau, want[0], want[2], g)
        assert not torch.isnan(want_grad).any()
        out = torch.full((5, 9, 300), float("nan"), dtype=dt, device=gpu_device)
        bwd(view, tau, got[0], got[2], g, out=out[..., start:start + V])
        assert same_bits(out[..., start:start + V].contiguous(), want_grad)
        assert torch.isnan(out[..., :start]).all() and torch.isnan(out[..., start + V:]).all()
        # a contiguous input with a strided output, and the reverse
        out.fill_(float("nan"))
        bwd(flat, tau, want[0], want[2], g, out=out[..., start:start + V])
        assert same_bits(out[..., start:start + V].contiguous(), want_grad)
        assert same_bits(bwd(view, tau, got[0], got[2], g), want_grad)


def test_offsets_beyond_two_to_the_31_elements(gpu_device):
    """A [2, 3, 256] bf16 view with a batch stride of 2^31 + 8 elements over one uninitialised
    allocation (about 4.3 GB; only the six rows are ever written or read), for the logits and for
    the gradient: bitwise the contiguous case."""
    sb = 2 ** 31 + 8
    n = sb + 3 * 256
    vals = randn4((2, 3, 256), torch.bfloat16, gpu_device, seed=31)
    g = torch.randn((2, 3), device=gpu_device)
    want = fwd(vals, 0.7, off=7)
    want_grad = bwd(vals, 0.7, want[0], want[2], g)
    src = torch.empty(n, dtype=torch.bfloat16, device=gpu_device).as_strided((2, 3, 256), (sb, 256, 1))
    dst = torch.empty(n, dtype=torch.bfloat16, device=gpu_device).as_strided((2, 3, 256), (sb, 256, 1))
    src.copy_(vals)
    dst.fill_(float("nan"))
    got = fwd(src, 0.7, off=7)
    assert all(same_bits(a, b) for a, b in zip(got, want))
    bwd(src, 0.7, got[0], got[2], g, out=dst)
    assert same_bits(dst.contiguous(), want_grad)


# -------------------------------------------------- determinism, batch independence --
@pytest.mark.parametrize("V", [257, 4097])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_runs_agree_bitwise_and_rows_do_not_depend_on_the_batch(dtype, V, gpu_device):
    l = randn4((6, 11, V), DTYPES[dtype], gpu_device, seed=V)
    g = torch.randn((6, 11), device=gpu_device)
    first = fwd(l, 1.3)
    grad = bwd(l, 1.3, first[0], first[2], g)
    again = fwd(l, 1.3)
    assert all(same_bits(a, b) for a, b in zip(first, again))
    assert same_bits(bwd(l, 1.3, again[0], again[2], g), grad)
    for b, k in ((0, 0), (2, 5), (5, 10)):
        one = l[b:b + 1, k:k + 1]
        m1, a1, s1 = fwd(one, 1.3)
        assert same_bits(m1, first[0][b:b + 1, k:k + 1]) and same_bits(a1, first[1][b:b + 1, k:k + 1])
        assert same_bits(s1, first[2][b:b + 1, k:k + 1])
        assert same_bits(bwd(one, 1.3, m1, s1, g[b:b + 1, k:k + 1].contiguous()), grad[b:b + 1, k:k + 1])


# --------------------------------------------------------------------------- argmax --
def test_argmax_is_numpy_argmax_on_every_row_ties_included(gpu_device):
    """bf16 randn * 2 has a tied maximum in about 2 % of its 256-wide rows: the lowest index wins,
    as in np.argmax, on every row; the offset is added."""
    l = randn4((64, 140, 256), torch.bfloat16, gpu_device, seed=2, scale=2.0)
    raw = l.float().cpu().numpy()
    tied = (raw == raw.max(-1, keepdims=True)).sum(-1) > 1
    print(f"argmax: {int(tied.sum())} of {tied.size} rows have a tied maximum")
    assert tied.sum() >= 20
    off = 32000 - 256
    got = fwd(l, 1.0, off=off, mean=False, stats=False)[1].cpu().numpy()
    assert np.array_equal(got, np.argmax(raw, -1) + off)
    both = fwd(l, 1.0, off=off)[1].cpu().numpy()           # the same kernel with every output
    assert np.array_equal(both, got)
    l4 = randn4((3, 5, 4097), torch.bfloat16, gpu_device, seed=3, scale=2.0)     # the online form
    assert np.array_equal(fwd(l4, 1.0, mean=False, stats=False)[1].cpu().numpy(),
                          np.argmax(l4.float().cpu().numpy(), -1))


# ------------------------------------------------------------------- special values --
@pytest.mark.parametrize("V", [256, 4097])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_minus_infinity_entries_and_huge_rows(dtype, V, gpu_device):
    dt = DTYPES[dtype]
    l = randn4((4, 6, V), dt, gpu_device, seed=V + 1)
    dead = torch.rand((4, 6, V), generator=torch.Generator().manual_seed(1)) < 0.5
    dead[0, 0, : V - 1] = True                              # one survivor, the last bin
    dead[0, 0, V - 1] = False
    l[dead.to(gpu_device)] = float("-inf")
    l[1, 1] = torch.where(torch.arange(V, device=gpu_device) % 2 == 0, 1e30, -1e30).to(dt)   # rows at +-1e30
    l[1, 2] = -1e30
    l[1, 3] = 1e30
    g = torch.randn((4, 6), device=gpu_device)
    for tau in (0.25, 1.0):
        mean, amax, stats = fwd(l, tau)
        grad = bwd(l, tau, mean, stats, g)
        want_mean, want_amax, _ = LO.expect(f64(l), tau)
        assert torch.isfinite(mean).all() and torch.isfinite(stats).all() and torch.isfinite(grad).all()
        assert np.abs(f64(mean) - want_mean).max() <= FLOOR
        assert np.array_equal(amax.cpu().numpy(), want_amax)
        assert (grad[torch.isneginf(l)] == 0).all()
        assert 1.0 - 4 * EPS <= float(mean[0, 0]) <= 1.0    # all the mass on bin V-1: never above 1
        assert abs(float(mean[1, 2])) <= FLOOR and abs(float(mean[1, 3])) <= FLOOR   # uniform rows


@pytest.mark.parametrize("V", [256, 4097])
def test_unspecified_rows_do_not_disturb_the_others(V, gpu_device):
    """A NaN row, a +inf row and an all -inf row in the middle of a batch: every other row is bitwise
    what it is in the batch without them."""
    clean = randn4((3, 9, V), torch.float32, gpu_device, seed=V + 2)
    dirty = clean.clone()
    dirty[1, 3, V // 3] = float("nan")
    dirty[1, 4, V // 2] = float("inf")
    dirty[1, 5] = float("-inf")
    keep = torch.ones((3, 9), dtype=torch.bool, device=gpu_device)
    keep[1, 3:6] = False
    g = torch.randn((3, 9), device=gpu_device)
    want = fwd(clean, 1.0)
    got = fwd(dirty, 1.0)
    for a, b in zip(got, want):
        assert same_bits(a[keep], b[keep])
    assert same_bits(bwd(dirty, 1.0, got[0], got[2], g)[keep], bwd(clean, 1.0, want[0], want[2], g)[keep])
    torch.cuda.synchronize(gpu_device)


# --------------------------------------------------------------- the Python surface --
def make_tok(dev, cls=BEASTBsplineTokenizer, **kw):
    tok = cls(num_dof=14, num_basis=10, seq_len=50, vocab_size=256, device=str(dev), **kw)
    gen = torch.Generator().manual_seed(9)
    tok.w_min.copy_(-1.0 - torch.rand(140, generator=gen))
    tok.w_max.copy_(1.0 + torch.rand(140, generator=gen))
    return tok


def chain_f64(tok, leaf64, target64, tau, off):
    """The whole chain in float64 torch on the CPU from the tokenizer's own slabs and bounds:
    logits -> expected normalised coefficients -> positions, accelerations -> loss."""
    N, D = tok.num_basis, tok.num_dof
    slabs = tok._basis.deriv_constants(tok.times.to(torch.float32).reshape(-1), tok._times_version).cpu().double()
    lo, hi = tok.w_min.detach().cpu().double().reshape(D, N), tok.w_max.detach().cpu().double().reshape(D, N)
    l = leaf64.reshape(leaf64.shape[0], N * D, -1)[..., off:off + tok.vocab_size]
    x = torch.tensor(LO.bins(tok.vocab_size))
    nt = (torch.softmax(l / tau, -1) * x).sum(-1).clamp(-1, 1).reshape(-1, N, D)
    w = (nt.permute(0, 2, 1) + 1) / 2 * (hi - lo) + lo                      # [B, D, N]
    pos = torch.einsum("tn,bdn->btd", slabs[0, 0], w)
    acc = torch.einsum("tn,bdn->btd", slabs[2, 0], w)
    return ((pos - target64) ** 2).sum() + 0.1 * (acc ** 2).sum()


@pytest.mark.parametrize("leaf", ["fp32-flat", "bf16-4d", "fp32-full-vocabulary"])
def test_whole_chain_gradient_reaches_the_logits_leaf(leaf, gpu_device):
    """loss = (pos - target)^2.sum() + 0.1 acc^2.sum() through reconstruct_traj_from_logits(orders=(0, 2)):
    the gradient in the leaf against the float64 composition, to the backward bound with the fp32
    CPU composition of the same chain as the yardstick."""
    tok = make_tok(gpu_device)
    B, N, D, V, tau = 5, 10, 14, 256, 0.8
    off, Vp, dt = 0, V, torch.float32
    shape = (B, N * D, V)
    if leaf == "bf16-4d":
        shape, dt = (B, N, D, V), torch.bfloat16
    elif leaf == "fp32-full-vocabulary":
        Vp = 1000
        tok.set_llm_vocab_size(Vp)
        off, shape = Vp - V, (B, N * D, Vp)
    gen = torch.Generator().manual_seed(4)
    init = (torch.randn(shape, generator=gen) * 4.0).to(dt)
    target = torch.randn((B, 50, D), generator=gen)
    x = init.to(gpu_device).requires_grad_(True)
    pos, acc = tok.reconstruct_traj_from_logits(x, temperature=tau, orders=(0, 2))
    assert pos.shape == acc.shape == (B, 50, D) and pos.grad_fn is not None
    loss = ((pos - target.to(gpu_device)) ** 2).sum() + 0.1 * (acc ** 2).sum()
    loss.backward()
    assert x.grad.shape == x.shape and x.grad.dtype == dt and x.grad.device == x.device
    # float64 reference and the fp32 yardstick, both on the CPU from the same leaf values
    ref = init.double().requires_grad_(True)
    chain_f64(tok, ref, target.double(), tau, off).backward()
    want = ref.grad.numpy()
    slabs32 = tok._basis.deriv_constants(tok.times.to(torch.float32).reshape(-1), tok._times_version).cpu()
    y = init.float().requires_grad_(True)
    l32 = y.reshape(B, N * D, -1)[..., off:off + V]
    nt = (torch.softmax(l32 / tau, -1) * torch.tensor(LO.bins(V), dtype=torch.float32)).sum(-1).clamp(-1, 1)
    lo, hi = tok.w_min.detach().cpu().reshape(D, N), tok.w_max.detach().cpu().reshape(D, N)
    w = (nt.reshape(B, N, D).permute(0, 2, 1) + 1) / 2 * (hi - lo) + lo
    p32, a32 = torch.einsum("tn,bdn->btd", slabs32[0, 0], w), torch.einsum("tn,bdn->btd", slabs32[2, 0], w)
    (((p32 - target) ** 2).sum() + 0.1 * (a32 ** 2).sum()).backward()
    scale = np.abs(want).max()
    yard = float(np.abs(y.grad.numpy().astype(np.float64) - want).max() / scale)
    slack = ulp(dt, want) if dt != torch.float32 else 0.0
    err = float(np.maximum(np.abs(f64(x.grad) - want) - slack, 0.0).max() / scale)
    print(f"whole chain {leaf}: err {err:.3e} bound {bound(yard):.3e}")
    assert err <= bound(yard), (leaf, err, bound(yard))
    if off:
        assert not x.grad[..., :off].any() and x.grad[..., off:].any()
    # no graph without requires_grad or under no_grad, and the same bits
    plain = tok.reconstruct_traj_from_logits(x.detach(), temperature=tau, orders=(0, 2))
    with torch.no_grad():
        quiet = tok.reconstruct_traj_from_logits(x, temperature=tau, orders=(0, 2))
    for o in range(2):
        assert plain[o].grad_fn is None and not plain[o].requires_grad and quiet[o].grad_fn is None
        assert same_bits(plain[o], (pos, acc)[o].detach()) and same_bits(quiet[o], plain[o])
    nt_plain = tok.expected_params_from_logits(x.detach(), temperature=tau)
    nt_grad = tok.expected_params_from_logits(x, temperature=tau)
    assert nt_plain.grad_fn is None and nt_grad.grad_fn is not None and same_bits(nt_plain, nt_grad.detach())
    assert nt_plain.shape == (B, N * D) and nt_plain.dtype == torch.float32


def test_peaked_logits_decode_like_their_greedy_tokens(gpu_device):
    """One logit 40 above the rest at a random bin per token: the expected coefficient is that
    bin's value to the forward bound E (the rest holds < 256 e^-30 of the mass), so
    reconstruct_traj_from_logits agrees with reconstruct_traj(greedy tokens) within
    sum_n |basis[t][n]| (E max(w_max - w_min) + (8 + 2 (N + 1)) 2^-24 max|bound|): the second term
    is test_continuous_form_matches_token_form's rounding of the two decode chains."""
    tok = make_tok(gpu_device)
    B, K, V = 7, 140, 256
    gen = torch.Generator().manual_seed(12)
    l = torch.randn((B, K, V), generator=gen)
    hot = torch.randint(0, V, (B, K), generator=gen)
    hot[0, :2] = torch.tensor([0, V - 1])
    l.scatter_add_(2, hot[..., None], torch.full((B, K, 1), 40.0))
    assert float(l.abs().max()) < 50.0
    l = l.to(gpu_device)
    toks = tok.greedy_tokens_from_logits(l)
    assert toks.dtype == torch.int64 and torch.equal(toks.cpu(), hot)
    nt, toks2 = tok.expected_params_from_logits(l, return_tokens=True)
    assert torch.equal(toks2, toks)
    want_nt = LO.bins(V)[hot.numpy()]
    y_f, _ = torch_fp32_errors(f64(l), np.ones((B, K)), 1.0, LO.expect(f64(l))[0], LO.grad(f64(l), np.ones((B, K))))
    E = bound(y_f) + V * np.exp(-30.0)
    e_nt = float(np.abs(f64(nt) - want_nt).max())
    print(f"peaked: |ntokens - bin| {e_nt:.3e} (bound {E:.3e})")
    assert e_nt <= E
    span = float((tok.w_max - tok.w_min).max())
    wmax = float(torch.maximum(tok.w_min.abs(), tok.w_max.abs()).max())
    phi = tok._basis.deriv_constants(tok.times.to(torch.float32).reshape(-1), tok._times_version)[0]
    rowsum = phi.abs().sum(-1).max(0).values
    tol = rowsum * (E * span + (8 + 2 * (10 + 1)) * EPS * wmax)
    diff = (tok.reconstruct_traj_from_logits(l) - tok.reconstruct_traj(toks)).abs()
    assert (diff <= tol[None, :, None]).all(), float((diff / tol[None, :, None]).max())


def test_greedy_tokens_respect_the_llm_vocabulary(gpu_device):
    """A full-vocabulary tensor: the argmax runs over the action slice only (a larger logit outside
    it is never chosen) and the LLM offset is added exactly as encode adds it."""
    tok = make_tok(gpu_device)
    tok.set_llm_vocab_size(1000)
    l = randn4((3, 140, 1000), torch.bfloat16, gpu_device, seed=8)
    l[..., :744] += 50.0                                    # everything outside the slice is larger
    want = np.argmax(l[..., 744:].float().cpu().numpy(), -1)
    assert np.array_equal(tok.greedy_tokens_from_logits(l).cpu().numpy(), want + 744)
    assert np.array_equal(tok.greedy_tokens_from_logits(l, respect_llm_vocab_size=False).cpu().numpy(), want)
    assert np.array_equal(tok.greedy_tokens_from_logits(l.reshape(3, 10, 14, 1000)).cpu().numpy(), want + 744)
    action = l[..., 744:]                                   # the slice itself is accepted too
    assert np.array_equal(tok.greedy_tokens_from_logits(action).cpu().numpy(), want + 744)
    x = l.clone().requires_grad_(True)
    assert not tok.greedy_tokens_from_logits(x).requires_grad
    traj = tok.reconstruct_traj(tok.greedy_tokens_from_logits(l))
    assert traj.shape == (3, 50, 14)


def test_other_input_forms(gpu_device):
    """float64 is cast to fp32, a host tensor is moved, a non-unit last stride is made contiguous:
    all inside the graph; an empty batch launches nothing; the BPE tokenizer inherits the methods."""
    tok = make_tok(gpu_device)
    l = randn4((4, 140, 256), torch.float32, gpu_device, seed=6)
    want = tok.expected_params_from_logits(l, temperature=0.9)
    assert same_bits(tok.expected_params_from_logits(l.double(), temperature=0.9), want)
    assert same_bits(tok.expected_params_from_logits(l.cpu(), temperature=0.9), want)
    swapped = l.transpose(1, 2).contiguous().transpose(1, 2)
    assert swapped.stride(2) != 1
    assert same_bits(tok.expected_params_from_logits(swapped, temperature=0.9), want)
    host = l.cpu().double().requires_grad_(True)
    tok.expected_params_from_logits(host, temperature=0.9).sum().backward()
    assert host.grad.shape == host.shape and host.grad.dtype == torch.float64 and host.grad.device.type == "cpu"
    assert abs(float(host.grad.sum())) <= 1e-3              # rows of a softmax gradient sum to 0
    assert tok.expected_params_from_logits(l[:0]).shape == (0, 140)
    assert tok.greedy_tokens_from_logits(l[:0]).shape == (0, 140)
    pos = tok.reconstruct_traj_from_logits(l, temperature=0.9)
    assert same_bits(pos, tok.reconstruct_traj_continuous(want))
    bpe = make_tok(gpu_device, cls=BEASTBsplineBPETokenizer)
    assert same_bits(bpe.expected_params_from_logits(l, temperature=0.9), want)
