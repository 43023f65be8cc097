"""beast_xent_rows / beast_xent_rows_bwd and ``cross_entropy_from_logits`` on the GPU, against the
float64 oracle (tests/xent_oracle.py).

Tolerances are measured, not fixed in advance (the rule of tests/test_gpu_logits.py and
tests/test_gpu_derivs.py):
    forward   max |loss - oracle|
    backward  max |grad - oracle|
each bounded by 4x the error of torch's own fp32 composition ``-(q * log_softmax(l)).sum(-1)`` (and its
autograd, with the same dense target q) evaluated on the CPU on the same inputs, with a floor of
16 * 2^-24 * max(1, max |oracle|).  A half / bf16 ``grad_logits`` is judged beyond one ulp of its type
at the oracle's value.  Every test prints what it measured.
"""
import numpy as np
import pytest
import torch

import logits_oracle as LO
import xent_oracle as XO
from beast_tokenizer_amd import BEASTBsplineBPETokenizer, _lib
from test_gpu_logits import DTYPES, EPS, FLOOR, f64, make_tok, randn4, same_bits, torch_fp32_errors, ulp
from test_gpu_logits import bound as logits_bound

pytestmark = pytest.mark.gpu

IGNORE = -100
NAN = float("nan")


def bound(yardstick, oracle):
    finite = np.abs(oracle[np.isfinite(oracle)])
    return max(4 * yardstick, FLOOR * max(1.0, float(finite.max()) if finite.size else 1.0))


# ------------------------------------------------------------------ raw entry points --
def targets_of(tgt):
    return (tgt.data_ptr(), None) if tgt.dtype is torch.int64 else (None, tgt.data_ptr())


def fwd(l, tgt, eps=0.0, off=0, ignore=IGNORE, loss=True, amax=True, stats=True):
    """beast_xent_rows on a [B, K, V] view; returns (loss, amax, stats), poisoned first."""
    B, K, V = l.shape
    dev = l.device
    assert tgt.shape == (B, K) and tgt.is_contiguous() and tgt.dtype in (torch.int64, torch.float32)
    lo = torch.full((B, K), NAN, device=dev) if loss else None
    a = torch.full((B, K), -7, dtype=torch.int64, device=dev) if amax else None
    s = torch.full((B, K, 2), NAN, device=dev) if stats else None
    _lib.run("beast_xent_rows", l.data_ptr(), _lib.LOGITS_DTYPES[l.dtype], B, K, V, l.stride(0), l.stride(1),
             *targets_of(tgt), off, ignore, eps, _lib.ptr(lo), _lib.ptr(s), _lib.ptr(a), _lib.stream_of(dev))
    return lo, a, s


def bwd(l, tgt, eps, stats, g, off=0, ignore=IGNORE, out=None):
    """beast_xent_rows_bwd into ``out`` (a [B, K, V] view; default: a fresh NaN-filled tensor)."""
    B, K, V = l.shape
    if out is None:
        out = torch.full((B, K, V), NAN, dtype=l.dtype, device=l.device)
    _lib.run("beast_xent_rows_bwd", l.data_ptr(), _lib.LOGITS_DTYPES[l.dtype], B, K, V, l.stride(0), l.stride(1),
             *targets_of(tgt), off, ignore, eps, stats.data_ptr(), g.data_ptr(), out.data_ptr(), out.stride(0),
             out.stride(1), _lib.stream_of(l.device))
    return out


def both(l, tgt, eps, g, **kw):
    """(loss, amax, stats, grad) of one forward and one backward launch."""
    lo, a, s = fwd(l, tgt, eps, **kw)
    return lo, a, s, bwd(l, tgt, eps, s, g, **kw)


def random_tokens(shape, V, seed, dev, special=True):
    """Tokens in [0, V): with ``special`` the first rows are 0, V-1 and the ignored one."""
    t = torch.randint(0, V, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.int64)
    if special and t.numel() >= 4:
        t.view(-1)[:3] = torch.tensor([0, V - 1, IGNORE])
    return t.to(dev)


def random_coeffs(shape, seed, dev, special=True):
    """Coefficients in [-1.05, 1.05): with ``special`` the first rows are -1, 1, NaN and 1.5."""
    x = torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 2.1 - 1.05
    if special and x.numel() >= 5:
        x.view(-1)[:4] = torch.tensor([-1.0, 1.0, NAN, 1.5])
    return x.to(dev)


def oracle_target(tgt, V, off=0, ignore=IGNORE):
    h = tgt.cpu().numpy()
    return XO.target_from_tokens(h, V, off, ignore) if tgt.dtype is torch.int64 else XO.target_from_coeffs(h, V)


def torch_fp32_yardstick(l64, ifk, eps, g64, want_loss, want_grad):
    """torch's fp32 composition and its autograd on the CPU, on the same inputs and the same dense
    target: its largest errors (loss, gradient) against the oracle, over the rows that have a target."""
    i, f, k = ifk
    keep = k == XO.TARGET
    t = torch.tensor(l64[keep], dtype=torch.float32, requires_grad=True)
    q = torch.tensor(XO.dense_target(i[keep], f[keep], l64.shape[-1], eps), dtype=torch.float32)
    out = -(q * torch.log_softmax(t, -1)).sum(-1)
    out.backward(torch.tensor(g64[keep], dtype=torch.float32))
    e_f = float(np.abs(out.detach().numpy().astype(np.float64) - want_loss[keep]).max())
    e_b = float(np.abs(t.grad.numpy().astype(np.float64) - want_grad[keep]).max())
    return e_f, e_b


def grad_error(grad, want, dtype):
    """max |grad - oracle|, for a half type beyond one ulp of the type at the oracle's value."""
    slack = ulp(dtype, want) if dtype != torch.float32 else 0.0
    return float(np.maximum(np.abs(f64(grad) - want) - slack, 0.0).max())


def check_against_oracle(l, tgt, eps, tag, dev):
    """Forward and backward of the [B, K, V] device tensor ``l`` against the oracle."""
    l64 = f64(l)
    V = l.shape[-1]
    g = torch.randn(l.shape[:2], generator=torch.Generator().manual_seed(V), dtype=torch.float32)
    g64 = g.numpy().astype(np.float64)
    ifk = oracle_target(tgt, V)
    want_loss, want_grad = XO.loss(l64, *ifk, eps), XO.grad(l64, *ifk, g64, eps)
    want_m, want_s, want_amax = XO.rows(l64)
    y_f, y_b = torch_fp32_yardstick(l64, ifk, eps, g64, want_loss, want_grad)
    b_f, b_b = bound(y_f, want_loss), bound(y_b, want_grad)
    loss, amax, stats, grad = both(l, tgt, eps, g.to(dev))
    torch.cuda.synchronize(dev)
    e_f = float(np.abs(f64(loss) - want_loss).max())
    e_b = grad_error(grad, want_grad, l.dtype)
    kind = "tokens" if tgt.dtype is torch.int64 else "coeffs"
    print(f"{tag} {kind} eps {eps}: forward {e_f:.3e} (bound {b_f:.3e})  backward {e_b:.3e} (bound {b_b:.3e})")
    assert np.array_equal(amax.cpu().numpy(), want_amax), tag
    # stats: m is the exact maximum; log s compares with the oracle's
    st = f64(stats)
    assert np.array_equal(st[..., 0], want_m)
    assert np.all(np.abs(np.log(st[..., 1]) - np.log(want_s)) <= 64 * EPS)
    ignored = ifk[2] == XO.IGNORED
    assert not f64(loss)[ignored].any() and not f64(grad)[ignored].any()
    assert e_f <= b_f, (tag, eps, e_f, b_f)
    assert e_b <= b_b, (tag, eps, e_b, b_b)
    return e_f, e_b


@pytest.mark.parametrize("BK", [(1, 1), (3, 7), (2, 140), (37, 140)], ids=lambda bk: f"B{bk[0]}K{bk[1]}")
@pytest.mark.parametrize("V", [2, 3, 255, 256, 257, 1000, 4097])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_forward_and_backward_against_the_oracle(dtype, V, BK, gpu_device):
    """V 2, 3: one lane partly filled; 255 / 256 / 257 (fp32): a partial chunk, a chunk exactly
    full, one element past a chunk; 1000: several chunks in registers; 4097: the online and the long
    form.  Each with both target kinds and label smoothing 0 and 0.1."""
    l = randn4((*BK, V), DTYPES[dtype], gpu_device, seed=V * 1000 + BK[0])
    for tgt in (random_tokens(BK, V, V + BK[1], gpu_device), random_coeffs(BK, V + BK[1], gpu_device)):
        for eps in (0.0, 0.1):
            check_against_oracle(l, tgt, eps, f"{dtype} V{V} B{BK[0]} K{BK[1]}", gpu_device)


@pytest.mark.parametrize("V", [1025, 2048])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_three_and_four_chunks_of_the_16_bit_types(dtype, V, gpu_device):
    """A 16-bit chunk is 512 logits, so the V list above reaches one chunk, two (1000) and the online
    and long forms (4097) for fp16 / bf16, never the three- and four-chunk in-register instantiation."""
    BK = (3, 7)
    l = randn4((*BK, V), DTYPES[dtype], gpu_device, seed=V)
    for tgt in (random_tokens(BK, V, V + 7, gpu_device), random_coeffs(BK, V + 7, gpu_device)):
        for eps in (0.0, 0.1):
            check_against_oracle(l, tgt, eps, f"{dtype} V{V} B3 K7", gpu_device)


# ------------------------------------------------------------------------- bitwise --
def test_grid_stride_over_four_times_the_resident_rows(gpu_device):
    """Four times as many rows as a decode launch keeps resident (beast_logits_resident_rows: the
    cross-entropy kernels use the same launch rule): every workgroup walks several groups of rows.
    The launch over everything is compared bitwise, on sampled rows, with launches that fit the
    resident grid, and the sample goes against the oracle."""
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
    for tgt in (random_tokens((B, K), 256, 1, gpu_device), random_coeffs((B, K), 2, gpu_device)):
        whole = both(l, tgt, 0.1, g)
        check_against_oracle(l[::17].contiguous(), tgt[::17].contiguous(), 0.1, "grid stride sample", gpu_device)
        for sl in (slice(None, None, 17), slice(0, 3), slice(B - 3, B)):
            part = both(l[sl].contiguous(), tgt[sl].contiguous(), 0.1, g[sl].contiguous())
            assert l[sl].shape[0] * K <= resident
            assert all(same_bits(a, b[sl]) for a, b in zip(part, whole))


@pytest.mark.parametrize("start", [13, 48])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_strided_slices_equal_the_contiguous_tensor_bitwise(dtype, start, gpu_device):
    """A 252-wide slice of a [B, K, 300] tensor from element 13 (no row is 16-byte aligned) and from
    48 (every fp32 row is; with 2-byte elements the 600-byte row stride alternates): the outputs, and
    a gradient written into such a slice, equal those of the same values in a contiguous tensor bit
    for bit, and nothing around the gradient's slice is touched."""
    dt, V = DTYPES[dtype], 252
    full = randn4((5, 9, 300), dt, gpu_device, seed=start)
    view = full[..., start:start + V]
    aligned = {(view[b, k].data_ptr() % 16 == 0) for b in range(5) for k in range(9)}
    assert aligned == ({False} if start == 13 else {True} if dt is torch.float32 else {True, False})
    flat = view.contiguous()
    assert flat.data_ptr() % 16 == 0
    g = torch.randn((5, 9), device=gpu_device)
    for tgt in (random_tokens((5, 9), V, 3, gpu_device), random_coeffs((5, 9), 4, gpu_device)):
        for eps in (0.0, 0.1):
            want = fwd(flat, tgt, eps, off=0)
            got = fwd(view, tgt, eps, off=0)
            assert all(same_bits(a, b) for a, b in zip(got, want))
            want_grad = bwd(flat, tgt, eps, want[2], g)
            assert not torch.isnan(want_grad).any()
            out = torch.full((5, 9, 300), NAN, dtype=dt, device=gpu_device)
            bwd(view, tgt, eps, got[2], g, out=out[..., start:start + V])
            assert same_bits(out[..., start:start + V].contiguous(), want_grad)
            assert torch.isnan(out[..., :start]).all() and torch.isnan(out[..., start + V:]).all()
            # a contiguous input with a strided output, and the reverse
            out.fill_(NAN)
            bwd(flat, tgt, eps, want[2], g, out=out[..., start:start + V])
            assert same_bits(out[..., start:start + V].contiguous(), want_grad)
            assert same_bits(bwd(view, tgt, eps, got[2], g), want_grad)


def test_offsets_beyond_two_to_the_31_elements(gpu_device):
    """A [2, 3, 256] bf16 view with a batch stride of 2^31 + 8 elements over one uninitialised
    allocation (about 4.3 GB; only the six rows are ever written or read), for the logits and for
    the gradient: bitwise the contiguous case."""
    sb = 2 ** 31 + 8
    n = sb + 3 * 256
    vals = randn4((2, 3, 256), torch.bfloat16, gpu_device, seed=31)
    g = torch.randn((2, 3), device=gpu_device)
    tgt = random_coeffs((2, 3), 5, gpu_device, special=False)
    want = both(vals, tgt, 0.1, g)
    src = torch.empty(n, dtype=torch.bfloat16, device=gpu_device).as_strided((2, 3, 256), (sb, 256, 1))
    dst = torch.empty(n, dtype=torch.bfloat16, device=gpu_device).as_strided((2, 3, 256), (sb, 256, 1))
    src.copy_(vals)
    dst.fill_(NAN)
    got = fwd(src, tgt, 0.1)
    assert all(same_bits(a, b) for a, b in zip(got, want[:3]))
    bwd(src, tgt, 0.1, got[2], g, out=dst)
    assert same_bits(dst.contiguous(), want[3])


@pytest.mark.parametrize("V", [257, 4097])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_runs_agree_bitwise_and_rows_do_not_depend_on_the_batch(dtype, V, gpu_device):
    l = randn4((6, 11, V), DTYPES[dtype], gpu_device, seed=V)
    g = torch.randn((6, 11), device=gpu_device)
    for tgt in (random_tokens((6, 11), V, 6, gpu_device), random_coeffs((6, 11), 7, gpu_device)):
        first = both(l, tgt, 0.1, g)
        again = both(l, tgt, 0.1, g)
        assert all(same_bits(a, b) for a, b in zip(first, again))
        for b, k in ((0, 0), (0, 2), (2, 5), (5, 10)):
            one = both(l[b:b + 1, k:k + 1], tgt[b:b + 1, k:k + 1].contiguous(), 0.1, g[b:b + 1, k:k + 1].contiguous())
            assert all(same_bits(a, w[b:b + 1, k:k + 1]) for a, w in zip(one, first))


# ------------------------------------------------------------------------- targets --
@pytest.mark.parametrize("V", [256, 257, 4097])
def test_a_token_and_the_coefficient_of_its_bin_agree_bitwise(V, gpu_device):
    """x = 2t/(V-1) - 1 rounded to fp32, kept where the fp32 replica of the kernel's position gives
    back the integer t exactly (asserted here on the host; all of them for V - 1 a power of two): the
    coefficient target then has f == 0 at bin t, and loss and gradient equal the token target's."""
    t_all = np.arange(V, dtype=np.int64)
    x_all = (2.0 * t_all / (V - 1) - 1.0).astype(np.float32)
    exact = XO.position_fp32(x_all, V) == t_all.astype(np.float32)
    assert exact[0] and exact[V - 1] and exact.sum() >= V // 2, int(exact.sum())
    if V != 256:
        assert exact.all()                          # V - 1 is a power of two: nothing rounds
    t, x = t_all[exact], x_all[exact]
    assert np.array_equal(XO.position_fp32(x, V), t.astype(np.float32))          # the precondition
    i, f, _ = XO.target_from_coeffs(x, V)
    assert np.array_equal(i, np.minimum(t, V - 2)) and np.array_equal(f, (t == V - 1).astype(np.float64))
    n = len(t)
    l = randn4((1, n, V), torch.float32, gpu_device, seed=V)
    g = torch.randn((1, n), device=gpu_device)
    for eps in (0.0, 0.1):
        by_token = both(l, torch.tensor(t, device=gpu_device)[None].contiguous(), eps, g)
        by_coeff = both(l, torch.tensor(x, device=gpu_device)[None].contiguous(), eps, g)
        assert all(same_bits(a, b) for a, b in zip(by_token, by_coeff))


def test_a_token_with_the_llm_offset_equals_the_plain_token(gpu_device):
    l = randn4((3, 140, 256), torch.bfloat16, gpu_device, seed=8)
    g = torch.randn((3, 140), device=gpu_device)
    t = random_tokens((3, 140), 256, 9, gpu_device, special=False)
    plain = both(l, t, 0.1, g)
    shifted = both(l, t + 744, 0.1, g, off=744)
    assert same_bits(shifted[0], plain[0]) and same_bits(shifted[2], plain[2]) and same_bits(shifted[3], plain[3])
    assert torch.equal(shifted[1], plain[1] + 744)
    tok = make_tok(gpu_device)
    tok.set_llm_vocab_size(1000)
    a = tok.cross_entropy_from_logits(l, t + 744, reduction="none", label_smoothing=0.1)
    b = tok.cross_entropy_from_logits(l, t, reduction="none", label_smoothing=0.1, respect_llm_vocab_size=False)
    assert same_bits(a, b) and same_bits(a, plain[0])


@pytest.mark.parametrize("V", [252, 4097])
def test_ignored_rows_are_exactly_zero_and_nothing_after_a_row_is_touched(V, gpu_device):
    """grad_logits rows lie V + 48 elements apart and are poisoned first: an ignored row (a token equal
    to ignore_index, a NaN coefficient) is written as V zeros, its loss is exactly 0, and the 48
    elements after every row keep their poison."""
    W = V + 48
    l = randn4((4, 6, V), torch.bfloat16, gpu_device, seed=V)
    g = torch.randn((4, 6), device=gpu_device)
    g[1, 2] = NAN                                   # an upstream NaN does not leak through an ignored row
    tok = random_tokens((4, 6), V, 1, gpu_device, special=False)
    pos = random_coeffs((4, 6), 2, gpu_device, special=False)
    ignored = torch.zeros((4, 6), dtype=torch.bool, device=gpu_device)
    ignored[0, 0] = ignored[1, 2] = ignored[3, 5] = True
    tok[ignored] = 7                                # an ignore_index inside the token range
    pos[ignored] = NAN
    for tgt, ignore in ((tok, 7), (pos, IGNORE)):
        for eps in (0.0, 0.1):
            loss, _, stats = fwd(l, tgt, eps, ignore=ignore)
            out = torch.full((4, 6, W), NAN, dtype=torch.bfloat16, device=gpu_device)
            poison = out.clone()
            bwd(l, tgt, eps, stats, g, ignore=ignore, out=out[..., :V])
            assert same_bits(out[..., V:].contiguous(), poison[..., V:].contiguous())
            zero = torch.zeros((3, V), dtype=torch.bfloat16, device=gpu_device)
            assert same_bits(out[..., :V][ignored], zero)                        # +0, every element
            assert same_bits(loss[ignored], torch.zeros(3, device=gpu_device))
            keep = ~ignored
            keep[1, 2] = False
            assert torch.isfinite(out[..., :V][keep]).all() and torch.isfinite(loss[~ignored]).all()


@pytest.mark.parametrize("V", [256, 4097])
def test_an_out_of_range_token_gives_nan_in_its_own_row_only(V, gpu_device):
    l = randn4((3, 9, V), torch.float32, gpu_device, seed=V + 3)
    g = torch.randn((3, 9), device=gpu_device)
    good = random_tokens((3, 9), V, 4, gpu_device, special=False) + 50
    bad = good.clone()
    bad[0, 1], bad[1, 4], bad[2, 8], bad[2, 0] = 50 + V, 49, -3, 2 ** 40
    wrong = bad != good
    assert int(wrong.sum()) == 4
    want = both(l, good, 0.1, g, off=50)
    got = both(l, bad, 0.1, g, off=50)
    torch.cuda.synchronize(gpu_device)
    assert torch.isnan(got[0][wrong]).all() and torch.isnan(got[3][wrong]).all()
    for a, b in zip(got, want):
        assert same_bits(a[~wrong], b[~wrong])
    assert same_bits(got[1], want[1]) and same_bits(got[2], want[2])             # argmax and stats: every row


# ------------------------------------------------------------------- special values --
@pytest.mark.parametrize("V", [256, 4097])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_minus_infinity_entries(dtype, V, gpu_device):
    """Half of every row is -inf, never the token's own bin.  Without smoothing those entries have
    weight zero: the loss is finite (the oracle's) and the gradient exactly 0 there -- also where the
    -inf entry is bin i+1 of a target with f == 0, and bin i of the last token (f == 1).  With
    smoothing every bin has weight: the loss is +inf."""
    dt = DTYPES[dtype]
    B, K = 4, 6
    l = randn4((B, K, V), dt, gpu_device, seed=V + 1)
    t = random_tokens((B, K), V, 11, gpu_device, special=False)
    t[0, 0], t[0, 1] = V - 1, 5
    dead = torch.rand((B, K, V), generator=torch.Generator().manual_seed(1)).to(gpu_device) < 0.5
    dead.scatter_(2, t[..., None], False)
    dead[0, 0, V - 2] = True                        # bin i of the last token: weight 1 - f == 0
    dead[0, 1, 6] = True                            # bin i+1 of a token with f == 0
    l[dead] = float("-inf")
    g = torch.randn((B, K), device=gpu_device)
    loss, amax, stats, grad = both(l, t, 0.0, g)
    want = XO.loss(f64(l), *oracle_target(t, V), 0.0)
    assert torch.isfinite(loss).all() and torch.isfinite(stats).all() and torch.isfinite(grad).all()
    assert np.abs(f64(loss) - want).max() <= FLOOR * max(1.0, np.abs(want).max())
    assert (grad[dead] == 0).all() and np.array_equal(amax.cpu().numpy(), XO.rows(f64(l))[2])
    smooth = fwd(l, t, 0.1)[0]
    assert torch.isposinf(smooth).all()
    # a coefficient between two bins of which one is -inf: its weight is positive, the loss +inf
    x0 = np.float32(-1.0 + 1.0 / (V - 1))           # u about 0.5: bins 0 and 1 both weigh
    i0, f0, _ = XO.target_from_coeffs(x0, V)
    assert i0 == 0 and 0.0 < f0 < 1.0
    l2 = l.clone()
    l2[..., 0] = 1.0
    l2[..., 1] = float("-inf")
    assert torch.isposinf(fwd(l2, torch.full((B, K), float(x0), device=gpu_device), 0.0)[0]).all()


@pytest.mark.parametrize("V", [256, 4097])
def test_unspecified_rows_do_not_disturb_the_others(V, gpu_device):
    """A NaN row, a +inf row and an all -inf row in the middle of a batch: every other row is bitwise
    what it is in the batch without them."""
    clean = randn4((3, 9, V), torch.float32, gpu_device, seed=V + 2)
    dirty = clean.clone()
    dirty[1, 3, V // 3] = NAN
    dirty[1, 4, V // 2] = float("inf")
    dirty[1, 5] = float("-inf")
    keep = torch.ones((3, 9), dtype=torch.bool, device=gpu_device)
    keep[1, 3:6] = False
    g = torch.randn((3, 9), device=gpu_device)
    for tgt in (random_tokens((3, 9), V, 1, gpu_device), random_coeffs((3, 9), 2, gpu_device)):
        for eps in (0.0, 0.1):
            want = both(clean, tgt, eps, g)
            got = both(dirty, tgt, eps, g)
            for a, b in zip(got, want):
                assert same_bits(a[keep], b[keep])
    torch.cuda.synchronize(gpu_device)


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
    t = random_tokens((64, 140), 256, 1, gpu_device) + off
    got = fwd(l, t, off=off, loss=False, stats=False)[1].cpu().numpy()
    assert np.array_equal(got, np.argmax(raw, -1) + off)
    assert np.array_equal(fwd(l, t, 0.1, off=off)[1].cpu().numpy(), got)         # the same kernel with every output
    l4 = randn4((3, 5, 4097), torch.bfloat16, gpu_device, seed=3, scale=2.0)     # the online form
    t4 = random_tokens((3, 5), 4097, 1, gpu_device)
    want4 = np.argmax(l4.float().cpu().numpy(), -1)
    assert np.array_equal(fwd(l4, t4, loss=False, stats=False)[1].cpu().numpy(), want4)
    assert np.array_equal(fwd(l4, t4, 0.1)[1].cpu().numpy(), want4)


# ------------------------------------------------- consistency with the decode direction --
def test_the_two_hot_optimum_decodes_to_the_coefficient(gpu_device):
    """logits = log q of the unsmoothed two-hot target of random x: expected_params_from_logits gives x
    back (to the forward bound of tests/test_gpu_logits.py, its fp32 yardstick on these logits), and the
    logits are a stationary point of the loss: max |grad| is at or below the gradient bound -- its floor
    alone, since torch's dense composition has no yardstick to offer here (0 * -inf is NaN)."""
    tok = make_tok(gpu_device)
    B, K, V = 6, 140, 256
    x = random_coeffs((B, K), 21, gpu_device, special=False).clamp(-1.0, 1.0)
    x.view(-1)[:3] = torch.tensor([-1.0, 1.0, 0.0])
    ifk = XO.target_from_coeffs(x.cpu().numpy(), V)
    with np.errstate(divide="ignore"):
        logq = np.log(XO.dense_target(ifk[0], ifk[1], V)).astype(np.float32)
    l = torch.tensor(logq, device=gpu_device)
    l64 = f64(l)
    ones = np.ones((B, K))
    y_f, _ = torch_fp32_errors(l64, ones, 1.0, LO.expect(l64)[0], LO.grad(l64, ones))
    got = tok.expected_params_from_logits(l)
    e = float(np.abs(f64(got) - f64(x)).max())
    print(f"two-hot optimum: |decoded - x| {e:.3e} (bound {logits_bound(y_f):.3e})")
    assert e <= logits_bound(y_f)
    want_loss, want_grad = XO.loss(l64, *ifk), XO.grad(l64, *ifk, ones)
    assert np.isfinite(want_loss).all() and np.abs(want_grad).max() <= 1e-6        # the oracle agrees: stationary
    loss, _, _, grad = both(l, x.contiguous(), 0.0, torch.ones((B, K), device=gpu_device))
    gmax = float(grad.abs().max())
    print(f"two-hot optimum: max |grad| {gmax:.3e} (bound {bound(0.0, want_grad):.3e})")
    assert torch.isfinite(loss).all() and gmax <= bound(0.0, want_grad)


# --------------------------------------------------------------- the Python surface --
@pytest.mark.parametrize("kind", ["tokens", "coefficients"])
@pytest.mark.parametrize("leaf", ["fp32-flat", "bf16-4d", "fp32-full-vocabulary"])
def test_autograd_reaches_the_logits_leaf(leaf, kind, gpu_device):
    """The three reductions (and a weighted "none") through ``cross_entropy_from_logits``: the loss
    and the gradient in the leaf against the oracle; the gradient has the leaf's shape and dtype and
    is zero outside the action slice."""
    tok = make_tok(gpu_device)
    B, N, D, V, eps = 5, 10, 14, 256, 0.1
    off, Vp, dt = 0, V, torch.float32
    shape, tshape = (B, N * D, V), (B, N * D)
    if leaf == "bf16-4d":
        shape, tshape, dt = (B, N, D, V), (B, N, D), torch.bfloat16
    elif leaf == "fp32-full-vocabulary":
        Vp = 1000
        tok.set_llm_vocab_size(Vp)
        off, shape = Vp - V, (B, N * D, Vp)
    init = (torch.randn(shape, generator=torch.Generator().manual_seed(4)) * 4.0).to(dt)
    if kind == "tokens":
        target = (random_tokens((B, N * D), V, 5, "cpu") + off).reshape(tshape)
        target.view(-1)[2] = IGNORE
    else:
        target = random_coeffs((B, N * D), 5, "cpu").reshape(tshape)
    l64 = init.double().numpy().reshape(B, N * D, -1)[..., off:off + V]
    ifk = oracle_target(target.reshape(B, N * D), V, off)
    n_kept = int((ifk[2] != XO.IGNORED).sum())
    assert n_kept < B * N * D
    want_loss = XO.loss(l64, *ifk, eps)
    w = torch.randn((B, N * D), generator=torch.Generator().manual_seed(6))
    for reduction, g64 in (("none", w.double().numpy()), ("sum", np.ones((B, N * D))),
                           ("mean", np.full((B, N * D), 1.0 / n_kept))):
        x = init.to(gpu_device).requires_grad_(True)
        out = tok.cross_entropy_from_logits(x, target, label_smoothing=eps, reduction=reduction)
        assert out.grad_fn is not None and out.dtype == torch.float32
        if reduction == "none":
            assert out.shape == (B, N * D)
            assert np.abs(f64(out) - want_loss).max() <= bound(0.0, want_loss)
            (out * w.to(gpu_device)).sum().backward()
        else:
            assert out.shape == ()
            want = want_loss.sum() / (n_kept if reduction == "mean" else 1)
            assert abs(float(out) - want) <= B * N * D * bound(0.0, want_loss) / (n_kept if reduction == "mean" else 1)
            out.backward()
        assert x.grad.shape == x.shape and x.grad.dtype == dt and x.grad.device == x.device
        want_grad = XO.grad(l64, *ifk, g64, eps)
        _, y_b = torch_fp32_yardstick(l64, ifk, eps, g64, want_loss, want_grad)
        got = x.grad.reshape(B, N * D, -1)[..., off:]
        e_b = grad_error(got, want_grad, dt)
        print(f"autograd {leaf} {kind} {reduction}: backward {e_b:.3e} (bound {bound(y_b, want_grad):.3e})")
        assert e_b <= bound(y_b, want_grad)
        if off:
            assert not x.grad[..., :off].any() and x.grad[..., off:].any()
    # the greedy tokens of the same launch; no graph without requires_grad or under no_grad
    x = init.to(gpu_device).requires_grad_(True)
    loss, toks = tok.cross_entropy_from_logits(x, target, label_smoothing=eps, return_tokens=True)
    assert torch.equal(toks, tok.greedy_tokens_from_logits(x)) and not toks.requires_grad and loss.grad_fn is not None
    plain = tok.cross_entropy_from_logits(x.detach(), target, label_smoothing=eps, reduction="none")
    with torch.no_grad():
        quiet, qt = tok.cross_entropy_from_logits(x, target, label_smoothing=eps, reduction="none", return_tokens=True)
    assert plain.grad_fn is None and not plain.requires_grad and quiet.grad_fn is None
    assert same_bits(plain, quiet) and torch.equal(qt, toks)
    assert same_bits(plain, tok.cross_entropy_from_logits(x, target, label_smoothing=eps, reduction="none").detach())


def test_other_input_forms(gpu_device):
    """float64 logits, host tensors, an int32 / float64 target, an empty batch, a batch in which every
    row is ignored (mean: NaN), and the BPE tokenizer's inherited method."""
    tok = make_tok(gpu_device)
    l = randn4((4, 140, 256), torch.float32, gpu_device, seed=6)
    t = random_tokens((4, 140), 256, 1, gpu_device)
    x = random_coeffs((4, 140), 2, gpu_device)
    want_t = tok.cross_entropy_from_logits(l, t, reduction="none")
    want_x = tok.cross_entropy_from_logits(l, x, reduction="none")
    assert same_bits(tok.cross_entropy_from_logits(l.double(), t.cpu(), reduction="none"), want_t)
    assert same_bits(tok.cross_entropy_from_logits(l.cpu(), t.to(torch.int32), reduction="none"), want_t)
    assert same_bits(tok.cross_entropy_from_logits(l, x.double().cpu().reshape(4, 10, 14), reduction="none"), want_x)
    host = l.cpu().double().requires_grad_(True)
    tok.cross_entropy_from_logits(host, x).backward()
    assert host.grad.shape == host.shape and host.grad.dtype == torch.float64 and host.grad.device.type == "cpu"
    assert abs(float(host.grad.sum())) <= 1e-4              # rows of p - q sum to 0
    assert tok.cross_entropy_from_logits(l[:0], t[:0], reduction="none").shape == (0, 140)
    assert float(tok.cross_entropy_from_logits(l[:0], t[:0], reduction="sum")) == 0.0
    nothing = torch.full((4, 140), IGNORE, dtype=torch.int64)
    assert torch.isnan(tok.cross_entropy_from_logits(l, nothing))
    assert float(tok.cross_entropy_from_logits(l, nothing, reduction="sum")) == 0.0
    assert torch.isnan(tok.cross_entropy_from_logits(l, torch.full((4, 140), NAN)))
    # the mean is over the rows that are not ignored, as torch's
    want = torch.nn.functional.cross_entropy(l.reshape(-1, 256), t.reshape(-1), ignore_index=IGNORE,
                                             label_smoothing=0.1)
    got = tok.cross_entropy_from_logits(l, t, label_smoothing=0.1)
    assert abs(float(got) - float(want)) <= 1e-5 * float(want)
    bpe = make_tok(gpu_device, cls=BEASTBsplineBPETokenizer)
    assert same_bits(bpe.cross_entropy_from_logits(l, x, reduction="none"), want_x)
