"""beast_score_rows / beast_score_rows_bwd and ``score_tokens_from_logits`` on the GPU.

Bitwise against the sampler, no tolerance: the tokens beast_sample_rows drew, scored under the same
(temperature, top_k, top_p), have the bits of its ``logprob_out``, and ``kept_out`` has the bits of its
``kept_out`` -- plain and truncated, in the in-register and the two-pass kernels.

Against the float64 definition (tests/score_oracle.py): as in tests/test_gpu_sample.py the kept set is
taken from the kernel's own ``kept_out`` (its legality is the business of the sampler's tests, whose
kept set this is bit for bit) and logprob, H, KL and grad_logits are evaluated on that set.  Tolerances
are measured, not fixed in advance (the rule of tests/test_gpu_logits.py): 4x the largest error of
torch's own fp32 composition on the CPU -- ``masked_fill(-inf)`` -> ``log_softmax`` -> gather /
entropy / KL and its autograd, on the same inputs and the same mask -- against float64, with a floor of
16 * 2^-24 * max(1, max |oracle|).  A half / bf16 ``grad_logits`` is judged beyond one ulp of its type
at the oracle's value.  Every check prints what it measured.
"""
import numpy as np
import pytest
import torch

import score_oracle as SC
from beast_tokenizer_amd import BEASTBsplineBPETokenizer, _lib
from beast_tokenizer_amd.beast_bspline_tokenizer import SCORE_STATS
from test_gpu_logits import DTYPES, f64, make_tok, randn4, same_bits
from test_gpu_sample import BKS, TAUS, WIDEST, sample, uniforms
from test_gpu_xent import bound, grad_error

pytestmark = pytest.mark.gpu

IGNORE = SC.IGNORE
NAN = float("nan")
DRAWS = (1, 5, 64)
OFF = 3


# ------------------------------------------------------------------ raw entry points --
def strides(t):
    return (t.data_ptr(), t.stride(0), t.stride(1)) if t is not None else (None, 0, 0)


def fwd(l, tok, tau=1.0, top_k=0, top_p=1.0, ref=None, off=OFF, ignore=IGNORE, logprob=True, entropy=True, kl=True,
        kept=True, stats=True):
    """beast_score_rows on a [B, K, V] view with tokens [S, B, K] (or None); returns (logprob, entropy,
    kl, kept, stats), poisoned first, None where not asked for."""
    B, K, V = l.shape
    dev = l.device
    S = 0 if tok is None else tok.shape[0]
    assert tok is None or (tok.shape == (S, B, K) and tok.dtype == torch.int64 and tok.is_contiguous())
    lp = torch.full((S, B, K), 7.0, device=dev) if logprob and S else None
    H = torch.full((B, K), NAN, device=dev) if entropy else None
    D = torch.full((B, K), NAN, device=dev) if kl and ref is not None else None
    kp = torch.full((B, K), -7, dtype=torch.int32, device=dev) if kept else None
    st = torch.full((B, K, SCORE_STATS), NAN, device=dev) if stats else None
    _lib.run("beast_score_rows", l.data_ptr(), _lib.LOGITS_DTYPES[l.dtype], B, K, V, l.stride(0), l.stride(1),
             *strides(ref), tau, top_k, top_p, _lib.ptr(tok), S, off, ignore, _lib.ptr(lp), _lib.ptr(H), _lib.ptr(D),
             _lib.ptr(kp), _lib.ptr(st), _lib.stream_of(dev))
    return lp, H, D, kp, st


def bwd(l, tok, stats, g_lp=None, g_h=None, g_kl=None, tau=1.0, top_k=0, top_p=1.0, ref=None, off=OFF, ignore=IGNORE,
        out=None):
    """beast_score_rows_bwd into ``out`` (a [B, K, V] view; default: a fresh NaN-filled tensor)."""
    B, K, V = l.shape
    S = 0 if tok is None else tok.shape[0]
    if out is None:
        out = torch.full((B, K, V), NAN, dtype=l.dtype, device=l.device)
    _lib.run("beast_score_rows_bwd", l.data_ptr(), _lib.LOGITS_DTYPES[l.dtype], B, K, V, l.stride(0), l.stride(1),
             *strides(ref), tau, top_k, top_p, _lib.ptr(tok), S, off, ignore, stats.data_ptr(), _lib.ptr(g_lp),
             _lib.ptr(g_h), _lib.ptr(g_kl), out.data_ptr(), out.stride(0), out.stride(1), _lib.stream_of(l.device))
    return out


def both(l, tok, g, tau=1.0, top_k=0, top_p=1.0, ref=None, **kw):
    """(logprob, entropy, kl, kept, stats, grad) of one forward and one backward launch; ``g`` is
    (g_lp [S, B, K], g_h [B, K], g_kl [B, K])."""
    out = fwd(l, tok, tau, top_k, top_p, ref, **kw)
    return (*out, bwd(l, tok, out[4], g[0], g[1], g[2] if ref is not None else None, tau, top_k, top_p, ref, **kw))


def upstream(S, B, K, dev, seed):
    gen = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(s, generator=gen, dtype=torch.float32).to(dev) for s in ((S, B, K), (B, K), (B, K)))


def mixed_tokens(l, S, tau, top_k, top_p, seed, special=True):
    """[S, B, K] tokens + OFF: even draws from the sampler (always kept), odd draws uniform over the
    bins (mostly outside a truncated kept set); with ``special`` one ignored token where there is room."""
    B, K, V = l.shape
    drawn = sample(l, uniforms(S, B, K, l.device, seed), tau, top_k, top_p, off=OFF)[0]
    rnd = torch.randint(0, V, (S, B, K), generator=torch.Generator().manual_seed(seed + 1)).to(l.device) + OFF
    tok = torch.where((torch.arange(S, device=l.device) % 2 == 0)[:, None, None], drawn, rnd)
    if special and tok.numel() >= 4:
        tok.view(-1)[1] = IGNORE
    return tok.contiguous()


# ------------------------------------------------------------- bitwise against the sampler --
def sampler_agrees(l, tau, top_k, top_p, S, seed, tag):
    B, K, _ = l.shape
    u = uniforms(S, B, K, l.device, seed)
    tok, want_lp, want_kept = sample(l, u, tau, top_k, top_p, off=OFF)
    lp, _, _, kept, _ = fwd(l, tok, tau, top_k, top_p, entropy=False, stats=False)
    torch.cuda.synchronize(l.device)
    assert same_bits(kept, want_kept), f"{tag}: kept_out differs from the sampler's"
    assert same_bits(lp, want_lp), f"{tag}: logprob differs from the sampler's by " \
        f"{float((lp - want_lp).abs().nan_to_num(nan=9e9).max()):.3e}"
    assert bool(torch.isfinite(lp).all())
    # the other outputs change nothing: all of them asked for, and with a reference
    full = fwd(l, tok, tau, top_k, top_p, ref=l.flip(1))
    assert same_bits(full[0], want_lp) and same_bits(full[3], want_kept), tag


@pytest.mark.parametrize("BK", BKS, ids=lambda bk: f"B{bk[0]}K{bk[1]}")
@pytest.mark.parametrize("V", [2, 3, 255, 256, 257, 1000, 4097])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_plain_logprob_has_the_samplers_bits(dtype, V, BK, gpu_device):
    """Every temperature and every S in {1, 5, 64}; 4097: the two-pass kernels, whose S2 is the online sum."""
    l = randn4((*BK, V), DTYPES[dtype], gpu_device, seed=V * 1000 + BK[0])
    for n, tau in enumerate(TAUS):
        for S in DRAWS:
            sampler_agrees(l, tau, 0, 1.0, S, V + n, f"{dtype} V{V} B{BK[0]} K{BK[1]} tau {tau} S {S}")


@pytest.mark.parametrize("BK", BKS, ids=lambda bk: f"B{bk[0]}K{bk[1]}")
@pytest.mark.parametrize("V", [2, 3, 255, 256, 257, 1000, "widest"])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_truncated_logprob_has_the_samplers_bits(dtype, V, BK, gpu_device):
    """top_k in {0, 1, 5, V-1} x top_p in {0.1, 0.9, 1}, temperatures and S in rotation; "widest": the
    last in-register width of the dtype."""
    V = WIDEST[dtype] if V == "widest" else V
    l = randn4((*BK, V), DTYPES[dtype], gpu_device, seed=V * 1000 + BK[0] + 1)
    n = 0
    for top_k in sorted({0, 1, 5, V - 1}):
        for top_p in (0.1, 0.9, 1.0):
            tau, S = TAUS[n % 3], DRAWS[(n // 3 + n) % 3]
            sampler_agrees(l, tau, top_k, top_p, S, V + n, f"{dtype} V{V} B{BK[0]} K{BK[1]} tau {tau} k {top_k} "
                           f"p {top_p} S {S}")
            n += 1


def test_python_ratio_of_the_on_policy_step_is_exactly_one(gpu_device):
    tok = make_tok(gpu_device)
    tok.set_llm_vocab_size(1000)
    for dtype, kw in ((torch.bfloat16, dict(temperature=0.8, top_k=50, top_p=0.9)), (torch.float32, dict()),
                      (torch.float16, dict(temperature=3.0, top_p=0.5))):
        l = randn4((5, 140, 1000), dtype, gpu_device, seed=21)
        for S in (None, 16):
            t, old = tok.sample_tokens_from_logits(l, num_samples=S, return_log_probs=True, **kw)
            new = tok.score_tokens_from_logits(l, t, **kw)
            assert new.shape == t.shape and new.dtype == torch.float32
            assert bool((torch.exp(new - old) == 1.0).all()) and same_bits(new, old)
            lp2, H, D = tok.score_tokens_from_logits(l.reshape(5, 10, 14, 1000), t, return_entropy=True, **kw)
            assert same_bits(lp2, old) and H.shape == (5, 140) and D is None


# --------------------------------------------------------------------- against the oracle --
def kept_from_count(l64, c):
    """The value-closed set of the c largest logits of every row ([R, V], [R])."""
    ls = -np.sort(-l64, axis=-1)
    thr = np.take_along_axis(ls, (c - 1)[:, None], -1)
    mask = l64 >= thr
    assert np.array_equal(mask.sum(-1), c), "a kept set is not value-closed"
    return mask


def torch_fp32(l64, r64, mask, tau, rel, part, g):
    """torch's fp32 composition and its autograd on the CPU: (logprob [S, R], H, KL, grad)."""
    t = torch.tensor(l64, dtype=torch.float32, requires_grad=True)
    keep = torch.tensor(mask)
    lp = torch.log_softmax((t / tau).masked_fill(~keep, -np.inf), -1)
    pi = lp.exp()
    safe = lp.masked_fill(lp == -np.inf, 0.0)
    H = -(pi * safe).sum(-1)
    loss = (H * torch.tensor(g[1], dtype=torch.float32)).sum()
    got = lp.gather(-1, torch.tensor(rel.T)).T
    loss = loss + (torch.where(torch.tensor(part), got, torch.zeros_like(got))
                   * torch.tensor(g[0], dtype=torch.float32)).sum()
    D = None
    if r64 is not None:
        lr = torch.log_softmax(torch.tensor(r64, dtype=torch.float32) / tau, -1)
        D = (pi * (safe - lr.masked_fill(pi == 0, 0.0))).sum(-1)
        loss = loss + (D * torch.tensor(g[2], dtype=torch.float32)).sum()
    loss.backward()
    return got.detach().numpy(), H.detach().numpy(), None if D is None else D.detach().numpy(), t.grad.numpy()


def err(got, want, where=None):
    got = np.asarray(got, dtype=np.float64)
    d = np.abs(got - want) if where is None else np.abs(got[where] - want[where])
    return float(d.max()) if d.size else 0.0


def check_against_oracle(l, ref, tok, tau, top_k, top_p, tag, seed=0):
    """Forward and backward of the [B, K, V] device tensor ``l`` against the oracle on the kernel's own
    kept set; returns the outputs."""
    B, K, V = l.shape
    R, S = B * K, tok.shape[0]
    g = upstream(S, B, K, l.device, seed)
    out = both(l, tok, g, tau, top_k, top_p, ref)
    torch.cuda.synchronize(l.device)
    lp, H, D, kept, stats, grad = out
    l64 = f64(l).reshape(R, V)
    r64 = f64(ref).reshape(R, V) if ref is not None else None
    c = kept.cpu().numpy().astype(np.int64).reshape(R)
    assert ((c >= 1) & (c <= V)).all(), tag
    if not (1 <= top_k < V or top_p < 1.0):
        assert (c == V).all(), tag
    mask = kept_from_count(l64, c)
    tokens = tok.cpu().numpy().reshape(S, R)
    g64 = [f64(x).reshape(-1, R) if i == 0 else f64(x).reshape(R) for i, x in enumerate(g)]
    want_lp, part = SC.logprob(l64, mask, tokens, tau, OFF)
    want_h = SC.entropy(l64, mask, tau)
    want_d = SC.kl(l64, r64, mask, tau) if ref is not None else None
    want_grad = SC.grad(l64, mask, tau, tokens, g64[0], g64[1], g64[2] if ref is not None else None, r64, OFF)
    rel, ignored, bad = SC.classify(tokens, V, OFF)
    assert not bad.any()
    y_lp, y_h, y_d, y_grad = torch_fp32(l64, r64, mask, tau, rel, part, g64)
    fin = np.isfinite(want_lp) & ~ignored
    got_lp = f64(lp).reshape(S, R)
    assert np.array_equal(np.isneginf(got_lp), np.isneginf(want_lp)), f"{tag}: -inf log-probabilities differ"
    assert not got_lp[ignored].any(), f"{tag}: an ignored token must score exactly 0"
    b_lp = bound(err(y_lp, want_lp, fin), want_lp[fin])
    b_h = bound(err(y_h, want_h), want_h)
    b_g = bound(err(y_grad, want_grad), want_grad)
    e_lp, e_h = err(got_lp, want_lp, fin), err(f64(H).reshape(R), want_h)
    e_g = grad_error(grad.reshape(R, V), want_grad, l.dtype)
    msg = f"{tag} tau {tau} k {top_k} p {top_p} S {S}: logprob {e_lp:.3e} (bound {b_lp:.3e})  H {e_h:.3e} " \
          f"(bound {b_h:.3e})  grad {e_g:.3e} (bound {b_g:.3e})"
    e_d = b_d = 0.0
    if ref is not None:
        b_d = bound(err(y_d, want_d), want_d)
        e_d = err(f64(D).reshape(R), want_d)
        msg += f"  KL {e_d:.3e} (bound {b_d:.3e})"
    print(msg)
    assert e_lp <= b_lp and e_h <= b_h and e_d <= b_d and e_g <= b_g, msg
    g_out = f64(grad).reshape(R, V)
    assert not g_out[~mask].any(), f"{tag}: a gradient outside the kept set"
    st = f64(stats).reshape(R, SCORE_STATS)
    assert np.array_equal(st[:, 0], np.float32(l64.max(-1)) * np.float32(1.0 / tau))      # zmax, one rounding
    assert np.array_equal(st[:, 3], f64(H).reshape(R))
    return out


@pytest.mark.parametrize("BK", BKS, ids=lambda bk: f"B{bk[0]}K{bk[1]}")
@pytest.mark.parametrize("V", [2, 3, 255, 256, 257, 1000, 4097])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_plain_scores_against_the_oracle(dtype, V, BK, gpu_device):
    """logprob, H, KL and the gradient of all three; the temperature and S rotate over the cases so
    that every value meets every kernel form."""
    n = list(DTYPES).index(dtype) + BKS.index(BK) + V
    tau, S = TAUS[n % 3], DRAWS[(n // 3) % 3]
    l = randn4((*BK, V), DTYPES[dtype], gpu_device, seed=V * 1000 + BK[0])
    ref = randn4((*BK, V), DTYPES[dtype], gpu_device, seed=V * 1000 + BK[0] + 7, scale=3.0)
    tok = mixed_tokens(l, S, tau, 0, 1.0, seed=V)
    check_against_oracle(l, ref, tok, tau, 0, 1.0, f"{dtype} V{V} B{BK[0]} K{BK[1]}", seed=n)


@pytest.mark.parametrize("BK", BKS, ids=lambda bk: f"B{bk[0]}K{bk[1]}")
@pytest.mark.parametrize("V", [2, 3, 255, 256, 257, 1000, "widest"])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_truncated_scores_against_the_oracle(dtype, V, BK, gpu_device):
    """Two truncations per case out of top_k in {0, 1, 5, V-1} x top_p in {0.1, 0.9, 1}, in rotation
    together with the temperature and S; the tokens are half the sampler's, half arbitrary bins."""
    V = WIDEST[dtype] if V == "widest" else V
    n = list(DTYPES).index(dtype) + 2 * BKS.index(BK) + V
    l = randn4((*BK, V), DTYPES[dtype], gpu_device, seed=V * 1000 + BK[0] + 1)
    ref = randn4((*BK, V), DTYPES[dtype], gpu_device, seed=V * 1000 + BK[0] + 8, scale=3.0)
    combos = [(k, p) for k in sorted({0, 1, 5, V - 1}) for p in (0.1, 0.9, 1.0) if 1 <= k < V or p < 1.0]
    for i in range(2):
        top_k, top_p = combos[(n + i * 5) % len(combos)]
        tau, S = TAUS[(n + i) % 3], DRAWS[(n // 3 + i) % 3]
        tok = mixed_tokens(l, S, tau, top_k, top_p, seed=V + i)
        check_against_oracle(l, ref if i == 0 else None, tok, tau, top_k, top_p, f"{dtype} V{V} B{BK[0]} K{BK[1]}",
                             seed=n + i)


def test_each_output_and_each_upstream_gradient_alone(gpu_device):
    """Every output asked for alone has the bits it has among the others; the gradients of the three
    upstream parts given alone add up to the gradient of all three within the oracle's bound."""
    for dtype, V, kw in ((torch.float32, 256, dict(tau=0.8, top_k=50, top_p=0.9)), (torch.bfloat16, 4097, dict(tau=1.0))):
        l = randn4((3, 7, V), dtype, gpu_device, seed=V)
        ref = randn4((3, 7, V), dtype, gpu_device, seed=V + 1)
        tok = mixed_tokens(l, 5, kw["tau"], kw.get("top_k", 0), kw.get("top_p", 1.0), seed=2)
        g = upstream(5, 3, 7, gpu_device, 4)
        full = both(l, tok, g, ref=ref, **kw)
        names = ("logprob", "entropy", "kl", "kept", "stats")
        for i, name in enumerate(names):
            only = fwd(l, tok if name in ("logprob", "stats") else None, ref=ref if name in ("kl", "stats") else None,
                       **{n: n == name for n in names}, **kw)
            if name == "stats":
                assert same_bits(only[4], full[4])
            else:
                assert same_bits(only[i], full[i]), name
                assert all(o is None for j, o in enumerate(only) if j != i)
        want = SC.grad(f64(l), kept_from_count(f64(l).reshape(21, V), full[3].cpu().numpy().reshape(21).astype(np.int64))
                       .reshape(3, 7, V), kw["tau"], tok.cpu().numpy(), f64(g[0]), f64(g[1]), f64(g[2]), f64(ref), OFF)
        parts = [bwd(l, tok, full[4], g[0], None, None, ref=None, **kw), bwd(l, None, full[4], None, g[1], None, **kw),
                 bwd(l, None, full[4], None, None, g[2], ref=ref, **kw)]
        total = sum(f64(p) for p in parts)
        # every part is rounded to the dtype on its own
        slack = (2.0 ** -8 if dtype != torch.float32 else 2.0 ** -23) * sum(np.abs(f64(p)).max() for p in parts)
        assert np.abs(total - want).max() <= slack + 16 * 2.0 ** -24 * max(1.0, np.abs(want).max())


# ---------------------------------------------------------------------------- special rows --
def test_special_tokens_and_rows(gpu_device):
    """Ignored, outside the kept set, out of range, on a -inf logit; rho_v = 0 < pi_v; top_k = 1; a
    peaked row; and NaN / +inf / all -inf rows between good neighbours."""
    dev, V = gpu_device, 256
    l = randn4((2, 6, V), torch.float32, dev, seed=77)
    l[0, 1, 9] = -np.inf                       # a -inf logit
    l[0, 2] = -3.0
    l[0, 2, 100] = 57.0                        # one logit 60 above the rest
    ref = randn4((2, 6, V), torch.float32, dev, seed=78)
    ref[0, 1, 9] = -np.inf                     # rho_v == 0 where pi_v == 0: the term is exactly 0
    top = l.argmax(-1)
    low = l.argmin(-1)
    tok = torch.stack([top, low, top, top, top]) + OFF
    tok[2, 0, 0] = IGNORE                      # row (0, 0): draws 0..4 = top, low (not kept), ignored, top, top
    tok[1, 0, 1] = 9 + OFF                     # row (0, 1): a token on the -inf logit
    tok[3, 1, 0] = V + OFF                     # row (1, 0): out of range above
    tok[4, 1, 1] = OFF - 1                     # row (1, 1): out of range below
    tok = tok.contiguous()
    g = upstream(5, 2, 6, dev, 5)
    kw = dict(tau=1.0, top_k=40, top_p=0.95, ref=ref)
    lp, H, D, kept, stats, grad = both(l, tok, g, **kw)
    torch.cuda.synchronize(dev)
    lp_c, grad_c = lp.cpu(), grad.cpu()
    assert lp_c[2, 0, 0] == 0.0 and lp_c[1, 0, 0] == -np.inf and lp_c[1, 0, 1] == -np.inf
    assert torch.isnan(lp_c[3, 1, 0]) and torch.isnan(lp_c[4, 1, 1])
    assert torch.isnan(grad_c[1, 0]).all() and torch.isnan(grad_c[1, 1]).all()
    assert not torch.isnan(lp_c[:, 1, 2:]).any() and torch.isfinite(grad_c[1, 2:]).all()
    assert torch.isfinite(H).all() and torch.isfinite(D).all()
    assert grad_c[0, 1, 9] == 0.0 and torch.isfinite(grad_c[0]).all()
    # the draws that take no part leave no trace: the same row with their upstream gradients changed
    g2 = (g[0].clone(), g[1], g[2])
    g2[0][2, 0, 0] = 1e6
    g2[0][1, 0, 0] = -1e6
    g2[0][1, 0, 1] = 1e6
    grad2 = bwd(l, tok, stats, *g2, **kw)
    assert same_bits(grad2[0], grad[0])
    # and against the oracle on the rows without an out-of-range token
    check_against_oracle(l[:1], ref[:1], tok[:, :1].contiguous(), 1.0, 40, 0.95, "special rows")
    check_against_oracle(l[:1], ref[:1], tok[:, :1].contiguous(), 1.0, 0, 1.0, "special rows, plain")
    # rho_v == 0 < pi_v: +inf, with and without the truncation (bin 5 of row (0, 3) is surely kept when it is the top)
    l2, ref2 = l.clone(), ref.clone()
    l2[0, 3, 5] = 30.0
    ref2[0, 3, 5] = -np.inf
    for k in (0, 40):
        D2 = fwd(l2, None, 1.0, k, 1.0, ref=ref2, logprob=False)[2].cpu()
        assert D2[0, 3] == np.inf and torch.isfinite(D2[0, :3]).all() and torch.isfinite(D2[1]).all()
    # the peaked row keeps its entropy within the bound (checked above); it is tiny and not negative
    assert 0.0 <= float(H[0, 2]) < 1e-20
    # top_k = 1: logprob 0 and H 0 to rounding, a zero gradient from g_s
    one = both(l, torch.stack([top]).contiguous() + OFF, (g[0][:1].contiguous(), g[1], g[2]), 3.0, 1, 1.0)
    assert float(one[0].abs().max()) <= 16 * 2.0 ** -24 and float(one[1].abs().max()) <= 16 * 2.0 ** -24
    assert bool((one[3] == 1).all())
    only_lp = bwd(l, torch.stack([top]).contiguous() + OFF, one[4], g[0][:1].contiguous(), None, None, 3.0, 1, 1.0)
    assert float(only_lp.abs().max()) <= 16 * 2.0 ** -24 * float(g[0].abs().max())
    # unspecified rows do not disturb their neighbours
    for dtype, width in ((torch.float32, 256), (torch.bfloat16, 4097)):
        good = randn4((1, 7, width), dtype, dev, seed=80)
        gref = randn4((1, 7, width), dtype, dev, seed=81)
        t = mixed_tokens(good, 5, 1.0, 0, 1.0, seed=3, special=False)
        gg = upstream(5, 1, 7, dev, 6)
        want = both(good, t, gg, ref=gref)
        ill, iref = good.clone(), gref.clone()
        ill[0, 1, 3] = NAN
        ill[0, 3, 200] = np.inf
        ill[0, 5] = -np.inf
        iref[0, 1] = -np.inf
        iref[0, 3, 0] = NAN
        got = both(ill, t, gg, ref=iref)
        sound = torch.tensor([0, 2, 4, 6], device=dev)
        for i, (a, b) in enumerate(zip(got, want)):                # logprob is [S, 1, K], the others [1, K, ...]
            assert same_bits(a.index_select(2 if i == 0 else 1, sound), b.index_select(2 if i == 0 else 1, sound)), i


# ------------------------------------------------------------------------- family contract --
@pytest.mark.parametrize("V", [257, 4097])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_runs_agree_bitwise_and_rows_do_not_depend_on_the_batch(dtype, V, gpu_device):
    l = randn4((6, 11, V), DTYPES[dtype], gpu_device, seed=V)
    ref = randn4((6, 11, V), DTYPES[dtype], gpu_device, seed=V + 1)
    for kw in (dict(), dict(tau=0.8, top_k=50, top_p=0.9)) if V == 257 else (dict(tau=3.0),):
        tok = mixed_tokens(l, 5, kw.get("tau", 1.0), kw.get("top_k", 0), kw.get("top_p", 1.0), seed=6)
        g = upstream(5, 6, 11, gpu_device, 8)
        first = both(l, tok, g, ref=ref, **kw)
        again = both(l, tok, g, ref=ref, **kw)
        assert all(same_bits(a, b) for a, b in zip(first, again))
        for b, k in ((0, 0), (0, 2), (2, 5), (5, 10)):
            cut = lambda t, lead: t[:, b:b + 1, k:k + 1].contiguous() if lead else t[b:b + 1, k:k + 1]   # noqa: E731
            one = both(cut(l, False), cut(tok, True), (cut(g[0], True), cut(g[1], False).contiguous(),
                                                       cut(g[2], False).contiguous()), ref=cut(ref, False), **kw)
            for i, (a, w) in enumerate(zip(one, first)):
                assert same_bits(a, cut(w, i == 0).contiguous()), (i, b, k)


@pytest.mark.parametrize("start", [13, 48])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_strided_slices_equal_the_contiguous_tensor_bitwise(dtype, start, gpu_device):
    """A 252-wide slice of a [B, K, 300] tensor from element 13 (no row is 16-byte aligned) and from 48;
    the reference is a slice with strides of its own ([B, K, 280] from element 7); a gradient written
    into a view with gsk > V leaves the gaps untouched."""
    dt, V = DTYPES[dtype], 252
    full = randn4((5, 9, 300), dt, gpu_device, seed=start)
    rfull = randn4((5, 9, 280), dt, gpu_device, seed=start + 1)
    view, rview = full[..., start:start + V], rfull[..., 7:7 + V]
    if start == 13:
        assert not any(view[b, k].data_ptr() % 16 == 0 for b in range(5) for k in range(9))
    flat, rflat = view.contiguous(), rview.contiguous()
    for kw in (dict(), dict(tau=0.8, top_k=50, top_p=0.9)):
        tok = mixed_tokens(flat, 5, kw.get("tau", 1.0), kw.get("top_k", 0), kw.get("top_p", 1.0), seed=3)
        g = upstream(5, 5, 9, gpu_device, 4)
        want = both(flat, tok, g, ref=rflat, **kw)
        assert not torch.isnan(want[5]).any()
        got = fwd(view, tok, ref=rview, **kw)
        assert all(same_bits(a, b) for a, b in zip(got, want[:5]))
        out = torch.full((5, 9, 300), NAN, dtype=dt, device=gpu_device)
        bwd(view, tok, got[4], *g, ref=rview, out=out[..., start:start + V], **kw)
        assert same_bits(out[..., start:start + V].contiguous(), want[5])
        assert torch.isnan(out[..., :start]).all() and torch.isnan(out[..., start + V:]).all()
        out.fill_(NAN)
        bwd(flat, tok, want[4], *g, ref=rflat, out=out[..., start:start + V], **kw)
        assert same_bits(out[..., start:start + V].contiguous(), want[5])
        assert torch.isnan(out[..., :start]).all() and torch.isnan(out[..., start + V:]).all()
        assert same_bits(bwd(view, tok, got[4], *g, ref=rview, **kw), want[5])


def test_grid_stride_over_four_times_the_resident_rows(gpu_device):
    """Four times as many rows as a decode launch keeps resident (beast_logits_resident_rows; the
    scoring kernels hold more registers, so they keep no more rows resident than it): every workgroup
    walks several groups of rows.  The launch over everything is compared bitwise, on sampled rows,
    with launches that fit the resident grid, and a sample goes against the oracle."""
    lib = _lib.load()
    code = _lib.LOGITS_DTYPES[torch.bfloat16]
    resident = max(lib.beast_logits_resident_rows(code, 256, b, _lib.stream_of(gpu_device)) for b in (0, 1))
    assert resident > 0
    K = 140
    B = -(-4 * resident // K)
    print(f"grid stride: {B * K} rows over {resident} resident")
    l = randn4((B, K, 256), torch.bfloat16, gpu_device, seed=5)
    ref = randn4((B, K, 256), torch.bfloat16, gpu_device, seed=6)
    kw = dict(tau=0.8, top_k=50, top_p=0.9)
    tok = mixed_tokens(l, 2, 0.8, 50, 0.9, seed=1)
    g = upstream(2, B, K, gpu_device, 2)
    whole = both(l, tok, g, ref=ref, **kw)
    step = max(17, B // 8)
    check_against_oracle(l[::step].contiguous(), ref[::step].contiguous(), tok[:, ::step].contiguous(), 0.8, 50, 0.9,
                         "grid stride sample")
    for sl in (slice(None, None, step), slice(0, 3), slice(B - 3, B)):
        part = both(l[sl].contiguous(), tok[:, sl].contiguous(), (g[0][:, sl].contiguous(), g[1][sl].contiguous(),
                                                                 g[2][sl].contiguous()), ref=ref[sl].contiguous(), **kw)
        assert l[sl].shape[0] * K <= resident
        for i, (a, b) in enumerate(zip(part, whole)):
            assert same_bits(a, (b[:, sl] if i == 0 else b[sl]).contiguous()), i


# -------------------------------------------------------------------- autograd end to end --
@pytest.mark.parametrize("cls", [None, BEASTBsplineBPETokenizer], ids=["bspline", "bpe"])
def test_ppo_shaped_loss_reaches_only_the_action_slice(cls, gpu_device):
    """-(A logp).mean() - c_H H.mean() + c_KL KL.mean() on a full-LLM-vocabulary bf16 tensor: the
    gradient is non-zero only in the action slice, where it equals the raw backward call's."""
    tok = make_tok(gpu_device) if cls is None else make_tok(gpu_device, cls=cls)
    tok.set_llm_vocab_size(1000)
    B, K, S, kw = 4, 140, 8, dict(temperature=0.8, top_k=50, top_p=0.9)
    leaf = randn4((B, K, 1000), torch.bfloat16, gpu_device, seed=41).requires_grad_()
    ref = randn4((B, K, 1000), torch.bfloat16, gpu_device, seed=42)
    t = tok.sample_tokens_from_logits(leaf.detach(), num_samples=S, **kw)
    A = torch.randn((S, B, K), generator=torch.Generator().manual_seed(43)).to(gpu_device)
    logp, H, D = tok.score_tokens_from_logits(leaf, t, ref_logits=ref, return_entropy=True, **kw)
    assert logp.requires_grad and H.requires_grad and D.requires_grad
    loss = -(A * logp).mean() - 0.01 * H.mean() + 0.1 * D.mean()
    loss.backward()
    assert leaf.grad.shape == leaf.shape and leaf.grad.dtype == torch.bfloat16
    assert not leaf.grad[..., :744].any() and bool(leaf.grad[..., 744:].any())
    rows = leaf.detach()[..., 744:]
    out = fwd(rows, t, 0.8, 50, 0.9, ref=ref[..., 744:], off=744)
    assert same_bits(out[0], logp.detach()) and same_bits(out[1], H.detach()) and same_bits(out[2], D.detach())
    heads = [o.clone().requires_grad_() for o in out[:3]]                     # the upstream gradients autograd forms
    ups = torch.autograd.grad(-(A * heads[0]).mean() - 0.01 * heads[1].mean() + 0.1 * heads[2].mean(), heads)
    raw = bwd(rows, t, out[4], *(u.contiguous() for u in ups), 0.8, 50, 0.9, ref=ref[..., 744:], off=744)
    assert same_bits(leaf.grad[..., 744:].contiguous(), raw)
    # without requires_grad, or under no_grad, no graph is recorded
    assert not tok.score_tokens_from_logits(leaf.detach(), t, **kw).requires_grad
    with torch.no_grad():
        assert not tok.score_tokens_from_logits(leaf, t, **kw).requires_grad
    # entropy alone, without tokens
    none, H2, D2 = tok.score_tokens_from_logits(leaf.detach(), return_entropy=True, **kw)
    assert none is None and D2 is None and same_bits(H2, H.detach())
