"""The scoring entry points are ordered on the stream they are given: the probe of
tests/stream_order.py (see tests/test_gpu_stream_order.py for what it proves) on

section A   beast_score_rows and beast_score_rows_bwd with the side stream's handle while torch's
            current stream is the null stream: fp32 contiguous, plain, and bf16 through strided slices
            (the element-access path) with top-k and top-p and a reference; the logits, the reference
            and the tokens are all inputs with a stale content;
section B   score_tokens_from_logits under ``torch.cuda.stream(s)``: the forward alone, and the forward
            with ``.backward()``.
"""
import numpy as np
import pytest
import torch

import sample_oracle as SO
import score_oracle as SC
import stream_order
from stream_order import Case, api, api_case, api_tok, capi, close, f64, logits
from stream_order import canary  # noqa: F401 (autouse)

pytestmark = pytest.mark.gpu

from beast_tokenizer_amd import _lib  # noqa: E402
from beast_tokenizer_amd.beast_bspline_tokenizer import SCORE_STATS  # noqa: E402

PROBED = ["beast_score_rows", "beast_score_rows_bwd"]


def check_scores(l64, r64, tok, tau, top_k, top_p, off, lp, H, D, kept=None, grad=None, g=None, rel=0.0):
    """The outputs against the oracle on the oracle's own kept set (the inputs hold no near-ties)."""
    mask = SO.kept_mask(l64, tau, top_k, top_p)
    if kept is not None:
        assert np.array_equal(kept.cpu().numpy(), mask.sum(-1))
    close(f64(lp), SC.logprob(l64, mask, tok, tau, off)[0])
    close(f64(H), SC.entropy(l64, mask, tau))
    if D is not None:
        close(f64(D), SC.kl(l64, r64, mask, tau))
    if grad is not None:
        close(f64(grad), SC.grad(l64, mask, tau, tok, g[0], g[1], g[2], r64, off), rel)


def raw_case(name, dev, dtype, strided, top_k, top_p, with_ref):
    """Forward then backward through the C-ABI on stream ``h``; with ``strided`` the logits, the
    reference and the gradient are 252-wide slices from element 13 of [B, K, 300] tensors (no row is
    16-byte aligned)."""
    B, K, V, S, tau, off = 9, 140, 252 if strided else 256, 3, 0.8, 5
    width = 300 if strided else V
    good, good_r = logits((B, K, width), dtype, dev, seed=1), logits((B, K, width), dtype, dev, seed=2)
    good_t = torch.randint(0, V, (S, B, K), generator=torch.Generator().manual_seed(3)).to(dev) + off
    buf, rbuf, tbuf, gbuf = torch.empty_like(good), torch.empty_like(good_r), torch.empty_like(good_t), \
        torch.empty_like(good)
    cut = (lambda t: t[..., 13:13 + V]) if strided else (lambda t: t)
    view, rview, gview = cut(buf), cut(rbuf), cut(gbuf)
    lp = torch.empty((S, B, K), device=dev)
    H, D = torch.empty((B, K), device=dev), torch.empty((B, K), device=dev)
    kept = torch.empty((B, K), dtype=torch.int32, device=dev)
    stats = torch.empty((B, K, SCORE_STATS), device=dev)
    gen = torch.Generator(dev).manual_seed(4)
    g = [torch.randn(s, device=dev, generator=gen) for s in ((S, B, K), (B, K), (B, K))]
    code = _lib.LOGITS_DTYPES[dtype]
    rargs = (rview.data_ptr(), rview.stride(0), rview.stride(1)) if with_ref else (None, 0, 0)

    def call(h):
        head = (view.data_ptr(), code, B, K, V, view.stride(0), view.stride(1), *rargs, tau, top_k, top_p,
                tbuf.data_ptr(), S, off, -100)
        _lib.run("beast_score_rows", *head, lp.data_ptr(), H.data_ptr(), D.data_ptr() if with_ref else None,
                 kept.data_ptr(), stats.data_ptr(), h)
        _lib.run("beast_score_rows_bwd", *head, stats.data_ptr(), g[0].data_ptr(), g[1].data_ptr(),
                 g[2].data_ptr() if with_ref else None, gview.data_ptr(), gview.stride(0), gview.stride(1), h)
        return [lp, H, kept, stats, gview] + ([D] if with_ref else [])

    def check(exp):
        check_scores(f64(cut(good)), f64(cut(good_r)) if with_ref else None, good_t.cpu().numpy(), tau, top_k, top_p,
                     off, exp[0], exp[1], exp[5] if with_ref else None, exp[2], exp[4],
                     [f64(g[0]), f64(g[1]), f64(g[2]) if with_ref else None],
                     rel=2.0 ** -8 if dtype != torch.float32 else 0.0)
    inputs = [(buf, good, good.flip(0).contiguous()), (tbuf, good_t, good_t.flip(1).contiguous())]
    if with_ref:
        inputs.append((rbuf, good_r, good_r.flip(0).contiguous()))
    return Case(name, tuple(PROBED), inputs, call, scratch=[lp, H, D, kept, stats, gbuf], check_expected=check)


@capi("score_rows+bwd[fp32-plain]", *PROBED)
def _(dev):
    return raw_case("score_rows+bwd[fp32-plain]", dev, torch.float32, False, 0, 1.0, False)


@capi("score_rows+bwd[bf16-strided-top-k-top-p-ref]", *PROBED)
def _(dev):
    return raw_case("score_rows+bwd[bf16-strided-top-k-top-p-ref]", dev, torch.bfloat16, True, 50, 0.9, True)


@pytest.mark.parametrize("cid", stream_order.ids(stream_order.CASES, __name__))
def test_capi_is_ordered_on_the_given_stream(cid, gpu_device):
    stream_order.check_capi(cid, gpu_device)


# ================================================================== B. the Python API ==
@api("score_tokens_from_logits")
def _(dev):
    tok = api_tok(dev)
    tok.set_llm_vocab_size(1000)
    good = logits((9, 140, 1000), torch.bfloat16, dev, seed=3)
    ref = logits((9, 140, 1000), torch.bfloat16, dev, seed=5)
    tokens = torch.randint(0, 256, (4, 9, 140), generator=torch.Generator().manual_seed(4)).to(dev) + 744

    def check(exp):
        check_scores(f64(good)[..., 744:], f64(ref)[..., 744:], tokens.cpu().numpy(), 0.8, 50, 0.9, 744, *exp)

    def fn(x):
        return list(tok.score_tokens_from_logits(x, tokens, temperature=0.8, top_k=50, top_p=0.9, ref_logits=ref,
                                                 return_entropy=True))
    return api_case("score_tokens_from_logits", good, fn, check)


@api("score_tokens_from_logits[backward]")
def _(dev):
    """Forward and ``.backward()``: the backward launch asks for the current stream when autograd runs
    it (on the forward's stream), so the gradient is part of the probed sequence."""
    tok = api_tok(dev)
    good = logits((9, 10, 14, 256), torch.float32, dev, seed=6)
    tokens = torch.randint(0, 256, (9, 10, 14), generator=torch.Generator().manual_seed(7)).to(dev)

    def fn(x):
        xr = x.detach().clone().requires_grad_()
        logp, H, _ = tok.score_tokens_from_logits(xr, tokens, return_entropy=True)
        (logp.sum() + H.sum()).backward()
        return [logp.detach(), H.detach(), xr.grad]

    def check(exp):
        assert exp[2].shape == good.shape
        ones = np.ones((9, 140))
        check_scores(f64(good).reshape(9, 140, 256), None, tokens.cpu().numpy().reshape(1, 9, 140), 1.0, 0, 1.0, 0,
                     exp[0].reshape(1, 9, 140), exp[1], None, None, exp[2].reshape(9, 140, 256), [ones[None], ones, None])
    return api_case("score_tokens_from_logits[backward]", good, fn, check)


@pytest.mark.parametrize("cid", stream_order.ids(stream_order.API_CASES, __name__))
def test_python_api_is_ordered_on_the_current_stream(cid, gpu_device):
    stream_order.check_api(cid, gpu_device)
