"""The sampling entry point is ordered on the stream it is given: the probe of tests/stream_order.py
(see tests/test_gpu_stream_order.py for what it proves) on

section A   beast_sample_rows with the side stream's handle while torch's current stream is the null
            stream: fp32 contiguous, plain, and bf16 through a strided slice (the element-access path)
            with top-k and top-p; the logits and the uniforms are both inputs with a stale content;
section B   sample_tokens_from_logits under ``torch.cuda.stream(s)``: with the caller's uniforms, and
            with a generator, where the ``torch.rand`` the method issues is part of the probed sequence.
"""
import numpy as np
import pytest
import torch

import sample_oracle as SO
import stream_order
from stream_order import FLOOR, Case, api, api_case, api_tok, capi, f64, logits
from stream_order import canary  # noqa: F401 (autouse)

pytestmark = pytest.mark.gpu

from beast_tokenizer_amd import _lib  # noqa: E402

PROBED = ["beast_sample_rows"]


def check_draws(l64, u64, tok, lp, tau, top_k, top_p, off=0):
    """Tokens against the oracle's wherever the uniform is not within 4 FLOOR of an edge of its CDF
    (nearly everywhere), the log-probabilities of the drawn tokens everywhere."""
    kept = SO.kept_mask(l64, tau, top_k, top_p)
    want_tok, _ = SO.draw(l64, u64, tau, kept)
    C, e = SO.cdf(l64, tau, kept)
    edge = np.abs(C[None] / C[None, ..., -1:] - u64[..., None]).min(-1)
    clear = edge > 4 * FLOOR
    assert clear.mean() > 0.99
    got = tok.cpu().numpy() - off
    assert np.array_equal(got[clear], want_tok[clear])
    d, _ = SO.shifted(l64, tau)
    dt = np.take_along_axis(np.broadcast_to(d, got.shape + d.shape[-1:]), got[..., None], -1)[..., 0]
    want_lp = dt - np.log(C[..., -1])[None]
    assert np.all(np.abs(f64(lp) - want_lp) <= 4 * FLOOR * np.maximum(1.0, np.abs(want_lp)))


def raw_case(name, dev, dtype, strided, top_k, top_p):
    """beast_sample_rows through the C-ABI on stream ``h``; with ``strided`` the logits are a 252-wide
    slice from element 13 of a [B, K, 300] tensor (no row is 16-byte aligned)."""
    B, K, V, S, tau = 9, 140, 252 if strided else 256, 3, 0.8
    width = 300 if strided else V
    good = logits((B, K, width), dtype, dev, seed=1)
    good_u = torch.rand((S, B, K), generator=torch.Generator().manual_seed(3)).to(dev)
    buf, ubuf = torch.empty_like(good), torch.empty_like(good_u)
    view = buf[..., 13:13 + V] if strided else buf
    tok = torch.empty((S, B, K), dtype=torch.int64, device=dev)
    lp = torch.empty((S, B, K), device=dev)
    kept = torch.empty((B, K), dtype=torch.int32, device=dev)
    code = _lib.LOGITS_DTYPES[dtype]

    def call(h):
        _lib.run("beast_sample_rows", view.data_ptr(), code, B, K, V, view.stride(0), view.stride(1), tau, top_k,
                 top_p, ubuf.data_ptr(), S, 5, tok.data_ptr(), lp.data_ptr(), kept.data_ptr(), h)
        return [tok, lp, kept]

    def check(exp):
        l64 = f64(good[..., 13:13 + V] if strided else good)
        check_draws(l64, f64(good_u), exp[0], exp[1], tau, top_k, top_p, off=5)
        assert np.array_equal(exp[2].cpu().numpy(), SO.kept_mask(l64, tau, top_k, top_p).sum(-1))
    inputs = [(buf, good, good.flip(0).contiguous()), (ubuf, good_u, good_u.flip(1).contiguous())]
    return Case(name, tuple(PROBED), inputs, call, scratch=[tok, lp, kept], check_expected=check)


@capi("sample_rows[fp32-plain]", *PROBED)
def _(dev):
    return raw_case("sample_rows[fp32-plain]", dev, torch.float32, False, 0, 1.0)


@capi("sample_rows[bf16-strided-top-k-top-p]", *PROBED)
def _(dev):
    return raw_case("sample_rows[bf16-strided-top-k-top-p]", dev, torch.bfloat16, True, 50, 0.9)


@pytest.mark.parametrize("cid", stream_order.ids(stream_order.CASES, __name__))
def test_capi_is_ordered_on_the_given_stream(cid, gpu_device):
    stream_order.check_capi(cid, gpu_device)


# ================================================================== B. the Python API ==
@api("sample_tokens_from_logits[uniforms]")
def _(dev):
    tok = api_tok(dev)
    tok.set_llm_vocab_size(1000)
    good = logits((9, 140, 1000), torch.bfloat16, dev, seed=3)
    u = torch.rand((4, 9, 140), generator=torch.Generator().manual_seed(4)).to(dev)

    def check(exp):
        check_draws(f64(good)[..., 744:], f64(u), exp[0], exp[1], 0.8, 50, 0.9, off=744)

    def fn(x):
        return list(tok.sample_tokens_from_logits(x, temperature=0.8, top_k=50, top_p=0.9, num_samples=4, uniforms=u,
                                                  return_log_probs=True))
    return api_case("sample_tokens_from_logits[uniforms]", good, fn, check)


@api("sample_tokens_from_logits[generator]")
def _(dev):
    """The method draws its uniforms with ``torch.rand`` on the current stream from a generator seeded
    anew in every call, so the uniforms -- and with them the expected tokens -- are the same each time."""
    tok = api_tok(dev)
    good = logits((9, 10, 14, 256), torch.float32, dev, seed=6)
    gen = torch.Generator(dev)

    def fn(x):
        gen.manual_seed(11)
        return list(tok.sample_tokens_from_logits(x, num_samples=2, generator=gen, return_log_probs=True))

    def check(exp):
        gen.manual_seed(11)
        u = torch.rand((2, 9, 140), device=dev, generator=gen)
        check_draws(f64(good).reshape(9, 140, 256), f64(u), exp[0], exp[1], 1.0, 0, 1.0)
    return api_case("sample_tokens_from_logits[generator]", good, fn, check)


@pytest.mark.parametrize("cid", stream_order.ids(stream_order.API_CASES, __name__))
def test_python_api_is_ordered_on_the_current_stream(cid, gpu_device):
    stream_order.check_api(cid, gpu_device)
