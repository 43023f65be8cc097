"""The logits entry points are ordered on the stream they are given: the probe of
tests/stream_order.py (see tests/test_gpu_stream_order.py for what it proves) on

section A   beast_logits_expect and beast_logits_expect_bwd with the side stream's handle while
            torch's current stream is the null stream: fp32 contiguous, and bf16 through a strided
            slice (the element-access path);
section B   expected_params_from_logits, reconstruct_traj_from_logits, greedy_tokens_from_logits and
            the autograd backward under ``torch.cuda.stream(s)``.

launches nothing (a query; it only asks the stream for its device)
    beast_logits_resident_rows
"""
import numpy as np
import pytest
import torch

import logits_oracle as LO
import stream_order as SO
from stream_order import FLOOR, Case, api, api_case, api_tok, capi, f64, logits
from stream_order import canary  # noqa: F401 (autouse)

pytestmark = pytest.mark.gpu

from beast_tokenizer_amd import _lib  # noqa: E402

PROBED = ["beast_logits_expect", "beast_logits_expect_bwd"]
NO_LAUNCH = {"beast_logits_resident_rows": "a query: asks the stream for its device and launches nothing"}


def raw_case(name, dev, dtype, strided):
    """Forward then backward through the C-ABI on stream ``h``; with ``strided`` the logits and the
    gradient are 252-wide slices from element 13 of [B, K, 300] tensors (no row is 16-byte aligned)."""
    B, K, V, tau = 9, 140, 252 if strided else 256, 0.8
    width = 300 if strided else V
    good = logits((B, K, width), dtype, dev, seed=1)
    buf = torch.empty_like(good)
    gbuf = torch.empty_like(good)
    view = buf[..., 13:13 + V] if strided else buf
    gview = gbuf[..., 13:13 + V] if strided else gbuf
    mean = torch.empty((B, K), device=dev)
    amax = torch.empty((B, K), dtype=torch.int64, device=dev)
    stats = torch.empty((B, K, 2), device=dev)
    g = torch.randn((B, K), device=dev, generator=torch.Generator(dev).manual_seed(2))
    code = _lib.LOGITS_DTYPES[dtype]

    def call(h):
        _lib.run("beast_logits_expect", view.data_ptr(), code, B, K, V, view.stride(0), view.stride(1), tau, 5,
                 mean.data_ptr(), amax.data_ptr(), stats.data_ptr(), h)
        _lib.run("beast_logits_expect_bwd", view.data_ptr(), code, B, K, V, view.stride(0), view.stride(1), tau,
                 mean.data_ptr(), stats.data_ptr(), g.data_ptr(), gview.data_ptr(), gview.stride(0), gview.stride(1),
                 h)
        return [mean, amax, stats, gview]

    def check(exp):
        l64 = f64(good[..., 13:13 + V] if strided else good)
        want_mean, want_amax, _ = LO.expect(l64, tau)
        want_grad = LO.grad(l64, f64(g), tau)
        assert np.abs(f64(exp[0]) - want_mean).max() <= FLOOR
        assert np.array_equal(exp[1].cpu().numpy(), want_amax + 5)
        # a 16-bit gradient is rounded to its type: half an ulp, 2^-8 relative for bf16
        rel = 2.0 ** -8 if dtype != torch.float32 else 0.0
        assert np.all(np.abs(f64(exp[3]) - want_grad) <= FLOOR * np.abs(want_grad).max() + rel * np.abs(want_grad))
    return Case(name, tuple(PROBED), [(buf, good, good.flip(0).contiguous())], call,
                scratch=[mean, amax, stats, gbuf], check_expected=check)


@capi("logits_expect+bwd[fp32]", *PROBED)
def _(dev):
    return raw_case("logits_expect+bwd[fp32]", dev, torch.float32, False)


@capi("logits_expect+bwd[bf16-strided]", *PROBED)
def _(dev):
    return raw_case("logits_expect+bwd[bf16-strided]", dev, torch.bfloat16, True)


@pytest.mark.parametrize("cid", SO.ids(SO.CASES, __name__))
def test_capi_is_ordered_on_the_given_stream(cid, gpu_device):
    SO.check_capi(cid, gpu_device)


# ================================================================== B. the Python API ==
def decode_tok(dev):
    def bounds(tok):
        gen = torch.Generator().manual_seed(9)
        tok.w_min.copy_(-1.0 - torch.rand(140, generator=gen))
        tok.w_max.copy_(1.0 + torch.rand(140, generator=gen))
    tok = api_tok(dev, bounds)
    tok._basis.deriv_constants(tok.times.to(dev, torch.float32).reshape(-1), tok._times_version)
    torch.cuda.synchronize(dev)          # the cached constants are not what this module probes
    return tok


@api("expected_params_from_logits")
def _(dev):
    tok = decode_tok(dev)
    good = logits((9, 140, 256), torch.bfloat16, dev, seed=3)

    def check(exp):
        want_mean, want_amax, _ = LO.expect(f64(good), 0.8)
        assert np.abs(f64(exp[0]) - want_mean).max() <= FLOOR
        assert np.array_equal(exp[1].cpu().numpy(), want_amax)
    return api_case("expected_params_from_logits", good,
                    lambda x: list(tok.expected_params_from_logits(x, temperature=0.8, return_tokens=True)), check)


@api("reconstruct_traj_from_logits")
def _(dev):
    tok = decode_tok(dev)
    good = logits((9, 10, 14, 256), torch.float32, dev, seed=4)

    def fn(x):
        return list(tok.reconstruct_traj_from_logits(x, orders=(0, 1))) + [tok.reconstruct_traj_from_logits(x)]

    def check(exp):
        assert torch.equal(exp[0], exp[2]) or float((exp[0] - exp[2]).abs().max()) <= 1e-5
        assert exp[0].shape == (9, 50, 14) and bool(torch.isfinite(exp[1]).all())
    return api_case("reconstruct_traj_from_logits", good, fn, check)


@api("greedy_tokens_from_logits")
def _(dev):
    tok = decode_tok(dev)
    tok.set_llm_vocab_size(1000)
    good = logits((9, 140, 1000), torch.float16, dev, seed=5)

    def check(exp):
        assert np.array_equal(exp[0].cpu().numpy(), np.argmax(f64(good)[..., 744:], -1) + 744)
    return api_case("greedy_tokens_from_logits", good, lambda x: [tok.greedy_tokens_from_logits(x)], check)


@api("reconstruct_traj_from_logits[backward]")
def _(dev):
    """Forward and ``.backward()``: both backward launches ask for the current stream when autograd
    runs them (on the forward's stream), so the gradient is part of the probed sequence."""
    tok = decode_tok(dev)
    good = logits((9, 140, 256), torch.float32, dev, seed=6)
    gup = torch.randn((9, 50, 14), device=dev, generator=torch.Generator(dev).manual_seed(7))

    def fn(x):
        xr = x.detach().clone().requires_grad_()
        pos = tok.reconstruct_traj_from_logits(xr, temperature=0.8)
        pos.backward(gup)
        return [pos.detach(), xr.grad]

    def check(exp):
        assert exp[1].shape == good.shape and bool(torch.isfinite(exp[1]).all()) and bool(exp[1].any())
        assert float(exp[1].sum(-1).abs().max()) <= 1e-3 * float(exp[1].abs().max()) * 256   # softmax rows sum to 0
    return api_case("reconstruct_traj_from_logits[backward]", good, fn, check)


@pytest.mark.parametrize("cid", SO.ids(SO.API_CASES, __name__))
def test_python_api_is_ordered_on_the_current_stream(cid, gpu_device):
    SO.check_api(cid, gpu_device)
