"""The cross-entropy entry points are ordered on the stream they are given: the probe of
tests/stream_order.py (see tests/test_gpu_stream_order.py for what it proves) on

section A   beast_xent_rows and beast_xent_rows_bwd with the side stream's handle while torch's
            current stream is the null stream: fp32 contiguous with token targets, and bf16 through a
            strided slice (the element-access path) with coefficient targets;
section B   cross_entropy_from_logits and its autograd backward under ``torch.cuda.stream(s)``.
"""
import numpy as np
import pytest
import torch

import xent_oracle as XO
import stream_order as SO
from stream_order import FLOOR, Case, api, api_case, api_tok, capi, f64, logits
from stream_order import canary  # noqa: F401 (autouse)

pytestmark = pytest.mark.gpu

from beast_tokenizer_amd import _lib  # noqa: E402

PROBED = ["beast_xent_rows", "beast_xent_rows_bwd"]


def raw_case(name, dev, dtype, strided, coeffs):
    """Forward then backward through the C-ABI on stream ``h``; with ``strided`` the logits and the
    gradient are 252-wide slices from element 13 of [B, K, 300] tensors (no row is 16-byte aligned).
    The logits and the target are both inputs with a stale content."""
    B, K, V, eps = 9, 140, 252 if strided else 256, 0.1
    width = 300 if strided else V
    good = logits((B, K, width), dtype, dev, seed=1)
    gen = torch.Generator().manual_seed(3)
    if coeffs:
        good_t = (torch.rand((B, K), generator=gen) * 2.0 - 1.0).to(dev)
    else:
        good_t = torch.randint(0, V, (B, K), generator=gen).to(dev) + 5
    buf, tbuf, gbuf = torch.empty_like(good), torch.empty_like(good_t), torch.empty_like(good)
    view = buf[..., 13:13 + V] if strided else buf
    gview = gbuf[..., 13:13 + V] if strided else gbuf
    loss = torch.empty((B, K), device=dev)
    amax = torch.empty((B, K), dtype=torch.int64, device=dev)
    stats = torch.empty((B, K, 2), device=dev)
    g = torch.randn((B, K), device=dev, generator=torch.Generator(dev).manual_seed(2))
    code = _lib.LOGITS_DTYPES[dtype]
    targets = (None, tbuf.data_ptr()) if coeffs else (tbuf.data_ptr(), None)

    def call(h):
        _lib.run("beast_xent_rows", view.data_ptr(), code, B, K, V, view.stride(0), view.stride(1), *targets, 5, -100,
                 eps, loss.data_ptr(), stats.data_ptr(), amax.data_ptr(), h)
        _lib.run("beast_xent_rows_bwd", view.data_ptr(), code, B, K, V, view.stride(0), view.stride(1), *targets, 5,
                 -100, eps, stats.data_ptr(), g.data_ptr(), gview.data_ptr(), gview.stride(0), gview.stride(1), h)
        return [loss, amax, stats, gview]

    def check(exp):
        l64 = f64(good[..., 13:13 + V] if strided else good)
        h = good_t.cpu().numpy()
        ifk = XO.target_from_coeffs(h, V) if coeffs else XO.target_from_tokens(h, V, 5)
        want_loss, want_grad = XO.loss(l64, *ifk, eps), XO.grad(l64, *ifk, f64(g), eps)
        assert np.abs(f64(exp[0]) - want_loss).max() <= FLOOR * max(1.0, np.abs(want_loss).max())
        assert np.array_equal(exp[1].cpu().numpy(), XO.rows(l64)[2] + 5)
        # a 16-bit gradient is rounded to its type: half an ulp, 2^-8 relative for bf16
        rel = 2.0 ** -8 if dtype != torch.float32 else 0.0
        assert np.all(np.abs(f64(exp[3]) - want_grad) <= FLOOR * max(1.0, np.abs(want_grad).max())
                      + rel * np.abs(want_grad))
    inputs = [(buf, good, good.flip(0).contiguous()), (tbuf, good_t, good_t.flip(0).contiguous())]
    return Case(name, tuple(PROBED), inputs, call, scratch=[loss, amax, stats, gbuf], check_expected=check)


@capi("xent_rows+bwd[fp32-tokens]", *PROBED)
def _(dev):
    return raw_case("xent_rows+bwd[fp32-tokens]", dev, torch.float32, False, False)


@capi("xent_rows+bwd[bf16-strided-coeffs]", *PROBED)
def _(dev):
    return raw_case("xent_rows+bwd[bf16-strided-coeffs]", dev, torch.bfloat16, True, True)


@pytest.mark.parametrize("cid", SO.ids(SO.CASES, __name__))
def test_capi_is_ordered_on_the_given_stream(cid, gpu_device):
    SO.check_capi(cid, gpu_device)


# ================================================================== B. the Python API ==
@api("cross_entropy_from_logits")
def _(dev):
    tok = api_tok(dev)
    tok.set_llm_vocab_size(1000)
    good = logits((9, 140, 1000), torch.bfloat16, dev, seed=3)
    target = torch.randint(0, 256, (9, 140), generator=torch.Generator().manual_seed(4)).to(dev) + 744

    def check(exp):
        l64 = f64(good)[..., 744:]
        ifk = XO.target_from_tokens(target.cpu().numpy(), 256, 744)
        want = XO.loss(l64, *ifk, 0.1)
        assert np.abs(f64(exp[0]) - want).max() <= FLOOR * max(1.0, np.abs(want).max())
        assert np.array_equal(exp[1].cpu().numpy(), XO.rows(l64)[2] + 744)
        assert abs(float(exp[2]) - want.mean()) <= 1e-5 * want.mean()

    def fn(x):
        return list(tok.cross_entropy_from_logits(x, target, label_smoothing=0.1, reduction="none",
                                                  return_tokens=True)) + \
            [tok.cross_entropy_from_logits(x, target, label_smoothing=0.1)]
    return api_case("cross_entropy_from_logits", good, fn, check)


@api("cross_entropy_from_logits[backward]")
def _(dev):
    """Forward and ``.backward()``: the backward launch asks for the current stream when autograd runs
    it (on the forward's stream), so the gradient is part of the probed sequence."""
    tok = api_tok(dev)
    good = logits((9, 10, 14, 256), torch.float32, dev, seed=6)
    target = (torch.rand((9, 10, 14), generator=torch.Generator().manual_seed(7)) * 2.0 - 1.0).to(dev)

    def fn(x):
        xr = x.detach().clone().requires_grad_()
        loss = tok.cross_entropy_from_logits(xr, target)
        loss.backward()
        return [loss.detach(), xr.grad]

    def check(exp):
        l64 = f64(good).reshape(9, 140, 256)
        ifk = XO.target_from_coeffs(target.cpu().numpy().reshape(9, 140), 256)
        want = XO.grad(l64, *ifk, np.full((9, 140), 1.0 / 1260))
        assert exp[1].shape == good.shape
        assert np.abs(f64(exp[1]).reshape(9, 140, 256) - want).max() <= FLOOR
    return api_case("cross_entropy_from_logits[backward]", good, fn, check)


@pytest.mark.parametrize("cid", SO.ids(SO.API_CASES, __name__))
def test_python_api_is_ordered_on_the_current_stream(cid, gpu_device):
    SO.check_api(cid, gpu_device)
