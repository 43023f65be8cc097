"""The windows entry point is ordered on the stream it is given: the probe of tests/stream_order.py
(see tests/test_gpu_stream_order.py for what it proves) on

section A   beast_encode_windows_f32 with the side stream's handle while torch's current stream is the
            null stream, on a dense table (every tile shares a staged segment) and on the same table
            shuffled (tiles gather); the frames have a good and a stale content, the window tables
            are never stale (they are indices);
section B   encode_windows under ``torch.cuda.stream(s)``, plain and with ``update_bounds``.
"""
import pytest
import torch

import windows_oracle as WO
import stream_order as SO
from stream_order import Case, api, capi
from stream_order import canary  # noqa: F401 (autouse)

pytestmark = pytest.mark.gpu

from beast_tokenizer_amd import BEASTBsplineTokenizer, _lib  # noqa: E402

PROBED = ["beast_encode_windows_f32"]
R, T, D, N = 1200, 50, 7, 10


def make_tok(dev, wide_bounds=True):
    tok = BEASTBsplineTokenizer(num_dof=D, num_basis=N, seq_len=T, vocab_size=256, device=str(dev))
    if wide_bounds:                       # the default +-0.02 is left for update_bounds to widen
        tok.w_min.fill_(-1.5)
        tok.w_max.fill_(1.5)
    tok._plan()
    torch.cuda.synchronize(dev)
    return tok


def good_frames(dev):
    gen = torch.Generator().manual_seed(17)
    x = torch.cumsum(torch.randn((R, D), generator=gen) * 0.08, 0)
    return (x - x.mean(0)).to(dev)


def tables(dev, shuffled):
    s, e, _ = make_tok_cpu().window_index([0, 500, R])
    if shuffled:
        perm = torch.randperm(len(s), generator=torch.Generator().manual_seed(3))
        s, e = s[perm], e[perm]
    return s, e, s.to(dev), e.to(dev)


def make_tok_cpu():
    return BEASTBsplineTokenizer(num_dof=D, num_basis=N, seq_len=T, device="cpu")


def expected_of(tok, good, s, e, dev):
    g = WO.gather_windows(good.cpu().numpy(), s.numpy(), e.numpy(), T)
    return tok.encode(torch.from_numpy(g).to(dev))


def raw_case(name, dev, shuffled):
    tok = make_tok(dev)
    p = tok._plan()
    good = good_frames(dev)
    buf = torch.empty_like(good)
    s, e, sd, ed = tables(dev, shuffled)
    W = len(s)
    params = torch.empty((W, D * N), device=dev)
    tokens = torch.empty((W, N * D), dtype=torch.int64, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)

    def call(h):
        _lib.run("beast_encode_windows_f32", buf.data_ptr(), R, buf.stride(0), buf.stride(1), D, sd.data_ptr(),
                 ed.data_ptr(), W, T, D, tok.joint_dof, p.p_src, p.p_proj, N, p.p_wmn, p.p_wmx, 256, 0,
                 params.data_ptr(), tokens.data_ptr(), counts.data_ptr(), h)
        return [params, tokens, counts]

    def check(exp):
        want_t, want = expected_of(tok, good, s, e, dev)
        assert torch.equal(exp[0], want["params"]) and torch.equal(exp[1], want_t)
        assert int(exp[2].sum()) == -(-W // 8) and int(exp[2][1 if shuffled else 0]) > 0
        assert shuffled or int(exp[2][1]) == 0
    return Case(name, tuple(PROBED), [(buf, good, good.flip(0).contiguous())], call,
                scratch=[params, tokens, counts], setup=counts.zero_, check_expected=check)


@capi("encode_windows[dense]", *PROBED)
def _(dev):
    return raw_case("encode_windows[dense]", dev, False)


@capi("encode_windows[shuffled]", *PROBED)
def _(dev):
    return raw_case("encode_windows[shuffled]", dev, True)


@pytest.mark.parametrize("cid", SO.ids(SO.CASES, __name__))
def test_capi_is_ordered_on_the_given_stream(cid, gpu_device):
    SO.check_capi(cid, gpu_device)


# ================================================================== B. the Python API ==
def api_case(name, dev, **kw):
    tok = make_tok(dev, wide_bounds=not kw)
    lo, hi = tok.w_min.clone(), tok.w_max.clone()
    good = good_frames(dev)
    x = torch.empty_like(good)
    s, e, sd, ed = tables(dev, False)

    def fn(_h):
        tok.w_min.copy_(lo)               # update_bounds moves them: every run starts from the same
        tok.w_max.copy_(hi)
        tokens, info = tok.encode_windows(x, sd, ed, return_tile_counts=True, **kw)
        return [tokens, info["params"], info["valid"], info["tile_counts"]]

    def check(exp):
        tok.w_min.copy_(lo)
        tok.w_max.copy_(hi)
        want_t, want = expected_of(tok, good, s, e, dev) if not kw else \
            tok.encode(torch.from_numpy(WO.gather_windows(good.cpu().numpy(), s.numpy(), e.numpy(), T)).to(dev), **kw)
        assert torch.equal(exp[0], want_t) and torch.equal(exp[1], want["params"])
    return Case(name, (name,), [(x, good, good.flip(0).contiguous())], fn, check_expected=check)


@api("encode_windows")
def _(dev):
    return api_case("encode_windows", dev)


@api("encode_windows[update_bounds]")
def _(dev):
    return api_case("encode_windows[update_bounds]", dev, update_bounds=True)


@pytest.mark.parametrize("cid", SO.ids(SO.API_CASES, __name__))
def test_python_api_is_ordered_on_the_current_stream(cid, gpu_device):
    SO.check_api(cid, gpu_device)
