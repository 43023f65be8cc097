"""The blend entry point is ordered on the stream it is given: the probe of tests/stream_order.py
(see tests/test_gpu_stream_order.py for what it proves) on

section A   beast_reconstruct_windows_f32 with the side stream's handle while torch's current stream
            is the null stream, from tokens and from normalised tokens; the tokens have a good and a
            stale content, the window tables are never stale (they are indices);
section B   reconstruct_windows and reconstruct_windows_continuous under ``torch.cuda.stream(s)``.
"""
import pytest
import torch

import blend_oracle as BO
import stream_order as SO
from stream_order import Case, api, capi
from stream_order import canary  # noqa: F401 (autouse)

pytestmark = pytest.mark.gpu

from beast_tokenizer_amd import BEASTBsplineTokenizer, _lib  # noqa: E402

PROBED = ["beast_reconstruct_windows_f32"]
R, T, D, N = 1200, 50, 7, 10
EPS = 2.0 ** -24


def make_tok(dev):
    tok = BEASTBsplineTokenizer(num_dof=D, num_basis=N, seq_len=T, vocab_size=256, device=str(dev))
    tok.w_min.fill_(-1.5)
    tok.w_max.fill_(1.5)
    tok._plan()
    torch.cuda.synchronize(dev)
    return tok


def tables(dev):
    s, e, _ = BEASTBsplineTokenizer(num_dof=D, num_basis=N, seq_len=T, device="cpu").window_index([0, 500, R], stride=2)
    return s, e, s.to(dev), e.to(dev)


def contents(W, dev, normalised):
    gen = torch.Generator().manual_seed(17)
    if normalised:
        good = torch.rand((W, N * D), generator=gen) * 2 - 1
    else:
        good = torch.randint(0, 256, (W, N * D), generator=gen)
    return good.to(dev), good.flip(0).contiguous().to(dev)


def check_expected(tok, good, s, e, bw, normalised):
    y = (tok.reconstruct_traj_continuous(good) if normalised else tok.reconstruct_traj(good)).cpu().numpy()

    def check(exp):
        want, cov, wt, C, ymax = BO.blend(y, s.numpy(), e.numpy(), bw.cpu().numpy(), R, -1.0)
        assert (abs(exp[0].cpu().numpy() - want) <= (2 * C + 2) * EPS * ymax).all()
        assert (exp[1].cpu().numpy() == cov).all() and (cov > 0).all()
    return check


def raw_case(name, dev, normalised):
    tok = make_tok(dev)
    p = tok._plan()
    s, e, sd, ed = tables(dev)
    W = len(s)
    good, stale = contents(W, dev, normalised)
    buf = torch.empty_like(good)
    bw = tok.blend_weights("exp", m=0.05)
    out = torch.empty((R, D), device=dev)
    cov = torch.empty(R, dtype=torch.int32, device=dev)
    wt = torch.empty(R, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)

    def call(h):
        _lib.run("beast_reconstruct_windows_f32", None if normalised else buf.data_ptr(),
                 buf.data_ptr() if normalised else None, W, D, tok.joint_dof, N, 256, 0, p.p_wmn, p.p_wmx, p.p_phi, T,
                 sd.data_ptr(), ed.data_ptr(), R, bw.data_ptr(), -1.0, p.p_dst, D, out.data_ptr(), D, cov.data_ptr(),
                 wt.data_ptr(), counts.data_ptr(), h)
        return [out, cov, wt, counts]

    return Case(name, tuple(PROBED), [(buf, good, stale)], call, scratch=[out, cov, wt, counts], setup=counts.zero_,
                check_expected=check_expected(tok, good, s, e, bw, normalised))


capi("reconstruct_windows[tokens]", *PROBED)(lambda dev: raw_case("reconstruct_windows[tokens]", dev, False))
capi("reconstruct_windows[ntokens]", *PROBED)(lambda dev: raw_case("reconstruct_windows[ntokens]", dev, True))


@pytest.mark.parametrize("cid", SO.ids(SO.CASES, __name__))
def test_capi_is_ordered_on_the_given_stream(cid, gpu_device):
    SO.check_capi(cid, gpu_device)


# ================================================================== B. the Python API ==
def api_case(name, dev, normalised):
    tok = make_tok(dev)
    s, e, sd, ed = tables(dev)
    good, stale = contents(len(s), dev, normalised)
    x = torch.empty_like(good)
    bw = tok.blend_weights("exp", m=0.05)

    def fn(_h):
        f = tok.reconstruct_windows_continuous if normalised else tok.reconstruct_windows
        out, info = f(x, sd, ed, R, blend=bw, fill=-1.0, return_tile_counts=True)
        return [out, info["coverage"], info["weight"], info["tile_counts"]]

    return Case(name, (name,), [(x, good, stale)], fn, check_expected=check_expected(tok, good, s, e, bw, normalised))


api("reconstruct_windows")(lambda dev: api_case("reconstruct_windows", dev, False))
api("reconstruct_windows_continuous")(lambda dev: api_case("reconstruct_windows_continuous", dev, True))


@pytest.mark.parametrize("cid", SO.ids(SO.API_CASES, __name__))
def test_python_api_is_ordered_on_the_current_stream(cid, gpu_device):
    SO.check_api(cid, gpu_device)
