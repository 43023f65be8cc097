"""Argument validation of beast_encode_windows_f32 and of the tokenizer's encode_windows family: it
all runs before any HIP call, so no GPU is needed."""
import ctypes as C
import inspect

import pytest
import torch

from beast_tokenizer_amd import BEASTBsplineBPETokenizer, BEASTBsplineTokenizer, _lib

FAKE = C.c_void_p(16)                   # never dereferenced: validation fails first
NAME = "beast_encode_windows_f32"


def win_args(**kw):
    """The argument list of beast_encode_windows_f32, in the header's order."""
    a = dict(frames=FAKE, R=1000, sr=14, sd=1, row_elems=14, win_start=FAKE, win_end=FAKE, W=4, T=50, D=14,
             n_joint=12, dof_src=FAKE, proj=FAKE, N=10, w_min=FAKE, w_max=FAKE, vocab=256, tok_offset=0,
             params_out=FAKE, tokens_out=FAKE, tile_counts=FAKE, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


def test_signature_is_bound_and_the_abi_version_moved():
    assert len(_lib.SIGNATURES[NAME][1]) == len(win_args()) == 22
    assert _lib.ABI_VERSION >= 5 and _lib.load().beast_abi_version() == _lib.ABI_VERSION


@pytest.mark.parametrize("kw", [dict(N=17), dict(T=257), dict(D=65, n_joint=63, row_elems=65, sr=65)])
def test_outside_the_envelope_is_unsupported(kw):
    lib = _lib.load()
    rc = lib.beast_encode_windows_f32(*win_args(**kw))
    assert rc == _lib.BEAST_E_UNSUPPORTED
    with pytest.raises(NotImplementedError, match="beast_encode_windows_f32 supports"):
        _lib.check(rc, NAME)


@pytest.mark.parametrize("kw", [
    dict(frames=None), dict(win_start=None), dict(win_end=None), dict(dof_src=None), dict(proj=None),
    dict(params_out=None, tokens_out=None), dict(R=0), dict(R=-1), dict(W=-1), dict(T=0), dict(N=0),
    dict(D=0, n_joint=0), dict(sr=-1), dict(sd=-1), dict(n_joint=15), dict(n_joint=-1), dict(row_elems=0),
    dict(vocab=1), dict(w_min=None), dict(w_max=None),
    dict(sr=13),                        # rows of 14 floats 13 apart overlap
    dict(sd=2),                         # a row of 14 elements 2 apart does not end within sr = 14
])
def test_bad_arguments_are_invalid(kw):
    lib = _lib.load()
    assert lib.beast_encode_windows_f32(*win_args(**kw)) == _lib.BEAST_E_INVALID
    assert NAME.encode() in lib.beast_last_error()
    with pytest.raises(ValueError):
        _lib.check(_lib.BEAST_E_INVALID, NAME)


@pytest.mark.parametrize("kw", [
    dict(W=0),
    dict(W=0, R=0),                                                # no windows need no frames
    dict(W=0, tokens_out=None, w_min=None, w_max=None, vocab=0),   # params only: no quantiser arguments
    dict(W=0, params_out=None),                                    # tokens only
    dict(W=0, tile_counts=None),                                   # the counters are optional
    dict(W=0, sr=28, sd=2),                                        # strided elements, rows that do not overlap
    dict(W=0, row_elems=16, sr=40),                                # wide rows, apart in memory
])
def test_no_windows_with_good_arguments_is_a_no_op(kw):
    assert _lib.load().beast_encode_windows_f32(*win_args(**kw)) == _lib.BEAST_OK


# ------------------------------------------------------------ the Python surface --
def cpu_tok(cls=BEASTBsplineTokenizer, **kw):
    return cls(num_dof=7, num_basis=10, seq_len=50, device="cpu", **kw)


def calls(tok):
    return (tok.encode_windows, tok.encode_continuous_windows, tok.fit_parameters_windows)


def test_conditioned_tokenizers_are_not_implemented():
    x, s, e = torch.zeros(60, 7), torch.tensor([0, 5]), torch.tensor([60, 60])
    for kw in (dict(init_cond_order=1), dict(end_cond_order=1), dict(init_cond_order=2, end_cond_order=-1)):
        for call in calls(cpu_tok(**kw)):
            with pytest.raises(NotImplementedError, match="init_cond_order"):
                call(x, s, e)


@pytest.mark.parametrize("s,e", [
    (torch.zeros(2, 1, dtype=torch.int64), torch.ones(2, 1, dtype=torch.int64)),    # not 1-d
    (torch.zeros(2, dtype=torch.int64), torch.ones(3, dtype=torch.int64)),          # two lengths
    (torch.zeros(2, dtype=torch.int32), torch.ones(2, dtype=torch.int32)),          # not int64
    (torch.zeros(2), torch.ones(2)),
    (torch.tensor(0), torch.tensor(1)),
])
def test_bad_table_shapes_are_value_errors(s, e):
    for call in calls(cpu_tok()):
        with pytest.raises(ValueError, match="int64 .W. tables"):
            call(torch.zeros(60, 7), s, e)


@pytest.mark.parametrize("s,e", [([0, 7], [60, 7]), ([0, 9], [60, 8]), ([-1, 0], [60, 60]), ([0, 0], [60, 61])])
def test_host_tables_are_range_checked(s, e):
    for call in calls(cpu_tok()):
        with pytest.raises(ValueError, match="0 <= start < end <= R=60"):
            call(torch.zeros(60, 7), torch.tensor(s), torch.tensor(e))


def test_bad_frames():
    s, e = torch.tensor([0]), torch.tensor([60])
    for call in calls(cpu_tok()):
        with pytest.raises(ValueError, match="flat frame buffer"):
            call(torch.zeros(2, 60, 7), s, e)
        with pytest.raises(IndexError, match="out of bounds for dimension 1"):
            call(torch.zeros(60, 6), s, e)
    with pytest.raises(ValueError, match="chunk_windows"):
        cpu_tok().fit_parameters_windows(torch.zeros(60, 7), s, e, chunk_windows=0)


def test_host_tokenizers_are_refused():
    """After every argument check: there is no CPU fallback."""
    x, s, e = torch.zeros(60, 7), torch.tensor([0, 5]), torch.tensor([60, 60])
    tok = cpu_tok()
    for call in (lambda: tok.encode_windows(x, s, e), lambda: tok.encode_windows(x, s, e, update_bounds=True),
                 lambda: tok.encode_windows(x, s[:0], e[:0]), lambda: tok.encode_continuous_windows(x, s, e),
                 lambda: tok.fit_parameters_windows(x, s, e, chunk_windows=1)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_bpe_tokenizer_has_the_method():
    assert "encode_windows" in vars(BEASTBsplineBPETokenizer)
    tok = cpu_tok(BEASTBsplineBPETokenizer)
    with pytest.raises(ValueError, match="0 <= start < end"):
        tok.encode_windows(torch.zeros(60, 7), torch.tensor([3]), torch.tensor([3]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tok.encode_windows(torch.zeros(60, 7), torch.tensor([0]), torch.tensor([60]))


def test_signatures():
    """encode keeps its signature; the new entry points are spelled as documented."""
    names = lambda f: list(inspect.signature(f).parameters)   # noqa: E731
    assert names(BEASTBsplineTokenizer.encode) == ["self", "trajs", "update_bounds", "respect_llm_vocab_size",
                                                   "process_group"]
    assert names(BEASTBsplineTokenizer.encode_windows) == [
        "self", "frames", "starts", "ends", "update_bounds", "respect_llm_vocab_size", "process_group",
        "return_tile_counts"]
    assert names(BEASTBsplineTokenizer.encode_continuous_windows) == [
        "self", "frames", "starts", "ends", "update_bounds", "process_group"]
    assert names(BEASTBsplineTokenizer.fit_parameters_windows) == [
        "self", "frames", "starts", "ends", "chunk_windows", "process_group"]
    assert names(BEASTBsplineTokenizer.window_index) == ["self", "episode_offsets", "stride", "pad"]
    assert names(BEASTBsplineBPETokenizer.encode_windows) == [
        "self", "frames", "starts", "ends", "update_bounds", "return_mp_tokens", "return_tensors", "process_group"]
