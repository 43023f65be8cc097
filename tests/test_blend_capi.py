"""Argument validation of beast_reconstruct_windows_f32 and of the tokenizer's reconstruct_windows
family: it all runs before any HIP call, so no GPU is needed."""
import ctypes as C
import inspect

import pytest
import torch

from beast_tokenizer_amd import BEASTBsplineBPETokenizer, BEASTBsplineTokenizer, _lib

FAKE = C.c_void_p(16)                   # never dereferenced: validation fails first
NAME = "beast_reconstruct_windows_f32"


def blend_args(**kw):
    """The argument list of beast_reconstruct_windows_f32, in the header's order."""
    a = dict(tokens=FAKE, ntokens=None, W=4, D=14, n_joint=12, N=10, vocab=256, tok_offset=0, w_min=FAKE, w_max=FAKE,
             basis=FAKE, T=50, win_start=FAKE, win_end=FAKE, R=1000, blend=FAKE, fill=float("nan"), dof_dst=FAKE,
             num_dof_out=14, frames_out=FAKE, out_sr=14, coverage_out=FAKE, weight_out=FAKE, tile_counts=FAKE,
             stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


def test_signature_is_bound_and_the_abi_version_moved():
    assert len(_lib.SIGNATURES[NAME][1]) == len(blend_args()) == 25
    assert len(_lib.SIGNATURES["beast_blend_candidates_host"][1]) == 9
    assert _lib.ABI_VERSION >= 6 and _lib.load().beast_abi_version() == _lib.ABI_VERSION


@pytest.mark.parametrize("kw", [dict(N=17), dict(T=257), dict(D=65, n_joint=63, num_dof_out=65, out_sr=65),
                                dict(num_dof_out=4097, out_sr=4097)])
def test_outside_the_envelope_is_unsupported(kw):
    lib = _lib.load()
    rc = lib.beast_reconstruct_windows_f32(*blend_args(**kw))
    assert rc == _lib.BEAST_E_UNSUPPORTED
    with pytest.raises(NotImplementedError, match="beast_reconstruct_windows_f32 supports"):
        _lib.check(rc, NAME)


@pytest.mark.parametrize("kw", [
    dict(w_min=None), dict(w_max=None), dict(basis=None), dict(win_start=None), dict(win_end=None), dict(blend=None),
    dict(dof_dst=None), dict(frames_out=None),
    dict(tokens=None),                  # neither tokens nor ntokens
    dict(ntokens=FAKE),                 # both
    dict(W=-1), dict(R=-1), dict(T=0), dict(N=0), dict(D=0, n_joint=0), dict(n_joint=15), dict(n_joint=-1),
    dict(num_dof_out=13), dict(out_sr=13), dict(num_dof_out=16, out_sr=15), dict(vocab=1),
])
def test_bad_arguments_are_invalid(kw):
    lib = _lib.load()
    assert lib.beast_reconstruct_windows_f32(*blend_args(**kw)) == _lib.BEAST_E_INVALID
    assert NAME.encode() in lib.beast_last_error()
    with pytest.raises(ValueError):
        _lib.check(_lib.BEAST_E_INVALID, NAME)


@pytest.mark.parametrize("kw", [
    dict(R=0),
    dict(R=0, W=0),
    dict(R=0, tokens=None, ntokens=FAKE, vocab=0),                  # normalised tokens need no vocabulary
    dict(R=0, coverage_out=None, weight_out=None, tile_counts=None),   # the optional outputs
    dict(R=0, num_dof_out=16, out_sr=40),                           # unnamed columns, rows apart in memory
])
def test_no_rows_with_good_arguments_is_a_no_op(kw):
    assert _lib.load().beast_reconstruct_windows_f32(*blend_args(**kw)) == _lib.BEAST_OK


# ------------------------------------------------------------ the Python surface --
def cpu_tok(cls=BEASTBsplineTokenizer, **kw):
    return cls(num_dof=7, num_basis=10, seq_len=50, device="cpu", **kw)


TOK = torch.zeros(2, 70, dtype=torch.int64)
S, E = torch.tensor([0, 5]), torch.tensor([60, 60])


def calls(tok):
    return ((tok.reconstruct_windows, TOK), (tok.reconstruct_windows_continuous, torch.zeros(2, 70)))


def test_conditioned_tokenizers_are_not_implemented():
    for kw in (dict(init_cond_order=1), dict(end_cond_order=1), dict(init_cond_order=2, end_cond_order=-1)):
        for call, x in calls(cpu_tok(**kw)):
            with pytest.raises(NotImplementedError, match="init_cond_order"):
                call(x, S, E, 60)


@pytest.mark.parametrize("s,e", [
    (torch.zeros(2, 1, dtype=torch.int64), torch.ones(2, 1, dtype=torch.int64)),    # not 1-d
    (torch.zeros(2, dtype=torch.int64), torch.ones(3, dtype=torch.int64)),          # two lengths
    (torch.zeros(2, dtype=torch.int32), torch.ones(2, dtype=torch.int32)),          # not int64
    (torch.zeros(2), torch.ones(2)),
    (torch.tensor(0), torch.tensor(1)),
])
def test_bad_table_shapes_are_value_errors(s, e):
    for call, x in calls(cpu_tok()):
        with pytest.raises(ValueError, match="int64 .W. tables"):
            call(x, s, e, 60)


@pytest.mark.parametrize("s,e", [([0, 7], [60, 7]), ([0, 9], [60, 8]), ([-1, 0], [60, 60]), ([0, 0], [60, 61])])
def test_host_tables_are_range_checked(s, e):
    for call, x in calls(cpu_tok()):
        with pytest.raises(ValueError, match="0 <= start < end <= R=60"):
            call(x, torch.tensor(s), torch.tensor(e), 60)


def test_unsorted_host_tables_are_refused():
    for call, x in calls(cpu_tok()):
        with pytest.raises(ValueError, match="not sorted"):
            call(x, torch.tensor([5, 0]), torch.tensor([60, 60]), 60)
        with pytest.raises(RuntimeError, match="no CPU fallback"):       # equal starts are allowed
            call(x, torch.tensor([5, 5]), torch.tensor([60, 60]), 60)


def test_bad_tokens_and_frame_counts():
    tok = cpu_tok()
    for bad in (torch.zeros(2, 69, dtype=torch.int64), torch.zeros(70, dtype=torch.int64),
                torch.zeros(3, 70, dtype=torch.int64), torch.zeros(2, 10, 6, dtype=torch.int64),
                torch.zeros(2, 70), torch.zeros(2, 70, dtype=torch.bool)):
        with pytest.raises(ValueError, match="tokens|token rows"):
            tok.reconstruct_windows(bad, S, E, 60)
    with pytest.raises(ValueError, match="floating point"):
        tok.reconstruct_windows_continuous(TOK, S, E, 60)
    with pytest.raises(ValueError, match="num_frames"):
        tok.reconstruct_windows(TOK, S, E, -1)
    with pytest.raises(ValueError, match="R=59"):                        # the table against num_frames
        tok.reconstruct_windows(TOK, S, E, 59)


@pytest.mark.parametrize("blend", [
    torch.ones(49), torch.ones(50, 1), torch.ones(50, dtype=torch.int64), "triangle", "first",
    torch.full((50,), float("nan")), -torch.ones(50), torch.cat([torch.ones(49), torch.tensor([float("inf")])]),
])
def test_bad_blend_weights_are_value_errors(blend):
    for call, x in calls(cpu_tok()):
        with pytest.raises(ValueError, match="blend|horizon"):
            call(x, S, E, 60, blend=blend)


def test_host_tokenizers_are_refused():
    """After every argument check: there is no CPU fallback."""
    tok = cpu_tok()
    for call in (lambda: tok.reconstruct_windows(TOK, S, E, 60),
                 lambda: tok.reconstruct_windows(TOK.reshape(2, 10, 7), S, E, 60, blend="exp", fill=0.0),
                 lambda: tok.reconstruct_windows(TOK[:0], S[:0], E[:0], 60),
                 lambda: tok.reconstruct_windows(TOK, S, E, 60, blend=torch.zeros(50)),
                 lambda: tok.reconstruct_windows_continuous(torch.zeros(2, 70), S, E, 60)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_bpe_tokenizer_has_the_method():
    assert "reconstruct_windows" in vars(BEASTBsplineBPETokenizer)


def test_signatures():
    names = lambda f: list(inspect.signature(f).parameters)   # noqa: E731
    assert names(BEASTBsplineTokenizer.reconstruct_windows) == [
        "self", "tokens", "starts", "ends", "num_frames", "blend", "fill", "respect_llm_vocab_size",
        "return_tile_counts"]
    assert names(BEASTBsplineTokenizer.reconstruct_windows_continuous) == [
        "self", "params", "starts", "ends", "num_frames", "blend", "fill", "return_tile_counts"]
    assert names(BEASTBsplineTokenizer.blend_weights) == ["self", "kind", "m", "horizon"]
    assert names(BEASTBsplineBPETokenizer.reconstruct_windows) == [
        "self", "ids", "starts", "ends", "num_frames", "blend", "fill", "return_tile_counts"]
    sig = inspect.signature(BEASTBsplineTokenizer.reconstruct_windows)
    assert sig.parameters["blend"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["blend"].default == "uniform"
