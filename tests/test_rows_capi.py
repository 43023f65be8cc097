"""Argument validation of beast_encode_rows_f32 and of the tokenizer's encode_at: it all runs
before any HIP call, so no GPU is needed."""
import ctypes as C

import pytest
import torch

from beast_tokenizer_amd import BEASTBsplineBPETokenizer, BEASTBsplineTokenizer, _lib

FAKE = C.c_void_p(16)                   # never dereferenced: validation fails first


def rows_args(**kw):
    """The argument list of beast_encode_rows_f32, in the header's order."""
    a = dict(traj=FAKE, B=4, T=50, sb=700, st=14, sd=1, D=14, n_joint=12, dof_src=FAKE, times=FAKE, times_sb=50,
             weights=FAKE, weights_sb=50, tau=2.0, delay=0.0, knots_joint=FAKE, n_knots_joint=15, knots_grip=FAKE,
             n_knots_grip=11, degree=4, N=10, reg=1e-9, w_min=FAKE, w_max=FAKE, vocab=256, tok_offset=0,
             params_out=FAKE, tokens_out=FAKE, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


def test_signature_is_bound():
    assert len(_lib.SIGNATURES["beast_encode_rows_f32"][1]) == len(rows_args()) == 29


@pytest.mark.parametrize("kw", [
    dict(N=17, n_knots_joint=22, n_knots_grip=18), dict(T=257), dict(D=65, n_joint=63),
    dict(degree=9, n_knots_joint=20),
])
def test_outside_the_envelope_is_unsupported(kw):
    lib = _lib.load()
    rc = lib.beast_encode_rows_f32(*rows_args(**kw))
    assert rc == _lib.BEAST_E_UNSUPPORTED
    with pytest.raises(NotImplementedError, match="beast_encode_rows_f32 supports"):
        _lib.check(rc, "beast_encode_rows_f32")


@pytest.mark.parametrize("kw", [
    dict(traj=None), dict(dof_src=None), dict(times=None), dict(params_out=None, tokens_out=None),
    dict(knots_joint=None), dict(knots_grip=None), dict(w_min=None), dict(w_max=None), dict(vocab=1),
    dict(B=-1), dict(T=0), dict(N=0, n_knots_joint=5, n_knots_grip=1), dict(D=0, n_joint=0), dict(n_joint=15),
    dict(n_joint=-1), dict(degree=-1, n_knots_joint=10),
    dict(sb=-1), dict(st=-1), dict(sd=-1), dict(times_sb=-1), dict(weights_sb=-1),
    dict(n_knots_joint=14), dict(n_knots_joint=16), dict(n_knots_grip=15), dict(n_knots_grip=10),
])
def test_bad_arguments_are_invalid(kw):
    lib = _lib.load()
    assert lib.beast_encode_rows_f32(*rows_args(**kw)) == _lib.BEAST_E_INVALID
    assert b"beast_encode_rows_f32" in lib.beast_last_error()
    with pytest.raises(ValueError):
        _lib.check(_lib.BEAST_E_INVALID, "beast_encode_rows_f32")


@pytest.mark.parametrize("kw", [
    dict(B=0),
    dict(B=0, weights=None),                                    # weights are optional
    dict(B=0, tokens_out=None, w_min=None, w_max=None, vocab=0),   # params only: no quantiser arguments
    dict(B=0, params_out=None),                                 # tokens only
    dict(B=0, n_joint=14, knots_grip=None, n_knots_grip=0),     # no gripper DoFs: no gripper knots
    dict(B=0, n_joint=0, knots_joint=None, n_knots_joint=0),    # only gripper DoFs
    dict(B=0, times_sb=0, weights_sb=0),                        # one shared row of times / weights
])
def test_an_empty_batch_with_good_arguments_is_a_no_op(kw):
    assert _lib.load().beast_encode_rows_f32(*rows_args(**kw)) == _lib.BEAST_OK


# ------------------------------------------------------------ the Python surface --
def cpu_tok(cls=BEASTBsplineTokenizer, **kw):
    return cls(num_dof=7, num_basis=10, seq_len=50, device="cpu", **kw)


def test_conditioned_tokenizers_are_not_implemented():
    x, t = torch.zeros(2, 50, 7), torch.zeros(2, 50)
    for kw in (dict(init_cond_order=1), dict(end_cond_order=1), dict(init_cond_order=2, end_cond_order=-1)):
        tok = cpu_tok(**kw)
        for call in (tok.encode_at, tok.encode_continuous_at):
            with pytest.raises(NotImplementedError, match="init_cond_order"):
                call(x, t)


@pytest.mark.parametrize("xs,ts", [((2, 50, 7), (2, 49)), ((2, 50, 7), (3, 50)), ((2, 50, 7), (49,)),
                                   ((50, 7), (50,)), ((2, 50, 7), (2, 50, 1)), ((2, 50, 7), ())])
def test_shape_mismatch_of_times_is_an_assertion_error(xs, ts):
    tok = cpu_tok()
    with pytest.raises(AssertionError, match="does not match times"):
        tok.encode_at(torch.zeros(xs), torch.zeros(ts))


@pytest.mark.parametrize("ws", [(2, 49), (3, 50), (49,), (2, 50, 1), ()])
def test_shape_mismatch_of_weights_is_a_value_error(ws):
    tok = cpu_tok()
    with pytest.raises(ValueError, match="weights must be"):
        tok.encode_at(torch.zeros(2, 50, 7), torch.zeros(2, 50), torch.zeros(ws))
    with pytest.raises(ValueError, match="weights must be"):
        tok.encode_continuous_at(torch.zeros(2, 50, 7), torch.zeros(50), torch.zeros(ws))


def test_too_few_dof_columns_and_empty_grids():
    tok = cpu_tok()
    with pytest.raises(IndexError, match="out of bounds for dimension 2"):
        tok.encode_at(torch.zeros(2, 50, 6), torch.zeros(2, 50))
    with pytest.raises(ValueError, match="at least one point"):
        tok.encode_at(torch.zeros(2, 0, 7), torch.zeros(2, 0))


def test_host_tensors_are_refused():
    """As the other entry points refuse them: there is no CPU fallback.  T need not be seq_len."""
    tok = cpu_tok()
    x, t, w = torch.zeros(2, 31, 7), torch.zeros(2, 31), torch.ones(31)
    for call in (lambda: tok.encode_at(x, t), lambda: tok.encode_at(x, t[0], w, update_bounds=True),
                 lambda: tok.encode_continuous_at(x, t, w)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_bpe_tokenizer_has_the_method():
    assert "encode_at" in vars(BEASTBsplineBPETokenizer)
    tok = cpu_tok(BEASTBsplineBPETokenizer)
    with pytest.raises(AssertionError, match="does not match times"):
        tok.encode_at(torch.zeros(2, 50, 7), torch.zeros(2, 49))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tok.encode_at(torch.zeros(2, 50, 7), torch.zeros(2, 50))


def test_encode_itself_is_unchanged():
    """encode keeps its signature: the new arguments live on encode_at."""
    import inspect
    assert list(inspect.signature(BEASTBsplineTokenizer.encode).parameters) == [
        "self", "trajs", "update_bounds", "respect_llm_vocab_size", "process_group"]
    assert list(inspect.signature(BEASTBsplineTokenizer.encode_at).parameters) == [
        "self", "trajs", "times", "weights", "update_bounds", "respect_llm_vocab_size", "process_group"]
