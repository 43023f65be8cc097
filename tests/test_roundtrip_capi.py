"""``beast_roundtrip_stats_f32`` validates its arguments before any HIP call, and the tokenizer's
``reconstruction_stats`` refuses a CPU device as every other entry point does: no GPU is needed."""
import ctypes as C

import pytest
import torch

from beast_tokenizer_amd import BEASTBsplineBPETokenizer, BEASTBsplineTokenizer, ReconstructionStats, _lib

FAKE = C.c_void_p(16)                   # never dereferenced: validation fails first


def rt_args(**kw):
    """traj, B, T, sb, st, sd, row_elems, D, n_joint, dof_src, proj, basis, N, w_min, w_max, vocab,
    tok_offset, tokens_out, stats_out, clip_counts, stream"""
    a = dict(traj=FAKE, B=4, T=50, sb=700, st=14, sd=1, row_elems=14, D=14, n_joint=14, dof_src=FAKE, proj=FAKE,
             basis=FAKE, N=10, w_min=FAKE, w_max=FAKE, vocab=256, tok_offset=0, tokens_out=FAKE, stats_out=FAKE,
             clip_counts=FAKE, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


@pytest.mark.parametrize("kw", [
    dict(traj=None), dict(proj=None), dict(basis=None), dict(stats_out=None), dict(dof_src=None), dict(w_min=None),
    dict(w_max=None), dict(N=17), dict(N=0), dict(T=257), dict(T=0), dict(D=65, n_joint=65), dict(D=0, n_joint=0),
    dict(n_joint=15), dict(vocab=1), dict(B=-1), dict(row_elems=0),
])
def test_bad_arguments_are_invalid(kw):
    lib = _lib.load()
    rc = lib.beast_roundtrip_stats_f32(*rt_args(**kw))
    assert rc == _lib.BEAST_E_INVALID
    assert lib.beast_last_error()
    with pytest.raises(ValueError):
        _lib.check(rc, "beast_roundtrip_stats_f32")


def test_null_pointer_message_names_the_entry_point():
    lib = _lib.load()
    assert lib.beast_roundtrip_stats_f32(*rt_args(traj=None)) == _lib.BEAST_E_INVALID
    assert b"beast_roundtrip_stats_f32" in lib.beast_last_error()


def test_empty_batch_is_a_no_op():
    lib = _lib.load()
    assert lib.beast_roundtrip_stats_f32(*rt_args(B=0)) == _lib.BEAST_OK
    # the optional outputs may be null
    assert lib.beast_roundtrip_stats_f32(*rt_args(B=0, tokens_out=None, clip_counts=None)) == _lib.BEAST_OK


def test_cpu_tensors_are_refused():
    tok = BEASTBsplineTokenizer(num_dof=7, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tok.reconstruction_stats(torch.zeros(2, 50, 7))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tok.evaluate_reconstruction([torch.zeros(2, 50, 7)])


def test_surface():
    for name in ("reconstruction_stats", "evaluate_reconstruction"):
        assert name in vars(BEASTBsplineTokenizer) and name not in vars(BEASTBsplineBPETokenizer)   # inherited
        assert getattr(BEASTBsplineBPETokenizer, name) is getattr(BEASTBsplineTokenizer, name)
    assert ReconstructionStats._fields == ("mse", "mean_err", "max_abs", "mse_fit", "clip_low", "clip_high", "tokens")
    s = ReconstructionStats(torch.tensor([[1.0, 3.0]]), torch.tensor([[-1.0, 2.0]]), None, None, None, None, None)
    assert float(s.l2) == 2.0 and float(s.l1) == 0.5
