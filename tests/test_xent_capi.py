"""Argument validation of beast_xent_rows / beast_xent_rows_bwd and of
``cross_entropy_from_logits``: it all runs before any HIP call, so no GPU is needed."""
import ctypes as C
import inspect
import math

import pytest
import torch

from beast_tokenizer_amd import BEASTBsplineBPETokenizer, BEASTBsplineTokenizer, _lib

FAKE = C.c_void_p(16)                   # never dereferenced: validation fails first


def fwd_args(**kw):
    """logits, dtype, B, K, V, sb, sk, target_tok, target_pos, tok_offset, ignore_index, smoothing, loss_out,
    stats_out, argmax_out, stream"""
    a = dict(logits=FAKE, dtype=0, B=4, K=140, V=256, sb=140 * 256, sk=256, target_tok=FAKE, target_pos=None,
             tok_offset=0, ignore_index=-100, smoothing=0.0, loss_out=FAKE, stats_out=FAKE, argmax_out=FAKE,
             stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


def bwd_args(**kw):
    """logits, dtype, B, K, V, sb, sk, target_tok, target_pos, tok_offset, ignore_index, smoothing, stats,
    grad_loss, grad_logits, gsb, gsk, stream"""
    a = dict(logits=FAKE, dtype=2, B=4, K=140, V=256, sb=140 * 256, sk=256, target_tok=None, target_pos=FAKE,
             tok_offset=0, ignore_index=-100, smoothing=0.1, stats=FAKE, grad_loss=FAKE, grad_logits=FAKE,
             gsb=140 * 256, gsk=256, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


ENTRY = {"beast_xent_rows": fwd_args, "beast_xent_rows_bwd": bwd_args}


def test_signatures_are_bound_and_the_abi_version_moved():
    assert len(_lib.SIGNATURES["beast_xent_rows"][1]) == len(fwd_args()) == 16
    assert len(_lib.SIGNATURES["beast_xent_rows_bwd"][1]) == len(bwd_args()) == 18
    assert _lib.ABI_VERSION >= 2 and _lib.load().beast_abi_version() == _lib.ABI_VERSION


@pytest.mark.parametrize("name", ENTRY)
@pytest.mark.parametrize("V", [1, 65537, 0, -3])
def test_outside_the_envelope_is_unsupported(name, V):
    lib = _lib.load()
    rc = getattr(lib, name)(*ENTRY[name](V=V))
    assert rc == _lib.BEAST_E_UNSUPPORTED
    assert name.encode() in lib.beast_last_error()
    with pytest.raises(NotImplementedError, match="2 <= V <= 65536"):
        _lib.check(rc, name)


@pytest.mark.parametrize("name", ENTRY)
@pytest.mark.parametrize("V", [2, 65536])
def test_the_envelope_ends_are_inside(name, V):
    assert getattr(_lib.load(), name)(*ENTRY[name](V=V, B=0, gsk=65536) if name.endswith("bwd")
                                      else ENTRY[name](V=V, B=0)) == _lib.BEAST_OK


@pytest.mark.parametrize("name", ENTRY)
@pytest.mark.parametrize("kw", [dict(logits=None), dict(dtype=3), dict(dtype=-1), dict(B=-1), dict(K=0),
                                dict(sb=-1), dict(sk=-1),
                                dict(target_tok=FAKE, target_pos=FAKE), dict(target_tok=None, target_pos=None),
                                dict(smoothing=1.0), dict(smoothing=-0.001), dict(smoothing=2.0),
                                dict(smoothing=math.nan), dict(smoothing=math.inf), dict(smoothing=-math.inf)])
def test_bad_arguments_are_invalid(name, kw):
    lib = _lib.load()
    assert getattr(lib, name)(*ENTRY[name](**kw)) == _lib.BEAST_E_INVALID
    assert name.encode() in lib.beast_last_error()
    # the same bad argument is refused for an empty batch too; good arguments make it a no-op
    if "B" not in kw:
        assert getattr(lib, name)(*ENTRY[name](B=0, **kw)) == _lib.BEAST_E_INVALID
    assert getattr(lib, name)(*ENTRY[name](B=0)) == _lib.BEAST_OK


@pytest.mark.parametrize("name", ENTRY)
def test_either_target_kind_and_the_largest_smoothing_are_accepted(name):
    lib = _lib.load()
    below_one = 1.0 - 2.0 ** -24                               # the largest fp32 below 1
    for kw in (dict(target_tok=FAKE, target_pos=None), dict(target_tok=None, target_pos=FAKE),
               dict(smoothing=below_one), dict(smoothing=0.0)):
        assert getattr(lib, name)(*ENTRY[name](B=0, **kw)) == _lib.BEAST_OK


def test_forward_needs_an_output():
    lib = _lib.load()
    assert lib.beast_xent_rows(*fwd_args(loss_out=None, stats_out=None, argmax_out=None)) == _lib.BEAST_E_INVALID
    assert b"beast_xent_rows: no output" in lib.beast_last_error()
    for one in ("loss_out", "stats_out", "argmax_out"):
        kw = dict(loss_out=None, stats_out=None, argmax_out=None, B=0)
        kw[one] = FAKE
        assert lib.beast_xent_rows(*fwd_args(**kw)) == _lib.BEAST_OK


@pytest.mark.parametrize("kw", [dict(stats=None), dict(grad_loss=None), dict(grad_logits=None),
                                dict(gsk=255), dict(gsb=-1)])
def test_backward_needs_its_inputs_and_disjoint_rows(kw):
    lib = _lib.load()
    assert lib.beast_xent_rows_bwd(*bwd_args(**kw)) == _lib.BEAST_E_INVALID
    assert b"beast_xent_rows_bwd" in lib.beast_last_error()
    assert lib.beast_xent_rows_bwd(*bwd_args(B=0, **kw)) == _lib.BEAST_E_INVALID


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_empty_batch_is_ok_for_every_dtype(dtype):
    lib = _lib.load()
    assert lib.beast_xent_rows(*fwd_args(B=0, dtype=dtype)) == _lib.BEAST_OK
    assert lib.beast_xent_rows_bwd(*bwd_args(B=0, dtype=dtype)) == _lib.BEAST_OK


# --------------------------------------------------------------- the Python surface --
def cpu_tok(**kw):
    return BEASTBsplineTokenizer(num_dof=7, num_basis=10, seq_len=50, device="cpu", **kw)


def good_target(kind="tokens", B=2):
    return torch.zeros((B, 70), dtype=torch.int64) if kind == "tokens" else torch.zeros((B, 70))


@pytest.mark.parametrize("shape", [(2, 70, 255), (2, 69, 256), (2, 10, 6, 256), (70, 256), (2, 70, 1000)])
def test_wrong_logits_shapes_raise_value_error(shape):
    with pytest.raises(ValueError, match="logits"):
        cpu_tok().cross_entropy_from_logits(torch.zeros(shape), good_target())


@pytest.mark.parametrize("kind", ["tokens", "coefficients"])
@pytest.mark.parametrize("shape", [(2, 69), (3, 70), (2, 7, 10), (2, 10, 7, 1), (70,), (2, 70, 256)])
def test_wrong_target_shapes_raise_value_error(kind, shape):
    target = torch.zeros(shape, dtype=torch.int64 if kind == "tokens" else torch.float32)
    with pytest.raises(ValueError, match="target must be"):
        cpu_tok().cross_entropy_from_logits(torch.zeros(2, 70, 256), target)


@pytest.mark.parametrize("target", [None, [[0] * 70] * 2, 3, torch.zeros((2, 70), dtype=torch.bool),
                                    torch.zeros((2, 70), dtype=torch.complex64)],
                         ids=["none", "list", "int", "bool", "complex"])
def test_non_tensor_and_bool_targets_raise_value_error(target):
    with pytest.raises(ValueError, match="target must be"):
        cpu_tok().cross_entropy_from_logits(torch.zeros(2, 70, 256), target)


@pytest.mark.parametrize("eps", [1.0, -0.1, 1.5, math.nan, math.inf, 1.0 - 1e-9, "much"])
def test_bad_label_smoothing_raises_value_error(eps):
    """1 - 1e-9 rounds to 1 in fp32, which is what the kernel would receive."""
    with pytest.raises(ValueError, match="label_smoothing"):
        cpu_tok().cross_entropy_from_logits(torch.zeros(2, 70, 256), good_target(), label_smoothing=eps)


def test_unknown_reduction_raises_value_error():
    with pytest.raises(ValueError, match="reduction"):
        cpu_tok().cross_entropy_from_logits(torch.zeros(2, 70, 256), good_target(), reduction="batchmean")


@pytest.mark.parametrize("kind", ["tokens", "coefficients"])
@pytest.mark.parametrize("dt", [torch.float32, torch.float16, torch.bfloat16, torch.float64])
def test_cpu_tokenizer_has_no_fallback(kind, dt):
    for grad in (False, True):
        logits = torch.zeros((2, 70, 256), dtype=dt, requires_grad=grad)
        for reduction in ("none", "sum", "mean"):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                cpu_tok().cross_entropy_from_logits(logits, good_target(kind), reduction=reduction,
                                                    label_smoothing=0.1)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            cpu_tok().cross_entropy_from_logits(logits.reshape(2, 10, 7, 256), good_target(kind).reshape(2, 10, 7))


def test_the_full_vocabulary_width_needs_llm_vocab_size():
    tok = cpu_tok()
    with pytest.raises(ValueError, match="vocab_size 256"):
        tok.cross_entropy_from_logits(torch.zeros(2, 70, 1000), good_target())
    tok.set_llm_vocab_size(1000)
    for V in (1000, 256):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            tok.cross_entropy_from_logits(torch.zeros(2, 70, V), good_target())


def test_signature_and_inheritance():
    sig = inspect.signature(BEASTBsplineTokenizer.cross_entropy_from_logits)
    assert list(sig.parameters) == ["self", "logits", "target", "label_smoothing", "ignore_index", "reduction",
                                    "return_tokens", "respect_llm_vocab_size"]
    defaults = {n: p.default for n, p in sig.parameters.items() if p.kind is inspect.Parameter.KEYWORD_ONLY}
    assert defaults == dict(label_smoothing=0.0, ignore_index=-100, reduction="mean", return_tokens=False,
                            respect_llm_vocab_size=True)
    assert BEASTBsplineBPETokenizer.cross_entropy_from_logits is BEASTBsplineTokenizer.cross_entropy_from_logits
    assert "action bins only" in BEASTBsplineTokenizer.cross_entropy_from_logits.__doc__
