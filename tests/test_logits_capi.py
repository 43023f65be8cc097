"""Argument validation of beast_logits_expect / beast_logits_expect_bwd and of the tokenizer's
logits methods: it all runs before any HIP call, so no GPU is needed."""
import ctypes as C
import math

import pytest
import torch

from beast_tokenizer_amd import BEASTBsplineBPETokenizer, BEASTBsplineTokenizer, _lib

FAKE = C.c_void_p(16)                   # never dereferenced: validation fails first


def fwd_args(**kw):
    """logits, dtype, B, K, V, sb, sk, temperature, tok_offset, mean_out, argmax_out, stats_out, stream"""
    a = dict(logits=FAKE, dtype=0, B=4, K=140, V=256, sb=140 * 256, sk=256, temperature=1.0, tok_offset=0,
             mean_out=FAKE, argmax_out=FAKE, stats_out=FAKE, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


def bwd_args(**kw):
    """logits, dtype, B, K, V, sb, sk, temperature, mean, stats, grad_mean, grad_logits, gsb, gsk, stream"""
    a = dict(logits=FAKE, dtype=2, B=4, K=140, V=256, sb=140 * 256, sk=256, temperature=1.0, mean=FAKE, stats=FAKE,
             grad_mean=FAKE, grad_logits=FAKE, gsb=140 * 256, gsk=256, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


ENTRY = {"beast_logits_expect": fwd_args, "beast_logits_expect_bwd": bwd_args}


def test_signatures_are_bound():
    assert len(_lib.SIGNATURES["beast_logits_expect"][1]) == len(fwd_args())
    assert len(_lib.SIGNATURES["beast_logits_expect_bwd"][1]) == len(bwd_args())
    assert _lib.LOGITS_DTYPES == {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


@pytest.mark.parametrize("name", ENTRY)
@pytest.mark.parametrize("V", [1, 65537, 0, -3])
def test_outside_the_envelope_is_unsupported(name, V):
    rc = getattr(_lib.load(), name)(*ENTRY[name](V=V))
    assert rc == _lib.BEAST_E_UNSUPPORTED
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
                                dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=math.nan),
                                dict(temperature=math.inf)])
def test_bad_arguments_are_invalid(name, kw):
    lib = _lib.load()
    assert getattr(lib, name)(*ENTRY[name](**kw)) == _lib.BEAST_E_INVALID
    assert name.encode() in lib.beast_last_error()
    # the same bad argument is refused for an empty batch too; good arguments make it a no-op
    if "B" not in kw:
        assert getattr(lib, name)(*ENTRY[name](B=0, **kw)) == _lib.BEAST_E_INVALID
    assert getattr(lib, name)(*ENTRY[name](B=0)) == _lib.BEAST_OK


def test_forward_needs_an_output():
    lib = _lib.load()
    assert lib.beast_logits_expect(*fwd_args(mean_out=None, argmax_out=None, stats_out=None)) == _lib.BEAST_E_INVALID
    assert b"no output" in lib.beast_last_error()
    for one in ("mean_out", "argmax_out", "stats_out"):
        kw = dict(mean_out=None, argmax_out=None, stats_out=None, B=0)
        kw[one] = FAKE
        assert lib.beast_logits_expect(*fwd_args(**kw)) == _lib.BEAST_OK


@pytest.mark.parametrize("kw", [dict(mean=None), dict(stats=None), dict(grad_mean=None), dict(grad_logits=None),
                                dict(gsk=255), dict(gsb=-1)])
def test_backward_needs_its_inputs_and_disjoint_rows(kw):
    lib = _lib.load()
    assert lib.beast_logits_expect_bwd(*bwd_args(**kw)) == _lib.BEAST_E_INVALID
    assert lib.beast_last_error()


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_empty_batch_is_ok_for_every_dtype(dtype):
    lib = _lib.load()
    assert lib.beast_logits_expect(*fwd_args(B=0, dtype=dtype)) == _lib.BEAST_OK
    assert lib.beast_logits_expect_bwd(*bwd_args(B=0, dtype=dtype)) == _lib.BEAST_OK


def test_resident_rows_validates_before_any_hip_call():
    lib = _lib.load()
    assert lib.beast_logits_resident_rows(7, 256, 0, None) == _lib.BEAST_E_INVALID
    assert lib.beast_logits_resident_rows(0, 1, 0, None) == _lib.BEAST_E_UNSUPPORTED
    assert lib.beast_logits_resident_rows(2, 65537, 1, None) == _lib.BEAST_E_UNSUPPORTED


# --------------------------------------------------------------- the Python surface --
def cpu_tok(**kw):
    return BEASTBsplineTokenizer(num_dof=7, num_basis=10, seq_len=50, device="cpu", **kw)


METHODS = ("expected_params_from_logits", "reconstruct_traj_from_logits", "greedy_tokens_from_logits")


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape", [(2, 70, 255), (2, 69, 256), (2, 10, 6, 256), (2, 7, 10, 256), (70, 256),
                                   (2, 1, 70, 256, 1), (2, 70, 1000)])
def test_wrong_shapes_raise_value_error_before_the_device_is_asked_for(method, shape):
    with pytest.raises(ValueError, match="logits"):
        getattr(cpu_tok(), method)(torch.zeros(shape))


@pytest.mark.parametrize("method", METHODS)
def test_the_full_vocabulary_width_needs_llm_vocab_size(method):
    tok = cpu_tok()
    with pytest.raises(ValueError, match="vocab_size 256"):
        getattr(tok, method)(torch.zeros(2, 70, 1000))
    tok.set_llm_vocab_size(1000)
    for V in (1000, 256):                # both widths are accepted now: the call reaches the device question
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            getattr(tok, method)(torch.zeros(2, 70, V))
    with pytest.raises(ValueError, match="llm_vocab_size 1000"):
        getattr(tok, method)(torch.zeros(2, 70, 999))


@pytest.mark.parametrize("method", METHODS)
def test_other_dtypes_raise_value_error(method):
    for dt in (torch.int64, torch.bool):
        with pytest.raises(ValueError, match="floating-point"):
            getattr(cpu_tok(), method)(torch.zeros((2, 70, 256), dtype=dt))
    with pytest.raises(ValueError, match="logits"):
        getattr(cpu_tok(), method)([[0.0] * 256] * 70)


@pytest.mark.parametrize("method", METHODS[:2])
@pytest.mark.parametrize("tau", [0.0, -1.0, math.nan, math.inf])
def test_bad_temperature_raises_value_error(method, tau):
    with pytest.raises(ValueError, match="temperature"):
        getattr(cpu_tok(), method)(torch.zeros(2, 70, 256), temperature=tau)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("dt", [torch.float32, torch.float16, torch.bfloat16, torch.float64])
def test_cpu_tokenizer_has_no_fallback(method, dt):
    for grad in (False, True):
        logits = torch.zeros((2, 70, 256), dtype=dt, requires_grad=grad)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            getattr(cpu_tok(), method)(logits)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            getattr(cpu_tok(), method)(logits.reshape(2, 10, 7, 256))


def test_reconstruct_traj_from_logits_signature():
    import inspect
    sig = inspect.signature(BEASTBsplineTokenizer.reconstruct_traj_from_logits)
    assert [p for p in sig.parameters] == ["self", "logits", "times", "temperature", "orders", "init_p"]
    assert sig.parameters["temperature"].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters["orders"].default is None and sig.parameters["temperature"].default == 1.0


def test_bpe_tokenizer_inherits_the_logits_methods():
    for name in METHODS:
        assert getattr(BEASTBsplineBPETokenizer, name) is getattr(BEASTBsplineTokenizer, name)
