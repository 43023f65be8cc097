"""Argument validation of beast_sample_rows and of ``sample_tokens_from_logits``: it all runs before
any HIP call, so no GPU is needed."""
import ctypes as C
import inspect
import math

import pytest
import torch

from beast_tokenizer_amd import BEASTBsplineBPETokenizer, BEASTBsplineTokenizer, _lib

FAKE = C.c_void_p(16)                   # never dereferenced: validation fails first
NAME = "beast_sample_rows"


def args(**kw):
    """logits, dtype, B, K, V, sb, sk, temperature, top_k, top_p, uniforms, S, tok_offset, tokens_out,
    logprob_out, kept_out, stream"""
    a = dict(logits=FAKE, dtype=0, B=4, K=140, V=256, sb=140 * 256, sk=256, temperature=1.0, top_k=0, top_p=1.0,
             uniforms=FAKE, S=1, tok_offset=0, tokens_out=FAKE, logprob_out=FAKE, kept_out=FAKE, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


def test_signature_is_bound_and_the_abi_version_moved():
    assert len(_lib.SIGNATURES[NAME][1]) == len(args()) == 17
    assert _lib.ABI_VERSION >= 3 and _lib.load().beast_abi_version() == _lib.ABI_VERSION


@pytest.mark.parametrize("kw", [dict(logits=None), dict(dtype=3), dict(dtype=-1), dict(B=-1), dict(K=0),
                                dict(sb=-1), dict(sk=-1),
                                dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=math.inf),
                                dict(temperature=math.nan),
                                dict(top_k=-1), dict(top_p=0.0), dict(top_p=-0.5), dict(top_p=1.0 + 2.0 ** -20),
                                dict(top_p=math.nan), dict(top_p=math.inf),
                                dict(S=0), dict(S=-1), dict(S=65),
                                dict(uniforms=None), dict(tokens_out=None)])
def test_bad_arguments_are_invalid_before_any_hip_call(kw):
    lib = _lib.load()
    assert lib.beast_sample_rows(*args(**kw)) == _lib.BEAST_E_INVALID
    assert NAME.encode() in lib.beast_last_error()
    with pytest.raises(ValueError):
        _lib.check(_lib.BEAST_E_INVALID, NAME)
    # the same bad argument is refused for an empty batch too; good arguments make it a no-op
    if "B" not in kw:
        assert lib.beast_sample_rows(*args(B=0, **kw)) == _lib.BEAST_E_INVALID
    assert lib.beast_sample_rows(*args(B=0)) == _lib.BEAST_OK


@pytest.mark.parametrize("V", [1, 65537, 0, -3])
def test_outside_the_envelope_is_unsupported(V):
    lib = _lib.load()
    rc = lib.beast_sample_rows(*args(V=V))
    assert rc == _lib.BEAST_E_UNSUPPORTED and NAME.encode() in lib.beast_last_error()
    with pytest.raises(NotImplementedError, match="2 <= V <= 65536"):
        _lib.check(rc, NAME)


@pytest.mark.parametrize("dtype,widest", [(0, 1024), (1, 2048), (2, 2048)])
def test_truncation_ends_with_the_in_register_rows(dtype, widest):
    """top_k / top_p up to four chunks of the dtype; one element more is unsupported, while plain
    sampling and the truncations that truncate nothing (top_k = 0, top_k >= V, top_p = 1) go on."""
    lib = _lib.load()
    for kw in (dict(top_k=5), dict(top_p=0.9), dict(top_k=5, top_p=0.9), dict(top_k=widest)):
        assert lib.beast_sample_rows(*args(B=0, dtype=dtype, V=widest, **kw)) == _lib.BEAST_OK
        rc = lib.beast_sample_rows(*args(B=0, dtype=dtype, V=widest + 1, **kw))
        assert rc == _lib.BEAST_E_UNSUPPORTED and b"top_k / top_p" in lib.beast_last_error()
        with pytest.raises(NotImplementedError):
            _lib.check(rc, NAME)
    for kw in (dict(), dict(top_k=0), dict(top_k=widest + 1), dict(top_k=70000), dict(top_p=1.0)):
        assert lib.beast_sample_rows(*args(B=0, dtype=dtype, V=widest + 1, **kw)) == _lib.BEAST_OK
    assert lib.beast_sample_rows(*args(B=0, dtype=dtype, V=65536)) == _lib.BEAST_OK


def test_the_range_ends_and_the_optional_outputs_are_accepted():
    lib = _lib.load()
    for kw in (dict(S=1), dict(S=64), dict(top_p=2.0 ** -126), dict(top_p=1.0), dict(top_k=2 ** 31 - 1),
               dict(logprob_out=None), dict(kept_out=None), dict(logprob_out=None, kept_out=None), dict(V=2)):
        assert lib.beast_sample_rows(*args(B=0, **kw)) == _lib.BEAST_OK


# --------------------------------------------------------------- the Python surface --
def cpu_tok(**kw):
    return BEASTBsplineTokenizer(num_dof=7, num_basis=10, seq_len=50, device="cpu", **kw)


LOGITS = torch.zeros(2, 70, 256)


@pytest.mark.parametrize("shape", [(2, 70, 255), (2, 69, 256), (2, 10, 6, 256), (70, 256), (2, 70, 1000)])
def test_wrong_logits_shapes_raise_value_error(shape):
    with pytest.raises(ValueError, match="logits"):
        cpu_tok().sample_tokens_from_logits(torch.zeros(shape))


@pytest.mark.parametrize("kw,match", [
    (dict(temperature=0.0), "temperature"), (dict(temperature=-1.0), "temperature"),
    (dict(temperature=math.inf), "temperature"), (dict(temperature=math.nan), "temperature"),
    (dict(top_k=-1), "top_k"), (dict(top_k=2.5), "top_k"), (dict(top_k=True), "top_k"), (dict(top_k="5"), "top_k"),
    (dict(top_k=2 ** 31), "top_k"),
    (dict(top_p=0.0), "top_p"), (dict(top_p=-0.1), "top_p"), (dict(top_p=1.5), "top_p"), (dict(top_p=math.nan), "top_p"),
    (dict(top_p=1e-60), "top_p"), (dict(top_p="most"), "top_p"),
    (dict(num_samples=0), "num_samples"), (dict(num_samples=65), "num_samples"), (dict(num_samples=2.0), "num_samples"),
    (dict(num_samples=True), "num_samples"),
    (dict(uniforms=[[0.5] * 70] * 2), "uniforms"), (dict(uniforms=torch.zeros((2, 70), dtype=torch.int64)), "uniforms"),
    (dict(uniforms=torch.zeros(2, 69)), "uniforms"), (dict(uniforms=torch.zeros(3, 2, 70)), "uniforms"),
    (dict(uniforms=torch.zeros(2, 70), num_samples=1), "uniforms"),
    (dict(uniforms=torch.zeros(1, 2, 70), num_samples=2), "uniforms"),
    (dict(uniforms=torch.zeros(2, 70), generator=torch.Generator()), "either generator or uniforms"),
])
def test_bad_arguments_raise_value_error_before_the_device_is_asked_for(kw, match):
    """1e-60 rounds to 0 in fp32, which is what the kernel would receive.  On a CPU tokenizer a good
    call ends in "no CPU fallback": a ValueError shows that the check came first."""
    with pytest.raises(ValueError, match=match):
        cpu_tok().sample_tokens_from_logits(LOGITS, **kw)


@pytest.mark.parametrize("kw", [dict(), dict(temperature=0.5, top_k=5, top_p=0.9, num_samples=4, return_log_probs=True),
                                dict(top_k=0, top_p=1.0), dict(uniforms=torch.zeros(2, 70)),
                                dict(uniforms=torch.zeros(2, 10, 7, dtype=torch.float64)),
                                dict(uniforms=torch.zeros(3, 2, 70, dtype=torch.bfloat16), num_samples=3),
                                dict(generator=torch.Generator(), num_samples=64)])
def test_cpu_tokenizer_has_no_fallback(kw):
    for l in (LOGITS, LOGITS.reshape(2, 10, 7, 256), LOGITS.to(torch.bfloat16), LOGITS.double()):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            cpu_tok().sample_tokens_from_logits(l, **kw)


@pytest.mark.parametrize("dt,vocab", [(torch.float32, 1025), (torch.float64, 1025), (torch.bfloat16, 2049),
                                      (torch.float16, 2049)])
def test_truncation_beyond_the_envelope_is_not_implemented(dt, vocab):
    tok = cpu_tok(vocab_size=vocab)
    l = torch.zeros((1, 70, vocab), dtype=dt)
    for kw in (dict(top_k=5), dict(top_p=0.5)):
        with pytest.raises(NotImplementedError, match="top_k / top_p"):
            tok.sample_tokens_from_logits(l, **kw)
    for kw in (dict(), dict(top_k=vocab), dict(top_p=1.0)):          # nothing is truncated
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            tok.sample_tokens_from_logits(l, **kw)
    inside = cpu_tok(vocab_size=vocab - 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        inside.sample_tokens_from_logits(torch.zeros((1, 70, vocab - 1), dtype=dt), top_k=5, top_p=0.5)


def test_signature_and_inheritance():
    sig = inspect.signature(BEASTBsplineTokenizer.sample_tokens_from_logits)
    assert list(sig.parameters) == ["self", "logits", "temperature", "top_k", "top_p", "num_samples", "generator",
                                    "uniforms", "return_log_probs", "respect_llm_vocab_size"]
    defaults = {n: p.default for n, p in sig.parameters.items() if p.kind is inspect.Parameter.KEYWORD_ONLY}
    assert defaults == dict(temperature=1.0, top_k=None, top_p=None, num_samples=None, generator=None, uniforms=None,
                            return_log_probs=False, respect_llm_vocab_size=True)
    assert BEASTBsplineBPETokenizer.sample_tokens_from_logits is BEASTBsplineTokenizer.sample_tokens_from_logits
