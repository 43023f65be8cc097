"""Argument validation of beast_score_rows / beast_score_rows_bwd and of ``score_tokens_from_logits``:
it all runs before any HIP call, so no GPU is needed."""
import ctypes as C
import inspect
import math

import pytest
import torch

from beast_tokenizer_amd import BEASTBsplineBPETokenizer, BEASTBsplineTokenizer, _lib

FAKE = C.c_void_p(16)                   # never dereferenced: validation fails first
FWD, BWD = "beast_score_rows", "beast_score_rows_bwd"


def common(**kw):
    return dict(logits=FAKE, dtype=0, B=4, K=140, V=256, sb=140 * 256, sk=256, ref_logits=FAKE, rsb=140 * 256, rsk=256,
                temperature=1.0, top_k=0, top_p=1.0, tokens=FAKE, S=1, tok_offset=0, ignore_index=-100)


def fwd_args(**kw):
    """the common inputs, then logprob_out, entropy_out, kl_out, kept_out, stats_out, stream"""
    a = common()
    a.update(logprob_out=FAKE, entropy_out=FAKE, kl_out=FAKE, kept_out=FAKE, stats_out=FAKE, stream=None)
    assert set(kw) <= set(a), kw
    a.update(kw)
    return list(a.values())


def bwd_args(**kw):
    """the common inputs, then stats, grad_logprob, grad_entropy, grad_kl, grad_logits, gsb, gsk, stream"""
    a = common()
    a.update(stats=FAKE, grad_logprob=FAKE, grad_entropy=FAKE, grad_kl=FAKE, grad_logits=FAKE, gsb=140 * 256, gsk=256,
             stream=None)
    assert set(kw) <= set(a), kw
    a.update(kw)
    return list(a.values())


ENTRY = {FWD: fwd_args, BWD: bwd_args}


def test_signatures_are_bound_and_the_abi_version_moved():
    assert len(_lib.SIGNATURES[FWD][1]) == len(fwd_args()) == 23
    assert len(_lib.SIGNATURES[BWD][1]) == len(bwd_args()) == 25
    assert _lib.ABI_VERSION >= 4 and _lib.load().beast_abi_version() == _lib.ABI_VERSION


SHARED_BAD = [dict(logits=None), dict(dtype=3), dict(dtype=-1), dict(B=-1), dict(K=0), dict(sb=-1), dict(sk=-1),
              dict(rsb=-1), dict(rsk=-1),
              dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=math.inf), dict(temperature=math.nan),
              dict(top_k=-1), dict(top_p=0.0), dict(top_p=-0.5), dict(top_p=1.0 + 2.0 ** -20), dict(top_p=math.nan),
              dict(top_p=math.inf), dict(S=-1), dict(S=65), dict(tokens=None)]
FWD_BAD = [dict(logprob_out=None, entropy_out=None, kl_out=None, kept_out=None, stats_out=None),
           dict(S=0, tokens=None), dict(ref_logits=None)]                    # logprob_out / kl_out ask for them
BWD_BAD = [dict(stats=None), dict(grad_logits=None), dict(grad_logprob=None, grad_entropy=None, grad_kl=None),
           dict(S=0, tokens=None), dict(ref_logits=None), dict(gsb=-1), dict(gsk=255), dict(gsk=0)]


@pytest.mark.parametrize("name,kw", [(n, kw) for n in ENTRY for kw in SHARED_BAD]
                         + [(FWD, kw) for kw in FWD_BAD] + [(BWD, kw) for kw in BWD_BAD])
def test_bad_arguments_are_invalid_before_any_hip_call(name, kw):
    lib = _lib.load()
    fn, args = getattr(lib, name), ENTRY[name]
    assert fn(*args(**kw)) == _lib.BEAST_E_INVALID
    assert name.encode() + b":" in lib.beast_last_error()
    with pytest.raises(ValueError):
        _lib.check(_lib.BEAST_E_INVALID, name)
    # the same bad argument is refused for an empty batch too; good arguments make it a no-op
    if "B" not in kw:
        assert fn(*args(B=0, **kw)) == _lib.BEAST_E_INVALID
    assert fn(*args(B=0)) == _lib.BEAST_OK


@pytest.mark.parametrize("name", list(ENTRY))
@pytest.mark.parametrize("V", [1, 65537, 0, -3])
def test_outside_the_envelope_is_unsupported(name, V):
    lib = _lib.load()
    rc = getattr(lib, name)(*ENTRY[name](V=V, **(dict(gsk=70000) if name == BWD else {})))
    assert rc == _lib.BEAST_E_UNSUPPORTED and name.encode() in lib.beast_last_error()
    with pytest.raises(NotImplementedError, match="2 <= V <= 65536"):
        _lib.check(rc, name)


@pytest.mark.parametrize("name", list(ENTRY))
@pytest.mark.parametrize("dtype,widest", [(0, 1024), (1, 2048), (2, 2048)])
def test_truncation_ends_with_the_in_register_rows(name, dtype, widest):
    """top_k / top_p up to four chunks of the dtype; one element more is unsupported, while plain
    scoring and the truncations that truncate nothing (top_k = 0, top_k >= V, top_p = 1) go on."""
    lib = _lib.load()
    fn, args = getattr(lib, name), ENTRY[name]
    wide = dict(gsk=70000) if name == BWD else {}
    for kw in (dict(top_k=5), dict(top_p=0.9), dict(top_k=5, top_p=0.9), dict(top_k=widest)):
        assert fn(*args(B=0, dtype=dtype, V=widest, **wide, **kw)) == _lib.BEAST_OK
        rc = fn(*args(B=0, dtype=dtype, V=widest + 1, **wide, **kw))
        assert rc == _lib.BEAST_E_UNSUPPORTED and b"top_k / top_p" in lib.beast_last_error()
        with pytest.raises(NotImplementedError):
            _lib.check(rc, name)
    for kw in (dict(), dict(top_k=0), dict(top_k=widest + 1), dict(top_k=70000), dict(top_p=1.0)):
        assert fn(*args(B=0, dtype=dtype, V=widest + 1, **wide, **kw)) == _lib.BEAST_OK
    assert fn(*args(B=0, dtype=dtype, V=65536, **wide)) == _lib.BEAST_OK
    assert fn(*args(B=0, dtype=dtype, V=2, **wide)) == _lib.BEAST_OK


def test_the_range_ends_and_the_nullable_outputs():
    lib = _lib.load()
    ok = _lib.BEAST_OK
    for kw in (dict(S=1), dict(S=64), dict(top_p=2.0 ** -126), dict(top_k=2 ** 31 - 1),
               dict(S=0, tokens=None, logprob_out=None),                     # entropy / KL alone
               dict(ref_logits=None, kl_out=None), dict(ref_logits=None, kl_out=None, rsb=-1, rsk=-1),
               dict(logprob_out=None, entropy_out=None, kl_out=None, kept_out=None),        # stats alone
               dict(logprob_out=None, entropy_out=None, kl_out=None, stats_out=None),       # kept alone
               dict(entropy_out=None, kl_out=None, kept_out=None, stats_out=None, ref_logits=None)):
        assert lib.beast_score_rows(*fwd_args(B=0, **kw)) == ok, kw
    for kw in (dict(S=64), dict(S=0, tokens=None, grad_logprob=None), dict(ref_logits=None, grad_kl=None),
               dict(grad_logprob=None, grad_entropy=None), dict(grad_entropy=None, grad_kl=None, ref_logits=None),
               dict(grad_logprob=None, grad_kl=None, S=0, tokens=None, ref_logits=None), dict(gsk=300), dict(gsb=0)):
        assert lib.beast_score_rows_bwd(*bwd_args(B=0, **kw)) == ok, kw
    # S = 0 with logprob_out, or a KL without a reference, is refused in both directions
    assert lib.beast_score_rows(*fwd_args(S=0)) == _lib.BEAST_E_INVALID
    assert lib.beast_score_rows(*fwd_args(ref_logits=None)) == _lib.BEAST_E_INVALID
    assert b"kl_out needs ref_logits" in lib.beast_last_error()
    assert lib.beast_score_rows_bwd(*bwd_args(S=0)) == _lib.BEAST_E_INVALID
    assert lib.beast_score_rows_bwd(*bwd_args(ref_logits=None)) == _lib.BEAST_E_INVALID


# --------------------------------------------------------------- the Python surface --
def cpu_tok(**kw):
    return BEASTBsplineTokenizer(num_dof=7, num_basis=10, seq_len=50, device="cpu", **kw)


LOGITS = torch.zeros(2, 70, 256)
TOKENS = torch.zeros((2, 70), dtype=torch.int64)


@pytest.mark.parametrize("shape", [(2, 70, 255), (2, 69, 256), (2, 10, 6, 256), (70, 256), (2, 70, 1000)])
def test_wrong_logits_shapes_raise_value_error(shape):
    with pytest.raises(ValueError, match="logits"):
        cpu_tok().score_tokens_from_logits(torch.zeros(shape), TOKENS)


@pytest.mark.parametrize("kw,match", [
    (dict(temperature=0.0), "temperature"), (dict(temperature=-1.0), "temperature"),
    (dict(temperature=math.inf), "temperature"), (dict(temperature=math.nan), "temperature"),
    (dict(top_k=-1), "top_k"), (dict(top_k=2.5), "top_k"), (dict(top_k=True), "top_k"), (dict(top_k="5"), "top_k"),
    (dict(top_k=2 ** 31), "top_k"),
    (dict(top_p=0.0), "top_p"), (dict(top_p=-0.1), "top_p"), (dict(top_p=1.5), "top_p"), (dict(top_p=math.nan), "top_p"),
    (dict(top_p=1e-60), "top_p"), (dict(top_p="most"), "top_p"),
    (dict(tokens=None), "tokens may be None only"),
    (dict(tokens=[[0] * 70] * 2), "tokens"), (dict(tokens=torch.zeros(2, 70)), "tokens"),
    (dict(tokens=torch.zeros((2, 70), dtype=torch.bool)), "tokens"),
    (dict(tokens=torch.zeros((2, 69), dtype=torch.int64)), "tokens"),
    (dict(tokens=torch.zeros((3, 70), dtype=torch.int64)), "tokens"),
    (dict(tokens=torch.zeros((65, 2, 70), dtype=torch.int64)), "tokens"),
    (dict(tokens=torch.zeros((0, 2, 70), dtype=torch.int64)), "tokens"),
    (dict(tokens=torch.zeros((2, 7, 10), dtype=torch.int64)), "tokens"),
    (dict(ref_logits=torch.zeros(2, 70, 256, dtype=torch.bfloat16)), "ref_logits must have the logits' dtype"),
    (dict(ref_logits=torch.zeros(2, 70, 256, dtype=torch.float64)), "ref_logits must have the logits' dtype"),
    (dict(ref_logits=torch.zeros(2, 10, 7, 256)), "ref_logits must have the logits' shape"),
    (dict(ref_logits=torch.zeros(1, 70, 256)), "ref_logits must have the logits' shape"),
    (dict(ref_logits=[0.0]), "ref_logits"),
])
def test_bad_arguments_raise_value_error_before_the_device_is_asked_for(kw, match):
    """On a CPU tokenizer a good call ends in "no CPU fallback": a ValueError shows that the check
    came first."""
    kw = dict(kw)
    tokens = kw.pop("tokens", TOKENS)
    with pytest.raises(ValueError, match=match):
        cpu_tok().score_tokens_from_logits(LOGITS, tokens, **kw)


@pytest.mark.parametrize("tokens,kw", [
    (TOKENS, dict()), (TOKENS.reshape(2, 10, 7).to(torch.int32), dict(temperature=0.5, top_k=5, top_p=0.9)),
    (torch.zeros((64, 2, 70), dtype=torch.int64), dict(return_entropy=True)),
    (torch.zeros((1, 2, 10, 7), dtype=torch.int64), dict(ref_logits="same")),
    (None, dict(return_entropy=True)), (None, dict(ref_logits="same", top_k=0, top_p=1.0)),
])
def test_cpu_tokenizer_has_no_fallback(tokens, kw):
    for l in (LOGITS, LOGITS.reshape(2, 10, 7, 256), LOGITS.to(torch.bfloat16), LOGITS.double(),
              LOGITS.clone().requires_grad_()):
        kw2 = {k: (torch.zeros_like(l) if isinstance(v, str) else v) for k, v in kw.items()}
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            cpu_tok().score_tokens_from_logits(l, tokens, **kw2)


@pytest.mark.parametrize("dt,vocab", [(torch.float32, 1025), (torch.float64, 1025), (torch.bfloat16, 2049),
                                      (torch.float16, 2049)])
def test_truncation_beyond_the_envelope_is_not_implemented(dt, vocab):
    tok = cpu_tok(vocab_size=vocab)
    l = torch.zeros((1, 70, vocab), dtype=dt)
    t = torch.zeros((1, 70), dtype=torch.int64)
    for kw in (dict(top_k=5), dict(top_p=0.5)):
        with pytest.raises(NotImplementedError, match="top_k / top_p"):
            tok.score_tokens_from_logits(l, t, **kw)
    for kw in (dict(), dict(top_k=vocab), dict(top_p=1.0)):          # nothing is truncated
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            tok.score_tokens_from_logits(l, t, **kw)
    inside = cpu_tok(vocab_size=vocab - 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        inside.score_tokens_from_logits(torch.zeros((1, 70, vocab - 1), dtype=dt), t, top_k=5, top_p=0.5)


def test_signature_and_inheritance():
    sig = inspect.signature(BEASTBsplineTokenizer.score_tokens_from_logits)
    assert list(sig.parameters) == ["self", "logits", "tokens", "temperature", "top_k", "top_p", "ref_logits",
                                    "return_entropy", "ignore_index", "respect_llm_vocab_size"]
    assert sig.parameters["tokens"].default is None
    assert sig.parameters["tokens"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    defaults = {n: p.default for n, p in sig.parameters.items() if p.kind is inspect.Parameter.KEYWORD_ONLY}
    assert defaults == dict(temperature=1.0, top_k=None, top_p=None, ref_logits=None, return_entropy=False,
                            ignore_index=-100, respect_llm_vocab_size=True)
    assert BEASTBsplineBPETokenizer.score_tokens_from_logits is BEASTBsplineTokenizer.score_tokens_from_logits
