"""Argument validation of beast_reconstruct_derivs_bwd_f32 and of the differentiable tokenizer
methods: it all runs before any HIP call, so no GPU is needed."""
import ctypes as C

import pytest
import torch

from beast_tokenizer_amd import BEASTBsplineBPETokenizer, BEASTBsplineTokenizer, _lib

FAKE = C.c_void_p(16)                   # never dereferenced: validation fails first


def bwd_args(**kw):
    """grad_pos, grad_vel, grad_acc, B, D, n_joint, N, w_min, w_max, basis, basis_sb, T_out, dof_dst,
    num_dof_out, ntokens, init_p_src, grad_ntokens, grad_init_p, grad_init_p_sb, stream"""
    a = dict(grad_pos=FAKE, grad_vel=FAKE, grad_acc=FAKE, B=4, D=14, n_joint=14, N=10, w_min=FAKE, w_max=FAKE,
             basis=FAKE, basis_sb=0, T_out=50, dof_dst=FAKE, num_dof_out=14, ntokens=FAKE, init_p_src=None,
             grad_ntokens=FAKE, grad_init_p=None, grad_init_p_sb=0, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


@pytest.mark.parametrize("kw", [dict(N=17), dict(D=65, num_dof_out=65), dict(T_out=4097), dict(num_dof_out=4097)])
def test_outside_the_envelope_is_unsupported(kw):
    lib = _lib.load()
    rc = lib.beast_reconstruct_derivs_bwd_f32(*bwd_args(**kw))
    assert rc == _lib.BEAST_E_UNSUPPORTED
    with pytest.raises(NotImplementedError, match="reconstruct derivs backward supports"):
        _lib.check(rc, "beast_reconstruct_derivs_bwd_f32")


@pytest.mark.parametrize("kw", [
    dict(grad_pos=None, grad_vel=None, grad_acc=None),   # no gradient given
    dict(ntokens=None), dict(w_min=None), dict(w_max=None), dict(basis=None), dict(dof_dst=None),
    dict(grad_ntokens=None),
    dict(N=0), dict(D=0), dict(n_joint=15), dict(T_out=0), dict(num_dof_out=13), dict(B=-1), dict(basis_sb=-1),
    dict(grad_init_p=FAKE),                              # grad_init_p without init_p_src
])
def test_bad_arguments_are_invalid(kw):
    lib = _lib.load()
    assert lib.beast_reconstruct_derivs_bwd_f32(*bwd_args(**kw)) == _lib.BEAST_E_INVALID
    assert lib.beast_last_error()
    # with good arguments an empty batch is a no-op
    assert lib.beast_reconstruct_derivs_bwd_f32(*bwd_args(B=0)) == _lib.BEAST_OK


@pytest.mark.parametrize("kw", [dict(grad_vel=None, grad_acc=None), dict(grad_pos=None), dict(init_p_src=FAKE),
                                dict(init_p_src=FAKE, grad_init_p=FAKE, grad_init_p_sb=14)])
def test_empty_batch_is_ok_for_every_argument_form(kw):
    assert _lib.load().beast_reconstruct_derivs_bwd_f32(*bwd_args(B=0, **kw)) == _lib.BEAST_OK


def test_cpu_tensors_are_refused_with_and_without_grad():
    """A params tensor that requires grad changes nothing: there is no CPU fallback."""
    tok = BEASTBsplineTokenizer(num_dof=7, device="cpu")
    for grad in (False, True):
        params = torch.zeros(2, 70, requires_grad=grad)
        init_p = torch.zeros(2, 7, requires_grad=grad)
        for call in (lambda: tok.reconstruct_traj_continuous(params),
                     lambda: tok.reconstruct_traj_continuous(params.detach(), init_p=init_p),
                     lambda: tok.reconstruct_traj_continuous_derivs(params),
                     lambda: tok.reconstruct_traj_continuous_derivs(params, orders=(2, 0), init_p=init_p)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call()
    with pytest.raises(ValueError, match="orders"):      # still checked first
        tok.reconstruct_traj_continuous_derivs(torch.zeros(2, 70, requires_grad=True), orders=(3,))


def test_bpe_tokenizer_inherits_the_differentiable_methods():
    for name in ("reconstruct_traj_continuous", "reconstruct_traj_continuous_derivs"):
        assert getattr(BEASTBsplineBPETokenizer, name) is getattr(BEASTBsplineTokenizer, name)
