"""Argument validation of the derivative entry points and of the tokenizer's ``orders``: it all
runs before any HIP call, so no GPU is needed."""
import ctypes as C

import pytest
import torch

from beast_tokenizer_amd import BEASTBsplineBPETokenizer, BEASTBsplineTokenizer, _lib
from beast_tokenizer_amd.bspline import DeviceBasis

FAKE = C.c_void_p(16)                   # never dereferenced: validation fails first


def derivs_args(**kw):
    """tokens, B, D, n_joint, N, vocab, tok_offset, w_min, w_max, basis, basis_sb, T_out, dof_dst,
    num_dof_out, init_p, init_p_sb, init_p_src, pos_out, vel_out, acc_out, ntokens, stream"""
    a = dict(tokens=FAKE, B=4, D=14, n_joint=14, N=10, vocab=256, tok_offset=0, w_min=FAKE, w_max=FAKE, basis=FAKE,
             basis_sb=0, T_out=50, dof_dst=FAKE, num_dof_out=14, init_p=None, init_p_sb=0, init_p_src=None,
             pos_out=FAKE, vel_out=FAKE, acc_out=FAKE, ntokens=None, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


@pytest.mark.parametrize("kw", [dict(N=17), dict(D=65, num_dof_out=65), dict(T_out=4097), dict(num_dof_out=4097)])
def test_outside_the_envelope_is_unsupported(kw):
    lib = _lib.load()
    rc = lib.beast_reconstruct_derivs_f32(*derivs_args(**kw))
    assert rc == _lib.BEAST_E_UNSUPPORTED
    with pytest.raises(NotImplementedError, match="reconstruct derivs supports"):
        _lib.check(rc, "beast_reconstruct_derivs_f32")


@pytest.mark.parametrize("kw", [
    dict(pos_out=None, vel_out=None, acc_out=None),      # no output requested
    dict(tokens=None), dict(w_min=None), dict(basis=None), dict(dof_dst=None),
    dict(N=0), dict(D=0), dict(n_joint=15), dict(T_out=0), dict(num_dof_out=13), dict(vocab=1), dict(B=-1),
    dict(basis_sb=-1), dict(init_p=FAKE),                # init_p without init_p_src
])
def test_bad_arguments_are_invalid(kw):
    lib = _lib.load()
    assert lib.beast_reconstruct_derivs_f32(*derivs_args(**kw)) == _lib.BEAST_E_INVALID
    assert lib.beast_last_error()
    # with good arguments an empty batch is a no-op
    assert lib.beast_reconstruct_derivs_f32(*derivs_args(B=0)) == _lib.BEAST_OK


def test_basis_deriv_validation():
    lib = _lib.load()
    #            times n  tau  delay knots n_knots degree num_basis order out stream
    good = [FAKE, 0, 2.0, 0.0, FAKE, 15, 4, 10, 1, FAKE, None]
    assert lib.beast_bspline_basis_deriv_f32(*good) == _lib.BEAST_OK          # n_times = 0: nothing to do
    for i, v in ((0, None), (4, None), (9, None), (8, 3), (8, -1), (6, 9), (5, 14), (1, -1)):
        bad = list(good)
        bad[i] = v
        assert lib.beast_bspline_basis_deriv_f32(*bad) == _lib.BEAST_E_INVALID, (i, v)


@pytest.mark.parametrize("orders", [(), (0, 0), (3,), (1, 2, 1), (-1,), (1.0,), (True,), 1, None, "01"])
def test_bad_orders_raise_value_error(orders):
    tok = BEASTBsplineTokenizer(num_dof=7, device="cpu")
    toks = torch.zeros((2, 70), dtype=torch.int64)
    with pytest.raises(ValueError, match="orders"):
        tok.reconstruct_traj_derivs(toks, orders=orders)
    with pytest.raises(ValueError, match="orders"):
        tok.reconstruct_traj_continuous_derivs(torch.zeros(2, 70), orders=orders)


def test_cpu_tensors_are_refused():
    """As the other entry points refuse them: there is no CPU fallback."""
    tok = BEASTBsplineTokenizer(num_dof=7, device="cpu")
    toks = torch.zeros((2, 70), dtype=torch.int64)
    for call in (lambda: tok.reconstruct_traj_derivs(toks), lambda: tok.reconstruct_traj_vel(toks),
                 lambda: tok.reconstruct_traj_acc(toks),
                 lambda: tok.reconstruct_traj_continuous_derivs(torch.zeros(2, 70))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    basis = DeviceBasis(10, 4, 2.0, False)
    for call in (lambda: basis.deriv_basis_at(torch.zeros(5), 1), lambda: basis.full_deriv_basis_at(torch.zeros(5), 2)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="order"):
        basis.deriv_basis_at(torch.zeros(5), 3)


def test_bpe_tokenizer_has_the_methods():
    for name in ("reconstruct_traj_derivs", "reconstruct_traj_vel", "reconstruct_traj_acc"):
        assert name in vars(BEASTBsplineBPETokenizer)
