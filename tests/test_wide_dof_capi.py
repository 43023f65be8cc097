"""The wide-DoF envelope (65 <= D <= 256) of beast_encode_f32 / beast_encode_list_f32 /
beast_quantize_f32 / beast_reconstruct_f32 at the C-ABI, without a GPU: B = 0 passes validation and
launches nothing, what lies outside is refused before any HIP call, the chunk queries are pure host
functions, and what the tokenizer cannot do at num_dof > 64 raises before the device is asked for."""
import ctypes as C

import pytest
import torch

from beast_tokenizer_amd import BEASTBsplineTokenizer, _lib

FAKE = C.c_void_p(16)   # never dereferenced: B = 0 returns, or validation fails, first


def _calls(D, basis_sb=0):
    lib = _lib.load()
    return {
        "encode": lambda: lib.beast_encode_f32(FAKE, 0, 50, 50 * D, D, 1, D, D, D, FAKE, FAKE, 10, FAKE, FAKE, 256, 0,
                                               FAKE, FAKE, None),
        "encode_list": lambda: lib.beast_encode_list_f32(FAKE, 0, 8, 50, D, D, D, FAKE, FAKE, 10, FAKE, None),
        "quantize": lambda: lib.beast_quantize_f32(FAKE, 0, D, 10, FAKE, FAKE, 256, 0, 0, FAKE, None, None),
        "reconstruct": lambda: lib.beast_reconstruct_f32(FAKE, 0, D, D, 10, 256, 0, FAKE, FAKE, FAKE, basis_sb, 50, FAKE,
                                                         D, None, 0, None, None, FAKE, None, None),
    }


@pytest.mark.parametrize("entry", ["encode", "encode_list", "quantize", "reconstruct"])
@pytest.mark.parametrize("D,code", [(65, _lib.BEAST_OK), (256, _lib.BEAST_OK), (257, _lib.BEAST_E_INVALID)])
def test_dof_envelope(entry, D, code):
    assert _calls(D)[entry]() == code


def test_per_trajectory_basis_stops_at_64():
    assert _calls(65, basis_sb=2 * 50 * 10)["reconstruct"]() == _lib.BEAST_E_UNSUPPORTED
    assert b"per-trajectory bases stop at D = 64" in _lib.load().beast_last_error()


def test_chunk_queries():
    lib = _lib.load()
    enc, rec = lib.beast_encode_stream_chunk, lib.beast_reconstruct_stream_rows
    for D in (65, 256):
        for T, N, nj in ((50, 10, D), (4096, 32, D - 2)):   # streamed at every T and N, a function of (N, kinds)
            tc, rc = enc(T, D, D, nj, N, 1), rec(T, D, nj, N, D)
            assert tc > 0 and tc % 4 == 0 and tc == enc(T, D, D, nj, N, 1) == enc(7, 65, 300, 65 - D + nj, N, 0)
            assert rc > 0 and rc % 16 == 0 and rc == rec(T, D, nj, N, D) == rec(7, 65, 65 - D + nj, N, 4096)
    assert enc(50, 257, 257, 257, 10, 1) == 0 and rec(50, 257, 257, 10, 257) == 0
    # D <= 64: what the parent commit returned
    assert enc(50, 14, 14, 14, 10, 1) == 0 and rec(50, 14, 14, 10, 14) == 0
    assert (enc(257, 14, 14, 14, 10, 1), enc(50, 14, 14, 14, 17, 1), enc(300, 14, 16, 12, 20, 0)) == (48, 40, 32)
    assert (rec(50, 14, 14, 17, 14), rec(50, 14, 12, 32, 17)) == (64, 32)


@pytest.mark.parametrize("call", [
    lambda tok, x: tok.encode_at(x, torch.linspace(0, 1, 50)),
    lambda tok, x: tok.encode_windows(x[0], torch.tensor([0]), torch.tensor([50])),
    lambda tok, x: tok.reconstruct_traj_derivs(torch.zeros(2, 650, dtype=torch.int64)),
    lambda tok, x: BEASTBsplineTokenizer(num_dof=65, init_cond_order=1, device="cpu").encode(x),
], ids=["encode_at", "encode_windows", "reconstruct_traj_derivs", "conditioned_encode"])
def test_tokenizer_refuses_before_the_device(call):
    with pytest.raises(NotImplementedError, match="num_dof <= 64"):
        call(BEASTBsplineTokenizer(num_dof=65, device="cpu"), torch.zeros(2, 50, 65))
