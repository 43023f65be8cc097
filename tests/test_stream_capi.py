"""The streamed envelope of beast_encode_f32 / beast_reconstruct_f32 (N <= 32, T <= 4096) at the C-ABI,
without a GPU: what lies outside it is refused before any HIP call, and the two chunk queries are
pure host functions.  No call here passes an in-envelope shape with its fake pointers."""
import ctypes as C

import pytest

from beast_tokenizer_amd import _lib

FAKE = C.c_void_p(16)   # never dereferenced: validation fails first


def _encode(T, N):
    return _lib.load().beast_encode_f32(FAKE, 4, T, T * 14, 14, 1, 14, 14, 14, FAKE, FAKE, N, FAKE, FAKE, 256, 0,
                                        FAKE, FAKE, None)


def _reconstruct(N, basis_sb):
    return _lib.load().beast_reconstruct_f32(FAKE, 4, 14, 14, N, 256, 0, FAKE, FAKE, FAKE, basis_sb, 50, FAKE, 14,
                                             None, 0, None, None, FAKE, None, None)


@pytest.mark.parametrize("T,N,code", [(50, 33, _lib.BEAST_E_UNSUPPORTED), (4097, 10, _lib.BEAST_E_UNSUPPORTED),
                                      (0, 10, _lib.BEAST_E_INVALID)])
def test_encode_envelope(T, N, code):
    assert _encode(T, N) == code
    assert b"T=" in _lib.load().beast_last_error()


def test_reconstruct_envelope():
    assert _reconstruct(33, 0) == _lib.BEAST_E_UNSUPPORTED
    assert _reconstruct(17, 50 * 17 * 2) == _lib.BEAST_E_UNSUPPORTED
    assert b"per-trajectory bases stop at N = 16" in _lib.load().beast_last_error()


def test_projection_stops_at_32():
    assert _lib.load().beast_bspline_projection_f64(FAKE, 50, 33, 1e-9, FAKE, None) == _lib.BEAST_E_INVALID


def test_chunk_queries_are_pure():
    lib = _lib.load()
    enc = lambda T, N: lib.beast_encode_stream_chunk(T, 14, 14, 14, N, 1)   # noqa: E731
    rec = lambda T, N: lib.beast_reconstruct_stream_rows(T, 14, 14, N, 14)   # noqa: E731
    assert enc(50, 10) == 0 and rec(50, 10) == 0          # a resident kernel serves the shape
    for T, N in ((257, 10), (50, 17)):
        tc = enc(T, N)
        assert tc > 0 and tc % 4 == 0 and tc == enc(T, N)
    rc = rec(50, 17)
    assert rc > 0 and rc % 4 == 0 and rc == rec(50, 17) == rec(4096, 17)
    assert enc(50, 33) == 0 and enc(4097, 10) == 0 and rec(50, 33) == 0   # what the entry points refuse
