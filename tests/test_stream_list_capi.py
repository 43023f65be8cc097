"""beast_encode_list_f32's envelope (N <= 32, T <= 4096) at the C-ABI, without a GPU: what lies outside
it is refused before any HIP call, and an empty list of a long shape is accepted."""
import ctypes as C

import pytest

from beast_tokenizer_amd import _lib

FAKE = C.c_void_p(16)   # never dereferenced: validation fails first, or there is nothing to launch


def _encode_list(nbatch, T, N, row_elems=14):
    return _lib.load().beast_encode_list_f32(FAKE, nbatch, 4096, T, row_elems, row_elems, row_elems, FAKE, FAKE, N,
                                             FAKE, None)


@pytest.mark.parametrize("T,N", [(4097, 10), (50, 33)])
def test_encode_list_envelope(T, N):
    assert _encode_list(3, T, N) == _lib.BEAST_E_INVALID
    assert b"outside [1," in _lib.load().beast_last_error()


def test_encode_list_long_shape_is_accepted():
    assert _encode_list(0, 300, 10) == _lib.BEAST_OK
    assert _encode_list(0, 257, 17, row_elems=7) == _lib.BEAST_OK   # T * row_elems odd: the streamed branch takes it
