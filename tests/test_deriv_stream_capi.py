"""beast_reconstruct_derivs_stream_rows, the chunk length beast_reconstruct_derivs_f32 streams a shared
basis with: a pure host function, so no GPU is needed.  D 14, n_joint 14, num_dof_out 14 throughout;
at N 10 (12 padded columns) three slabs fit the resident kernel's 48 KB up to T_out 341."""
import pytest

from beast_tokenizer_amd import _lib


def rows(T_out, N=10, mask=7):
    return _lib.load().beast_reconstruct_derivs_stream_rows(T_out, 14, 14, N, 14, mask)


@pytest.mark.parametrize("T_out", [2000, 342])
def test_streamed_shapes_have_a_chunk(T_out):
    rc = rows(T_out)
    assert rc > 0 and rc % 4 == 0 and rc == rows(T_out)


@pytest.mark.parametrize("kw", [dict(T_out=50), dict(T_out=341),                      # the resident kernel's
                                dict(T_out=2000, N=17), dict(T_out=4097), dict(T_out=2000, mask=0)])   # refused
def test_no_chunk_where_nothing_streams(kw):
    assert rows(**kw) == 0
