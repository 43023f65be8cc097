"""beast::exact_quotient (csrc/common.h) is RN(t / (V - 1)) for every vocab V in 2..4096 and every
token t in 0..4095: all 16.8 M pairs, in exact integer arithmetic.

The device function is

    r  = RN(1 / vm1)            vm1 = (float)(V - 1); IEEE division on the host, an argument
    q0 = RN(t * r)              __fmul_rn
    e  = fma(-q0, vm1, t)       __fmaf_rn: one rounding
    q  = fma(e, r, q0)          __fmaf_rn: one rounding

and k_reconstruct_v uses q in place of the dequantise LUT's __fdiv_rn(t, vm1).  Here the two FMAs are
evaluated on integers: a float32 is m * 2^x with |m| < 2^24, so t - q0 * vm1 and e * r + q0 are integers
times a power of two, formed exactly in int64 and rounded once to 24 significant bits, ties to even.
No wider float takes part.  The multiplication and the two divisions (r, and the reference t / vm1) are
single float32 operations of numpy, correctly rounded by IEEE 754.
"""
import numpy as np

F32 = np.float32
VMAX = 4096      # beast::EXACT_QUOTIENT_MAX


def _split(x):
    """float32 array -> (m, x) with value m * 2^x exactly, m an int64 of at most 24 bits."""
    m, e = np.frexp(x)                                  # exact: x = m * 2^e, |m| in [0.5, 1)
    return np.ldexp(m, 24).astype(np.int64), e.astype(np.int64) - 24


def _bitlen(a):
    """Bit length of non-negative int64 (< 2^62)."""
    _, e = np.frexp(a.astype(np.float64))               # may round up across a power of two: corrected below
    e = e.astype(np.int64)
    return np.where(a == 0, 0, e - ((a >> np.maximum(e - 1, 0)) == 0))


def _round_parts(s, x):
    """RN_even(s * 2^x) to 24 significant bits, s int64 (|s| < 2^62), by integer arithmetic alone:
    (float32 value, m, y) with value = m * 2^y exactly and |m| <= 2^24.  The results here are zero or far
    above the subnormals (>= 2^-60), so 24 bits is the whole story."""
    neg = s < 0
    a = np.abs(s)
    sh = np.maximum(_bitlen(a) - 24, 0)
    q = a >> sh
    rem = a - (q << sh)
    half = np.where(sh > 0, np.int64(1) << np.maximum(sh - 1, 0), np.int64(0))
    up = (sh > 0) & ((rem > half) | ((rem == half) & ((q & 1) == 1)))
    q = q + up                                          # 2^24 after a carry is still exact in float32
    v = np.ldexp(q.astype(F32), (x + sh).astype(np.int32))
    return np.where(neg, -v, v).astype(F32), np.where(neg, -q, q), x + sh


def _round_f32(s, x):
    return _round_parts(s, x)[0]


def exact_quotient(t, vm1, r):
    """beast::exact_quotient of csrc/common.h, restated: t, vm1, r float32 arrays (t, vm1 integers)."""
    q0 = (t * r).astype(F32)                            # q0 = __fmul_rn(t, r)
    mq, xq = _split(q0)                                 # q0 = mq * 2^xq; q0 < 4096, so xq <= -11
    assert (xq <= 0).all() and (xq >= -40).all()
    ti, vi = t.astype(np.int64), vm1.astype(np.int64)
    # e = __fmaf_rn(-q0, vm1, t):  t - q0 * vm1 = (t * 2^-xq - mq * vm1) * 2^xq, exactly (< 2^49 in int64)
    _, me, xe = _round_parts((ti << -xq) - mq * vi, xq)          # e = me * 2^xe, me not normalised: it stays small
    # q = __fmaf_rn(e, r, q0):  e * r + q0 = (me * mr * 2^(xe + xr - x) + mq * 2^(xq - x)) * 2^x, x the smaller exponent
    mr, xr = _split(r)
    xp = xe + xr
    x = np.minimum(xp, xq)
    assert (np.abs(me) < (1 << 20)).all()                         # the remainder is a few thousand units of q0's last place
    assert ((xp - x) <= 16).all() and ((xq - x) <= 37).all()     # 44 + 16 and 24 + 37 bits: inside int64
    return _round_f32(((me * mr) << (xp - x)) + (mq << (xq - x)), x)


def test_split_and_round_helpers():
    """The helpers on values whose answers are known: exact splits, ties to even, a carry into 2^24."""
    x = np.array([0.0, 1.0, 0.5, 3.0, 1 / 3, 16777215.0], dtype=F32)
    m, e = _split(x)
    assert np.array_equal(np.ldexp(m.astype(np.float64), e.astype(np.int32)), x.astype(np.float64))
    s = np.array([(1 << 24) + 1, (1 << 24) + 3, (1 << 25) + 2, (1 << 25) + 6, (1 << 25) - 1, -((1 << 24) + 3), 5, 0],
                 dtype=np.int64)
    want = np.array([1 << 24, (1 << 24) + 4, 1 << 25, (1 << 25) + 8, 1 << 25, -((1 << 24) + 4), 5, 0], dtype=np.float64)
    got = _round_f32(s, np.zeros(len(s), dtype=np.int64))
    assert np.array_equal(got.astype(np.float64), want)
    assert np.array_equal(_bitlen(np.array([0, 1, 2, 3, (1 << 53) - 1, 1 << 53, (1 << 60) - 1], dtype=np.int64)),
                          [0, 1, 2, 2, 53, 54, 60])


def test_exact_quotient_equals_ieee_division_everywhere():
    t = np.arange(VMAX, dtype=F32)[None, :]
    bad = 0
    for v0 in range(2, VMAX + 1, 256):                  # 256 vocabularies x 4096 tokens at a time
        vs = np.arange(v0, min(v0 + 256, VMAX + 1))
        vm1 = (vs - 1).astype(F32)[:, None]
        r = (F32(1) / vm1).astype(F32)
        tt, vv, rr = np.broadcast_arrays(t, vm1, r)
        got = exact_quotient(tt.ravel(), vv.ravel(), rr.ravel())
        want = (tt / vv).astype(F32).ravel()            # numpy's float32 t / (V - 1)
        bad += int((got.view(np.int32) != want.view(np.int32)).sum())
    assert bad == 0, f"{bad} of {(VMAX - 1) * VMAX} (V, t) pairs differ from the IEEE quotient"
