"""beast_sample_rows and ``sample_tokens_from_logits`` on the GPU, against the float64 definition
(tests/sample_oracle.py; include/beast_hip.h).

No token is compared with the oracle's token: where a uniform lies within rounding of a CDF edge, or a
nucleus' mass within rounding of top_p, two correct implementations differ.  Instead EVERY row must
pass, in float64 from the kernel's own outputs (``check_rows``):
    (a) the kept set is legal: kept_out = c is value-closed (the c-th largest logit is strictly above
        the (c+1)-th, or c = V); c <= |K1| with |K1| exact, c == |K1| when top_p = 1; when top_p < 1 the
        mass of the top c over S1 is >= top_p - delta and the mass without its lowest value group is
        < top_p + delta (or there is only one group);
    (b) the draw is legal: tok is kept and e_tok > 0, and u lies in
        [C_{tok-1} / S2 - delta, C_tok / S2 + delta] on the kernel's own kept set;
    (c) |logprob - ((z_tok - zmax) - log S2)| <= bound * max(1, |that|).
delta and the bound of (c) are measured, not fixed in advance (the rule of tests/test_gpu_logits.py):
4x the largest error, on the same inputs and the same kept set, of torch's own fp32 composition on the
CPU -- softmax, mask, renormalise, cumsum (delta) and the log of the renormalised probability (c) --
against float64, with a floor of 16 * 2^-24.  Every check prints what it measured.
"""
import numpy as np
import pytest
import torch

import sample_oracle as SO
from beast_tokenizer_amd import BEASTBsplineBPETokenizer, BEASTBsplineTokenizer, _lib

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
FLOOR = 16 * EPS
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
WIDEST = {"fp32": 1024, "fp16": 2048, "bf16": 2048}          # the last in-register width
TAUS = (0.25, 1.0, 3.0)


def bound(yardstick):
    return max(4 * yardstick, FLOOR)


def bits(t):
    return t.contiguous().view(torch.uint8) if t.dtype != torch.uint8 else t


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def randn4(shape, dtype, dev, seed, scale=4.0):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=gen, dtype=torch.float32) * scale).to(dtype).to(dev)


def uniforms(S, B, K, dev, seed):
    return torch.rand((S, B, K), generator=torch.Generator().manual_seed(seed), dtype=torch.float32).to(dev)


# ------------------------------------------------------------------ the raw entry point --
def raw_rc(l, u, tau=1.0, top_k=0, top_p=1.0, off=0, tok=None, lp=None, kept=None, stream=None):
    B, K, V = l.shape
    return _lib.call("beast_sample_rows", l.data_ptr(), _lib.LOGITS_DTYPES[l.dtype], B, K, V, l.stride(0), l.stride(1),
                     tau, top_k, top_p, u.data_ptr(), u.shape[0], off, _lib.ptr(tok), _lib.ptr(lp), _lib.ptr(kept),
                     _lib.stream_of(l.device) if stream is None else stream)


def sample(l, u, tau=1.0, top_k=0, top_p=1.0, off=0, logprob=True, kept=True):
    """beast_sample_rows on a [B, K, V] view with uniforms [S, B, K]; returns (tokens, logprob, kept),
    poisoned first."""
    B, K, V = l.shape
    S, dev = u.shape[0], l.device
    assert u.shape == (S, B, K) and u.dtype == torch.float32 and u.is_contiguous()
    tok = torch.full((S, B, K), -7, dtype=torch.int64, device=dev)
    lp = torch.full((S, B, K), float("nan"), device=dev) if logprob else None
    kp = torch.full((B, K), -7, dtype=torch.int32, device=dev) if kept else None
    _lib.check(raw_rc(l, u, tau, top_k, top_p, off, tok, lp, kp), "beast_sample_rows")
    return tok, lp, kp


# ------------------------------------------------------------------------- the checks --
class Rows:
    """What the checks need of one logits tensor, computed once and left unchanged."""

    def __init__(self, l):
        self.V = l.shape[-1]
        self.l = l.detach().to("cpu", torch.float64).reshape(-1, self.V)
        self.l32 = self.l.to(torch.float32)
        self._sorted = None

    def sorted(self):
        if self._sorted is None:
            self._sorted = torch.sort(self.l, dim=-1, descending=True, stable=True)
        return self._sorted


def check_rows(rows, tau, top_k, top_p, calls, tag, off=0):
    """(a) - (c) for every row; ``calls`` is a list of (u, tok, lp, kept) device tensors from calls on
    the same logits and parameters (their kept sets must agree bitwise).  Returns the measured
    (delta error, logprob error) over their bounds."""
    l, V = rows.l, rows.V
    R = l.shape[0]
    z = l / tau
    d = z - z.max(-1, keepdim=True).values
    e = d.exp()
    c = calls[0][3].cpu().long().reshape(R)
    for call in calls[1:]:
        assert torch.equal(call[3].cpu().long().reshape(R), c), tag
    assert bool(((c >= 1) & (c <= V)).all()), tag
    truncating = 1 <= top_k < V or top_p < 1.0
    if truncating:
        ls, order = rows.sorted()
        thr = ls.gather(1, (c - 1)[:, None])                                   # the lowest kept value
        nxt = ls.gather(1, c.clamp(max=V - 1)[:, None])
        assert bool(((c == V) | (thr > nxt)[:, 0]).all()), f"{tag}: a kept set is not value-closed"
        k1 = (ls >= ls[:, top_k - 1:top_k]).sum(-1) if 1 <= top_k < V else torch.full((R,), V)
        assert bool((c <= k1).all()), f"{tag}: more bins kept than top_k allows"
        if top_p >= 1.0:
            assert torch.equal(c, k1), f"{tag}: top_p = 1 must keep exactly the top-k set"
        mask = l >= thr
    else:
        assert bool((c == V).all()), tag
        mask = torch.ones_like(l, dtype=torch.bool)
    em = e * mask
    C = em.cumsum(-1)
    S2 = C[:, -1:]
    # the yardstick: torch's fp32 softmax, mask, renormalise, cumsum on the same inputs
    pm = torch.softmax(rows.l32 / tau, -1) * mask
    pm = pm / pm.sum(-1, keepdim=True)
    y_delta = float((pm.cumsum(-1).double() - C / S2).abs().max())
    delta = bound(y_delta)
    if top_p < 1.0:
        cum = e.gather(1, order).cumsum(-1)
        S1 = cum.gather(1, (k1 - 1)[:, None])
        top = cum.gather(1, (c - 1)[:, None]) / S1
        assert bool((top >= top_p - delta).all()), f"{tag}: a nucleus holds less than top_p ({float(top.min())})"
        g0 = (ls > thr).sum(-1)                                                # where the lowest group starts
        without = cum.gather(1, (g0 - 1).clamp(min=0)[:, None]) / S1
        assert bool(((g0 == 0) | (without[:, 0] < top_p + delta)).all()), f"{tag}: a nucleus is larger than needed"
    e_delta = e_lp = y_lp = 0.0
    for u, tok, lp, _ in calls:
        S = u.shape[0]
        t = (tok.cpu() - off).reshape(S, R).T                                  # [R, S]
        assert bool(((t >= 0) & (t < V)).all()), f"{tag}: a token is out of range"
        emt = em.gather(1, t)
        assert bool((emt > 0).all()), f"{tag}: a bin outside the kept set, or one without mass, was drawn"
        Ct = C.gather(1, t)
        u64 = u.cpu().double().reshape(S, R).T
        lo, hi = (Ct - emt) / S2, Ct / S2
        e_delta = max(e_delta, float(torch.maximum(lo - u64, u64 - hi).max()))
        assert bool(((u64 >= lo - delta) & (u64 <= hi + delta)).all()), \
            f"{tag}: a uniform lies {e_delta:.3e} outside its token's interval (delta {delta:.3e})"
        want = d.gather(1, t) - S2.log()
        scale = want.abs().clamp(min=1.0)
        y_lp = max(y_lp, float(((pm.log().gather(1, t).double() - want).abs() / scale).max()))
        e_lp = max(e_lp, float(((lp.cpu().double().reshape(S, R).T - want).abs() / scale).max()))
    print(f"{tag} tau {tau} k {top_k} p {top_p}: interval {max(e_delta, 0.0):.3e} of delta {delta:.3e} "
          f"({max(e_delta, 0.0) / delta:.0%})  logprob {e_lp:.3e} of bound {bound(y_lp):.3e} ({e_lp / bound(y_lp):.0%})")
    assert e_lp <= bound(y_lp), (tag, e_lp, bound(y_lp))
    return max(e_delta, 0.0) / delta, e_lp / bound(y_lp)


def run_and_check(l, rows, tau, top_k, top_p, tag, seed):
    """S = 5 and S = 1 on the same logits, both against (a) - (c)."""
    B, K, _ = l.shape
    calls = []
    for S in (5, 1):
        u = uniforms(S, B, K, l.device, seed + S)
        calls.append((u, *sample(l, u, tau, top_k, top_p, off=3)))
    torch.cuda.synchronize(l.device)
    return check_rows(rows, tau, top_k, top_p, calls, tag, off=3)


BKS = [(1, 1), (3, 7), (2, 140), (37, 140)]


@pytest.mark.parametrize("BK", BKS, ids=lambda bk: f"B{bk[0]}K{bk[1]}")
@pytest.mark.parametrize("V", [2, 3, 255, 256, 257, 1000, 4097])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_plain_sampling_against_the_oracle(dtype, V, BK, gpu_device):
    """V 2, 3: one lane partly filled; 255 / 256 / 257 (fp32): a partial chunk, a chunk exactly full,
    one element past a chunk; 1000: several chunks in registers; 4097: the two-pass form."""
    l = randn4((*BK, V), DTYPES[dtype], gpu_device, seed=V * 1000 + BK[0])
    rows = Rows(l)
    for tau in TAUS:
        run_and_check(l, rows, tau, 0, 1.0, f"{dtype} V{V} B{BK[0]} K{BK[1]}", seed=V)


@pytest.mark.parametrize("BK", BKS, ids=lambda bk: f"B{bk[0]}K{bk[1]}")
@pytest.mark.parametrize("V", [2, 3, 255, 256, 257, 1000, "widest"])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_truncated_sampling_against_the_oracle(dtype, V, BK, gpu_device):
    """top_k in {0, 1, 5, V-1} x top_p in {0.1, 0.9, 1}, the temperatures in rotation; bf16 at V 1000
    has real tie groups at both thresholds.  "widest": the last in-register width."""
    V = WIDEST[dtype] if V == "widest" else V
    l = randn4((*BK, V), DTYPES[dtype], gpu_device, seed=V * 1000 + BK[0] + 1)
    rows = Rows(l)
    if dtype == "bf16" and V == 1000 and BK[1] == 140:
        ls = rows.sorted()[0]
        assert float((ls[:, 4] == ls[:, 5]).double().mean()) > 0.01          # ties at the 5th value
    n = 0
    for top_k in sorted({0, 1, 5, V - 1}):
        for top_p in (0.1, 0.9, 1.0):
            run_and_check(l, rows, TAUS[n % 3], top_k, top_p, f"{dtype} V{V} B{BK[0]} K{BK[1]}", seed=V + n)
            n += 1


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_truncation_beyond_the_in_register_rows_is_unsupported(dtype, gpu_device):
    V = WIDEST[dtype] + 1
    l = randn4((2, 3, V), DTYPES[dtype], gpu_device, seed=1)
    u = uniforms(1, 2, 3, gpu_device, 1)
    tok = torch.full((1, 2, 3), -7, dtype=torch.int64, device=gpu_device)
    for kw in (dict(top_k=5), dict(top_p=0.9)):
        assert raw_rc(l, u, tok=tok, **kw) == _lib.BEAST_E_UNSUPPORTED
    torch.cuda.synchronize(gpu_device)
    assert bool((tok == -7).all())
    rows = Rows(l)
    run_and_check(l, rows, 1.0, 0, 1.0, f"{dtype} V{V} plain", seed=2)          # plain sampling goes on
    run_and_check(l, rows, 1.0, V, 1.0, f"{dtype} V{V} top_k = V", seed=3)


# ----------------------------------------------------------------- stratified uniforms --
@pytest.mark.parametrize("top_p", [1.0, 0.9])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_stratified_uniforms_hit_every_bin_within_two(dtype, top_p, gpu_device):
    """M identical rows, u_j = (j + 1/2) / M: a grid of spacing 1 / M puts M P_v +- 1 points into an
    interval of length P_v, and the second unit covers its two edges moving by delta (M delta << 1)."""
    M, V = 4096, 256
    row = randn4((V,), DTYPES[dtype], gpu_device, seed=11)
    l = row.expand(M, 1, V).contiguous()
    u = ((torch.arange(M, dtype=torch.float64) + 0.5) / M).to(torch.float32).reshape(1, M, 1).to(gpu_device)
    tok, _, kept = sample(l, u, 1.0, 0, top_p)
    P = SO.probabilities(row.double().cpu().numpy()[None], 1.0, 0, top_p)[0]
    counts = np.bincount(tok.cpu().numpy().reshape(-1), minlength=V)
    worst = float(np.abs(counts - M * P).max())
    print(f"stratified {dtype} top_p {top_p}: max |count - M P| = {worst:.3f}, kept {int(kept[0, 0])}")
    assert int(kept[0, 0]) == int((P > 0).sum()) and bool((kept == kept[0, 0]).all())
    assert worst <= 2.0


# ------------------------------------------------------------------------- edge cases --
@pytest.mark.parametrize("V", [256, 1000, 4097])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_the_ends_of_the_unit_interval(dtype, V, gpu_device):
    """u = 0 gives the lowest kept bin that has mass, u = 1 - 2^-24 a valid bin, plain and truncated."""
    l = randn4((4, 6, V), DTYPES[dtype], gpu_device, seed=V + 7)
    l[0, 0, :3] = float("-inf")                                  # the lowest bins without mass
    rows = Rows(l)
    u = torch.zeros((2, 4, 6), device=gpu_device)
    u[1] = 1.0 - EPS
    for top_k, top_p in ((0, 1.0),) + (((5, 1.0), (0, 0.5)) if V <= 2048 else ()):
        tok, lp, kept = sample(l, u, 1.0, top_k, top_p)
        check_rows(rows, 1.0, top_k, top_p, [(u, tok, lp, kept)], f"ends {dtype} V{V}")
        want = SO.sample(rows.l.numpy(), np.zeros((1, 24)), 1.0, top_k, top_p)
        if torch.equal(kept.cpu().long().reshape(-1), torch.from_numpy(want[2])):
            assert np.array_equal(tok[0].cpu().numpy().reshape(-1), want[0][0])
    assert int(tok[0, 0, 0]) >= 3


@pytest.mark.parametrize("V", [256, 4097])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_minus_infinity_entries_are_never_drawn(dtype, V, gpu_device):
    """Half the entries -inf, bins 0 and V-1 among them, and one row with a single survivor."""
    l = randn4((4, 6, V), DTYPES[dtype], gpu_device, seed=V + 1)
    dead = torch.rand((4, 6, V), generator=torch.Generator().manual_seed(1)) < 0.5
    dead[..., 0] = True
    dead[..., V - 1] = True
    dead[0, 0] = True
    dead[0, 0, V // 2] = False                                    # one survivor
    l[dead.to(gpu_device)] = float("-inf")
    rows = Rows(l)
    u = uniforms(16, 4, 6, gpu_device, 5)
    u[0] = 0.0
    u[1] = 1.0 - EPS
    for top_k, top_p in ((0, 1.0),) + (((V - 1, 1.0), (0, 0.9)) if V <= 2048 else ()):
        tok, lp, kept = sample(l, u, 0.5, top_k, top_p)
        assert not bool(torch.isneginf(l.gather(2, tok.permute(1, 2, 0))).any())
        assert bool(torch.isfinite(lp).all())
        assert bool((tok[:, 0, 0] == V // 2).all()) and float(lp[:, 0, 0].abs().max()) == 0.0
        check_rows(rows, 0.5, top_k, top_p, [(u, tok, lp, kept)], f"-inf {dtype} V{V}")


def test_top_k_one_is_the_greedy_token(gpu_device):
    """bf16 randn * 2 has a tied maximum in about 2 % of its 256-wide rows: top_k = 1 equals
    greedy_tokens_from_logits where the maximum is single and lands in the tie set otherwise."""
    tok = make_tok(gpu_device)
    l = randn4((64, 140, 256), torch.bfloat16, gpu_device, seed=2, scale=2.0)
    raw = l.float()
    tied = (raw == raw.max(-1, keepdim=True).values).sum(-1) > 1
    assert int(tied.sum()) >= 20
    u = uniforms(3, 64, 140, gpu_device, 4)
    got, lp, kept = sample(l, u, 1.0, 1, 1.0)
    greedy = tok.greedy_tokens_from_logits(l)
    assert torch.equal(kept.long(), (raw == raw.max(-1, keepdim=True).values).sum(-1))
    for s in range(3):
        assert torch.equal(got[s][~tied], greedy[~tied])
        assert bool((raw.gather(2, got[s][..., None])[..., 0] == raw.max(-1).values).all())
    assert float(lp[:, ~tied].abs().max()) == 0.0
    assert bool((got[:, tied] != greedy[tied][None]).any())          # the tie set is really sampled


@pytest.mark.parametrize("V", [256, 4097])
def test_unspecified_rows_do_not_disturb_the_others(V, gpu_device):
    """A NaN row, a +inf row, an all -inf row and a NaN uniform in the middle of a batch: every other
    row is bitwise what it is in the batch without them, and every token is in range."""
    clean = randn4((3, 9, V), torch.float32, gpu_device, seed=V + 2)
    dirty = clean.clone()
    dirty[1, 3, V // 3] = float("nan")
    dirty[1, 4, V // 2] = float("inf")
    dirty[1, 5] = float("-inf")
    u = uniforms(4, 3, 9, gpu_device, 6)
    ud = u.clone()
    ud[2, 1, 6] = float("nan")
    ud[1, 1, 7] = 1.5
    keep = torch.ones((3, 9), dtype=torch.bool, device=gpu_device)
    keep[1, 3:8] = False
    for top_k, top_p in ((0, 1.0),) + (((5, 0.9),) if V <= 1024 else ()):
        want = sample(clean, u, 1.0, top_k, top_p, off=100)
        got = sample(dirty, ud, 1.0, top_k, top_p, off=100)
        assert same_bits(got[0][:, keep], want[0][:, keep]) and same_bits(got[1][:, keep], want[1][:, keep])
        assert same_bits(got[2][keep], want[2][keep])
        assert bool(((got[0] >= 100) & (got[0] < 100 + V)).all())
    torch.cuda.synchronize(gpu_device)


# -------------------------------------------------------- the siblings' bitwise properties --
@pytest.mark.parametrize("V", [257, 4097])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_runs_agree_bitwise_rows_do_not_depend_on_the_batch_nor_draws_on_each_other(dtype, V, gpu_device):
    l = randn4((6, 11, V), DTYPES[dtype], gpu_device, seed=V)
    u = uniforms(7, 6, 11, gpu_device, V)
    for top_k, top_p in ((0, 1.0),) + (((9, 0.8),) if V <= 1024 else ()):
        first = sample(l, u, 1.3, top_k, top_p)
        again = sample(l, u, 1.3, top_k, top_p)
        assert all(same_bits(a, b) for a, b in zip(first, again))
        for b, k in ((0, 0), (2, 5), (5, 10)):
            one = sample(l[b:b + 1, k:k + 1], u[:, b:b + 1, k:k + 1].contiguous(), 1.3, top_k, top_p)
            assert all(same_bits(x, y[..., b:b + 1, k:k + 1]) for x, y in zip(one, first))
        for s in (0, 3, 6):                                        # draw s alone: the S = 1 call with u_s
            one = sample(l, u[s:s + 1].contiguous(), 1.3, top_k, top_p)
            assert same_bits(one[0], first[0][s:s + 1]) and same_bits(one[1], first[1][s:s + 1])
            assert same_bits(one[2], first[2])
        few = sample(l, u, 1.3, top_k, top_p, logprob=False, kept=False)      # the optional outputs
        assert same_bits(few[0], first[0]) and few[1] is None and few[2] is None
    many = uniforms(64, 6, 11, gpu_device, V + 1)                  # the most draws a call takes
    m = sample(l, many, 1.3)
    assert same_bits(sample(l, many[40:41].contiguous(), 1.3)[0], m[0][40:41])
    check_rows(Rows(l), 1.3, 0, 1.0, [(many, *m)], f"S 64 {dtype} V{V}")


@pytest.mark.parametrize("start", [13, 48])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_strided_slices_equal_the_contiguous_tensor_bitwise(dtype, start, gpu_device):
    """A 252-wide slice of a [B, K, 300] tensor from element 13 (no row is 16-byte aligned) and from 48
    (every fp32 row is; with 2-byte elements the 600-byte row stride alternates): a full-vocabulary
    view of the action slice is such a tensor."""
    dt, V = DTYPES[dtype], 252
    full = randn4((5, 9, 300), dt, gpu_device, seed=start)
    view = full[..., start:start + V]
    assert view.stride() == (9 * 300, 300, 1) and view.data_ptr() == full.data_ptr() + start * full.element_size()
    aligned = {(view[b, k].data_ptr() % 16 == 0) for b in range(5) for k in range(9)}
    assert aligned == ({False} if start == 13 else {True} if dt is torch.float32 else {True, False})
    flat = view.contiguous()
    assert flat.data_ptr() % 16 == 0
    u = uniforms(5, 5, 9, gpu_device, start)
    for tau, top_k, top_p in ((0.5, 0, 1.0), (2.0, 7, 0.9)):
        want = sample(flat, u, tau, top_k, top_p, off=100)
        got = sample(view, u, tau, top_k, top_p, off=100)
        assert all(same_bits(a, b) for a, b in zip(got, want))
    tail = full[..., 300 - V:]                                     # up to the end of every row
    assert all(same_bits(a, b) for a, b in zip(sample(tail, u, 1.0, 7, 0.9), sample(tail.contiguous(), u, 1.0, 7, 0.9)))


def test_offsets_beyond_two_to_the_31_elements(gpu_device):
    """A [2, 3, 256] bf16 view with a batch stride of 2^31 + 8 elements over one uninitialised
    allocation (about 4.3 GB; only the six rows are ever written or read): bitwise the contiguous case."""
    sb = 2 ** 31 + 8
    vals = randn4((2, 3, 256), torch.bfloat16, gpu_device, seed=31)
    u = uniforms(4, 2, 3, gpu_device, 31)
    src = torch.empty(sb + 3 * 256, dtype=torch.bfloat16, device=gpu_device).as_strided((2, 3, 256), (sb, 256, 1))
    src.copy_(vals)
    for top_k, top_p in ((0, 1.0), (5, 0.9)):
        want = sample(vals, u, 0.7, top_k, top_p, off=7)
        got = sample(src, u, 0.7, top_k, top_p, off=7)
        assert all(same_bits(a, b) for a, b in zip(got, want))


def test_grid_stride_over_four_times_the_resident_rows(gpu_device):
    """150,000 rows of V 8 in bf16 (2.4 MB): a launch keeps at most 256 CUs x 32 waves x 4 rows =
    32,768 rows resident, so every workgroup walks several groups of rows.  A row's outputs do not
    depend on the batch: the launch over everything is compared bitwise with launches that fit the
    resident grid, and every row goes against the checks."""
    B, K, V = 15000, 10, 8
    assert B * K >= 4 * 256 * 32 * 4
    l = randn4((B, K, V), torch.bfloat16, gpu_device, seed=5)
    u = uniforms(2, B, K, gpu_device, 5)
    for top_k, top_p in ((0, 1.0), (3, 0.9)):
        tok, lp, kept = sample(l, u, 1.0, top_k, top_p)
        check_rows(Rows(l), 1.0, top_k, top_p, [(u, tok, lp, kept)], "grid stride")
        for sl in (slice(None, None, 17), slice(0, 3), slice(B - 3, B)):
            part = sample(l[sl].contiguous(), u[:, sl].contiguous(), 1.0, top_k, top_p)
            assert same_bits(part[0], tok[:, sl]) and same_bits(part[1], lp[:, sl]) and same_bits(part[2], kept[sl])


# --------------------------------------------------------------- the Python surface --
def make_tok(dev, cls=BEASTBsplineTokenizer, **kw):
    tok = cls(num_dof=14, num_basis=10, seq_len=50, vocab_size=256, device=str(dev), **kw)
    gen = torch.Generator().manual_seed(9)
    tok.w_min.copy_(-1.0 - torch.rand(140, generator=gen))
    tok.w_max.copy_(1.0 + torch.rand(140, generator=gen))
    return tok


def test_uniforms_pass_through_to_the_raw_call(gpu_device):
    """[B, N, D, V] and full-vocabulary inputs with the LLM offset, ``uniforms`` in every accepted
    form, ``return_log_probs`` and ``num_samples``: the raw call's outputs, bit for bit."""
    tok = make_tok(gpu_device)
    tok.set_llm_vocab_size(1000)
    full = randn4((3, 140, 1000), torch.bfloat16, gpu_device, seed=8)
    full[..., :744] += 50.0                                  # everything outside the slice is larger
    action = full[..., 744:]
    u = uniforms(4, 3, 140, gpu_device, 8)
    want_tok, want_lp, _ = sample(action, u, 0.8, 20, 0.95, off=744)
    got = tok.sample_tokens_from_logits(full, temperature=0.8, top_k=20, top_p=0.95, num_samples=4, uniforms=u,
                                        return_log_probs=True)
    assert isinstance(got, tuple) and same_bits(got[0], want_tok) and same_bits(got[1], want_lp)
    assert got[0].shape == (4, 3, 140) and got[0].dtype == torch.int64 and got[1].dtype == torch.float32
    assert bool(((got[0] >= 744) & (got[0] < 1000)).all())
    for form in (full.reshape(3, 10, 14, 1000), action, action.contiguous(), full.cpu()):
        again = tok.sample_tokens_from_logits(form, temperature=0.8, top_k=20, top_p=0.95, num_samples=4, uniforms=u)
        assert same_bits(again, want_tok)
    plain = tok.sample_tokens_from_logits(full, temperature=0.8, top_k=20, top_p=0.95, num_samples=4,
                                          uniforms=u.double().cpu().reshape(4, 3, 10, 14), respect_llm_vocab_size=False)
    assert same_bits(plain, want_tok - 744)
    # without num_samples: [B, N*D], from uniforms [B, N*D], [B, N, D] or [1, B, N*D]
    for form in (u[1], u[1].reshape(3, 10, 14), u[1:2]):
        one, lp = tok.sample_tokens_from_logits(full, temperature=0.8, top_k=20, top_p=0.95, uniforms=form,
                                                return_log_probs=True)
        assert same_bits(one, want_tok[1]) and same_bits(lp, want_lp[1])
    # None / 0 / 1.0 switch the truncations off; float64 logits are cast
    off_tok = sample(action, u[:1], 1.0, 0, 1.0, off=744)[0][0]
    assert same_bits(tok.sample_tokens_from_logits(full, uniforms=u[0]), off_tok)
    assert same_bits(tok.sample_tokens_from_logits(full, top_k=0, top_p=1.0, uniforms=u[0]), off_tok)
    assert same_bits(tok.sample_tokens_from_logits(full.double(), uniforms=u[0]),
                     sample(action.float(), u[:1], 1.0, 0, 1.0, off=744)[0][0])
    x = full.clone().requires_grad_(True)
    assert not tok.sample_tokens_from_logits(x, uniforms=u[0]).requires_grad
    assert tok.sample_tokens_from_logits(full[:0]).shape == (0, 140)
    assert tok.sample_tokens_from_logits(full[:0], num_samples=3, return_log_probs=True)[1].shape == (3, 0, 140)
    bpe = make_tok(gpu_device, cls=BEASTBsplineBPETokenizer)
    bpe.set_llm_vocab_size(1000)
    assert same_bits(bpe.sample_tokens_from_logits(full, uniforms=u[0]), off_tok)


def test_generator_seeds_reproduce_and_tokens_round_trip(gpu_device):
    tok = make_tok(gpu_device)
    l = randn4((5, 10, 14, 256), torch.float32, gpu_device, seed=3)
    gen = torch.Generator(gpu_device)
    draws = []
    for seed in (7, 7, 8):
        gen.manual_seed(seed)
        draws.append(tok.sample_tokens_from_logits(l, temperature=1.5, num_samples=6, generator=gen, return_log_probs=True))
    assert same_bits(draws[0][0], draws[1][0]) and same_bits(draws[0][1], draws[1][1])
    assert not torch.equal(draws[0][0], draws[2][0])
    gen.manual_seed(7)
    u = torch.rand((6, 5, 140), device=gpu_device, generator=gen)        # what the method draws
    assert same_bits(tok.sample_tokens_from_logits(l, temperature=1.5, num_samples=6, uniforms=u), draws[0][0])
    a, b = tok.sample_tokens_from_logits(l), tok.sample_tokens_from_logits(l)     # the global generator moves on
    assert a.shape == (5, 140) and not torch.equal(a, b)
    # the tokens are MP tokens: reconstruct_traj takes them unchanged, draw by draw
    check_rows(Rows(l.reshape(5, 140, 256)), 1.5, 0, 1.0,
               [(u, draws[0][0], draws[0][1], torch.full((5, 140), 256, dtype=torch.int32))], "generator")
    traj = tok.reconstruct_traj(draws[0][0][2])
    assert traj.shape == (5, 50, 14) and bool(torch.isfinite(traj).all())
    greedy = tok.sample_tokens_from_logits(l, top_k=1)
    assert torch.equal(greedy, tok.greedy_tokens_from_logits(l))
    assert same_bits(tok.reconstruct_traj(greedy), tok.reconstruct_traj(tok.greedy_tokens_from_logits(l)))
