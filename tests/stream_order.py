"""The ordering probe of the tests/test_gpu_*stream_order.py modules: does a call do ALL its device
work, in order, on the stream it is given?  Below the probe, what those modules share: the case
registries, the two test bodies, the canary, the fault guard and the logits-family helpers.

A case names the buffers a call reads (each with a ``good`` and a ``stale`` content of the same shape),
the buffers it writes or uses as scratch, and the call itself.  ``probe`` then

1. puts ``stale`` into the inputs on the null stream and synchronises the device;
2. computes ``expected`` from ``good`` on the null stream, fully synchronised (the case's
   ``check_expected`` ties it to an oracle), timing the host side of the call;
3. runs the call on ``stale`` too: a case whose result cannot tell the two apart proves nothing;
4. on a fresh side stream ``s`` that demonstrably runs beside the null stream (``side_stream``: two
   streams that share a hardware queue run in submission order), with no host synchronisation
   anywhere, enqueues: a delay, a poison fill of every output / scratch buffer (NaN
   for floats, 0xFF bytes otherwise), the caller's own preparation (``setup``: zero fills the entry
   point leaves to the caller), the copy of ``good`` over the inputs, the call, a snapshot of the
   results;
5. records ``busy = not s.query()`` right after the call returned;
6. synchronises ``s`` alone and compares the snapshot with ``expected``.

A kernel or copy the call issued on another stream ran before the delay was over: it read ``stale``,
or its output was poisoned afterwards.  An internal memset on another stream ran early too: the
poison fill then overwrote it.  ``busy`` shows that the delay was still running when the call
returned, so "early" really was early; a delay that is too short is a loud failure.

Nothing here can fault: stale contents are valid inputs (zeros, reversed rows, in-range ids; offset
and index tables are never stale), and poison goes only into buffers the entry point documents as
outputs or scratch.
"""
from __future__ import annotations

import functools
import time
from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import pytest
import torch

from beast_tokenizer_amd import BEASTBsplineTokenizer, _lib

MIN_DELAY_MS = 10.0     # the delay of a case: max(MIN_DELAY_MS, HOST_FACTOR * host time of the call) ...
HOST_FACTOR = 20.0      # ... the factor is headroom for host jitter
MAX_DELAY_MS = 99.0     # no single delay reaches 100 ms

# what the probe learned about the machine (the canary fixture prints it when a module ends)
MEASURED = {"cycles_per_ms": None, "max_host_ms": 0.0, "max_host_case": None, "max_delay_ms": 0.0}


def cycles_per_ms(dev: torch.device) -> float:
    """``torch.cuda._sleep`` cycles per millisecond, measured once with two events."""
    if MEASURED["cycles_per_ms"] is not None:
        return MEASURED["cycles_per_ms"]
    with torch.cuda.device(dev):
        torch.cuda._sleep(1000)          # loads the kernel
        torch.cuda.synchronize(dev)
        cycles = 1_000_000
        for _ in range(8):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch.cuda._sleep(cycles)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            if ms >= 4.0:                # a launch's few microseconds are below 1 % of it
                MEASURED["cycles_per_ms"] = cycles / ms
                return MEASURED["cycles_per_ms"]
            cycles = int(cycles * min(64.0, max(2.0, 8.0 / max(ms, 0.01))))
    raise AssertionError("torch.cuda._sleep could not be calibrated: no sleep reached 4 ms")


def sleep_ms(ms: float, dev: torch.device) -> None:
    """Enqueue a delay of ``ms`` on the current stream."""
    torch.cuda._sleep(int(cycles_per_ms(dev) * ms))


def runs_beside(blocker: torch.cuda.Stream, other: torch.cuda.Stream, dev: torch.device) -> bool:
    """Does work on ``other`` run while ``blocker`` is held up?  Streams are software objects: the
    runtime maps them onto a few hardware queues (four by default), and two streams that share a
    queue run in submission order whatever their flags say -- a mis-ordered call would then look
    ordered.  A 3 ms delay goes on ``blocker``, a one-element fill and an event on ``other``; the
    event must complete while the delay is still running."""
    cell = torch.zeros(1, device=dev)
    ev = torch.cuda.Event()
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(blocker):
        sleep_ms(3.0, dev)
    with torch.cuda.stream(other):
        cell.fill_(1.0)
        ev.record()
    t0 = time.perf_counter()
    while not ev.query() and time.perf_counter() - t0 < 2e-3:
        pass
    beside = ev.query() and not blocker.query()
    torch.cuda.synchronize(dev)
    return beside


def side_stream(dev: torch.device, beside=()) -> torch.cuda.Stream:
    """A fresh stream on which a delay holds up none of ``beside`` (default: the null stream).  torch
    hands out its pool's streams in turn, so the next candidate sits on another hardware queue; this
    chooses where the probe runs, it never repeats a probe."""
    others = list(beside) or [torch.cuda.default_stream(dev)]
    for _ in range(16):
        s = torch.cuda.Stream(device=dev)
        if all(runs_beside(s, o, dev) for o in others):
            return s
    raise AssertionError("no side stream runs independently of the null stream on this device: "
                         "the ordering probe cannot see a mis-ordering here")


def poison_(t: torch.Tensor) -> None:
    """NaN for floats, 0xFF bytes otherwise (on the current stream)."""
    if t.numel() == 0:
        return
    if t.dtype.is_floating_point:
        t.fill_(float("nan"))
    elif t.dtype is torch.uint8:
        t.fill_(255)
    else:
        t.fill_(-1)                       # two's complement: every byte 0xFF


def bits(t: torch.Tensor) -> torch.Tensor:
    """The tensor's bytes, so that NaN compares equal to the same NaN."""
    return t.contiguous().reshape(-1).view(torch.uint8)


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


@dataclass
class Case:
    """One probed call.  ``call(stream_handle)`` enqueues the entry point(s) on that raw stream and
    returns the tensors that hold its results; ``inputs`` are (buffer the call reads, good, stale);
    ``scratch`` every output and workspace buffer (poisoned); ``setup`` what the entry point leaves
    to the caller (zero fills), as torch ops on the current stream; ``canon`` brings results whose
    order is unspecified into a comparable form (host side, after the synchronisation);
    ``check_expected`` compares the canonical ``expected`` with an oracle; ``equal`` compares one
    result tensor (default: bitwise)."""
    name: str
    entries: Tuple[str, ...]
    inputs: List[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]]
    call: Callable[[int], Sequence[torch.Tensor]]
    scratch: List[torch.Tensor] = field(default_factory=list)
    setup: Optional[Callable[[], None]] = None
    canon: Optional[Callable[[List[torch.Tensor]], List[torch.Tensor]]] = None
    check_expected: Optional[Callable[[List[torch.Tensor]], None]] = None
    equal: Callable[[torch.Tensor, torch.Tensor], bool] = bits_equal
    synchronous: bool = False          # the entry point synchronises the host inside: no ``busy``


@dataclass
class Report:
    name: str
    busy: bool
    mismatch: List[int]                 # indices of the result tensors that differ from expected
    host_ms: float
    delay_ms: float
    expected: List[torch.Tensor]
    snapshot: List[torch.Tensor]

    @property
    def ordered(self) -> bool:
        return not self.mismatch


def _prepare(case: Case, which: int) -> None:
    """poison, the caller's preparation, the inputs (1: good, 2: stale), on the current stream."""
    for t in case.scratch:
        poison_(t)
    if case.setup is not None:
        case.setup()
    for item in case.inputs:
        item[0].copy_(item[which])


def _canon(case: Case, res: Sequence[torch.Tensor]) -> List[torch.Tensor]:
    res = [r.clone() for r in res]
    return list(case.canon(res)) if case.canon is not None else res


def probe(case: Case, dev: torch.device, api: bool = False) -> Report:
    """Run the probe.  ``api`` False: the C-ABI form -- the call gets ``s``'s handle while torch's
    current stream is the null stream.  ``api`` True: the call runs under ``torch.cuda.stream(s)``
    (and gets the same handle), for Python entry points that ask torch for the current stream."""
    null = torch.cuda.default_stream(dev)
    assert torch.cuda.current_stream(dev) == null, "the probe starts from the null stream"
    rate = cycles_per_ms(dev)
    # 1. stale inputs, everywhere
    for buf, _, stale in case.inputs:
        buf.copy_(stale)
    torch.cuda.synchronize(dev)
    # 2. expected, on the null stream; the first call loads the kernels, the second is timed
    host_ms = 0.0
    for _ in range(2):
        _prepare(case, 1)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        res = case.call(null.cuda_stream)
        host_ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize(dev)
    raw_expected = [r.clone() for r in res]
    expected = _canon(case, res)
    if case.check_expected is not None:
        case.check_expected(expected)
    # 3. the case must be able to see a mis-ordering
    if case.inputs:
        _prepare(case, 2)
        torch.cuda.synchronize(dev)
        stale_res = _canon(case, case.call(null.cuda_stream))
        torch.cuda.synchronize(dev)
        assert len(stale_res) == len(expected)
        assert any(not case.equal(e, g) for e, g in zip(expected, stale_res)), \
            f"{case.name}: the result from the stale input equals the expected one; the case detects nothing"
    else:
        # a branch that reads no input (an early return after a memset): only the poison can show a
        # mis-ordering, so every result must differ from its poisoned state
        assert case.scratch, f"{case.name}: neither inputs nor poisoned outputs"
        for e in raw_expected:
            p = torch.empty_like(e)
            poison_(p)
            assert not bits_equal(e, p), f"{case.name}: the result equals the poison pattern; the case detects nothing"
    # the inputs hold ``stale`` again; 4. the probed sequence
    snap = [torch.empty_like(e) for e in raw_expected]
    delay_ms = min(max(MIN_DELAY_MS, HOST_FACTOR * host_ms), MAX_DELAY_MS)
    if host_ms > MEASURED["max_host_ms"]:
        MEASURED["max_host_ms"], MEASURED["max_host_case"] = host_ms, case.name
    MEASURED["max_delay_ms"] = max(MEASURED["max_delay_ms"], delay_ms)
    s = side_stream(dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(s):
        torch.cuda._sleep(int(rate * delay_ms))
        _prepare(case, 1)
        if api:
            res = case.call(s.cuda_stream)
            busy = not s.query()
    if not api:
        assert torch.cuda.current_stream(dev) == null
        res = case.call(s.cuda_stream)
        busy = not s.query()
    with torch.cuda.stream(s):
        for d, r in zip(snap, res):
            d.copy_(r)
    # 6. this stream alone
    s.synchronize()
    got = list(case.canon([t.clone() for t in snap])) if case.canon is not None else snap
    mismatch = [i for i, (e, g) in enumerate(zip(expected, got)) if not case.equal(e, g)]
    torch.cuda.synchronize(dev)          # leave nothing in flight for the next test
    return Report(case.name, busy, mismatch, host_ms, delay_ms, expected, got)


def assert_ordered(case: Case, dev: torch.device, api: bool = False) -> Report:
    r = probe(case, dev, api)
    if not case.synchronous:
        assert r.busy, (f"{case.name}: the stream was idle when the call returned (host {r.host_ms:.3f} ms, delay "
                        f"{r.delay_ms:.1f} ms): the delay rule is too short, or the call synchronises inside")
    assert r.ordered, (f"{case.name}: result tensors {r.mismatch} differ from the null-stream result: part of the "
                       f"call did not run in order on the stream it was given ({case.entries})")
    return r


# ------------------------------------------------------------------- registries --
CASES = {}        # section A: id -> (registering module, entry points, builder(dev) -> Case)
API_CASES = {}    # section B: id -> (registering module, builder(dev) -> Case)


def capi(cid, *entries):
    def deco(fn):
        assert cid not in CASES
        CASES[cid] = (fn.__module__, entries, fn)
        return fn
    return deco


def api(cid):
    def deco(fn):
        assert cid not in API_CASES
        API_CASES[cid] = (fn.__module__, fn)
        return fn
    return deco


def ids(registry, module):
    """The ids that ``module`` registered: a module parametrises its tests over its own cases."""
    return sorted(cid for cid, item in registry.items() if item[0] == module)


# ------------------------------------------------------------------ fault guard --
_FAULT = []       # the message of a HIP error met in this process: nothing more is started after one


def stops_after_a_fault(fn):
    """A HIP fault is sticky: once a HIP error has been seen in any stream-order test, every later one,
    in any module, fails at once instead of launching more work on a faulted device."""
    @functools.wraps(fn)
    def wrapper(*args, **kw):
        if _FAULT:
            pytest.fail(f"not run: a HIP error was met earlier in a stream-order test ({_FAULT[0][:200]})")
        try:
            return fn(*args, **kw)
        except (RuntimeError, _lib.BeastError) as e:
            if "HIP error" in str(e) or "illegal memory access" in str(e) or "hipError" in str(e):
                _FAULT.append(str(e))
            raise
    return wrapper


# ------------------------------------------------------------------ test bodies --
@stops_after_a_fault
def check_capi(cid, dev):
    """Section A: the entry point gets the side stream's handle while torch's current stream is the
    null stream, so any internal use of the current stream or of stream 0 shows."""
    _, entries, build = CASES[cid]
    case = build(dev)
    case.entries = entries
    assert_ordered(case, dev)


@stops_after_a_fault
def check_api(cid, dev):
    """Section B: the same probe with ``s`` current: _lib.stream_of / raw_stream, the C++ fast path's
    stream query and the handles captured at construction all have to resolve to ``s``."""
    assert_ordered(API_CASES[cid][1](dev), dev, api=True)


# ----------------------------------------------------------------------- canary --
@stops_after_a_fault
def canary_report(dev):
    """The probe on a deliberately mis-ordered torch-only call: ``out.copy_(inp)`` issued on the
    null stream whatever stream it is given."""
    good = torch.arange(1, 4097, dtype=torch.float32, device=dev)
    stale = torch.zeros_like(good)
    inp, out = torch.empty_like(good), torch.empty_like(good)
    null = torch.cuda.default_stream(dev)

    def call(_handle):
        with torch.cuda.stream(null):
            out.copy_(inp)
        return [out]
    return probe(Case("canary", ("torch copy on the null stream",), [(inp, good, stale)], call, scratch=[out]), dev)


_CANARY = {}      # "report": computed once per process; "printed": the figures last printed


@pytest.fixture(scope="module", autouse=True)
def canary(gpu_device):
    """Every test of a stream-order module needs the canary: if the probe calls a mis-ordered copy
    "ordered" (a side stream that blocks on the null stream, say), no other result means anything,
    so all fail.  Each module imports this fixture; the report is shared."""
    if "report" not in _CANARY:
        _CANARY["report"] = canary_report(gpu_device)
    r = _CANARY["report"]
    if not (r.busy and r.mismatch):
        pytest.fail(f"canary: a copy on the null stream was reported as ordered on the side stream "
                    f"(busy={r.busy}, mismatch={r.mismatch}): the probe cannot see a mis-ordering here")
    yield r
    m = MEASURED
    if _CANARY.get("printed") != m:       # a module that raised no figure repeats no line
        _CANARY["printed"] = dict(m)
        print(f"\nstream-order probe: {m['cycles_per_ms']:.0f} sleep cycles/ms; largest host time "
              f"{m['max_host_ms']:.3f} ms ({m['max_host_case']}); largest delay {m['max_delay_ms']:.1f} ms")


# --------------------------------------------- the logits family's case helpers --
FLOOR = 16 * 2.0 ** -24


def logits(shape, dtype, dev, seed):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=gen) * 4.0).to(dtype).to(dev)


def f64(t):
    return t.detach().to("cpu", torch.float64).numpy()


def close(got, want, rel=0.0):
    fin = np.isfinite(want)
    assert np.array_equal(np.isneginf(want), np.isneginf(got))
    scale = max(1.0, float(np.abs(want[fin]).max()))
    assert np.all(np.abs(got[fin] - want[fin]) <= 4 * FLOOR * scale + rel * np.abs(want[fin]))


def api_tok(dev, init=None):
    """A default-shaped tokenizer whose plan is built and complete; ``init(tok)`` runs before the plan."""
    tok = BEASTBsplineTokenizer(num_dof=14, num_basis=10, seq_len=50, vocab_size=256, device=str(dev))
    if init is not None:
        init(tok)
    tok._plan()
    torch.cuda.synchronize(dev)
    return tok


def api_case(name, good, fn, check=None):
    x = torch.empty_like(good)
    return Case(name, (name,), [(x, good, good.flip(0).contiguous())], lambda h: fn(x), check_expected=check)
