"""Time the fused cross-entropy against what a user could write without it.

At the default shape (K 140 = N 10 x D 14 tokens, V 256), B = 256 and 4,096, fp32 and bf16, token
and coefficient (two-hot) targets, label smoothing 0 and 0.1:
  (a) one beast_xent_rows launch: logits, target -> loss and the row statistics;
  (b) the ATen composition: F.cross_entropy(l.view(-1, V), t.view(-1), reduction="none",
      label_smoothing=eps), for the two-hot case with a dense soft target [B*K, V] built beforehand
      (its construction is not in the window);
  (c) one beast_xent_rows_bwd launch: logits, target, stats, grad_loss -> grad_logits;
  (d) the ATen backward of (b): torch.autograd.grad through the graph (b) recorded, kept alive
      with retain_graph, so only the backward's own kernels are in the window.

The protocol is tests/tools/logits_timing.py's: HIP events around windows of back-to-back calls (each
window at least ``--window-ms`` of work), after a warm-up of every variant; the variants alternate
inside each repeat and the median over the repeats is reported with the minimum and maximum.  The
buffers rotate over enough copies that the working set exceeds twice the 256 MB of last-level
cache.  A fused kernel's share of the 8 TB/s HBM peak is its algorithmic bytes over its time: the
logits read plus the per-row target, loss and statistics (forward); the logits read and the gradient
written plus the per-row target, statistics and upstream gradient (backward).  The gate: each fused
variant's slowest repeat is faster than its ATen counterpart's fastest, everywhere
(``gate_fused_below_aten``).

Peak extra memory: ``torch.cuda.max_memory_allocated`` over one forward and backward from a leaf that
requires a gradient, above what was allocated before, through ``cross_entropy_from_logits`` and
through the composition.

    python tests/tools/xent_timing.py [--out FILE.json]

Needs a GPU; prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

K, V = 140, 256
HBM_PEAK = 8.0e12
CACHE_BYTES = 256 << 20
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def two_hot(x, dtype):
    """The dense two-hot target [B, K, V] of coefficients x [B, K] (unsmoothed: F.cross_entropy smooths)."""
    u = (((x + 1.0) * 0.5) * (V - 1)).clamp(0.0, float(V - 1))
    i = u.floor().clamp(max=V - 2)
    f = u - i
    q = torch.zeros((*x.shape, V), device=x.device)
    q.scatter_(-1, i.long()[..., None], (1.0 - f)[..., None])
    q.scatter_add_(-1, i.long()[..., None] + 1, f[..., None])
    return q.to(dtype)


def peak_extra(fn, dev):
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize(dev)
    return torch.cuda.max_memory_allocated(dev) - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--dtypes", nargs="+", default=list(DTYPES), choices=list(DTYPES))
    ap.add_argument("--targets", nargs="+", default=["tokens", "coefficients"], choices=["tokens", "coefficients"])
    ap.add_argument("--smoothing", type=float, nargs="+", default=[0.0, 0.1])
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--window-ms", type=float, default=30.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from beast_tokenizer_amd import BEASTBsplineTokenizer, _lib
    if not torch.cuda.is_available():
        raise SystemExit("xent_timing.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    stream = _lib.stream_of(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    tok = BEASTBsplineTokenizer(num_dof=14, num_basis=10, seq_len=50, vocab_size=V, device="cuda:0")
    results = []
    for name, dt in ((n, DTYPES[n]) for n in args.dtypes):
        code, size = _lib.LOGITS_DTYPES[dt], torch.empty((), dtype=dt).element_size()
        for B in args.batches:
            for kind in args.targets:
                for eps in args.smoothing:
                    per_set = B * K * V * size
                    n_sets = max(1, -(-2 * CACHE_BYTES // per_set))
                    logits = [(torch.randn((B, K, V), device=dev, generator=gen) * 4.0).to(dt).requires_grad_()
                              for _ in range(n_sets)]
                    if kind == "tokens":
                        target = [torch.randint(0, V, (B, K), device=dev, generator=gen) for _ in range(n_sets)]
                        aten_target = [t.view(-1) for t in target]
                        tptr = [(t.data_ptr(), None) for t in target]
                    else:
                        target = [torch.rand((B, K), device=dev, generator=gen) * 2.0 - 1.0 for _ in range(n_sets)]
                        aten_target = [two_hot(t, dt).view(-1, V) for t in target]
                        tptr = [(None, t.data_ptr()) for t in target]
                    gl = [torch.randn((B, K), device=dev, generator=gen) for _ in range(n_sets)]
                    loss = [torch.empty((B, K), device=dev) for _ in range(n_sets)]
                    stats = [torch.empty((B, K, 2), device=dev) for _ in range(n_sets)]
                    grad = [torch.empty((B, K, V), dtype=dt, device=dev) for _ in range(n_sets)]

                    def aten(i):
                        return F.cross_entropy(logits[i].view(-1, V), aten_target[i], reduction="none",
                                               label_smoothing=eps)

                    graph = [aten(i) for i in range(n_sets)]                   # (b) recorded once, for (d)

                    def fused_forward(i):
                        _lib.check(lib.beast_xent_rows(logits[i].data_ptr(), code, B, K, V, K * V, V, *tptr[i], 0, -100,
                                                       eps, loss[i].data_ptr(), stats[i].data_ptr(), None, stream),
                                   "beast_xent_rows")

                    def aten_forward(i):
                        with torch.no_grad():
                            return aten(i)

                    def fused_backward(i):
                        _lib.check(lib.beast_xent_rows_bwd(logits[i].data_ptr(), code, B, K, V, K * V, V, *tptr[i], 0,
                                                           -100, eps, stats[i].data_ptr(), gl[i].data_ptr(),
                                                           grad[i].data_ptr(), K * V, V, stream),
                                   "beast_xent_rows_bwd")

                    def aten_backward(i):
                        return torch.autograd.grad(graph[i], logits[i], gl[i].view(-1).to(graph[i].dtype),
                                                   retain_graph=True)[0]

                    # the two paths agree before anything is timed
                    for i in range(n_sets):
                        fused_forward(i)
                    fused_backward(0)
                    ref_f = aten_forward(0).float().view(B, K)
                    err_f = float(((loss[0] - ref_f).abs() / ref_f.abs().clamp(min=1.0)).max())
                    ref = aten_backward(0).float()
                    err_b = float((grad[0].float() - ref).abs().max() / ref.abs().max())
                    # a guard against timing two different things, not an accuracy test: ATen's bf16
                    # log-softmax rounds every entry to 8 bits
                    lim = 1e-4 if dt is torch.float32 else 1e-1
                    if not (err_f < lim and err_b < lim):
                        raise SystemExit(f"fused and ATen disagree at B={B} {name} {kind} eps={eps}: "
                                         f"forward {err_f}, backward {err_b}")

                    variants = {"fused_forward": fused_forward, "aten_forward": aten_forward,
                                "fused_backward": fused_backward, "aten_backward": aten_backward}
                    order = list(variants)

                    def window(vname, n_calls):
                        fn = variants[vname]
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for k in range(n_calls):
                            fn(k % n_sets)
                        e1.record()
                        e1.synchronize()
                        return e0.elapsed_time(e1) * 1e3 / n_calls            # us per call

                    calls = {}
                    for vname in order:                                        # warm-up, and size the windows
                        window(vname, 3)
                        us = window(vname, max(3, n_sets))
                        calls[vname] = max(n_sets, int(args.window_ms * 1e3 / us) + 1)
                    samples = {vname: [] for vname in order}
                    for _ in range(args.repeats):
                        for vname in order:
                            samples[vname].append(window(vname, calls[vname]))
                    row = {"B": B, "dtype": name, "target": kind, "smoothing": eps, "buffer_sets": n_sets,
                           "calls_per_window": calls, "forward_rel_err_vs_aten": err_f,
                           "backward_rel_err_vs_aten": err_b}
                    for vname, v in samples.items():
                        row[vname + "_us"] = round(statistics.median(v), 3)
                        row[vname + "_us_min_max"] = [round(min(v), 3), round(max(v), 3)]
                    tbytes = 8 if kind == "tokens" else 4
                    fwd_bytes = per_set + B * K * (tbytes + 4 + 8)             # logits + target, loss, stats
                    bwd_bytes = 2 * per_set + B * K * (tbytes + 8 + 4)         # logits + grad + target, stats, g
                    row["forward_algorithmic_bytes"], row["backward_algorithmic_bytes"] = fwd_bytes, bwd_bytes
                    row["forward_hbm_fraction_of_8TBps"] = round(
                        fwd_bytes / (row["fused_forward_us"] * 1e-6) / HBM_PEAK, 4)
                    row["backward_hbm_fraction_of_8TBps"] = round(
                        bwd_bytes / (row["fused_backward_us"] * 1e-6) / HBM_PEAK, 4)
                    row["aten_over_fused_forward"] = round(row["aten_forward_us"] / row["fused_forward_us"], 3)
                    row["aten_over_fused_backward"] = round(row["aten_backward_us"] / row["fused_backward_us"], 3)
                    row["gate_fused_below_aten"] = (max(samples["fused_forward"]) < min(samples["aten_forward"])
                                                    and max(samples["fused_backward"]) < min(samples["aten_backward"]))
                    del graph, grad, loss, stats
                    torch.cuda.empty_cache()

                    # peak extra memory of one training step's loss, from a leaf
                    def fused_step():
                        leaf = logits[0].detach().requires_grad_()
                        tok.cross_entropy_from_logits(leaf, target[0], label_smoothing=eps).backward()

                    def aten_step():
                        leaf = logits[0].detach().requires_grad_()
                        F.cross_entropy(leaf.view(-1, V), aten_target[0], label_smoothing=eps).backward()

                    fused_step(), aten_step()
                    row["fused_peak_extra_bytes"] = peak_extra(fused_step, dev)
                    row["aten_peak_extra_bytes"] = peak_extra(aten_step, dev)
                    row["logits_bytes"] = per_set
                    results.append(row)
                    del logits, target, aten_target, gl, tptr
                    torch.cuda.empty_cache()
    gate = all(r["gate_fused_below_aten"] for r in results)
    line = json.dumps({"tool": "xent_timing", "shape": {"K": K, "V": V}, "device": torch.cuda.get_device_name(0),
                       "results": results, "gate_fused_below_aten": gate})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not gate:
        raise SystemExit("gate failed: a fused cross-entropy kernel is not below its ATen composition by more than "
                         "the spread")


if __name__ == "__main__":
    main()
