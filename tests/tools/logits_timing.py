"""Time the fused logits decode against what a user could write without it.

At the default shape (K 140 = N 10 x D 14 tokens, V 256), B = 256 and 4,096, fp32 and bf16:
  (a) one beast_logits_expect launch: logits -> mean and the row statistics;
  (b) the ATen composition of the same value: (softmax(l / tau, -1) * x).sum(-1);
  (c) one beast_logits_expect_bwd launch: logits, mean, stats, grad_mean -> grad_logits;
  (d) the ATen backward of (b): torch.autograd.grad through the graph (b) recorded, kept alive
      with retain_graph, so only the backward's own kernels are in the window.

HIP events around windows of back-to-back calls (each window at least ``--window-ms`` of work),
after a warm-up of every variant; the variants alternate inside each repeat and the median over
the repeats is reported with the minimum and maximum (the run's spread).  The buffers rotate
over enough copies that the working set exceeds twice the 256 MB of last-level cache, so every
call reads its logits from HBM.  A fused kernel's share of the 8 TB/s HBM peak is its
algorithmic bytes over its time: the logits read plus the per-row outputs (forward), the logits
read and the gradient written plus the per-row inputs (backward).  The gate: each fused variant's
slowest repeat is faster than its ATen counterpart's fastest at every batch size and dtype
(``gate_fused_below_aten``).

``--rows R`` sets BEAST_DEBUG_LOGITS_ROWS (rows a wave works on at once: 1, 2 or 4) before the
library is loaded: the measurement behind the default.

    python tests/tools/logits_timing.py [--rows R] [--out FILE.json]

Needs a GPU; prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

K, V, TAU = 140, 256, 0.8
HBM_PEAK = 8.0e12
CACHE_BYTES = 256 << 20
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--dtypes", nargs="+", default=list(DTYPES), choices=list(DTYPES))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--window-ms", type=float, default=30.0)
    ap.add_argument("--rows", type=int, default=None, choices=[1, 2, 4])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.rows is not None:
        os.environ["BEAST_DEBUG_LOGITS_ROWS"] = str(args.rows)
    from beast_tokenizer_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("logits_timing.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    stream = _lib.stream_of(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    x = (2.0 * torch.arange(V, device=dev, dtype=torch.float64) / (V - 1) - 1.0).to(torch.float32)
    results = []
    for name, dt in ((n, DTYPES[n]) for n in args.dtypes):
        code, size = _lib.LOGITS_DTYPES[dt], torch.empty((), dtype=dt).element_size()
        for B in args.batches:
            per_set = B * K * V * size
            n_sets = max(1, -(-2 * CACHE_BYTES // per_set))
            logits = [(torch.randn((B, K, V), device=dev, generator=gen) * 4.0).to(dt).requires_grad_()
                      for _ in range(n_sets)]
            gm = [torch.randn((B, K), device=dev, generator=gen) for _ in range(n_sets)]
            mean = [torch.empty((B, K), device=dev) for _ in range(n_sets)]
            stats = [torch.empty((B, K, 2), device=dev) for _ in range(n_sets)]
            grad = [torch.empty((B, K, V), dtype=dt, device=dev) for _ in range(n_sets)]
            graph = [(torch.softmax(l / TAU, -1) * x).sum(-1) for l in logits]      # (b) recorded once, for (d)

            def fused_forward(i):
                _lib.check(lib.beast_logits_expect(logits[i].data_ptr(), code, B, K, V, K * V, V, TAU, 0,
                                                   mean[i].data_ptr(), None, stats[i].data_ptr(), stream),
                           "beast_logits_expect")

            def aten_forward(i):
                with torch.no_grad():
                    return (torch.softmax(logits[i] / TAU, -1) * x).sum(-1)

            def fused_backward(i):
                _lib.check(lib.beast_logits_expect_bwd(logits[i].data_ptr(), code, B, K, V, K * V, V, TAU,
                                                       mean[i].data_ptr(), stats[i].data_ptr(), gm[i].data_ptr(),
                                                       grad[i].data_ptr(), K * V, V, stream),
                           "beast_logits_expect_bwd")

            def aten_backward(i):
                return torch.autograd.grad(graph[i], logits[i], gm[i].to(graph[i].dtype), retain_graph=True)[0]

            # the two paths agree before anything is timed
            for i in range(n_sets):
                fused_forward(i)
            fused_backward(0)
            err_f = float((mean[0] - aten_forward(0).float()).abs().max())
            ref = aten_backward(0).float()
            err_b = float((grad[0].float() - ref).abs().max() / ref.abs().max())
            # a guard against timing two different things, not an accuracy test: ATen's bf16 softmax
            # rounds every probability to 8 bits
            if not (err_f < (1e-5 if dt is torch.float32 else 1e-1) and err_b < (1e-4 if dt is torch.float32 else 1e-1)):
                raise SystemExit(f"fused and ATen disagree at B={B} {name}: forward {err_f}, backward {err_b}")

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
            row = {"B": B, "dtype": name, "buffer_sets": n_sets, "calls_per_window": calls,
                   "forward_abs_err_vs_aten": err_f, "backward_rel_err_vs_aten": err_b}
            for vname, v in samples.items():
                row[vname + "_us"] = round(statistics.median(v), 3)
                row[vname + "_us_min_max"] = [round(min(v), 3), round(max(v), 3)]
            fwd_bytes = per_set + B * K * 3 * 4                        # logits + mean + stats
            bwd_bytes = 2 * per_set + B * K * 4 * 4                    # logits + grad + mean, stats, grad_mean
            row["forward_algorithmic_bytes"], row["backward_algorithmic_bytes"] = fwd_bytes, bwd_bytes
            row["forward_hbm_fraction_of_8TBps"] = round(fwd_bytes / (row["fused_forward_us"] * 1e-6) / HBM_PEAK, 4)
            row["backward_hbm_fraction_of_8TBps"] = round(bwd_bytes / (row["fused_backward_us"] * 1e-6) / HBM_PEAK, 4)
            row["aten_over_fused_forward"] = round(row["aten_forward_us"] / row["fused_forward_us"], 3)
            row["aten_over_fused_backward"] = round(row["aten_backward_us"] / row["fused_backward_us"], 3)
            row["gate_fused_below_aten"] = (max(samples["fused_forward"]) < min(samples["aten_forward"])
                                            and max(samples["fused_backward"]) < min(samples["aten_backward"]))
            results.append(row)
            del logits, gm, mean, stats, grad, graph
            torch.cuda.empty_cache()
    gate = all(r["gate_fused_below_aten"] for r in results)
    line = json.dumps({"tool": "logits_timing", "shape": {"K": K, "V": V, "temperature": TAU},
                       "rows_per_wave": args.rows or "default", "device": torch.cuda.get_device_name(0),
                       "results": results, "gate_fused_below_aten": gate})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not gate:
        raise SystemExit("gate failed: a fused logits kernel is not below its ATen composition by more than the spread")


if __name__ == "__main__":
    main()
