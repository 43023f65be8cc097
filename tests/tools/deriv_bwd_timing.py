"""Time the fused reconstruct backward against what a user could write without it.

At the default shape (T 50, D 14, N 10, degree 4), all three orders, B = 4,096 and 262,144:
  (a) one beast_reconstruct_derivs_bwd_f32 launch: gradients of pos, vel, acc -> grad_ntokens;
  (b) the ATen composition of the same gradient: one einsum per order of that order's slab with
      its gradient, their sum times s = (w_max - w_min) / 2, the clamp mask, and the
      (d n) -> (n d) permute into a contiguous result;
  (c) the forward, one beast_reconstruct_derivs_f32 launch from normalised tokens: the same
      bytes in the opposite direction.

HIP events around windows of back-to-back calls (each window at least ``--window-ms`` of work),
after a warm-up of every variant; the variants alternate inside each repeat and the median over
the repeats is reported with the minimum and maximum (the run's spread).  The buffers rotate
over enough copies that the working set exceeds twice the 256 MB of last-level cache, so every
call reads its gradients from HBM.  (a)'s share of the 8 TB/s HBM peak is its algorithmic bytes
(three gradients + ntokens read, grad_ntokens written) over its time.  The gate: (a)'s slowest
repeat is faster than (b)'s fastest at every batch size (``gate_a_below_b``).

    python tests/tools/deriv_bwd_timing.py [--out FILE.json]

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
from beast_tokenizer_amd import _lib  # noqa: E402
from beast_tokenizer_amd.bspline import DeviceBasis  # noqa: E402

T, D, N, DEGREE = 50, 14, 10, 4
HBM_PEAK = 8.0e12
CACHE_BYTES = 256 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[4096, 262144])
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--window-ms", type=float, default=30.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("deriv_bwd_timing.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    stream = _lib.stream_of(dev)
    basis = DeviceBasis(N, DEGREE, 2 * torch.pi, False)
    slabs = basis.deriv_constants(torch.linspace(0, 2 * torch.pi, T, device=dev))      # [3][2][T][N]
    g = torch.Generator(device=dev).manual_seed(0)
    w_min = -torch.rand((D * N,), device=dev, generator=g) - 0.5
    w_max = torch.rand((D * N,), device=dev, generator=g) + 0.5
    scale = (0.5 * (w_max - w_min)).reshape(D, N)
    dst = torch.arange(D, dtype=torch.int32, device=dev)
    joint = [slabs[o, 0].contiguous() for o in range(3)]                               # [T][N] per order
    results = []
    for B in args.batches:
        per_set = B * (3 * T * D * 4 + 2 * N * D * 4)
        n_sets = max(1, -(-2 * CACHE_BYTES // per_set))
        ntok = [torch.rand((B, N * D), device=dev, generator=g) * 2.2 - 1.1 for _ in range(n_sets)]
        grads = [[torch.randn((B, T, D), device=dev, generator=g) for _ in range(3)] for _ in range(n_sets)]
        gout = [torch.empty((B, N * D), device=dev) for _ in range(n_sets)]
        outs = [[torch.empty((B, T, D), device=dev) for _ in range(3)] for _ in range(n_sets)]   # the forward's

        def fused(i):
            gr = grads[i]
            _lib.check(lib.beast_reconstruct_derivs_bwd_f32(
                gr[0].data_ptr(), gr[1].data_ptr(), gr[2].data_ptr(), B, D, D, N, w_min.data_ptr(), w_max.data_ptr(),
                slabs.data_ptr(), 0, T, dst.data_ptr(), D, ntok[i].data_ptr(), None, gout[i].data_ptr(), None, 0,
                stream), "beast_reconstruct_derivs_bwd_f32")

        def aten(i):
            gr, x = grads[i], ntok[i].view(B, N, D)
            s = torch.einsum("tn,btd->bdn", joint[0], gr[0])
            s = s + torch.einsum("tn,btd->bdn", joint[1], gr[1])
            s = s + torch.einsum("tn,btd->bdn", joint[2], gr[2])
            s = (s * scale).permute(0, 2, 1)
            gout[i].view(B, N, D).copy_(torch.where((x >= -1) & (x <= 1), s, 0.0))

        def forward(i):
            o = outs[i]
            _lib.check(lib.beast_reconstruct_derivs_f32(
                None, B, D, D, N, 256, 0, w_min.data_ptr(), w_max.data_ptr(), slabs.data_ptr(), 0, T, dst.data_ptr(),
                D, None, 0, None, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), ntok[i].data_ptr(), stream),
                "beast_reconstruct_derivs_f32")

        # the two backward paths agree before anything is timed
        fused(0)
        a = gout[0].clone()
        aten(0)
        err = float((a - gout[0]).abs().max() / gout[0].abs().max())
        if not err < 1e-4:
            raise SystemExit(f"fused and ATen backward disagree at B={B}: relative error {err}")

        variants = {"fused_backward": fused, "aten_backward": aten, "forward_3_orders": forward}
        order = list(variants)

        def window(name, n_calls):
            fn = variants[name]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(n_calls):
                fn(k % n_sets)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / n_calls            # us per call

        calls = {}
        for name in order:                                         # warm-up, and size the windows
            window(name, 3)
            us = window(name, max(3, n_sets))
            calls[name] = max(n_sets, int(args.window_ms * 1e3 / us) + 1)
        samples = {name: [] for name in order}
        for _ in range(args.repeats):
            for name in order:
                samples[name].append(window(name, calls[name]))
        row = {"B": B, "buffer_sets": n_sets, "calls_per_window": calls, "fused_vs_aten_rel_err": err}
        for name, v in samples.items():
            row[name + "_us"] = round(statistics.median(v), 3)
            row[name + "_us_min_max"] = [round(min(v), 3), round(max(v), 3)]
        algo_bytes = B * (3 * T * D * 4 + 2 * N * D * 4)
        row["fused_algorithmic_bytes"] = algo_bytes
        row["fused_hbm_fraction_of_8TBps"] = round(algo_bytes / (row["fused_backward_us"] * 1e-6) / HBM_PEAK, 4)
        row["fused_over_forward"] = round(row["fused_backward_us"] / row["forward_3_orders_us"], 3)
        row["aten_over_fused"] = round(row["aten_backward_us"] / row["fused_backward_us"], 3)
        row["gate_a_below_b"] = max(samples["fused_backward"]) < min(samples["aten_backward"])
        results.append(row)
        del ntok, grads, gout, outs
        torch.cuda.empty_cache()
    line = json.dumps({"tool": "deriv_bwd_timing", "shape": {"T": T, "D": D, "N": N, "degree": DEGREE},
                       "device": torch.cuda.get_device_name(0), "results": results,
                       "gate_a_below_b": all(r["gate_a_below_b"] for r in results)})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not all(r["gate_a_below_b"] for r in results):
        raise SystemExit("gate failed: the fused backward is not below the ATen composition by more than the spread")


if __name__ == "__main__":
    main()
