"""Time the fused multi-order reconstruct against what the existing kernels offer.

At the default shape (T 50, D 14, N 10, V 256, degree 4) and B = 4,096 and 262,144:
  (a) one beast_reconstruct_derivs_f32 launch writing positions, velocities and accelerations;
  (b) three beast_reconstruct_f32 launches, one per order, each fed that order's basis slab
      (the kernels of before the fused one: the tokens are read three times);
  (c) one beast_reconstruct_f32 launch with k_reconstruct_v forced (positions only), for scale.

HIP events around windows of back-to-back launches (each window at least ``--window-ms`` of
work), after a warm-up of every variant; the variants alternate inside each repeat and the
median over the repeats is reported.  The buffers rotate over enough copies that the working
set exceeds the 256 MB of last-level cache, so every launch reads its tokens from HBM.  (a)'s
share of the 8 TB/s HBM peak is its algorithmic bytes (tokens + three outputs) over its time.

    python tests/tools/deriv_timing.py [--out FILE.json]

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

T, D, N, V, DEGREE = 50, 14, 10, 256, 4
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
        raise SystemExit("deriv_timing.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    stream = _lib.stream_of(dev)
    basis = DeviceBasis(N, DEGREE, 2 * torch.pi, False)
    slabs = basis.deriv_constants(torch.linspace(0, 2 * torch.pi, T, device=dev))      # [3][2][T][N]
    w_min = torch.full((D * N,), -1.0, device=dev)
    w_max = torch.full((D * N,), 1.0, device=dev)
    dst = torch.arange(D, dtype=torch.int32, device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    results = []
    for B in args.batches:
        per_set = B * (N * D * 8 + 3 * T * D * 4)
        n_sets = max(1, -(-2 * CACHE_BYTES // per_set))
        toks = [torch.randint(0, V, (B, N * D), dtype=torch.int64, device=dev, generator=g) for _ in range(n_sets)]
        outs = [[torch.empty((B, T, D), dtype=torch.float32, device=dev) for _ in range(3)] for _ in range(n_sets)]

        def rec(tok, slab, out):
            _lib.check(lib.beast_reconstruct_f32(tok.data_ptr(), B, D, D, N, V, 0, w_min.data_ptr(), w_max.data_ptr(),
                                                 slab.data_ptr(), 0, T, dst.data_ptr(), D, None, 0, None, None,
                                                 out.data_ptr(), None, stream), "beast_reconstruct_f32")

        def fused(i):
            o = outs[i]
            _lib.check(lib.beast_reconstruct_derivs_f32(toks[i].data_ptr(), B, D, D, N, V, 0, w_min.data_ptr(),
                                                        w_max.data_ptr(), slabs.data_ptr(), 0, T, dst.data_ptr(), D,
                                                        None, 0, None, o[0].data_ptr(), o[1].data_ptr(),
                                                        o[2].data_ptr(), None, stream), "beast_reconstruct_derivs_f32")

        def three(i):
            for o in range(3):
                rec(toks[i], slabs[o], outs[i][o])

        def one_v(i):
            rec(toks[i], slabs[0], outs[i][0])

        variants = {"fused_3_orders": (fused, 0), "three_reconstruct_launches": (three, 0),
                    "k_reconstruct_v_positions": (one_v, 8)}
        families = {}

        def window(name, n_calls):
            fn, waves = variants[name]
            lib.beast_set_option(_lib.OPT_BLOCK_WAVES, waves)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(n_calls):
                fn(k % n_sets)
            e1.record()
            e1.synchronize()
            lib.beast_set_option(_lib.OPT_BLOCK_WAVES, 0)
            if name != "fused_3_orders":
                families[name] = _lib.last_codec_launch().family
            return e0.elapsed_time(e1) * 1e3 / n_calls            # us per call

        calls = {}
        for name in variants:                                      # warm-up, and size the windows
            window(name, 3)
            us = window(name, max(3, n_sets))
            calls[name] = max(n_sets, int(args.window_ms * 1e3 / us) + 1)
        samples = {name: [] for name in variants}
        for _ in range(args.repeats):
            for name in variants:
                samples[name].append(window(name, calls[name]))
        row = {"B": B, "buffer_sets": n_sets, "calls_per_window": calls, "families": families}
        for name, v in samples.items():
            row[name + "_us"] = round(statistics.median(v), 3)
            row[name + "_us_min_max"] = [round(min(v), 3), round(max(v), 3)]
        algo_bytes = B * (N * D * 8 + 3 * T * D * 4)
        row["fused_algorithmic_bytes"] = algo_bytes
        row["fused_hbm_fraction_of_8TBps"] = round(algo_bytes / (row["fused_3_orders_us"] * 1e-6) / HBM_PEAK, 4)
        results.append(row)
        del toks, outs
        torch.cuda.empty_cache()
    line = json.dumps({"tool": "deriv_timing", "shape": {"T": T, "D": D, "N": N, "V": V, "degree": DEGREE},
                       "device": torch.cuda.get_device_name(0), "results": results})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
