"""Time reconstruct_windows (beast_reconstruct_windows_f32, csrc/blend.hip) against what a user could
do without it.

At the default shape (T 50, D 14, N 10, V 256), one episode of W frames, a stride-1 table on the
device, "exp" blend weights, and W = 4,096 and 262,144:
  (a) ``reconstruct_windows``;
  (b) the composition available before that kernel: ``reconstruct_traj(tokens)`` -> a prebuilt [W T]
      row index -> ``index_add_`` of the weighted values and of the weights -> divide (float atomics:
      not reproducible run to run);
  (c) (a)'s kernel alone: ``beast_reconstruct_windows_f32`` called through ctypes into preallocated
      outputs, and, beside it, the host time of one ``reconstruct_windows`` call (wall clock over calls
      that are never synchronised on), to tell a host-bound call from a kernel-bound one.

HIP events around windows of back-to-back calls (each window at least ``--window-ms`` of work),
after a warm-up of every variant; the variants alternate inside each repeat and the median over the
repeats is reported with its min - max.  The token buffers rotate over enough copies that a variant's
inputs exceed twice the 256 MB of last-level cache.  Also reported: the peak of
``torch.cuda.max_memory_allocated`` over one call of (a) and of (b), above what was allocated before
the call, the largest difference between (a) and (b), and whether (a) meets the bar: not slower than
(b) by more than (b)'s own min - max spread, with a smaller peak.

    python tests/tools/blend_timing.py [--out FILE.json]

Needs a GPU; prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from beast_tokenizer_amd import BEASTBsplineTokenizer, _lib  # noqa: E402

T, D, N, V = 50, 14, 10, 256
CACHE_BYTES = 256 << 20
MAX_SETS = 2048


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, nargs="+", default=[4096, 262144])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=30.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("blend_timing.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    tok = BEASTBsplineTokenizer(num_dof=D, num_basis=N, seq_len=T, vocab_size=V, device="cuda:0")
    tok.load_state_dict({"w_min": [-2.0] * (D * N), "w_max": [2.0] * (D * N)})
    g = torch.Generator(device=dev).manual_seed(0)
    bw = tok.blend_weights("exp", m=0.1)
    results = []
    for W in args.windows:
        R = W                                                  # one episode, a window from every frame
        n_sets = min(MAX_SETS, max(2, -(-2 * CACHE_BYTES // (W * N * D * 8))))
        tokens = [torch.randint(0, V, (W, N * D), device=dev, generator=g) for _ in range(n_sets)]
        starts, ends, _ = tok.window_index([0, R])
        assert len(starts) == W
        s_d, e_d = starts.to(dev), ends.to(dev)
        # (b)'s prebuilt index: sample t of window w lies on row start + t while t < end - start
        t = torch.arange(T, device=dev)
        own = t[None, :] < (e_d - s_d)[:, None]
        ridx = torch.where(own, s_d[:, None] + t[None, :], torch.zeros_like(s_d)[:, None]).reshape(-1)
        wts = torch.where(own, bw[None, :], torch.zeros((), device=dev)).reshape(-1)

        def blend(i):
            return tok.reconstruct_windows(tokens[i % n_sets], s_d, e_d, R, blend=bw)[0]

        def composition(i):
            y = tok.reconstruct_traj(tokens[i % n_sets]).reshape(W * T, D)
            num = torch.zeros((R, D), device=dev).index_add_(0, ridx, y * wts[:, None])
            den = torch.zeros((R,), device=dev).index_add_(0, ridx, wts)
            return num / den[:, None]

        p = tok._plan()
        k_out = torch.empty((R, D), dtype=torch.float32, device=dev)
        k_cov = torch.empty((R,), dtype=torch.int32, device=dev)
        k_wt = torch.empty((R,), dtype=torch.float32, device=dev)
        lib, stream = _lib.load(), _lib.raw_stream(0)

        def kernel_only(i):
            rc = lib.beast_reconstruct_windows_f32(tokens[i % n_sets].data_ptr(), None, W, D, tok.joint_dof, N, V, 0,
                                                   p.p_wmn, p.p_wmx, p.p_phi, T, s_d.data_ptr(), e_d.data_ptr(), R,
                                                   bw.data_ptr(), float("nan"), p.p_dst, D, k_out.data_ptr(), D,
                                                   k_cov.data_ptr(), k_wt.data_ptr(), None, stream)
            _lib.check(rc, "beast_reconstruct_windows_f32")

        variants = {"blend": blend, "composition": composition, "blend_kernel_only": kernel_only}
        row = {"W": W, "token_sets": n_sets}
        a0, b0 = blend(0), composition(0)
        row["max_abs_difference"] = float((a0 - b0).abs().max())
        row["runs_bitwise_equal"] = {"blend": bool(torch.equal(a0, blend(0))),
                                     "composition": bool(torch.equal(b0, composition(0)))}
        info = tok.reconstruct_windows(tokens[0], s_d, e_d, R, blend=bw, return_tile_counts=True)[1]
        row["tile_counts"] = info["tile_counts"].tolist()
        del a0, b0, info

        for name in ("blend", "composition"):                      # peak memory of one call
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            out = variants[name](0)
            torch.cuda.synchronize()
            row[name + "_peak_bytes"] = int(torch.cuda.max_memory_allocated() - base)
            del out

        def window(name, n_calls):
            fn = variants[name]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(n_calls):
                fn(k)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / n_calls            # us per call

        calls = {}
        for name in variants:                                      # warm-up, and size the windows
            window(name, 3)
            us = window(name, 8)
            calls[name] = max(8, min(4000, int(args.window_ms * 1e3 / us) + 1))
        samples = {name: [] for name in variants}
        for _ in range(args.repeats):
            for name in variants:
                samples[name].append(window(name, calls[name]))
        row["calls_per_window"] = calls
        for name, v in samples.items():
            row[name + "_us"] = round(statistics.median(v), 3)
            row[name + "_us_min_max"] = [round(min(v), 3), round(max(v), 3)]
        torch.cuda.synchronize()
        n_host = min(calls["blend"], 500)
        t0 = time.perf_counter()
        for k in range(n_host):
            blend(k)
        row["blend_host_us"] = round((time.perf_counter() - t0) / n_host * 1e6, 3)
        torch.cuda.synchronize()
        c = samples["composition"]
        row["composition_over_blend"] = round(row["composition_us"] / row["blend_us"], 2)
        row["bar_met"] = bool(row["blend_us"] - row["composition_us"] <= max(c) - min(c)
                              and row["blend_peak_bytes"] < row["composition_peak_bytes"])
        results.append(row)
        del tokens, ridx, wts, own
        torch.cuda.empty_cache()
    line = json.dumps({"tool": "blend_timing", "shape": {"T": T, "D": D, "N": N, "V": V},
                       "library": os.path.basename(_lib.LIB_PATH), "device": torch.cuda.get_device_name(0),
                       "results": results})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
