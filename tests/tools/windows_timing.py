"""Time encode_windows (beast_encode_windows_f32, csrc/windows.hip) against what a user could do
without it.

At the default shape (T 50, D 14, N 10, V 256) and W = 4,096 and 262,144 windows of one long episode:
  (a) ``encode_windows`` on the dense stride-1 table (every tile shares one staged segment);
  (b) ``encode_windows`` on the same table shuffled (tiles gather window by window);
  (c) the route before that kernel: ``encode(frames[idx])`` with a prebuilt [W, T] row index -- the
      index gather writes the [W, T, D] windows, encode reads them back;
  (d) ``encode`` on an already materialised [W, T, D] tensor, as the floor of (c);
  (e) (a)'s kernel alone: ``beast_encode_windows_f32`` called through ctypes into preallocated outputs,
      and, beside it, the host time of one ``encode_windows`` call (wall clock over calls that are
      never synchronised on), to tell a host-bound call from a kernel-bound one.

HIP events around windows of back-to-back calls (each window at least ``--window-ms`` of work),
after a warm-up of every variant; the variants alternate inside each repeat and the median over the
repeats is reported.  The frame buffers (a, b, c) and the materialised tensors (d) rotate over
enough copies that each variant's inputs exceed the 256 MB of last-level cache.  Also reported: the
peak of ``torch.cuda.max_memory_allocated`` over one call of (a) and of (c), above what was
allocated before the call, and whether (a) meets the bar: its median below (c)'s by more than (c)'s
own min-max spread over the repeats.

    python tests/tools/windows_timing.py [--out FILE.json]

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
        raise SystemExit("windows_timing.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    tok = BEASTBsplineTokenizer(num_dof=D, num_basis=N, seq_len=T, vocab_size=V, device="cuda:0")
    tok.load_state_dict({"w_min": [-2.0] * (D * N), "w_max": [2.0] * (D * N)})
    g = torch.Generator(device=dev).manual_seed(0)
    results = []
    for W in args.windows:
        R = W                                                  # one episode, a window from every frame
        n_sets = min(MAX_SETS, max(1, -(-2 * CACHE_BYTES // (R * D * 4))))
        n_mat = max(2, -(-2 * CACHE_BYTES // (W * T * D * 4)))
        frames = [torch.cumsum(0.05 * torch.randn((R, D), device=dev, generator=g), dim=0) for _ in range(n_sets)]
        starts, ends, _ = tok.window_index([0, R])
        assert len(starts) == W
        perm = torch.randperm(W, generator=torch.Generator().manual_seed(1))
        s_d, e_d = starts.to(dev), ends.to(dev)
        s_p, e_p = starts[perm].to(dev), ends[perm].to(dev)
        idx = torch.minimum(s_d[:, None] + torch.arange(T, device=dev), e_d[:, None] - 1)      # [W, T]
        mats = [frames[i % n_sets][idx] for i in range(n_mat)]

        variants = {"windows_dense": lambda i: tok.encode_windows(frames[i % n_sets], s_d, e_d),
                    "windows_shuffled": lambda i: tok.encode_windows(frames[i % n_sets], s_p, e_p),
                    "gather_then_encode": lambda i: tok.encode(frames[i % n_sets][idx]),
                    "encode_materialised": lambda i: tok.encode(mats[i % n_mat])}
        p = tok._plan()
        k_params = torch.empty((W, D * N), dtype=torch.float32, device=dev)
        k_tokens = torch.empty((W, N * D), dtype=torch.int64, device=dev)
        lib, stream = _lib.load(), _lib.raw_stream(0)

        def kernel_only(i):
            f = frames[i % n_sets]
            rc = lib.beast_encode_windows_f32(f.data_ptr(), R, D, 1, D, s_d.data_ptr(), e_d.data_ptr(), W, T, D,
                                              tok.joint_dof, p.p_src, p.p_proj, N, p.p_wmn, p.p_wmx, V, 0,
                                              k_params.data_ptr(), k_tokens.data_ptr(), None, stream)
            _lib.check(rc, "beast_encode_windows_f32")
        variants["windows_dense_kernel_only"] = kernel_only
        row = {"W": W, "frame_sets": n_sets, "materialised_sets": n_mat}
        # the four routes compute the same thing
        ta, pa = variants["windows_dense"](0)
        tc, pc = variants["gather_then_encode"](0)
        tb, pb = variants["windows_shuffled"](0)
        row["bitwise_equal"] = {"dense_tokens": bool(torch.equal(ta, tc)),
                                "dense_params": bool(torch.equal(pa["params"], pc["params"])),
                                "shuffled_tokens": bool(torch.equal(tb, tc[perm.to(dev)]))}
        cnt = tok.encode_windows(frames[0], s_d, e_d, return_tile_counts=True)[1]["tile_counts"].tolist()
        cnt_p = tok.encode_windows(frames[0], s_p, e_p, return_tile_counts=True)[1]["tile_counts"].tolist()
        row["tile_counts_dense"], row["tile_counts_shuffled"] = cnt, cnt_p
        del ta, pa, tc, pc, tb, pb

        for name in ("windows_dense", "gather_then_encode"):      # peak memory of one call
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
        n_host = min(calls["windows_dense"], 500)
        t0 = time.perf_counter()
        for k in range(n_host):
            variants["windows_dense"](k)
        row["windows_dense_host_us"] = round((time.perf_counter() - t0) / n_host * 1e6, 3)
        torch.cuda.synchronize()
        c = samples["gather_then_encode"]
        row["gather_over_windows_dense"] = round(row["gather_then_encode_us"] / row["windows_dense_us"], 2)
        row["bar_met"] = bool(row["gather_then_encode_us"] - row["windows_dense_us"] > max(c) - min(c))
        results.append(row)
        del frames, mats, idx
        torch.cuda.empty_cache()
    line = json.dumps({"tool": "windows_timing", "shape": {"T": T, "D": D, "N": N, "V": V},
                       "library": os.path.basename(_lib.LIB_PATH), "device": torch.cuda.get_device_name(0),
                       "results": results})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
