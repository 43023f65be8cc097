"""Time the fused encode -> reconstruct statistics against the launches it replaces.

At the default shape (T 50, D 14, N 10, V 256, degree 4) and B = 4,096 and 262,144:
  (a)  one beast_roundtrip_stats_f32 launch, statistics and clip counts only;
  (a') the same launch also writing the tokens; and, for scale, without the clip counts;
  (b)  beast_encode_f32 (params + tokens) then beast_reconstruct_f32, the launches alone;
  (c)  compute_reconstruction_error as it stands: those launches plus the torch reductions
       (no .item(): the host never waits inside the window).

HIP events around windows of back-to-back calls (each window at least ``--window-ms`` of work),
after a warm-up of every variant; the variants alternate inside each repeat and the median over the
repeats is reported with the minimum and maximum.  The trajectory buffers rotate over enough copies
that the working set exceeds the 256 MB of last-level cache, so every call reads its trajectories
from HBM.  (a)'s share of the 8 TB/s HBM peak is its algorithmic bytes (the trajectory in, 16 B per
trajectory and DoF out) over its time.

    python tests/tools/roundtrip_timing.py [--out FILE.json]

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
from beast_tokenizer_amd import BEASTBsplineTokenizer, _lib  # noqa: E402
from beast_tokenizer_amd.synthetic import synth_trajectories  # noqa: E402

T, D, N, V = 50, 14, 10, 256
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
        raise SystemExit("roundtrip_timing.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    tok = BEASTBsplineTokenizer(num_dof=D, num_basis=N, seq_len=T, vocab_size=V, device="cuda:0")
    seed = torch.from_numpy(synth_trajectories(4096, T, D, seed=3)).to(dev)
    tok.fit_parameters([{"actions": seed}], verbose=False)           # 1 % / 99 % bounds: some params clip
    p = tok._plan()
    stream = _lib.raw_stream(p.idx)
    results = []
    for B in args.batches:
        per_set = B * T * D * 4
        n_sets = max(1, -(-2 * CACHE_BYTES // per_set))
        reps = -(-B // seed.shape[0])
        xs = [(seed.repeat(reps, 1, 1)[:B] * (1.0 + 0.01 * i)).contiguous() for i in range(n_sets)]
        stats = torch.empty((B, D, 4), dtype=torch.float32, device=dev)
        clip = torch.zeros((2, D * N), dtype=torch.int32, device=dev)
        tokens = torch.empty((B, N * D), dtype=torch.int64, device=dev)
        params = torch.empty((B, D * N), dtype=torch.float32, device=dev)
        pos = torch.empty((B, T, D), dtype=torch.float32, device=dev)

        def fused(i, tk=None, counts=True):
            x = xs[i]
            _lib.check(lib.beast_roundtrip_stats_f32(x.data_ptr(), B, T, T * D, D, 1, D, D, D, p.p_src, p.p_proj, p.p_phi,
                                                     N, p.p_wmn, p.p_wmx, V, 0, tk, stats.data_ptr(),
                                                     clip.data_ptr() if counts else None, stream),
                       "beast_roundtrip_stats_f32")

        def fused_tokens(i):
            fused(i, tokens.data_ptr())

        def fused_no_counts(i):
            fused(i, None, False)

        def two_launches(i):
            x = xs[i]
            _lib.check(lib.beast_encode_f32(x.data_ptr(), B, T, T * D, D, 1, D, D, D, p.p_src, p.p_proj, N, p.p_wmn,
                                            p.p_wmx, V, 0, params.data_ptr(), tokens.data_ptr(), stream),
                       "beast_encode_f32")
            _lib.check(lib.beast_reconstruct_f32(tokens.data_ptr(), B, D, D, N, V, 0, p.p_wmn, p.p_wmx, p.p_phi, 0, T,
                                                 p.p_dst, D, None, 0, None, None, pos.data_ptr(), None, stream),
                       "beast_reconstruct_f32")

        def error_api(i):
            tok.compute_reconstruction_error(xs[i])

        variants = {"fused": fused, "fused_with_tokens": fused_tokens, "fused_without_clip_counts": fused_no_counts,
                    "encode_plus_reconstruct": two_launches,
                    "compute_reconstruction_error": error_api}

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
        for name in variants:                                      # warm-up, and size the windows
            window(name, 3)
            us = window(name, max(3, n_sets))
            calls[name] = max(n_sets, int(args.window_ms * 1e3 / us) + 1)
        samples = {name: [] for name in variants}
        for _ in range(args.repeats):
            for name in variants:
                samples[name].append(window(name, calls[name]))
        row = {"B": B, "buffer_sets": n_sets, "calls_per_window": calls}
        for name, v in samples.items():
            row[name + "_us"] = round(statistics.median(v), 3)
            row[name + "_us_min_max"] = [round(min(v), 3), round(max(v), 3)]
        algo_bytes = B * (T * D * 4 + D * 16)
        row["fused_algorithmic_bytes"] = algo_bytes
        row["fused_hbm_fraction_of_8TBps"] = round(algo_bytes / (row["fused_us"] * 1e-6) / HBM_PEAK, 4)
        results.append(row)
        del xs, stats, tokens, params, pos
        torch.cuda.empty_cache()
    line = json.dumps({"tool": "roundtrip_timing", "shape": {"T": T, "D": D, "N": N, "V": V},
                       "device": torch.cuda.get_device_name(0), "results": results})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
