"""Time the fit stage of ``fit_parameters`` at a long horizon: list mode (k_encode_stream_list, one
``beast_encode_list_f32`` launch per group of batches) against one ``beast_encode_f32`` launch per
dataloader batch, which is what ``fit_parameters`` did at these shapes before list mode took them.

T = 1024, N = 32, D = 14; two datasets of device-resident batches: 64 batches of 1,024 rows and 245
batches of 256 rows.  Timed: the encode launches of one pass over the dataset (``_fit_list`` per group
with its pointer table, or ``compute_weights`` per batch, output allocation included), HIP events
around windows of back-to-back passes (each at least ``--window-ms`` of work); the quantile passes
that follow in ``fit_parameters`` are not part of it.  ``single`` is the plain streamed encode of the
same rows as one tensor in one launch: the per-trajectory rate a launch without a table reaches.  The variants alternate inside each repeat; the median over the
repeats is reported with its min - max.  A dataset (3.6 - 3.8 GB) exceeds the last-level cache many
times over, so every pass reads its rows from HBM.

    python tests/tools/stream_list_timing.py [--out profiles/stream_list_timing.json]

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

T, N, D = 1024, 32, 14


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--datasets", type=int, nargs="+", default=[64, 1024, 245, 256], help="batches rows pairs")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=150.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stream_list_timing.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    tok = BEASTBsplineTokenizer(num_dof=D, num_basis=N, seq_len=T, device="cuda:0")
    results = []
    for nbatch, rows in zip(args.datasets[0::2], args.datasets[1::2]):
        whole = torch.randn((nbatch * rows, T, D), device=dev, generator=g)
        batches = [whole[i * rows:(i + 1) * rows].clone() for i in range(nbatch)]   # one allocation per batch
        per_group = max(tok._FIT_GROUP_ROWS // rows, 1)
        groups = [batches[i:i + per_group] for i in range(0, nbatch, per_group)]

        def list_mode():
            return [tok._fit_list(grp) for grp in groups]

        def per_batch():
            return [tok.compute_weights(b) for b in batches]

        def single():
            return [tok.compute_weights(whole)]

        variants = {"list": list_mode, "per_batch": per_batch, "single": single}
        row = {"T": T, "N": N, "D": D, "batches": nbatch, "rows_per_batch": rows, "list_launches": len(groups)}
        out = list_mode()
        row["list_launch"], row["list_grid"] = _lib.last_codec_launch()._asdict(), _lib.last_launch_grid()
        row["bitwise_equal"] = bool(torch.equal(torch.cat(out), torch.cat(per_batch())))
        del out

        def window(fn, passes):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(passes):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / passes   # us per pass

        passes = {}
        for name, fn in variants.items():   # warm-up, and size the windows
            window(fn, 2)
            passes[name] = max(4, int(args.window_ms * 1e3 / window(fn, 4)) + 1)
        row["passes_per_window"] = passes
        samples = {name: [] for name in variants}
        for _ in range(args.repeats):
            for name, fn in variants.items():
                samples[name].append(window(fn, passes[name]))
        for name, v in samples.items():
            us = statistics.median(v)
            row[name + "_us"] = round(us, 1)
            row[name + "_us_min_max"] = [round(min(v), 1), round(max(v), 1)]
            row[name + "_ns_per_trajectory"] = round(us * 1e3 / (nbatch * rows), 2)
            row[name + "_gbytes_per_s"] = round(nbatch * rows * (T * D + D * N) * 4 / us * 1e-3, 1)
        results.append(row)
        del whole, batches, groups, variants
        torch.cuda.empty_cache()
    line = json.dumps({"tool": "stream_list_timing", "library": os.path.basename(_lib.LIB_PATH),
                       "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "results": results})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
