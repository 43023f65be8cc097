"""Time the wide-DoF codec kernels (k_encode_dof, k_reconstruct_dof, csrc/codec_wide_dof.h) beside the
way such data was handled before them, and beside a plain copy of the same bytes.

``encode`` and ``reconstruct_traj`` at B = 4,096 for (T 50, N 10) at D = 128 and 256 and (T 1024, N 32)
at D = 128.  The yardstick (``sliced_*``) is D / 64 tokenizers of 64 DoFs on column slices of the same
tensors, launched back to back: encode reads ``x[..., 64 s : 64 s + 64]`` in place (a strided view),
reconstruct takes each slice's own contiguous token tensor and writes its own [B, T, 64] output, so
it does less than the wide call (no single (n d) token row, no single output) and is the faster side
of a fair comparison.  Algorithmic bytes: encode reads B T D fp32 and writes B D N fp32 params + int64
tokens; reconstruct reads B N D int64 tokens and writes B T D fp32.  The copy moves as many bytes (half
read, half written) with ``Tensor.copy_``: the figure of interest is the fraction of the copy's rate.

HIP events around windows of back-to-back calls (each window at least ``--window-ms`` of work) after a
warm-up of every variant; the variants alternate inside each repeat and the median over the repeats
is reported with its min - max.  Inputs rotate over enough copies to exceed twice the 256 MB of
last-level cache.

    python tests/tools/wide_dof_timing.py [--out profiles/wide_dof_timing.json]

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

V, SLICE = 256, 64
CACHE_BYTES = 256 << 20


def _tok(D, N, T):
    tok = BEASTBsplineTokenizer(num_dof=D, num_basis=N, seq_len=T, vocab_size=V, device="cuda:0")
    tok.load_state_dict({"w_min": [-2.0] * (D * N), "w_max": [2.0] * (D * N)})
    return tok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=int, nargs="+", default=[50, 10, 128, 50, 10, 256, 1024, 32, 128],
                    help="T N D triples")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=250.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wide_dof_timing.py needs a GPU: nothing is measured without one")
    dev, B = torch.device("cuda", 0), args.batch
    g = torch.Generator(device=dev).manual_seed(0)
    results = []
    for T, N, D in zip(args.shapes[0::3], args.shapes[1::3], args.shapes[2::3]):
        tok, part, ns = _tok(D, N, T), _tok(SLICE, N, T), D // SLICE
        enc_bytes = B * T * D * 4 + B * D * N * 12
        rec_bytes = B * N * D * 8 + B * T * D * 4
        n_x = max(2, -(-2 * CACHE_BYTES // (B * T * D * 4)))
        n_t = max(2, -(-2 * CACHE_BYTES // (B * N * D * 8)))
        xs = [torch.randn((B, T, D), device=dev, generator=g) for _ in range(n_x)]
        toks = [torch.randint(0, V, (B, N * D), device=dev, generator=g) for _ in range(n_t)]
        # the slices' own token tensors: [B, N, 64] of every 64 columns, contiguous
        parts = [[t.view(B, N, D)[:, :, s * SLICE:(s + 1) * SLICE].reshape(B, N * SLICE).contiguous() for s in range(ns)]
                 for t in toks]
        src = [torch.empty(((enc_bytes + rec_bytes) // 4 // 4,), device=dev) for _ in range(n_x)]   # mean of the two, halved
        dst = torch.empty_like(src[0])

        def sliced_encode(i):
            return [part.encode(xs[i % n_x][:, :, s * SLICE:(s + 1) * SLICE]) for s in range(ns)]

        def sliced_reconstruct(i):
            return [part.reconstruct_traj(t) for t in parts[i % n_t]]

        variants = {"encode": lambda i: tok.encode(xs[i % n_x]), "sliced_encode": sliced_encode,
                    "reconstruct": lambda i: tok.reconstruct_traj(toks[i % n_t]),
                    "sliced_reconstruct": sliced_reconstruct, "copy": lambda i: dst.copy_(src[i % n_x])}
        row = {"T": T, "N": N, "D": D, "B": B, "slices": ns,
               "bytes": {"encode": enc_bytes, "reconstruct": rec_bytes, "copy": 2 * dst.numel() * 4}}
        tok.encode(xs[0])
        row["encode_launch"], row["encode_grid"] = _lib.last_codec_launch()._asdict(), _lib.last_launch_grid()
        tok.reconstruct_traj(toks[0])
        row["reconstruct_launch"], row["reconstruct_grid"] = _lib.last_codec_launch()._asdict(), _lib.last_launch_grid()
        # the slices compute what the wide call computes (another kernel, so another order of summation)
        wide, cut = tok.encode(xs[0])[1]["params"].view(B, D, N), sliced_encode(0)
        row["max_param_diff_vs_slices"] = max(
            float((wide[:, s * SLICE:(s + 1) * SLICE] - c[1]["params"].view(B, SLICE, N)).abs().max()) for s, c in enumerate(cut))

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
            calls[name] = max(8, min(4000, int(args.window_ms * 1e3 / window(name, 8)) + 1))
        samples = {name: [] for name in variants}
        for _ in range(args.repeats):
            for name in variants:
                samples[name].append(window(name, calls[name]))
        row["calls_per_window"] = calls
        for name, v in samples.items():
            us = statistics.median(v)
            row[name + "_us"] = round(us, 3)
            row[name + "_us_min_max"] = [round(min(v), 3), round(max(v), 3)]
            row[name + "_gbytes_per_s"] = round(row["bytes"][name.replace("sliced_", "")] / us * 1e-3, 1)
        for name in ("encode", "sliced_encode", "reconstruct", "sliced_reconstruct"):
            row[name + "_fraction_of_copy"] = round(row[name + "_gbytes_per_s"] / row["copy_gbytes_per_s"], 3)
        results.append(row)
        del xs, toks, parts, src, dst, variants
        torch.cuda.empty_cache()
    line = json.dumps({"tool": "wide_dof_timing", "V": V, "library": os.path.basename(_lib.LIB_PATH),
                       "device": torch.cuda.get_device_name(0), "results": results})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
