"""Time the streamed codec kernels (k_encode_stream, k_reconstruct_wide, csrc/codec_stream.h) beside a
plain copy of the same bytes.

``encode`` and ``reconstruct_traj`` at D = 14, (T 1024, N 32) and (T 300, N 24), B = 4,096 and 65,536.
Algorithmic bytes: encode reads B T D fp32 and writes B D N fp32 params + int64 tokens; reconstruct
reads B N D int64 tokens and writes B T D fp32.  The copy moves as many bytes (half read, half
written) with ``Tensor.copy_``.  No other library can run these shapes, so there is no ratio to hold:
the figure of interest is the fraction of the copy's rate each kernel reaches.

``encode`` / ``reconstruct`` are the API calls, the allocation of their outputs included;
``encode_kernel`` / ``reconstruct_kernel`` are the same launches through ctypes into preallocated
outputs, i.e. the kernels alone.  The copy is ``Tensor.copy_``, not a kernel of the library on the same
grid: it stands for what the memory system gives a streaming kernel, not for a launch of equal shape.

HIP events around windows of back-to-back calls (each window at least ``--window-ms`` of work) after a
warm-up of every variant; the variants alternate inside each repeat and the median over the repeats
is reported with its min - max.  Inputs rotate over enough copies to exceed twice the 256 MB of
last-level cache.

    python tests/tools/stream_timing.py [--out profiles/stream_timing.json]

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

D, V = 14, 256
CACHE_BYTES = 256 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=int, nargs="+", default=[1024, 32, 300, 24], help="T N pairs")
    ap.add_argument("--batches", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=250.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stream_timing.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    results = []
    for T, N in zip(args.shapes[0::2], args.shapes[1::2]):
        tok = BEASTBsplineTokenizer(num_dof=D, num_basis=N, seq_len=T, vocab_size=V, device="cuda:0")
        tok.load_state_dict({"w_min": [-2.0] * (D * N), "w_max": [2.0] * (D * N)})
        for B in args.batches:
            enc_bytes = B * T * D * 4 + B * D * N * 12
            rec_bytes = B * N * D * 8 + B * T * D * 4
            n_x = max(2, -(-2 * CACHE_BYTES // (B * T * D * 4)))
            n_t = max(2, -(-2 * CACHE_BYTES // (B * N * D * 8)))
            xs = [torch.randn((B, T, D), device=dev, generator=g) for _ in range(n_x)]
            toks = [torch.randint(0, V, (B, N * D), device=dev, generator=g) for _ in range(n_t)]
            src = [torch.empty(((enc_bytes + rec_bytes) // 4 // 4,), device=dev) for _ in range(n_x)]   # mean of the two, halved
            dst = torch.empty_like(src[0])
            p, lib, stream = tok._plan(), _lib.load(), _lib.raw_stream(0)
            k_par = torch.empty((B, D * N), dtype=torch.float32, device=dev)
            k_tok = torch.empty((B, N * D), dtype=torch.int64, device=dev)
            k_pos = torch.empty((B, T, D), dtype=torch.float32, device=dev)

            def encode_kernel(i):
                _lib.check(lib.beast_encode_f32(xs[i % n_x].data_ptr(), B, T, T * D, D, 1, D, D, D, p.p_src, p.p_proj, N,
                                                p.p_wmn, p.p_wmx, V, 0, k_par.data_ptr(), k_tok.data_ptr(), stream))

            def reconstruct_kernel(i):
                _lib.check(lib.beast_reconstruct_f32(toks[i % n_t].data_ptr(), B, D, D, N, V, 0, p.p_wmn, p.p_wmx,
                                                     p.p_phi, 0, T, p.p_dst, D, None, 0, None, None, k_pos.data_ptr(),
                                                     None, stream))

            variants = {"encode": lambda i: tok.encode(xs[i % n_x]), "encode_kernel": encode_kernel,
                        "reconstruct": lambda i: tok.reconstruct_traj(toks[i % n_t]),
                        "reconstruct_kernel": reconstruct_kernel, "copy": lambda i: dst.copy_(src[i % n_x])}
            row = {"T": T, "N": N, "B": B, "bytes": {"encode": enc_bytes, "reconstruct": rec_bytes,
                                                     "copy": 2 * dst.numel() * 4}}
            tok.encode(xs[0])
            row["encode_launch"] = _lib.last_codec_launch()._asdict()
            tok.reconstruct_traj(toks[0])
            row["reconstruct_launch"] = _lib.last_codec_launch()._asdict()

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
                row[name + "_gbytes_per_s"] = round(row["bytes"][name.replace("_kernel", "")] / us * 1e-3, 1)
            for name in ("encode", "encode_kernel", "reconstruct", "reconstruct_kernel"):
                row[name + "_fraction_of_copy"] = round(row[name + "_gbytes_per_s"] / row["copy_gbytes_per_s"], 3)
            results.append(row)
            del xs, toks, src, dst, variants
            torch.cuda.empty_cache()
    line = json.dumps({"tool": "stream_timing", "D": D, "V": V, "library": os.path.basename(_lib.LIB_PATH),
                       "device": torch.cuda.get_device_name(0), "results": results})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
