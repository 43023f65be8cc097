"""Time beast_reconstruct_derivs_f32 on dense output grids, this tree against another build.

Shared order slabs past the resident kernel's 48 KB stream through k_reconstruct_derivs_stream; the
library given by ``--parent-lib`` (a build of the parent commit) reads them from memory element by
element.  Per shape (D 14, all three orders, degree 4):
  (a) ``tree``    one launch of this tree's library;
  (b) ``parent``  one launch of the other library on the same inputs and outputs;
  (c) ``copy``    one Tensor.copy_ of the three outputs' bytes: what storing them costs at least.
The outputs of (a) and (b) are compared bit for bit first.

HIP events around windows of back-to-back calls (each window at least ``--window-ms`` of work) after a
warm-up of every form; the forms alternate inside each repeat; median of 7 with min - max.  The
buffers rotate over up to 8 copies, enough to exceed the 256 MB of last-level cache at B >= 64.

    python tests/tools/deriv_dense_timing.py --parent-lib OTHER/libbeast_hip.so [--out FILE.json]

Needs a GPU; prints one JSON line.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from beast_tokenizer_amd import _lib  # noqa: E402
from beast_tokenizer_amd.bspline import DeviceBasis  # noqa: E402

D, V, DEGREE = 14, 256, 4
SHAPES = [(10, T, B) for T in (512, 2048) for B in (1, 64, 4096)] + [(16, 1024, 4096)]   # N, T_out, B
CACHE_BYTES = 256 << 20
ENTRY = "beast_reconstruct_derivs_f32"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=100.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("deriv_dense_timing.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    tree = _lib.load()
    parent = C.CDLL(os.path.abspath(args.parent_lib))
    getattr(parent, ENTRY).restype, getattr(parent, ENTRY).argtypes = _lib.SIGNATURES[ENTRY]
    stream = _lib.stream_of(dev)
    dst = torch.arange(D, dtype=torch.int32, device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    results = []
    for N, T, B in SHAPES:
        slabs = DeviceBasis(N, DEGREE, 2 * torch.pi, False).deriv_constants(torch.linspace(0, 2 * torch.pi, T, device=dev))
        w_min = torch.full((D * N,), -1.0, device=dev)
        w_max = torch.full((D * N,), 1.0, device=dev)
        out_bytes = 3 * B * T * D * 4
        n_sets = max(1, min(8, -(-2 * CACHE_BYTES // out_bytes)))
        toks = [torch.randint(0, V, (B, N * D), dtype=torch.int64, device=dev, generator=g) for _ in range(n_sets)]
        outs = [torch.empty((3, B, T, D), dtype=torch.float32, device=dev) for _ in range(n_sets)]
        src = torch.randn((3, B, T, D), dtype=torch.float32, device=dev, generator=g)

        def derivs(lib, i):
            o = outs[i]
            rc = getattr(lib, ENTRY)(toks[i].data_ptr(), B, D, D, N, V, 0, w_min.data_ptr(), w_max.data_ptr(),
                                     slabs.data_ptr(), 0, T, dst.data_ptr(), D, None, 0, None, o[0].data_ptr(),
                                     o[1].data_ptr(), o[2].data_ptr(), None, stream)
            if rc:
                raise RuntimeError(f"{ENTRY} returned {rc}")

        forms = {"tree": lambda i: derivs(tree, i), "parent": lambda i: derivs(parent, i),
                 "copy": lambda i: outs[i].copy_(src)}
        derivs(parent, 0)
        want = outs[0].clone()
        derivs(tree, 0)
        grid = _lib.last_launch_grid()
        same = torch.equal(outs[0], want)
        max_diff = float((outs[0] - want).abs().max())

        def window(name, n_calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(n_calls):
                forms[name](k % n_sets)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / n_calls            # us per call

        calls = {}
        for name in forms:                                        # warm-up, and size the windows
            window(name, 3)
            us = window(name, max(3, n_sets))
            calls[name] = max(n_sets, int(args.window_ms * 1e3 / us) + 1)
        samples = {name: [] for name in forms}
        for _ in range(args.repeats):
            for name in forms:
                samples[name].append(window(name, calls[name]))
        rc = tree.beast_reconstruct_derivs_stream_rows(T, D, D, N, D, 7)
        row = {"N": N, "T_out": T, "B": B, "chunk_rows": rc, "tree_grid": grid, "buffer_sets": n_sets,
               "calls_per_window": calls, "tree_equals_parent_bitwise": same, "tree_parent_max_abs_diff": max_diff,
               "output_bytes": out_bytes}
        for name, v in samples.items():
            row[name + "_us"] = round(statistics.median(v), 3)
            row[name + "_us_min_max"] = [round(min(v), 3), round(max(v), 3)]
        row["parent_over_tree"] = round(row["parent_us"] / row["tree_us"], 3)
        row["tree_fraction_of_copy_rate"] = round(row["copy_us"] / row["tree_us"], 3)
        results.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del toks, outs, src, want
        torch.cuda.empty_cache()
    line = json.dumps({"tool": "deriv_dense_timing", "shape": {"D": D, "V": V, "degree": DEGREE, "orders": [0, 1, 2]},
                       "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "results": results})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
