"""Time encode_at (beast_encode_rows_f32, csrc/fit_rows.hip) against what a user could do without it.

At the default shape (T 50, D 14, N 10, V 256, degree 4) and B = 4,096 and 262,144, with per-row
jittered times and weights in [0.25, 4]:
  (a) ``encode_at``: one launch, basis + float64 Gram + solve + quantise;
  (b) the torch composition of before that kernel: ``DeviceBasis.basis_at`` (a [B, T, N] slab),
      float64 einsums for G and R, ``torch.linalg.solve``, ``beast_quantize_f32``;
  (c) the shared-grid ``encode`` on the same trajectories, as the floor: one projection for all rows.

HIP events around windows of back-to-back calls (each window at least ``--window-ms`` of work),
after a warm-up of every variant; the variants alternate inside each repeat and the median over the
repeats is reported.  The trajectories rotate over enough copies that the working set exceeds the
256 MB of last-level cache.  Also reported: the largest difference between (a)'s and (b)'s params,
as a check that both solve the same problem.

    python tests/tools/rows_timing.py [--out FILE.json]

Needs a GPU; prints one JSON line.  BEAST_LIB selects another build of the library (a build with
-DBEAST_ROWS_FMA accumulates by v_fma_f64 instead of the float64 MFMA).
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

T, D, N, V, DEGREE = 50, 14, 10, 256, 4
CACHE_BYTES = 256 << 20


def torch_rows(tok, x, t, w, dev):
    """(tokens, params) by torch ops over a basis slab: the route before beast_encode_rows_f32."""
    B = x.shape[0]
    phi = tok._basis.basis_at(t)[0].double()                                   # [B, T, N]
    wphi = phi * w.double()[..., None]
    G = torch.einsum("btn,btm->bnm", wphi, phi) + tok._basis.reg * torch.eye(N, dtype=torch.float64, device=dev)
    R = torch.einsum("btn,btd->bnd", wphi, x.double())
    W = torch.linalg.solve(G, R)                                               # [B, N, D]
    params = W.transpose(1, 2).reshape(B, -1).float().contiguous()
    return tok._quantize(params, 0, dev, 0), params


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[4096, 262144])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=30.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rows_timing.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    tok = BEASTBsplineTokenizer(num_dof=D, num_basis=N, degree_p=DEGREE, seq_len=T, vocab_size=V, device="cuda:0")
    tok.load_state_dict({"w_min": [-2.0] * (D * N), "w_max": [2.0] * (D * N)})
    duration = float(tok.duration)
    g = torch.Generator(device=dev).manual_seed(0)
    results = []
    for B in args.batches:
        n_sets = max(1, -(-2 * CACHE_BYTES // (B * T * D * 4)))
        xs = [torch.cumsum(0.05 * torch.randn((B, T, D), device=dev, generator=g), dim=1) for _ in range(n_sets)]
        grid = torch.linspace(0, duration, T, device=dev)
        t = grid + (torch.rand((B, T), device=dev, generator=g) * 0.8 - 0.4) * (duration / (T - 1))
        w = 0.25 + 3.75 * torch.rand((B, T), device=dev, generator=g)

        variants = {"encode_at": lambda i: tok.encode_at(xs[i], t, w),
                    "torch_composition": lambda i: torch_rows(tok, xs[i], t, w, dev),
                    "shared_grid_encode": lambda i: tok.encode(xs[i])}
        row = {"B": B, "buffer_sets": n_sets}
        try:
            pa, pb = variants["encode_at"](0)[1]["params"], variants["torch_composition"](0)[1]
            row["max_abs_param_diff_a_b"] = float((pa - pb).abs().max())
        except Exception as e:   # a torch build without a batched float64 solve
            row["torch_composition_error"] = repr(e)[:200]
            del variants["torch_composition"]

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
            calls[name] = max(n_sets, min(2000, int(args.window_ms * 1e3 / us) + 1))
        samples = {name: [] for name in variants}
        for _ in range(args.repeats):
            for name in variants:
                samples[name].append(window(name, calls[name]))
        row["calls_per_window"] = calls
        for name, v in samples.items():
            row[name + "_us"] = round(statistics.median(v), 3)
            row[name + "_us_min_max"] = [round(min(v), 3), round(max(v), 3)]
        if "torch_composition" in samples:
            row["torch_over_encode_at"] = round(row["torch_composition_us"] / row["encode_at_us"], 2)
        row["encode_at_over_shared_grid"] = round(row["encode_at_us"] / row["shared_grid_encode_us"], 2)
        results.append(row)
        del xs
        torch.cuda.empty_cache()
    line = json.dumps({"tool": "rows_timing", "shape": {"T": T, "D": D, "N": N, "V": V, "degree": DEGREE},
                       "library": os.path.basename(_lib.LIB_PATH), "device": torch.cuda.get_device_name(0),
                       "results": results})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
