"""Time the boundary-condition add of a long reconstruction: k_cond_add_long against k_cond_add
(csrc/cond.hip), both behind ``beast_cond_add_f32``.

Conditioned ``reconstruct_traj`` at T = 1024, N = 32, D = 14, (ic, ec) = (2, 2), B = 4,096 and 65,536,
beside the plain ``reconstruct_traj`` of an unconditioned tokenizer of the same shape (what the
conditions cost on top), and the ``beast_cond_add_f32`` launch alone through ctypes.  The library has no
switch between the two kernels: ``--old-lib`` names a library built from the commit before
k_cond_add_long, whose ``beast_cond_add_f32`` runs k_cond_add at every shape; the two libraries are
loaded side by side and their launches alternate inside each repeat, on the same buffers (the add
accumulates into ``pos``; its values do not matter to the time).

HIP events around windows of back-to-back calls (each window at least ``--window-ms`` of work) after a
warm-up of every variant; the median over the repeats is reported with its min - max.

    python tests/tools/cond_long_timing.py --old-lib PATH [--out profiles/cond_long_timing.json]

Needs a GPU; prints one JSON line.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from beast_tokenizer_amd import BEASTBsplineTokenizer, _lib  # noqa: E402

D, V, T, N, IC, EC = 14, 256, 1024, 32, 2, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old-lib", default=None, help="a library whose beast_cond_add_f32 has k_cond_add only")
    ap.add_argument("--batches", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=250.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cond_long_timing.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    libs = {"new": _lib.load()}
    if args.old_lib:
        libs["old"] = ctypes.CDLL(os.path.abspath(args.old_lib))
    for lib in libs.values():
        lib.beast_cond_add_f32.restype = ctypes.c_int
        lib.beast_cond_add_f32.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                           ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    kw = dict(num_dof=D, num_basis=N, seq_len=T, vocab_size=V, device="cuda:0")
    tok, plain = BEASTBsplineTokenizer(init_cond_order=IC, end_cond_order=EC, **kw), BEASTBsplineTokenizer(**kw)
    for t in (tok, plain):
        t.load_state_dict({"w_min": [-2.0] * (D * N), "w_max": [2.0] * (D * N)})
    full = tok._basis.full_basis_at(tok.times.to(dev).reshape(-1))
    jidx = torch.arange(D, dtype=torch.int32, device=dev)
    results = []
    for B in args.batches:
        x = torch.randn((B, T, D), device=dev, generator=g)
        toks = torch.randint(0, V, (B, N * D), device=dev, generator=g)
        tok.encode(x)                                            # the conditions of this batch
        st = tok._cond_state
        pos = torch.zeros((B, T, D), device=dev)
        stream = _lib.raw_stream(0)

        def add(lib):
            rc = lib.beast_cond_add_f32(pos.data_ptr(), B, T, D, jidx.data_ptr(), D, full.data_ptr(), 0, N + IC + EC, IC, EC,
                                        st["params_init"].data_ptr(), st["params_end"].data_ptr(),
                                        st["init_pos"].data_ptr(), stream)
            if rc:
                raise RuntimeError(f"beast_cond_add_f32 returned {rc}")

        variants = {"reconstruct_conditioned": lambda: tok.reconstruct_traj(toks),
                    "reconstruct_plain": lambda: plain.reconstruct_traj(toks)}
        variants.update({f"cond_add_{name}": (lambda lib=lib: add(lib)) for name, lib in libs.items()})

        def window(name, n_calls):
            fn = variants[name]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n_calls):
                fn()
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
        row = {"T": T, "N": N, "B": B, "ic": IC, "ec": EC, "cond_add_bytes": 2 * B * T * D * 4, "calls_per_window": calls}
        for name, v in samples.items():
            row[name + "_us"] = round(statistics.median(v), 3)
            row[name + "_us_min_max"] = [round(min(v), 3), round(max(v), 3)]
        for name in libs:
            row[f"cond_add_{name}_gbytes_per_s"] = round(row["cond_add_bytes"] / row[f"cond_add_{name}_us"] * 1e-3, 1)
        results.append(row)
        del x, toks, pos, variants
        torch.cuda.empty_cache()
    line = json.dumps({"tool": "cond_long_timing", "D": D, "V": V, "old_library": bool(args.old_lib),
                       "device": torch.cuda.get_device_name(0), "results": results})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
