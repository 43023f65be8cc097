"""Time the fused sampler against what a user could write without it.

At the default shape (K 140 = N 10 x D 14 tokens, V 256), B = 256 and 4,096, fp32 and bf16, S = 1 and
16 draws per row, plain (temperature only) and truncated (top_k 50, top_p 0.9), temperature 0.8:
  (a) fused: the uniforms (``uniform_`` into a preallocated [S, B, K] buffer) and one
      beast_sample_rows launch: logits -> tokens and their log-probabilities;
  (b) the ATen composition, which returns tokens only:
      plain      torch.multinomial(softmax(l.float() / tau), S, replacement=True)
      truncated  the usual sort-based warpers in front of it: topk -> masked_fill, sort -> softmax ->
                 cumsum -> mask -> scatter -> masked_fill.

The protocol is tests/tools/xent_timing.py's: HIP events around windows of back-to-back calls (each
window at least ``--window-ms`` of work), after a warm-up of every variant; the variants alternate
inside each repeat and the median over the repeats is reported with the minimum and maximum.  The
buffers rotate over enough copies that the working set exceeds twice the 256 MB of last-level cache.
The fused kernel's share of the 8 TB/s HBM peak is its algorithmic bytes over its time: the logits
read once, the uniforms written and read, tokens and log-probabilities written.  The gate: the fused
variant's slowest repeat is faster than the ATen composition's fastest, in every cell
(``gate_fused_below_aten``).

Peak extra memory: ``torch.cuda.max_memory_allocated`` over one call, above what was allocated
before, through ``sample_tokens_from_logits(..., return_log_probs=True)`` and through the composition.

    python tests/tools/sample_timing.py [--out FILE.json]

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

K, V = 140, 256
TAU, TOP_K, TOP_P = 0.8, 50, 0.9
HBM_PEAK = 8.0e12
CACHE_BYTES = 256 << 20
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def aten_sample(l, S, truncated):
    z = l.float().view(-1, V) / TAU
    if truncated:
        kth = torch.topk(z, TOP_K)[0][..., -1, None]
        z = z.masked_fill(z < kth, float("-inf"))
        sorted_z, sorted_idx = torch.sort(z, descending=False)
        remove = sorted_z.softmax(-1).cumsum(-1) <= 1.0 - TOP_P
        remove[..., -1:] = False
        z = z.masked_fill(remove.scatter(1, sorted_idx, remove), float("-inf"))
    return torch.multinomial(torch.softmax(z, -1), S, replacement=True)


def peak_extra(fn, dev):
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize(dev)
    return torch.cuda.max_memory_allocated(dev) - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--dtypes", nargs="+", default=list(DTYPES), choices=list(DTYPES))
    ap.add_argument("--draws", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--modes", nargs="+", default=["plain", "truncated"], choices=["plain", "truncated"])
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--window-ms", type=float, default=30.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from beast_tokenizer_amd import BEASTBsplineTokenizer, _lib
    if not torch.cuda.is_available():
        raise SystemExit("sample_timing.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    stream = _lib.stream_of(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    tok = BEASTBsplineTokenizer(num_dof=14, num_basis=10, seq_len=50, vocab_size=V, device="cuda:0")
    results = []
    for name, dt in ((n, DTYPES[n]) for n in args.dtypes):
        code, size = _lib.LOGITS_DTYPES[dt], torch.empty((), dtype=dt).element_size()
        for B in args.batches:
            per_set = B * K * V * size
            n_sets = max(1, -(-2 * CACHE_BYTES // per_set))
            logits = [(torch.randn((B, K, V), device=dev, generator=gen) * 4.0).to(dt) for _ in range(n_sets)]
            for S in args.draws:
                u = torch.empty((S, B, K), device=dev)
                tokens = torch.empty((S, B, K), dtype=torch.int64, device=dev)
                logprob = torch.empty((S, B, K), device=dev)
                for mode in args.modes:
                    truncated = mode == "truncated"
                    top_k, top_p = (TOP_K, TOP_P) if truncated else (0, 1.0)

                    def fused(i):
                        u.uniform_(generator=gen)
                        _lib.check(lib.beast_sample_rows(logits[i].data_ptr(), code, B, K, V, K * V, V, TAU, top_k,
                                                         top_p, u.data_ptr(), S, 0, tokens.data_ptr(),
                                                         logprob.data_ptr(), None, stream), "beast_sample_rows")

                    def aten(i):
                        return aten_sample(logits[i], S, truncated)

                    # a guard against timing two different things, not an accuracy test: the fused draws
                    # are legal under the composition's own distribution
                    fused(0)
                    z = logits[0].float() / TAU
                    if truncated:
                        kth = torch.topk(z, TOP_K)[0][..., -1, None]
                        if not bool((z.gather(2, tokens.permute(1, 2, 0)) >= kth).all()):
                            raise SystemExit(f"a fused draw lies outside the top-k set at B={B} {name} S={S}")
                    else:
                        ref = torch.log_softmax(z, -1).gather(2, tokens.permute(1, 2, 0)).permute(2, 0, 1)
                        err = float(((logprob - ref).abs() / ref.abs().clamp(min=1.0)).max())
                        if not err < 1e-4:
                            raise SystemExit(f"fused and ATen log-probabilities disagree at B={B} {name} S={S}: {err}")
                    assert aten(0).shape == (B * K, S)
                    del z

                    variants = {"fused": fused, "aten": aten}
                    order = list(variants)

                    def window(vname, n_calls):
                        fn = variants[vname]
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for k in range(n_calls):
                            fn(k % n_sets)
                        e1.record()
                        e1.synchronize()
                        return e0.elapsed_time(e1) * 1e3 / n_calls            # us per call

                    calls = {}
                    for vname in order:                                        # warm-up, and size the windows
                        window(vname, 3)
                        us = window(vname, max(3, n_sets))
                        calls[vname] = max(n_sets, int(args.window_ms * 1e3 / us) + 1)
                    samples = {vname: [] for vname in order}
                    for _ in range(args.repeats):
                        for vname in order:
                            samples[vname].append(window(vname, calls[vname]))
                    row = {"B": B, "dtype": name, "S": S, "mode": mode, "buffer_sets": n_sets, "calls_per_window": calls}
                    for vname, v in samples.items():
                        row[vname + "_us"] = round(statistics.median(v), 3)
                        row[vname + "_us_min_max"] = [round(min(v), 3), round(max(v), 3)]
                    nbytes = per_set + S * B * K * (4 + 4 + 8 + 4)             # logits; u written + read, tokens, logprob
                    row["algorithmic_bytes"] = nbytes
                    row["hbm_fraction_of_8TBps"] = round(nbytes / (row["fused_us"] * 1e-6) / HBM_PEAK, 4)
                    row["aten_over_fused"] = round(row["aten_us"] / row["fused_us"], 3)
                    row["gate_fused_below_aten"] = max(samples["fused"]) < min(samples["aten"])

                    def fused_call():
                        tok.sample_tokens_from_logits(logits[0], temperature=TAU, top_k=top_k, top_p=top_p,
                                                      num_samples=S, return_log_probs=True)

                    fused_call()
                    row["fused_peak_extra_bytes"] = peak_extra(fused_call, dev)
                    row["aten_peak_extra_bytes"] = peak_extra(lambda: aten(0), dev)
                    row["logits_bytes"] = per_set
                    results.append(row)
                    torch.cuda.empty_cache()
                del u, tokens, logprob
            del logits
            torch.cuda.empty_cache()
    gate = all(r["gate_fused_below_aten"] for r in results)
    line = json.dumps({"tool": "sample_timing", "shape": {"K": K, "V": V}, "temperature": TAU, "top_k": TOP_K,
                       "top_p": TOP_P, "device": torch.cuda.get_device_name(0), "results": results,
                       "gate_fused_below_aten": gate})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not gate:
        raise SystemExit("gate failed: the fused sampler is not below its ATen composition by more than the spread")


if __name__ == "__main__":
    main()
