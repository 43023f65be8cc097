"""Time the fused scoring of tokens against what a user could write without it.

At the default shape (K 140 = N 10 x D 14 tokens, V 256), B = 256 and 4,096, fp32 and bf16, S = 1 and
16 scored tokens per row, plain (temperature only) and truncated (top_k 50, top_p 0.9), temperature
0.8, always with a reference: log-probabilities, entropy and KL, forward alone and forward + backward.
  (a) fused: one beast_score_rows launch (forward), plus one beast_score_rows_bwd launch for the
      gradient of all three (forward + backward; the forward then also writes the row statistics);
  (b) the ATen composition: ``log_softmax(l.float() / tau)`` -- behind the usual sort-based warpers when
      truncated: topk -> masked_fill, sort -> softmax -> cumsum -> mask -> scatter -> masked_fill --
      then gather, ``-(p * log p).sum(-1)`` and ``(p * (log p - log_softmax(ref.float() / tau))).sum(-1)``;
      forward + backward is its autograd from the same three upstream gradients into ``l.grad``.

The protocol is tests/tools/sample_timing.py's: HIP events around windows of back-to-back calls (each
window at least ``--window-ms`` of work), after a warm-up of every variant; the variants alternate
inside each repeat and the median over the repeats is reported with the minimum and maximum.  The
buffers rotate over enough copies that the working set exceeds twice the 256 MB of last-level cache.
The fused kernels' share of the 8 TB/s HBM peak is their algorithmic bytes over their time -- forward:
the logits and the reference rows read once, the tokens read, the outputs written; backward: both rows
read once more, the gradient written once, tokens, upstream gradients and statistics read.  The gate:
the fused variant's slowest repeat is faster than the ATen composition's fastest, in every cell and in
both directions (``gate_fused_below_aten``).

Peak extra memory: ``torch.cuda.max_memory_allocated`` over one forward + backward, above what was
allocated before, through ``score_tokens_from_logits`` and through the composition.

    python tests/tools/score_timing.py [--out FILE.json]

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
NEG_INF = float("-inf")


def aten_scores(l, ref, tok, truncated):
    """(logprob [S, B, K], entropy [B, K], kl [B, K]) as a user would compose them."""
    z = l.float() / TAU
    if truncated:
        flat = z.view(-1, V)
        kth = torch.topk(flat, TOP_K)[0][..., -1, None]
        masked = flat.masked_fill(flat < kth, NEG_INF)
        sorted_z, sorted_idx = torch.sort(masked, descending=False)
        remove = sorted_z.softmax(-1).cumsum(-1) <= 1.0 - TOP_P
        remove[..., -1:] = False
        z = masked.masked_fill(remove.scatter(1, sorted_idx, remove), NEG_INF).view(z.shape)
    lp = torch.log_softmax(z, -1)
    logprob = lp.gather(2, tok.permute(1, 2, 0)).permute(2, 0, 1)
    p = lp.exp()
    safe = lp.masked_fill(lp == NEG_INF, 0.0)
    entropy = -(p * safe).sum(-1)
    kl = (p * (safe - torch.log_softmax(ref.float() / TAU, -1))).sum(-1)
    return logprob, entropy, kl


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
    from beast_tokenizer_amd.beast_bspline_tokenizer import SCORE_STATS
    if not torch.cuda.is_available():
        raise SystemExit("score_timing.py needs a GPU: nothing is measured without one")
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
            n_sets = max(1, -(-2 * CACHE_BYTES // (2 * per_set)))           # logits and reference rotate together
            logits = [(torch.randn((B, K, V), device=dev, generator=gen) * 4.0).to(dt) for _ in range(n_sets)]
            refs = [(torch.randn((B, K, V), device=dev, generator=gen) * 4.0).to(dt) for _ in range(n_sets)]
            leaves = [l.clone().requires_grad_() for l in logits]
            grad = torch.empty((B, K, V), dtype=dt, device=dev)
            entropy, kl = torch.empty((B, K), device=dev), torch.empty((B, K), device=dev)
            stats = torch.empty((B, K, SCORE_STATS), device=dev)
            g_h, g_kl = torch.randn((B, K), device=dev, generator=gen), torch.randn((B, K), device=dev, generator=gen)
            for S in args.draws:
                logprob = torch.empty((S, B, K), device=dev)
                g_lp = torch.randn((S, B, K), device=dev, generator=gen)
                for mode in args.modes:
                    truncated = mode == "truncated"
                    top_k, top_p = (TOP_K, TOP_P) if truncated else (0, 1.0)
                    # tokens the policy itself drew: inside the kept set of every buffer set's own rows
                    tokens = [tok.sample_tokens_from_logits(l, temperature=TAU, top_k=top_k, top_p=top_p, num_samples=S)
                              for l in logits]

                    def head(i):
                        return (logits[i].data_ptr(), code, B, K, V, K * V, V, refs[i].data_ptr(), K * V, V, TAU, top_k,
                                top_p, tokens[i].data_ptr(), S, 0, -100)

                    def fused_fwd(i, st=None):
                        _lib.check(lib.beast_score_rows(*head(i), logprob.data_ptr(), entropy.data_ptr(), kl.data_ptr(),
                                                        None, st, stream), "beast_score_rows")

                    def fused_fb(i):
                        fused_fwd(i, stats.data_ptr())
                        _lib.check(lib.beast_score_rows_bwd(*head(i), stats.data_ptr(), g_lp.data_ptr(), g_h.data_ptr(),
                                                            g_kl.data_ptr(), grad.data_ptr(), K * V, V, stream),
                                   "beast_score_rows_bwd")

                    def aten_fwd(i):
                        with torch.no_grad():
                            return aten_scores(logits[i], refs[i], tokens[i], truncated)

                    def aten_fb(i):
                        leaves[i].grad = None
                        lp_, h_, kl_ = aten_scores(leaves[i], refs[i], tokens[i], truncated)
                        torch.autograd.backward([lp_, h_, kl_], [g_lp, g_h, g_kl])
                        return leaves[i].grad

                    # a guard against timing two different things, not an accuracy test
                    fused_fb(0)
                    want = aten_fwd(0)
                    want_grad = aten_fb(0).float()
                    tol = 1e-4 if not truncated else 1e-3
                    for what, got, ref_ in (("logprob", logprob, want[0]), ("entropy", entropy, want[1]),
                                            ("kl", kl, want[2])):
                        err = float(((got - ref_).abs() / ref_.abs().clamp(min=1.0)).median())
                        if not err < tol:
                            raise SystemExit(f"fused and ATen {what} disagree at B={B} {name} S={S} {mode}: {err}")
                    err = float((grad.float() - want_grad).abs().median())
                    if not err < (1e-2 if dt is torch.bfloat16 else 1e-4):
                        raise SystemExit(f"fused and ATen gradients disagree at B={B} {name} S={S} {mode}: {err}")
                    del want, want_grad

                    variants = {"fused_fwd": fused_fwd, "aten_fwd": aten_fwd, "fused_fb": fused_fb, "aten_fb": aten_fb}
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
                    rows = B * K
                    fwd_bytes = 2 * per_set + rows * (S * (8 + 4) + 4 + 4)      # rows + reference; tokens; outputs
                    bwd_bytes = 3 * per_set + rows * (S * (8 + 4) + 4 + 4 + 4 * SCORE_STATS)
                    fb_bytes = fwd_bytes + rows * 4 * SCORE_STATS + bwd_bytes
                    row["forward_algorithmic_bytes"] = fwd_bytes
                    row["forward_backward_algorithmic_bytes"] = fb_bytes
                    row["forward_hbm_fraction_of_8TBps"] = round(fwd_bytes / (row["fused_fwd_us"] * 1e-6) / HBM_PEAK, 4)
                    row["forward_backward_hbm_fraction_of_8TBps"] = round(fb_bytes / (row["fused_fb_us"] * 1e-6)
                                                                          / HBM_PEAK, 4)
                    row["aten_over_fused_fwd"] = round(row["aten_fwd_us"] / row["fused_fwd_us"], 3)
                    row["aten_over_fused_fb"] = round(row["aten_fb_us"] / row["fused_fb_us"], 3)
                    row["gate_fused_below_aten"] = (max(samples["fused_fwd"]) < min(samples["aten_fwd"])
                                                    and max(samples["fused_fb"]) < min(samples["aten_fb"]))

                    def fused_call():
                        leaves[0].grad = None
                        out = tok.score_tokens_from_logits(leaves[0], tokens[0], temperature=TAU, top_k=top_k,
                                                           top_p=top_p, ref_logits=refs[0], return_entropy=True)
                        torch.autograd.backward(list(out), [g_lp, g_h, g_kl])

                    fused_call()
                    row["fused_peak_extra_bytes"] = peak_extra(fused_call, dev)
                    row["aten_peak_extra_bytes"] = peak_extra(lambda: aten_fb(0), dev)
                    row["logits_bytes"] = per_set
                    for leaf in leaves:
                        leaf.grad = None
                    results.append(row)
                    del tokens
                    torch.cuda.empty_cache()
                del logprob, g_lp
            del logits, refs, leaves, grad, stats
            torch.cuda.empty_cache()
    gate = all(r["gate_fused_below_aten"] for r in results)
    line = json.dumps({"tool": "score_timing", "shape": {"K": K, "V": V}, "temperature": TAU, "top_k": TOP_K,
                       "top_p": TOP_P, "device": torch.cuda.get_device_name(0), "results": results,
                       "gate_fused_below_aten": gate})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not gate:
        raise SystemExit("gate failed: the fused scoring is not below its ATen composition by more than the spread")


if __name__ == "__main__":
    main()
