#!/usr/bin/env python3
"""Tokens per second of TransformerLM.generate(zeros(B, 1), N) at the scaled shape (ctx 256, C 384, 6 layers, 6 heads, V 80):
the reference's inference.py default, N = 1000 new tokens from a one-token prompt.

    python tools/generate_bench.py [--sampler host|device] [--precision fp32 bf16] [--batch 1] [--tokens 1000] [--repeats 3]
                                   [--top-p P] [--min-p P] [--vocab 80]
                                   [--repetition-penalty R] [--presence-penalty A] [--frequency-penalty F]

Two phases are reported separately.  With a one-token prompt the first ctx tokens are made while the sequence still fits the
window (one prefill, then K/V-cached steps); the rest by the sliding-window algorithm (a full forward per token).  The first
phase is timed as a call that stops at ctx tokens, the second as the difference between the full call and that one (the
per-call set-up cancels), each as the median of --repeats calls that alternate between the two lengths.
--sampler host passes no keyword that an older generate() does not have, so this file also times a commit without the device
sampler; --top-p / --min-p are passed only when given, for the same reason.  --vocab widens the vocabulary (50257: the sampler
at a GPT-2 row).  The three penalty flags are passed only when given too: with one of them the device sampler replays the
decoder's second pair of graphs (dg_sample_rows_control).  One JSON line per precision.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import drakegpt_amd as D  # noqa: E402
from drakegpt_amd.config import PRESETS  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sampler", default="host", choices=["host", "device"])
    ap.add_argument("--precision", nargs="+", default=["fp32", "bf16"])
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--tokens", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--top-p", type=float, default=None)
    ap.add_argument("--min-p", type=float, default=None)
    ap.add_argument("--vocab", type=int, default=80)
    ap.add_argument("--repetition-penalty", type=float, default=None)
    ap.add_argument("--presence-penalty", type=float, default=None)
    ap.add_argument("--frequency-penalty", type=float, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("generate_bench needs the GPU: a timing taken anywhere else says nothing")
    cfg = PRESETS["scaled"]
    dev = torch.device("cuda:0")
    V, C, T, NH, NL = args.vocab, cfg["embedding_dim"], cfg["context_length"], cfg["num_heads"], cfg["num_layers"]
    n_cached = min(args.tokens, T)
    kw = {} if args.sampler == "host" else dict(sampler="device", seed=1234)
    if args.top_p is not None:
        kw["top_p"] = args.top_p
    if args.min_p is not None:
        kw["min_p"] = args.min_p
    for name in ("repetition_penalty", "presence_penalty", "frequency_penalty"):
        if getattr(args, name) is not None:
            kw[name] = getattr(args, name)
    for precision in args.precision:
        torch.manual_seed(42)
        m = D.TransformerLM(V, C, T, NH, NL, cfg["dropout"], precision=precision).to(dev).eval()
        start = torch.zeros((args.batch, 1), dtype=torch.long, device=dev)

        def timed(n):
            torch.manual_seed(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = m.generate(start, n, **kw)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert out.shape == (args.batch, 1 + n)
            return dt

        timed(args.tokens)                                   # warm-up: code objects, allocator, graph capture
        short, full = [], []
        for _ in range(args.repeats):
            short.append(timed(n_cached))
            full.append(timed(args.tokens))
        t_short, t_full = statistics.median(short), statistics.median(full)
        line = {"tool": "generate_bench", "sampler": args.sampler, "precision": precision, "batch": args.batch,
                "vocab": V, "top_p": args.top_p, "min_p": args.min_p, "repetition_penalty": args.repetition_penalty,
                "presence_penalty": args.presence_penalty, "frequency_penalty": args.frequency_penalty, "tokens": args.tokens, "ctx": T, "repeats": args.repeats,
                "total_s": round(t_full, 4), "total_tok_per_s": round(args.batch * args.tokens / t_full, 1),
                "cached_tokens": n_cached, "cached_s": round(t_short, 4),
                "cached_tok_per_s": round(args.batch * n_cached / t_short, 1),
                "total_s_all": [round(x, 4) for x in full], "cached_s_all": [round(x, 4) for x in short]}
        if args.tokens > n_cached:
            line["sliding_tokens"] = args.tokens - n_cached
            line["sliding_s"] = round(t_full - t_short, 4)
            line["sliding_tok_per_s"] = round(args.batch * (args.tokens - n_cached) / (t_full - t_short), 1)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
