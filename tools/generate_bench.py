#!/usr/bin/env python3
"""Tokens per second of TransformerLM.generate(zeros(B, 1), N) at the scaled shape (ctx 256, C 384, 6 layers, 6 heads, V 80):
the reference's inference.py default, N = 1000 new tokens from a one-token prompt.

    python tools/generate_bench.py [--sampler host|device] [--precision fp32 bf16] [--batch 1] [--tokens 1000] [--repeats 3]
                                   [--top-p P] [--min-p P] [--vocab 80]
                                   [--repetition-penalty R] [--presence-penalty A] [--frequency-penalty F]
                                   [--prompt-lengths 4,64,128,...] [--sampler-launch]
                                   [--logprobs] [--top-logprobs N]

Two phases are reported separately.  With a one-token prompt the first ctx tokens are made while the sequence still fits the
window (one prefill, then K/V-cached steps); the rest by the sliding-window algorithm (a full forward per token).  The first
phase is timed as a call that stops at ctx tokens, the second as the difference between the full call and that one (the
per-call set-up cancels), each as the median of --repeats calls that alternate between the two lengths.
--sampler host passes no keyword that an older generate() does not have, so this file also times a commit without the device
sampler; --top-p / --min-p are passed only when given, for the same reason.  --vocab widens the vocabulary (50257: the sampler
at a GPT-2 row).  The three penalty flags are passed only when given too: with one of them the device sampler replays the
decoder's second pair of graphs (dg_sample_rows_control).  One JSON line per precision.

--logprobs / --top-logprobs N: the same call with return_logprobs=True (and top_logprobs=N): every step also scores its token
(dg_token_logprobs; with the device sampler inside the decoder's scored twin graphs).  Passed only when given.

--prompt-lengths 4,64,128,... (device sampler; the batch size is the count): one generate(prompt_lengths=...) call on right-padded
prompts of these lengths, --tokens new tokens per row, against the same prompts as separate B = 1 calls (their times summed) and
against the rectangular call on B prompts of the longest length, which has no forced steps.  Tokens per second count new tokens
only.  The three kinds of call alternate within a repeat.
--sampler-launch: no model -- the time of one sampler launch on [--batch, --vocab] logits with penalties on: dg_sample_rows_control,
dg_sample_rows_ragged with no forced row, and dg_sample_rows_ragged with every row forced (what a forced step adds), each the
median over --repeats replays of a graph of 200 such launches (no host work between them), the replays alternating between the three.
The same mode times the scoring launch alone, dg_token_logprobs in its decode form on the same logits: with top_n = 0, and with
top_n = --top-logprobs (default 5).
--score-launch: no model -- the one scoring launch of score() (dg_token_logprobs with ranks, rows = --batch, default 8192 there,
bf16 logits at --vocab) beside the loss-only dg_cross_entropy launch on the same logits, which reads the same bytes; top_n = 0 and
--top-logprobs (default 5); medians over --repeats, the kinds alternating.
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


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def ragged(args, cfg, dev):
    """--prompt-lengths: the ragged call, the same prompts one by one, and the rectangular call at the longest length"""
    if args.sampler != "device":
        raise SystemExit("--prompt-lengths times the device sampler: pass --sampler device")
    p, n = args.prompt_lengths, args.tokens
    B, V, T = len(p), args.vocab, cfg["context_length"]
    kw = dict(sampler="device", seed=1234, pad_token=0)
    for name in ("top_p", "min_p", "repetition_penalty", "presence_penalty", "frequency_penalty"):
        if getattr(args, name) is not None:
            kw[name] = getattr(args, name)
    g = torch.Generator().manual_seed(0)
    idx = torch.randint(1, V, (B, max(p)), generator=g).to(dev)
    singles = [idx[b:b + 1, :p[b]].contiguous() for b in range(B)]
    for precision in args.precision:
        torch.manual_seed(42)
        m = D.TransformerLM(V, cfg["embedding_dim"], T, cfg["num_heads"], cfg["num_layers"], cfg["dropout"], precision=precision).to(dev).eval()

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        calls = {"ragged": lambda: m.generate(idx, n, prompt_lengths=p, **kw),
                 "separate": lambda: [m.generate(s, n, **{k: v for k, v in kw.items() if k != "pad_token"}) for s in singles],
                 "rect_longest": lambda: m.generate(idx, n, **{k: v for k, v in kw.items() if k != "pad_token"})}
        for fn in calls.values():                            # warm-up: code objects, allocator, graph captures (B and 1)
            fn()
        times = {k: [] for k in calls}
        for _ in range(args.repeats):
            for k, fn in calls.items():
                times[k].append(timed(fn))
        line = {"tool": "generate_bench", "mode": "prompt_lengths", "precision": precision, "prompt_lengths": p, "vocab": V, "tokens": n,
                "ctx": T, "repeats": args.repeats, "forced_steps": max(p) - min(p)}
        for k, ts in times.items():
            line[k + "_s"] = spread(ts)
            line[k + "_new_tok_per_s"] = round(B * n / statistics.median(ts), 1)
        print(json.dumps(line), flush=True)


def sampler_launch(args, dev):
    """--sampler-launch: microseconds per launch of the control entry, the ragged entry with no forced row and with all rows forced"""
    from drakegpt_amd import ops
    M, V, L, cap = args.batch, args.vocab, 64, 128
    g = torch.Generator().manual_seed(0)
    logits = (torch.randn((M, V), generator=g) * 3).to(dev)
    ctl = ops.new_sample_control(repetition_penalty=1.3, presence_penalty=0.2, frequency_penalty=0.1, device=dev)
    params = ops.new_sample_params(1.0, None, dev, top_p=args.top_p, min_p=args.min_p, four=True)
    state = ops.new_rng_state(1234, dev, step=L)
    ids = torch.zeros((M, cap), dtype=torch.int64, device=dev)
    counts = torch.randint(0, 3, (M, V), generator=g).to(dev, torch.int32)
    lengths = torch.zeros(M, dtype=torch.int32, device=dev)
    spans = {"ragged_none_forced": torch.tensor([[1, cap]] * M, dtype=torch.int32, device=dev),
             "ragged_all_forced": torch.tensor([[L + 1, cap]] * M, dtype=torch.int32, device=dev)}
    kinds = {"control": {}, **{k: dict(spans=v) for k, v in spans.items()}}
    # the scoring launch alone: dg_token_logprobs as a decode step makes it, without and with a top-n selection
    top = args.top_logprobs or 5
    lp = torch.zeros((M, cap), dtype=torch.float32, device=dev)
    ti = torch.zeros((M, cap, ops.LOGPROBS_MAX_TOP), dtype=torch.int32, device=dev)
    tl = torch.zeros((M, cap, ops.LOGPROBS_MAX_TOP), dtype=torch.float32, device=dev)
    words = {0: torch.zeros(1, dtype=torch.int32, device=dev), top: torch.full((1,), top, dtype=torch.int32, device=dev)}
    kinds.update({"logprobs_top0": dict(score=0), f"logprobs_top{top}": dict(score=top)})

    n = 200

    def chain(kw):
        """n launches captured as one graph: a replay costs no host work between them"""
        def run():
            for _ in range(n):
                if "score" in kw:
                    ops.token_logprobs(logits, ids, state=state, lengths=lengths, out=lp, out_top_ids=ti, out_top_lp=tl,
                                       top_n=words[kw["score"]])
                else:
                    ops.sample_rows(logits, state, params, ids=ids, control=ctl, counts=counts, lengths=lengths, **kw)
        run()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            run()
        return graph

    def block(graph):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / n

    graphs = {k: chain(kw) for k, kw in kinds.items()}
    for graph in graphs.values():
        block(graph)
    us = {k: [] for k in kinds}
    for _ in range(args.repeats):
        for k, graph in graphs.items():
            us[k].append(block(graph))
    line = {"tool": "generate_bench", "mode": "sampler_launch", "batch": M, "vocab": V, "top_p": args.top_p, "min_p": args.min_p,
            "repeats": args.repeats, "launches_per_replay": n}
    line.update({k + "_us": {kk: round(v, 2) for kk, v in spread(xs).items()} for k, xs in us.items()})
    print(json.dumps(line), flush=True)


def score_launch(args, dev):
    """--score-launch: microseconds of score()'s scoring launch and of the loss-only cross entropy on the same bf16 logits"""
    from drakegpt_amd import ops
    M, V = args.batch, args.vocab
    g = torch.Generator().manual_seed(0)
    ld = (V + 7) // 8 * 8
    buf = torch.zeros((M, ld), dtype=torch.bfloat16)
    buf[:, :V] = (torch.randn((M, V), generator=g) * 2.0).bfloat16()
    logits = buf.to(dev)[:, :V]
    tok = torch.randint(0, V, (M,), generator=g).to(dev)
    top = args.top_logprobs or 5
    kinds = {"cross_entropy_loss_only": lambda: ops.cross_entropy(logits, tok, V),
             "token_logprobs_rank": lambda: ops.token_logprobs(logits, tok, rank=True),
             f"token_logprobs_rank_top{top}": lambda: ops.token_logprobs(logits, tok, rank=True, top_n=top)}

    def block(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3

    for fn in kinds.values():
        block(fn)
        block(fn)
    us = {k: [] for k in kinds}
    for _ in range(args.repeats):
        for k, fn in kinds.items():
            us[k].append(block(fn))
    line = {"tool": "generate_bench", "mode": "score_launch", "rows": M, "vocab": V, "dtype": "bf16", "repeats": args.repeats,
            "logits_gb": round(M * ld * 2e-9, 3)}
    line.update({k + "_us": {kk: round(v, 1) for kk, v in spread(xs).items()} for k, xs in us.items()})
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sampler", default="host", choices=["host", "device"])
    ap.add_argument("--precision", nargs="+", default=["fp32", "bf16"])
    ap.add_argument("--batch", type=int, default=None, help="default 1 (--score-launch: 8192 rows)")
    ap.add_argument("--tokens", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--top-p", type=float, default=None)
    ap.add_argument("--min-p", type=float, default=None)
    ap.add_argument("--vocab", type=int, default=80)
    ap.add_argument("--repetition-penalty", type=float, default=None)
    ap.add_argument("--presence-penalty", type=float, default=None)
    ap.add_argument("--frequency-penalty", type=float, default=None)
    ap.add_argument("--prompt-lengths", type=lambda s: [int(x) for x in s.split(",")], default=None)
    ap.add_argument("--sampler-launch", action="store_true")
    ap.add_argument("--score-launch", action="store_true")
    ap.add_argument("--logprobs", action="store_true")
    ap.add_argument("--top-logprobs", type=int, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("generate_bench needs the GPU: a timing taken anywhere else says nothing")
    cfg = PRESETS["scaled"]
    dev = torch.device("cuda:0")
    if args.score_launch:
        args.batch = args.batch or 8192
        return score_launch(args, dev)
    args.batch = args.batch or 1
    if args.sampler_launch:
        return sampler_launch(args, dev)
    if args.prompt_lengths is not None:
        return ragged(args, cfg, dev)
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
    if args.logprobs:
        kw["return_logprobs"] = True
    if args.top_logprobs is not None:
        kw["top_logprobs"] = args.top_logprobs
    scored = args.logprobs or bool(args.top_logprobs)
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
            assert (out.ids if scored else out).shape == (args.batch, 1 + n)
            return dt

        timed(args.tokens)                                   # warm-up: code objects, allocator, graph capture
        short, full = [], []
        for _ in range(args.repeats):
            short.append(timed(n_cached))
            full.append(timed(args.tokens))
        t_short, t_full = statistics.median(short), statistics.median(full)
        line = {"tool": "generate_bench", "sampler": args.sampler, "precision": precision, "batch": args.batch,
                "vocab": V, "top_p": args.top_p, "min_p": args.min_p, "repetition_penalty": args.repetition_penalty,
                "presence_penalty": args.presence_penalty, "frequency_penalty": args.frequency_penalty, "logprobs": scored, "top_logprobs": args.top_logprobs,
                "tokens": args.tokens, "ctx": T, "repeats": args.repeats,
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
