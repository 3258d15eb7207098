#!/usr/bin/env python3
"""Document-masked attention: what the mask costs or saves per launch and per step.

Attention at the headline shape (B 64, T 256, NH 6, H 64, p 0.2, bf16), forward and backward (dQ + dK/dV launches), for four
variants timed INTERLEAVED with HIP events (rounds x reps launches, the median over the rounds of the per-launch mean):
  plain    the plain entries (dg_attn_fwd / dg_attn_bwd)
  doc-1    the document entries with one document (starts all 0): the price of the DOC instances themselves
  doc-64   boundaries every 64 positions (on tile edges: whole tiles skipped)
  doc-37   boundaries every 37 positions (inside tiles)
The dQ / dK/dV split of the backward figure is read from the profiler's kernel table where the profiler is available (else null).
Then the scaled engine step (bf16, B 64) with and without doc_separator on a corpus with a separator about every 200 tokens, in
alternating blocks.  Prints one JSON line with the timings, then one with the profiler's split.
    python tools/docmask_bench.py [--rounds 9] [--reps 20] [--steps 100] [--no-step]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, T, NH, H, P = 64, 256, 6, 64, 0.2


def starts_every(n, dev):
    """int32 [B*T]: documents of n positions each (n = 0: one document)"""
    t = torch.arange(T, dtype=torch.int32)
    return (torch.zeros_like(t) if n == 0 else (t // n) * n).repeat(B).to(dev)


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / reps          # us per call


def kernel_split(fn, reps):
    """us per launch of the dQ and the dK/dV kernels of fn (the attention backward), from the profiler's kernel table"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        out = {"dq": 0.0, "dkv": 0.0}
        for ev in prof.key_averages():
            t = getattr(ev, "device_time_total", None)
            t = getattr(ev, "cuda_time_total", 0.0) if t is None else t
            if "attn_bwd_dq" in ev.key:
                out["dq"] += t / reps
            elif "attn_bwd_dkv" in ev.key:
                out["dkv"] += t / reps
        return {k: round(v, 2) for k, v in out.items()} if out["dq"] > 0 else None
    except Exception as e:      # noqa: BLE001  (no profiler in this build: the split is reported as not measured)
        return {"error": type(e).__name__}


def attention(dev, rounds, reps):
    from drakegpt_amd import ops
    g = torch.Generator().manual_seed(0)
    C = NH * H
    qkv = torch.randn(B * T, 3 * C, generator=g).bfloat16().to(dev)
    dout = torch.randn(B * T, C, generator=g).bfloat16().to(dev)
    rng = ops.new_rng_state(1, dev, 3)
    variants = {"plain": None, "doc-1": starts_every(0, dev), "doc-64": starts_every(64, dev), "doc-37": starts_every(37, dev)}
    fwd, bwd = {}, {}
    for nm, st in variants.items():
        kw = {} if st is None else {"doc_starts": st}
        out, lse = ops.attn_fwd(qkv, B, T, NH, H, H ** -0.5, P, rng, 4, keep=True, **kw)
        fwd[nm] = lambda kw=kw: ops.attn_fwd(qkv, B, T, NH, H, H ** -0.5, P, rng, 4, keep=True, **kw)
        bwd[nm] = lambda kw=kw, out=out, lse=lse: ops.attn_bwd(qkv, out, dout, lse, B, T, NH, H, H ** -0.5, P, rng, 4, keep_bits=out.dg_keep, **kw)
    res = {}
    for what, fns in (("forward", fwd), ("backward", bwd)):
        for fn in fns.values():
            timed(fn, 5)
        t = {nm: [] for nm in fns}
        names = list(fns)
        for r in range(rounds):                      # interleaved, rotating the order
            k = r % len(names)
            for nm in names[k:] + names[:k]:
                t[nm].append(timed(fns[nm], reps))
        res[what + "_us"] = {nm: round(statistics.median(v), 2) for nm, v in t.items()}
        res[what + "_spread_pct"] = {nm: round(100 * (max(v) - min(v)) / statistics.median(v), 1) for nm, v in t.items()}
    return res, bwd


def step(dev, rounds, steps):
    import drakegpt_amd as D
    from drakegpt_amd.config import DRAKE_VOCAB_SIZE, PRESETS
    from drakegpt_amd.engine import TrainEngine
    cfg = PRESETS["scaled"]
    V, Tc = cfg.get("vocab_size", DRAKE_VOCAB_SIZE), cfg["context_length"]
    n = 1_000_000
    corpus = torch.randint(1, V, (n,), generator=torch.Generator().manual_seed(42))
    corpus[torch.randint(0, n, (n // 200,), generator=torch.Generator().manual_seed(43))] = 0          # token 0: the separator
    engs = {}
    for nm, kw in (("default", {}), ("doc", {"doc_separator": 0}), ("default-b", {})):                 # default-b: the A/A control
        torch.manual_seed(42)
        m = D.TransformerLM(V, cfg["embedding_dim"], Tc, cfg["num_heads"], cfg["num_layers"], cfg["dropout"], precision="bf16").to(dev)
        e = TrainEngine(m, 64, Tc, lr=cfg["base_lr"], betas=cfg["betas"], seed=42, use_graph=True, **kw)
        e.set_corpus(corpus)
        gen = torch.Generator().manual_seed(42)
        e.stage_offsets(torch.stack([torch.randint(n - Tc, (64,), generator=gen) for _ in range(10 + rounds * steps)]).to(dev))
        for _ in range(10):
            e.step()
        engs[nm] = e
    t = {nm: [] for nm in engs}
    names = list(engs)
    for r in range(rounds):
        k = r % len(names)
        for nm in names[k:] + names[:k]:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(steps):
                engs[nm].step()
            torch.cuda.synchronize(dev)
            t[nm].append((time.perf_counter() - t0) / steps * 1e3)
    for e in engs.values():
        e.check_status()
    return {"step_ms": {nm: round(statistics.median(v), 4) for nm, v in t.items()},
            "step_spread_pct": {nm: round(100 * (max(v) - min(v)) / statistics.median(v), 2) for nm, v in t.items()},
            "loss": {nm: round(e.loss.item(), 4) for nm, e in engs.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=100, help="engine steps per timed block")
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"shape": [B, T, NH, H, P], "rounds": a.rounds, "reps": a.reps}
    att, bwd = attention(dev, a.rounds, a.reps)
    res.update(att)
    if not a.no_step:
        res.update(step(dev, a.rounds, a.steps))
    print(json.dumps(res), flush=True)
    print(json.dumps({"backward_split_us": {nm: kernel_split(fn, a.reps) for nm, fn in bwd.items()}}), flush=True)


if __name__ == "__main__":
    main()
