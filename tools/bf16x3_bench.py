#!/usr/bin/env python3
"""precision "bf16x3" against "fp32" and "bf16": the scaled training step (B 64, T 256, dropout 0.2, graph on) in each mode, and
the step's GEMMs one by one as exact fp32 and as split bf16 (HIP events around captured repeats).  Prints one JSON line.
    python tools/bf16x3_bench.py [--steps 30] [--warmup 5] [--reps 20]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import flops_per_token  # noqa: E402  (algorithmic FLOP per token of the headline metric)


def step_time(precision, B, steps, warmup, dev):
    import drakegpt_amd as D
    from drakegpt_amd.config import DRAKE_VOCAB_SIZE, PRESETS
    from drakegpt_amd.engine import TrainEngine
    cfg = dict(PRESETS["scaled"])
    V, T = DRAKE_VOCAB_SIZE, cfg["context_length"]
    torch.manual_seed(42)
    model = D.TransformerLM(V, cfg["embedding_dim"], T, cfg["num_heads"], cfg["num_layers"], cfg["dropout"], precision=precision).to(dev)
    eng = TrainEngine(model, B, T, lr=cfg["base_lr"], betas=cfg["betas"], seed=42, use_graph=True)
    n_corpus = 1_000_000
    eng.set_corpus(torch.randint(0, V, (n_corpus,), generator=torch.Generator().manual_seed(42)))
    gen = torch.Generator().manual_seed(42)
    eng.stage_offsets(torch.stack([torch.randint(n_corpus - T, (B,), generator=gen) for _ in range(warmup + steps)]).to(dev))
    for _ in range(warmup):
        eng.step()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.step()
    torch.cuda.synchronize(dev)
    dt = (time.perf_counter() - t0) / steps
    loss = eng.loss.item()
    eng.check_status()
    tok_s = B * T / dt
    del eng, model
    return {"ms_per_step": 1e3 * dt, "tokens_per_s": tok_s, "tflops": tok_s * flops_per_token(cfg, V) / 1e12, "final_loss": loss}


def timeit(fn, reps):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    g.replay()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e-3 / reps


def gemm_table(dev, reps):
    """the scaled step's contractions at M = B T = 16384: forward / dX as NT (N, K), dW as TN (P, Q) over the M rows"""
    from drakegpt_amd import ops
    from drakegpt_amd import sublayers as S
    from drakegpt_amd.config import DRAKE_VOCAB_SIZE
    M, V = 16384, DRAKE_VOCAB_SIZE
    gen = torch.Generator(device=dev).manual_seed(0)
    out = {}
    for name, N, K in (("qkv", 1152, 384), ("proj", 384, 384), ("ffn1", 1536, 384), ("ffn2", 384, 1536), ("lm_head", V, 384)):
        A = torch.randn((M, K), device=dev, generator=gen)
        B = torch.randn((N, K), device=dev, generator=gen)
        C = torch.empty((M, N), device=dev)
        row = {}
        for mode, split in (("fp32", False), ("bf16x3", True)):
            t = timeit(lambda: ops.gemm_nt(A, B, torch.float32, out=C, split=split), reps)
            row[mode] = {"us": 1e6 * t, "tflops": 2 * M * N * K / t / 1e12}
        row["speedup"] = row["fp32"]["us"] / row["bf16x3"]["us"]
        out[f"nt_{name}_N{N}_K{K}"] = row
        # the matching weight gradient dW[N, K] = dY[M, N]^T X[M, K], split-K slabs as the fp32 program launches it
        dY = torch.randn((M, N), device=dev, generator=gen)
        n = S.splits_for_matrix(N, K, M, S.n_splits_for(M), dev)
        part = torch.empty((n, N * K), device=dev)
        row = {"n_splits": n}
        for mode, split in (("fp32", False), ("bf16x3", True)):
            t = timeit(lambda: ops.gemm_tn(dY, A, part, N * K, n, N, K, split=split), reps)
            row[mode] = {"us": 1e6 * t, "tflops": 2 * M * N * K / t / 1e12}
        row["speedup"] = row["fp32"]["us"] / row["bf16x3"]["us"]
        out[f"tn_{name}_P{N}_Q{K}"] = row
        del A, B, C, dY, part
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    steps = {p: step_time(p, args.batch, args.steps, args.warmup, dev) for p in ("fp32", "bf16x3", "bf16")}
    res = {"workload": f"TransformerLM_scaled B={args.batch} T=256 dropout=0.2 hipGraph=on; fwd+bwd+AdamW",
           "steps": steps, "bf16x3_over_fp32_tokens_per_s": steps["bf16x3"]["tokens_per_s"] / steps["fp32"]["tokens_per_s"],
           "gemms": gemm_table(dev, args.reps)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
