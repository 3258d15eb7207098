#!/usr/bin/env python3
"""Global-norm gradient clipping: the training step with clipping off and on (TrainEngine(max_grad_norm=...)), engines built from
the same seed, timed in alternating blocks in one process (graph replay, window offsets resident, synchronize around each block),
with a second clipping-off engine as the A/A control.  Also times the norm alone (dg_sumsq_partials + dg_grad_norm_finalize on the engine's flat gradient, captured repeats).
Prints one JSON line per configuration.
    python tools/grad_clip_bench.py [--configs scaled:bf16:64,gpt2_small:bf16:8,gpt2_medium:fp8:8] [--steps 20] [--rounds 5]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_engine(preset, precision, B, max_grad_norm, dev, n_rows):
    import drakegpt_amd as D
    from drakegpt_amd.config import DRAKE_VOCAB_SIZE, PRESETS
    from drakegpt_amd.engine import TrainEngine
    cfg = dict(PRESETS[preset])
    V, T = cfg.get("vocab_size", DRAKE_VOCAB_SIZE), cfg["context_length"]
    torch.manual_seed(42)
    model = D.TransformerLM(V, cfg["embedding_dim"], T, cfg["num_heads"], cfg["num_layers"], cfg["dropout"], precision=precision).to(dev)
    eng = TrainEngine(model, B, T, lr=cfg["base_lr"], betas=cfg["betas"], seed=42, use_graph=True, max_grad_norm=max_grad_norm)
    n_corpus = 1_000_000
    eng.set_corpus(torch.randint(0, V, (n_corpus,), generator=torch.Generator().manual_seed(42)))
    gen = torch.Generator().manual_seed(42)
    eng.stage_offsets(torch.stack([torch.randint(n_corpus - T, (B,), generator=gen) for _ in range(n_rows)]).to(dev))
    return eng, model, B * T


def time_block(eng, steps, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.step()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / steps


def norm_time(eng, reps):
    from drakegpt_amd import ops

    def fn():
        ops.grad_norm(eng.gflat, 1.0, eng.clip_state[2:3], eng.clip_state, eng.norm_work)
    fn()
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


def run(preset, precision, B, steps, warmup, rounds, reps, dev):
    # three engines: clipping off, on, and a second one off -- the A/A control: off vs off2 is what two engines of the same
    # program differ by (placement of their buffers), the floor under any off/on difference
    n_rows = warmup + rounds * steps
    names = ("off", "on", "off2")
    built = {k: make_engine(preset, precision, B, 1.0 if k == "on" else None, dev, n_rows) for k in names}
    engs = {k: v[0] for k, v in built.items()}
    tok = built["off"][2]
    for _ in range(warmup):
        for k in names:
            engs[k].step()
    t = {k: [] for k in names}
    for r in range(rounds):                      # alternate, rotating the order: drift of the box hits all alike
        for k in names[r % 3:] + names[:r % 3]:
            t[k].append(time_block(engs[k], steps, dev))
    for e in engs.values():
        e.check_status()
    med = {k: statistics.median(v) for k, v in t.items()}
    tn = norm_time(engs["on"], reps)
    n = engs["on"].n_active
    res = {"config": f"{preset} {precision} B={B}", "n_active": n, "grad_mb": 4 * n / 1e6,
           "ms_off": 1e3 * med["off"], "ms_on": 1e3 * med["on"], "ms_off2": 1e3 * med["off2"],
           "overhead_pct": 100.0 * (med["on"] - med["off"]) / med["off"],
           "control_pct": 100.0 * (med["off2"] - med["off"]) / med["off"],
           "rounds_ms": {k: [round(1e3 * x, 4) for x in v] for k, v in t.items()},
           "norm_us": 1e6 * tn, "norm_gb_per_s": 4 * n / tn / 1e9, "tokens_per_s_on": tok / med["on"],
           "last_grad_norm": engs["on"].last_grad_norm.item(), "loss_off": engs["off"].loss.item(), "loss_on": engs["on"].loss.item()}
    del engs, built
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="scaled:bf16:64,gpt2_small:bf16:8,gpt2_medium:fp8:8",
                    help="comma-separated preset:precision:batch")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for spec in args.configs.split(","):
        preset, precision, B = spec.split(":")
        print(json.dumps(run(preset, precision, int(B), args.steps, args.warmup, args.rounds, args.reps, dev)), flush=True)


if __name__ == "__main__":
    main()
