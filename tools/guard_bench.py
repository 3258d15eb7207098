#!/usr/bin/env python3
"""The update guard: the training step with the guard off and on (TrainEngine(skip_nonfinite=True)), engines built from the same
seed, timed in alternating blocks in one process (graph replay, window offsets resident, synchronize around each block), with a
second guard-off engine as the A/A control -- once without and once with gradient clipping, where the guard adds no launch.  A
fourth engine runs with the device-side limit at 0, so that every step is skipped: what a skipped step costs (the
forward / backward still run; the AdamW launch streams nothing).
Prints one JSON line per configuration.
    python tools/guard_bench.py [--configs scaled:bf16:64] [--steps 20] [--rounds 5]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_engine(preset, precision, B, dev, n_rows, **kw):
    import drakegpt_amd as D
    from drakegpt_amd.config import DRAKE_VOCAB_SIZE, PRESETS
    from drakegpt_amd.engine import TrainEngine
    cfg = dict(PRESETS[preset])
    V, T = cfg.get("vocab_size", DRAKE_VOCAB_SIZE), cfg["context_length"]
    torch.manual_seed(42)
    model = D.TransformerLM(V, cfg["embedding_dim"], T, cfg["num_heads"], cfg["num_layers"], cfg["dropout"], precision=precision).to(dev)
    eng = TrainEngine(model, B, T, lr=cfg["base_lr"], betas=cfg["betas"], seed=42, use_graph=True, **kw)
    n_corpus = 1_000_000
    eng.set_corpus(torch.randint(0, V, (n_corpus,), generator=torch.Generator().manual_seed(42)))
    gen = torch.Generator().manual_seed(42)
    eng.stage_offsets(torch.stack([torch.randint(n_corpus - T, (B,), generator=gen) for _ in range(n_rows)]).to(dev))
    return eng


def time_block(eng, steps, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.step()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / steps


def run(preset, precision, B, clip, steps, warmup, rounds, dev):
    n_rows = warmup + rounds * steps
    base = {} if clip is None else {"max_grad_norm": clip}
    names = ("off", "on", "off2", "skip_all")
    kws = {"off": {}, "on": {"skip_nonfinite": True}, "off2": {}, "skip_all": {"skip_nonfinite": True}}
    engs = {k: make_engine(preset, precision, B, dev, n_rows, **base, **kws[k]) for k in names}
    engs["skip_all"].guard_limit.fill_(0.0)          # (below what set_skip_grad_norm accepts: no norm of a real gradient passes)
    for _ in range(warmup):
        for k in names:
            engs[k].step()
    t = {k: [] for k in names}
    for r in range(rounds):                      # alternate, rotating the order: drift of the box hits all alike
        for k in names[r % 4:] + names[:r % 4]:
            t[k].append(time_block(engs[k], steps, dev))
    for e in engs.values():
        e.check_status()
    med = {k: statistics.median(v) for k, v in t.items()}
    n = engs["on"].n_active
    res = {"config": f"{preset} {precision} B={B}", "max_grad_norm": clip, "n_active": n, "grad_mb": 4 * n / 1e6,
           "ms_off": 1e3 * med["off"], "ms_on": 1e3 * med["on"], "ms_off2": 1e3 * med["off2"], "ms_skip_all": 1e3 * med["skip_all"],
           "guard_us": 1e6 * (med["on"] - med["off"]), "control_us": 1e6 * (med["off2"] - med["off"]),
           "skipped_step_saves_us": 1e6 * (med["on"] - med["skip_all"]),
           "overhead_pct": 100.0 * (med["on"] - med["off"]) / med["off"],
           "control_pct": 100.0 * (med["off2"] - med["off"]) / med["off"],
           "rounds_ms": {k: [round(1e3 * x, 4) for x in v] for k, v in t.items()},
           "skipped_on": engs["on"].skipped_steps(), "skipped_skip_all": engs["skip_all"].skipped_steps(),
           "steps_skip_all": engs["skip_all"].step_count(), "micro_steps_skip_all": engs["skip_all"].micro_step_count(),
           "last_grad_norm": engs["on"].last_grad_norm.item(), "loss_off": engs["off"].loss.item(), "loss_on": engs["on"].loss.item()}
    del engs
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="scaled:bf16:64", help="comma-separated preset:precision:batch")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for spec in args.configs.split(","):
        preset, precision, B = spec.split(":")
        for clip in (None, 1.0):
            print(json.dumps(run(preset, precision, int(B), clip, args.steps, args.warmup, args.rounds, dev)), flush=True)


if __name__ == "__main__":
    main()
