#!/usr/bin/env python3
"""Gradient accumulation: tokens/s of the training step at accum_steps k in {1, 2, 4, 8} (TrainEngine(accum_steps=k)), engines built
from the same seed, timed in alternating blocks of the same number of MICRO-batches in one process (graph replay, window offsets
resident, synchronize around each block), with a second k = 1 engine as the A/A control.  Also times the accumulate launch alone
(dg_grad_accumulate on the engine's flat gradient, captured repeats, the 12 B/param form).  Prints one JSON line.
--tree DIR imports the package from another checkout of this project (an older one has no accum_steps: run it with --ks 1), so that
a baseline can be measured by the same script in the same session:
    python tools/accum_bench.py [--config scaled:bf16:64] [--ks 1,2,4,8] [--micro 256] [--rounds 7] [--tree DIR]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

TREE = None


def make_engine(preset, precision, B, k, dev, n_rows):
    import drakegpt_amd as D
    from drakegpt_amd.config import DRAKE_VOCAB_SIZE, PRESETS
    from drakegpt_amd.engine import TrainEngine
    cfg = dict(PRESETS[preset])
    V, T = cfg.get("vocab_size", DRAKE_VOCAB_SIZE), cfg["context_length"]
    torch.manual_seed(42)
    model = D.TransformerLM(V, cfg["embedding_dim"], T, cfg["num_heads"], cfg["num_layers"], cfg["dropout"], precision=precision).to(dev)
    kw = {"accum_steps": k} if k > 1 else {}            # k = 1 is the engine built without the argument (the same graphs)
    eng = TrainEngine(model, B, T, lr=cfg["base_lr"], betas=cfg["betas"], seed=42, use_graph=True, **kw)
    n_corpus = 1_000_000
    eng.set_corpus(torch.randint(0, V, (n_corpus,), generator=torch.Generator().manual_seed(42)))
    gen = torch.Generator().manual_seed(42)
    eng.stage_offsets(torch.stack([torch.randint(n_corpus - T, (B,), generator=gen) for _ in range(n_rows)]).to(dev))
    return eng, model, B * T


def time_block(eng, k, micro, dev):
    """seconds per micro-batch over micro / k optimizer steps"""
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(micro // k):
        eng.step()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / micro


def accumulate_time(eng, reps):
    from drakegpt_amd import ops
    acc = torch.zeros_like(eng.gflat)
    ctl = ops.new_accum_ctl(1 << 20, eng.dev)               # j > 0 from the second launch on: acc = acc + g, 12 B/param
    loss_out = torch.zeros(2, dtype=torch.float32, device=eng.dev)

    def fn():
        ops.grad_accumulate(acc, eng.gflat, eng.n_active, ctl, eng.loss, loss_out)
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


def run(preset, precision, B, ks, micro, warmup, rounds, reps, dev):
    lcm = 1
    for k in ks:
        lcm = lcm * k // math.gcd(lcm, k)
    micro = (micro + lcm - 1) // lcm * lcm
    n_rows = lcm * ((warmup + lcm - 1) // lcm) + rounds * micro
    names = [f"k{k}" for k in ks] + ["k1b"]              # k1b: the A/A control -- what two engines of the same program differ by
    kof = {**{f"k{k}": k for k in ks}, "k1b": 1}
    built = {nm: make_engine(preset, precision, B, kof[nm], dev, n_rows) for nm in names}
    engs = {nm: v[0] for nm, v in built.items()}
    tok = built[names[0]][2]
    for nm in names:
        for _ in range((warmup + lcm - 1) // lcm * lcm // kof[nm]):
            engs[nm].step()
    t = {nm: [] for nm in names}
    for r in range(rounds):                              # alternate, rotating the order: drift of the box hits all alike
        s = r % len(names)
        for nm in names[s:] + names[:s]:
            t[nm].append(time_block(engs[nm], kof[nm], micro, dev))
    for e in engs.values():
        e.check_status()
    med = {nm: statistics.median(v) for nm, v in t.items()}
    n = engs[names[0]].n_active
    res = {"config": f"{preset} {precision} B={B}", "tree": os.path.abspath(TREE), "n_active": n, "micro_batches_per_block": micro,
           "ms_per_micro_batch": {nm: round(1e3 * med[nm], 5) for nm in names},
           "tokens_per_s": {nm: round(tok / med[nm]) for nm in names},
           "spread_pct": {nm: round(100.0 * (max(v) - min(v)) / med[nm], 3) for nm, v in t.items()},
           "rounds_ms": {nm: [round(1e3 * x, 4) for x in v] for nm, v in t.items()},
           "loss": {nm: round(engs[nm].loss.item(), 5) for nm in names}}
    from drakegpt_amd import ops
    if hasattr(ops, "grad_accumulate"):              # (absent in a --tree from before the feature)
        ta = accumulate_time(engs[names[0]], reps)
        res.update(accumulate_us=round(1e6 * ta, 3), accumulate_gb_per_s=round(12 * n / ta / 1e9, 1))
    return res


def main():
    global TREE
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="scaled:bf16:64", help="preset:precision:batch")
    ap.add_argument("--ks", default="1,2,4,8")
    ap.add_argument("--micro", type=int, default=256, help="micro-batches per timed block (rounded up to a multiple of every k)")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    TREE = args.tree
    sys.path.insert(0, os.path.abspath(TREE))
    dev = torch.device("cuda:0")
    preset, precision, B = args.config.split(":")
    ks = [int(k) for k in args.ks.split(",")]
    print(json.dumps(run(preset, precision, int(B), ks, args.micro, args.warmup, args.rounds, args.reps, dev)), flush=True)


if __name__ == "__main__":
    main()
