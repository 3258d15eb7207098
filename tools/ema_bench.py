#!/usr/bin/env python3
"""What the moving average of the weights costs: the AdamW launch and the captured training step with and without ema_decay.

Launch (per preset, at the flat size of its engine): variants timed in one process in rotating order (HIP events around `reps`
back-to-back launches, warmed up, several rounds each; median and spread per variant):
    a  dg_adamw_step of ANOTHER build of the library (--parent-lib PATH: e.g. the parent commit's libdrakegpt_hip.so); skipped
       without the flag
    b  dg_adamw_step of this tree (bf16 shadow, advance on: 28 + 2 B per parameter)
    b2 the same again: the A/A control, what one program differs from itself by
    e  dg_adamw_step_ema (decay 0.999): one more fp32 stream, 36 + 2 B per parameter
Step (--step-presets, default the scaled shape in bf16 at B 64): three engines built from the same seed -- two without ema_decay
(`plain`, and `plain2` as the A/A control) and one with it -- their captured steps replayed in blocks of `step-reps`, interleaved,
HIP events around every block; median per engine.
Prints one JSON line per measurement.
    python tools/ema_bench.py [--presets scaled,gpt2_medium] [--step-presets scaled] [--reps 20] [--rounds 9] [--parent-lib PATH]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.adamw_sched_bench import flat_layout  # noqa: E402


def _timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps          # us per call


def _rotate(variants, reps, rounds):
    names = list(variants)
    t = {nm: [] for nm in names}
    for r in range(rounds):
        s = r % len(names)
        for nm in names[s:] + names[:s]:
            t[nm].append(_timed(variants[nm], reps))
    return t


def launch_bench(preset, args, parent, dev):
    from drakegpt_amd import ops
    from drakegpt_amd.config import DRAKE_VOCAB_SIZE, PRESETS
    cfg = PRESETS[preset]
    n = sum(flat_layout(cfg, cfg.get("vocab_size", DRAKE_VOCAB_SIZE)))
    g = torch.Generator().manual_seed(1)
    p = torch.randn(n, generator=g).to(dev)
    gr = (0.01 * torch.randn(n, generator=g)).to(dev)
    m, v, ema = torch.zeros_like(p), torch.zeros_like(p), p.clone()
    shadow = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    hyper = torch.tensor([3e-4, 0.9, 0.95, 1e-8, 0.1], device=dev)
    state = ops.new_rng_state(1, dev, 1)
    ema_hyper = ops.new_ema_hyper(0.999, False, dev)

    def old(lib):
        def fn():
            ops.check(lib.dg_adamw_step(ops._p(p), ops._p(gr), ops._p(m), ops._p(v), n, ops._p(hyper), ops._p(state), 1.0, ops._p(shadow), 1,
                                        ops._stream()), "dg_adamw_step")
        return fn

    def with_ema():
        ops.adamw_step(p, gr, m, v, hyper, state, 1.0, shadow_bf16=shadow, n=n, advance=True, ema=ema, ema_hyper=ema_hyper)
    variants = {"b": old(ops.lib), "b2": old(ops.lib), "e": with_ema}
    if parent is not None:
        variants = {"a": old(parent), **variants}
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = _rotate(variants, args.reps, args.rounds)
    med = {nm: statistics.median(x) for nm, x in t.items()}
    nbytes = {nm: (38 if nm == "e" else 30) * n for nm in t}
    print(json.dumps({"what": "adamw_launch", "preset": preset, "n": n, "reps": args.reps, "rounds": args.rounds,
                      "us_median": {nm: round(x, 2) for nm, x in med.items()},
                      "us_min": {nm: round(min(x), 2) for nm, x in t.items()}, "us_max": {nm: round(max(x), 2) for nm, x in t.items()},
                      "gb_per_s": {nm: round(nbytes[nm] / med[nm] / 1e3, 1) for nm in t},
                      "ema_over_plain": round(med["e"] / med["b"], 3)}), flush=True)


def step_bench(preset, args, dev):
    import drakegpt_amd as D
    from drakegpt_amd.config import DRAKE_VOCAB_SIZE, PRESETS
    from drakegpt_amd.engine import TrainEngine
    cfg = PRESETS[preset]
    V, T, B = cfg.get("vocab_size", DRAKE_VOCAB_SIZE), cfg["context_length"], args.batch or cfg["batch_size"]
    n_corpus = 1_000_000 if V <= 256 else 10_000_000
    corpus = torch.randint(0, V, (n_corpus,), generator=torch.Generator().manual_seed(42))
    total = 3 + args.step_reps * args.rounds
    offs = torch.stack([torch.randint(n_corpus - T, (B,), generator=torch.Generator().manual_seed(7 + i)) for i in range(total)]).to(dev)
    engines = {}
    for name, kw in (("plain", {}), ("plain2", {}), ("ema", {"ema_decay": 0.999})):
        torch.manual_seed(42)
        model = D.TransformerLM(V, cfg["embedding_dim"], T, cfg["num_heads"], cfg["num_layers"], cfg["dropout"], precision=args.precision).to(dev)
        eng = TrainEngine(model, B, T, lr=cfg["base_lr"], betas=cfg["betas"], seed=42, **kw)
        eng.set_corpus(corpus)
        eng.stage_offsets(offs)
        for _ in range(3):
            eng.step()
        engines[name] = eng
    torch.cuda.synchronize()
    t = _rotate({nm: e.step for nm, e in engines.items()}, args.step_reps, args.rounds)
    for e in engines.values():
        e.check_status()
    med = {nm: statistics.median(x) for nm, x in t.items()}
    print(json.dumps({"what": "captured_step", "preset": preset, "precision": args.precision, "batch": B, "n_active": engines["ema"].n_active,
                      "reps": args.step_reps, "rounds": args.rounds, "us_median": {nm: round(x, 1) for nm, x in med.items()},
                      "us_min": {nm: round(min(x), 1) for nm, x in t.items()}, "us_max": {nm: round(max(x), 1) for nm, x in t.items()},
                      "ema_minus_plain_us": round(med["ema"] - med["plain"], 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--presets", default="scaled,gpt2_medium")
    ap.add_argument("--step-presets", default="scaled")
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step-reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()
    from drakegpt_amd import _lib
    dev = torch.device("cuda:0")
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        parent.dg_adamw_step.argtypes = _lib.SIGNATURES["dg_adamw_step"]
        parent.dg_adamw_step.restype = ctypes.c_int
    for preset in filter(None, args.presets.split(",")):
        launch_bench(preset, args, parent, dev)
    for preset in filter(None, args.step_presets.split(",")):
        step_bench(preset, args, dev)


if __name__ == "__main__":
    main()
