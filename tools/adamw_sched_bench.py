#!/usr/bin/env python3
"""AdamW launch time with and without the learning-rate table and the no-decay bitmap (dg_adamw_step_sched), at the flat sizes of
the engine's presets.  Variants, timed in one process in rotating order (HIP events around `reps` back-to-back launches, warmed
up, several rounds each; median and spread per variant):
    a  dg_adamw_step of ANOTHER build of the library (--parent-lib PATH: e.g. the parent commit's libdrakegpt_hip.so); skipped
       without the flag
    b  dg_adamw_step of this tree
    b2 the same again: the A/A control, what one program differs from itself by
    c  dg_adamw_step_sched with a table and the bitmap TrainEngine(no_decay=("bias", "layernorm")) builds (the bias / LayerNorm
       section of the flat buffer)
    d  the same with every other granule masked (the least uniform bitmap)
All variants update the same buffers (bf16 shadow included, advance on), 28 + 2 B per parameter.  Prints one JSON line per size.
    python tools/adamw_sched_bench.py [--presets scaled,gpt2_medium] [--reps 20] [--rounds 9] [--parent-lib PATH]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _round(n, a=64):
    return (n + a - 1) // a * a


def flat_layout(cfg, V):
    """(matrices, vectors, embeddings) sizes of TrainEngine's flat buffer (engine._build_layout restated)"""
    C, L, T = cfg["embedding_dim"], cfg["num_layers"], cfg["context_length"]
    A = L * (_round(3 * C * C) + _round(C * C) + 2 * _round(4 * C * C)) + _round(V * C)
    Bv = L * (6 * _round(C) + _round(4 * C)) + _round(V)
    E = _round(V * C) + _round(T * C)
    return A, Bv, E


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--presets", default="scaled,gpt2_medium")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()
    from drakegpt_amd import _lib, ops
    from drakegpt_amd.config import DRAKE_VOCAB_SIZE, PRESETS
    dev = torch.device("cuda:0")
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        parent.dg_adamw_step.argtypes = _lib.SIGNATURES["dg_adamw_step"]
        parent.dg_adamw_step.restype = ctypes.c_int
    for preset in args.presets.split(","):
        cfg = PRESETS[preset]
        A, Bv, E = flat_layout(cfg, cfg.get("vocab_size", DRAKE_VOCAB_SIZE))
        n = A + Bv + E
        g = torch.Generator().manual_seed(1)
        p = torch.randn(n, generator=g).to(dev)
        gr = (0.01 * torch.randn(n, generator=g)).to(dev)
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        shadow = torch.zeros(n, dtype=torch.bfloat16, device=dev)
        hyper = torch.tensor([3e-4, 0.9, 0.95, 1e-8, 0.1], device=dev)
        state = ops.new_rng_state(1, dev, 0)
        table = torch.full((10000,), 3e-4, device=dev)
        bits_groups = ops.new_no_decay_bits([(A, A + Bv)], n, dev)
        bits_alt = torch.full((ops.no_decay_words(n),), 0x55555555, dtype=torch.int32, device=dev)

        def old(lib):
            def fn():
                ops.check(lib.dg_adamw_step(ops._p(p), ops._p(gr), ops._p(m), ops._p(v), n, ops._p(hyper), ops._p(state), 1.0, ops._p(shadow), 1,
                                            ops._stream()), "dg_adamw_step")
            return fn

        def sched(bits):
            return lambda: ops.adamw_step(p, gr, m, v, hyper, state, 1.0, shadow_bf16=shadow, n=n, advance=True, lr_table=table,
                                          no_decay_bits=bits)
        variants = {"b": old(ops.lib), "b2": old(ops.lib), "c": sched(bits_groups), "d": sched(bits_alt)}
        if parent is not None:
            variants = {"a": old(parent), **variants}
        names = list(variants)
        for fn in variants.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        t = {nm: [] for nm in names}
        for r in range(args.rounds):
            s = r % len(names)
            for nm in names[s:] + names[:s]:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    variants[nm]()
                e1.record()
                e1.synchronize()
                t[nm].append(e0.elapsed_time(e1) * 1e3 / args.reps)
        med = {nm: statistics.median(x) for nm, x in t.items()}
        print(json.dumps({"preset": preset, "n": n, "reps": args.reps, "rounds": args.rounds,
                          "us_median": {nm: round(med[nm], 2) for nm in names},
                          "us_min": {nm: round(min(x), 2) for nm, x in t.items()}, "us_max": {nm: round(max(x), 2) for nm, x in t.items()},
                          "gb_per_s": {nm: round(30 * n / med[nm] / 1e3, 1) for nm in names},
                          "steps_taken": int(state[2].item())}), flush=True)


if __name__ == "__main__":
    main()
