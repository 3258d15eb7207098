"""Learning-rate schedules as tables: one value per optimizer step, computed on the host once.

Every function returns a Python list of float64 values for the optimizer steps s = 0 .. N - 1: the update that takes the step
count from s to s + 1 uses entry s.  ``as_table`` turns such a list (or a callable s -> lr with a length) into the CPU fp32
tensor that TrainEngine(lr_schedule=...) stages in HBM; AdamW then looks its rate up by its own step word
(dg_adamw_step_sched), and past the end of the table the last entry holds.  Nothing here touches the GPU."""
from __future__ import annotations

import math
from typing import List

import torch

MAX_STEPS = 1 << 32          # a table index has to fit the device-side step word (uint32)


def _check_count(v, what: str, lo: int) -> int:
    if isinstance(v, bool) or not isinstance(v, int) or v < lo:
        raise ValueError(f"{what} must be an integer >= {lo}, got {v!r}")
    return int(v)


def _check_rate(v, what: str) -> float:
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a finite number >= 0, got {v!r}") from None
    if not math.isfinite(f) or f < 0.0:
        raise ValueError(f"{what} must be a finite number >= 0, got {v!r}")
    return f


def _check_warmup(peak, warmup, total, min_lr):
    """warmup >= 0 steps of linear warm-up, then at least one step of decay before the final entry: total > warmup + 1"""
    peak, min_lr = _check_rate(peak, "peak"), _check_rate(min_lr, "min_lr")
    warmup = _check_count(warmup, "warmup", 0)
    total = _check_count(total, "total", 1)
    if total <= warmup + 1:
        raise ValueError(f"total must be > warmup + 1, got total = {total!r} with warmup = {warmup!r}")
    return peak, warmup, total, min_lr


def constant(lr, N: int = 1) -> List[float]:
    """N entries of lr (one is enough: the last entry holds past the end)"""
    return [_check_rate(lr, "lr")] * _check_count(N, "N", 1)


def warmup_cosine(peak, warmup: int, total: int, min_lr=0.0) -> List[float]:
    """s < warmup: peak (s + 1) / warmup;  warmup <= s < total - 1: min_lr + (peak - min_lr) (1 + cos(pi (s - warmup) /
    (total - 1 - warmup))) / 2;  s >= total - 1: min_lr.  The last entry is min_lr, and the clamp past the table holds it."""
    peak, warmup, total, min_lr = _check_warmup(peak, warmup, total, min_lr)
    out = []
    for s in range(total):
        if s < warmup:
            out.append(peak * (s + 1) / warmup)
        elif s < total - 1:
            out.append(min_lr + 0.5 * (peak - min_lr) * (1.0 + math.cos(math.pi * (s - warmup) / (total - 1 - warmup))))
        else:
            out.append(min_lr)
    return out


def warmup_linear(peak, warmup: int, total: int, min_lr=0.0) -> List[float]:
    """the warm-up of warmup_cosine, then a straight line from peak at s = warmup to min_lr at s = total - 1"""
    peak, warmup, total, min_lr = _check_warmup(peak, warmup, total, min_lr)
    out = []
    for s in range(total):
        if s < warmup:
            out.append(peak * (s + 1) / warmup)
        elif s < total - 1:
            out.append(peak + (min_lr - peak) * (s - warmup) / (total - 1 - warmup))
        else:
            out.append(min_lr)
    return out


def cyclic(base_lr, max_lr, step_size_up: int, total: int) -> List[float]:
    """train.cyclic_lr(s, ...) for every s: torch's CyclicLR(mode='triangular') stepped after every optimizer step"""
    from .train import cyclic_lr
    base_lr, max_lr = _check_rate(base_lr, "base_lr"), _check_rate(max_lr, "max_lr")
    step_size_up = _check_count(step_size_up, "step_size_up", 1)
    return [cyclic_lr(s, base_lr, max_lr, step_size_up) for s in range(_check_count(total, "total", 1))]


def as_table(values, n=None) -> torch.Tensor:
    """the CPU fp32 tensor of a schedule: `values` is a sequence or 1-D tensor of rates (n, if given, must be its length), or a
    callable s -> rate evaluated for s = 0 .. n - 1.  ValueError for an empty table, a rate that is not finite or is negative
    (before or after rounding to fp32), or a length the step word cannot index."""
    if callable(values):
        n = _check_count(n, "schedule_steps (the length of a callable schedule)", 1)
        if n > MAX_STEPS:
            raise ValueError(f"a schedule of {n} steps does not fit the step word (at most {MAX_STEPS})")
        values = [values(s) for s in range(n)]
    elif isinstance(values, torch.Tensor):
        if values.dim() != 1:
            raise ValueError(f"a schedule must be 1-D, got a tensor of shape {tuple(values.shape)}")
        values = values.detach().cpu().double().tolist()
    else:
        try:
            values = list(values)
        except TypeError:
            raise ValueError(f"a schedule must be a sequence, a 1-D tensor or a callable, got {type(values).__name__}") from None
    if n is not None and _check_count(n, "schedule_steps", 1) != len(values):
        raise ValueError(f"schedule_steps is {n}, the schedule has {len(values)} entries")
    if not values:
        raise ValueError("a schedule must have at least one entry")
    if len(values) > MAX_STEPS:
        raise ValueError(f"a schedule of {len(values)} steps does not fit the step word (at most {MAX_STEPS})")
    vals = [_check_rate(v, f"schedule entry {s}") for s, v in enumerate(values)]
    table = torch.tensor(vals, dtype=torch.float64).to(torch.float32)
    if not bool(torch.isfinite(table).all()):
        raise ValueError("a schedule entry overflows fp32")
    return table
