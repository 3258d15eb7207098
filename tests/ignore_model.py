"""fp64 restatement of ignore_index on top of tests/loss_model.py's objective, and the masks the tests of the option use.  With
keep_r = (t_r != I) and N = sum keep_r:

    rows      l_r keep_r                          (l the row objective of loss_model.objective_fp64: eps and zeta included)
    loss      sum_r keep_r l_r / N                (NaN at N = 0, as torch's)
    gradient  keep_r g_r grad_scale / N           (zero rows at N = 0: the one documented difference from torch, whose are NaN)

Not a test module: the tests of the option import it."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_model as LM  # noqa: E402

PATTERNS = ("none", "first", "last", "block16", "share", "all_but_one", "random")
IGNORE_VALUES = (-100, 3)


def masked_objective_fp64(logits, targets, ignore_index, label_smoothing=0.0, z_loss=0.0, grad_scale=1.0):
    """logits [M, V], targets [M] -> (rows [M], loss (0-d), gradient [M, V], keep [M] bool), fp64 on the CPU"""
    t = targets.detach().cpu().long()
    keep = t != int(ignore_index)
    n = int(keep.sum())
    safe = torch.where(keep, t, torch.zeros_like(t))
    rows, g = LM.objective_fp64(logits, safe, label_smoothing, z_loss)
    rows = torch.where(keep, rows, torch.zeros_like(rows))
    g = torch.where(keep[:, None], g, torch.zeros_like(g))
    if n:
        g = g * (float(grad_scale) / n)
        loss = rows.sum() / n
    else:
        loss = torch.tensor(float("nan"), dtype=torch.float64)
    return rows, loss, g, keep


def count_np(n):
    """the numpy restatement of dg_ce_count_valid's output: {(float)N, one fp32 division}"""
    import numpy as np
    with np.errstate(divide="ignore"):
        return np.array([np.float32(n), np.float32(1) / np.float32(n)], dtype=np.float32)


def ignored_rows(pattern, M, rows_per=None, seed=0):
    """bool [M], True where the row is ignored; None where the pattern does not fit M rows.  share: the rows of workgroup 1 of the
    fused kernel at rows_per rows per workgroup (default: M split in three)"""
    m = torch.zeros(M, dtype=torch.bool)
    if pattern == "none":
        return m
    if pattern == "first":
        m[0] = True
    elif pattern == "last":
        m[M - 1] = True
    elif pattern == "block16":
        if M <= 16:
            return None
        m[16:32] = True
    elif pattern == "share":
        rp = rows_per if rows_per is not None else (M + 2) // 3
        if 2 * rp > M:
            return None
        m[rp:2 * rp] = True
    elif pattern == "all_but_one":
        m[:] = True
        m[1] = False          # (row 1 of loss_model.edge_case_logits: target V - 1, a gradient of ordinary size -- the one row left is
                              # the whole tensor, and the +50 / -50 row's gradient, about 1e-40, is below what bf16 can hold)
    elif pattern == "random":
        m = torch.rand(M, generator=torch.Generator().manual_seed(1000 + seed + M)) < 0.4
    else:
        raise ValueError(pattern)
    if M < 2 or bool(m.all()):
        return None
    return m


def apply_mask(targets, ignored, ignore_index, V):
    """targets with the ignored rows set to ignore_index; an in-vocabulary ignore_index appears nowhere else"""
    t = targets.clone()
    if 0 <= ignore_index < V:
        t[t == ignore_index] = (ignore_index + 1) % V
    t[ignored] = ignore_index
    return t


def cases(M, V, rows_per=None, seed=0):
    """every (pattern, I, ignored) that fits M rows"""
    out = []
    for p in PATTERNS:
        ig = ignored_rows(p, M, rows_per, seed)
        if ig is None:
            continue
        for I in IGNORE_VALUES:
            out.append((p, I, ig))
    return out
