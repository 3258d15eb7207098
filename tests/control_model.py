"""numpy restatement of the sampler controls (dg_sample_rows_control, include/drakegpt_hip.h) -- TEST INFRASTRUCTURE.

On top of nucleus_model: the logits are adjusted first, every step one fp32 rounding (numpy's float32 arithmetic is correctly
rounded, as __fmul_rn / __fsub_rn / __fadd_rn are), c = the token's count in the row's sequence so far:

    y = c > 0 ? (x > 0 ? x * inv_rep : x * rep) : x          inv_rep = fp32(1 / rep)
    y = y - (c > 0 ? presence : 0)
    y = y - frequency * (float)c
    y = y + bias                                             only with a bias; -inf bans

and everything else is nucleus_model on y.  The generation loop recounts from the ids prefix at every token (nothing is carried),
and applies the stop rule: a row keeps its stop token, every later position is the pad token, the width is the longest row.
"""
from __future__ import annotations

import numpy as np

import nucleus_model as NM

f32 = np.float32


def adjust(logits, counts=None, rep=1.0, presence=0.0, frequency=0.0, bias=None) -> np.ndarray:
    """logits fp32 [..., V], counts int [..., V] (None: zeros) -> y fp32 [..., V]"""
    x = np.asarray(logits, dtype=f32)
    c = np.zeros(x.shape, dtype=np.int32) if counts is None else np.broadcast_to(np.asarray(counts, dtype=np.int32), x.shape)
    rep32 = f32(rep)
    inv_rep = f32(1.0 / float(rep))                  # made on the host from the Python float, rounded once
    seen = c > 0
    with np.errstate(invalid="ignore", over="ignore"):
        y = np.where(seen, np.where(x > 0, x * inv_rep, x * rep32), x).astype(f32)
        y = (y - np.where(seen, f32(presence), f32(0))).astype(f32)
        y = (y - (f32(frequency) * c.astype(f32)).astype(f32)).astype(f32)
        if bias is not None:
            y = (y + np.asarray(bias, dtype=f32)).astype(f32)
    return y


def probs(logits, counts=None, rep=1.0, presence=0.0, frequency=0.0, bias=None, **kw):
    return NM.probs(adjust(logits, counts, rep, presence, frequency, bias), **kw)


def sample(logits, seed, L, counts=None, rep=1.0, presence=0.0, frequency=0.0, bias=None, **kw):
    return NM.sample(adjust(logits, counts, rep, presence, frequency, bias), seed, L, **kw)


def margins(logits, counts=None, rep=1.0, presence=0.0, frequency=0.0, bias=None, **kw):
    return NM.margins(adjust(logits, counts, rep, presence, frequency, bias), **kw)


def count_prefix(ids: np.ndarray, V: int) -> np.ndarray:
    """ids int [B, n] -> counts int32 [B, V] of the clamped ids"""
    ids = np.clip(np.asarray(ids), 0, V - 1)
    return np.stack([np.bincount(r, minlength=V) for r in ids]).astype(np.int32)


def apply_stop(ids: np.ndarray, t0: int, stop, pad: int) -> np.ndarray:
    """the stop and pad rule on a finished plain run ids [B, t0 + n]: each row keeps its first stop token after the prompt, pad
    behind it, and the width is the longest row's"""
    ids = np.array(ids)
    B, total = ids.shape
    ends = []
    for m in range(B):
        hit = [j for j in range(t0, total) if int(ids[m, j]) in stop]
        end = hit[0] + 1 if hit else total
        ids[m, end:] = pad
        ends.append(end)
    return ids[:, :max(ends)]


def generate(logits_fn, prompt: np.ndarray, n_new: int, V: int, seed: int, rep=1.0, presence=0.0, frequency=0.0, bias=None,
             stop=(), pad=None, **kw) -> np.ndarray:
    """the generation loop: logits_fn(ids [B, L]) -> fp32 [B, V] of the next position.  Counts are recounted from the whole
    prefix (prompt included) at every token; finished rows get pad; the loop ends when every row is finished."""
    ids = np.array(prompt, dtype=np.int64)
    B, t0 = ids.shape
    pad = (stop[0] if stop else 0) if pad is None else pad
    finished = np.zeros(B, dtype=bool)
    for L in range(t0, t0 + n_new):
        x = np.asarray(logits_fn(ids), dtype=f32)
        tok = sample(x, seed, L, count_prefix(ids, V), rep, presence, frequency, bias, **kw)
        tok = np.where(finished, pad, tok)
        ids = np.concatenate([ids, tok[:, None]], axis=1)
        finished |= np.isin(tok, list(stop)) if stop else False
        if stop and finished.all():
            break
    return ids


# the kernel-against-restatement cases: V, M, temperature, top_k, top_p, min_p, rep, presence, frequency, seed.  Logits are
# default_rng(seed).standard_normal((M, V)) * 3, counts drawn from {0, 0, 0, 1, 2, 7}, the bias -inf / +2 / -2 on a few entries.
# The seeds are the first for which every row clears nucleus_model's MARGIN on the adjusted row (test_control_host verifies).
CASES = [
    (80, 64, 0.7, None, 0.9, None, 1.3, 0.0, 0.0, 2000),
    (257, 64, 1.0, 40, 0.8, None, 1.0, 0.5, 0.25, 2001),
    (8192, 16, 1.0, None, 0.95, None, 1.2, 0.1, 0.1, 2002),
    (8193, 16, 0.8, 500, 0.9, 0.02, 0.8, -0.3, 0.2, 2003),
    (50257, 4, 1.0, None, 0.9, None, 1.3, 0.0, 0.0, 2004),
    (50257, 4, 0.7, 200, 0.5, 0.05, 1.1, 0.4, 0.3, 2005),
]
COUNT_VALUES = np.array([0, 0, 0, 1, 2, 7], dtype=np.int32)


def case_inputs(i: int):
    """-> logits fp32 [M, V], counts int32 [M, V], bias fp32 [V]"""
    V, M = CASES[i][:2]
    g = np.random.default_rng(CASES[i][-1])
    x = (g.standard_normal((M, V)) * 3).astype(f32)
    counts = COUNT_VALUES[g.integers(0, COUNT_VALUES.size, size=(M, V))]
    bias = np.zeros(V, dtype=f32)
    pick = g.permutation(V)[:12]
    bias[pick[:4]] = -np.inf
    bias[pick[4:8]] = 2.0
    bias[pick[8:]] = -2.0
    return x, counts, bias
