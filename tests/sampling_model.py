"""numpy / fp64 restatement of the device sampler (dg_sample_rows, include/drakegpt_hip.h) -- TEST INFRASTRUCTURE.

    z = logits * inv_temp (fp32);  tau = k-th largest z, keep z >= tau (ties kept), never -inf;
    e = exp(z - max z) on the kept set (the subtraction in fp32, as the kernel does it; exp and everything after it in fp64);
    u = (h >> 8) * 2^-24, h = element_hash(site_key(seed, L, SITE_SAMPLE), [row]);
    token = smallest n with sum_{j <= n} e_j > u * S, else the last kept index;  temperature 0 = lowest argmax.
"""
from __future__ import annotations

import numpy as np

from oracle import rng_ref

SITE_SAMPLE = 0x53414D50


def inv_temp(temperature: float) -> np.float32:
    return np.float32(0.0 if temperature == 0 else 1.0 / float(temperature))


def uniforms(seed: int, L: int, rows: int) -> np.ndarray:
    """u of rows 0..rows-1 at sequence length L, fp64 (exact: 24-bit fractions)"""
    h = rng_ref.element_hash(rng_ref.site_key(seed, L, SITE_SAMPLE), np.arange(rows, dtype=np.uint64))
    return (h >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def weights(logits: np.ndarray, temperature: float = 1.0, top_k=None):
    """logits fp32 [..., V] -> (e fp64 [..., V] (0 off the kept set), kept bool [..., V])"""
    logits = np.asarray(logits, dtype=np.float32)
    V = logits.shape[-1]
    z = (logits * inv_temp(temperature)).astype(np.float32)
    kept = z > -np.inf
    if top_k is not None and 0 < top_k < V:
        tau = np.partition(z, V - top_k, axis=-1)[..., V - top_k]
        kept &= z >= tau[..., None]
    with np.errstate(invalid="ignore"):
        d = (z - z.max(axis=-1, keepdims=True)).astype(np.float32)
    e = np.where(kept, np.exp(np.where(kept, d, 0).astype(np.float64)), 0.0)
    return e, kept


def probs(logits, temperature: float = 1.0, top_k=None):
    e, kept = weights(logits, temperature, top_k)
    return e / e.sum(axis=-1, keepdims=True), kept


def _pick(e_row: np.ndarray, kept_row: np.ndarray, u: np.ndarray) -> np.ndarray:
    F = np.cumsum(e_row)
    n = np.searchsorted(F, u * F[-1], side="right")            # first n with F[n] > u * S
    return np.where(n < F.size, n, np.flatnonzero(kept_row)[-1])


def sample(logits, seed: int, L: int, temperature: float = 1.0, top_k=None, rows=None) -> np.ndarray:
    """tokens int64 [M].  logits [M, V]; or one row [V] shared by `rows` rows (M = rows)"""
    logits = np.asarray(logits, dtype=np.float32)
    shared = logits.ndim == 1
    M = rows if shared else logits.shape[0]
    if temperature == 0:
        am = np.argmax(logits, axis=-1)
        return np.full(M, am, dtype=np.int64) if shared else am.astype(np.int64)
    u = uniforms(seed, L, M)
    e, kept = weights(logits, temperature, top_k)
    if shared:
        return _pick(e, kept, u).astype(np.int64)
    return np.array([_pick(e[m], kept[m], u[m:m + 1])[0] for m in range(M)], dtype=np.int64)


def freq_bound_ok(tokens: np.ndarray, p: np.ndarray):
    """|freq - p| <= 5 sqrt(p (1 - p) / N) + 1 / N for every token; returns (ok, worst standardised deviation)"""
    N = tokens.size
    freq = np.bincount(tokens, minlength=p.size) / N
    sd = np.sqrt(p * (1 - p) / N)
    ok = bool(np.all(np.abs(freq - p) <= 5 * sd + 1.0 / N))
    worst = float(np.max(np.abs(freq - p)[sd > 0] / sd[sd > 0])) if np.any(sd > 0) else 0.0
    return ok, worst
