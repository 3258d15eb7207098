"""numpy restatement of the top-p / min-p sampler (dg_sample_rows_nucleus, include/drakegpt_hip.h) -- TEST INFRASTRUCTURE.

On top of sampling_model (z, top-k, e = exp(z - max z) in fp64, the uniforms, the token rule):

    min-p:  K1 = { j in K0 : e_j >= (double)min_p }
    top-p:  w_j = rint(e_j * 2^40) as uint64 on K1, else 0;  S1 = sum w_j;  G(t) = sum { w_i : z_i > t };
            T = (double)top_p * (double)S1;  K = { j in K1 : (double)G(z_j) < T }
    top_p None or 1 and min_p None or 0 are "off": sampling_model.weights, untouched.

The masses are uint64 / Python ints throughout: no result depends on a summation order.
"""
from __future__ import annotations

import numpy as np

import sampling_model as SM

SCALE = 2.0 ** 40


def _f32(x) -> np.float64:
    """the fp32 the kernel reads, widened to a double"""
    return np.float64(np.float32(x))


def masses(e_row: np.ndarray, k1_row: np.ndarray) -> np.ndarray:
    return np.where(k1_row, np.rint(e_row * SCALE), 0.0).astype(np.uint64)


def _row(z, e, k0, top_p, min_p):
    """one row -> (kept, G uint64 [V], T, S1, K1)"""
    k1 = k0.copy()
    if min_p is not None and _f32(min_p) > 0:
        k1 &= e >= _f32(min_p)
    if top_p is None or not _f32(top_p) < 1:
        return k1, None, None, None, k1
    w = masses(e, k1)
    S1 = int(w.sum(dtype=np.uint64))
    uz, inv = np.unique(z, return_inverse=True)                  # ascending
    per = np.zeros(uz.size, dtype=np.uint64)
    np.add.at(per, inv, w)
    above = np.uint64(S1) - np.cumsum(per, dtype=np.uint64)      # mass of strictly larger z: exact, every term < 2^61
    G = above[inv]
    T = _f32(top_p) * np.float64(S1)                             # float(int) and astype(float64) round to nearest even, as the kernel does
    kept = k1 & (G.astype(np.float64) < T)
    return kept, G, T, S1, k1


def weights(logits, temperature: float = 1.0, top_k=None, top_p=None, min_p=None):
    """logits fp32 [..., V] -> (e fp64 [..., V] (0 off the kept set), kept bool [..., V])"""
    logits = np.asarray(logits, dtype=np.float32)
    e0, k0 = SM.weights(logits, temperature, top_k)
    if (top_p is None or not _f32(top_p) < 1) and (min_p is None or not _f32(min_p) > 0):
        return e0, k0
    z = (logits * SM.inv_temp(temperature)).astype(np.float32)
    V = logits.shape[-1]
    kept = np.empty(k0.shape, dtype=bool)
    for r, (zr, er, kr) in enumerate(zip(z.reshape(-1, V), e0.reshape(-1, V), k0.reshape(-1, V))):
        kept.reshape(-1, V)[r] = _row(zr, er, kr, top_p, min_p)[0]
    return np.where(kept, e0, 0.0), kept


def probs(logits, temperature: float = 1.0, top_k=None, top_p=None, min_p=None):
    e, kept = weights(logits, temperature, top_k, top_p, min_p)
    return e / e.sum(axis=-1, keepdims=True), kept


def margins(logits, temperature: float = 1.0, top_k=None, top_p=None, min_p=None):
    """per row: (min_j |G(z_j) - T| / S1 over K1, min_j |e_j - min_p| / min_p over K0) -- how far the row is from a decision that
    the last bit of an exp could turn; inf where the filter is off"""
    logits = np.asarray(logits, dtype=np.float32)
    e0, k0 = SM.weights(logits, temperature, top_k)
    z = (logits * SM.inv_temp(temperature)).astype(np.float32)
    V = logits.shape[-1]
    mg, mm = [], []
    for zr, er, kr in zip(z.reshape(-1, V), e0.reshape(-1, V), k0.reshape(-1, V)):
        _, G, T, S1, k1 = _row(zr, er, kr, top_p, min_p)
        mg.append(np.inf if G is None else float(np.min(np.abs(G[k1].astype(np.float64) - T)) / S1))
        on = min_p is not None and _f32(min_p) > 0
        mm.append(float(np.min(np.abs(er[kr] - _f32(min_p))) / _f32(min_p)) if on else np.inf)
    return np.array(mg), np.array(mm)


def sample(logits, seed: int, L: int, temperature: float = 1.0, top_k=None, top_p=None, min_p=None, rows=None) -> np.ndarray:
    """tokens int64 [M].  logits [M, V]; or one row [V] shared by `rows` rows (M = rows)"""
    logits = np.asarray(logits, dtype=np.float32)
    if temperature == 0:
        return SM.sample(logits, seed, L, temperature, top_k, rows=rows)      # greedy ignores both filters
    shared = logits.ndim == 1
    M = rows if shared else logits.shape[0]
    u = SM.uniforms(seed, L, M)
    e, kept = weights(logits, temperature, top_k, top_p, min_p)
    if shared:
        return SM._pick(e, kept, u).astype(np.int64)
    return np.array([SM._pick(e[m], kept[m], u[m:m + 1])[0] for m in range(M)], dtype=np.int64)


# the kernel-against-restatement cases: V, M, temperature, top_k, top_p, min_p (None = off); case i's logits are
# default_rng(1000 + i).standard_normal((M, V)) * 3 as fp32.  Both kernel variants (256 threads up to V = 8192, 1024 above), the
# switch between them, ragged last chunks and the GPT-2 row.
CASES = [
    (80, 64, 0.7, None, 0.9, None),
    (257, 64, 1.0, 40, 0.8, None),
    (8192, 16, 1.0, None, 0.95, None),
    (8193, 16, 0.8, 500, 0.9, 0.02),
    (50257, 4, 1.0, None, 0.9, None),
    (50257, 4, 0.7, 200, 0.5, 0.05),
    (80, 64, 1.0, None, 1.0, 0.1),
    (1000, 32, 1.3, None, 0.3, None),
]
MARGIN = 1e-8


def case_logits(i: int) -> np.ndarray:
    V, M = CASES[i][:2]
    return (np.random.default_rng(1000 + i).standard_normal((M, V)) * 3).astype(np.float32)


def hand_rows():
    """name -> (logits fp32 [V], kwargs, expected kept indices, None for "everything", or "finite" for "some of the finite entries")"""
    V = 300
    equal = np.full(V, -1.25, dtype=np.float32)
    dominant = np.zeros(V, dtype=np.float32)
    dominant[17] = 10.0                                           # p = e^10 / (e^10 + 299) = 0.987
    four = np.linspace(-10, -8, V).astype(np.float32)
    four[[3, 100, 101, 299]] = 2.0                                # four equal maxima, each with 0.25 of the mass: one alone is < 0.3
    holes = np.random.default_rng(5).standard_normal(V).astype(np.float32)
    holes[::2] = -np.inf
    return {
        "all equal, top_p 0.5": (equal, dict(top_p=0.5), None),
        "all equal, top_p 1e-3": (equal, dict(top_p=1e-3), None),
        "all equal, top_p 0.999, min_p 0.5": (equal, dict(top_p=0.999, min_p=0.5), None),
        "one dominant token": (dominant, dict(top_p=0.5), [17]),
        "four equal maxima": (four, dict(top_p=0.3), [3, 100, 101, 299]),
        "-inf entries, top_p": (holes, dict(top_p=0.9), "finite"),
        "-inf entries, min_p": (holes, dict(min_p=0.05), "finite"),
        "-inf entries, top_k + top_p + min_p": (holes, dict(top_k=20, top_p=0.7, min_p=0.01, temperature=0.8), "finite"),
    }
