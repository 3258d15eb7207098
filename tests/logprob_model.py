"""numpy restatement of dg_token_logprobs (include/drakegpt_hip.h) -- TEST INFRASTRUCTURE.

    m* = max x (fp32);  d_j = x_j - m* (one fp32 rounding);  e_j = exp((double)d_j);
    Z  = the e_j summed in the kernel's fixed order (fixed_order_sum: chunk sums in index order, the 6-level scan of every wave,
         the wave totals in wave order);  lp_j = (float)((double)d_j - log(Z));
    rank = #{x_i > x_t} + #{i < t : x_i == x_t};  top-n = the n largest x > -inf, descending by fp32 bit order, lowest index first;
    skipped rows (finished before L, or forced) are left exactly as they were.

`defect=` plants one of the mistakes the GPU comparison has to refuse (tests/test_logprobs_host.py shows that `compare` does).
"""
from __future__ import annotations

import numpy as np

MAX_TOP = 20
DEFECTS = ("logp", "tie_reversed", "rank_ge", "stop_unscored")


def threads_of(V: int) -> int:
    return 256 if V <= 8192 else 1024


def fixed_order_sum(e: np.ndarray) -> np.ndarray:
    """e fp64 [M, V] -> Z fp64 [M], the additions in the kernel's order"""
    M, V = e.shape
    NT = threads_of(V)
    chunk = -(-V // NT)
    pad = np.zeros((M, NT * chunk), dtype=np.float64)          # x + 0.0 == x: the padding changes no bit
    pad[:, :V] = e
    c = pad.reshape(M, NT, chunk)
    cs = np.zeros((M, NT), dtype=np.float64)
    with np.errstate(invalid="ignore"):
        for j in range(chunk):
            cs = cs + c[:, :, j]
        w = cs.reshape(M, NT // 64, 64).copy()
        for o in (1, 2, 4, 8, 16, 32):
            w[:, :, o:] = w[:, :, o:] + w[:, :, :-o]
        Z = np.zeros(M, dtype=np.float64)
        for v in range(NT // 64):
            Z = Z + w[:, v, 63]
    return Z


def keys(x: np.ndarray) -> np.ndarray:
    """order-preserving uint32 keys of fp32 values, as int64 (so that they can be negated)"""
    b = np.asarray(x, dtype=np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.int64)


def row_math(x: np.ndarray, defect=None):
    """x fp32 [M, V] -> lp fp32 [M, V] (every column's log-probability)"""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        mx = x.max(axis=1, keepdims=True)
        d = (x - mx).astype(np.float32)
        e = np.exp(d.astype(np.float64))
        Z = fixed_order_sum(e)[:, None]
        if defect == "logp":                                    # log of the fp32 probability: -inf once p underflows
            return np.log((e / Z).astype(np.float32)).astype(np.float32)
        return (d.astype(np.float64) - np.log(Z)).astype(np.float32)


def new_outputs(shape, fill_lp=0.0, fill_rank=0):
    """(lp, rank, top_ids, top_lp) for `shape` output elements"""
    return (np.full(shape, fill_lp, dtype=np.float32), np.full(shape, fill_rank, dtype=np.int32),
            np.full(tuple(shape) + (MAX_TOP,), -1, dtype=np.int32), np.full(tuple(shape) + (MAX_TOP,), -np.inf, dtype=np.float32))


def token_logprobs(logits, V, tokens, top_n=0, L=None, lengths=None, spans=None, outputs=None, defect=None):
    """logits fp32 [M, >= V]; tokens int64 [M] (L None) or [M, cap] with the position L.  Returns (lp, rank, top_ids, top_lp) with
    the layout of tokens (+ [MAX_TOP]); `outputs`: arrays to write into (the skipped rows keep what they hold)."""
    x = np.asarray(logits, dtype=np.float32)[:, :V]
    M = x.shape[0]
    tokens = np.asarray(tokens, dtype=np.int64)
    decode = L is not None
    out = outputs if outputs is not None else new_outputs(tokens.shape)
    lp_o, rk_o, ti_o, tl_o = out
    if decode and L >= tokens.shape[1]:
        return out
    lp_all = row_math(x, defect)
    kx = keys(x)
    n = min(max(int(top_n), 0), MAX_TOP)
    for m in range(M):
        if decode:
            if lengths is not None and lengths[m] != 0 and L >= lengths[m] - (1 if defect == "stop_unscored" else 0):
                continue
            if spans is not None and L < spans[m][0]:
                continue
        t = int(np.clip(tokens[m, L] if decode else tokens[m], 0, V - 1))
        at = (m, L) if decode else (m,)
        lp_o[at] = lp_all[m, t]
        i = np.arange(V)
        with np.errstate(invalid="ignore"):
            above = x[m] >= x[m, t] if defect == "rank_ge" else x[m] > x[m, t]
            ties = np.zeros(V, dtype=bool) if defect == "rank_ge" else (x[m] == x[m, t]) & (i < t)
        rk_o[at] = int(above.sum() + ties.sum())
        ti_o[at] = -1
        tl_o[at] = -np.inf
        if n:
            if defect == "tie_reversed":
                order = np.argsort(-kx[m][::-1], kind="stable")
                order = V - 1 - order
            else:
                order = np.argsort(-kx[m], kind="stable")
            order = order[x[m, order] > -np.inf][:n]
            ti_o[at + (slice(0, order.size),)] = order
            tl_o[at + (slice(0, order.size),)] = lp_all[m, order]
    return out


# ----------------------------------------------------------------------------------------------- the comparison
def _ordered(a: np.ndarray) -> np.ndarray:
    """fp32 -> int64 that counts ulps along the number line"""
    b = a.view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFF), b)


def lp_mismatch(got: np.ndarray, want: np.ndarray, share: float = 1e-3):
    """None when `got` is bit-equal to `want` in all but at most `share` of the entries and those differ by one fp32 ulp (NaN where
    and only where want is NaN); else a description.  Both sides sum bit-identical fp64 terms in one order and differ in the last
    bit of exp / log, which moves the fp32 rounding only at a boundary: the share is a condition, not a tolerance."""
    got = np.ascontiguousarray(got, dtype=np.float32).ravel()
    want = np.ascontiguousarray(want, dtype=np.float32).ravel()
    if got.shape != want.shape:
        return f"shape {got.shape} != {want.shape}"
    gn, wn = np.isnan(got), np.isnan(want)
    if not np.array_equal(gn, wn):
        return f"NaN pattern differs at {np.flatnonzero(gn != wn)[:5]}"
    inf = np.isinf(want) | np.isinf(got)
    if not np.array_equal(got[inf], want[inf]):
        return f"infinities differ at {np.flatnonzero(inf & (got != want))[:5]}"
    ok = ~wn & ~inf
    ulps = np.abs(_ordered(got[ok]) - _ordered(want[ok]))
    if ulps.size and ulps.max() > 1:
        j = int(np.argmax(ulps))
        return f"{int(ulps.max())} ulps apart: got {got[ok][j]!r}, want {want[ok][j]!r}"
    if (ulps != 0).sum() > share * got.size:
        return f"{int((ulps != 0).sum())} of {got.size} entries are not bit-equal (cap {share})"
    return None


def compare(got, want):
    """got / want: (lp, rank, top_ids, top_lp), any of got's None = not produced.  Returns the list of what differs: ranks and top
    ids exactly, the two lp arrays under lp_mismatch."""
    bad = []
    names = ("lp", "rank", "top_ids", "top_lp")
    for name, g, w in zip(names, got, want):
        if g is None:
            continue
        g = np.asarray(g)
        if name in ("rank", "top_ids"):
            if g.shape != w.shape or not np.array_equal(g, w):
                bad.append(f"{name}: differs" + (f" at {np.argwhere(g != w)[:3].tolist()}" if g.shape == w.shape else " in shape"))
        else:
            why = lp_mismatch(g, w)
            if why:
                bad.append(f"{name}: {why}")
    return bad


# ----------------------------------------------------------------------------------------------- the case table
VOCABS = (1, 2, 63, 64, 65, 80, 257, 1000, 4099)
ROWS = (1, 3, 8)
KINDS = ("randn1", "randn30", "quant4", "special")


def bf16_round(x: np.ndarray) -> np.ndarray:
    """fp32 -> the nearest bf16 (ties to even), as fp32; infinities stay"""
    b = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    out = r.astype(np.uint32).view(np.float32)
    return np.where(np.isfinite(x), out, x).astype(np.float32)


def make_case(V: int, M: int, kind: str, seed: int, bf16: bool = False):
    """(logits fp32 [M, ldl] with NaN in the pad columns V..ldl-1, tokens int64 [M]).  kind "special" has 8 rows: some -inf with
    the token on one, all -inf, one entry 200 above the rest with the token off it and on it, a token beyond V - 1 and one below 0,
    the token at the maximum, a plain row."""
    g = np.random.default_rng(seed)
    if kind == "special":
        M = 8
    ldl = V + 3
    x = g.standard_normal((M, V)).astype(np.float32)
    tok = g.integers(0, V, size=M).astype(np.int64)
    if kind == "randn30":
        x *= np.float32(30)
    elif kind == "quant4":
        x = (np.floor(x.clip(-2, 1.99)) + np.float32(0.5)).astype(np.float32)          # -1.5, -0.5, 0.5, 1.5: never +-0
    elif kind == "special":
        hole = g.random(V) < 0.3
        hole[g.integers(0, V)] = True
        if V > 1 and hole.all():
            hole[V - 1] = False                                 # one finite entry stays: the row's lp are -inf, not NaN
        x[0, hole] = -np.inf
        tok[0] = int(np.flatnonzero(hole)[0])
        x[1] = -np.inf
        for r in (2, 3):
            s = int(g.integers(0, V))
            x[r] = x[r] * np.float32(0.01)
            x[r, s] = np.float32(200)
            tok[r] = s if r == 3 else (s + 1) % V
        tok[4], tok[5] = V + 7, -3
    if bf16:
        x = bf16_round(x)
    if kind == "special":
        tok[6] = int(np.argmax(x[6]))                           # the lowest index of the (rounded) maximum
    full = np.full((M, ldl), np.nan, dtype=np.float32)
    full[:, :V] = x
    return full, tok


def case_table():
    """(id, V, M, kind, seed): every vocabulary with every kind, the row counts taken in turn; two rows at the GPT-2 vocabulary"""
    out, n = [], 0
    for V in VOCABS:
        for kind in KINDS:
            M = ROWS[n % len(ROWS)]
            out.append((f"V{V}-M{8 if kind == 'special' else M}-{kind}", V, M, kind, 1000 + n))
            n += 1
    out.append(("V50257-M2-randn1", 50257, 2, "randn1", 77))
    out.append(("V50257-M2-quant4", 50257, 2, "quant4", 78))
    return out


# ----------------------------------------------------------------------------------------------- score() against the oracle
def rank_case_ids(V: int, T: int, seed: int = 11, B: int = 2):
    """the token ids of the score() rank test (torch int64 [B, T]), shared by its CPU and GPU halves"""
    import torch
    return torch.randint(0, V, (B, T), generator=torch.Generator().manual_seed(seed))


def clear_positions(logits, targets, e: float):
    """logits fp64 [B, T, V] (the oracle's), targets int64 [B, T] -> (clear bool [B, T]: no other logit lies within 4 e of the
    target's, so logits within e of these rank the target alike;  the oracle's rank of the target int64 [B, T])"""
    import torch
    xt = logits.gather(2, targets[:, :, None])
    d = (logits - xt).abs()
    d.scatter_(2, targets[:, :, None], float("inf"))
    return d.min(-1).values > 4 * e, (logits > xt).sum(-1)
