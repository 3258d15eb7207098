"""Document-masked attention (dg_doc_starts, dg_attn_fwd_doc / dg_attn_bwd_doc): the case table of tests/test_gpu_docmask.py and
the fp64 reference those cases share -- TEST INFRASTRUCTURE (CPU).

The reference needs nothing new in oracle/: document-masked attention IS plain causal attention applied to each document alone.
``stitched`` runs oracle.parity.attention_fp64 per document [a, b) on qkv[:, a:b], dout[:, a:b] with the keep decisions
keep[:, :, a:b, a:b] (the dropout element index stays on absolute positions) and assembles the block-diagonal P and Pd, lse, the
outputs and the three gradients; the same stitching gives the rounding models (model=True for the bf16 MFMA kernels,
model="fp32" for the generic ones).  tests/test_docmask_cases_host.py holds the stitched P to a direct fp64 softmax under the mask
start[i] <= j <= i.

A layout is the tuple of positions at which documents START (the first one 0); every batch row of a case has the same layout.

Backward bound.  oracle.parity.attention_bwd_bounds_by_position takes, per group, BWD_MARGIN x the rounding model's worst group
among the positions within BWD_WINDOW of the group's own: the model's worst dq groups are the near-cancelled first query rows.
Every document restarts those rows, so a window over ABSOLUTE positions compares the first row of a document with rows 100 deep
in the one before it, and by the project's own criterion (attention_cases.dq_conditioning > 1) rejects most draws.  Here the same
maximum is taken over the groups whose offset inside their document, t - start[t], is within BWD_WINDOW of the group's own,
across all documents and all (batch, head) pairs: ``bwd_bounds_by_offset``.  Nothing else changes: same margin, same window."""
import collections
import functools

import torch

import attention_cases as A
from oracle import parity as P

HD = A.HD


def starts_of(T, firsts):
    """int64 [T]: start[t] = the last document start <= t"""
    assert firsts[0] == 0 and list(firsts) == sorted(set(firsts)) and firsts[-1] < T
    s = torch.zeros(T, dtype=torch.int64)
    for a in firsts:
        s[a:] = a
    return s


def documents(T, firsts):
    return list(zip(firsts, list(firsts[1:]) + [T]))


def starts_tensor(B, T, firsts):
    """int32 [B*T], what dg_doc_starts leaves for ids with a separator at the last position of every document but the last"""
    return starts_of(T, firsts).to(torch.int32).repeat(B)


def ids_of(T, firsts, sep, other):
    """int64 [T] token ids with exactly this layout: ``sep`` at a - 1 for every later document start a, ``other`` elsewhere"""
    ids = torch.full((T,), other, dtype=torch.int64)
    for a in firsts[1:]:
        ids[a - 1] = sep
    return ids


def mask(T, firsts):
    """bool [T, T]: query i sees key j"""
    s = starts_of(T, firsts)
    j = torch.arange(T)
    return (j.view(1, T) <= j.view(T, 1)) & (j.view(1, T) >= s.view(T, 1))


def stitched(qkv, dout, B, T, NH, H, firsts, keep=None, p=0.0, model=False):
    """oracle.parity.attention_fp64 per document, assembled: dict(out, lse, P, Pd, v, dq, dk, dv [, dq_mag, dk_mag, dv_mag])"""
    C = NH * H
    q3, d3 = qkv.view(B, T, 3 * C), dout.view(B, T, C)
    res = dict(out=torch.zeros(B, T, C, dtype=torch.float64), lse=torch.zeros(B, NH, T, dtype=torch.float64),
               P=torch.zeros(B, NH, T, T, dtype=torch.float64), Pd=torch.zeros(B, NH, T, T, dtype=torch.float64),
               v=torch.zeros(B, NH, T, H, dtype=torch.float64))
    grads = ("dq", "dk", "dv") + (() if model else ("dq_mag", "dk_mag", "dv_mag"))
    for n in grads:
        res[n] = torch.zeros(B, T, C, dtype=torch.float64)
    for a, b in documents(T, firsts):
        L = b - a
        kp = None if keep is None else keep[:, :, a:b, a:b]
        R = P.attention_fp64(q3[:, a:b].reshape(B * L, 3 * C), d3[:, a:b].reshape(B * L, C), B, L, NH, H, kp, p, model=model)
        res["out"][:, a:b] = R["out"].view(B, L, C)
        res["lse"][:, :, a:b] = R["lse"]
        res["P"][:, :, a:b, a:b] = R["P"].double()
        res["Pd"][:, :, a:b, a:b] = R["Pd"].double()
        res["v"][:, :, a:b] = R["v"].double()
        for n in grads:
            res[n][:, a:b] = R[n].view(B, L, C)
    for n in ("out",) + grads:
        res[n] = res[n].reshape(B * T, C)
    return res


def bwd_bounds_by_offset(ref, model, B, T, NH, H, firsts, at_least=0.0, floors=None):
    """attention_bwd_bounds_by_position with the window over the offset inside the document (module docstring): per group,
    BWD_MARGIN x the model's worst group among all (batch, head, document) at offsets within BWD_WINDOW of the group's own"""
    off = torch.arange(T) - starts_of(T, firsts)
    n_off = int(off.max()) + 1
    out = {}
    for n in ("dq", "dk", "dv"):
        e = P.rowwise_rel(model[n], ref[n], H, floors[n] if floors else 0.0).view(B, T, NH).amax(dim=(0, 2))      # worst per position
        eo = torch.zeros(n_off, dtype=e.dtype).scatter_reduce(0, off, e, "amax", include_self=True)             # worst per offset
        pad = torch.nn.functional.pad(eo.view(1, 1, n_off), (P.BWD_WINDOW, P.BWD_WINDOW), value=0.0)
        win = torch.nn.functional.max_pool1d(pad, 2 * P.BWD_WINDOW + 1, 1).view(n_off)
        out[n] = (P.BWD_MARGIN * win[off]).clamp_min(at_least).view(1, T, 1).expand(B, T, NH).reshape(-1)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the cases: NH = 3, H = 64, bf16 (the MFMA kernels), p in {0, 0.2}
# ---------------------------------------------------------------------------------------------------------------------
class Case(collections.namedtuple("Case", "name B T NH firsts draw order note")):
    """firsts: where documents start; draw: the operand draw (attention_cases.operands) -- the one the conditioning criterion
    was checked for (tests/test_docmask_cases_host.py); order: the block order the case is named for"""
    __slots__ = ()


PS = (0.0, 0.2)
CASES = [
    Case("doc-one-tile", 2, 32, 3, (0, 1, 5, 31), 0, 0, "documents of length 1 at both ends of a tile"),
    Case("doc-ragged", 3, 66, 3, (0, 31, 33, 64), 1, 0, "block 1 visits tile 0 with rows 33.. wholly masked (the NaN guard); block 2 "
         "starts at kt0 = 2; 2-row last tile; an invalid wave"),
    Case("doc-pairs", 2, 128, 3, (0, 40, 64, 100), 0, 1, "a boundary on a tile edge and two inside tiles"),
    Case("doc-heavy", 1, 512, 3, (0, 130, 256, 300, 511), 3, 2, "the shared dQ form with four different kt0 in one workgroup; zero tiles"),
]
NAMES = [c.name for c in CASES]
CASE_P = [(c.name, p) for c in CASES for p in PS]


def case(name):
    return next(c for c in CASES if c.name == name)


@functools.lru_cache(maxsize=2)
def reference(name, p):
    """as attention_cases.reference, stitched: dict(qkv, dout, starts (int32 [B*T]); fp64: out, lse, dq, dk, dv, P, env, dead,
    delta_noise, floors, bounds (bwd_bounds_by_offset against the bf16 rounding model), model_worst).  Nothing returned is modified
    by the tests."""
    c = case(name)
    B, T, NH = c.B, c.T, c.NH
    qkv, dout = A.operands(B, T, NH, c.draw)
    keep = None
    if p > 0:
        keep = torch.from_numpy(A.keep_slab(p, 0, B * NH * T * T).reshape(B, NH, T, T)).double()
    R = stitched(qkv, dout, B, T, NH, HD, c.firsts, keep, p)
    M = stitched(qkv, dout, B, T, NH, HD, c.firsts, keep, p, model=True)
    ref = {k: R[k] for k in ("out", "lse", "dq", "dk", "dv", "dq_mag", "dk_mag", "dv_mag", "P")}
    ref["env"] = P.attention_fwd_envelope(R)
    ref["dead"] = None if keep is None else (keep * mask(T, c.firsts).double()).sum(-1) == 0
    ref["delta_noise"] = A.delta_noise(R, P._split(qkv, B, T, NH, HD)[1], dout, B, T, NH)
    ref["floors"] = {k: P.structured_floor(ref, k, HD) if ref[k].reshape(-1, HD).norm(dim=1).median().item() == 0 else 0.0
                     for k in ("dq", "dk", "dv")}
    model = {k: M[k] for k in ("dq", "dk", "dv")}
    ref["bounds"] = bwd_bounds_by_offset(ref, model, B, T, NH, HD, c.firsts, floors=ref["floors"])
    ref["model_err"] = {k: P.rowwise_rel(model[k], ref[k], HD, ref["floors"][k]) for k in ("dq", "dk", "dv")}
    ref["model_worst"] = {k: ref["model_err"][k].max().item() for k in ("dq", "dk", "dv")}
    for k in ("dq_mag", "dk_mag", "dv_mag"):
        del ref[k]
    ref.update(qkv=qkv, dout=dout, starts=starts_tensor(B, T, c.firsts))
    return ref
