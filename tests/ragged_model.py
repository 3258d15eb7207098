"""numpy restatement of generate(prompt_lengths=...) under the device sampler (dg_sample_rows_ragged, include/drakegpt_hip.h)
-- TEST INFRASTRUCTURE.

On top of control_model: one shared position L walks all rows from the shortest prompt.  At L a finished row gets the pad token,
a row still inside its prompt (L < p_b) keeps its prompt token, and every other row samples exactly as control_model does -- the
same adjusted logits, the same u keyed by (seed, L, row) -- counts its token, and is finished if the token is a stop token or the
last of its budget (L + 1 >= p_b + n_new).  A row's counts are those of its whole prompt plus what it has sampled, recounted at
every position (nothing is carried).
"""
from __future__ import annotations

import numpy as np

import control_model as CM


def pad_prompts(prompts, pad: int, width=None) -> tuple:
    """a list of 1-D prompts -> (right-padded int64 [B, width], lengths [B])"""
    p = [len(r) for r in prompts]
    out = np.full((len(prompts), max(p) if width is None else width), pad, dtype=np.int64)
    for b, r in enumerate(prompts):
        out[b, :p[b]] = r
    return out, p


def generate(logits_fn, prompt, lengths, n_new: int, V: int, seed: int, rep=1.0, presence=0.0, frequency=0.0, bias=None, stop=(),
             pad=None, **kw):
    """prompt int [B, >= max p_b], right-padded (what lies at or beyond p_b is never read); logits_fn(ids [B, L]) -> fp32 [B, V]
    of the next position.  -> (ids [B, n], n = the longest final row; final lengths int [B])"""
    prompt = np.asarray(prompt)
    p = np.asarray(lengths, dtype=np.int64)
    B = p.size
    pad = (stop[0] if stop else 0) if pad is None else pad
    t0, total = int(p.min()), int(p.max()) + n_new
    ids = np.full((B, total), pad, dtype=np.int64)
    for b in range(B):
        ids[b, :p[b]] = prompt[b, :p[b]]
    final = np.where(n_new < 1, p, 0)                       # 0: running
    for L in range(t0, total):
        if final.all():
            break
        x = np.asarray(logits_fn(ids[:, :L]), dtype=np.float32)
        counts = np.stack([CM.count_prefix(ids[b:b + 1, :max(L, int(p[b]))], V)[0] for b in range(B)])
        tok = CM.sample(x, seed, L, counts, rep, presence, frequency, bias, **kw)
        for b in range(B):
            if final[b]:
                ids[b, L] = pad
            elif L >= p[b]:
                ids[b, L] = tok[b]
                if int(tok[b]) in stop or L + 1 >= p[b] + n_new:
                    final[b] = L + 1
    return ids[:, :int(final.max())], final
