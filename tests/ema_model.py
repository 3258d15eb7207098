"""numpy restatement of the moving average dg_adamw_step_ema keeps (include/drakegpt_hip.h): with s the step word the launch reads,

    d_s = decay, or with warm-up min(decay, (s + 1) / (s + 10))       (fp32, the division too)
    w   = 1 - d_s                                                      (fp32)
    s == 0:  ema = p                  s > 0:  ema = ema + (p - ema) * w

`step` is the kernel's arithmetic: fp32, three separately rounded operations (numpy rounds every ufunc's result: no FMA).
`step64` carries the average in fp64 with the SAME fp32 w: what the fp32 recurrence is an approximation of."""
import numpy as np

F = np.float32


def decay_at(decay, warmup, s):
    """d_s as the kernel computes it, an fp32 scalar"""
    d = F(decay)
    if warmup:
        d = min(d, (F(s) + F(1)) / (F(s) + F(10)))
    return F(d)


def weight(decay, warmup, s):
    return F(1) - decay_at(decay, warmup, s)


def step(ema, p, decay, warmup, s):
    """one update in fp32; ema is not read at s == 0 (it may be None)"""
    p = np.asarray(p, dtype=F)
    if s == 0:
        return p.copy()
    ema = np.asarray(ema, dtype=F)
    w = weight(decay, warmup, s)
    d = np.subtract(p, ema, dtype=F)
    t = np.multiply(d, w, dtype=F)
    return np.add(ema, t, dtype=F)


def step64(ema, p, decay, warmup, s):
    """the same update carried in fp64 (p is fp32 data; w is the fp32 weight, widened)"""
    p = np.asarray(p, dtype=F).astype(np.float64)
    if s == 0:
        return p.copy()
    w = np.float64(weight(decay, warmup, s))
    return ema + (p - ema) * w


def run(ps, decay, warmup=False, first=0, ema=None, fn=step):
    """the average after the weights ps[0], ps[1], ... were seen at step words first, first + 1, ..."""
    for k, p in enumerate(ps):
        ema = fn(ema, p, decay, warmup, first + k)
    return ema
