"""numpy restatement of the update guard's decision and counters (dg_grad_norm_finalize_guard, include/drakegpt_hip.h):

    apply       = total_norm <= limit  and  (loss is None or isfinite(loss))          (fp32 comparison: NaN and Inf fail)
    skipped     += not apply
    consecutive = 0 if apply else consecutive + 1

and of the norm's non-finite caveat: the sum of squares is taken in fp32, so |g| > sqrt(FLT_MAX) = 1.8e19 squares to Inf."""
import numpy as np

F = np.float32
FLT_MAX = float(np.finfo(np.float32).max)


def decide(total_norm, limit, loss=None) -> int:
    """apply (1 or 0) from the fp32 norm, the fp32 limit and the optional fp32 loss"""
    ok = bool(F(total_norm) <= F(limit))          # False for a NaN norm, and for +Inf against any finite limit
    if loss is not None:
        ok = ok and bool(np.isfinite(F(loss)))
    return int(ok)


def advance(guard, apply: int):
    """the guard block {apply, skipped, consecutive, spare} after one decision"""
    _, skipped, consecutive, spare = guard
    return [apply, skipped + (1 - apply), 0 if apply else consecutive + 1, spare]


def run(decisions, guard=(1, 0, 0, 0)):
    """the block after a sequence of decisions, and the block after each of them"""
    trace, guard = [], list(guard)
    for a in decisions:
        guard = advance(guard, a)
        trace.append(list(guard))
    return guard, trace


def reads_nonfinite(g) -> bool:
    """does the fp32 sum of squares see the buffer as non-finite?  NaN, +-Inf, or a finite element whose fp32 square overflows"""
    g = np.asarray(g, dtype=F)
    with np.errstate(over="ignore", invalid="ignore"):
        return not bool(np.isfinite(np.multiply(g, g, dtype=F)).all())


def words(engine_steps):
    """(data word, optimizer word) after a sequence of per-step decisions: the data word moves every step, the optimizer's only
    with an applied update"""
    return len(engine_steps), int(sum(engine_steps))
