"""time the loss-head kernels:  python tools/ce_time.py [M=8192] [V=50257] [--label-smoothing E] [--z-loss Z] [--fused] [--reps N]
                                [--ignore-index I [--ignore-frac F]] [--count]

default: dg_cross_entropy on bf16 logits in place (with the options: dg_cross_entropy_smooth).  --fused: the one-launch loss head
of the captured step, dg_cross_entropy_fused(_smooth), fp32 logits, bf16 gradient, M 16384, V 80 unless given.
--ignore-index I: the ignore forms (dg_cross_entropy_ignore, dg_cross_entropy_fused_ignore) on targets of which a fraction F
(--ignore-frac, default 0) is I, the count taken once outside the timed region; --count times the count launch (dg_ce_count_valid)
alone instead.
Each timing is --inner launches (default 5; --fused: 100) inside one graph replay, minus the same graph without the kernel (the
copy that restores the logits); --reps of them (after 3 unreported warm-up replays), reported as median and min .. max."""
import argparse
import os
import statistics
import sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drakegpt_amd import ops
ap = argparse.ArgumentParser()
ap.add_argument("M", nargs="?", type=int, default=None)
ap.add_argument("V", nargs="?", type=int, default=None)
ap.add_argument("--label-smoothing", type=float, default=0.0)
ap.add_argument("--z-loss", type=float, default=0.0)
ap.add_argument("--fused", action="store_true")
ap.add_argument("--ignore-index", type=int, default=None)
ap.add_argument("--ignore-frac", type=float, default=0.0)
ap.add_argument("--count", action="store_true")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--inner", type=int, default=None)
a = ap.parse_args()
inner = a.inner or (100 if a.fused else 5)
M = a.M or (16384 if a.fused else 8192)
V = a.V or (80 if a.fused else 50257)
okw = {k: v for k, v in (("label_smoothing", a.label_smoothing), ("z_loss", a.z_loss)) if v}      # (none: the call of every earlier version)
dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(1)
tg = torch.randint(0, V, (M,), generator=g).to(dev)
eps, zeta = a.label_smoothing, a.z_loss
I = a.ignore_index
if I is None and (a.ignore_frac or a.count):
    ap.error("--ignore-frac and --count go with --ignore-index")
keep = torch.ones(M, dtype=torch.bool, device=dev)
gs = 1.0 / M
if I is not None:
    if 0 <= I < V:
        tg[tg == I] = (I + 1) % V          # (an in-vocabulary I: no other target is I)
    keep = (torch.rand(M, generator=g) >= a.ignore_frac).to(dev)
    tg[~keep] = I
    cnt = ops.count_valid(tg, I)
    okw.update(ignore_index=I, inv_count=cnt[1:])
    gs = 1.0
    print(f"ignore_index {I}: {int(cnt[0].item())} of {M} targets count")
if a.fused:
    n = 256
    src = (torch.randn(M, V, generator=g) * 2.0).to(dev)
    buf = src.clone()
    dl = torch.zeros((M, 128), dtype=torch.bfloat16, device=dev)
    part = torch.zeros((n, 128), device=dev)
    scratch, loss = torch.zeros(n + 1, device=dev), torch.zeros((), device=dev)
    def kernel():
        return ops.cross_entropy_fused(buf, tg, V, dl, gs, part, 128, n, scratch, loss, gs, **okw)
    rows = kernel()
    grad = dl[:, :V]
    x = src.double()
    moved = M * V * 4 + M * 128 * 2
else:
    ld = (V + 7) // 8 * 8
    src = torch.zeros((M, ld), dtype=torch.bfloat16)
    src[:, :V] = (torch.randn(M, V, generator=g) * 2.0).bfloat16()
    src = src.to(dev)
    buf = src.clone()
    def kernel():
        return ops.cross_entropy(buf[:, :V], tg, V, dlogits=buf, grad_scale=gs, **okw)
    rows = kernel()
    grad = buf[:, :V]
    x = src[:, :V].double()
    moved = 2 * M * ld * 2
lse = torch.logsumexp(x, 1)
tc = tg.clamp(0, V - 1)
ref_rows = (lse - (1 - eps) * x.gather(1, tc[:, None])[:, 0] - eps / V * x.sum(1) + zeta * lse * lse) * keep
ref_g = torch.softmax(x, 1) * (1 + 2 * zeta * lse)[:, None] - eps / V
ref_g[torch.arange(M, device=dev), tc] -= 1 - eps
ref_g *= keep[:, None] / max(int(keep.sum().item()), 1)
print("loss rows rel err %.3e; gradient rel err %.3e (bf16 rounding)" % (((rows.double() - ref_rows).norm() / ref_rows.norm()).item(),
      ((grad.double() - ref_g).norm() / ref_g.norm()).item()))
del x, ref_g
if a.count:
    cbuf = torch.zeros(2, device=dev)
    def kernel():      # noqa: F811
        return ops.count_valid(tg, I, out=cbuf)
def body(with_ce):
    buf.copy_(src)
    if with_ce:
        kernel()
def graph(with_ce):
    body(with_ce); torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for _ in range(inner): body(with_ce)
    gr.replay(); torch.cuda.synchronize()
    return gr
def timeit(gr):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(); gr.replay(); e.record(); e.synchronize()
    return s.elapsed_time(e) * 1e3 / inner
g0, g1 = graph(False), graph(True)
for _ in range(3):
    timeit(g0); timeit(g1)
ts = []
for _ in range(a.reps):
    c = timeit(g0)
    ts.append(timeit(g1) - c)
med = statistics.median(ts)
what = ("fused loss head" if a.fused else "cross entropy in place") + (f" (label_smoothing {eps}, z_loss {zeta})" if eps or zeta else "")
if I is not None:
    what += f" (ignore_index {I}, fraction {a.ignore_frac})"
if a.count:
    what, moved = f"count launch (ignore_index {I})", M * 8
print(f"M={M} V={V}: {what} median {med:.1f} us, min {min(ts):.1f} .. max {max(ts):.1f} over {a.reps} (copy {c:.0f} us); "
      f"{moved / med * 1e-6:.2f} TB/s at the median")
