"""fp64 restatement of the training objective of the loss-head kernels (label smoothing eps, z-loss zeta), written out by hand
(no autograd, no F.cross_entropy: torch carries label_smoothing in single precision even for fp64 inputs).  Per row, with
lse = logsumexp(x), p = softmax(x), t the target:

    objective  l   = lse - (1 - eps) x_t - (eps / V) sum_i x_i + zeta lse^2
    gradient   g_i = grad_scale (p_i (1 + 2 zeta lse) - (1 - eps) [i == t] - eps / V)

The loss is the mean of l over the rows.  Not a test module: the tests of the loss options import it."""
import torch


def objective_fp64(logits, targets, label_smoothing=0.0, z_loss=0.0, grad_scale=1.0):
    """logits [M, V] (any float type: taken as stored), targets [M] -> (rows [M], gradient [M, V]), both fp64 on the CPU"""
    x = logits.detach().double().cpu()
    t = targets.detach().cpu().long()
    M, V = x.shape
    eps, zeta = float(label_smoothing), float(z_loss)
    lse = torch.logsumexp(x, 1)
    xt = x[torch.arange(M), t]
    rows = lse - (1.0 - eps) * xt - (eps / V) * x.sum(1) + zeta * lse * lse
    p = torch.exp(x - lse[:, None])
    g = p * (1.0 + 2.0 * zeta * lse)[:, None] - eps / V
    g[torch.arange(M), t] -= 1.0 - eps
    return rows, g * float(grad_scale)


def objective_torch(logits, targets, label_smoothing=0.0, z_loss=0.0):
    """the same objective (mean over rows) through torch's own F.cross_entropy, differentiable: the cross-check of the
    restatement, and what autograd applies to a CPU oracle's logits"""
    ce = torch.nn.functional.cross_entropy(logits, targets, label_smoothing=float(label_smoothing))
    if z_loss:
        ce = ce + float(z_loss) * torch.logsumexp(logits, 1).pow(2).mean()
    return ce


def edge_case_logits(M, V, seed, scale=3.0):
    """random logits [M, V] (M >= 5) and targets that cover: target 0 (row 0), target V - 1 (row 1), the row's argmax (row 2), a row
    of equal logits (row 3), a row with one logit at +50 and the rest at -50, the target on it (row 4)"""
    assert M >= 5
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, V, generator=g) * scale
    t = torch.randint(0, V, (M,), generator=g)
    x[3] = 0.75
    x[4] = -50.0
    x[4, V // 2] = 50.0
    t[0], t[1], t[2], t[4] = 0, V - 1, int(x[2].argmax()), V // 2
    return x, t
