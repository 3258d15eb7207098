"""GPU: ignore_index inside the loss-head kernels, through every dispatch path of dg_cross_entropy_ignore /
dg_cross_entropy_fused_ignore, the count launch, the autograd path, the training engine, resume and the harness.

The reference is the explicit formula in fp64 (tests/ignore_model.py on tests/loss_model.py) evaluated on the logits as stored.
Shapes and bounds are those of tests/test_gpu_loss_options.py and tests/test_gpu_ops.py: rows 1e-6 (norm), mean loss 1e-5, gradient
1e-6 (fp32) / 5e-3 (bf16) with every bf16 element inside the single-rounding envelope, fused column sums 1e-4, padding columns
exactly zero.  Two checks on top: every ignored row is compared with torch.equal (its loss_rows entry 0, its whole dlogits row
zeros where NaN / stale logits were), and the gradient bound holds for every valid row on its own.

The per-row bound.  bf16 gradients: 5e-3, as for the whole tensor (the plain kernels' worst row at these shapes: 3.56e-3).  fp32
gradients: single rows of the PLAIN kernels (no ignore_index; the kernels of the parent commit, whose device code this change
leaves identical) already exceed 1e-6 on these very inputs -- measured on an MI355X, worst row of each: M=33 V=7 1.904e-6
(eps 0.125), 1.791e-6 (eps 0); M=48 V=80 1.269e-6; fused head M=48 V=7 1.918e-6 (first launch's data, eps 0.125) and 5.293e-6
(second launch's data, eps 0: a row whose p_t is near 1, where p_t - 1 cancels) -- so the per-row fp32 bound is twice the largest
of them, 2 x 5.293e-6, for the different order in which the scale is formed (1 / N from the device times grad_scale, not 1 / M
from the host); the whole-tensor bound stays 1e-6.  A valid row whose fp64 gradient norm is below fp32's smallest normal number
(2^-126: the +50 / -50 edge-case row without smoothing, about 1e-40) has no relative error to speak of in these formats: it is
held by the whole-tensor norm and, in bf16, by the element-wise envelope only."""
PLAIN_WORST_ROW_FP32 = 5.293e-6
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ignore_model as IM  # noqa: E402
import loss_model as LM  # noqa: E402

pytestmark = pytest.mark.gpu
V = 80
OPTS = [(0.0, 0.0), (0.125, 0.0), (0.125, 1e-2)]


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _check(rows, dl, V_, ref_rows, ref_loss, ref_grad, keep, name, inv_count=None):
    """the bounds of test_cross_entropy_and_reduce on the masked formula, the gradient bound per valid row, the ignored rows exact;
    every figure printed before it is asserted"""
    from drakegpt_amd import ops
    from oracle import parity as P
    bound, row_bound = (1e-6, 2 * PLAIN_WORST_ROW_FP32) if dl.dtype == torch.float32 else (5e-3, 5e-3)
    got, want = dl[:, :V_].double().cpu(), ref_grad
    held = keep & (want.norm(dim=1) >= 2.0 ** -126)
    per_row = ((got - want).norm(dim=1) / want.norm(dim=1).clamp_min(1e-300))[held]
    e_rows, e_grad, e_row = rel(rows, ref_rows), rel(got, want), per_row.max().item() if per_row.numel() else 0.0
    mean = rows.double().sum().item() / max(int(keep.sum()), 1)
    e_loss = abs(mean - ref_loss.item())
    print(f"{name}: rows {e_rows:.3e} loss {e_loss:.3e} gradient {e_grad:.3e} worst row {e_row:.3e}")
    assert e_rows < 1e-6, (name, e_rows)
    assert e_loss < 1e-5 * max(1.0, abs(ref_loss.item())), (name, e_loss)
    if inv_count is not None:                          # the mean as the device takes it: the scaled reduction
        dev_mean = ops.reduce_sum(rows, 1.0, scale_dev=inv_count).item()
        assert abs(dev_mean - ref_loss.item()) < 1e-5 * max(1.0, abs(ref_loss.item())), (name, dev_mean)
    assert e_grad < bound, (name, e_grad)
    assert e_row < row_bound, (name, e_row)
    if dl.dtype == torch.bfloat16:
        P.assert_within_rounding(dl[:, :V_], ref_grad, P.single_rounding_envelope(ref_grad, V_), 1, name)
    assert torch.all(dl[:, V_:] == 0), name
    ig = ~keep
    if ig.any():
        assert torch.equal(rows.cpu()[ig], torch.zeros(int(ig.sum()))), name
        assert torch.equal(dl.cpu()[ig], torch.zeros((int(ig.sum()), dl.shape[1]), dtype=dl.dtype)), name


# ------------------------------------------------------------------------------------------------ kernels
# fp32 logits: (M, V, ldl, ldd) -- the small kernel (width <= 128), the wave-per-row kernel, the whole-row kernel (V > 4096)
F32_SHAPES = [(33, 7, 7, 8), (48, 80, 128, 88), (5, 129, 136, 136), (20, 300, 300, 304), (8, 4099, 4104, 4104)]


@pytest.mark.parametrize("M,V_,ldl,ldd", F32_SHAPES)
@pytest.mark.parametrize("shift", [0.0, 1000.0])
def test_fp32_logits_every_kernel(dev, M, V_, ldl, ldd, shift):
    from drakegpt_amd import ops
    x, t0 = LM.edge_case_logits(M, V_, seed=V_)
    buf = torch.full((M, ldl), 99.0)                                     # stale padding columns must not enter the sum
    buf[:, :V_] = x + shift
    logits = buf.to(dev)[:, :V_]
    for pattern, I, ig in IM.cases(M, V_):
        t = IM.apply_mask(t0, ig, I, V_)
        td = t.to(dev)
        cnt = ops.count_valid(td, I)
        assert cnt.cpu().numpy().tobytes() == IM.count_np(int((~ig).sum())).tobytes()
        for eps, zeta in OPTS:
            ref_rows, ref_loss, ref_grad, keep = IM.masked_objective_fp64(buf[:, :V_], t, I, eps, zeta)
            for dt in (torch.float32, torch.bfloat16):
                dl = torch.full((M, ldd), float("nan"), dtype=dt, device=dev)
                rows = ops.cross_entropy(logits, td, V_, dlogits=dl, grad_scale=1.0, label_smoothing=eps, z_loss=zeta,
                                         ignore_index=I, inv_count=cnt[1:])
                torch.cuda.synchronize()
                _check(rows, dl, V_, ref_rows, ref_loss, ref_grad, keep,
                       f"fp32 logits M={M} V={V_} shift={shift} {pattern} I={I} eps={eps} zeta={zeta} {dt}", cnt[1:])
                rows_only = ops.cross_entropy(logits, td, V_, label_smoothing=eps, z_loss=zeta, ignore_index=I, inv_count=cnt[1:])
                assert torch.equal(rows_only, rows)


@pytest.mark.parametrize("M,V_,ld", [(8, 4099, 4099), (8, 4099, 4104), (8, 50257, 50304)])
def test_bf16_logits_in_place(dev, M, V_, ld):
    """ld 4099: the generic whole-row kernel (2-byte accesses); ld % 8 == 0: the vectorised one; both overwrite the logits, an
    ignored row's with zeros"""
    from drakegpt_amd import ops
    x, t0 = LM.edge_case_logits(M, V_, seed=V_ + ld)
    buf = torch.full((M, ld), 7.0, dtype=torch.bfloat16)                 # stale padding must not survive
    buf[:, :V_] = x.bfloat16()
    for pattern, I, ig in IM.cases(M, V_):
        t = IM.apply_mask(t0, ig, I, V_)
        cnt = ops.count_valid(t.to(dev), I)
        for eps, zeta in OPTS:
            ref_rows, ref_loss, ref_grad, keep = IM.masked_objective_fp64(buf[:, :V_], t, I, eps, zeta)
            d = buf.to(dev)
            rows = ops.cross_entropy(d[:, :V_], t.to(dev), V_, dlogits=d, grad_scale=1.0, label_smoothing=eps, z_loss=zeta,
                                     ignore_index=I, inv_count=cnt[1:])
            torch.cuda.synchronize()
            _check(rows, d, V_, ref_rows, ref_loss, ref_grad, keep, f"bf16 logits in place V={V_} ld={ld} {pattern} I={I} eps={eps} zeta={zeta}",
                   cnt[1:])


@pytest.mark.parametrize("M,V_,ldl,ldd,n", [(48, 7, 7, 8, 3), (1000, 80, 80, 88, 7)])
def test_fused_loss_head(dev, M, V_, ldl, ldd, n):
    """the one-launch loss head: rows, gradient, column-sum partials over the valid rows and loss_out = the masked mean; two
    launches on new data, the counter back at zero after each; `share` leaves workgroup 1 nothing but ignored rows"""
    from drakegpt_amd import ops
    rows_per = (M + n - 1) // n
    cases = IM.cases(M, V_, rows_per=rows_per)
    assert any(p == "share" and bool(ig[rows_per:2 * rows_per].all()) for p, _, ig in cases)
    for pattern, I, ig in cases:
        for eps, zeta in OPTS:
            for dt in (torch.bfloat16, torch.float32):
                scratch = torch.zeros(n + 1, device=dev)
                for trial in range(2):
                    x, t0 = LM.edge_case_logits(M, V_, seed=M + V_ + trial)
                    t = IM.apply_mask(t0, ig, I, V_)
                    buf = torch.full((M, ldl), 99.0)
                    buf[:, :V_] = x
                    ref_rows, ref_loss, ref_grad, keep = IM.masked_objective_fp64(x, t, I, eps, zeta)
                    dl = torch.full((M, ldd), float("nan"), dtype=dt, device=dev)
                    part = torch.full((n, 200), float("nan"), device=dev)
                    loss = torch.full((), float("nan"), device=dev)
                    logits = buf.to(dev)[:, :V_]
                    cnt = ops.count_valid(t.to(dev), I)
                    rows = ops.cross_entropy_fused(logits, t.to(dev), V_, dl, 1.0, part[:, 3:], 200, n, scratch, loss, 1.0,
                                                   label_smoothing=eps, z_loss=zeta, ignore_index=I, inv_count=cnt[1:])
                    torch.cuda.synchronize()
                    name = f"fused head M={M} V={V_} {pattern} I={I} eps={eps} zeta={zeta} {dt} launch {trial}"
                    _check(rows, dl, V_, ref_rows, ref_loss, ref_grad, keep, name)
                    e_loss = abs(loss.item() - ref_loss.item())
                    cs, ref_cs = part[:, 3:3 + V_].double().sum(0).cpu(), ref_grad.sum(0)
                    e_cs = rel(cs, ref_cs)
                    print(f"{name}: loss_out {e_loss:.3e} column sums {e_cs:.3e} (largest {ref_cs.abs().max().item():.3e})")
                    assert e_loss < 1e-5 * max(1.0, abs(ref_loss.item())), name
                    assert e_cs < 1e-4 or ref_cs.abs().max() < 1e-6, (name, e_cs)
                    if pattern == "share":             # a workgroup with nothing but ignored rows: a partial row of exact zeros
                        assert torch.equal(part[1, 3:3 + V_].cpu(), torch.zeros(V_)), name
                    assert torch.isnan(part[:, :3]).all() and torch.isnan(part[:, 3 + V_:]).all()
                    assert scratch[n].view(torch.int32).item() == 0


@pytest.mark.parametrize("M", [1, 33, 1000, 16384])
def test_count_valid_bit_exact(dev, M):
    from drakegpt_amd import ops
    g = torch.Generator().manual_seed(M)
    t = torch.randint(0, V, (M,), generator=g)
    for I in IM.IGNORE_VALUES:
        for frac in (0.0, 0.4, 1.0):
            tt = IM.apply_mask(t, torch.rand(M, generator=g) < frac, I, V)
            out = torch.full((4,), float("nan"), device=dev)
            got = ops.count_valid(tt.to(dev), I, out=out[1:3])
            torch.cuda.synchronize()
            n = int((tt != I).sum())
            assert got.cpu().numpy().tobytes() == IM.count_np(n).tobytes(), (M, I, frac, got, n)
            assert torch.isnan(out[0]) and torch.isnan(out[3])


def test_nothing_counts(dev):
    """N = 0: the count is {0, inf}, every gradient row is exact zeros (torch's are NaN), the mean is NaN (as torch's)"""
    from drakegpt_amd import ops
    for M, V_, ldd, dt_l in ((33, 80, 88, torch.float32), (5, 300, 304, torch.float32), (4, 4099, 4104, torch.float32), (4, 4099, 4104, torch.bfloat16)):
        x, _ = LM.edge_case_logits(max(M, 5), V_, seed=2)
        t = torch.full((M,), -100, dtype=torch.long, device=dev)
        cnt = ops.count_valid(t, -100)
        assert cnt[0].item() == 0.0 and cnt[1].item() == float("inf")
        logits = torch.zeros((M, ldd), dtype=dt_l, device=dev)
        logits[:, :V_] = x[:M].to(dev)
        dl = torch.full((M, ldd), float("nan"), dtype=dt_l, device=dev)
        rows = ops.cross_entropy(logits[:, :V_], t, V_, dlogits=dl, grad_scale=1.0, ignore_index=-100, inv_count=cnt[1:])
        torch.cuda.synchronize()
        assert torch.equal(dl, torch.zeros_like(dl)) and torch.equal(rows, torch.zeros_like(rows))
        assert torch.isnan(ops.reduce_sum(rows, 1.0, scale_dev=cnt[1:]))
    n, M = 3, 48
    dl = torch.full((M, 88), float("nan"), device=dev)
    loss, scratch, part = torch.zeros((), device=dev), torch.zeros(n + 1, device=dev), torch.full((n, 88), float("nan"), device=dev)
    t = torch.full((M,), 3, dtype=torch.long, device=dev)
    cnt = ops.count_valid(t, 3)
    ops.cross_entropy_fused(torch.randn(M, V, device=dev), t, V, dl, 1.0, part, 88, n, scratch, loss, 1.0, ignore_index=3, inv_count=cnt[1:])
    torch.cuda.synchronize()
    assert torch.equal(dl, torch.zeros_like(dl)) and torch.isnan(loss) and torch.equal(part[:, :V], torch.zeros_like(part[:, :V]))


def test_entry_points_reject_bad_arguments(dev):
    """return codes and Python errors only: nothing is launched (DG_ERR_ARG = -1)"""
    from drakegpt_amd import _lib, ops
    M, V_ = 8, 80
    x = torch.randn(M, V_, device=dev)
    t = torch.zeros(M, dtype=torch.long, device=dev)
    rows = torch.full((M,), 5.0, device=dev)
    inv = torch.ones(1, device=dev)
    s = ops._stream()
    f = _lib.lib.dg_cross_entropy_ignore
    assert f(x.data_ptr(), _lib.DG_F32, V_, t.data_ptr(), rows.data_ptr(), None, 0, _lib.DG_F32, 1.0, None, M, V_, 0.0, 0.0, -100, None, s) == -1
    assert f(x.data_ptr(), _lib.DG_F32, V_, t.data_ptr(), rows.data_ptr(), None, 0, _lib.DG_F32, 1.0, None, M, V_, 1.0, 0.0, -100, inv.data_ptr(), s) == -1
    g = _lib.lib.dg_cross_entropy_fused_ignore
    dl = torch.full((M, 88), 5.0, device=dev)
    assert g(x.data_ptr(), V_, t.data_ptr(), rows.data_ptr(), dl.data_ptr(), 88, _lib.DG_F32, 1.0, M, V_, None, 0, 2, None, None, None, 1.0,
             0.0, 0.0, -100, None, s) == -1
    assert _lib.lib.dg_ce_count_valid(t.data_ptr(), M, -100, None, s) == -1
    assert _lib.lib.dg_ce_count_valid(t.data_ptr(), 0, -100, inv.data_ptr(), s) == -1
    assert _lib.lib.dg_reduce_sum_scaled(rows.data_ptr(), M, 1.0, None, inv.data_ptr(), s) == -1
    with pytest.raises(ValueError, match="inv_count"):
        ops.cross_entropy(x, t, V_, dlogits=dl, ignore_index=-100)
    with pytest.raises(ValueError, match="inv_count"):
        ops.cross_entropy(x, t, V_, inv_count=inv)
    with pytest.raises(ValueError, match="ignore_index"):
        ops.cross_entropy(x, t, V_, ignore_index=3.0, inv_count=inv)
    b = torch.zeros(M, 128, dtype=torch.bfloat16, device=dev)
    q8 = torch.zeros(M, 128, device=dev).to(torch.float8_e5m2)
    with pytest.raises(ValueError, match="ignore_index"):
        ops.cross_entropy_fp8(b[:, :V_], t, V_, b, 1.0 / M, q8, ignore_index=-100)
    torch.cuda.synchronize()
    assert torch.all(rows == 5.0) and torch.all(dl == 5.0) and torch.all(b == 0)


# ------------------------------------------------------------------------------------------------ autograd path
@pytest.fixture(scope="module")
def fix(golden_dir):
    return torch.load(os.path.join(golden_dir, "traj5_TransformerLM.pt"), weights_only=True)


def _masked_y(y, I=-100):
    """a third of the targets (every third position) set to I"""
    y = y.clone()
    y.view(-1)[::3] = I
    return y


def _oracle(sd, x, y, I, eps=0.0, zeta=0.0, **kw):
    """autograd through the CPU oracle's logits with torch's own F.cross_entropy(ignore_index=): (loss, {name: gradient})"""
    from oracle import drake_ref as R
    keys = R.trainable_keys("TransformerLM", sd)
    work, leaves = dict(sd), []
    for k in keys:
        leaf = sd[k].detach().clone().requires_grad_(True)
        work[k] = leaf
        leaves.append(leaf)
    logits = R.lm_forward("TransformerLM", work, x, **kw)[0]
    logits, t = logits.reshape(-1, logits.shape[-1]), y.reshape(-1)
    loss = torch.nn.functional.cross_entropy(logits, t, ignore_index=I, label_smoothing=float(eps))
    if zeta:
        keep = t != I
        loss = loss + float(zeta) * (torch.logsumexp(logits, 1).pow(2) * keep).sum() / keep.sum()
    gs = torch.autograd.grad(loss, leaves, allow_unused=True)
    return loss.item(), dict(zip(keys, gs))


@pytest.fixture(scope="module")
def tiny_ref(fix):
    """the oracle's masked loss and gradients of the tiny TransformerLM on batch 0, once for the module and the engine tests"""
    sd = {k: v.clone() for k, v in fix["init"].items()}
    return _oracle(sd, fix["x"][0], _masked_y(fix["y"][0]), -100)


def _tiny_model(dev, fix):
    import drakegpt_amd as D
    m = D.TransformerLM(V, 32, 8, 4, 3, 0.0)
    m.load_state_dict(fix["init"])
    return m.to(dev).train()


def test_functional_cross_entropy_backward(dev):
    """HF.cross_entropy(..., ignore_index=) with (3 * loss).backward(): grad_scale = 3 / N, the 3 through grad_scale_dev"""
    from drakegpt_amd import functional as HF
    M, V_ = 20, 300
    x, t0 = LM.edge_case_logits(M, V_, seed=5)
    for pattern, I, ig in IM.cases(M, V_):
        t = IM.apply_mask(t0, ig, I, V_)
        for eps, zeta in OPTS:
            xd = x.to(dev).requires_grad_(True)
            loss = HF.cross_entropy(xd, t.to(dev), eps, zeta, ignore_index=I)
            (3 * loss).backward()
            _, ref_loss, ref_grad, keep = IM.masked_objective_fp64(x, t, I, eps, zeta, grad_scale=3.0)
            assert abs(loss.item() - ref_loss.item()) < 1e-5 * max(1.0, ref_loss.item())
            assert rel(xd.grad, ref_grad) < 1e-6, rel(xd.grad, ref_grad)
            assert torch.equal(xd.grad.cpu()[ig], torch.zeros(int(ig.sum()), V_))


def test_module_path_train_and_eval(dev, fix, tiny_ref):
    """train(): the masked loss and every gradient against the oracle (loss 1e-4, flat gradient 2e-4, per tensor 3e-4); eval(): the
    same masked loss; without the option the same targets raise, with it a -1 still does"""
    x, y = fix["x"][0].to(dev), _masked_y(fix["y"][0]).to(dev)
    m = _tiny_model(dev, fix).set_loss_options(ignore_index=-100)
    _, loss = m(x, y)
    loss.backward()
    ref_loss, gr = tiny_ref
    assert abs(loss.item() - ref_loss) < 1e-4 * abs(ref_loss), (loss.item(), ref_loss)
    named = dict(m.named_parameters())
    keys = [k for k in gr if gr[k] is not None]
    flat = rel(torch.cat([named[k].grad.reshape(-1) for k in keys]), torch.cat([gr[k].reshape(-1) for k in keys]))
    assert flat < 2e-4, flat
    for k in keys:
        assert rel(named[k].grad, gr[k]) < 3e-4, (k, rel(named[k].grad, gr[k]))
    m.eval()
    assert abs(m(x, y)[1].item() - ref_loss) < 1e-4 * abs(ref_loss)
    with pytest.raises(IndexError):
        _tiny_model(dev, fix)(x, y)
    bad = y.clone()
    bad[0, 1] = -1
    with pytest.raises(IndexError):
        m(x, bad)


def test_bigram_forward_takes_the_option(dev):
    import drakegpt_amd as D
    m = D.BigramLM(V).to(dev).train().set_loss_options(ignore_index=-100)
    g = torch.Generator().manual_seed(2)
    x, y = torch.randint(0, V, (4, 8), generator=g), _masked_y(torch.randint(0, V, (4, 8), generator=g))
    logits, loss = m(x.to(dev), y.to(dev))
    _, ref_loss, _, _ = IM.masked_objective_fp64(logits, y.reshape(-1), -100)
    assert abs(loss.item() - ref_loss.item()) < 1e-5 * ref_loss.item()
    assert abs(m.eval()(x.to(dev), y.to(dev))[1].item() - ref_loss.item()) < 1e-5 * ref_loss.item()


# ------------------------------------------------------------------------------------------------ engine
def _tiny_engine(dev, fix, B=32, **kw):
    from drakegpt_amd.engine import TrainEngine
    m = _tiny_model(dev, fix)
    return m, TrainEngine(m, B, 8, lr=1e-3, betas=(0.9, 0.95), **kw)


def _same_grads(a, b):
    for k in a:
        if k == "token_embedding_table.weight":          # (fp32 atomics in a free order in this configuration)
            assert torch.allclose(a[k], b[k], rtol=1e-5, atol=1e-9)
        else:
            assert torch.equal(a[k], b[k]), k


def test_tiny_fp32_engine_step(dev, fix, tiny_ref):
    """one step() on masked targets: loss and named_grads() against the oracle (loss 1e-4, flat gradient 1e-4, per tensor 3e-4);
    the captured graph and the eager program agree bit for bit (but for the token table); last_token_count is N; eval_loss is the
    masked loss; a default engine refuses the targets"""
    x, y = fix["x"][0].to(dev), _masked_y(fix["y"][0]).to(dev)
    n_valid = int((y != -100).sum())
    ref_loss, gr = tiny_ref
    res = []
    for graph in (True, False):
        m, eng = _tiny_engine(dev, fix, use_graph=graph, ignore_index=-100)
        ev = eng.eval_loss(x, y)
        assert abs(ev.item() - ref_loss) < 1e-4 * ref_loss
        eng.set_batch(x, y)
        loss = eng.step().item()
        torch.cuda.synchronize()
        assert eng.last_token_count.dim() == 0 and eng.last_token_count.item() == n_valid
        got = {k: v.detach().clone().cpu() for k, v in eng.named_grads().items()}
        assert abs(loss - ref_loss) < 1e-4 * ref_loss, (loss, ref_loss)
        keys = [k for k in gr if gr[k] is not None]
        assert rel(torch.cat([got[k].reshape(-1) for k in keys]), torch.cat([gr[k].reshape(-1) for k in keys])) < 1e-4
        for k in keys:
            assert rel(got[k], gr[k]) < 3e-4, (k, rel(got[k], gr[k]))
        res.append((loss, got))
    assert res[0][0] == res[1][0]
    _same_grads(res[0][1], res[1][1])
    _, plain = _tiny_engine(dev, fix)
    assert plain.ignore_index is None and plain.token_count is None and plain.last_token_count is None
    with pytest.raises(IndexError):
        plain.set_batch(x, y)
    bad = y.clone()
    bad[0, 1] = -1
    with pytest.raises(IndexError):
        eng.set_batch(x, bad)


def test_default_engines_agree_bit_for_bit(dev, fix):
    """two default engines, one step each on the same batch: the same loss and gradients, and none of the option's buffers"""
    x, y = fix["x"][0].to(dev), fix["y"][0].to(dev)
    res = []
    for _ in range(2):
        _, eng = _tiny_engine(dev, fix)
        eng.set_batch(x, y)
        loss = eng.step().item()
        torch.cuda.synchronize()
        res.append((loss, {k: v.detach().clone().cpu() for k, v in eng.named_grads().items()}))
        assert "ignore_index" not in eng.state_dict()["meta"]
    assert res[0][0] == res[1][0]
    _same_grads(res[0][1], res[1][1])


def test_corpus_path_in_vocabulary_ignore_with_accumulation(dev, fix):
    """accum_steps = 2, batches from staged offset rows, I an ordinary token that is never a target (the one that both
    micro-batches hold most often as a target): step() returns the mean of the two masked micro-batch means (the bound of
    test_accumulation_returns_the_mean_objective: 1e-4)"""
    from oracle import drake_ref as R
    B, T = 16, 8
    data = torch.randint(0, V, (5000,), generator=torch.Generator().manual_seed(42))
    rows = torch.randint(0, 5000 - T - 1, (2, B), generator=torch.Generator().manual_seed(3))
    seen = torch.stack([torch.bincount(torch.stack([data[o + 1:o + T + 1] for o in r.tolist()]).reshape(-1), minlength=V) for r in rows])
    I = int(seen.min(0).values.argmax())
    assert seen[:, I].min() > 0
    m, eng = _tiny_engine(dev, fix, B=B, accum_steps=2, ignore_index=I)
    eng.set_corpus(data.to(dev))
    eng.stage_offsets(rows)
    mean = eng.step().item()
    sd = {k: v.clone() for k, v in fix["init"].items()}
    want, counts = [], []
    for r in rows:
        x = torch.stack([data[o:o + T] for o in r.tolist()])
        y = torch.stack([data[o + 1:o + T + 1] for o in r.tolist()])
        logits = R.lm_forward("TransformerLM", sd, x)[0]
        want.append(IM.masked_objective_fp64(logits.reshape(-1, V), y.reshape(-1), I)[1].item())
        counts.append(int((y != I).sum()))
    assert all(0 < c < B * T for c in counts)                      # both micro-batches hold the ignored token, each its own count
    assert abs(mean - sum(want) / 2) < 1e-4 * mean, (mean, want)
    assert eng.last_token_count.item() == counts[1]
    assert eng.step_count() == 1 and eng.micro_step_count() == 2


SV, SC, SNH, ST, SB, SP, SL = 80, 384, 6, 256, 8, 0.2, 2          # the bf16 configuration of tests/test_gpu_schedule.py


def _scaled(dev, model_seed=42, seed=20240607, use_graph=True, **kw):
    import drakegpt_amd as D
    from drakegpt_amd.engine import TrainEngine
    torch.manual_seed(model_seed)
    m = D.TransformerLM(SV, SC, ST, SNH, SL, SP, precision="bf16").to(dev).train()
    eng = TrainEngine(m, SB, ST, lr=3e-4, betas=(0.9, 0.95), seed=seed, use_graph=use_graph, weight_decay=0.1, **kw)
    assert eng.onehot is not None and eng.grouped_dw            # no atomics in the step: bit-reproducible across engines
    return m, eng


def test_scaled_bf16_engine_uses_the_fused_head(dev, monkeypatch):
    """the headline dispatch (chain kernel, one-launch loss head) with the option: the fused head is the one called, with the
    option and the engine's count buffer; its gradient rows of the ignored targets are zeros and the step's loss is the masked mean
    of its own rows"""
    from drakegpt_amd import ops
    calls = []
    real = ops.cross_entropy_fused

    def spy(*a, **kw):
        rows = real(*a, **kw)
        calls.append((kw, rows.clone(), a[3].clone()))
        return rows
    monkeypatch.setattr(ops, "cross_entropy_fused", spy)
    m, eng = _scaled(dev, use_graph=False, ignore_index=-100)          # (eager: the spy keeps copies of what the launch wrote)
    assert eng.chain_full and not eng.bf16_logits
    g = torch.Generator().manual_seed(3)
    x, y = torch.randint(0, SV, (SB, ST), generator=g), _masked_y(torch.randint(0, SV, (SB, ST), generator=g))
    eng.set_batch(x.to(dev), y.to(dev))
    loss = eng.step().item()
    torch.cuda.synchronize()
    assert calls and all(kw.get("ignore_index") == -100 and kw["inv_count"].data_ptr() == eng.token_count.data_ptr() + 4 for kw, _, _ in calls)
    ig = (y.reshape(-1) == -100)
    n = int((~ig).sum())
    assert eng.last_token_count.item() == n
    _, rows, dl = calls[-1]
    assert torch.equal(rows.cpu()[ig], torch.zeros(int(ig.sum()))) and torch.equal(dl.cpu()[ig], torch.zeros((int(ig.sum()), dl.shape[1]), dtype=dl.dtype))
    want = rows.double().sum().item() / n
    assert abs(loss - want) < 1e-5 * want, (loss, want)
    assert abs(eng.eval_loss(x.to(dev), y.to(dev)).item() - loss) < 0.1 * loss          # (dropout off: close, not equal)


def test_bf16_logits_engine_gradient_in_place(dev, monkeypatch):
    """the smallest vocabulary with bf16 logits (V 4099): the engine hands the option to the whole-row kernel; the in-place gradient
    matches fp64 on the engine's own logits and the ignored rows of the buffer are zeros after the step"""
    import drakegpt_amd as D
    from drakegpt_amd import ops
    from drakegpt_amd.engine import TrainEngine
    V_, B, T = 4099, 4, 16
    seen = {}
    real = ops.cross_entropy

    def spy(logits, targets, Vv, dlogits=None, **kw):
        if dlogits is not None and logits.dtype == torch.bfloat16:
            seen["logits"], seen["kw"] = logits.clone(), kw
            seen["in_place"] = dlogits.data_ptr() == logits.data_ptr()
        rows = real(logits, targets, Vv, dlogits=dlogits, **kw)
        if dlogits is not None and logits.dtype == torch.bfloat16:
            seen["rows"], seen["grad"] = rows.clone(), dlogits.clone()
        return rows
    monkeypatch.setattr(ops, "cross_entropy", spy)
    torch.manual_seed(42)
    m = D.TransformerLM(V_, 64, T, 2, 1, 0.0, precision="bf16").to(dev).train()
    eng = TrainEngine(m, B, T, lr=1e-3, use_graph=False, ignore_index=-100)
    assert eng.bf16_logits and not eng.fp8_head
    g = torch.Generator().manual_seed(4)
    x, y = torch.randint(0, V_, (B, T), generator=g), _masked_y(torch.randint(0, V_, (B, T), generator=g))
    eng.set_batch(x.to(dev), y.to(dev))
    loss = eng.step().item()
    torch.cuda.synchronize()
    assert seen["in_place"] and seen["kw"]["ignore_index"] == -100 and seen["kw"]["grad_scale"] == 1.0
    ref_rows, ref_loss, ref_grad, keep = IM.masked_objective_fp64(seen["logits"], y.reshape(-1), -100)
    _check(seen["rows"], seen["grad"], V_, ref_rows, ref_loss, ref_grad, keep, "engine, bf16 logits in place")
    assert abs(loss - ref_loss.item()) < 1e-5 * ref_loss.item()


def test_fp8_head_refuses_ignore_index(dev):
    import drakegpt_amd as D
    from drakegpt_amd.engine import TrainEngine
    torch.manual_seed(42)
    m = D.TransformerLM(50257, 1024, 1024, 16, 1, 0.0, precision="fp8").to(dev).train()          # (test_fp8_head_engine_step's)
    with pytest.raises(ValueError, match=r"ignore_index cannot be combined with the fp8 loss head.*1 / N"):
        TrainEngine(m, 1, 1024, lr=1e-4, seed=3, use_graph=False, ignore_index=-100)
    assert TrainEngine(m, 1, 1024, lr=1e-4, seed=3, use_graph=False).fp8_head


# ------------------------------------------------------------------------------------------------ resume
def test_resume_with_ignore_index_bit_for_bit(dev, tmp_path):
    """3 + 3 steps equal 6 steps bit for bit with the option on (bf16, corpus path, an in-vocabulary I); a state saved with it is
    refused by an engine without it or with another I, and the reverse"""
    from drakegpt_amd import checkpoint as CK
    corpus = torch.randint(0, SV, (20_000,), generator=torch.Generator().manual_seed(1)).to(dev)
    rows = torch.randint(0, 20_000 - ST - 1, (6, SB), generator=torch.Generator().manual_seed(2))
    _, A = _scaled(dev, ignore_index=3)
    A.set_corpus(corpus)
    A.stage_offsets(rows)
    for _ in range(3):
        A.step()
    path = str(tmp_path / "ign.state.pt")
    CK.save_train_state(path, A.state_dict())
    sd = CK.load_train_state(path)
    assert sd["meta"]["ignore_index"] == 3
    la = [A.step().item() for _ in range(3)]
    _, Bn = _scaled(dev, model_seed=7, seed=99, ignore_index=3)
    Bn.set_corpus(corpus)
    Bn.load_state_dict(sd)
    lb = [Bn.step().item() for _ in range(3)]
    torch.cuda.synchronize()
    assert la == lb, (la, lb)
    for k in ("flat", "m_", "v_", "shadow"):
        assert torch.equal(getattr(A, k), getattr(Bn, k)), k
    assert A.step_count() == Bn.step_count() == 6
    assert 0 < A.last_token_count.item() < SB * ST
    _, Dn = _scaled(dev, model_seed=9, seed=6)
    Dn.set_corpus(corpus)
    before = Dn.flat.clone()
    with pytest.raises(ValueError, match=r"meta\.ignore_index differs.*saved 3.*None"):
        Dn.load_state_dict(sd)
    assert torch.equal(Dn.flat, before)
    _, En = _scaled(dev, model_seed=9, seed=6, ignore_index=-100)
    En.set_corpus(corpus)
    with pytest.raises(ValueError, match=r"meta\.ignore_index differs.*saved 3.*-100"):
        En.load_state_dict(sd)
    plain = Dn.state_dict()
    assert "ignore_index" not in plain["meta"]                     # the file a default engine always wrote
    with pytest.raises(ValueError, match=r"meta\.ignore_index differs.*saved None.*3"):
        Bn.load_state_dict(plain)
    Dn.load_state_dict(plain)


# ------------------------------------------------------------------------------------------------ harness
def test_train_harness_with_ignore_token(dev, tmp_path, capsys):
    """4 iterations on each training path (engine, autograd) with --ignore-token, in the style of test_train_harness_with_both_flags;
    the evaluation lines are there and sane (about log V on the synthetic uniform corpus)"""
    import json
    import math
    from drakegpt_amd import train
    from drakegpt_amd.config import DRAKE_VOCAB_SIZE
    flags = ["--ignore-token", "3", "--iters", "4", "--eval-interval", "2", "--eval-iters", "2", "--precision", "fp32", "--no-save",
             "--sample", "3"]
    for model in ("TransformerLM", "BlocksLM"):
        train.main(["--model", model] + flags)
        out = capsys.readouterr().out
        lines = [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")]
        assert len(lines) == 2 and all(abs(ln["val_loss"] - math.log(DRAKE_VOCAB_SIZE)) < 0.5 for ln in lines), lines
