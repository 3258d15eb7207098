"""GPU: label smoothing and z-loss inside the loss-head kernels, through every dispatch path of dg_cross_entropy_smooth /
dg_cross_entropy_fp8_smooth / dg_cross_entropy_fused_smooth, the autograd path, the training engine, resume and the harness.

The reference is the explicit formula in fp64 (tests/loss_model.py) evaluated on the logits as stored (bf16 logits: the bf16
values).  Bounds are those of the existing tests of the plain kernels (tests/test_gpu_ops.py): rows 1e-6 (norm), mean loss 1e-5,
gradient 1e-6 (fp32) / 5e-3 (bf16) with every bf16 element inside the single-rounding envelope, fused column sums 1e-4, padding
columns of dlogits exactly zero.

(A row of equal logits has the off-target gradient grad_scale (1 - eps) / V, which is zero only without smoothing: the row is
one of the edge cases, compared with the formula like every other.)"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_model as LM  # noqa: E402

pytestmark = pytest.mark.gpu
V = 80
OPTS = [(0.125, 0.0), (0.0, 1e-2), (0.125, 1e-2)]


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _check(rows, dl, V_, ref_rows, ref_grad, name):
    """the bounds of test_cross_entropy_and_reduce; every figure printed before it is asserted"""
    from oracle import parity as P
    e_rows, e_loss, e_grad = rel(rows, ref_rows), abs(rows.double().mean().item() - ref_rows.mean().item()), rel(dl[:, :V_], ref_grad)
    print(f"{name}: rows {e_rows:.3e} loss {e_loss:.3e} gradient {e_grad:.3e}")
    assert e_rows < 1e-6, (name, e_rows)
    assert e_loss < 1e-5 * max(1.0, abs(ref_rows.mean().item())), (name, e_loss)
    assert e_grad < (1e-6 if dl.dtype == torch.float32 else 5e-3), (name, e_grad)
    if dl.dtype == torch.bfloat16:
        P.assert_within_rounding(dl[:, :V_], ref_grad, P.single_rounding_envelope(ref_grad, V_), 1, name)
    assert torch.all(dl[:, V_:] == 0), name


# ------------------------------------------------------------------------------------------------ kernels
# fp32 logits: (M, V, ldl, ldd) -- the small kernel (width <= 128), the wave-per-row kernel, the whole-row kernel (V > 4096)
F32_SHAPES = [(33, 7, 7, 8), (48, 80, 128, 88), (5, 129, 136, 136), (20, 300, 300, 304), (8, 4099, 4104, 4104)]


@pytest.mark.parametrize("M,V_,ldl,ldd", F32_SHAPES)
@pytest.mark.parametrize("shift", [0.0, 1000.0])
def test_fp32_logits_every_kernel(dev, M, V_, ldl, ldd, shift):
    """shift 1000: the conditioning case -- all logits moved by +1000, against fp64 on the shifted fp32 values"""
    from drakegpt_amd import ops
    x, t = LM.edge_case_logits(M, V_, seed=V_)
    buf = torch.full((M, ldl), 99.0)                                     # stale padding columns must not enter the sum
    buf[:, :V_] = x + shift
    logits = buf.to(dev)[:, :V_]
    for eps, zeta in OPTS:
        ref_rows, ref_grad = LM.objective_fp64(buf[:, :V_], t, eps, zeta, grad_scale=1.0 / M)
        for dt in (torch.float32, torch.bfloat16):
            dl = torch.full((M, ldd), float("nan"), dtype=dt, device=dev)
            rows = ops.cross_entropy(logits, t.to(dev), V_, dlogits=dl, grad_scale=1.0 / M, label_smoothing=eps, z_loss=zeta)
            torch.cuda.synchronize()
            _check(rows, dl, V_, ref_rows, ref_grad, f"fp32 logits M={M} V={V_} shift={shift} eps={eps} zeta={zeta} {dt}")
            rows_only = ops.cross_entropy(logits, t.to(dev), V_, label_smoothing=eps, z_loss=zeta)      # no gradient asked for
            assert torch.equal(rows_only, rows)


@pytest.mark.parametrize("M,V_,ld", [(8, 4099, 4099), (8, 4099, 4104), (8, 50257, 50304)])
def test_bf16_logits_in_place(dev, M, V_, ld):
    """ld 4099: the generic whole-row kernel (2-byte accesses); ld % 8 == 0: the vectorised one; both overwrite the logits"""
    from drakegpt_amd import ops
    x, t = LM.edge_case_logits(M, V_, seed=V_ + ld)
    buf = torch.full((M, ld), 7.0, dtype=torch.bfloat16)                 # stale padding must not survive
    buf[:, :V_] = x.bfloat16()
    for eps, zeta in OPTS:
        ref_rows, ref_grad = LM.objective_fp64(buf[:, :V_], t, eps, zeta, grad_scale=1.0 / M)
        d = buf.to(dev)
        rows = ops.cross_entropy(d[:, :V_], t.to(dev), V_, dlogits=d, grad_scale=1.0 / M, label_smoothing=eps, z_loss=zeta)
        torch.cuda.synchronize()
        _check(rows, d, V_, ref_rows, ref_grad, f"bf16 logits in place V={V_} ld={ld} eps={eps} zeta={zeta}")


def test_fp8_gradient_copy_with_smoothing(dev):
    """the checks of test_cross_entropy_fp8_gradient_copy with label smoothing: rows and the bf16 gradient are those of
    dg_cross_entropy_smooth, the e5m2 copy times grad_scale / 57344 is the fp64 gradient to e5m2 rounding, pad columns zero"""
    from drakegpt_amd import ops
    M, V_, ld, eps = 8, 50257, 50304, 0.125
    x, t = LM.edge_case_logits(M, V_, seed=3)
    buf = torch.zeros(M, ld, dtype=torch.bfloat16)
    buf[:, :V_] = x.bfloat16()
    ref_rows, ref = LM.objective_fp64(buf[:, :V_], t, eps, 0.0, grad_scale=1.0 / M)
    assert ref.abs().max().item() <= 1.0 / M                              # the bound the a-priori scale rests on
    a, b = buf.to(dev), buf.to(dev)
    rows0 = ops.cross_entropy(a[:, :V_], t.to(dev), V_, dlogits=a, grad_scale=1.0 / M, label_smoothing=eps)
    q8 = torch.full((M, ld), 7.0, device=dev).to(torch.float8_e5m2)
    rows1 = ops.cross_entropy_fp8(b[:, :V_], t.to(dev), V_, b, 1.0 / M, q8, label_smoothing=eps)
    torch.cuda.synchronize()
    assert torch.equal(rows0, rows1) and torch.equal(a, b) and rel(rows1, ref_rows) < 1e-6
    _check(rows1, b, V_, ref_rows, ref, "fp8 entry, bf16 gradient")
    deq = q8.float().cpu().double() * (1.0 / M / 57344.0)
    assert torch.all(deq[:, V_:] == 0)
    assert rel(deq[:, :V_], ref) < 4e-2, rel(deq[:, :V_], ref)
    el = ((deq[:, :V_] - ref).abs() / ref.abs().clamp_min(1e-30))
    big = ref.abs() > 1e-4 / M                     # above e5m2's subnormal range at this scale
    assert el[big].max().item() <= 2 ** -3 * 1.02, el[big].max().item()
    assert torch.isfinite(deq).all()


@pytest.mark.parametrize("M,V_,ldl,ldd,n", [(48, 7, 7, 8, 3), (1000, 80, 80, 88, 7)])
def test_fused_loss_head(dev, M, V_, ldl, ldd, n):
    """the one-launch loss head with the options: rows, gradient, column-sum partials (non-zero once zeta > 0) and loss_out =
    loss_scale * sum of the row objectives; two launches on new data, the counter back at zero after each"""
    from drakegpt_amd import ops
    for eps, zeta in OPTS:
        for dt in (torch.bfloat16, torch.float32):
            scratch = torch.zeros(n + 1, device=dev)
            for trial in range(2):
                x, t = LM.edge_case_logits(M, V_, seed=M + V_ + trial)
                buf = torch.full((M, ldl), 99.0)
                buf[:, :V_] = x
                ref_rows, ref_grad = LM.objective_fp64(x, t, eps, zeta, grad_scale=1.0 / M)
                dl = torch.full((M, ldd), float("nan"), dtype=dt, device=dev)
                part = torch.full((n, 200), float("nan"), device=dev)
                loss = torch.full((), float("nan"), device=dev)
                logits = buf.to(dev)[:, :V_]
                rows = ops.cross_entropy_fused(logits, t.to(dev), V_, dl, 1.0 / M, part[:, 3:], 200, n, scratch, loss, 1.0 / M,
                                               label_smoothing=eps, z_loss=zeta)
                torch.cuda.synchronize()
                name = f"fused head M={M} V={V_} eps={eps} zeta={zeta} {dt} launch {trial}"
                _check(rows, dl, V_, ref_rows, ref_grad, name)
                e_loss = abs(loss.item() - ref_rows.mean().item())
                cs, ref_cs = part[:, 3:3 + V_].double().sum(0).cpu(), ref_grad.sum(0)
                e_cs = rel(cs, ref_cs)
                print(f"{name}: loss_out {e_loss:.3e} column sums {e_cs:.3e} (largest {ref_cs.abs().max().item():.3e})")
                assert e_loss < 1e-5 * max(1.0, abs(ref_rows.mean().item())), name
                assert e_cs < 1e-4 or ref_cs.abs().max() < 1e-6, (name, e_cs)
                if zeta > 0:                       # the partials are the true column sums: they add up to 2 zeta sum(lse) / M
                    tot = 2 * zeta * torch.logsumexp(x.double(), 1).sum().item() / M
                    assert abs(cs.sum().item() - tot) < 1e-4 * tot, (name, cs.sum().item(), tot)
                assert torch.isnan(part[:, :3]).all() and torch.isnan(part[:, 3 + V_:]).all()
                assert scratch[n].view(torch.int32).item() == 0


def test_entry_points_reject_bad_options(dev):
    """return codes only: nothing is launched (DG_ERR_ARG = -1); both options at 0 are the old entry point"""
    from drakegpt_amd import _lib, ops
    M, V_ = 8, 80
    x = torch.randn(M, V_, device=dev)
    t = torch.zeros(M, dtype=torch.long, device=dev)
    rows = torch.zeros(M, device=dev)
    s = ops._stream()
    f = _lib.lib.dg_cross_entropy_smooth
    for eps, zeta in ((1.0, 0.0), (-0.1, 0.0), (float("nan"), 0.0), (0.0, -1.0), (0.0, float("inf")), (0.0, float("nan"))):
        assert f(x.data_ptr(), _lib.DG_F32, V_, t.data_ptr(), rows.data_ptr(), None, 0, _lib.DG_F32, 1.0, None, M, V_, eps, zeta, s) == -1
    assert f(x.data_ptr(), _lib.DG_F32, V_, t.data_ptr(), rows.data_ptr(), None, 0, _lib.DG_F32, 1.0, None, M, V_, 0.0, 0.0, s) == 0
    torch.cuda.synchronize()
    assert torch.equal(rows, ops.cross_entropy(x, t, V_))
    g = _lib.lib.dg_cross_entropy_fused_smooth
    dl = torch.zeros(M, 88, device=dev)
    assert g(x.data_ptr(), V_, t.data_ptr(), rows.data_ptr(), dl.data_ptr(), 88, _lib.DG_F32, 1.0, M, V_, None, 0, 2, None, None, None, 1.0,
             1.5, 0.0, s) == -1
    h = _lib.lib.dg_cross_entropy_fp8_smooth
    b = torch.zeros(M, 128, dtype=torch.bfloat16, device=dev)
    q8 = torch.zeros(M, 128, device=dev).to(torch.float8_e5m2)
    assert h(b.data_ptr(), 128, t.data_ptr(), rows.data_ptr(), b.data_ptr(), 128, 1.0, M, V_, q8.data_ptr(), 128, 1.0, s) == -1


# ------------------------------------------------------------------------------------------------ autograd path
@pytest.fixture(scope="module")
def fix(golden_dir):
    return torch.load(os.path.join(golden_dir, "traj5_TransformerLM.pt"), weights_only=True)


def _oracle(sd, x, y, eps, zeta, **kw):
    """autograd through the CPU oracle's logits with the objective applied by torch: (loss, {name: gradient})"""
    from oracle import drake_ref as R
    keys = R.trainable_keys("TransformerLM", sd)
    work, leaves = dict(sd), []
    for k in keys:
        leaf = sd[k].detach().clone().requires_grad_(True)
        work[k] = leaf
        leaves.append(leaf)
    logits = R.lm_forward("TransformerLM", work, x, **kw)[0]
    loss = LM.objective_torch(logits.reshape(-1, logits.shape[-1]), y.reshape(-1), eps, zeta)
    gs = torch.autograd.grad(loss, leaves, allow_unused=True)
    return loss.item(), dict(zip(keys, gs))


@pytest.fixture(scope="module")
def tiny_ref(fix):
    """the oracle's objective and gradients of the tiny TransformerLM on batch 0, once for the module and the engine tests"""
    sd = {k: v.clone() for k, v in fix["init"].items()}
    return {o: _oracle(sd, fix["x"][0], fix["y"][0], *o) for o in OPTS + [(0.0, 0.0)]}


def _tiny_model(dev, fix):
    import drakegpt_amd as D
    m = D.TransformerLM(V, 32, 8, 4, 3, 0.0)
    m.load_state_dict(fix["init"])
    return m.to(dev).train()


def test_functional_cross_entropy_backward(dev):
    """HF.cross_entropy(..., eps, zeta) with (3 * loss).backward(): the factor arrives through grad_scale_dev"""
    from drakegpt_amd import functional as HF
    M, V_ = 20, 300
    x, t = LM.edge_case_logits(M, V_, seed=5)
    for eps, zeta in OPTS:
        xd = x.to(dev).requires_grad_(True)
        loss = HF.cross_entropy(xd, t.to(dev), eps, zeta)
        (3 * loss).backward()
        ref_rows, ref_grad = LM.objective_fp64(x, t, eps, zeta, grad_scale=3.0 / M)
        assert abs(loss.item() - ref_rows.mean().item()) < 1e-5 * max(1.0, ref_rows.mean().item())
        assert rel(xd.grad, ref_grad) < 1e-6, rel(xd.grad, ref_grad)


@pytest.mark.parametrize("eps,zeta", OPTS)
def test_module_path_train_and_eval(dev, fix, tiny_ref, eps, zeta):
    """train(): the objective and every gradient against the oracle (the bounds of the module path's train-mode comparison in
    tests/test_gpu_models.py: loss 1e-4, flat gradient 2e-4, per tensor 3e-4); eval(): the plain loss, bit for bit"""
    x, y = fix["x"][0].to(dev), fix["y"][0].to(dev)
    m = _tiny_model(dev, fix).set_loss_options(eps, zeta)
    _, loss = m(x, y)
    loss.backward()
    ref_loss, gr = tiny_ref[(eps, zeta)]
    assert abs(loss.item() - ref_loss) < 1e-4 * abs(ref_loss), (loss.item(), ref_loss)
    named = dict(m.named_parameters())
    keys = [k for k in gr if gr[k] is not None]
    flat = rel(torch.cat([named[k].grad.reshape(-1) for k in keys]), torch.cat([gr[k].reshape(-1) for k in keys]))
    assert flat < 2e-4, flat
    for k in keys:
        assert rel(named[k].grad, gr[k]) < 3e-4, (k, rel(named[k].grad, gr[k]))
    m.eval()
    plain = _tiny_model(dev, fix).eval()
    assert torch.equal(m(x, y)[1], plain(x, y)[1])
    assert abs(m(x, y)[1].item() - tiny_ref[(0.0, 0.0)][0]) < 1e-4 * tiny_ref[(0.0, 0.0)][0]


def test_bigram_forward_takes_the_options(dev):
    import drakegpt_amd as D
    m = D.BigramLM(V).to(dev).train().set_loss_options(0.125, 1e-2)
    g = torch.Generator().manual_seed(2)
    x, y = torch.randint(0, V, (4, 8), generator=g), torch.randint(0, V, (4, 8), generator=g)
    logits, loss = m(x.to(dev), y.to(dev))
    ref_rows, _ = LM.objective_fp64(logits, y.reshape(-1), 0.125, 1e-2)
    assert abs(loss.item() - ref_rows.mean().item()) < 1e-5 * ref_rows.mean().item()
    plain_rows, _ = LM.objective_fp64(logits, y.reshape(-1))
    assert abs(m.eval()(x.to(dev), y.to(dev))[1].item() - plain_rows.mean().item()) < 1e-5 * plain_rows.mean().item()


# ------------------------------------------------------------------------------------------------ engine
def _tiny_engine(dev, fix, B=32, **kw):
    from drakegpt_amd.engine import TrainEngine
    m = _tiny_model(dev, fix)
    return m, TrainEngine(m, B, 8, lr=1e-3, betas=(0.9, 0.95), **kw)


@pytest.mark.parametrize("eps,zeta", OPTS)
def test_tiny_fp32_engine_step(dev, fix, tiny_ref, eps, zeta):
    """one step(): the objective and named_grads() against the oracle (the bounds of the fp32 engine comparison: loss 1e-4, flat
    gradient 1e-4, per tensor 3e-4); eval_loss stays the plain cross entropy; the captured graph and the eager program agree bit
    for bit (but for the token table, whose rows this configuration sums with fp32 atomics in a free order)"""
    x, y = fix["x"][0].to(dev), fix["y"][0].to(dev)
    ref_loss, gr = tiny_ref[(eps, zeta)]
    res = []
    for graph in (True, False):
        m, eng = _tiny_engine(dev, fix, use_graph=graph, label_smoothing=eps, z_loss=zeta)
        _, plain_eng = _tiny_engine(dev, fix, use_graph=graph)
        ev = eng.eval_loss(x, y)
        assert torch.equal(ev, plain_eng.eval_loss(x, y)) and abs(ev.item() - tiny_ref[(0.0, 0.0)][0]) < 1e-4 * ev.item()
        eng.set_batch(x, y)
        loss = eng.step().item()
        torch.cuda.synchronize()
        got = {k: v.detach().clone().cpu() for k, v in eng.named_grads().items()}
        assert abs(loss - ref_loss) < 1e-4 * ref_loss, (loss, ref_loss)
        keys = [k for k in gr if gr[k] is not None]
        assert rel(torch.cat([got[k].reshape(-1) for k in keys]), torch.cat([gr[k].reshape(-1) for k in keys])) < 1e-4
        for k in keys:
            assert rel(got[k], gr[k]) < 3e-4, (k, rel(got[k], gr[k]))
        res.append((loss, got))
    assert res[0][0] == res[1][0]
    for k in res[0][1]:
        if k == "token_embedding_table.weight":
            assert torch.allclose(res[0][1][k], res[1][1][k], rtol=1e-5, atol=1e-9)
        else:
            assert torch.equal(res[0][1][k], res[1][1][k]), k


def test_accumulation_returns_the_mean_objective(dev, fix):
    """accum_steps = 2, batches from staged offset rows: step() returns the mean of the two micro-batch objectives"""
    eps, zeta, B, T = 0.125, 1e-2, 16, 8
    data = torch.randint(0, V, (5000,), generator=torch.Generator().manual_seed(42))
    rows = torch.randint(0, 5000 - T - 1, (2, B), generator=torch.Generator().manual_seed(3))
    m, eng = _tiny_engine(dev, fix, B=B, accum_steps=2, label_smoothing=eps, z_loss=zeta)
    eng.set_corpus(data.to(dev))
    eng.stage_offsets(rows)
    mean = eng.step().item()
    sd = {k: v.clone() for k, v in fix["init"].items()}
    want = []
    for r in rows:
        x = torch.stack([data[o:o + T] for o in r.tolist()])
        y = torch.stack([data[o + 1:o + T + 1] for o in r.tolist()])
        want.append(_oracle(sd, x, y, eps, zeta)[0])
    assert abs(mean - sum(want) / 2) < 1e-4 * mean, (mean, want)
    assert eng.step_count() == 1 and eng.micro_step_count() == 2


SV, SC, SNH, ST, SB, SP, SL = 80, 384, 6, 256, 8, 0.2, 2          # the bf16 configuration of tests/test_gpu_schedule.py


def _scaled(dev, model_seed=42, seed=20240607, **kw):
    import drakegpt_amd as D
    from drakegpt_amd.engine import TrainEngine
    torch.manual_seed(model_seed)
    m = D.TransformerLM(SV, SC, ST, SNH, SL, SP, precision="bf16").to(dev).train()
    eng = TrainEngine(m, SB, ST, lr=3e-4, betas=(0.9, 0.95), seed=seed, use_graph=True, weight_decay=0.1, **kw)
    assert eng.onehot is not None and eng.grouped_dw            # no atomics in the step: bit-reproducible across engines
    return m, eng


def test_scaled_bf16_engine_uses_the_fused_head(dev, monkeypatch):
    """the headline dispatch (chain kernel, one-launch loss head) with the options: the first step's objective against the
    oracle's bf16 rounding model with the kernels' own dropout masks (the loss bound of tests/test_gpu_engine_oracle.py: 1e-4)"""
    from drakegpt_amd import ops
    from oracle import rng_ref
    eps, zeta, seed = 0.125, 1e-2, 20240607
    calls = []
    real = ops.cross_entropy_fused

    def spy(*a, **kw):
        calls.append(kw)
        return real(*a, **kw)
    monkeypatch.setattr(ops, "cross_entropy_fused", spy)
    m, eng = _scaled(dev, seed=seed, label_smoothing=eps, z_loss=zeta)
    assert eng.chain_full and not eng.bf16_logits
    g = torch.Generator().manual_seed(3)
    x, y = torch.randint(0, SV, (SB, ST), generator=g), torch.randint(0, SV, (SB, ST), generator=g)
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    eng.set_batch(x.to(dev), y.to(dev))
    loss = eng.step().item()
    torch.cuda.synchronize()
    assert calls and all(kw.get("label_smoothing") == eps and kw.get("z_loss") == zeta for kw in calls)      # the fused head is in use
    masks = rng_ref.transformer_masks(seed, 0, SP, SB, ST, SC, SNH, SL)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    want, _ = _oracle(sd, x, y, eps, zeta, p=SP, training=True, masks=masks, bf16=True, stream_bf16=eng.stream_dtype == torch.bfloat16)
    print(f"scaled bf16 engine, fused head with options: loss {loss:.6f} oracle {want:.6f}")
    assert abs(loss - want) < 1e-4 * want, (loss, want)
    plain = eng.eval_loss(x.to(dev), y.to(dev)).item()
    assert abs(plain - loss) > 1e-2 * loss                                   # evaluation reports the plain cross entropy


def test_bf16_logits_engine_gradient_in_place(dev, monkeypatch):
    """the smallest vocabulary with bf16 logits (V 4099): the engine hands both options to the whole-row kernel, whose in-place
    gradient matches fp64 on the engine's own logits"""
    import drakegpt_amd as D
    from drakegpt_amd import ops
    from drakegpt_amd.engine import TrainEngine
    eps, zeta, V_, B, T = 0.125, 1e-2, 4099, 4, 16
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
    eng = TrainEngine(m, B, T, lr=1e-3, use_graph=False, label_smoothing=eps, z_loss=zeta)
    assert eng.bf16_logits and not eng.fp8_head
    g = torch.Generator().manual_seed(4)
    x, y = torch.randint(0, V_, (B, T), generator=g), torch.randint(0, V_, (B, T), generator=g)
    eng.set_batch(x.to(dev), y.to(dev))
    loss = eng.step().item()
    torch.cuda.synchronize()
    M = B * T
    assert seen["in_place"] and seen["kw"]["label_smoothing"] == eps and seen["kw"]["z_loss"] == zeta
    ref_rows, ref_grad = LM.objective_fp64(seen["logits"], y.reshape(-1), eps, zeta, grad_scale=1.0 / M)
    _check(seen["rows"], seen["grad"], V_, ref_rows, ref_grad, "engine, bf16 logits in place")
    assert abs(loss - ref_rows.mean().item()) < 1e-5 * ref_rows.mean().item()


def test_fp8_head_takes_smoothing_and_refuses_z_loss(dev, monkeypatch):
    """the fp8 loss head (the configuration of test_fp8_head_engine_step): label smoothing runs -- the e5m2 gradient copy against
    fp64 on the engine's own logits -- and z_loss > 0 raises at construction"""
    import drakegpt_amd as D
    from drakegpt_amd import ops
    from drakegpt_amd.engine import TrainEngine
    V_, C, T, NH, L, B, eps = 50257, 1024, 1024, 16, 1, 1, 0.125
    seen = {}
    real = ops.cross_entropy_fp8

    def spy(logits, targets, Vv, dlogits, grad_scale, q8, **kw):
        seen["logits"], seen["kw"] = logits.clone(), kw
        rows = real(logits, targets, Vv, dlogits, grad_scale, q8, **kw)
        seen["rows"], seen["q8"] = rows.clone(), q8.clone()
        return rows
    monkeypatch.setattr(ops, "cross_entropy_fp8", spy)
    torch.manual_seed(42)
    m = D.TransformerLM(V_, C, T, NH, L, 0.0, precision="fp8").to(dev).train()
    with pytest.raises(ValueError, match="z_loss"):
        TrainEngine(m, B, T, lr=1e-4, seed=3, use_graph=False, label_smoothing=eps, z_loss=1e-2)
    eng = TrainEngine(m, B, T, lr=1e-4, seed=3, use_graph=False, label_smoothing=eps)
    assert eng.fp8_head and eng.bf16_logits
    g = torch.Generator().manual_seed(8)
    x, y = torch.randint(0, V_, (B, T), generator=g), torch.randint(0, V_, (B, T), generator=g)
    eng.set_batch(x.to(dev), y.to(dev))
    loss = eng.step().item()
    torch.cuda.synchronize()
    eng.check_status()
    M, R = B * T, 64                                                     # (fp64 on the first 64 rows: 26 MB instead of 412)
    assert seen["kw"] == {"label_smoothing": eps}
    ref_rows, ref = LM.objective_fp64(seen["logits"][:R], y.reshape(-1)[:R], eps, 0.0, grad_scale=1.0 / M)
    assert rel(seen["rows"][:R], ref_rows) < 1e-6
    assert abs(loss - seen["rows"].double().mean().item()) < 1e-5 * loss
    deq = seen["q8"][:R].float().cpu().double() * (1.0 / M / 57344.0)
    assert torch.all(deq[:, V_:] == 0) and rel(deq[:, :V_], ref) < 4e-2, rel(deq[:, :V_], ref)


# ------------------------------------------------------------------------------------------------ resume
def test_resume_with_options_bit_for_bit(dev, tmp_path):
    """3 + 3 steps equal 6 steps bit for bit with the options on; a state saved with options is refused by a default engine and
    the reverse; a state without the fields loads into a default engine"""
    from drakegpt_amd import checkpoint as CK
    opts = dict(label_smoothing=0.125, z_loss=1e-2)
    corpus = torch.randint(0, SV, (20_000,), generator=torch.Generator().manual_seed(1)).to(dev)
    rows = torch.randint(0, 20_000 - ST - 1, (6, SB), generator=torch.Generator().manual_seed(2))
    _, A = _scaled(dev, **opts)
    A.set_corpus(corpus)
    A.stage_offsets(rows)
    for _ in range(3):
        A.step()
    path = str(tmp_path / "opts.state.pt")
    CK.save_train_state(path, A.state_dict())
    sd = CK.load_train_state(path)
    assert sd["meta"]["label_smoothing"] == 0.125 and sd["meta"]["z_loss"] == 1e-2
    la = [A.step().item() for _ in range(3)]
    _, Bn = _scaled(dev, model_seed=7, seed=99, **opts)
    Bn.set_corpus(corpus)
    Bn.load_state_dict(sd)
    lb = [Bn.step().item() for _ in range(3)]
    torch.cuda.synchronize()
    assert la == lb, (la, lb)
    for k in ("flat", "m_", "v_", "shadow"):
        assert torch.equal(getattr(A, k), getattr(Bn, k)), k
    assert A.step_count() == Bn.step_count() == 6
    # refusals, both directions, leave the engine as it was
    _, Dn = _scaled(dev, model_seed=9, seed=6)
    Dn.set_corpus(corpus)
    before = Dn.flat.clone()
    with pytest.raises(ValueError, match=r"meta\.label_smoothing differs.*0\.125.*0\.0"):
        Dn.load_state_dict(sd)
    assert torch.equal(Dn.flat, before)
    _, Zn = _scaled(dev, model_seed=9, seed=6, z_loss=1e-2)
    Zn.set_corpus(corpus)
    with pytest.raises(ValueError, match=r"meta\.label_smoothing differs.*0\.125.*0\.0"):
        Zn.load_state_dict(sd)                                         # one field equal, the other not
    plain = Dn.state_dict()
    assert "label_smoothing" not in plain["meta"] and "z_loss" not in plain["meta"]          # the file a default engine always wrote
    before = Bn.flat.clone()
    with pytest.raises(ValueError, match=r"meta\.label_smoothing differs.*0\.0.*0\.125"):
        Bn.load_state_dict(plain)
    assert torch.equal(Bn.flat, before)
    Dn.load_state_dict(plain)


# ------------------------------------------------------------------------------------------------ harness
def test_train_harness_with_both_flags(dev, tmp_path, capsys):
    """4 iterations on each training path (engine, autograd) with both flags, in the style of test_train_harness_smoke; the
    evaluation lines are there and sane (about log V on the synthetic uniform corpus)"""
    import json
    import math
    from drakegpt_amd import train
    from drakegpt_amd.config import DRAKE_VOCAB_SIZE
    flags = ["--label-smoothing", "0.125", "--z-loss", "1e-2", "--iters", "4", "--eval-interval", "2", "--eval-iters", "2",
             "--precision", "fp32", "--no-save", "--sample", "3"]
    for model in ("TransformerLM", "BlocksLM"):
        train.main(["--model", model] + flags)
        out = capsys.readouterr().out
        lines = [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")]
        assert len(lines) == 2 and all(abs(ln["val_loss"] - math.log(DRAKE_VOCAB_SIZE)) < 0.5 for ln in lines), lines
