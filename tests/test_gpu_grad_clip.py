"""Global-norm gradient clipping (ref: torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm) before optimizer.step()):
the sum-of-squares / finalize kernels against fp64, the engine and the autograd-path AdamW against the oracle with torch's clip
formula applied in fp64, the bucketed and unbucketed data-parallel steps, and the harness flag.

Adam's first update is about lr * sign(g) whatever the scale of g, so a wrong coefficient can leave the weights nearly right: every
comparison here also checks the moments (m_1 = (1 - b1) coef g is linear in the coefficient) and the reported norm."""
import json
import math
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
V = 80


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _norm64(tensors):
    return math.sqrt(sum(float(t.double().square().sum()) for t in tensors))


def _coef64(norm, max_norm):
    return min(1.0, max_norm / (norm + 1e-6))


def _moment_views(eng, buf):
    """buf (eng.m_ / eng.v_) cut like eng.named_grads(): same layout as the flat gradient"""
    return {k: buf.as_strided(g.size(), g.stride(), g.storage_offset()) for k, g in eng.named_grads().items()}


# ------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("n", [1, 5, 1024, 262_147, 10_800_003, 100_000_000])
@pytest.mark.parametrize("kind", ["normal", "wide"])
def test_grad_norm_kernel_against_fp64(dev, n, kind):
    from drakegpt_amd import ops
    gen = torch.Generator(device=dev).manual_seed(n % 1000 + 7)
    g = torch.randn(n, device=dev, generator=gen)
    if kind == "wide":                      # magnitudes spread over 1e-6 .. 1e3, random signs
        mag = torch.pow(10.0, torch.rand(n, device=dev, generator=gen) * 9.0 - 6.0)
        g = torch.where(g < 0, -mag, mag)
    ref = g.double().square().sum().sqrt().item()
    work = ops.grad_norm_workspace([g], dev)
    for scale in (1.0, 0.5):
        norm = ref * scale
        for max_norm in (0.5 * norm, 4.0 * norm):
            mn = torch.tensor([max_norm], dtype=torch.float32, device=dev)
            out = torch.zeros(2, dtype=torch.float32, device=dev)
            ops.grad_norm(g, scale, mn, out, work)
            a = out.cpu().clone()
            ops.grad_norm(g, scale, mn, out, work)
            assert torch.equal(out.cpu(), a)                                        # bitwise reproducible
            assert abs(a[0].item() - norm) <= 1e-6 * norm, (n, kind, scale, a[0].item(), norm)
            want = _coef64(norm, float(mn.item()))
            assert abs(a[1].item() - want) <= 1e-6 * want, (a[1].item(), want)
            assert (a[1].item() == 1.0) == (max_norm > norm)


def test_grad_norm_over_several_buffers_and_non_finite(dev):
    from drakegpt_amd import ops
    gen = torch.Generator(device=dev).manual_seed(11)
    parts = [torch.randn(n, device=dev, generator=gen) for n in (3, 70_001, 1_000_000)]
    mn = torch.tensor([1.0], dtype=torch.float32, device=dev)
    out = torch.zeros(2, dtype=torch.float32, device=dev)
    ops.grad_norm(parts, 1.0, mn, out)
    ref = _norm64(parts)
    assert abs(out[0].item() - ref) <= 1e-6 * ref
    # torch's formula in fp32: an inf norm gives coef 0, a NaN norm a NaN coef (clamp keeps NaN)
    parts[1][5] = float("inf")
    ops.grad_norm(parts, 1.0, mn, out)
    assert out[0].item() == float("inf") and out[1].item() == 0.0
    parts[1][5] = float("nan")
    ops.grad_norm(parts, 1.0, mn, out)
    assert math.isnan(out[0].item()) and math.isnan(out[1].item())


def test_adamw_step_with_unit_coefficient_is_bit_identical(dev):
    from drakegpt_amd import ops
    n = 100_003
    res = []
    for clip in (None, torch.ones(1, dtype=torch.float32, device=dev)):
        p = torch.randn(n, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        hyper = torch.tensor([1e-3, 0.9, 0.95, 1e-8, 1e-2], dtype=torch.float32, device=dev)
        st = ops.new_rng_state(0, dev, 0)
        for it in range(3):
            g = torch.randn(n, device=dev, generator=torch.Generator(device=dev).manual_seed(10 + it))
            ops.adamw_step(p, g, m, v, hyper, st, 0.5, advance=True, clip=clip)
        res.append((p.cpu(), m.cpu(), v.cpu()))
    assert all(torch.equal(a, b) for a, b in zip(*res))


# ------------------------------------------------------------------------------------------------ engine
@pytest.mark.parametrize("graph", [False, True])
def test_tiny_fp32_engine_clipped_steps_match_oracle(dev, golden_dir, graph):
    """fp32, tiny config, dropout 0.1, 3 steps: max_norm = half of the first step's unclipped norm, so every step clips"""
    import drakegpt_amd as D
    from drakegpt_amd.engine import TrainEngine
    from oracle import drake_ref as R
    from oracle import rng_ref
    fix = torch.load(os.path.join(golden_dir, "traj5_TransformerLM.pt"), weights_only=True)
    p, seed, B, T, b1, b2 = 0.1, 77, 32, 8, 0.9, 0.95
    sd = {k: v.clone() for k, v in fix["init"].items()}
    _, _, gr0 = R.loss_and_grads("TransformerLM", sd, fix["x"][0], fix["y"][0], p=p, training=True,
                                 masks=rng_ref.transformer_masks(seed, 0, p, B, T, 32, 4, 3))
    max_norm = 0.5 * _norm64(gr0.values())
    m = D.TransformerLM(V, 32, 8, 4, 3, p)
    m.load_state_dict(fix["init"])
    m = m.to(dev).train()
    eng = TrainEngine(m, B, T, lr=1e-3, betas=(b1, b2), seed=seed, use_graph=graph, max_grad_norm=max_norm)
    opt = R.AdamWState(R.trainable_keys("TransformerLM", sd), 1e-3, (b1, b2))
    for step in range(3):
        x, y = fix["x"][step], fix["y"][step]
        eng.set_batch(x.to(dev), y.to(dev))
        eng.step()
        masks = rng_ref.transformer_masks(seed, step, p, B, T, 32, 4, 3)
        _, _, gr = R.loss_and_grads("TransformerLM", sd, x, y, p=p, training=True, masks=masks)
        norm = _norm64(gr.values())
        coef = _coef64(norm, max_norm)
        assert coef < 1.0, (step, norm, max_norm)
        assert abs(eng.last_grad_norm.item() - norm) <= 1e-4 * norm, (step, eng.last_grad_norm.item(), norm)
        # the stored gradient stays unclipped
        got = eng.named_grads()
        assert rel(torch.cat([got[k].reshape(-1) for k in gr]), torch.cat([gr[k].reshape(-1) for k in gr])) < 1e-4
        opt.step(sd, {k: (g.double() * coef).float() for k, g in gr.items()})
        mv, vv = _moment_views(eng, eng.m_), _moment_views(eng, eng.v_)
        for k in gr:
            assert rel(mv[k], opt.m[k]) < 3e-4, (step, k, rel(mv[k], opt.m[k]))
            assert rel(vv[k], opt.v[k]) < 3e-4, (step, k, rel(vv[k], opt.v[k]))
        cur = m.state_dict()
        for k in gr:
            assert (cur[k].cpu() - sd[k]).abs().max().item() < 2e-5, (step, k)
    eng.set_max_grad_norm(1e30)                  # no recapture: the next replay reads the new threshold
    eng.set_batch(fix["x"][3].to(dev), fix["y"][3].to(dev))
    eng.step()
    assert eng.clip_state[1].item() == 1.0


def _scaled_engine(dev, precision, B, max_grad_norm, seed=20240607):
    import drakegpt_amd as D
    from drakegpt_amd.engine import TrainEngine
    from oracle import drake_ref as R
    cfg = R.SCALED
    torch.manual_seed(42)
    m = D.TransformerLM(V, cfg["embedding_dim"], cfg["context_length"], cfg["num_heads"], cfg["num_layers"], cfg["dropout"],
                        precision=precision).to(dev).train()
    eng = TrainEngine(m, B, cfg["context_length"], lr=cfg["base_lr"], betas=cfg["betas"], seed=seed, use_graph=True,
                      max_grad_norm=max_grad_norm)
    return m, eng, cfg


def _batches(B, T, n, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randint(0, V, (B, T), generator=g), torch.randint(0, V, (B, T), generator=g)) for _ in range(n)]


def test_scaled_bf16_clipped_steps_report_the_norm_and_scale_the_moments(dev):
    """the benchmark configuration (B 64, dropout 0.2, graph on: steps 1 and 2 are replays)"""
    _, eng, cfg = _scaled_engine(dev, "bf16", 64, 1e-3)
    for step, (x, y) in enumerate(_batches(64, cfg["context_length"], 3)):
        eng.set_batch(x.to(dev), y.to(dev))
        eng.step()
        torch.cuda.synchronize()
        norm = _norm64(eng.named_grads().values())
        got_norm, coef = eng.clip_state[0].item(), eng.clip_state[1].item()
        assert abs(got_norm - norm) <= 1e-6 * norm, (step, got_norm, norm)
        assert abs(coef - _coef64(norm, 1e-3)) <= 1e-6 * coef and coef < 1.0
        if step == 0:
            # the kernel's own fp32 terms: gj = g * coef, m = gj * (1 - b1), v = ((1 - b2) * gj) * gj, with b1, b2 as fp32
            gj = eng.gflat * eng.clip_state[1]
            m1 = gj * (1.0 - eng.hyper[1])
            v1 = ((1.0 - eng.hyper[2]) * gj) * gj
            torch.testing.assert_close(eng.m_, m1, rtol=2e-7, atol=1e-30)
            torch.testing.assert_close(eng.v_, v1, rtol=4e-7, atol=1e-36)
            assert eng.m_.abs().max().item() > 0


def test_scaled_bf16_huge_threshold_is_bit_identical_to_no_clipping(dev):
    res = []
    for mg in (None, 1e30):
        m, eng, cfg = _scaled_engine(dev, "bf16", 64, mg)
        for x, y in _batches(64, cfg["context_length"], 3):
            eng.set_batch(x.to(dev), y.to(dev))
            eng.step()
        torch.cuda.synchronize()
        res.append((eng.flat.cpu(), eng.m_.cpu(), eng.v_.cpu()))
        if mg is not None:
            assert eng.clip_state[1].item() == 1.0 and eng.last_grad_norm.item() > 0
        else:
            assert eng.last_grad_norm is None
        del m, eng
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("precision,B", [("fp8", 8), ("bf16x3", 64)])
def test_scaled_clipped_norm_in_other_precisions(dev, precision, B):
    """the norm covers every region of the flat gradient and nothing else: its alignment gaps stay zero in every precision"""
    _, eng, cfg = _scaled_engine(dev, precision, B, 1e-3, seed=777)
    for step, (x, y) in enumerate(_batches(B, cfg["context_length"], 3, seed=1)):
        eng.set_batch(x.to(dev), y.to(dev))
        eng.step()
        torch.cuda.synchronize()
        grads = eng.named_grads()
        norm = _norm64(grads.values())
        assert abs(eng.last_grad_norm.item() - norm) <= 1e-6 * norm, (precision, step, eng.last_grad_norm.item(), norm)
        covered = torch.zeros(eng.n_active, dtype=torch.bool, device=dev)
        for g in grads.values():
            covered.as_strided(g.size(), g.stride(), g.storage_offset()).fill_(True)
        assert not eng.gflat[~covered].any().item()


def test_engine_rejects_bad_thresholds(dev, golden_dir):
    import drakegpt_amd as D
    from drakegpt_amd.engine import TrainEngine
    m = D.TransformerLM(V, 32, 8, 4, 3, 0.0).to(dev)
    for bad in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            TrainEngine(m, 32, 8, max_grad_norm=bad)
    eng = TrainEngine(m, 32, 8)
    with pytest.raises(RuntimeError):
        eng.set_max_grad_norm(1.0)


# ------------------------------------------------------------------------------------------------ data parallel
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_dp(rank, world, port, golden_dir, ret, precision, buckets, key, max_norm):
    import torch.distributed as dist
    import drakegpt_amd as D
    from drakegpt_amd import dist as ddist
    from drakegpt_amd.engine import TrainEngine
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    dev = torch.device("cuda:0")
    pg = None
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        pg = dist.group.WORLD
    try:
        fix = torch.load(os.path.join(golden_dir, "traj5_TransformerLM.pt"), weights_only=True)
        m = D.TransformerLM(V, 32, 8, 4, 3, 0.0, precision=precision)
        m.load_state_dict(fix["init"])
        m = m.to(dev)
        eng = TrainEngine(m, 32 // world, 8, lr=1e-3, betas=(0.9, 0.95), rank=rank, world_size=world, process_group=pg,
                          dp_buckets=buckets, max_grad_norm=max_norm)
        if buckets and world > 1:
            assert eng.dp_buckets == buckets
        losses, norms, coefs = [], [], []
        for it in range(3):
            x = ddist.shard_rows(fix["x"][it], rank, world)
            y = ddist.shard_rows(fix["y"][it], rank, world)
            eng.set_batch(x.to(dev), y.to(dev))
            losses.append(ddist.mean_loss(eng.step().clone(), pg).item())
            norms.append(eng.last_grad_norm.item())
            coefs.append(eng.clip_state[1].item())
        eng.check_status()
        ret[(key, rank)] = (losses, norms, coefs, {k: v.detach().cpu().clone() for k, v in m.state_dict().items()},
                            eng.m_.cpu().clone())
    finally:
        if world > 1:
            dist.destroy_process_group()


def _spawn(golden_dir, runs, max_norm):
    mgr = mp.Manager()
    ret = mgr.dict()
    ctx = mp.get_context("spawn")
    for key, world, precision, buckets in runs:
        port = _free_port()
        procs = [ctx.Process(target=_run_dp, args=(r, world, port, golden_dir, ret, precision, buckets, key, max_norm))
                 for r in range(world)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(300)
            assert p.exitcode == 0
    return dict(ret)


def _half_first_norm(golden_dir):
    from oracle import drake_ref as R
    fix = torch.load(os.path.join(golden_dir, "traj5_TransformerLM.pt"), weights_only=True)
    _, _, gr = R.loss_and_grads("TransformerLM", {k: v.clone() for k, v in fix["init"].items()}, fix["x"][0], fix["y"][0])
    return 0.5 * _norm64(gr.values())


def test_two_rank_clipped_engine_equals_single_process(dev, golden_dir):
    mn = _half_first_norm(golden_dir)
    ret = _spawn(golden_dir, [("one", 1, "fp32", None), ("two", 2, "fp32", None)], mn)
    l1, n1, c1, sd1, _ = ret[("one", 0)]
    l2, n2, c2, sd2, _ = ret[("two", 0)]
    assert ret[("two", 1)][1] == n2 and ret[("two", 1)][2] == c2          # every rank applies the same norm
    assert all(c < 1.0 for c in c1)
    for a, b in zip(n1, n2):
        assert abs(a - b) <= 1e-5 * a, (n1, n2)
    for a, b in zip(l1, l2):
        assert abs(a - b) < 2e-5 * abs(a), (l1, l2)
    for k in sd1:
        assert (sd1[k] - sd2[k]).abs().max().item() < 2e-6, k


def test_two_rank_clipped_bucketed_equals_single_exchange(dev, golden_dir):
    mn = _half_first_norm(golden_dir)
    ret = _spawn(golden_dir, [("flat", 2, "bf16", 1), ("bucketed", 2, "bf16", 3)], mn)
    l2, n2, c2, sd2, m2 = ret[("flat", 0)]
    l3, n3, c3, sd3, m3 = ret[("bucketed", 0)]
    assert ret[("bucketed", 1)][1] == n3 and ret[("flat", 1)][1] == n2
    assert all(c < 1.0 for c in c2 + c3)
    for a, b in zip(n2, n3):
        assert abs(a - b) <= 2e-5 * a, (n2, n3)
    for a, b in zip(l2, l3):
        assert abs(a - b) < 2e-5 * abs(b), (l2, l3)
    for k in sd2:
        assert (sd2[k] - sd3[k]).abs().max().item() < 2e-5, k
    assert rel(m3, m2) < 1e-4


# ------------------------------------------------------------------------------------------------ autograd path
@pytest.mark.parametrize("name", ["BigramLM", "TransformerLM"])
def test_module_path_clipped_adamw_matches_oracle(dev, golden_dir, name):
    import drakegpt_amd as D
    from drakegpt_amd.optim import AdamW
    from oracle import drake_ref as R
    fix = torch.load(os.path.join(golden_dir, f"traj5_{name}.pt"), weights_only=True)
    sd = {k: v.clone() for k, v in fix["init"].items()}
    _, _, gr0 = R.loss_and_grads(name, sd, fix["x"][0], fix["y"][0])
    max_norm = 0.5 * _norm64(gr0.values())
    m = D.BigramLM(V) if name == "BigramLM" else D.TransformerLM(V, 32, 8, 4, 3, 0.0)
    m.load_state_dict(fix["init"])
    m = m.to(dev).train()
    opt = AdamW(m.parameters(), lr=1e-3, betas=(0.9, 0.95), max_grad_norm=max_norm)
    ref = R.AdamWState(R.trainable_keys(name, sd), 1e-3, (0.9, 0.95))
    names = [k for k, _ in m.named_parameters()]
    for it in range(5):
        x, y = fix["x"][it], fix["y"][it]
        _, loss = m(x.to(dev), y.to(dev))
        opt.zero_grad()
        loss.backward()
        unclipped = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
        opt.step()
        _, _, gr = R.loss_and_grads(name, sd, x, y)
        norm = _norm64(gr.values())
        coef = _coef64(norm, max_norm)
        assert coef < 1.0
        assert abs(opt.last_grad_norm.item() - norm) <= 1e-4 * norm, (it, opt.last_grad_norm.item(), norm)
        for k, g in unclipped.items():                                     # p.grad is left unclipped
            assert torch.equal(dict(m.named_parameters())[k].grad, g)
        ref.step(sd, {k: (g.double() * coef).float() for k, g in gr.items()})
        st = opt.state_dict()["state"]
        for i, k in enumerate(names):
            if k not in gr:
                continue
            assert rel(st[i]["exp_avg"], ref.m[k]) < 3e-4, (it, k)
            assert rel(st[i]["exp_avg_sq"], ref.v[k]) < 3e-4, (it, k)
        cur = m.state_dict()
        for k in gr:
            assert (cur[k].cpu() - sd[k]).abs().max().item() < 2e-5, (it, k)


def test_module_path_two_groups_share_one_norm(dev, golden_dir):
    import drakegpt_amd as D
    from drakegpt_amd.optim import AdamW
    from oracle import drake_ref as R
    fix = torch.load(os.path.join(golden_dir, "traj5_TransformerLM.pt"), weights_only=True)
    sd = {k: v.clone() for k, v in fix["init"].items()}
    _, _, gr0 = R.loss_and_grads("TransformerLM", sd, fix["x"][0], fix["y"][0])
    max_norm = 0.5 * _norm64(gr0.values())
    m = D.TransformerLM(V, 32, 8, 4, 3, 0.0)
    m.load_state_dict(fix["init"])
    m = m.to(dev).train()
    emb = [k for k, _ in m.named_parameters() if "embedding" in k or k.startswith("lm_head")]
    rest = [k for k, _ in m.named_parameters() if k not in emb]
    P = dict(m.named_parameters())
    opt = AdamW([{"params": [P[k] for k in emb], "lr": 2e-3}, {"params": [P[k] for k in rest]}], lr=1e-3, betas=(0.9, 0.95),
                max_grad_norm=max_norm)
    keys = R.trainable_keys("TransformerLM", sd)
    ref_a = R.AdamWState([k for k in keys if k in emb], 2e-3, (0.9, 0.95))
    ref_b = R.AdamWState([k for k in keys if k in rest], 1e-3, (0.9, 0.95))
    order = emb + rest
    for it in range(3):
        x, y = fix["x"][it], fix["y"][it]
        _, loss = m(x.to(dev), y.to(dev))
        opt.zero_grad()
        loss.backward()
        opt.step()
        _, _, gr = R.loss_and_grads("TransformerLM", sd, x, y)
        norm = _norm64(gr.values())
        coef = _coef64(norm, max_norm)
        assert coef < 1.0 and abs(opt.last_grad_norm.item() - norm) <= 1e-4 * norm
        clipped = {k: (g.double() * coef).float() for k, g in gr.items()}
        ref_a.step(sd, {k: g for k, g in clipped.items() if k in emb})
        ref_b.step(sd, {k: g for k, g in clipped.items() if k in rest})
        st = opt.state_dict()["state"]
        for i, k in enumerate(order):
            if k not in gr:
                continue
            r = ref_a if k in emb else ref_b
            assert rel(st[i]["exp_avg"], r.m[k]) < 3e-4, (it, k)
            assert rel(st[i]["exp_avg_sq"], r.v[k]) < 3e-4, (it, k)
        cur = m.state_dict()
        for k in gr:
            assert (cur[k].cpu() - sd[k]).abs().max().item() < 2e-5, (it, k)


# ------------------------------------------------------------------------------------------------ harness
def _eval_lines(out):
    return [json.loads(s) for s in out.splitlines() if s.startswith("{") and '"val_loss"' in s]


@pytest.mark.parametrize("model", ["TransformerLM", "BlocksLM"])
def test_train_harness_reports_grad_norm(dev, capsys, model):
    from drakegpt_amd import train
    base = ["--model", model, "--iters", "4", "--eval-interval", "2", "--eval-iters", "2", "--precision", "fp32", "--no-save",
            "--sample", "3"]
    train.main(base + ["--grad-clip", "1.0"])
    lines = _eval_lines(capsys.readouterr().out)
    assert len(lines) == 2
    for ln in lines:
        assert math.isfinite(ln["grad_norm"]) and ln["grad_norm"] > 0
    train.main(base)
    lines = _eval_lines(capsys.readouterr().out)
    assert len(lines) == 2 and all("grad_norm" not in ln for ln in lines)
