"""precision "bf16x3" on the GPU: fp32 operands contracted on the bf16 matrix cores as hi.hi + hi.lo + lo.hi of split
operands (hi = bf16(x), lo = bf16(x - hi)), against fp64 and against the CPU oracle.

Kernels: the wave-specialised NT GEMM's split form (K a multiple of 32, K >= 128), the generic split NT GEMM (every other
shape), the split TN GEMM (split-K dW slabs).  Each GEMM is checked twice: against fp64 (relative L2 <= 1e-5), and against the
same product of bf16-ROUNDED operands (at least 20x smaller error), which shows the lo terms are really there.
"""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
V = 80


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _report(name, d):
    if os.environ.get("DG_TEST_REPORT"):
        print(f"[bf16x3] {name}: " + ", ".join(f"{k}={v:.3e}" for k, v in d.items()), flush=True)


def _bf(t):
    return t.to(torch.bfloat16).double()


def _check(name, got, ref64, ref_bf):
    e, e_bf = rel(got, ref64), rel(ref_bf, ref64)
    _report(name, dict(split=e, bf16_operands=e_bf))
    # measured on MI355X: 4.2e-6 .. 4.7e-6 for every shape and epilogue below (bf16-rounded operands: 2.3e-3)
    assert e <= 1e-5, (name, e)
    assert 20 * e < e_bf, (name, e, e_bf)


# ---------------------------------------------------------------------------------------------------------- NT
NT_SHAPES = [
    (16384, 1152, 384),     # wave-specialised, 128 x 192 tiles
    (16384, 384, 1536),
    (16384, 80, 384),       # partial tile (lm_head width)
    (100, 96, 32),          # generic: K < 128
    (100, 96, 200),         # generic: K % 32 != 0
]


@pytest.mark.parametrize("M,N,K", NT_SHAPES)
def test_gemm_nt_split_plain(dev, M, N, K):
    from drakegpt_amd import ops
    g = torch.Generator(device=dev).manual_seed(M + N + K)
    A = torch.randn((M, K), device=dev, generator=g)
    B = torch.randn((N, K), device=dev, generator=g)
    got = ops.gemm_nt(A, B, torch.float32, split=True)
    torch.cuda.synchronize()
    _check(f"nt {M}x{N}x{K}", got, A.double() @ B.double().T, _bf(A) @ _bf(B).T)


@pytest.mark.parametrize("M,N,K", [(16384, 1536, 384), (100, 96, 200)])
def test_gemm_nt_split_bias_relu(dev, M, N, K):
    from drakegpt_amd import ops
    g = torch.Generator(device=dev).manual_seed(7)
    A = torch.randn((M, K), device=dev, generator=g)
    B = torch.randn((N, K), device=dev, generator=g)
    bias = torch.randn((N,), device=dev, generator=g)
    got = ops.gemm_nt(A, B, torch.float32, bias=bias, relu=True, split=True)
    torch.cuda.synchronize()
    ref = torch.relu(A.double() @ B.double().T + bias.double())
    _check(f"nt bias+relu {M}x{N}x{K}", got, ref, torch.relu(_bf(A) @ _bf(B).T + bias.double()))


@pytest.mark.parametrize("M,N,K", [(16384, 384, 1536), (100, 96, 200)])
def test_gemm_nt_split_fp32_relu_mask(dev, M, N, K):
    """dX of the second FFN Linear in the fp32 program: the mask is the fp32 hidden activation (read as fp32, not bf16)"""
    from drakegpt_amd import ops
    g = torch.Generator(device=dev).manual_seed(11)
    A = torch.randn((M, K), device=dev, generator=g)
    B = torch.randn((N, K), device=dev, generator=g)
    mask = torch.randn((M, N), device=dev, generator=g)      # read as bf16 it would be other elements' halves
    got = ops.gemm_nt(A, B, torch.float32, relu_mask=mask, split=True)
    torch.cuda.synchronize()
    keep = (mask > 0).double()
    assert keep.mean().item() > 0.3
    _check(f"nt relu_mask {M}x{N}x{K}", got, (A.double() @ B.double().T) * keep, (_bf(A) @ _bf(B).T) * keep)


@pytest.mark.parametrize("M,N,K,with_bias", [(16384, 384, 1536, True), (16384, 384, 384, False), (100, 96, 200, True)])
def test_gemm_nt_split_residual_dropout(dev, M, N, K, with_bias):
    from drakegpt_amd import ops
    from oracle import rng_ref
    g = torch.Generator(device=dev).manual_seed(13)
    A = torch.randn((M, K), device=dev, generator=g)
    B = torch.randn((N, K), device=dev, generator=g)
    bias = torch.randn((N,), device=dev, generator=g) if with_bias else None
    res = torch.randn((M, N), device=dev, generator=g)
    p, seed, site = 0.2, 1234, 5
    rs = ops.new_rng_state(seed, dev, 3)
    got = ops.gemm_nt(A, B, torch.float32, bias=bias, residual=res, dropout_p=p, rng_state=rs, site=site, split=True)
    torch.cuda.synchronize()
    keep = torch.from_numpy(rng_ref.keep_mask(seed, 3, site, p, M * N).reshape(M, N)).to(dev).double()
    scale = 1.0 / (1.0 - p)
    b64 = bias.double() if with_bias else 0.0

    def epi(acc):
        return (acc + b64) * keep * scale + res.double()
    # the residual dominates the output: compare the GEMM part (output - residual) so that the bound speaks of the contraction
    _check(f"nt residual+dropout {M}x{N}x{K} bias={with_bias}", got.double() - res.double(),
           epi(A.double() @ B.double().T) - res.double(), epi(_bf(A) @ _bf(B).T) - res.double())


# ---------------------------------------------------------------------------------------------------------- TN
@pytest.mark.parametrize("R,P,Q,n_splits", [(16384, 384, 1536, 1), (16384, 1152, 384, 8), (1000, 96, 200, 3), (256, 80, 384, 2)])
def test_gemm_tn_split_slabs(dev, R, P, Q, n_splits):
    from drakegpt_amd import ops
    g = torch.Generator(device=dev).manual_seed(R + P + Q)
    A = torch.randn((R, P), device=dev, generator=g)
    B = torch.randn((R, Q), device=dev, generator=g)
    part = torch.zeros((n_splits, P * Q), device=dev)
    ops.gemm_tn(A, B, part, P * Q, n_splits, P, Q, split=True)
    got = torch.empty((P, Q), device=dev)
    ops.reduce_partials(part, P * Q, n_splits, got, P * Q)
    torch.cuda.synchronize()
    _check(f"tn {R}x{P}x{Q} splits={n_splits}", got, A.double().T @ B.double(), _bf(A).T @ _bf(B))


def test_split_needs_fp32_operands(dev):
    from drakegpt_amd import ops
    a = torch.randn((128, 128), device=dev).to(torch.bfloat16)
    with pytest.raises(TypeError):
        ops.gemm_nt(a, a, torch.float32, split=True)
    f = torch.randn((128, 128), device=dev)
    with pytest.raises(TypeError):
        ops.gemm_nt(f, f, torch.bfloat16, split=True)
    part = torch.zeros((1, 128 * 128), device=dev)
    with pytest.raises(TypeError):
        ops.gemm_tn(a, a, part, 128 * 128, 1, 128, 128, split=True)


# ---------------------------------------------------------------------------------------------------------- engine
def _flat(grads, keys):
    return torch.cat([grads[k].reshape(-1).double().cpu() for k in keys])


def test_scaled_bf16x3_graph_step_with_dropout_matches_oracle(dev):
    """TransformerLM_scaled at B = 64, dropout 0.2, graph on (step 1 is a replay), against the fp32 reference arithmetic with
    the kernels' dropout masks (as test_gpu_engine_oracle.py does for bf16)."""
    import drakegpt_amd as D
    from drakegpt_amd.engine import TrainEngine
    from oracle import drake_ref as R
    from oracle import rng_ref
    cfg = R.SCALED
    B, T, C, NH, L, p = cfg["batch_size"], cfg["context_length"], cfg["embedding_dim"], cfg["num_heads"], cfg["num_layers"], cfg["dropout"]
    seed = 20240607
    torch.manual_seed(42)
    m = D.TransformerLM(V, C, T, NH, L, p, precision="bf16x3").to(dev).train()
    eng = TrainEngine(m, B, T, lr=cfg["base_lr"], betas=cfg["betas"], seed=seed, use_graph=True)
    eng.keep_logits = True
    # the fp32 program, with every GEMM split
    assert eng.split_bf16 and eng.act == torch.float32 and not eng.grouped_dw and not eng.chain_full
    g = torch.Generator().manual_seed(3)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    for step in range(2):
        x = torch.randint(0, V, (B, T), generator=g)
        y = torch.randint(0, V, (B, T), generator=g)
        sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
        eng.set_batch(x.to(dev), y.to(dev))
        loss = eng.step().item()
        torch.cuda.synchronize()
        logits = eng.last_logits.float().cpu()
        got = {k: v.detach().clone().cpu() for k, v in eng.named_grads().items()}
        masks = rng_ref.transformer_masks(seed, step, p, B, T, C, NH, L)
        keys = list(R.trainable_keys("TransformerLM", sd))
        lo, ls, gr = R.loss_and_grads("TransformerLM", sd, x, y, p=p, training=True, masks=masks)
        per = {k: rel(got[k], gr[k]) for k in keys}
        worst = max(per.items(), key=lambda kv: kv[1])
        e = dict(logits=rel(logits, lo), loss=abs(loss - ls.item()) / ls.item(), flat=rel(_flat(got, keys), _flat(gr, keys)),
                 worst_tensor=worst[1])
        _report(f"scaled engine step {step} (worst {worst[0]})", e)
        # measured on MI355X (step 0): logits 5.2e-6, loss 2.0e-7, flat gradient 2.8e-4
        assert e["logits"] <= 2e-5 and e["loss"] <= 1e-6 and e["flat"] <= 1e-3, e
        # Per tensor <= 1e-3, except the gradients that sit behind the first FFN Linear's ReLU: W1 (measured 1.17e-3 .. 1.38e-3)
        # and LayerNorm-2's weight (0.92e-3 .. 1.10e-3).  A forward difference of ~5e-6 flips the ReLU mask of the
        # pre-activations that close to zero, and each flip moves a whole term of a 16384-row sum.  The exact-fp32 mode on the
        # same step is already at 1.9e-4 .. 6.8e-4 on W1 against this fp32 CPU reference.  These two get 4e-3, about 3x measured.
        for k, v in per.items():
            assert v <= (4e-3 if k.endswith("ffwd.net.0.weight") or k.endswith("ln2.weight") else 1e-3), (k, v)
        del masks, lo, gr


@pytest.mark.parametrize("graph", [False, True])
def test_tiny_bf16x3_engine_steps_match_oracle(dev, golden_dir, graph):
    """tiny config (C = 32: every GEMM takes the generic split form), dropout 0.1, 3 steps including AdamW"""
    import drakegpt_amd as D
    from drakegpt_amd.engine import TrainEngine
    from oracle import drake_ref as R
    from oracle import rng_ref
    fix = torch.load(os.path.join(golden_dir, "traj5_TransformerLM.pt"), weights_only=True)
    p, seed, B, T = 0.1, 77, 32, 8
    m = D.TransformerLM(V, 32, 8, 4, 3, p, precision="bf16x3")
    m.load_state_dict(fix["init"])
    m = m.to(dev).train()
    eng = TrainEngine(m, B, T, lr=1e-3, betas=(0.9, 0.95), seed=seed, use_graph=graph)
    eng.keep_logits = True
    assert eng.split_bf16
    sd = {k: v.clone() for k, v in fix["init"].items()}
    opt = R.AdamWState(R.trainable_keys("TransformerLM", sd), 1e-3, (0.9, 0.95))
    for step in range(3):
        x, y = fix["x"][step], fix["y"][step]
        eng.set_batch(x.to(dev), y.to(dev))
        loss = eng.step().item()
        got = {k: v.detach().clone().cpu() for k, v in eng.named_grads().items()}
        masks = rng_ref.transformer_masks(seed, step, p, B, T, 32, 4, 3)
        lo, ls, gr = R.loss_and_grads("TransformerLM", sd, x, y, p=p, training=True, masks=masks)
        keys = list(gr)
        per = {k: rel(got[k], gr[k]) for k in keys}
        e = dict(logits=rel(eng.last_logits, lo), loss=abs(loss - ls.item()) / ls.item(), flat=rel(_flat(got, keys), _flat(gr, keys)),
                 worst_tensor=max(per.values()))
        opt.step(sd, gr)
        cur = m.state_dict()
        e["max_dW"] = max((cur[k].cpu() - sd[k]).abs().max().item() for k in gr)
        _report(f"tiny engine graph={graph} step {step}", e)
        # measured on MI355X (3 steps, both graph modes): logits <= 5.6e-6, loss <= 1.0e-7, flat <= 6.2e-6, worst tensor <= 1.5e-5,
        # largest weight difference after AdamW 3.0e-5 (the fp32 mode: < 2e-5)
        assert e["logits"] <= 2e-5 and e["loss"] <= 5e-7 and e["flat"] <= 2e-5, e
        assert e["worst_tensor"] <= 5e-5, sorted(per.items(), key=lambda kv: -kv[1])[:6]
        assert e["max_dW"] <= 1e-4, e


# ---------------------------------------------------------------------------------------------------------- module path
KW = {
    "BigramLM": dict(vocab_size=V),
    "SingleHeadAttentionLM": dict(vocab_size=V, embedding_dim=32, context_length=8, head_size=32),
    "MultiHeadAttentionLM": dict(vocab_size=V, embedding_dim=32, context_length=8, head_size=32, num_heads=4),
    "BlocksLM": dict(vocab_size=V, embedding_dim=32, context_length=8, num_heads=4, num_layers=3),
    "ResidualBlocksLM": dict(vocab_size=V, embedding_dim=32, context_length=8, num_heads=4, num_layers=3),
    "TransformerLM": dict(vocab_size=V, embedding_dim=32, context_length=8, num_heads=4, num_layers=3, dropout=0.1),
}


def _build(name, dev, golden_dir):
    import drakegpt_amd as D
    m = D.MODEL_CLASSES[name](**KW[name], precision="bf16x3")
    m.load_state_dict(torch.load(os.path.join(golden_dir, "checkpoints", f"{name}.pt"), weights_only=True))
    return m.to(dev)


@pytest.mark.parametrize("name", list(KW))
def test_checkpoint_forward_backward_bf16x3(dev, golden_dir, name):
    fix = torch.load(os.path.join(golden_dir, f"fwdbwd_{name}.pt"), weights_only=True)
    m = _build(name, dev, golden_dir).eval()
    logits, loss = m(fix["x"].to(dev), fix["y"].to(dev))
    loss.backward()
    e = dict(logits=rel(logits, fix["logits"]), loss=abs(loss.item() - fix["loss"].item()) / abs(fix["loss"].item()))
    grads = {k: rel(p.grad, fix["grad." + k]) for k, p in m.named_parameters() if not k.startswith("ln_f.")}
    e["worst_grad"] = max(grads.values())
    _report(f"module {name}", e)
    # measured on MI355X over the six models: logits <= 6.3e-6, loss <= 2.1e-6, worst gradient <= 8.3e-5
    assert e["logits"] <= 2e-5 and e["loss"] <= 6e-6, e
    assert e["worst_grad"] <= 2.5e-4, grads


@pytest.mark.parametrize("name", list(KW))
def test_generate_tokens_bf16x3(dev, golden_dir, name):
    gold = json.load(open(os.path.join(golden_dir, "generate.json")))
    m = _build(name, dev, golden_dir).eval()
    torch.manual_seed(gold["seed"])
    out = m.generate(torch.zeros((1, 1), dtype=torch.long, device=dev), max_new_tokens=gold["max_new_tokens"])
    assert out[0].tolist() == gold["tokens"][name]


def test_kv_cached_logits_equal_uncached_bf16x3(dev):
    import drakegpt_amd as D
    torch.manual_seed(0)
    m = D.TransformerLM(V, 64, 24, 4, 2, 0.1, precision="bf16x3").to(dev).eval()
    start = torch.zeros((2, 3), dtype=torch.long, device=dev)
    torch.manual_seed(11)
    a = m.generate(start, 20, use_cache=True)
    ws, w_lm = m._decode_weights()
    caches = [torch.zeros((2, 24, 3 * 64), device=dev) for _ in m.blocks]
    seq = a[:, :10].contiguous()
    for t in range(10):
        lg = m._decode_step(seq[:, t:t + 1].contiguous(), t, caches, ws, w_lm)
    full, _ = m(seq)
    e = rel(lg, full[:, -1, :])
    _report("cached vs uncached logits", dict(rel=e))
    assert e <= 1e-5          # measured on MI355X: 0 (bit-identical)
