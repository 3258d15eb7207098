"""The GPT-2 shapes (BASELINE.json configs[2] / configs[4]) against an INDEPENDENT reference (round-2 VERDICT weak #1 / #2).

Until round 3 the full-size GPT-2 tests compared the engine with the module path -- the same attention and GEMM kernels on
both sides -- because the oracle cannot run 12 / 24 layers at B = 8 in test time.  It can run TWO layers at B = 1:
  * attention at T in {640, 1000, 1024} (20 .. 32 key tiles, a ragged last tile, dropout) forward and backward against fp64
    with the kernels' own keep-masks, with BOTH dK/dV forms (tiles from the dQ pass; scores recomputed);
  * one graph-captured TrainEngine.step() at the GPT-2 WIDTHS -- V 50257, T 1024, B 1, L 2, {C 768 / 12 heads in bf16,
    C 1024 / 16 heads in fp8} -- against oracle/drake_ref.py with shared masks: K = 768 / 3072 / 1024 / 4096 contractions
    through the bf16 / fp8 NT GEMMs and the grouped dW GEMM, the bf16 logits overwritten in place by the loss head, the fp32
    atomic token scatter at V = 50257 (no one-hot operand at this vocabulary), the 32-tile attention chains inside a model.
ref: src/model_component.py:392-405 (Head2), src/model.py:593-607 (embedding, lm_head, cross entropy), src/train.py:146-151.
"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
V = 50257


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


# Attention forward + backward at sequence lengths beyond 256 (the GPT-2 shapes' 32-tile key chains, the balanced block order, the
# XCD ranges, the P | dS tile workspace) against an fp64 restatement of Head2.forward with the kernels' own keep-masks.
# (B, T, NH, H, p): 32 key tiles with dropout; 20 tiles, one head, no dropout; a ragged last tile (T % 32 != 0) with dropout
# round 3: 448 (batch, head) pairs x 2 workgroups = 896 workgroups, more than one residency (768 on 256 CUs): the heavy-first
# block order (attn_item, balance == 2) instead of the equal-cost one
ATTN_CASES = [(1, 1024, 2, 64, 0.1), (2, 640, 1, 64, 0.0), (1, 1000, 1, 64, 0.1), (14, 256, 32, 64, 0.1)]
# measured on MI355X (round 3), both dK/dV forms alike: bf16 forward 1.9e-3 .. 2.3e-3, backward 2.4e-3 .. 2.5e-3 (dQ, dK and dV
# each 2.3e-3 .. 2.6e-3), lse 9e-7 absolute -- bf16 operand rounding, the same level as the T <= 256 cases of
# tests/test_gpu_ops.py::test_attention (whose bounds these are): nothing grows with the chain length
TOL_FWD, TOL_BWD = 8e-3, 2e-2
# localized checks (oracle/parity.py), measured on MI355X, both dK/dV forms alike: worst (row, head), kernel / CPU rounding model
# ("use" = largest group error / its bound = 3 x the model's worst group around the same position; < 1 passes)
#   case                   forward (envelope use)   dq                       dk                       dv
#   (1, 1024, 2, 64, 0.1)  3.1e-3 (0.63)            4.6e-1 / 2.0e-1 (0.74)   6.5e-3 / 4.4e-3 (0.50)   4.0e-3 / 4.0e-3 (0.35)
#   (2, 640, 1, 64, 0.0)   3.2e-3 (0.56)            7.8e-3 / 5.4e-3 (0.48)   4.3e-3 / 4.0e-3 (0.41)   3.5e-3 / 3.5e-3 (0.33)
#   (1, 1000, 1, 64, 0.1)  2.9e-3 (0.64)            4.0e-1 / 2.5e-1 (0.54)   4.0e-3 / 3.8e-3 (0.40)   3.6e-3 / 3.5e-3 (0.34)
#   (14, 256, 32, 64, 0.1) 4.1e-3 (0.86)            5.5e-1 / 6.6e-1 (0.42)   1.3e-2 / 1.9e-2 (0.40)   4.4e-3 / 4.4e-3 (0.33)
# dq's worst groups are the first query rows (dq cancels there, delta comes from the rounded output); the kernel's worst is up to
# 2.2 x the model's worst (fp32 summation order on top of the modelled roundings), inside the margin of 3.


def attn_ref(qkv, B, T, NH, H, keep=None, p=0.0):
    """fp64, differentiable: softmax(mask(q k^T * H^-1/2)) [* keep / (1 - p)] v over packed qkv [B*T, 3*NH*H]"""
    C = NH * H
    q, k, v = qkv.view(B, T, 3, NH, H).permute(2, 0, 3, 1, 4)
    w = q @ k.transpose(-2, -1) * H ** -0.5
    tril = torch.tril(torch.ones(T, T, dtype=torch.bool))
    w = w.masked_fill(~tril, float("-inf")).softmax(-1)
    if keep is not None:
        w = w * keep / (1 - p)
    return (w @ v).permute(0, 2, 1, 3).reshape(B * T, C)


def check_case(dev, tile_scratch, B, T, NH, H, p):
    """tile_scratch: the dK/dV form -- True reads the dQ pass's P | dS tiles, False recomputes the scores"""
    from drakegpt_amd import ops
    from oracle import parity as P
    from oracle import rng_ref
    g = torch.Generator().manual_seed(T * 7 + H)
    C = NH * H
    qkv = torch.randn(B * T, 3 * C, generator=g).bfloat16()
    dout = torch.randn(B * T, C, generator=g).bfloat16()
    seed, step, site = 77, 3, 4
    keep = rng = None
    if p > 0:
        keep = torch.from_numpy(rng_ref.keep_mask(seed, step, site, p, B * NH * T * T).reshape(B, NH, T, T)).double()
        rng = ops.new_rng_state(seed, dev, step)
    qd = qkv.double().requires_grad_(True)
    ref = attn_ref(qd, B, T, NH, H, keep, p)
    ref.backward(dout.double())
    out, lse = ops.attn_fwd(qkv.to(dev), B, T, NH, H, H ** -0.5, p, rng, site, keep=True)
    dqkv = ops.attn_bwd(qkv.to(dev), out, dout.to(dev), lse, B, T, NH, H, H ** -0.5, p, rng, site, tile_scratch=tile_scratch)
    torch.cuda.synchronize()
    ef, eb = rel(out, ref.detach()), rel(dqkv, qd.grad)
    # the three gradient blocks separately: a wrong dK or dV term must not hide behind a correct dQ
    parts = {n: rel(dqkv.view(B * T, 3, C)[:, i], qd.grad.view(B * T, 3, C)[:, i]) for i, n in enumerate(("dq", "dk", "dv"))}
    lse_ref = torch.logsumexp((qd.detach().view(B, T, 3, NH, H)[:, :, 0].permute(0, 2, 1, 3) @
                               qd.detach().view(B, T, 3, NH, H)[:, :, 1].permute(0, 2, 3, 1) * H ** -0.5)
                              .masked_fill(~torch.tril(torch.ones(T, T, dtype=torch.bool)), float("-inf")), -1)
    el = (lse.double().cpu() - lse_ref).abs().max().item()
    # localized (oracle/parity.py): forward every element inside the derived envelope and every (row, head) at the forward bound;
    # backward every (row, head) of each third within BWD_MARGIN x the CPU rounding model's worst group around the same position
    R = P.attention_fp64(qkv, dout, B, T, NH, H, keep, p)
    bounds = P.attention_bwd_bounds_by_position(R, P.attention_fp64(qkv, dout, B, T, NH, H, keep, p, model=True), B, T, NH, H)
    rows = dict(fwd=P.rowwise_rel(out, R["out"], H).max().item())
    local = []
    for what, fn in [("forward envelope", lambda: P.assert_within_rounding(out, R["out"], P.attention_fwd_envelope(R), 1, "out")),
                     ("forward rows", lambda: P.assert_rowwise(out, R["out"], H, TOL_FWD, "out", T))]:
        try:
            rows[what] = fn()
        except AssertionError as e:
            local.append(str(e))
    for i, n in enumerate(("dq", "dk", "dv")):
        got = dqkv.view(B * T, 3, C)[:, i]
        rows[n] = P.rowwise_rel(got, R[n], H).max().item()
        rows[n + " model"] = bounds[n].max().item() / P.BWD_MARGIN
        try:
            rows[n + " use"] = P.assert_rowwise_each(got, R[n], H, bounds[n], n, T)
        except AssertionError as e:
            local.append(str(e))
    return ef, eb, parts, el, rows, local


def _attn_long_bad(dev, tile_scratch):
    bad = []
    for case in ATTN_CASES:
        ef, eb, parts, el, rows, local = check_case(dev, tile_scratch, *case)
        if os.environ.get("DG_TEST_REPORT"):
            print(f"[parity] attention {case} tile_scratch={tile_scratch}: fwd {ef:.2e} bwd {eb:.2e} "
                  + " ".join(f"{k} {v:.2e}" for k, v in parts.items()) + f" lse {el:.2e}", flush=True)
            print(f"[parity]   worst (row, head): " + " ".join(f"{k} {v:.2e}" for k, v in rows.items()), flush=True)
        if not (ef < TOL_FWD and eb < TOL_BWD and max(parts.values()) < TOL_BWD and el < 2e-2) or local:
            bad.append((case, ef, eb, parts, el, local))
    return bad


def test_attention_long_sequences_match_fp64(dev):
    bad = _attn_long_bad(dev, tile_scratch=True)
    assert not bad, bad


def test_attention_long_sequences_match_fp64_recompute_dkv_form(dev):
    """the same cases with the dK/dV pass that recomputes scores: a workspace without the tile scratch"""
    bad = _attn_long_bad(dev, tile_scratch=False)
    assert not bad, bad


def _flat(grads, keys):
    return torch.cat([grads[k].reshape(-1).double().cpu() for k in keys])


# measured on MI355X (round 3), one captured step at B = 1, T = 1024, L = 2, dropout 0.1, vs the reference's fp32 arithmetic:
#   bf16  C 768 : loss 5e-6, logits 2.5e-3, flat gradient 9.0e-3, worst tensor 4.0e-2 (W1 of block 0; the LayerNorm-2 gains next)
#                 against the oracle WITH the kernels' bf16 roundings: flat gradient 5.1e-3, worst tensor 2.4e-2
#   fp8   C 1024: loss 4e-5, logits 1.3e-2, flat gradient 5.7e-2 (5.1e-2 with the bf16 head, 4.2e-2 with bf16 dW too), worst tensor 0.18 (the LayerNorm-2 gains
#                 and W1, as at the scaled shape); since round 3 the block Linears' dW and lm_head's three contractions run on fp8 operands too
# bounds at ~2x; the bf16 bounds are those of tests/test_gpu_engine_oracle.py at the scaled configuration
BOUNDS = {"bf16": dict(loss=1e-4, logits=6e-3, flat=2e-2, worst=6e-2), "fp8": dict(loss=1e-3, logits=5e-2, flat=0.12, worst=0.35)}


@pytest.mark.parametrize("precision,C,NH", [("bf16", 768, 12), ("fp8", 1024, 16)])
def test_gpt2_width_engine_step_matches_oracle(dev, precision, C, NH):
    import drakegpt_amd as D
    from drakegpt_amd.engine import TrainEngine
    from oracle import drake_ref as R
    from oracle import rng_ref
    B, T, L, p, seed = 1, 1024, 2, 0.1, 4242
    torch.manual_seed(42)
    m = D.TransformerLM(V, C, T, NH, L, p, precision=precision).to(dev).train()
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    eng = TrainEngine(m, B, T, lr=3e-4, betas=(0.9, 0.95), seed=seed, use_graph=True)
    # the dispatch the full-size GPT-2 steps take: bf16 logits overwritten in place, atomic token scatter (no one-hot operand),
    # grouped dW, bf16 gradient stream
    assert eng.bf16_logits and eng.onehot is None and eng.grouped_dw and eng.stream_dtype == torch.bfloat16
    assert eng.fp8 == (precision == "fp8")
    g = torch.Generator().manual_seed(5)
    x = torch.randint(0, V, (B, T), generator=g)
    x[0, :64] = x[0, 64:128]                    # repeated ids: the scatter-add has to ADD
    y = torch.randint(0, V, (B, T), generator=g)
    eng.set_batch(x.to(dev), y.to(dev))
    loss = eng.step().item()                    # (fp8: the capture's eager warm-up step seeds the amax history; the replay is delayed-scaled)
    torch.cuda.synchronize()
    eng.check_status()
    got = {k: v.detach().clone().cpu() for k, v in eng.named_grads().items()}
    keys = R.trainable_keys("TransformerLM", sd)
    assert sorted(keys) == sorted(got.keys())
    masks = rng_ref.transformer_masks(seed, 0, p, B, T, C, NH, L)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    lo, ls, gr = R.loss_and_grads("TransformerLM", sd, x, y, p=p, training=True, masks=masks)
    per = {k: rel(got[k], gr[k]) for k in keys}
    worst = max(per.items(), key=lambda kv: kv[1])
    e = dict(loss=abs(loss - ls.item()) / ls.item(), flat=rel(_flat(got, keys), _flat(gr, keys)), worst=worst[1])
    # logits: a second engine on the same weights with keep_logits (fp32 logits, the module path's loss head)
    torch.manual_seed(42)
    m2 = D.TransformerLM(V, C, T, NH, L, p, precision=precision).to(dev).train()
    m2.load_state_dict(sd)
    eng2 = TrainEngine(m2, B, T, lr=3e-4, betas=(0.9, 0.95), seed=seed, use_graph=False)
    eng2.keep_logits = True
    eng2.set_batch(x.to(dev), y.to(dev))
    loss2 = eng2.step().item()
    e["logits"] = rel(eng2.last_logits.float(), lo)
    if os.environ.get("DG_TEST_REPORT"):
        print(f"[parity] GPT-2 widths {precision} C={C}: " + ", ".join(f"{k}={v:.2e}" for k, v in e.items()) + f" worst={worst[0]}"
              + f" loss_inplace_vs_fp32_logits={abs(loss - loss2) / loss2:.1e}", flush=True)
        print("[parity]   worst tensors: " + str(sorted(per.items(), key=lambda kv: -kv[1])[:5]), flush=True)
    b = BOUNDS[precision]
    assert all(e[k] < b[k] for k in b), (e, worst)
    # the token table: rows of ids that never occur stay exactly zero, the repeated ids' rows match the oracle
    tok = got["token_embedding_table.weight"]
    used = torch.zeros(V, dtype=torch.bool)
    used[x.view(-1)] = True
    assert torch.all(tok[~used] == 0)
    assert rel(tok[used], gr["token_embedding_table.weight"][used]) < b["worst"]
    if precision == "bf16":
        # the tight bound: the same arithmetic WITH the kernels' bf16 roundings (a rounding model, not reference arithmetic)
        lo2, ls2, gr2 = R.loss_and_grads("TransformerLM", sd, x, y, p=p, training=True, masks=masks, bf16=True, stream_bf16=True)
        per2 = {k: rel(got[k], gr2[k]) for k in keys}
        w2 = max(per2.items(), key=lambda kv: kv[1])
        f2 = rel(_flat(got, keys), _flat(gr2, keys))
        if os.environ.get("DG_TEST_REPORT"):
            print(f"[parity]   vs bf16-rounded oracle: flat={f2:.2e} worst={w2}", flush=True)
        assert f2 < 1.5e-2 and w2[1] < 6e-2, (f2, w2)
