"""The graph-captured training engine against the reference's 5-step AdamW trajectory (golden)
and against its own eager execution."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
V = 80


def _mk(dev, golden_dir, precision="fp32", dropout=0.0, graph=True, B=32, T=8):
    import drakegpt_amd as D
    from drakegpt_amd.engine import TrainEngine
    fix = torch.load(os.path.join(golden_dir, "traj5_TransformerLM.pt"), weights_only=True)
    m = D.TransformerLM(V, 32, 8, 4, 3, dropout, precision=precision)
    m.load_state_dict(fix["init"])
    m = m.to(dev)
    eng = TrainEngine(m, B, T, lr=1e-3, betas=(0.9, 0.95), use_graph=graph)
    return m, eng, fix


@pytest.mark.parametrize("graph", [False, True])
def test_five_step_trajectory_matches_reference(dev, golden_dir, graph):
    m, eng, fix = _mk(dev, golden_dir, graph=graph)
    losses = []
    for it in range(5):
        eng.set_batch(fix["x"][it].to(dev), fix["y"][it].to(dev))
        losses.append(eng.step().item())
    ref = fix["losses"].tolist()
    for a, b in zip(losses, ref):
        assert abs(a - b) < 2e-4 * abs(b), (losses, ref)
    sd = m.state_dict()
    for k, v in fix["final"].items():
        assert (sd[k].cpu() - v).abs().max().item() < 2e-5, k
    # ln_f untouched by the optimizer (no grad, no weight decay): the reference leaves it at init
    assert torch.equal(sd["ln_f.weight"].cpu(), torch.ones(32)) and torch.equal(sd["ln_f.bias"].cpu(), torch.zeros(32))
    assert eng.step_count() == 5


def test_state_dict_views_and_checkpoint_roundtrip(dev, golden_dir, tmp_path):
    """parameters are views of the flat buffer; the saved state_dict loads into a fresh model."""
    import drakegpt_amd as D
    m, eng, fix = _mk(dev, golden_dir)
    eng.set_batch(fix["x"][0].to(dev), fix["y"][0].to(dev))
    eng.step()
    path = tmp_path / "TransformerLM.pt"
    torch.save(m.state_dict(), path)
    sd = torch.load(path, weights_only=True)
    ck = torch.load(os.path.join(golden_dir, "checkpoints", "TransformerLM.pt"), weights_only=True)
    assert list(sd.keys()) == list(ck.keys()) and all(sd[k].shape == ck[k].shape for k in ck)
    m2 = D.TransformerLM(V, 32, 8, 4, 3, 0.0).to(dev)
    m2.load_state_dict(sd)
    x = fix["x"][1].to(dev)
    m.eval(); m2.eval()
    assert torch.allclose(m(x)[0], m2(x)[0], atol=1e-6)
    # the module (autograd) path and the engine's eval path agree on the adopted weights
    y = fix["y"][1].to(dev)
    l_mod = m(x, y)[1].item()
    l_eng = eng.eval_loss(x, y).item()
    assert abs(l_mod - l_eng) < 1e-5


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_graph_equals_eager_with_dropout(dev, golden_dir, precision):
    """same seed => the captured graph and the eager program produce the same losses, including
    the device-side step counter that re-keys the dropout masks every replay."""
    out = []
    for graph in (False, True):
        m, eng, fix = _mk(dev, golden_dir, precision=precision, dropout=0.1, graph=graph)
        ls = []
        for it in range(5):
            eng.set_batch(fix["x"][it].to(dev), fix["y"][it].to(dev))
            ls.append(eng.step().item())
        out.append(ls)
    # equal up to the one non-deterministic reduction this small configuration still has: the fp32 atomics of the
    # token-embedding scatter-add (the one-hot GEMM form needs C >= V / 2; see test_scaled_bf16_step_is_bit_reproducible)
    for a, b in zip(*out):
        assert abs(a - b) <= 2e-6 * abs(b), out
    assert len(set(out[0])) == 5


def test_scaled_bf16_step_is_bit_reproducible(dev):
    """TransformerLM_scaled in bf16: no atomics anywhere in the step (the token-table gradient is a problem of the grouped dW
    GEMM, the K halves of every dW tile are summed in a fixed order), so two engines with the same seed -- one replaying a
    captured graph, one running eagerly -- agree bit for bit in losses, gradients and updated weights."""
    import drakegpt_amd as D
    from drakegpt_amd.engine import TrainEngine
    from oracle import drake_ref as R
    cfg = R.SCALED
    Vv, B, T = 80, 8, 256
    g = torch.Generator().manual_seed(7)
    xs = torch.randint(0, Vv, (3, B, T), generator=g)
    ys = torch.randint(0, Vv, (3, B, T), generator=g)
    res = []
    for graph in (True, False):
        torch.manual_seed(42)
        m = D.TransformerLM(Vv, cfg["embedding_dim"], T, cfg["num_heads"], cfg["num_layers"], cfg["dropout"], precision="bf16").to(dev).train()
        eng = TrainEngine(m, B, T, lr=1e-3, betas=(0.9, 0.95), use_graph=graph, seed=5)
        assert eng.onehot is not None and eng.grouped_dw
        losses = []
        for it in range(3):
            eng.set_batch(xs[it].to(dev), ys[it].to(dev))
            losses.append(eng.step().item())
        torch.cuda.synchronize()
        res.append((losses, eng.gflat.clone(), eng.flat.clone()))
    assert res[0][0] == res[1][0], (res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])
    assert len(set(res[0][0])) == 3


def test_corpus_gather_path(dev, golden_dir):
    from oracle import drake_ref as R
    m, eng, fix = _mk(dev, golden_dir)
    data = torch.randint(0, V, (5000,), generator=torch.Generator().manual_seed(42))
    eng.set_corpus(data)
    gen = torch.Generator().manual_seed(5)
    ix = torch.randint(len(data) - 8, (32,), generator=gen)
    eng.set_offsets(ix.to(dev))
    eng.step()
    gen = torch.Generator().manual_seed(5)
    x, y = R.get_batch(data, 8, 32, gen)
    assert torch.equal(eng.x.cpu(), x) and torch.equal(eng.y.cpu(), y)


def test_staged_offsets_walk_equals_per_step_offsets(dev, golden_dir):
    """stage_offsets: the captured step picks row (step word - word at staging) of the block by itself; the batches, losses
    and parameters are those of set_offsets before every step (get_batch, ref: src/preprocessing.py:43-45), across two stagings
    and a switch back to the one-row form; a used-up block raises instead of silently reusing its last row"""
    from oracle import drake_ref as R
    from drakegpt_amd.engine import TrainEngine
    data = torch.randint(0, V, (5000,), generator=torch.Generator().manual_seed(42))
    offs = torch.stack([torch.randint(len(data) - 8, (32,), generator=torch.Generator().manual_seed(50 + i)) for i in range(7)])
    res = []
    for staged in (False, True):
        m, eng, fix = _mk(dev, golden_dir)
        eng.set_corpus(data)
        losses, xs = [], []
        for i in range(7):
            if not staged or i == 6:
                eng.set_offsets(offs[i].to(dev) if i % 2 else offs[i])
            elif i in (0, 4):
                eng.stage_offsets(offs[0:4] if i == 0 else offs[4:6].to(dev))
            losses.append(eng.step().item())
            xs.append(eng.x.cpu().clone())
            if i == 5 and staged:
                with pytest.raises(RuntimeError, match="used up"):
                    eng.step()
        res.append((losses, xs, eng.flat.clone()))
    # (this tiny fp32 model takes the atomic token scatter-add: two runs agree to fp32 summation order, not bit for bit)
    assert res[0][0] == pytest.approx(res[1][0], rel=1e-5)
    assert all(torch.equal(a, b) for a, b in zip(res[0][1], res[1][1])) and torch.allclose(res[0][2], res[1][2], rtol=1e-4, atol=1e-6)
    for i in range(7):
        x, _ = R.get_batch(data, 8, 32, torch.Generator().manual_seed(50 + i))
        assert torch.equal(res[1][1][i], x)
    with pytest.raises(IndexError, match="do not fit"):
        eng.stage_offsets(torch.full((2, 32), len(data) - 8))
    with pytest.raises(ValueError, match="stage_offsets"):
        eng.stage_offsets(offs[0])
    big = torch.randint(len(data) - 8, (TrainEngine.OFFSET_ROWS + 3, 32), generator=torch.Generator().manual_seed(9))
    eng.stage_offsets(big)                                    # grows the block (new address: the step is captured again)
    for i in range(3):
        eng.step()
    assert torch.equal(eng.x.cpu(), torch.stack([data[o:o + 8] for o in big[2].tolist()]))


@pytest.mark.parametrize("name", ["BigramLM", "TransformerLM"])
def test_module_path_with_hip_adamw_matches_reference_trajectory(dev, golden_dir, name):
    """the drop-in loop of src/train.py:146-151 (forward, zero_grad, backward, step) on the autograd path"""
    import drakegpt_amd as D
    from drakegpt_amd.optim import AdamW
    fix = torch.load(os.path.join(golden_dir, f"traj5_{name}.pt"), weights_only=True)
    m = D.BigramLM(V) if name == "BigramLM" else D.TransformerLM(V, 32, 8, 4, 3, 0.0)
    m.load_state_dict(fix["init"])
    m = m.to(dev).train()
    opt = AdamW(m.parameters(), lr=1e-3, betas=(0.9, 0.95))
    for it in range(5):
        logits, loss = m(fix["x"][it].to(dev), fix["y"][it].to(dev))
        opt.zero_grad()
        loss.backward()
        opt.step()
        assert abs(loss.item() - fix["losses"][it].item()) < 2e-4 * abs(fix["losses"][it].item())
    sd = m.state_dict()
    for k, v in fix["final"].items():
        assert (sd[k].cpu() - v).abs().max().item() < 2e-5, k


def test_train_harness_smoke(dev, tmp_path, capsys):
    from drakegpt_amd import train
    train.main(["--model", "TransformerLM", "--iters", "6", "--eval-interval", "3", "--eval-iters", "2", "--precision", "fp32",
                "--model-dir", str(tmp_path), "--sample", "5"])
    out = capsys.readouterr().out
    assert '"val_loss"' in out and "saved" in out
    sd = torch.load(tmp_path / "TransformerLM.pt", weights_only=True)
    assert "blocks.2.sa_head.heads.3.tril" in sd and sd["ln_f.weight"].eq(1).all()
    train.main(["--model", "BlocksLM", "--iters", "4", "--eval-interval", "2", "--eval-iters", "2", "--precision", "fp32", "--no-save",
                "--sample", "3"])


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_captured_evaluation_equals_eager(dev, golden_dir, precision):
    """evaluate_loss through the engine (one gather + one captured forward per batch, losses kept on the device) gives the
    same batch losses as the eager eval path, before and after a training step (the graph reads the live weights), and
    evaluate_loss consumes the CPU generator exactly as the reference's loop does."""
    from drakegpt_amd import ops, train
    m, eng, fix = _mk(dev, golden_dir, precision=precision, dropout=0.1)
    g = torch.Generator().manual_seed(11)
    data = torch.randint(0, V, (5000,), generator=g).to(dev)
    offs = torch.randint(5000 - 8, (6, 32), generator=g).to(dev)

    def eager():
        out = []
        for i in range(offs.shape[0]):
            x, y = ops.batch_gather(data, offs[i], 8)
            out.append(eng.eval_loss(x, y).item())
        return torch.tensor(out)
    assert torch.equal(eng.eval_losses(data, offs).cpu(), eager())
    eng.set_batch(fix["x"][0].to(dev), fix["y"][0].to(dev))
    eng.step()
    after = eng.eval_losses(data, offs).cpu()
    assert torch.equal(after, eager())
    assert not torch.equal(after[:1], torch.tensor([0.0]))
    # evaluate_loss: train then val, eval_iters draws of B offsets each from the given generator
    m.eval()
    ga, gb = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    got = train.evaluate_loss(data, data[:3000], m, 4, 8, 32, dev, engine=eng, generator=ga)
    want = {}
    for name, d in (("train", data), ("val", data[:3000])):
        ls = []
        for _ in range(4):
            ix = torch.randint(len(d) - 8, (32,), generator=gb).to(dev)
            x, y = ops.batch_gather(d, ix, 8)
            ls.append(eng.eval_loss(x, y).item())
        want[name] = sum(ls) / 4
    for k in want:
        assert abs(got[k].item() - want[k]) < 1e-6, (k, got, want)
    assert torch.equal(torch.randint(10, (3,), generator=ga), torch.randint(10, (3,), generator=gb))


def test_rccl_data_parallel_path_world_size_one():
    """the multi-rank step (backward graph -> RCCL all-reduce of the flat gradient -> optimizer graph) on a world-size-1
    "nccl" group in a child process: same losses as the single-graph step (tools/dp_rccl_smoke.py)."""
    import random
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(random.randint(20000, 40000)), RANK="0", WORLD_SIZE="1",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "dp_rccl_smoke.py")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "RCCL data-parallel path ok" in r.stdout


def test_out_of_range_ids_raise_like_torch(dev, golden_dir):
    """nn.Embedding / F.cross_entropy raise on a bad id in the reference (ref: src/model.py:595,606); the kernels clamp (they must
    never fault), so the Python layer raises where ids enter: module forward / generate, engine set_corpus / set_batch / host
    offsets -- a vocabulary mismatch must not train on aliased ids with a plausible loss."""
    import drakegpt_amd as D
    m, eng, fix = _mk(dev, golden_dir)
    x, y = fix["x"][0].clone(), fix["y"][0].clone()
    bad = x.clone(); bad[3, 5] = V
    neg = y.clone(); neg[0, 0] = -1
    with pytest.raises(IndexError, match="out of range"):
        m(bad.to(dev), y.to(dev))
    with pytest.raises(IndexError, match="out of range"):
        m(x.to(dev), neg.to(dev))
    with pytest.raises(IndexError, match="out of range"):
        m.eval().generate(bad[3:4, 2:6].to(dev), 3)
    with pytest.raises(IndexError, match="out of range"):
        D.BigramLM(V).to(dev)(bad.to(dev))
    with pytest.raises(IndexError, match="out of range"):
        eng.set_batch(bad.to(dev), y.to(dev))
    with pytest.raises(IndexError, match="out of range"):
        eng.set_corpus(torch.arange(200) % (V + 1))
    eng.set_corpus(torch.arange(200) % V)
    with pytest.raises(IndexError, match="do not fit"):
        eng.set_offsets(torch.full((32,), 200 - 8))           # needs T + 1 = 9 tokens from the offset on
    eng.set_offsets(torch.full((32,), 200 - 9))
    m.train()
    logits, loss = m(x.to(dev), y.to(dev))                     # the valid batch still runs
    assert torch.isfinite(loss)
    # the range check is one or two device-to-host syncs per forward that nn.Embedding does not have: a caller that has
    # validated its data source once can switch it off -- a bad id is then clamped by the kernels, never a fault
    m.check_ids = False
    _, loss_bad = m(bad.to(dev), y.to(dev))
    assert torch.isfinite(loss_bad)
    m.check_ids = True
    with pytest.raises(IndexError, match="out of range"):
        m(bad.to(dev), y.to(dev))


def test_train_harness_on_text_and_on_pt_files(dev, golden_dir, tmp_path, capsys):
    """the data-side row: text -> get_train_val_data -> train_data.pt / val_data.pt -> train.py, and train.py on
    the text directly; both see the same token streams, so with the same seed they print the same losses
    (ref: src/preprocessing.py:48-86, src/train.py:94-100)."""
    from drakegpt_amd import preprocessing, train
    src = os.path.join(golden_dir, "corpus_fixture.txt")
    tp, vp = str(tmp_path / "train_data.pt"), str(tmp_path / "val_data.pt")
    _, _, vocab = preprocessing.get_train_val_data(src, tp, vp, verbose=False)
    common = ["--model", "TransformerLM", "--iters", "8", "--eval-interval", "4", "--eval-iters", "3", "--precision", "fp32", "--no-save",
              "--sample", "12"]
    train.main(common + ["--data", src])
    a = capsys.readouterr().out
    train.main(common + ["--data", src, "--train-data", tp, "--val-data", vp])
    b = capsys.readouterr().out
    import json
    la = [json.loads(l) for l in a.splitlines() if l.startswith("{")]
    lb = [json.loads(l) for l in b.splitlines() if l.startswith("{")]
    # (equal up to the fp32 atomics of the token-table scatter-add at this tiny configuration)
    assert len(la) == 2 and len(lb) == 2
    for ra, rb in zip(la, lb):
        assert ra["train_loss"] == pytest.approx(rb["train_loss"], rel=1e-5) and ra["val_loss"] == pytest.approx(rb["val_loss"], rel=1e-5)
    assert all(0 < r["val_loss"] < 6 for r in la) and la[1]["lr"] == pytest.approx(2.6e-3)
    # the sample is decoded with the text's own mapper: characters of the fixture's vocabulary
    fix = torch.load(os.path.join(golden_dir, "corpus_fixture.pt"), weights_only=True)
    sample = a[a.rindex("}\n") + 2:]                        # everything after the last JSON line: 1 start token + 12 sampled + newline
    assert len(sample) == 14 and set(sample) <= set(fix["vocab"]) | {"\n"} and vocab == fix["vocab_size"]
    # .pt files alone (no text): the vocabulary is taken from the streams
    train.main(common + ["--train-data", tp, "--val-data", vp, "--iters", "4"])
    assert '"val_loss"' in capsys.readouterr().out


def test_dw_handover_error_word_stops_the_harness(dev):
    """a timed-out split-K hand-over of the grouped dW GEMM sets a sticky error word and the launch carries
    on with incomplete sums -- the losses still look plausible.  The harness reads the word wherever it synchronises anyway
    (on_eval, end of the run; bench.py after its timed region) and raises.  Here the word is set by hand."""
    import drakegpt_amd as D
    from drakegpt_amd import train
    from drakegpt_amd.engine import TrainEngine
    torch.manual_seed(0)
    B, T, C = 8, 64, 128
    m = D.TransformerLM(V, C, T, 2, 2, 0.0, precision="bf16").to(dev).train()
    eng = TrainEngine(m, B, T, lr=1e-3, seed=1, use_graph=False)
    assert eng.grouped_dw
    n_train = 4000
    eng.set_corpus(torch.randint(0, V, (n_train,), generator=torch.Generator().manual_seed(1)))
    seen = []
    train.engine_loop(eng, n_train, T, B, 0, 1, 4, 2, lambda it: (eng.check_status(), seen.append(it)), dev, generator=torch.Generator().manual_seed(2))
    assert seen == [1, 3] and eng.tn_workspaces
    ws = next(iter(eng.tn_workspaces.values()))
    ws[-16:].view(torch.int32)[0] = 1                 # what dg_gemm_tn_grouped's bounded wait leaves behind when it runs out
    with pytest.raises(RuntimeError, match="hand-over timed out"):
        eng.check_status()
    with pytest.raises(RuntimeError, match="hand-over timed out"):      # the loop's own end-of-run check (no evaluation in range)
        train.engine_loop(eng, n_train, T, B, 0, 1, 2, 100, lambda it: None, dev, generator=torch.Generator().manual_seed(3))
    ws[-16:].view(torch.int32)[0] = 0
    eng.check_status()


def test_bench_entry_under_torch_distributed_run():
    """the exact entry the driver's SCALE leg uses -- `python -m torch.distributed.run --nproc-per-node N bench.py --gpus N` --
    with N = 1 (the box has one GPU): a fresh child, a world-size-1 "nccl" group created before any other GPU call, one JSON
    line on stdout carrying the contract's fields"""
    import json
    import random
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(random.randint(20000, 40000)), os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
           "--no-extra", "--no-cpu-baseline", "--no-kernel-timing"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 1 and out["steps"] == 3 and out["warmup"] == 2 and out["scaling"] == "weak" and out["value"] > 0
    assert out["config"]["parallelism"] == "dp1" and "TransformerLM_scaled" in out["config"]["workload"] and out["dtype"] == "bf16"


def test_bench_plain_run_is_the_headline_only():
    """`python bench.py --steps K --warmup W` without --full: the headline line's fields, and none of the legs that take
    runs of their own (roofline / hbm_kernels, extra_configs, cpu_baseline) -- the line says so with nulls"""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "TORCHELASTIC_RUN_ID"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2"],
                       env=env, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["metric"] == "training tokens/sec (fwd+bwd+AdamW)" and out["unit"] == "tokens/s" and out["higher_is_better"] is True
    assert out["steps"] == 3 and out["warmup"] == 2 and out["dtype"] == "bf16" and out["value"] > 0 and out["ms_per_step"] > 0
    assert out["roofline"] is None and out["hbm_kernels"] is None and out["extra_configs"] is None and out["cpu_baseline"] is None
    assert "[bench] cpu baseline" not in r.stderr and "[bench] extra " not in r.stderr, r.stderr[-2000:]


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


@pytest.mark.parametrize("switch", ["DG_CHAIN_LN", "DG_CHAIN", "DG_CHAIN_BWD"])
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_layernorm_inside_gemm_epilogue_equals_separate_launches(dev, p, switch):
    """round 3: proj + residual + LayerNorm 2 and FFN2 + residual + the next block's LayerNorm 1 as row-complete GEMMs whose
    epilogue runs the LayerNorm (dg_block_chain_fwd modes 3 / 4, ref: src/model_component.py:454,505-506,320-325) against the
    same engine with the separate dg_gemm_nt + dg_layernorm_fwd launches (DG_CHAIN_LN=0), and the WHOLE row-local chain between two
    attention calls as one launch per layer (DG_CHAIN=1: modes 2 / 0 / 1) against the same: same GEMM arithmetic and dropout masks,
    row statistics combined from four 96-column partials instead of one wave-wide sum -- differences at fp32 rounding level in
    mean / rstd, an occasional bf16 ulp in the normalised activations.  Also the packed-weight refresh after the optimizer step
    (second step: Adam's first update is lr * sign(g), so gradients that differ in the last bit near zero move weights apart by
    2 lr -- the second step's bounds are those of two bf16 runs, not of one kernel) and the forward-only evaluation path.
    DG_CHAIN_BWD=1: the backward pass's row-local chain (dg_block_chain_bwd modes 1 / 0 / 2: dX GEMMs with the LayerNorm backward in
    the epilogue, two partial rows per 64-row block for the bias / LayerNorm gradients) against the separate launches."""
    import drakegpt_amd as D
    from drakegpt_amd.engine import TrainEngine
    B, T, C, NH, L = 8, 256, 384, 6, 3
    g = torch.Generator().manual_seed(4)
    xs = [torch.randint(0, V, (B, T), generator=g).to(dev) for _ in range(2)]
    ys = [torch.randint(0, V, (B, T), generator=g).to(dev) for _ in range(2)]
    out = {}
    for mode in ("1", "0"):
        os.environ[switch] = mode
        if switch == "DG_CHAIN_LN":
            os.environ["DG_CHAIN"] = "0"                # (the one-launch chain is the default: off for this comparison)
        try:
            torch.manual_seed(42)
            m = D.TransformerLM(V, C, T, NH, L, p, precision="bf16").to(dev).train()
            eng = TrainEngine(m, B, T, lr=1e-3, seed=11, use_graph=True)
        finally:
            os.environ.pop(switch, None)
            os.environ.pop("DG_CHAIN", None)
        assert {"DG_CHAIN_LN": eng.chain_ln, "DG_CHAIN": eng.chain_full, "DG_CHAIN_BWD": eng.chain_bwd}[switch] == (mode == "1")
        if switch == "DG_CHAIN_LN":
            assert not eng.chain_full
        eng.keep_logits = True
        res = []
        for x, y in zip(xs, ys):
            eng.set_batch(x, y)
            loss = eng.step().item()
            res.append((loss, eng.last_logits.float().clone(), torch.cat([v.reshape(-1).float() for v in eng.named_grads().values()]).clone()))
        res.append(eng.eval_loss(xs[0], ys[0]).item())
        out[mode] = res
    for s in range(2):
        (l1, lg1, g1), (l0, lg0, g0) = out["1"][s], out["0"][s]
        # measured: step 0 logits 8e-4 / gradient 3e-3, step 1 logits 2.0e-3 / gradient 4.3e-3
        assert abs(l1 - l0) < (2e-5, 2e-4)[s] * abs(l0), (s, l1, l0)
        assert rel(lg1, lg0) < (2e-3, 6e-3)[s] and rel(g1, g0) < (6e-3, 1.2e-2)[s], (s, rel(lg1, lg0), rel(g1, g0))
    assert abs(out["1"][2] - out["0"][2]) < 2e-4 * abs(out["0"][2])
