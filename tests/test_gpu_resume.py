"""GPU: TrainEngine.state_dict() / load_state_dict() and the harness's --save-every / --resume: a resumed run is the same run.

"The same" is asserted bit for bit where the step has no atomics: the scaled widths of
test_gpu_engine.py::test_scaled_bf16_step_is_bit_reproducible (V 80, C 384, 6 heads, T 256, dropout 0.2, B 8; 2 layers here), where
the token-table gradient is a problem of the grouped dW GEMM.  The tiny C 32 configuration still has the fp32 atomics of the
embedding scatter-add; there the bound is the one test_graph_equals_eager_with_dropout gives them (2e-6 relative)."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
V, C, NH, T, B, P, L = 80, 384, 6, 256, 8, 0.2, 2
BETAS = (0.9, 0.95)


def _corpus():
    return torch.randint(0, V, (20_000,), generator=torch.Generator().manual_seed(1))


def _rows(n, seed=2):
    return torch.randint(0, 20_000 - T - 1, (n, B), generator=torch.Generator().manual_seed(seed))


def _scaled(dev, precision="bf16", model_seed=42, seed=20240607, graph=True, lr=3e-4, **kw):
    import drakegpt_amd as D
    from drakegpt_amd.engine import TrainEngine
    torch.manual_seed(model_seed)
    m = D.TransformerLM(V, C, T, NH, L, P, precision=precision).to(dev).train()
    eng = TrainEngine(m, B, T, lr=lr, betas=BETAS, seed=seed, use_graph=graph, **kw)
    assert eng.onehot is not None and eng.grouped_dw            # no atomics in the step: bit-reproducible across engines
    eng.set_corpus(_corpus().to(dev))
    return m, eng


def _through_a_file(sd, path):
    from drakegpt_amd import checkpoint as CK
    CK.save_train_state(path, sd)
    return CK.load_train_state(path)                            # torch.load(..., weights_only=True)


def _run_and_save(dev, path, precision, steps_before=3, steps_after=3):
    """engine A: stage 6 rows, 3 steps, state -> file, 3 more steps.  Returns what the continuations are compared with."""
    m, A = _scaled(dev, precision)
    A.stage_offsets(_rows(steps_before + steps_after))
    first = [A.step().item() for _ in range(steps_before)]
    sd = _through_a_file(A.state_dict(), path)
    at_save = {"state": A.state.clone(), "off": A.off_block[steps_before:steps_before + steps_after].clone(),
               "sites": {k: v.clone() for k, v in A.fp8_sites.items()}, "seeded": A._fp8_seeded}
    rest = [A.step().item() for _ in range(steps_after)]
    torch.cuda.synchronize()
    A.check_status()
    out = {"sd": sd, "first": first, "losses": rest, "at_save": at_save, "steps": A.step_count(),
           "final": {k: getattr(A, k).clone() for k in ("flat", "m_", "v_", "shadow")}}
    assert len(set(first + rest)) == steps_before + steps_after
    return out


@pytest.fixture(scope="module")
def bf16_run(dev, tmp_path_factory):
    return _run_and_save(dev, str(tmp_path_factory.mktemp("resume") / "bf16.state.pt"), "bf16")


def _assert_same_end(eng, losses, ref):
    torch.cuda.synchronize()
    eng.check_status()
    assert losses == ref["losses"], (losses, ref["losses"])
    for k, t in ref["final"].items():
        assert torch.equal(getattr(eng, k), t), k
    assert eng.step_count() == ref["steps"] == 6


# ------------------------------------------------------------------------------------------------ test 1
@pytest.mark.parametrize("graph", [True, False])
def test_bf16_fresh_engine_continues_in_the_middle_of_a_staged_block(dev, bf16_run, graph):
    """B: other initial weights, other dropout seed, other learning rate; loaded before any step, so capture (and its warm-up
    step) comes after the load.  No stage_offsets call: the three unconsumed rows travel in the file."""
    m, Bn = _scaled(dev, model_seed=7, seed=99, graph=graph, lr=1e-3)
    Bn.load_state_dict(bf16_run["sd"])
    assert Bn.step_count() == 3 and torch.equal(Bn.state, bf16_run["at_save"]["state"])
    assert Bn.hyper_host[0] == 3e-4 and Bn.seed == 20240607
    losses = [Bn.step().item() for _ in range(3)]
    _assert_same_end(Bn, losses, bf16_run)
    with pytest.raises(RuntimeError, match="used up"):
        Bn.step()                                               # the staged-row bookkeeping came along too


def test_bf16_running_engine_is_loaded_in_place(dev, bf16_run):
    """C has taken 2 steps of its own: graphs are captured and hold raw pointers.  The load keeps them, and the Parameters."""
    m, Cn = _scaled(dev, model_seed=8, seed=5)
    Cn.stage_offsets(_rows(2, seed=9))
    for _ in range(2):
        Cn.step()
    graphs, ptr = Cn._graphs, m.lm_head.weight.data_ptr()
    assert graphs is not None
    Cn.load_state_dict(bf16_run["sd"])
    assert Cn._graphs is graphs and m.lm_head.weight.data_ptr() == ptr and ptr == Cn.param_view("lm.w").data_ptr()
    losses = [Cn.step().item() for _ in range(3)]
    _assert_same_end(Cn, losses, bf16_run)
    # "model" loads into a plain module under the reference's names; the engine's weights are what it holds
    import drakegpt_amd as D
    plain = D.TransformerLM(V, C, T, NH, L, P, precision="bf16")
    plain.load_state_dict(bf16_run["sd"]["model"])


# ------------------------------------------------------------------------------------------------ test 2
def test_accumulation_and_clipping_continue(dev, tmp_path):
    kw = dict(accum_steps=2, max_grad_norm=0.5)
    m, A = _scaled(dev, **kw)
    A.stage_offsets(_rows(8))
    for _ in range(2):
        A.step()
    sd = _through_a_file(A.state_dict(), str(tmp_path / "acc.state.pt"))
    la = [A.step().item() for _ in range(2)]
    m2, Bn = _scaled(dev, model_seed=7, seed=99, accum_steps=2, max_grad_norm=2.0)
    Bn.load_state_dict(sd)
    assert Bn.max_grad_norm == 0.5 and Bn.step_count() == 2 and Bn.micro_step_count() == 4
    lb = [Bn.step().item() for _ in range(2)]
    torch.cuda.synchronize()
    assert la == lb, (la, lb)
    for k in ("flat", "m_", "v_", "gacc", "last_grad_norm", "shadow"):
        assert torch.equal(getattr(A, k), getattr(Bn, k)), k
    assert A.step_count() == Bn.step_count() == 4 and A.micro_step_count() == Bn.micro_step_count() == 8
    assert float(Bn.clip_state[2]) == 0.5                       # the file's threshold is the one in force
    Bn.stage_offsets(_rows(2, seed=4))
    Bn.micro_step()
    with pytest.raises(RuntimeError, match="1 of 2 micro-steps"):
        Bn.state_dict()
    Bn.micro_step()
    Bn.state_dict()


# ------------------------------------------------------------------------------------------------ test 3
@pytest.fixture(scope="module")
def fp8_runs(dev, tmp_path_factory):
    d = tmp_path_factory.mktemp("resume8")
    return [_run_and_save(dev, str(d / f"fp8_{i}.state.pt"), "fp8") for i in range(2)]


def test_fp8_uninterrupted_run_reproduces_itself(fp8_runs):
    """measured before anything is claimed about a continuation: the same six steps twice, two engines, same seeds"""
    a, b = fp8_runs
    la, lb = a["first"] + a["losses"], b["first"] + b["losses"]
    print("fp8 run-to-run: max |loss difference|", max(abs(x - y) for x, y in zip(la, lb)),
          "max |weight difference|", float((a["final"]["flat"] - b["final"]["flat"]).abs().max()))
    assert la == lb
    for k in a["final"]:
        assert torch.equal(a["final"][k], b["final"][k]), k
    assert a["at_save"]["sites"].keys() == b["at_save"]["sites"].keys()
    for k, t in a["at_save"]["sites"].items():
        assert torch.equal(t, b["at_save"]["sites"][k]), k


@pytest.mark.parametrize("running", [False, True])
def test_fp8_histories_are_restored_and_the_run_continues(dev, fp8_runs, running):
    """every buffer of the "engine" section and every amax history equals A's at the time of saving; the continuation is
    asserted bit for bit, which test_fp8_uninterrupted_run_reproduces_itself entitles it to"""
    ref = fp8_runs[0]
    m, Bn = _scaled(dev, "fp8", model_seed=7, seed=99)
    if running:                                                 # histories seeded and graphs captured by steps of its own
        Bn.stage_offsets(_rows(2, seed=9))
        for _ in range(2):
            Bn.step()
        graphs, sites = Bn._graphs, dict(Bn.fp8_sites)
    Bn.load_state_dict(ref["sd"])
    if running:
        assert Bn._graphs is graphs and all(Bn.fp8_sites[k] is t for k, t in sites.items())
    saved = ref["at_save"]
    assert saved["seeded"] and Bn._fp8_seeded and len(saved["sites"]) > 0
    assert torch.equal(Bn.state, saved["state"]) and torch.equal(Bn.off_block[:3], saved["off"])
    assert Bn.off_ctl.tolist() == [3, 3] and (Bn._off_rows, Bn._off_left) == (3, 3)
    assert Bn.fp8_sites.keys() == saved["sites"].keys()
    for k, t in saved["sites"].items():
        assert torch.equal(Bn.fp8_sites[k], t), k
    losses = [Bn.step().item() for _ in range(3)]
    _assert_same_end(Bn, losses, ref)


# ------------------------------------------------------------------------------------------------ tiny configuration (C 32)
def _tiny(dev, golden_dir, precision="fp32", dropout=0.0, init=True, B_=32, **kw):
    import drakegpt_amd as D
    from drakegpt_amd.engine import TrainEngine
    fix = torch.load(os.path.join(golden_dir, "traj5_TransformerLM.pt"), weights_only=True)
    m = D.TransformerLM(V, 32, 8, 4, 3, dropout, precision=precision)
    if init:
        m.load_state_dict(fix["init"])
    m = m.to(dev).train()
    return m, TrainEngine(m, B_, 8, lr=1e-3, betas=BETAS, **kw), fix


def _steps(eng, fix, its, dev):
    out = []
    for it in its:
        eng.set_batch(fix["x"][it][:eng.B].to(dev), fix["y"][it][:eng.B].to(dev))
        out.append(eng.step().item())
    return out


def test_fp32_set_batch_path_with_dropout(dev, golden_dir, tmp_path):
    """test 4: restored buffers are equal; the next two losses are within the bound the embedding atomics get elsewhere"""
    m, A, fix = _tiny(dev, golden_dir, dropout=0.1)
    _steps(A, fix, range(3), dev)
    sd = _through_a_file(A.state_dict(), str(tmp_path / "fp32.state.pt"))
    want = {k: getattr(A, k).clone() for k in ("flat", "m_", "v_", "state")}
    torch.manual_seed(123)
    m2, Bn, _ = _tiny(dev, golden_dir, dropout=0.1, init=False, seed=7)
    Bn.load_state_dict(sd)
    for k, t in want.items():
        assert torch.equal(getattr(Bn, k), t), k
    la, lb = _steps(A, fix, (3, 4), dev), _steps(Bn, fix, (3, 4), dev)
    for a, b in zip(la, lb):
        assert abs(a - b) <= 2e-6 * abs(a), (la, lb)
    assert A.step_count() == Bn.step_count() == 5


def _moments(eng):
    """{reference parameter name: (view of m_, view of v_)}"""
    return {k: tuple(buf.as_strided(g.size(), g.stride(), g.storage_offset()) for buf in (eng.m_, eng.v_))
            for k, g in eng.named_grads().items()}


def test_optimizer_state_interoperates_with_torch_and_the_module_path(dev, golden_dir):
    """test 5"""
    import drakegpt_amd as D
    from drakegpt_amd.optim import AdamW
    m, eng, fix = _tiny(dev, golden_dir)
    _steps(eng, fix, range(2), dev)
    osd = eng.optimizer_state_dict()
    mom = _moments(eng)
    names = [n for n, _ in m.named_parameters()]
    assert set(mom) == {n for n in names if not n.startswith("ln_f.")}
    # -> torch.optim.AdamW over a CPU copy
    cpu = D.TransformerLM(V, 32, 8, 4, 3, 0.0)
    cpu.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
    topt = torch.optim.AdamW(cpu.parameters(), lr=5.0)
    topt.load_state_dict(osd)
    assert topt.param_groups[0]["lr"] == 1e-3 and tuple(topt.param_groups[0]["betas"]) == BETAS
    for n, p in cpu.named_parameters():
        if n.startswith("ln_f."):
            assert p not in topt.state
            continue
        st = topt.state[p]
        assert float(st["step"]) == 2.0 and torch.equal(st["exp_avg"], mom[n][0].cpu()) and torch.equal(st["exp_avg_sq"], mom[n][1].cpu()), n
    # -> drakegpt_amd.optim.AdamW over a GPU copy
    gpu = D.TransformerLM(V, 32, 8, 4, 3, 0.0)
    gpu.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
    gpu = gpu.to(dev).train()
    gopt = AdamW(gpu.parameters(), lr=5.0)
    gopt.load_state_dict(osd)
    back = gopt.state_dict()
    assert set(back["state"]) == set(osd["state"])
    for i, st in back["state"].items():
        assert float(st["step"]) == 2.0
        assert torch.equal(st["exp_avg"].cpu(), osd["state"][i]["exp_avg"]) and torch.equal(st["exp_avg_sq"].cpu(), osd["state"][i]["exp_avg_sq"])
    # <- drakegpt_amd.optim.AdamW after 2 module-path steps, into another engine
    mod = D.TransformerLM(V, 32, 8, 4, 3, 0.0)
    mod.load_state_dict(fix["init"])
    mod = mod.to(dev).train()
    mopt = AdamW(mod.parameters(), lr=2e-3, betas=BETAS)
    for it in range(2):
        _, loss = mod(fix["x"][it].to(dev), fix["y"][it].to(dev))
        mopt.zero_grad()
        loss.backward()
        mopt.step()
    msd = mopt.state_dict()
    m3, eng3, _ = _tiny(dev, golden_dir)
    eng3.load_optimizer_state_dict(msd)
    assert eng3.step_count() == 2 and eng3.hyper_host[0] == 2e-3 and abs(float(eng3.hyper[0]) - 2e-3) < 1e-9
    mom3 = _moments(eng3)
    for i, n in enumerate(names):
        if n.startswith("ln_f."):
            assert i not in msd["state"]
            continue
        assert torch.equal(mom3[n][0], msd["state"][i]["exp_avg"]) and torch.equal(mom3[n][1], msd["state"][i]["exp_avg_sq"]), n
    # a state whose parameters disagree about the step count is refused and nothing is written
    before = eng3.m_.clone()
    msd["state"][0]["step"] = torch.tensor(5.0)
    with pytest.raises(ValueError, match="step count"):
        eng3.load_optimizer_state_dict(msd)
    assert torch.equal(eng3.m_, before) and eng3.step_count() == 2


def test_refusals_leave_the_engine_untouched(dev, golden_dir):
    """test 6"""
    m, A, fix = _tiny(dev, golden_dir)
    _steps(A, fix, range(1), dev)
    sd = A.state_dict()

    def refused(eng, state, field):
        if eng._graphs is None and eng.accum == 1:
            _steps(eng, fix, range(2), dev)                     # a state of its own to lose
        before = {k: getattr(eng, k).clone() for k in ("flat", "m_", "v_", "state")}
        with pytest.raises(ValueError, match=field) as ei:
            eng.load_state_dict(state)
        for k, t in before.items():
            assert torch.equal(getattr(eng, k), t), (field, k)
        return str(ei.value)

    msg = refused(_tiny(dev, golden_dir, accum_steps=2)[1], sd, r"meta\.accum_steps")
    assert "1" in msg and "2" in msg
    msg = refused(_tiny(dev, golden_dir, B_=16)[1], sd, r"meta\.batch_size")
    assert "32" in msg and "16" in msg
    msg = refused(_tiny(dev, golden_dir, precision="bf16")[1], sd, r"meta\.precision")
    assert "fp32" in msg and "bf16" in msg
    m2, E, _ = _tiny(dev, golden_dir, init=False)
    for section, key in (("engine", "step_word"), ("meta", "dropout"), ("model", "lm_head.bias"), (None, "optimizer")):
        bad = {k: (dict(v) if isinstance(v, dict) else v) for k, v in sd.items()}
        del (bad if section is None else bad[section])[key]
        refused(E, bad, key.replace(".", r"\."))
    refused(E, dict(sd, version=sd["version"] + 1), "version")
    refused(E, dict(sd, format="x"), "format")
    bad = dict(sd, optimizer={"state": {k: dict(v) for k, v in sd["optimizer"]["state"].items()}, "param_groups": sd["optimizer"]["param_groups"]})
    bad["optimizer"]["state"][3]["step"] = torch.tensor(9.0)
    refused(E, bad, "step count")
    E.load_state_dict(sd)                                       # and the good one still loads
    assert torch.equal(E.flat, A.flat) and E.step_count() == 1


def test_other_rank_rederives_its_dropout_stream(dev, golden_dir):
    """test 7: every rank loads rank 0's file"""
    from drakegpt_amd.engine import TrainEngine
    m, A, fix = _tiny(dev, golden_dir, dropout=0.1, seed=77)
    _steps(A, fix, range(2), dev)
    sd = A.state_dict()
    assert sd["engine"]["seed"] == 77
    m1, R1, _ = _tiny(dev, golden_dir, dropout=0.1, seed=5, rank=1)
    R1.load_state_dict(sd)
    m2, fresh, _ = _tiny(dev, golden_dir, dropout=0.1, seed=77, rank=1)
    assert torch.equal(R1.state[0:2], fresh.state[0:2]) and not torch.equal(R1.state[0:2], A.state[0:2])
    assert int(R1.state[2]) == 2 == R1.step_count()
    assert torch.equal(R1.flat, A.flat)


def test_a_diverged_run_is_not_saved(dev, golden_dir, tmp_path):
    """test 8"""
    from drakegpt_amd import train
    from drakegpt_amd.optim import AdamW
    m, A, fix = _tiny(dev, golden_dir)
    _steps(A, fix, range(1), dev)
    path = str(tmp_path / "run.state.pt")
    kw = dict(next_iteration=1, sched_steps=0, must_match={"model": "TransformerLM"}, model=m, engine=A)
    assert A.is_finite()
    train.save_run_state(path, **kw)
    good = open(path, "rb").read()
    for buf, val in ((A.flat, float("nan")), (A.v_, float("inf")), (A.m_, float("-inf"))):
        keep = buf[A.n_active - 1].clone()
        buf[A.n_active - 1] = val
        assert not A.is_finite()
        with pytest.raises(RuntimeError, match="diverged"):
            train.save_run_state(path, **kw)
        assert open(path, "rb").read() == good and os.listdir(str(tmp_path)) == ["run.state.pt"]
        buf[A.n_active - 1] = keep
    assert A.is_finite()
    # the autograd path's optimizer has the same helper, before and after its first step
    import drakegpt_amd as D
    mod = D.BlocksLM(V, 32, 8, 4, 3).to(dev).train()
    opt = AdamW(mod.parameters(), lr=1e-3)
    assert opt.is_finite()
    _, loss = mod(fix["x"][0].to(dev), fix["y"][0].to(dev))
    loss.backward()
    opt.step()
    assert opt.is_finite()
    with torch.no_grad():
        mod.lm_head.bias[3] = float("nan")
    assert not opt.is_finite()
    with pytest.raises(RuntimeError, match="diverged"):
        train.save_run_state(path, next_iteration=1, sched_steps=0, must_match={}, model=mod, optimizer=opt)
    assert open(path, "rb").read() == good


# ------------------------------------------------------------------------------------------------ harness
def _harness(capsys, argv):
    from drakegpt_amd import train
    train.main(argv)
    out = capsys.readouterr().out.split("\n")
    is_eval = [s.startswith("{") and '"val_loss"' in s for s in out]
    evals = [json.loads(s) for s, e in zip(out, is_eval) if e]
    saved = [i for i, s in enumerate(out) if s.startswith("saved ")]
    assert len(saved) == 1 and any(is_eval)
    last = max(i for i, e in enumerate(is_eval) if e)
    return evals, "\n".join(out[last + 1:saved[0]])             # the sample (it may hold line breaks of its own)


def _three_runs(capsys, tmp_path, golden_dir, base, name):
    data = ["--data", os.path.join(golden_dir, "corpus_fixture.txt"), "--eval-interval", "4", "--eval-iters", "2", "--sample", "8"]
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    ea, sa = _harness(capsys, base + data + ["--iters", "8", "--model-dir", a])
    eb, _ = _harness(capsys, base + data + ["--iters", "4", "--save-every", "4", "--model-dir", b])
    state = os.path.join(b, name + ".state.pt")
    assert os.path.isfile(state)
    ec, sc = _harness(capsys, base + data + ["--iters", "8", "--resume", state, "--model-dir", b])
    assert [ln["step"] for ln in ea] == [4, 8] and [ln["step"] for ln in eb] == [4] and [ln["step"] for ln in ec] == [8]
    fa = torch.load(os.path.join(a, name + ".pt"), weights_only=True)
    fc = torch.load(os.path.join(b, name + ".pt"), weights_only=True)
    return ea, eb + ec, sa, sc, fa, fc


def test_harness_resume_is_bit_for_bit(dev, capsys, monkeypatch, tmp_path, golden_dir):
    """test 9: --iters 8 against --iters 4 --save-every 4 followed by --resume --iters 8"""
    from drakegpt_amd import train
    monkeypatch.setitem(train.PRESETS, "resume_test", {
        "context_length": T, "batch_size": B, "base_lr": 3e-4, "max_lr": 6e-4, "betas": BETAS, "embedding_dim": C, "head_size": 64,
        "num_heads": NH, "num_layers": L, "dropout": P})
    ea, ec, sa, sc, fa, fc = _three_runs(capsys, tmp_path, golden_dir, ["--preset", "resume_test", "--precision", "bf16"], "TransformerLM")
    strip = lambda lines: [{k: v for k, v in ln.items() if k != "tokens_per_s"} for ln in lines]      # noqa: E731
    assert strip(ea) == strip(ec), (ea, ec)
    assert sa == sc
    assert fa.keys() == fc.keys()
    for k in fa:
        assert torch.equal(fa[k], fc[k]), k
    # tokens_per_s counts this process's steps: the resumed run took 4 of the 8
    assert all(ln["tokens_per_s"] > 0 for ln in ec)


def test_harness_resume_autograd_path(dev, capsys, tmp_path, golden_dir):
    """test 10: BlocksLM (optim.AdamW's state_dict in the engine's place).  2e-5 relative is the bound
    test_two_ranks_equal_one_process gives the same kind of difference (atomics in the module path's backward); a run resumed
    with the wrong generator state trains on other batches and misses it by orders of magnitude."""
    ea, ec, sa, sc, fa, fc = _three_runs(capsys, tmp_path, golden_dir, ["--model", "BlocksLM", "--precision", "fp32"], "BlocksLM")
    assert len(ea) == len(ec) == 2
    for x, y in zip(ea, ec):
        assert x["step"] == y["step"] and x["lr"] == y["lr"]
        for k in ("train_loss", "val_loss"):
            print(k, x[k], y[k])
            assert abs(x[k] - y[k]) <= 2e-5 * abs(x[k]), (k, x, y)
    assert fa.keys() == fc.keys()
