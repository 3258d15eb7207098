"""GPU: the learning-rate table and the no-decay bitmap inside the AdamW launch (dg_adamw_step_sched), and TrainEngine(lr_schedule=,
no_decay=) on top of it.

Kernel level: every comparison is bit for bit -- p, m, v, the bf16 shadow and the step word -- against dg_adamw_step /
dg_adamw_step_clip: with hyper[0] set to the table entry the clamp rule picks, and, for the bitmap, against two runs with
weight_decay 0.1 and 0 stitched per 64-float granule on the host.  n = 2048 * 256 * 4 + 64 * 5 + 3 takes the grid-stride loop
round a second time, has a scalar tail of n % 4 = 3 elements and a partial last granule; n = 67 is one partial workgroup.

Engine level: the tiny fixture's model (traj5_TransformerLM.pt: C 32, T 8, 3 layers) in fp32.  Two engines are compared bit for
bit there, and this configuration sums the token-table gradient with fp32 atomics whose order is free: the batches of those
tests repeat ONE sequence of distinct tokens in every row, so every contribution to a table row is the same number and the sum
does not depend on the order (the trick of test_gpu_accum.py::test_accum_steps_one_is_bit_identical_to_no_argument, which
cannot be used as it is at B 32: 256 tokens do not fit 80 ids twice each).  The comparison with the oracle has a tolerance and
runs on the fixture's own batches.  The resume test runs at the widths of tests/test_gpu_resume.py, where the step has no
atomics."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
V = 80
BETAS = (0.9, 0.95)
N_BIG = 2048 * 256 * 4 + 64 * 5 + 3
SIZES = [N_BIG, 67]
HYPER = [1e-3, 0.9, 0.95, 1e-8, 0.1]


# ------------------------------------------------------------------------------------------------ kernel
@pytest.fixture(scope="module")
def base(dev):
    """p, g, m, v of both sizes, made once and never written (every run works on clones)"""
    out = {}
    for n in SIZES:
        g = torch.Generator().manual_seed(n)
        out[n] = tuple(t.to(dev) for t in (torch.randn(n, generator=g), 0.01 * torch.randn(n, generator=g),
                                            0.01 * torch.randn(n, generator=g), 1e-4 * torch.rand(n, generator=g)))
    return out


def _run(base, n, dev, entry, *, step=0, hyper=HYPER, clip=None, table=None, bits=None, advance=False, scale=0.5):
    """one launch on clones; entry "old": ops.adamw_step without table / bitmap (dg_adamw_step, dg_adamw_step_clip), "sched":
    dg_adamw_step_sched called directly (also with both NULL, which ops.adamw_step never does)"""
    from drakegpt_amd import ops
    p, g, m, v = (t.clone() for t in base[n])
    shadow = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    state = ops.new_rng_state(123, dev, step)
    hy = torch.tensor(hyper, dtype=torch.float32, device=dev)
    coef = None if clip is None else torch.tensor([clip], dtype=torch.float32, device=dev)
    if entry == "old":
        ops.adamw_step(p, g, m, v, hy, state, scale, shadow_bf16=shadow, n=n, advance=advance, clip=coef)
    else:
        ops.check(ops.lib.dg_adamw_step_sched(ops._p(p), ops._p(g), ops._p(m), ops._p(v), n, ops._p(hy), ops._p(state), scale, ops._p(coef),
                                              ops._p(table), 0 if table is None else table.numel(), ops._p(bits), ops._p(shadow),
                                              int(advance), ops._stream()), "dg_adamw_step_sched")
    torch.cuda.synchronize()
    assert torch.equal(g, base[n][1])
    return {"p": p.cpu(), "m": m.cpu(), "v": v.cpu(), "shadow": shadow.cpu(), "state": state.cpu()}


def _assert_same_bits(got, want, what):
    for k in ("p", "m", "v"):
        assert np.array_equal(got[k].numpy().view(np.uint32), want[k].numpy().view(np.uint32)), (what, k)
    assert np.array_equal(got["shadow"].view(torch.int16).numpy(), want["shadow"].view(torch.int16).numpy()), (what, "shadow")
    assert got["state"].tolist() == want["state"].tolist(), (what, got["state"].tolist(), want["state"].tolist())


@pytest.mark.parametrize("n", SIZES)
def test_without_table_and_bitmap_the_new_entry_is_the_old_one(dev, base, n):
    for advance in (False, True):
        _assert_same_bits(_run(base, n, dev, "sched", step=3, advance=advance), _run(base, n, dev, "old", step=3, advance=advance), "plain")
        _assert_same_bits(_run(base, n, dev, "sched", step=3, clip=0.37, advance=advance),
                          _run(base, n, dev, "old", step=3, clip=0.37, advance=advance), "clip")
    moved = _run(base, n, dev, "old", step=3)
    assert not torch.equal(moved["p"], base[n][0].cpu()) and not torch.equal(moved["p"], _run(base, n, dev, "old", step=3, clip=0.37)["p"])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("length", [5, 1])
def test_table_entry_by_the_step_word(dev, base, n, length):
    """lr = table[min(step word, len - 1)]: against dg_adamw_step with that entry in hyper[0]; hyper[0] itself is not read"""
    values = [7e-4, 1e-3, 2.5e-4, 0.0, 3e-5][:length] if length > 1 else [4e-4]
    table = torch.tensor(values, dtype=torch.float32, device=dev)
    seen = set()
    for step in sorted({0, 3, length - 1, length, length + 1000}):
        lr = float(table[min(step, length - 1)])
        want = _run(base, n, dev, "old", step=step, hyper=[lr] + HYPER[1:], advance=True)
        got = _run(base, n, dev, "sched", step=step, hyper=[123.0] + HYPER[1:], table=table, advance=True)
        _assert_same_bits(got, want, f"step word {step}")
        assert got["state"].tolist()[2:] == [step + 1, 0]          # advance: the word moves once, the arrival counter is clear again
        still = _run(base, n, dev, "sched", step=step, hyper=[123.0] + HYPER[1:], table=table, advance=False)
        assert still["state"].tolist()[2:] == [step, 0] and torch.equal(still["p"], got["p"])
        seen.add(lr)
    assert len(seen) == (3 if length == 5 else 1)                  # the step words picked entries 0, 3 and 4 (three times)


def _granules(n):
    return (n + 63) // 64


def _patterns(n):
    ng = _granules(n)
    pats = {"none": [], "all": list(range(ng)), "alternating": list(range(0, ng, 2)), "last": [ng - 1],
            "random": torch.nonzero(torch.rand(ng, generator=torch.Generator().manual_seed(7)) < 0.5).flatten().tolist()}
    if ng > 16:          # the seam between two 1024-float workgroup iterations
        pats.update({"granule15": [15], "granule16": [16]})
    return pats


def _bits_and_mask(granules, n, dev):
    from drakegpt_amd import ops
    bits = ops.new_no_decay_bits([(64 * G, min(64 * G + 64, n)) for G in granules], n, dev)
    flags = torch.zeros(_granules(n), dtype=torch.bool)
    flags[granules] = True
    return bits, flags.repeat_interleave(64)[:n]


def _stitch(decayed, plain, mask):
    """elements of a masked granule from the weight_decay = 0 run, every other element from the decayed run"""
    assert torch.equal(decayed["m"], plain["m"]) and torch.equal(decayed["v"], plain["v"])
    out = dict(decayed)
    out["p"] = torch.where(mask, plain["p"], decayed["p"])
    out["shadow"] = torch.where(mask, plain["shadow"], decayed["shadow"])
    return out


@pytest.mark.parametrize("n,pattern", [(n, k) for n in SIZES for k in _patterns(n)])
def test_bitmap_per_granule(dev, base, n, pattern):
    granules = _patterns(n)[pattern]
    bits, mask = _bits_and_mask(granules, n, dev)
    decayed = _run(base, n, dev, "old", step=2, advance=True)
    plain = _run(base, n, dev, "old", step=2, hyper=HYPER[:4] + [0.0], advance=True)
    assert (decayed["p"] != plain["p"]).float().mean().item() > 0.99          # the decay is visible in (nearly) every element
    got = _run(base, n, dev, "sched", step=2, bits=bits, advance=True)
    _assert_same_bits(got, _stitch(decayed, plain, mask), pattern)


@pytest.mark.parametrize("n", SIZES)
def test_table_bitmap_and_clip_together(dev, base, n):
    granules = _patterns(n)["random"]
    bits, mask = _bits_and_mask(granules, n, dev)
    table = torch.tensor([7e-4, 1e-3, 2.5e-4], dtype=torch.float32, device=dev)
    lr = float(table[2])
    decayed = _run(base, n, dev, "old", step=9, hyper=[lr] + HYPER[1:], clip=0.37, advance=True)
    plain = _run(base, n, dev, "old", step=9, hyper=[lr] + HYPER[1:4] + [0.0], clip=0.37, advance=True)
    got = _run(base, n, dev, "sched", step=9, hyper=[123.0] + HYPER[1:], clip=0.37, table=table, bits=bits, advance=True)
    _assert_same_bits(got, _stitch(decayed, plain, mask), "table + bitmap + clip")
    # the same through the wrapper
    from drakegpt_amd import ops
    p, g, m, v = (t.clone() for t in base[n])
    state = ops.new_rng_state(123, dev, 9)
    shadow = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    ops.adamw_step(p, g, m, v, torch.tensor([123.0] + HYPER[1:], device=dev), state, 0.5, shadow_bf16=shadow, n=n, advance=True,
                   clip=torch.tensor([0.37], device=dev), lr_table=table, no_decay_bits=bits)
    torch.cuda.synchronize()
    _assert_same_bits({"p": p.cpu(), "m": m.cpu(), "v": v.cpu(), "shadow": shadow.cpu(), "state": state.cpu()}, got, "ops.adamw_step")


def test_argument_checks(dev, base):
    from drakegpt_amd import ops
    n = 67
    p, g, m, v = (t.clone() for t in base[n])
    hy = torch.tensor(HYPER, device=dev)
    state = ops.new_rng_state(1, dev, 0)
    table = torch.tensor([1e-3, 2e-3], device=dev)

    def call(tab, length, pp=p):
        return ops.lib.dg_adamw_step_sched(ops._p(pp), ops._p(g), ops._p(m), ops._p(v), n, ops._p(hy), ops._p(state), 1.0, None, tab, length,
                                           None, None, 0, ops._stream())
    err_arg = ops.lib.dg_adamw_step(None, ops._p(g), ops._p(m), ops._p(v), n, ops._p(hy), ops._p(state), 1.0, None, 0, ops._stream())
    assert err_arg != 0
    assert call(None, 2) == err_arg and call(ops._p(table), 0) == err_arg and call(ops._p(table), -1) == err_arg
    assert call(None, 0) == 0 and call(ops._p(table), 2) == 0
    err_align = ops.lib.dg_adamw_step(p.data_ptr() + 4, ops._p(g), ops._p(m), ops._p(v), 8, ops._p(hy), ops._p(state), 1.0, None, 0, ops._stream())
    assert err_align not in (0, err_arg)
    assert ops.lib.dg_adamw_step_sched(p.data_ptr() + 4, ops._p(g), ops._p(m), ops._p(v), 8, ops._p(hy), ops._p(state), 1.0, None,
                                       ops._p(table), 2, None, None, 0, ops._stream()) == err_align
    torch.cuda.synchronize()
    # the wrapper checks what the kernel would index
    bits = ops.new_no_decay_bits([], n, dev)
    with pytest.raises(ValueError, match="no_decay_bits needs"):
        ops.adamw_step(*base[N_BIG], hy, state, n=64 * 33, no_decay_bits=bits)       # (refused on the host: nothing is launched)
    with pytest.raises(ValueError, match="does not fit"):
        ops.adamw_step(p, g, m, v, hy, state, n=n + 1, lr_table=table)
    with pytest.raises(ValueError, match="lr_table"):
        ops.adamw_step(p, g, m, v, hy, state, lr_table=table[:0])
    with pytest.raises(TypeError, match="no_decay_bits"):
        ops.adamw_step(p, g, m, v, hy, state, no_decay_bits=bits.float())


# ------------------------------------------------------------------------------------------------ engine
@pytest.fixture(scope="module")
def fix(golden_dir):
    return torch.load(os.path.join(golden_dir, "traj5_TransformerLM.pt"), weights_only=True)


def _tiny(dev, fix, B, **kw):
    import drakegpt_amd as D
    from drakegpt_amd.engine import TrainEngine
    m = D.TransformerLM(V, 32, 8, 4, 3, 0.0)
    m.load_state_dict(fix["init"])
    m = m.to(dev).train()
    kw.setdefault("lr", 1e-3)
    return m, TrainEngine(m, B, 8, betas=BETAS, **kw)


def _one_sequence_batch(i, B, dev):
    """every row the same 8 distinct tokens (see the module docstring): another sequence for every i"""
    row = torch.randperm(V, generator=torch.Generator().manual_seed(100 + i))[:9]
    return row[:8].repeat(B, 1).to(dev), row[1:9].repeat(B, 1).to(dev)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("accum", [1, 2])
def test_engine_schedule_equals_set_lr_before_every_step(dev, fix, graph, accum):
    """A looks its rate up on the device; B is told the same fp32 value by the host before every optimizer step.  With
    accum_steps = 2 the table advances per optimizer step: 10 micro-batches consume 5 entries."""
    from drakegpt_amd import schedules as SCH
    values = SCH.warmup_cosine(1e-3, 2, 5)
    table = SCH.as_table(values)
    B = 32 // accum
    kw = dict(use_graph=graph, accum_steps=accum)
    _, A = _tiny(dev, fix, B, lr_schedule=values, **kw)
    _, Bn = _tiny(dev, fix, B, **kw)
    assert A.lr_table is not None and A.no_decay_bits is None and Bn.lr_table is None
    for s in range(5):
        assert A.current_lr() == float(table[s])
        Bn.set_lr(float(table[s]))
        for j in range(accum):
            x, y = _one_sequence_batch(s * accum + j, B, dev)
            for e in (A, Bn):
                e.set_batch(x, y)
                e.micro_step() if accum > 1 else e.step()
        torch.cuda.synchronize()
        for k in ("flat", "m_", "v_"):
            assert np.array_equal(_bits(getattr(A, k)), _bits(getattr(Bn, k))), (s, k)
    assert A.step_count() == Bn.step_count() == 5 and A.micro_step_count() == 5 * accum
    assert A.current_lr() == float(table[4]) == 0.0                # past the end the last entry holds
    assert len({float(x) for x in table}) >= 3                     # (the steps did run at different rates)


def test_engine_with_groups_against_the_oracle(dev, fix):
    """weight_decay 0.1, biases and LayerNorm parameters out of it, the schedule above: the oracle side is two AdamWState objects
    (the second with weight_decay 0) whose lr is set per step.  The bound on the weights is the one of
    test_gpu_engine.py::test_five_step_trajectory_matches_reference (2e-5); the peak rate is that test's rate, so no update is
    larger.  It still sees a wrong bitmap: a LayerNorm weight of 1.0 that is decayed by mistake moves by lr * wd per step."""
    from drakegpt_amd import checkpoint as CK
    from drakegpt_amd import schedules as SCH
    from oracle import drake_ref as R
    bound, wd, kinds, steps = 2e-5, 0.1, ("bias", "layernorm"), 3
    table = SCH.as_table(SCH.warmup_cosine(1e-3, 2, 5))
    sd = {k: v.clone() for k, v in fix["init"].items()}
    keys = R.trainable_keys("TransformerLM", sd)
    dec, nod = CK.split_param_names(keys, 4, 8, kinds)
    ln = [k for k in nod if ".ln" in k and k.endswith(".weight")]
    assert len(ln) == 6 and len(dec) + len(nod) == len(keys)
    margin = min(float(sd[k].abs().min()) for k in ln) * float(table[:steps].sum()) * wd
    print(f"a LayerNorm weight decayed by mistake would move by {margin:.2e}, the bound is {bound:.0e}")
    assert margin > 5 * bound and min(float(sd[k].abs().min()) for k in ln) * float(table[:steps].max()) * wd > 4 * bound
    m, eng = _tiny(dev, fix, 32, weight_decay=wd, no_decay=kinds, lr_schedule=table, use_graph=True)
    assert eng.no_decay == kinds and eng.no_decay_bits is not None
    opt_d = R.AdamWState(dec, 1e-3, BETAS, weight_decay=wd)
    opt_n = R.AdamWState(nod, 1e-3, BETAS, weight_decay=0.0)
    for s in range(steps):
        x, y = fix["x"][s], fix["y"][s]
        eng.set_batch(x.to(dev), y.to(dev))
        loss = eng.step().item()
        _, lref, gr = R.loss_and_grads("TransformerLM", sd, x, y)
        opt_d.lr = opt_n.lr = float(table[s])
        opt_d.step(sd, {k: gr[k] for k in dec})
        opt_n.step(sd, {k: gr[k] for k in nod})
        cur = m.state_dict()
        worst = max((cur[k].cpu() - sd[k]).abs().max().item() for k in keys)
        print(f"step {s}: lr {float(table[s]):.2e}, loss {loss:.6f} (oracle {lref.item():.6f}), weights abs {worst:.3e}")
        assert worst < bound, (s, worst)
    # the export names the two groups as torch would
    osd = eng.optimizer_state_dict()
    assert [g["weight_decay"] for g in osd["param_groups"]] == [wd, 0.0]
    assert osd["param_groups"][0]["lr"] == osd["param_groups"][1]["lr"] == float(table[3]) == eng.current_lr()
    named = dict(m.named_parameters())
    d2, n2 = CK.split_param_names(list(named), 4, 8, kinds)
    topt = torch.optim.AdamW([{"params": [named[k] for k in d2]}, {"params": [named[k] for k in n2], "weight_decay": 0.0}])
    topt.load_state_dict(osd)
    before = {k: getattr(eng, k).clone() for k in ("flat", "m_", "v_")}
    eng.load_optimizer_state_dict(osd)
    assert eng.step_count() == steps and all(torch.equal(getattr(eng, k), t) for k, t in before.items())


# ------------------------------------------------------------------------------------------------ resume (no atomics: bit for bit)
RV, RC, RNH, RT, RB, RP, RL = 80, 384, 6, 256, 8, 0.2, 2


def _scaled(dev, model_seed=42, seed=20240607, **kw):
    import drakegpt_amd as D
    from drakegpt_amd.engine import TrainEngine
    torch.manual_seed(model_seed)
    m = D.TransformerLM(RV, RC, RT, RNH, RL, RP, precision="bf16").to(dev).train()
    eng = TrainEngine(m, RB, RT, lr=3e-4, betas=BETAS, seed=seed, use_graph=True, weight_decay=0.1, **kw)
    assert eng.onehot is not None and eng.grouped_dw            # no atomics in the step: bit-reproducible across engines
    eng.set_corpus(torch.randint(0, RV, (20_000,), generator=torch.Generator().manual_seed(1)).to(dev))
    return m, eng


def test_resume_continues_the_schedule_bit_for_bit(dev, tmp_path):
    from drakegpt_amd import checkpoint as CK
    from drakegpt_amd import schedules as SCH
    values = SCH.warmup_cosine(3e-4, 2, 5, 3e-5)
    kinds = ("bias", "layernorm")
    rows = torch.randint(0, 20_000 - RT - 1, (5, RB), generator=torch.Generator().manual_seed(2))
    _, A = _scaled(dev, lr_schedule=values, no_decay=kinds)
    A.stage_offsets(rows)
    for _ in range(2):
        A.step()
    path = str(tmp_path / "sched.state.pt")
    CK.save_train_state(path, A.state_dict())
    sd = CK.load_train_state(path)                                 # torch.load(..., weights_only=True)
    assert torch.equal(sd["engine"]["lr_table"], SCH.as_table(values)) and sd["engine"]["no_decay"] == ["bias", "layernorm"]
    la = [A.step().item() for _ in range(3)]
    # a fresh engine built with the same arguments (other initial weights, dropout seed and table VALUES: the file's replace them)
    _, Bn = _scaled(dev, model_seed=7, seed=99, lr_schedule=SCH.constant(1e-3, 5), no_decay=kinds)
    table_ptr = Bn.lr_table.data_ptr()
    Bn.load_state_dict(sd)
    assert Bn.lr_table.data_ptr() == table_ptr and torch.equal(Bn.lr_table.cpu(), SCH.as_table(values))
    assert Bn.step_count() == 2 and Bn.current_lr() == float(SCH.as_table(values)[2])
    lb = [Bn.step().item() for _ in range(3)]
    torch.cuda.synchronize()
    assert la == lb, (la, lb)
    for k in ("flat", "m_", "v_", "shadow"):
        assert torch.equal(getattr(A, k), getattr(Bn, k)), k
    assert A.step_count() == Bn.step_count() == 5
    # refusals leave the engine as it was
    for kw, what in ((dict(lr_schedule=SCH.warmup_cosine(3e-4, 2, 6, 3e-5), no_decay=kinds), r"lr_table differs.*5.*6"),
                     (dict(no_decay=kinds), r"lr_table differs.*5.*None"),
                     (dict(lr_schedule=values, no_decay=("bias",)), r"no_decay differs.*\['bias', 'layernorm'\].*\['bias'\]"),
                     (dict(lr_schedule=values), r"no_decay differs.*\['bias', 'layernorm'\].*\[\]")):
        _, Cn = _scaled(dev, model_seed=8, seed=5, **kw)
        before = {k: getattr(Cn, k).clone() for k in ("flat", "m_", "v_", "state", "hyper")}
        tab = None if Cn.lr_table is None else Cn.lr_table.clone()
        with pytest.raises(ValueError, match=what):
            Cn.load_state_dict(sd)
        assert all(torch.equal(getattr(Cn, k), t) for k, t in before.items())
        assert tab is None or torch.equal(Cn.lr_table, tab)
    # a state written by an engine without schedule and groups carries None / []: an engine with them refuses it, one without loads it
    _, Dn = _scaled(dev, model_seed=9, seed=6)
    plain = Dn.state_dict()
    assert plain["engine"]["lr_table"] is None and plain["engine"]["no_decay"] == []
    old = dict(plain, engine={k: v for k, v in plain["engine"].items() if k not in ("lr_table", "no_decay")})      # written before this
    Dn.load_state_dict(old)
    with pytest.raises(ValueError, match="lr_table differs"):
        Bn.load_state_dict(old)


def test_set_lr_and_set_lr_schedule(dev, fix):
    from drakegpt_amd import schedules as SCH
    _, eng = _tiny(dev, fix, 32, lr_schedule=SCH.constant(1e-3, 5), use_graph=True)
    with pytest.raises(RuntimeError, match="schedule"):
        eng.set_lr(5e-4)
    x, y = _one_sequence_batch(0, 32, dev)
    eng.set_batch(x, y)
    eng.step()
    graphs = eng._graphs
    assert graphs is not None
    flat, m_ = eng.flat.clone(), eng.m_.clone()
    eng.set_lr_schedule([0.0] * 5)                                  # lr 0: p * (1 - 0 * wd) - 0 * (...) = p
    assert eng.current_lr() == 0.0
    eng.step()
    torch.cuda.synchronize()
    assert eng._graphs is graphs and torch.equal(eng.flat, flat) and not torch.equal(eng.m_, m_)
    eng.set_lr_schedule(lambda s: 1e-3, 5)
    eng.step()
    torch.cuda.synchronize()
    assert eng._graphs is graphs and not torch.equal(eng.flat, flat) and eng.step_count() == 3
    for bad in ([1e-3] * 4, [1e-3] * 6):
        with pytest.raises(ValueError, match="entries"):
            eng.set_lr_schedule(bad)
    with pytest.raises(ValueError, match="entry 1"):
        eng.set_lr_schedule([1e-3, -1.0, 0, 0, 0])
    _, plain = _tiny(dev, fix, 32)
    with pytest.raises(RuntimeError, match="without a schedule"):
        plain.set_lr_schedule([1e-3])
    assert plain.current_lr() == 1e-3
    plain.set_lr(5e-4)
    assert plain.current_lr() == 5e-4


def test_constructor_refusals(dev, fix):
    for kw, what in ((dict(no_decay=("biases",)), "no_decay"), (dict(no_decay="bias"), "no_decay"), (dict(lr_schedule=[]), "at least one"),
                     (dict(lr_schedule=[1e-3, float("nan")]), "entry 1"), (dict(lr_schedule=lambda s: 1e-3), "schedule_steps"),
                     (dict(schedule_steps=5), "schedule_steps goes with lr_schedule")):
        with pytest.raises(ValueError, match=what):
            _tiny(dev, fix, 32, **kw)
    _, eng = _tiny(dev, fix, 32, lr_schedule=lambda s: 1e-3 * (s + 1), schedule_steps=3, no_decay=["embedding", "bias", "layernorm"])
    assert eng.lr_table.tolist() == torch.tensor([1e-3, 2e-3, 3e-3]).tolist() and eng.no_decay == ("bias", "embedding", "layernorm")
    # the bitmap covers exactly the regions of those kinds, whole granules
    from drakegpt_amd import checkpoint as CK
    words = [w & 0xFFFFFFFF for w in eng.no_decay_bits.cpu().tolist()]
    for key in eng._trained_keys():
        off, shape = eng._region(key)
        for G in range(off // 64, (off + int(np.prod(shape)) + 63) // 64):
            assert (words[G >> 5] >> (G & 31)) & 1 == int(CK.region_no_decay(key, eng.no_decay)), (key, G)


# ------------------------------------------------------------------------------------------------ harness
@pytest.mark.parametrize("model", ["TransformerLM", "BlocksLM"])
def test_train_harness_follows_the_schedule(dev, capsys, model):
    """both training paths report, at every evaluation, the rate of the step that follows it"""
    import json
    from drakegpt_amd import schedules as SCH
    from drakegpt_amd import train
    from drakegpt_amd.config import PARAMS
    train.main(["--model", model, "--iters", "6", "--eval-interval", "2", "--eval-iters", "2", "--precision", "fp32", "--no-save",
                "--sample", "3", "--lr-schedule", "warmup-cosine", "--warmup-steps", "2", "--min-lr", "1e-5", "--no-decay", "bias,layernorm"])
    lines = [json.loads(s) for s in capsys.readouterr().out.splitlines() if s.startswith("{") and '"val_loss"' in s]
    table = SCH.as_table(SCH.warmup_cosine(PARAMS["max_lr"], 2, 6, 1e-5)).tolist()
    assert [ln["step"] for ln in lines] == [2, 4, 6]
    assert [ln["lr"] for ln in lines] == [table[2], table[4], table[5]]
    assert all(np.isfinite(ln["train_loss"]) and np.isfinite(ln["val_loss"]) for ln in lines)


def test_default_engine_makes_the_adamw_call_it_always_made(dev, fix, monkeypatch):
    """tools that stand in for ops.adamw_step with its earlier signature (the benchmark's roofline leg does) keep working: an
    engine with neither argument passes no new keyword"""
    from drakegpt_amd import ops
    real, seen = ops.adamw_step, []

    def earlier(p, g, m, v, hyper, rng_state, grad_scale=1.0, shadow_bf16=None, n=None, advance=False, *, clip=None):
        seen.append(clip is not None)
        return real(p, g, m, v, hyper, rng_state, grad_scale, shadow_bf16, n, advance, clip=clip)
    monkeypatch.setattr(ops, "adamw_step", earlier)
    for kw in ({}, {"max_grad_norm": 1.0}, {"accum_steps": 2}):
        _, eng = _tiny(dev, fix, 16, use_graph=False, **kw)
        x, y = _one_sequence_batch(0, 16, dev)
        for _ in range(eng.accum):
            eng.set_batch(x, y)
            eng.micro_step() if eng.accum > 1 else eng.step()
        assert eng.step_count() == 1
    assert seen == [False, True, False]
