"""CPU: learning-rate tables (drakegpt_amd.schedules), the no-decay bitmap, the two-group optimizer export and the harness flags
--lr-schedule / --warmup-steps / --min-lr / --no-decay.

Schedules are compared with torch's own schedulers at peak 3e-4, min 3e-5, 2000 steps.  torch computes its cosine recursively
and drifts from the closed form by up to 1.9e-14 relative over those steps; the bound is 1e-9 relative: more than 10^4 times
that drift, and 60 times below one fp32 ulp (6e-8), which is all the device table holds.  Past T_max torch's cosine rises again
while the table holds min_lr, so only s < N is compared."""
import math
import warnings

import pytest
import torch

from drakegpt_amd import checkpoint as CK
from drakegpt_amd import schedules as SCH

PEAK, MIN, N, W = 3e-4, 3e-5, 2000, 37
BOUND = 1e-9


def _torch_rates(make_sched, n):
    """the rate each of n optimizer steps runs at under a torch scheduler stepped after every optimizer.step()"""
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=PEAK)
    sched = make_sched(opt)
    out = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for _ in range(n):
            out.append(opt.param_groups[0]["lr"])
            opt.step()
            sched.step()
    return out


def _worst(ours, theirs):
    assert len(ours) == len(theirs)
    return max(abs(a - b) / abs(b) for a, b in zip(ours, theirs))


# ------------------------------------------------------------------------------------------------ schedules
def test_warmup_cosine_against_torch_sequential_lr():
    L = torch.optim.lr_scheduler
    ref = _torch_rates(lambda o: L.SequentialLR(o, [L.LinearLR(o, start_factor=1.0 / W, total_iters=W - 1),
                                                    L.CosineAnnealingLR(o, T_max=N - 1 - W, eta_min=MIN)], milestones=[W]), N)
    e = _worst(SCH.warmup_cosine(PEAK, W, N, MIN), ref)
    print(f"warmup_cosine, warm-up {W}: worst relative difference {e:.2e}")
    assert e < BOUND


def test_cosine_without_warmup_against_torch():
    ref = _torch_rates(lambda o: torch.optim.lr_scheduler.CosineAnnealingLR(o, T_max=N - 1, eta_min=MIN), N)
    e = _worst(SCH.warmup_cosine(PEAK, 0, N, MIN), ref)
    print(f"warmup_cosine, warm-up 0: worst relative difference {e:.2e}")
    assert e < BOUND


def test_warmup_alone_against_torch_linear_lr():
    ref = _torch_rates(lambda o: torch.optim.lr_scheduler.LinearLR(o, start_factor=1.0 / W, total_iters=W - 1), W)
    for form in (SCH.warmup_cosine, SCH.warmup_linear):
        e = _worst(form(PEAK, W, N, MIN)[:W], ref)
        print(f"{form.__name__}: warm-up part, worst relative difference {e:.2e}")
        assert e < BOUND


def test_cyclic_is_the_harness_formula_exactly():
    from drakegpt_amd import train
    for up, total in ((5, 40), (3, 7), (1, 4)):
        got = SCH.cyclic(2.6e-4, 2.6e-3, up, total)
        assert got == [train.cyclic_lr(s, 2.6e-4, 2.6e-3, up) for s in range(total)]
    assert SCH.cyclic(1e-4, 1e-3, 5, 11)[0] == 1e-4 and SCH.cyclic(1e-4, 1e-3, 5, 11)[5] == pytest.approx(1e-3, rel=1e-15)


def test_end_points_and_the_clamp_rule():
    for form in (SCH.warmup_cosine, SCH.warmup_linear):
        t = form(PEAK, W, N, MIN)
        assert len(t) == N
        assert t[0] == PEAK * 1 / W and t[W - 1] == PEAK           # (s + 1) / warmup: the last warm-up step runs at the peak
        assert t[W] == PEAK and t[-1] == MIN                       # the decay starts at the peak and ends on min_lr exactly
        assert all(a >= b for a, b in zip(t[W:], t[W + 1:]))       # and never rises
        assert max(t) == PEAK and min(t[W:]) == MIN
        assert form(PEAK, 0, 2)[0] == PEAK and form(PEAK, 0, 2)[1] == 0.0          # the shortest: total = warmup + 2
    lin = SCH.warmup_linear(PEAK, W, N, MIN)
    mid = W + (N - 1 - W) // 2
    assert lin[mid] == pytest.approx(PEAK + (MIN - PEAK) * (mid - W) / (N - 1 - W), rel=1e-15)
    cos = SCH.warmup_cosine(1.0, 0, 3)
    assert cos[0] == 1.0 and cos[1] == pytest.approx(0.5, abs=1e-16) and cos[2] == 0.0
    assert SCH.constant(2e-3) == [2e-3] and SCH.constant(2e-3, 4) == [2e-3] * 4
    # the clamp the kernel and TrainEngine.current_lr() apply: past the end the last entry holds
    table = SCH.as_table(SCH.warmup_cosine(PEAK, 2, 5, MIN))
    assert table.dtype == torch.float32 and table.device.type == "cpu" and tuple(table.shape) == (5,)
    for s in (4, 5, 1004):
        assert float(table[min(s, table.numel() - 1)]) == float(torch.tensor(MIN, dtype=torch.float32))


@pytest.mark.parametrize("kw", [dict(warmup=-1, total=10), dict(warmup=2, total=3), dict(warmup=0, total=1), dict(warmup=2.0, total=10),
                                dict(warmup=True, total=10), dict(warmup=1, total=10.0)])
def test_warmup_and_total_are_checked(kw):
    for form in (SCH.warmup_cosine, SCH.warmup_linear):
        with pytest.raises(ValueError, match="warmup|total"):
            form(PEAK, kw["warmup"], kw["total"])


def test_rates_are_checked():
    for bad in (-1e-3, float("nan"), float("inf"), "fast", None):
        with pytest.raises(ValueError, match="peak"):
            SCH.warmup_cosine(bad, 2, 10)
        with pytest.raises(ValueError, match="min_lr"):
            SCH.warmup_linear(PEAK, 2, 10, bad)
        with pytest.raises(ValueError, match="lr"):
            SCH.constant(bad)
    with pytest.raises(ValueError, match="N"):
        SCH.constant(1e-3, 0)
    with pytest.raises(ValueError, match="step_size_up"):
        SCH.cyclic(1e-4, 1e-3, 0, 10)


def test_as_table_validation():
    assert SCH.as_table([1e-3, 5e-4]).tolist() == torch.tensor([1e-3, 5e-4], dtype=torch.float32).tolist()
    assert torch.equal(SCH.as_table(torch.tensor([1e-3, 0.0], dtype=torch.float64)), torch.tensor([1e-3, 0.0]))
    assert torch.equal(SCH.as_table(lambda s: 1e-3 / (s + 1), 3), torch.tensor([1e-3, 5e-4, 1e-3 / 3], dtype=torch.float64).float())
    assert torch.equal(SCH.as_table((x for x in (1.0, 2.0))), torch.tensor([1.0, 2.0]))
    assert SCH.as_table([1e-3, 2e-3], 2).numel() == 2
    for bad, what in (([], "at least one"), ([1e-3, float("nan")], "entry 1"), ([float("inf")], "entry 0"), ([-1e-9], "entry 0"),
                      ([1e-3, "x"], "entry 1"), ([1e39], "fp32"), (torch.zeros(2, 2), "1-D"), (3.0, "sequence"), (torch.zeros(0), "at least one")):
        with pytest.raises(ValueError, match=what):
            SCH.as_table(bad)
    with pytest.raises(ValueError, match="schedule_steps"):
        SCH.as_table(lambda s: 1e-3)                             # a callable has no length of its own
    with pytest.raises(ValueError, match="schedule_steps"):
        SCH.as_table(lambda s: 1e-3, 0)
    with pytest.raises(ValueError, match="3.*2 entries"):
        SCH.as_table([1e-3, 2e-3], 3)
    with pytest.raises(ValueError, match="step word"):
        SCH.as_table(lambda s: 1e-3, (1 << 32) + 1)              # refused before anything is evaluated


# ------------------------------------------------------------------------------------------------ bitmap
def _bits_by_hand(ranges, n):
    """bit (G & 31) of word (G >> 5) covers elements [64 G, 64 G + 64): element by element"""
    ng = (n + 63) // 64
    words = [0] * ((ng + 31) // 32)
    for i in range(n):
        if any(lo <= i < hi for lo, hi in ranges):
            words[(i // 64) >> 5] |= 1 << ((i // 64) & 31)
    return words


@pytest.mark.parametrize("ranges,n", [([], 64), ([(0, 64)], 64), ([(64, 128), (192, 200)], 200), ([(0, 131)], 131),
                                       ([(64 * 31, 64 * 33), (64 * 40, 64 * 41)], 64 * 70 + 5), ([(64 * 70, 64 * 70 + 5)], 64 * 70 + 5),
                                       ([(128, 128)], 300), ([(0, 64 * 64)], 64 * 64)])
def test_no_decay_bits_against_a_plain_restatement(ranges, n):
    from drakegpt_amd import ops
    bits = ops.new_no_decay_bits(ranges, n, "cpu")
    assert bits.dtype == torch.int32 and bits.numel() == ops.no_decay_words(n) == ((n + 63) // 64 + 31) // 32
    assert [w & 0xFFFFFFFF for w in bits.tolist()] == _bits_by_hand(ranges, n)


def test_no_decay_bits_refuses_half_a_granule():
    from drakegpt_amd import ops
    for bad in ([(32, 64)], [(0, 32)], [(64, 100)], [(0, 201)], [(-64, 0)], [(128, 64)]):
        with pytest.raises(ValueError, match="range"):
            ops.new_no_decay_bits(bad, 200, "cpu")
    ops.new_no_decay_bits([(128, 200)], 200, "cpu")              # ... but a range may end at n
    for bad_n in (0, -5, 64.0, True):
        with pytest.raises(ValueError, match="n must be"):
            ops.new_no_decay_bits([], bad_n, "cpu")


# ------------------------------------------------------------------------------------------------ decay groups
V, C, CTX, NH, L = 80, 32, 8, 4, 3
H = C // NH


def _tiny():
    import drakegpt_amd as D
    torch.manual_seed(0)
    return D.TransformerLM(V, C, CTX, NH, L, 0.1)


def _region_shapes():
    shp = {"lm.w": (V, C), "lm.b": (V,), "tok": (V, C), "pos": (CTX, C)}
    for l in range(L):
        shp.update({f"{l}.wqkv": (3 * C, C), f"{l}.wproj": (C, C), f"{l}.w1": (4 * C, C), f"{l}.w2": (C, 4 * C), f"{l}.bproj": (C,),
                    f"{l}.b1": (4 * C,), f"{l}.b2": (C,), f"{l}.ln1w": (C,), f"{l}.ln1b": (C,), f"{l}.ln2w": (C,), f"{l}.ln2b": (C,)})
    return shp


def test_no_decay_kinds():
    assert CK.check_no_decay(()) == () and CK.check_no_decay(["layernorm", "bias", "bias"]) == ("bias", "layernorm")
    assert CK.check_no_decay({"embedding"}) == ("embedding",)
    for bad in (["biases"], "bias", [1], 7, ["bias", None]):
        with pytest.raises(ValueError, match="no_decay"):
            CK.check_no_decay(bad)
    want = {"bias": {"lm.b"} | {f"{l}.{k}" for l in range(L) for k in ("bproj", "b1", "b2")},
            "layernorm": {f"{l}.{k}" for l in range(L) for k in ("ln1w", "ln1b", "ln2w", "ln2b")}, "embedding": {"tok", "pos"}}
    for kind, keys in want.items():
        assert {k for k in _region_shapes() if CK.region_no_decay(k, (kind,))} == keys
    assert CK.region_no_decay("lnf.w", ("layernorm",)) and not CK.region_no_decay("lm.w", ("bias", "layernorm", "embedding"))
    # by name, against the module types of the model itself
    model = _tiny()
    names = [n for n, _ in model.named_parameters()]
    dec, nod = CK.split_param_names(names, NH, H, ("bias", "layernorm", "embedding"))
    by_type = set()
    for mn, mod in model.named_modules():
        if isinstance(mod, (torch.nn.LayerNorm, torch.nn.Embedding)):
            by_type |= {f"{mn}.{pn}" for pn, _ in mod.named_parameters(recurse=False)}
        elif isinstance(mod, torch.nn.Linear) and mod.bias is not None:
            by_type.add(f"{mn}.bias")
    assert set(nod) == by_type and dec + nod != names and sorted(dec + nod) == sorted(names)
    assert [n for n in names if n in set(dec)] == dec and [n for n in names if n in set(nod)] == nod          # model order inside a group
    assert CK.split_param_names(names, NH, H, ()) == (names, [])


def test_two_group_optimizer_state_loads_into_torch_adamw_and_back():
    model = _tiny()
    named = dict(model.named_parameters())
    names = list(named)
    kinds = ("bias", "layernorm")
    g = torch.Generator().manual_seed(21)
    regions = {k: (torch.randn(s, generator=g), torch.rand(s, generator=g)) for k, s in _region_shapes().items()}
    sd = CK.optimizer_state_from_regions(names, regions, NH, H, step=7, lr=2e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.1,
                                         no_decay=kinds)
    dec, nod = CK.split_param_names(names, NH, H, kinds)
    opt = torch.optim.AdamW([{"params": [named[n] for n in dec]}, {"params": [named[n] for n in nod], "weight_decay": 0.0}])
    opt.load_state_dict(sd)
    assert [set(gr) for gr in opt.state_dict()["param_groups"]] == [set(gr) for gr in sd["param_groups"]]
    g0, g1 = opt.param_groups
    assert (g0["lr"], tuple(g0["betas"]), g0["eps"], g0["weight_decay"]) == (2e-3, (0.9, 0.95), 1e-8, 0.1)
    assert (g1["lr"], tuple(g1["betas"]), g1["eps"], g1["weight_decay"]) == (2e-3, (0.9, 0.95), 1e-8, 0.0)
    assert len(g0["params"]) == len(dec) and len(g1["params"]) == len(nod)
    for n in names:
        if n.startswith("ln_f."):
            assert named[n] not in opt.state
            continue
        key, rows = CK.param_region(n, NH, H)
        m, v = regions[key]
        if rows is not None:
            m, v = m[rows[0]:rows[1]], v[rows[0]:rows[1]]
        st = opt.state[named[n]]
        assert float(st["step"]) == 7.0 and torch.equal(st["exp_avg"], m) and torch.equal(st["exp_avg_sq"], v), n
    for src in (sd, opt.state_dict()):
        back, step, hyper = CK.regions_from_optimizer_state(src, names, NH, H, no_decay=kinds)
        assert step == 7 and hyper == {"lr": 2e-3, "betas": (0.9, 0.95), "eps": 1e-8, "weight_decay": 0.1}
        assert set(back) == set(regions)
        for k in regions:
            assert torch.equal(back[k][0], regions[k][0]) and torch.equal(back[k][1], regions[k][1]), k
    # one side with groups, the other without: refused, naming what was expected
    with pytest.raises(ValueError, match="one parameter group, found 2"):
        CK.regions_from_optimizer_state(sd, names, NH, H)
    one = CK.optimizer_state_from_regions(names, regions, NH, H, 7, 2e-3, (0.9, 0.95), 1e-8, 0.1)
    with pytest.raises(ValueError, match="two parameter groups, found 1"):
        CK.regions_from_optimizer_state(one, names, NH, H, no_decay=kinds)
    with pytest.raises(ValueError, match="splits the model"):
        CK.regions_from_optimizer_state(sd, names, NH, H, no_decay=("bias",))
    sd["param_groups"][1]["weight_decay"] = 0.01
    with pytest.raises(ValueError, match="second group has weight_decay"):
        CK.regions_from_optimizer_state(sd, names, NH, H, no_decay=kinds)
    # without groups the export is what it was: one group over the model's parameters in order
    assert [gr["params"] for gr in one["param_groups"]] == [list(range(len(names)))]


# ------------------------------------------------------------------------------------------------ harness flags
def test_parser_flags_for_schedules_and_groups(capsys):
    from drakegpt_amd import train
    a = train.parse_args([])
    assert (a.lr_schedule, a.warmup_steps, a.min_lr, a.no_decay) == ("reference", 0, 0.0, ())
    assert train.lr_values(a, 1e-4, 1e-3) is None
    a = train.parse_args(["--lr-schedule", "warmup-cosine", "--warmup-steps", "10", "--min-lr", "1e-5", "--iters", "100",
                          "--no-decay", "layernorm,bias"])
    assert (a.lr_schedule, a.warmup_steps, a.min_lr, a.no_decay) == ("warmup-cosine", 10, 1e-5, ("bias", "layernorm"))
    assert train.lr_values(a, 1e-4, 1e-3) == SCH.warmup_cosine(1e-3, 10, 100, 1e-5)          # the peak is the preset's max_lr
    a = train.parse_args(["--lr-schedule", "warmup-linear", "--warmup-steps", "3", "--iters", "9"])
    assert train.lr_values(a, 1e-4, 1e-3) == SCH.warmup_linear(1e-3, 3, 9, 0.0)
    a = train.parse_args(["--lr-schedule", "cyclic", "--iters", "12"])
    assert train.lr_values(a, 1e-4, 1e-3) == [train.cyclic_lr(s, 1e-4, 1e-3) for s in range(12)]
    a = train.parse_args(["--lr-schedule", "constant", "--iters", "12", "--no-decay", "embedding"])
    assert train.lr_values(a, 1e-4, 1e-3) == [1e-4] * 12 and a.no_decay == ("embedding",)
    for bad, word in ((["--lr-schedule", "exponential"], "--lr-schedule"), (["--no-decay", "bias,norms"], "--no-decay"),
                      (["--lr-schedule", "warmup-cosine", "--warmup-steps", "10", "--iters", "11"], "--lr-schedule"),
                      (["--lr-schedule", "warmup-linear", "--warmup-steps", "-1"], "--lr-schedule"),
                      (["--lr-schedule", "warmup-cosine", "--min-lr", "-1"], "--lr-schedule"),
                      (["--warmup-steps", "10"], "--warmup-steps"), (["--lr-schedule", "cyclic", "--min-lr", "1e-5"], "--min-lr")):
        with pytest.raises(SystemExit) as ei:
            train.parse_args(bad)
        assert ei.value.code == 2
        assert word in capsys.readouterr().err


def test_resume_must_repeat_the_schedule_and_old_files_resume_with_default_flags(tmp_path):
    from drakegpt_amd import train
    path = str(tmp_path / "s.pt")

    def write(mm):
        CK.save_train_state(path, {"format": CK.FORMAT, "version": CK.VERSION, "iteration": 4, "sched_steps": 1,
                                   "rng_state": torch.get_rng_state(), "args": mm, "engine": None, "model": {}, "optimizer": {}})
    base = ["--model", "BlocksLM", "--precision", "fp32"]
    default = train.run_args(train.parse_args(base), 1, 1)
    old = {k: default[k] for k in ("model", "preset", "scale", "precision", "accum_steps", "world_size")}       # what was written before
    assert set(default) - set(old) == set(train.RUN_ARG_DEFAULTS) and all(default[k] == v for k, v in train.RUN_ARG_DEFAULTS.items())
    write(old)
    assert train.load_run_state(path, default)["iteration"] == 4
    sched = train.run_args(train.parse_args(base + ["--lr-schedule", "warmup-cosine", "--warmup-steps", "5", "--iters", "50",
                                                    "--min-lr", "1e-5", "--no-decay", "bias"]), 1, 1)
    for field in ("lr_schedule", "warmup_steps", "min_lr", "no_decay", "schedule_iters"):
        with pytest.raises(SystemExit, match=field):
            train.load_run_state(path, dict(default, **{field: sched[field]}))           # the old file ran without it
    write(sched)
    assert train.load_run_state(path, sched)["iteration"] == 4
    for field, other in (("lr_schedule", "warmup-linear"), ("warmup_steps", 6), ("min_lr", 0.0), ("no_decay", ["bias", "layernorm"]),
                         ("schedule_iters", 60)):
        with pytest.raises(SystemExit, match=field):
            train.load_run_state(path, dict(sched, **{field: other}))
    assert math.isclose(sched["min_lr"], 1e-5)


def test_no_decay_groups_of_the_autograd_path():
    from drakegpt_amd import train
    model = _tiny()
    groups = train.no_decay_groups(model, ("bias", "layernorm"))
    names = {id(p): n for n, p in model.named_parameters()}
    dec, nod = CK.split_param_names(list(names.values()), NH, H, ("bias", "layernorm"))
    assert [names[id(p)] for p in groups[0]["params"]] == dec and [names[id(p)] for p in groups[1]["params"]] == nod
    assert "weight_decay" not in groups[0] and groups[1]["weight_decay"] == 0.0
