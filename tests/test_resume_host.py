"""CPU: training-state files (drakegpt_amd.checkpoint), the optimizer-format mapping behind TrainEngine.optimizer_state_dict()
and the harness flags --save-every / --state-path / --resume.  No GPU: the mapping is a pure function of names and shapes."""
import os

import pytest
import torch

from drakegpt_amd import checkpoint as CK


def _state():
    g = torch.Generator().manual_seed(3)
    return {"format": CK.FORMAT, "version": CK.VERSION,
            "model": {"w": torch.randn(4, 3, generator=g)},
            "optimizer": {"state": {0: {"step": torch.tensor(2.0), "exp_avg": torch.randn(4, 3, generator=g)}},
                          "param_groups": [{"lr": 1e-3, "betas": (0.9, 0.95), "params": [0], "fused": None, "amsgrad": False}]},
            "engine": {"seed": 42, "offsets": torch.randint(0, 100, (2, 8), generator=g), "offsets_left": None, "fp8_sites": {}},
            "meta": {"precision": "bf16", "dropout": 0.2, "batch_size": 8}}


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


def test_round_trip_through_a_file(tmp_path):
    st = _state()
    path = str(tmp_path / "sub" / "run.state.pt")           # the directory is made on demand
    CK.save_train_state(path, st)
    back = CK.load_train_state(path)
    assert _same(st, back)
    assert os.listdir(os.path.dirname(path)) == ["run.state.pt"]


def test_failed_write_keeps_the_old_file_and_leaves_no_temporary(tmp_path, monkeypatch):
    path = str(tmp_path / "run.state.pt")
    CK.save_train_state(path, _state())
    before = open(path, "rb").read()

    def boom(obj, f, *a, **kw):
        with open(f, "wb") as fh:                           # a write that dies half way
            fh.write(b"partial")
        raise OSError("disk full")
    monkeypatch.setattr(torch, "save", boom)
    st = _state()
    st["model"]["w"] += 1.0
    with pytest.raises(OSError, match="disk full"):
        CK.save_train_state(path, st)
    assert open(path, "rb").read() == before
    assert os.listdir(str(tmp_path)) == ["run.state.pt"]


@pytest.mark.parametrize("field,value", [("version", CK.VERSION + 1), ("format", "somebody.else")])
def test_wrong_format_or_version_is_refused(tmp_path, field, value):
    st = _state()
    st[field] = value
    path = str(tmp_path / "x.pt")
    with pytest.raises(ValueError, match=field):
        CK.save_train_state(path, st)
    torch.save(st, path)
    with pytest.raises(ValueError, match=field):
        CK.load_train_state(path)
    del st[field]
    torch.save(st, path)
    with pytest.raises(ValueError, match=field):
        CK.load_train_state(path)


def test_check_compat_names_the_field_and_both_values():
    own = {"precision": "bf16", "batch_size": 8, "dropout": 0.2}
    CK.check_compat(dict(own, extra=1), own)
    with pytest.raises(ValueError, match=r"meta\.batch_size.*16.*8"):
        CK.check_compat(dict(own, batch_size=16), own)
    with pytest.raises(ValueError, match=r"meta\.precision.*'fp8'.*'bf16'"):
        CK.check_compat(dict(own, precision="fp8"), own)
    with pytest.raises(ValueError, match=r"missing key meta\.dropout"):
        CK.check_compat({"precision": "bf16", "batch_size": 8}, own)
    with pytest.raises(ValueError, match=r"meta\.batch_size"):
        CK.check_compat(dict(own, batch_size=8.0), own)          # a float is not the int that was written


# ------------------------------------------------------------------------------------------------ optimizer mapping
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


def test_names_and_regions_are_inverse_and_cover_the_model():
    model = _tiny()
    names = [n for n, _ in model.named_parameters()]
    shapes = _region_shapes()
    seen = {}
    for n, p in model.named_parameters():
        key, rows = CK.param_region(n, NH, H)
        if key in CK.UNTRAINED:
            assert n.startswith("ln_f.")
            continue
        full = shapes[key]
        assert tuple(p.shape) == (full if rows is None else (rows[1] - rows[0],) + full[1:]), n
        assert (n, rows) in CK.region_params(key, NH, H)
        seen.setdefault(key, []).append(rows)
    assert set(seen) == set(shapes)
    for key, rows in seen.items():                   # the heads tile the packed QKV rows exactly once
        if rows[0] is not None:
            assert sorted(rows) == [(k * H, (k + 1) * H) for k in range(3 * NH)]
        assert len(CK.region_params(key, NH, H)) == len(rows)
    assert CK.param_region("blocks.1.sa_head.heads.2.query.weight", NH, H) == ("1.wqkv", (2 * H, 3 * H))
    assert CK.param_region("blocks.1.sa_head.heads.2.key.weight", NH, H) == ("1.wqkv", ((NH + 2) * H, (NH + 3) * H))
    assert CK.param_region("blocks.1.sa_head.heads.2.value.weight", NH, H) == ("1.wqkv", ((2 * NH + 2) * H, (2 * NH + 3) * H))
    for bad in ("blocks.0.sa_head.heads.4.key.weight", "blocks.0.nothing", "nothing"):
        with pytest.raises(KeyError):
            CK.param_region(bad, NH, H)
    assert len(names) == len(set(names))


def test_optimizer_state_in_torch_format_and_back():
    model = _tiny()
    names = [n for n, _ in model.named_parameters()]
    g = torch.Generator().manual_seed(11)
    regions = {k: (torch.randn(s, generator=g), torch.rand(s, generator=g)) for k, s in _region_shapes().items()}
    sd = CK.optimizer_state_from_regions(names, regions, NH, H, step=7, lr=2e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=1e-2)
    opt = torch.optim.AdamW(model.parameters())
    opt.load_state_dict(sd)                                  # torch accepts it ...
    assert set(opt.state_dict()["param_groups"][0]) == set(sd["param_groups"][0])          # ... and it has torch's own group keys
    grp = opt.param_groups[0]
    assert (grp["lr"], tuple(grp["betas"]), grp["eps"], grp["weight_decay"]) == (2e-3, (0.9, 0.95), 1e-8, 1e-2)
    params = list(model.parameters())
    for i, (n, p) in enumerate(model.named_parameters()):
        if n.startswith("ln_f."):
            assert i not in sd["state"] and p not in opt.state
            continue
        st = opt.state[params[i]]
        key, rows = CK.param_region(n, NH, H)
        m, v = regions[key]
        if rows is not None:
            m, v = m[rows[0]:rows[1]], v[rows[0]:rows[1]]
        assert float(st["step"]) == 7.0
        assert st["exp_avg"].shape == p.shape and torch.equal(st["exp_avg"], m) and torch.equal(st["exp_avg_sq"], v), n
    # the per-head slices by hand: head 1 of layer 2, the layout engine._alloc_and_adopt gives the packed operand
    m = regions["2.wqkv"][0]
    idx = {n: i for i, n in enumerate(names)}
    assert torch.equal(sd["state"][idx["blocks.2.sa_head.heads.1.query.weight"]]["exp_avg"], m[1 * H:2 * H])
    assert torch.equal(sd["state"][idx["blocks.2.sa_head.heads.1.key.weight"]]["exp_avg"], m[(NH + 1) * H:(NH + 2) * H])
    assert torch.equal(sd["state"][idx["blocks.2.sa_head.heads.1.value.weight"]]["exp_avg"], m[(2 * NH + 1) * H:(2 * NH + 2) * H])
    # the inverse, also on what torch itself writes after loading
    for src in (sd, opt.state_dict()):
        back, step, hyper = CK.regions_from_optimizer_state(src, names, NH, H)
        assert step == 7 and hyper == {"lr": 2e-3, "betas": (0.9, 0.95), "eps": 1e-8, "weight_decay": 1e-2}
        assert set(back) == set(regions)
        for k in regions:
            assert torch.equal(back[k][0], regions[k][0]) and torch.equal(back[k][1], regions[k][1]), k


def test_optimizer_state_refusals():
    model = _tiny()
    names = [n for n, _ in model.named_parameters()]
    g = torch.Generator().manual_seed(12)
    regions = {k: (torch.randn(s, generator=g), torch.rand(s, generator=g)) for k, s in _region_shapes().items()}
    sd = CK.optimizer_state_from_regions(names, regions, NH, H, 3, 1e-3, (0.9, 0.95), 1e-8, 1e-2)
    sd["state"][0]["step"] = torch.tensor(4.0)
    with pytest.raises(ValueError, match=r"step count.*\[3, 4\]"):
        CK.regions_from_optimizer_state(sd, names, NH, H)
    sd = CK.optimizer_state_from_regions(names, regions, NH, H, 3, 1e-3, (0.9, 0.95), 1e-8, 1e-2)
    del sd["state"][names.index("blocks.0.sa_head.heads.0.key.weight")]
    with pytest.raises(ValueError, match="0.wqkv"):
        CK.regions_from_optimizer_state(sd, names, NH, H)
    with pytest.raises(ValueError, match="parameters"):
        CK.regions_from_optimizer_state(sd, names[:-1], NH, H)
    empty = CK.optimizer_state_from_regions(names, {}, NH, H, 0, 1e-3, (0.9, 0.95), 1e-8, 1e-2)       # before the first step: as torch
    assert empty["state"] == {} and CK.regions_from_optimizer_state(empty, names, NH, H)[:2] == ({}, 0)


# ------------------------------------------------------------------------------------------------ harness flags
def test_parser_flags(tmp_path, capsys):
    from drakegpt_amd import train
    a = train.parse_args([])
    assert a.save_every is None and a.resume is None and a.state_path == os.path.join("model", "TransformerLM.state.pt")
    a = train.parse_args(["--scale", "--model-dir", "m", "--save-every", "8", "--eval-interval", "4"])
    assert a.save_every == 8 and a.state_path == os.path.join("m", "TransformerLM_scaled.state.pt")
    existing = tmp_path / "s.pt"
    existing.write_bytes(b"")
    a = train.parse_args(["--save-every", "500", "--state-path", "x/y.pt", "--resume", str(existing)])
    assert (a.save_every, a.state_path, a.resume) == (500, "x/y.pt", str(existing))
    for bad in (["--save-every", "6", "--eval-interval", "4"], ["--save-every", "0"], ["--save-every", "-500"]):
        with pytest.raises(SystemExit) as ei:
            train.parse_args(bad)
        assert ei.value.code == 2
        assert "--save-every" in capsys.readouterr().err


def test_resume_of_a_missing_file_says_so(tmp_path, capsys):
    from drakegpt_amd import train
    missing = str(tmp_path / "nothing.state.pt")
    with pytest.raises(SystemExit) as ei:
        train.main(["--resume", missing])
    assert ei.value.code == 2
    err = capsys.readouterr().err
    assert "--resume" in err and missing in err


def test_resume_argument_mismatch_names_the_field(tmp_path):
    from drakegpt_amd import train
    path = str(tmp_path / "s.pt")
    args = train.parse_args(["--model", "BlocksLM", "--precision", "fp32"])
    mm = train.run_args(args, 1, 1)
    CK.save_train_state(path, {"format": CK.FORMAT, "version": CK.VERSION, "iteration": 4, "sched_steps": 1,
                               "rng_state": torch.get_rng_state(), "args": mm, "engine": None, "model": {}, "optimizer": {}})
    assert train.load_run_state(path, mm)["iteration"] == 4
    for field, other in (("model", "BigramLM"), ("precision", "bf16"), ("accum_steps", 2), ("world_size", 8), ("preset", "scaled"),
                         ("scale", True)):
        with pytest.raises(SystemExit, match=field):
            train.load_run_state(path, dict(mm, **{field: other}))


def test_engine_loop_resumes_on_the_uninterrupted_draws():
    """a run cut after iteration 5 of 11 (evaluation every 4) and resumed stages, in all, the rows the uninterrupted run stages"""
    from drakegpt_amd import train

    class Eng:
        def __init__(self):
            self.rows = []

        def stage_offsets(self, block):
            self.rows += [r.clone() for r in block]

        def step(self):
            pass

        def check_status(self):
            pass
    n_train, T, B = 1000, 8, 4
    one, g = Eng(), torch.Generator().manual_seed(5)
    train.engine_loop(one, n_train, T, B, 0, 1, 11, 4, lambda it: torch.rand(3, generator=g), "cpu", generator=g)
    two, g = Eng(), torch.Generator().manual_seed(5)
    train.engine_loop(two, n_train, T, B, 0, 1, 5, 4, lambda it: torch.rand(3, generator=g), "cpu", generator=g)
    train.engine_loop(two, n_train, T, B, 0, 1, 11, 4, lambda it: torch.rand(3, generator=g), "cpu", generator=g, start=5)
    assert len(one.rows) == len(two.rows) == 11
    assert all(torch.equal(a, b) for a, b in zip(one.rows, two.rows))
