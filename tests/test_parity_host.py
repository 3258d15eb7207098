"""oracle/parity.py on the CPU: the derived bounds hold for the reference's own rounding model, and every localized check
fails on a planted defect that the whole-tensor ratio at the suite's old tolerance lets through.

The "kernel output" here is always an emulation in torch on the host (fp64 arithmetic with bf16 roundings at the kernels'
documented rounding points, or fp32 torch ops where a kernel accumulates in fp32); defects are planted in those tensors."""
import pytest
import torch
import torch.nn.functional as F

from oracle import parity as P
from oracle import rng_ref

bf = torch.bfloat16

# the bf16 attention cases of tests/test_gpu_ops.py::test_attention / test_attention_more_shapes, of tests/test_gpu_gpt2_parity.py
# (B * NH cut to 1 .. 2 where T >= 640; 14 x 32 heads cut to 2 x 4) and of tests/test_gpu_conditioning.py (T = 256 form)
ATTN_CASES = [(2, 8, 4, 8, 0.0), (3, 37, 2, 16, 0.1), (2, 256, 3, 64, 0.2), (1, 1, 1, 32, 0.0), (2, 130, 2, 64, 0.0), (3, 100, 2, 64, 0.3),
              (2, 255, 2, 64, 0.1), (2, 256, 2, 128, 0.1), (1, 1024, 1, 64, 0.1), (1, 640, 1, 64, 0.0), (1, 1000, 1, 64, 0.1), (2, 256, 4, 64, 0.1)]
TOL_FWD, TOL_BWD = 8e-3, 2e-2                  # the suite's whole-tensor bounds (tests/test_gpu_ops.py, tests/test_gpu_gpt2_parity.py)


def _attn_inputs(B, T, NH, H, p, seed=None):
    g = torch.Generator().manual_seed(T * 7 + H if seed is None else seed)
    C = NH * H
    qkv = torch.randn(B * T, 3 * C, generator=g).to(bf)
    dout = torch.randn(B * T, C, generator=g).to(bf)
    keep = None
    if p > 0:
        keep = torch.from_numpy(rng_ref.keep_mask(77, 3, 4, p, B * NH * T * T).reshape(B, NH, T, T)).double()
    return qkv, dout, keep


@pytest.mark.parametrize("B,T,NH,H,p", ATTN_CASES)
def test_attention_rounding_model_stays_inside_its_bounds(B, T, NH, H, p):
    qkv, dout, keep = _attn_inputs(B, T, NH, H, p)
    ref = P.attention_fp64(qkv, dout, B, T, NH, H, keep, p)
    mod = P.attention_fp64(qkv, dout, B, T, NH, H, keep, p, model=True)
    P.assert_within_rounding(mod["out"], ref["out"], P.attention_fwd_envelope(ref), 1, "model forward")
    P.assert_rowwise(mod["out"], ref["out"], H, TOL_FWD, "model forward", T)
    # the hand-written backward is the autograd gradient of the hand-written forward
    qd = qkv.double().requires_grad_(True)
    q, k, v = qd.view(B, T, 3, NH, H).permute(2, 0, 3, 1, 4)
    w = (q @ k.transpose(-2, -1) * H ** -0.5).masked_fill(~torch.tril(torch.ones(T, T, dtype=torch.bool)), float("-inf")).softmax(-1)
    if keep is not None:
        w = w * keep / (1 - p)
    (w @ v).permute(0, 2, 1, 3).reshape(B * T, NH * H).backward(dout.double())
    assert P.rel(ref["dqkv"], qd.grad) < 1e-12
    # the model's worst (row, head) is what the GPU tests multiply by BWD_MARGIN.  It is a rounding-sized number: the model
    # as a whole meets the whole-tensor bound the project already uses for the backward, and its worst group stays within
    # the few bf16 roundings that enter one gradient row (a (row, head) of H = 8 averages over 8 elements only)
    bounds = P.attention_bwd_bounds(ref, mod, H)
    assert P.rel(mod["dqkv"], ref["dqkv"]) < TOL_BWD
    print(f"[parity-model] {(B, T, NH, H, p)}: fwd {P.rowwise_rel(mod['out'], ref['out'], H).max().item():.2e} "
          + " ".join(f"{n} {b / P.BWD_MARGIN:.2e}" for n, b in bounds.items()))
    pos = P.attention_bwd_bounds_by_position(ref, mod, B, T, NH, H)
    for n, b in bounds.items():
        assert 0 <= b / P.BWD_MARGIN < 0.5, (n, b)          # (dq: the first query rows, see attention_bwd_bounds_by_position)
        assert pos[n].max().item() <= b and (T < 128 or pos[n].median().item() < TOL_BWD)
        if b > 0:
            P.assert_rowwise(mod[n], ref[n], H, b, n, T)
            P.assert_rowwise_each(mod[n], ref[n], H, pos[n], n, T)


@pytest.mark.parametrize("B,T,NH,H,p", [(2, 256, 3, 64, 0.2), (1, 513, 1, 96, 0.2), (2, 300, 2, 128, 0.0), (1, 1024, 1, 64, 0.1)])
def test_attention_fp32_model_meets_the_fp32_tolerances(B, T, NH, H, p):
    """the fp32 kernels' counterpart (torch float32 arithmetic): every (row, head) at the suite's fp32 tolerances, except where dq
    cancels (the first query rows: delta from an fp32-rounded output against a denominator at its floor), which is what the
    position-resolved bound is for"""
    qkv, dout, keep = _attn_inputs(B, T, NH, H, p)
    qkv, dout = qkv.float() + 0.001, dout.float()               # (not bf16-representable: fp32 operands)
    ref = P.attention_fp64(qkv, dout, B, T, NH, H, keep, p)
    mod = P.attention_fp64(qkv, dout, B, T, NH, H, keep, p, model="fp32")
    P.assert_rowwise(mod["out"], ref["out"], H, 2e-5, "fp32 model forward", T)
    pos = P.attention_bwd_bounds_by_position(ref, mod, B, T, NH, H, at_least=3e-5)
    for n in ("dq", "dk", "dv"):
        e = P.rowwise_rel(mod[n], ref[n], H).view(B, T, NH)
        assert e[:, 64:].max().item() < 3e-5 and pos[n].view(B, T, NH)[:, 64 + P.BWD_WINDOW:].max().item() == 3e-5, n
        P.assert_rowwise_each(mod[n], ref[n], H, pos[n], n, T)


def _conditioning():
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("_dg_conditioning", os.path.join(os.path.dirname(__file__), "test_gpu_conditioning.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("kind,T,p", [("rising", 256, 0.0), ("rising", 1024, 0.1), ("falling", 256, 0.1), ("falling", 1024, 0.0), ("onehot", 256, 0.0),
                                      ("uniform", 256, 0.1), ("same_keys", 256, 0.0), ("randn", 8, 0.9), ("randn", 64, 0.9)])
def test_attention_rounding_model_on_structured_operands(kind, T, p):
    """the operands of tests/test_gpu_conditioning.py (B * NH = 1 at T = 1024): the model stays inside the forward envelope, finite
    everywhere, and the position-resolved backward bounds it yields are finite"""
    cond = _conditioning()
    assert (kind, T, p) in cond.ATTN_KINDS
    B, NH, H = (4, 4, 64) if T <= 64 else (1, 1 if T == 1024 else 2, 64)
    g = torch.Generator().manual_seed(T + len(kind))
    q, k, v = cond._attn_operands(kind, B, T, NH, H, g)
    qkv = torch.stack([q, k, v], 2).reshape(B * T, 3 * NH * H).to(bf)
    dout = torch.randn(B * T, NH * H, generator=g).to(bf)
    keep = torch.from_numpy(rng_ref.keep_mask(5, 2, 8, p, B * NH * T * T).reshape(B, NH, T, T)).double() if p > 0 else None
    ref = P.attention_fp64(qkv, dout, B, T, NH, H, keep, p)
    mod = P.attention_fp64(qkv, dout, B, T, NH, H, keep, p, model=True)
    P.assert_within_rounding(mod["out"], ref["out"], P.attention_fwd_envelope(ref), 1, f"{kind} model forward")
    floors = {n: P.structured_floor(ref, n, H) for n in ("dq", "dk", "dv")}
    bounds = P.attention_bwd_bounds_by_position(ref, mod, B, T, NH, H, at_least=3e-5, floors=floors)
    for n in ("dq", "dk", "dv"):
        # (the bound means something: see the comment at the same assertion in tests/test_gpu_conditioning.py)
        assert torch.isfinite(mod[n]).all() and bounds[n].max().item() < 10 and (n == "dq" or bounds[n].median().item() < 0.1), (n, bounds[n].max().item())
        P.assert_rowwise_each(mod[n], ref[n], H, bounds[n], n, T, floor=floors[n])


def _gemm_case(M=40000, N=192, K=128):
    g = torch.Generator().manual_seed(1)
    A = torch.randn(M, K, generator=g).to(bf)
    B = torch.randn(N, K, generator=g).to(bf)
    bias = torch.randn(N, generator=g)
    resid = torch.randn(M, N, generator=g)
    return A, B, bias, resid


@pytest.mark.parametrize("M,N,K", [(320, 200, 128), (300, 384, 128), (1100, 1152, 192), (256, 1536, 128), (40000, 192, 128)])
def test_gemm_envelope_holds_for_fp32_accumulation(M, N, K):
    """bf16 operands, fp32 accumulation (torch's fp32 matmul: another summation order than the MFMA's, the same bound), bias +
    ReLU and bias + dropout + residual, rounded once to bf16"""
    A, B, bias, resid = _gemm_case(M, N, K)
    acc = A.double() @ B.double().T + bias.double()
    env = P.gemm_envelope(A, B, K, bias)
    got = (A.float() @ B.float().T + bias).clamp_min(0).to(bf)
    decided = P.mask_margin(acc, env)
    P.assert_within_rounding(got, acc.clamp_min(0), env, 1, "bias + relu", where=decided)
    keep = torch.from_numpy(rng_ref.keep_mask(1234, 5, 9, 0.25, M * N).reshape(M, N)).double()
    got = ((A.float() @ B.float().T + bias) * keep.float() * (1 / 0.75) + resid).to(bf)
    env = P.gemm_envelope(A, B, K, bias, resid, keep_scale=keep / 0.75)
    P.assert_within_rounding(got, acc * keep / 0.75 + resid.double(), env, 1, "bias + dropout + residual")


@pytest.mark.parametrize("C", [32, 384, 1024, 100])
def test_single_rounding_envelopes(C):
    g = torch.Generator().manual_seed(C)
    x = torch.randn(517, C, generator=g) * 2 + 0.5
    w, b = torch.randn(C, generator=g), torch.randn(C, generator=g)
    ref = F.layer_norm(x.double(), (C,), w.double(), b.double(), 1e-5)
    P.assert_within_rounding(F.layer_norm(x, (C,), w, b, 1e-5).to(bf), ref, P.single_rounding_envelope(ref, C), 1, "layernorm")
    V = C
    logits = torch.randn(64, V, generator=g) * 3
    tgt = torch.randint(0, V, (64,), generator=g)
    gref = (torch.softmax(logits.double(), 1) - F.one_hot(tgt, V)) / 64
    got = ((torch.softmax(logits, 1) - F.one_hot(tgt, V)) / 64).to(bf)
    P.assert_within_rounding(got, gref, P.single_rounding_envelope(gref, V), 1, "cross entropy gradient")


# ---------------------------------------------------------------------------------------------------------------------
# planted defects
# ---------------------------------------------------------------------------------------------------------------------
def _subjects():
    """name -> (emulated kernel output, fp64 reference, new check, old whole-tensor tolerance, elements per group)"""
    out = {}
    # attention: the (14, 256, 32, 64) case of the long-sequence tests
    B, T, NH, H, p = 14, 256, 32, 64, 0.1
    qkv, dout, keep = _attn_inputs(B, T, NH, H, p)
    ref = P.attention_fp64(qkv, dout, B, T, NH, H, keep, p)
    mod = P.attention_fp64(qkv, dout, B, T, NH, H, keep, p, model=True)
    env = P.attention_fwd_envelope(ref)

    def fwd_check(x):
        P.assert_within_rounding(x, ref["out"], env, 1, "out")
        P.assert_rowwise(x, ref["out"], H, TOL_FWD, "out", T)
    out["attention forward"] = (mod["out"], ref["out"], fwd_check, TOL_FWD, H)
    bounds = P.attention_bwd_bounds_by_position(ref, mod, B, T, NH, H)

    def bwd_check(x):
        for i, n in enumerate(("dq", "dk", "dv")):
            P.assert_rowwise_each(x.view(B * T, 3, NH * H)[:, i], ref[n], H, bounds[n], n, T)
    out["attention backward"] = (mod["dqkv"], ref["dqkv"], bwd_check, TOL_BWD, H)
    # bf16-output GEMM, bias + ReLU, 40000 x 192 (the many-tiles-per-workgroup case of test_gemm_nt_epilogue)
    A, Bm, bias, _ = _gemm_case()
    acc = A.double() @ Bm.double().T + bias.double()
    genv = P.gemm_envelope(A, Bm, 128, bias)
    decided = P.mask_margin(acc, genv)
    out["gemm bf16 out"] = ((A.float() @ Bm.float().T + bias).clamp_min(0).to(bf).double(), acc.clamp_min(0),
                            lambda x: P.assert_within_rounding(x, acc.clamp_min(0), genv, 1, "gemm", where=decided), 6e-3, 32)
    # LayerNorm bf16 output (517 x 2048, the widest case of test_layernorm); the defects are one 16-byte chunk wide
    g = torch.Generator().manual_seed(2048)
    x = torch.randn(517, 2048, generator=g) * 2 + 0.5
    w, b = torch.randn(2048, generator=g), torch.randn(2048, generator=g)
    lref = F.layer_norm(x.double(), (2048,), w.double(), b.double(), 1e-5)
    lenv = P.single_rounding_envelope(lref, 2048)
    out["layernorm bf16 out"] = (F.layer_norm(x, (2048,), w, b, 1e-5).to(bf).double(), lref,
                                 lambda y: P.assert_within_rounding(y, lref, lenv, 1, "layernorm"), 4e-3, 8)
    return out


_SUBJECTS = {}
# the one pair that the old check does notice at the size of the test it is taken from (ratio 4.3e-3 against 4e-3: two
# chunks' worth of difference in 1.06 M elements on top of 2.2e-3 of bf16 rounding)
OLD_CHECK_SEES_IT = {("layernorm bf16 out", "chunk_from_neighbour")}


def _subject(name):
    if not _SUBJECTS:
        _SUBJECTS.update(_subjects())
    return _SUBJECTS[name]


@pytest.mark.parametrize("third", [0, 1, 2])
@pytest.mark.parametrize("defect", P.DEFECTS)
def test_planted_defect_in_attention_backward(defect, third):
    _planted("attention backward", defect, third)


@pytest.mark.parametrize("defect", P.DEFECTS)
@pytest.mark.parametrize("name", ["attention forward", "gemm bf16 out", "layernorm bf16 out"])
def test_planted_defect_is_caught_by_the_new_check_and_missed_by_the_old(name, defect):
    _planted(name, defect)


def _planted(name, defect, third=1):
    got, ref, check, old_tol, group = _subject(name)
    check(got)                                              # the undamaged emulation passes
    assert P.rel(got, ref) < old_tol
    if name == "attention backward":
        # plant in one third: the other two, correct, must not hide it
        C = got.shape[1] // 3
        bad = got.clone()
        bad[:, third * C:(third + 1) * C] = P.plant(got[:, third * C:(third + 1) * C], defect, group)
    else:
        bad = P.plant(got, defect, group)
    assert not torch.equal(bad, got)
    with pytest.raises(AssertionError, match="tile"):
        check(bad)
    # the table of the issue as a test: the whole-tensor ratio at the old tolerance does not see it
    if (name, defect) not in OLD_CHECK_SEES_IT:
        assert P.rel(bad, ref) < old_tol, (name, defect, P.rel(bad, ref))


def test_rowwise_rel_floors_tiny_rows_and_reports_the_worst_group():
    ref = torch.ones(64, 128, dtype=torch.float64)
    ref[5] *= 1e-6                                          # a legitimately tiny row
    got = ref.clone()
    got[5, :64] += 1e-6                                     # 100 % of itself, nothing at the tensor's scale
    assert P.rowwise_rel(got, ref, 64).max().item() < 1e-5
    got[40, 64:] *= 1.5
    e = P.rowwise_rel(got, ref, 64)
    assert int(e.argmax()) == 81 and abs(e.max().item() - 0.5) < 1e-12
    with pytest.raises(AssertionError, match=r"row 40.*head 1, 32-row tile 1 \(row 8 of it\)"):
        P.assert_rowwise(got, ref, 64, 1e-2, "x")
    got[40, 64] = float("nan")
    assert P.rowwise_rel(got, ref, 64).max().item() == float("inf")


def test_assert_within_rounding_counts_and_locates():
    ref = torch.linspace(1, 2, 64 * 96, dtype=torch.float64).reshape(64, 96)
    P.assert_within_rounding(P.rb(ref), ref, 0.0, 1, "rounded")           # one round-to-nearest is inside one ulp, no envelope
    got = P.rb(ref)
    got[33, 72:80] += 0.1
    with pytest.raises(AssertionError, match=r"8 of 6144 elements.*tile \(1, 2\), 8-element chunk 9 of row 33"):
        P.assert_within_rounding(got, ref, 0.0, 1, "x")
    got[0, 0] = float("inf")
    with pytest.raises(AssertionError, match="9 of 6144"):
        P.assert_within_rounding(got, ref, 0.0, 1, "x")


# ---------------------------------------------------------------------------------------------------------------------
# decode attention: the reference, the spotlight inputs, and the defects the checks of tests/test_gpu_decode.py must refuse
# ---------------------------------------------------------------------------------------------------------------------
def test_decode_reference_is_row_t_of_the_causal_reference():
    B, Tcap, NH, H, t = 2, 40, 3, 8, 29
    g = torch.Generator().manual_seed(3)
    cache = torch.randn(B, Tcap, 3 * NH * H, generator=g)
    cache[:, t + 1:] = float("nan")                          # rows past t are not read
    out, Pr = P.decode_attention_fp64(cache, t, B, Tcap, NH, H)
    full = P.attention_fp64(cache[:, :t + 1].reshape(B * (t + 1), -1), None, B, t + 1, NH, H)
    assert (out - full["out"].view(B, t + 1, NH * H)[:, t]).abs().max().item() < 1e-13
    assert (Pr - full["P"][:, :, t]).abs().max().item() < 1e-14 and (Pr.sum(-1) - 1).abs().max().item() < 1e-14
    # the append form: row t comes from the staging row, whatever the cache holds there
    stale = cache.clone()
    stale[:, t] = float("nan")
    out2, P2 = P.decode_attention_fp64(stale, t, B, Tcap, NH, H, row=cache[:, t])
    assert torch.equal(out2, out) and torch.equal(P2, Pr)
    out3, _ = P.decode_attention_fp64(cache, t, B, Tcap, NH, H, scale=0.3)
    assert not torch.allclose(out3, out)


@pytest.mark.parametrize("dtype", [torch.float32, bf])
@pytest.mark.parametrize("Tcap,H,t,j_star", [(70, 8, 1, 0), (70, 8, 69, 64), (131, 96, 130, 130), (1024, 64, 1023, 1022)])
def test_spotlight_key_holds_half_of_the_mass(dtype, Tcap, H, t, j_star):
    B, NH = 2, 3
    cache = P.spotlight_decode_inputs(B, Tcap, NH, H, t, j_star, 5, dtype)
    assert cache.dtype == dtype and tuple(cache.shape) == (B, Tcap, 3 * NH * H)
    _, Pr = P.decode_attention_fp64(cache, t, B, Tcap, NH, H)
    assert (Pr[:, :, j_star] - 0.5).abs().max().item() < 0.05
    # only the key row's k third differs from the plain draw of the same seed
    plain = torch.randn((B, Tcap, 3 * NH * H), generator=torch.Generator().manual_seed(5)).to(dtype)
    diff = (cache != plain).view(B, Tcap, 3, NH * H)
    assert bool(diff[:, j_star, 1].any()) and int(diff.sum()) == int(diff[:, j_star, 1].sum())


DECODE_DEFECTS = ("key_t_left_out", "stale_row_t", "one_key_too_many", "v_of_next_head", "last_group_unwritten", "first_lane_round_only")


@pytest.mark.parametrize("defect", DECODE_DEFECTS)
def test_planted_decode_defect_is_refused(defect):
    """(B, NH, H, t) = (3, 3, 96, 130), spotlight on key t; the emulated kernel output is the fp64 result of the defective
    algorithm rounded as a bf16 kernel stores it (P.rb), judged by the helper and bound the GPU tests use"""
    B, NH, H, t, Tcap = 3, 3, 96, 130, 132
    good = P.spotlight_decode_inputs(B, Tcap, NH, H, t, t, 9, bf)
    good[:, t + 1:] = float("nan")                           # poisoned like the GPU tests' caches
    row = good[:, t].clone()
    stale = good.clone()
    stale[:, t] = torch.randn(B, 3 * NH * H, generator=torch.Generator().manual_seed(10)).to(bf)   # what an earlier call left there
    ref, _ = P.decode_attention_fp64(stale, t, B, Tcap, NH, H, row=row)
    assert torch.equal(ref, P.decode_attention_fp64(good, t, B, Tcap, NH, H)[0])
    P.assert_decode_output(P.rb(ref), ref, H, bf, "undamaged")
    P.assert_decode_output(ref.float(), ref, H, torch.float32, "undamaged fp32")

    def heads(c):
        return c.view(B, Tcap, 3, NH, H)

    def attend(keys):                                        # query t over the given key positions only
        q = heads(good)[:, t, 0].double()
        k, v = heads(good)[:, keys, 1].double(), heads(good)[:, keys, 2].double()
        w = torch.softmax(torch.einsum("bhd,bjhd->bhj", q, k) * H ** -0.5, -1)
        return torch.einsum("bhj,bjhd->bhd", w, v).reshape(B, NH * H)

    assert (attend(slice(0, t + 1)) - ref).abs().max().item() < 1e-13
    if defect == "key_t_left_out":
        bad = attend(slice(0, t))
    elif defect == "stale_row_t":
        bad = P.decode_attention_fp64(stale, t, B, Tcap, NH, H)[0]
    elif defect == "one_key_too_many":                       # the poisoned row t + 1
        bad = attend(slice(0, t + 2))
        assert not torch.isfinite(bad).any()
    elif defect == "v_of_next_head":
        c = good.clone()
        heads(c)[:, :t + 1, 2, 1] = heads(good)[:, :t + 1, 2, 2]
        bad = P.decode_attention_fp64(c, t, B, Tcap, NH, H)[0]
    elif defect == "last_group_unwritten":
        bad = ref.clone()
        bad[B - 1, (NH - 1) * H:] = 55.0                     # the guard fill of the GPU tests
    elif defect == "first_lane_round_only":                  # keys j >= 64 never visited
        bad = attend(slice(0, 64))
    with pytest.raises(AssertionError, match="non-finite" if defect == "one_key_too_many" else "worst group"):
        P.assert_decode_output(P.rb(bad), ref, H, bf, defect)
    with pytest.raises(AssertionError):
        P.assert_decode_output(bad.float(), ref, H, torch.float32, defect)


# ---------------------------------------------------------------------------------------------------------------------
# the block chain: the stage checks of tests/test_gpu_chain_parity.py on a CPU stand-in (tests/chain_model.py)
# ---------------------------------------------------------------------------------------------------------------------
import os  # noqa: E402
import sys  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_model as CM  # noqa: E402

CHAIN_OLD_TOL = 3e-4                           # the whole-tensor ratio of test_block_chain_kernel_equals_the_launches_it_replaces
_CHAIN = {}


def _chain_case(M, mode, p):
    key = (M, mode, p)
    if key not in _CHAIN:
        op = CM.fwd_operands(M, M + mode)
        _CHAIN[key] = (op, CM.fwd_standin(op, mode, p))
    return _CHAIN[key]


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("M,p", [(64, 0.0), (64, 0.2), (320, 0.0), (320, 0.2)])
def test_chain_standin_stays_inside_every_stage_bound(M, mode, p):
    """the envelopes are not vacuous: fp64 rounded at the kernel's store points passes every stage, and the roundings alone
    use a visible part of the bf16 stages' bounds"""
    op, good = _chain_case(M, mode, p)
    use = CM.check_fwd(good, op, mode, p, mask=good.get("mask"), grid=2)
    assert use and all(0 <= u <= 1 for u in use.values()), use
    for k in ("h2", "f", "h1", "qkv"):
        assert k not in use or use[k] > 0.3, (k, use[k])


@pytest.mark.parametrize("M", [64, 320])
def test_chain_operand_recipe_leaves_few_signs_undecided(M):
    """mask_margin's cap (1e-3) is a condition on the operands: the recipe meets it with a wide margin on the fp64 reference alone"""
    op, good = _chain_case(M, 0, 0.2)
    pre = good["h2"].double() @ op["w1"].double().T + op["b1"].double()
    decided = P.mask_margin(pre, P.gemm_envelope(good["h2"], op["w1"], CM.C, op["b1"]))
    assert 1.0 - decided.double().mean().item() < 5e-4


# defects the old comparison (ratio of the whole tensor against the clean result at 3e-4; up to max(2, bytes / 100000) differing
# sign-bit bytes) lets through at M = 320
CHAIN_OLD_CHECK_MISSES = {"decided_sign_bit_flipped"}


@pytest.mark.parametrize("defect", CM.FWD_DEFECTS)
def test_planted_chain_defect_is_refused_at_its_stage(defect):
    M, mode, p = 320, 0, 0.2
    op, good = _chain_case(M, mode, p)
    bad = CM.fwd_standin(op, mode, p, defect=defect, cus=2)
    assert any(not torch.equal(bad[k], good[k]) for k in good)
    with pytest.raises(AssertionError, match=CM.FWD_DEFECT_STAGE[defect] + r":.*\[64-row block \d+: workgroup \d+, round \d+"):
        CM.check_fwd(bad, op, mode, p, mask=bad["mask"], grid=2)
    flipped = int((bad["mask"] != good["mask"]).sum())
    old_passes = all(P.rel(bad[k], good[k]) < CHAIN_OLD_TOL for k in good if k != "mask") and flipped <= 2
    assert old_passes == (defect in CHAIN_OLD_CHECK_MISSES), (defect, {k: P.rel(bad[k], good[k]) for k in good}, flipped)


def _chain_bwd_case(M, mode, p):
    key = ("bwd", M, mode, p)
    if key not in _CHAIN:
        op = CM.bwd_operands(M, 7 * M + mode)
        _CHAIN[key] = (op,) + CM.bwd_standin(op, mode, p)
    return _CHAIN[key]


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("M,p", [(64, 0.0), (64, 0.2), (320, 0.2)])
def test_chain_bwd_standin_stays_inside_every_stage_bound(M, mode, p):
    op, good, parts = _chain_bwd_case(M, mode, p)
    use = CM.check_bwd(good, parts, op, mode, p, op["mask"])
    assert use and all(0 <= u <= 1 for u in use.values()), use
    for k in ("dx1", "g1", "dx2", "g2", "df", "dout"):                    # the stand-in's own roundings use a visible part of each bound
        assert k not in use or use[k] > 0.2, (k, use[k])


@pytest.mark.parametrize("defect", CM.BWD_DEFECTS)
def test_planted_chain_bwd_defect_is_refused_at_its_stage(defect):
    M, mode, p = 320, 0, 0.2
    op, good, parts = _chain_bwd_case(M, mode, p)
    bad, bad_parts = CM.bwd_standin(op, mode, p, defect=defect)
    assert any(not torch.equal(bad[k], good[k]) for k in good) or not torch.equal(bad_parts, parts)
    with pytest.raises(AssertionError, match=CM.BWD_DEFECT_STAGE[defect] + ".*(row|block) "):
        CM.check_bwd(bad, bad_parts, op, mode, p, op["mask"])


def test_rounding_margin_marks_values_near_a_bf16_rounding_boundary():
    # bf16 neighbours of 1.0 upwards: 1, 1 + 2^-7; the boundary between them is 1 + 2^-8
    v = torch.tensor([1.0, 1.0 + 2.0 ** -8 - 1e-6, 1.0 + 2.0 ** -8 + 1e-6, 1.0 + 2.0 ** -8 - 1e-3, -(2.0 + 2.0 ** -7) + 1e-7, 0.75], dtype=torch.float64)
    allow, share = P.rounding_margin(v, torch.full_like(v, 1e-5), max_share=1.0)
    assert allow.tolist() == [0.0, 2.0 ** -7, 2.0 ** -7, 0.0, 2.0 ** -6, 0.0] and abs(share - 0.5) < 1e-12
    with pytest.raises(AssertionError, match="rounding boundary"):
        P.rounding_margin(v, torch.full_like(v, 1e-5))
    # what the margin is for: a value computed in fp32 rounds to rb(v) or, only where it is marked, to the neighbour one ulp away
    g = torch.Generator().manual_seed(0)
    A, B = torch.randn(256, 384, generator=g).to(bf), (torch.randn(384, 384, generator=g) * 384 ** -0.5).to(bf)
    exact = A.double() @ B.double().T
    allow, share = P.rounding_margin(exact, P.gemm_envelope(A, B, 384), max_share=1.0)
    diff = ((A.float() @ B.float().T).to(bf).double() - P.rb(exact)).abs()
    assert bool((diff <= allow).all()) and 0 < share < 1
