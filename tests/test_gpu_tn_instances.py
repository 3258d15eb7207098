"""The dW (TN) GEMMs per kernel, split map, K-step class and launch chunk (tests/tn_cases.py), element by element.

Every case first asserts, from the library's own launch plan with the CU count of this device, that it is the case it is named
for.  All outputs, slabs and the gaps between them start as NaN.

dg_gemm_tn, every case twice:
  (a) iid integers in [-4, 4]: every partial sum is an integer below 2^24, so every slab must be BIT-EQUAL to the fp64 product
      over its own rows (that pins r_per_split and the (tile, split) map, not only the sum; an empty split's slab is exactly
      0.0), and nothing outside [P, Q] of a slab may be written: padding of ldo, the gaps of a wider split_stride, the float in
      front of an offset `out`, the tail;
  (b) N(0, 1): every element of every slab and of dg_reduce_partials' sum within the rounding envelope of its own sum
      (tn_cases.slab_envelope / sum_envelope: derived, ulps = 0); precision "bf16x3" keeps the whole-tensor bound of
      tests/test_gpu_bf16x3.py on every non-empty slab and on the sum.
dg_gemm_tn_grouped: the fp8 body on single problems of one to four K steps (whole, and in halves of 1 + 1, 1 + 2, 2 + 2) behind
NaN-padded leading dimensions into an output view, and calls of more problems than one launch holds for both bodies, each
without a workspace and then three times on ONE workspace that lies inside a larger allocation: bit-equal runs, status word 0,
the band behind the workspace untouched.  Exact data must come out exact for fp8 too (A in [-4, 4], B in [-8, 8], power-of-two
scales: every K-step sum is an integer below 2^13); random data: the bf16 element envelope (K = R, and R + 1 for a tile summed
from two halves), fp8 the project's 4e-5 whole-problem bound.

Largest error / envelope over all cases, measured on MI355X (256 CUs; a report, not a bound; DG_TEST_REPORT=1 prints them):
  gemm_tn_ws_kernel 0.025, gemm_tn_bf16_kernel 0.185 (its largest at R = 40: the fewer rows, the fewer roundings the bound
  over-counts), gemm_tn_f32_kernel 0.357, dg_reduce_partials' sum 0.079; gemm_tn_x3_kernel 3.9e-6 .. 4.6e-6 against its 1e-5;
  grouped bf16 whole tiles 0.018, summed from two halves 0.011; grouped fp8 exact on the integer data (the instruction's adder
  keeps every bit of K-step sums below 2^13).
On the parent of the change that added this file the 70-problem bf16 case failed as predicted from the code: problems 65, 66, 67
and 69 -- of the second launch's six -- came out with hundreds to thousands of wrong elements, other ones in each of the three
runs on the workspace, with status word 0 and no fault (the second launch's flags lay in the first launch's partials)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tn_cases as T  # noqa: E402
from oracle import parity as P  # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")
USE = {}


def _ops():
    from drakegpt_amd import ops
    return ops


def _ncu(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _note(key, use):
    USE[key] = max(USE.get(key, 0.0), use)
    if os.environ.get("DG_TEST_REPORT"):
        print(f"[tn] envelope use {key}: {use:.3f} (largest so far {USE[key]:.3f})", flush=True)


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


# ---------------------------------------------------------------------------------------------------------------------
# dg_gemm_tn
# ---------------------------------------------------------------------------------------------------------------------
MAT_NAMES = [c.name for c in T.mat_cases(256)]


def run_mat(dev, case, kind):
    """(buffer [total] on the host after the launch, reduced sum [slab], plan)"""
    ops = _ops()
    lay = T.layout(case)
    pl = T.plan(case.R, case.P, case.Q, case.S, case.dtype)
    A, B, Ad, Bd = T.mat_operands(case, kind)
    A, B = A.to(dev), B.to(dev)
    buf = torch.full((lay.total,), NAN, device=dev)
    out = buf[lay.offset:]
    assert (out.data_ptr() % 16 == 0) == (case.layout != "out+1")
    ops.gemm_tn(A[:, :case.P], B[:, :case.Q], out, lay.stride, case.S, case.P, case.Q, ldo=lay.ldo, split=case.kind == "x3")
    red = torch.full((lay.slab + 3,), NAN, device=dev)
    ops.reduce_partials(out, lay.stride, case.S, red, lay.slab)
    torch.cuda.synchronize()
    return buf.cpu(), red.cpu(), pl, Ad, Bd


def slabs_of(case, host):
    """the [P, Q] views of the S slabs, and the mask of everything else in the buffer"""
    lay = T.layout(case)
    rest = torch.ones(lay.total, dtype=torch.bool)
    views = []
    for s in range(case.S):
        o = lay.offset + s * lay.stride
        views.append(host.as_strided((case.P, case.Q), (lay.ldo, 1), o))
        rest.as_strided((case.P, case.Q), (lay.ldo, 1), o).fill_(False)
    return views, rest


@pytest.mark.parametrize("name", MAT_NAMES)
def test_gemm_tn_case(dev, name):
    case = {c.name: c for c in T.mat_cases(_ncu(dev))}[name]
    kernel, _, _ = case.check_class()                                  # with the device's CU count
    fp32 = case.dtype != T.BF16
    # (a) exact data
    host, red, pl, Ad, Bd = run_mat(dev, case, "exact")
    rows = T.slab_rows(case.R, case.S, pl.r_per_split)
    refs = T.slab_references(Ad, Bd, rows)
    views, rest = slabs_of(case, host)
    assert bool(torch.isnan(host[rest]).all()), f"{name}: {int((~torch.isnan(host[rest])).sum())} floats outside the slabs were written"
    for s, (v, (ref, _, n)) in enumerate(zip(views, refs)):
        assert ref.abs().max().item() < 2 ** 24
        bad = v.double() != ref                                        # (NaN != x: an unwritten element counts)
        assert not bool(bad.any()), (f"{name}: slab {s} (rows {rows[s]}) differs from the product over its own rows in {int(bad.sum())} elements, "
                                     f"first at {tuple(int(i) for i in bad.nonzero()[0])}")
        if n == 0:
            assert bool((v == 0).all())
    lay = T.layout(case)
    total = red.as_strided((case.P, case.Q), (lay.ldo, 1), 0)
    assert torch.equal(total.double(), Ad.T @ Bd) and bool(torch.isnan(red[lay.slab:]).all())
    # (b) random data
    host, red, pl, Ad, Bd = run_mat(dev, case, "randn")
    refs = T.slab_references(Ad, Bd, rows)
    views, rest = slabs_of(case, host)
    assert bool(torch.isnan(host[rest]).all())
    total, whole = red.as_strided((case.P, case.Q), (lay.ldo, 1), 0), Ad.T @ Bd
    if case.kind == "x3":
        from test_gpu_bf16x3 import _bf, _check
        A32, B32 = Ad.float(), Bd.float()
        for s, (v, (ref, _, n)) in enumerate(zip(views, refs)):
            lo, hi = rows[s]
            if n:
                _check(f"{name} slab {s}", v, ref, _bf(A32[lo:hi]).T @ _bf(B32[lo:hi]))
            else:
                assert bool((v == 0).all())
        _check(f"{name} sum", total, whole, _bf(A32).T @ _bf(B32))
        return
    use = 0.0
    for s, (v, (ref, mag, n)) in enumerate(zip(views, refs)):
        if n == 0:
            assert bool((v == 0).all())
            continue
        use = max(use, P.assert_within_rounding(v, ref, T.slab_envelope(mag, n, fp32), ulps=0, name=f"{name} slab {s} (rows {rows[s]})"))
    _note(kernel, use)
    _note("reduce_partials", P.assert_within_rounding(total, whole, T.sum_envelope(refs, fp32), ulps=0, name=f"{name} sum"))


# ---------------------------------------------------------------------------------------------------------------------
# dg_gemm_tn_grouped
# ---------------------------------------------------------------------------------------------------------------------
GROUPS = {g.name: g for g in T.group_cases(256)}
SINGLE_NAMES = [n for n, g in GROUPS.items() if len(g.shapes) == 1]
MULTI_NAMES = [n for n, g in GROUPS.items() if len(g.shapes) > 1]
GUARD_BYTE = 0xA5


def guarded_workspace(dev, case):
    """(buffer, reported bytes): the zero-filled workspace of the size the library reports at the front of a larger allocation.
    The band behind it is sized by this test's own arithmetic -- partials and flags of the call's largest launch, 128 KB + 32
    bytes per tile, + 16 -- plus 4 MiB: whatever size the library reports, nothing it could write for these launches leaves
    the allocation."""
    reported = T.workspace_bytes(case.rpq)
    step = T.MAX_GROUP[case.f8]
    tiles = [T.group_tiles(Pn, Q) for Pn, Q in case.shapes]
    largest = max(sum(tiles[b:b + step]) for b in range(0, len(tiles), step))
    front = -(-reported // 16) * 16
    buf = torch.full((front + largest * (T.PART_BYTES + 32) + 16 + (4 << 20),), GUARD_BYTE, dtype=torch.uint8, device=dev)
    buf[:reported].zero_()
    assert buf.data_ptr() % 16 == 0 and buf.numel() - reported >= 4 << 20
    return buf, reported


def guard_untouched(buf, reported):
    return bool((buf[reported:] == GUARD_BYTE).all())


def status(buf, reported):
    return int(buf[reported - 16:reported].view(torch.int32)[0].item())


def call_grouped(arr, n, code, buf, reported):
    ops = _ops()
    ops.check(ops.lib.dg_gemm_tn_grouped(arr, n, code, buf.data_ptr() if buf is not None else None, reported if buf is not None else 0,
                                         ops._stream()), "dg_gemm_tn_grouped")
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", SINGLE_NAMES)
def test_grouped_fp8_single_problem(dev, name):
    """one fp8 problem of 1, 2, 3, 4 K steps: whole, and (from two steps on) in halves through the workspace"""
    ops = _ops()
    case = {g.name: g for g in T.group_cases(_ncu(dev))}[name]
    cut, _ = case.check_class()
    (Pn, Q), ldo = case.shapes[0], case.shapes[0][1] + 5
    assert cut[0].splits == (2 if case.R >= 256 else 1)
    buf, reported = guarded_workspace(dev, case)
    for kind in ("exact", "randn"):
        A, B, ref, sa, sb = T.fp8_single_operands(case, kind)
        Ad, Bd = A.to(dev), B.to(dev)
        out = torch.empty(Pn, ldo, device=dev)
        probs = [(Ad[:, :Pn], Bd[:, :Q], out, Pn, Q, sa.to(dev), sb.to(dev))]
        arr, code = ops._tn_problem_array(probs)
        arr[0].ldo = ldo
        runs = []
        for ws in (None, buf, buf):
            out.fill_(NAN)
            call_grouped(arr, 1, code, ws, reported)
            got = out.cpu()
            assert bool(torch.isnan(got[:, Q:]).all()), f"{name} {kind}: written between the rows of the output view"
            if kind == "exact":
                bad = got[:, :Q].double() != ref
                assert not bool(bad.any()), f"{name}: {int(bad.sum())} elements differ from the exact product, first at {tuple(int(i) for i in bad.nonzero()[0])}"
            else:
                assert rel(got[:, :Q], ref) < 4e-5, (name, ws is not None, rel(got[:, :Q], ref))
                _note("grouped fp8, whole-problem error / 4e-5", rel(got[:, :Q], ref) / 4e-5)
            runs.append(got[:, :Q].clone())
        assert torch.equal(runs[1], runs[2])
    assert status(buf, reported) == 0 and guard_untouched(buf, reported)


@pytest.mark.parametrize("name", MULTI_NAMES)
def test_grouped_more_problems_than_one_launch(dev, name):
    ops = _ops()
    case = {g.name: g for g in T.group_cases(_ncu(dev))}[name]
    cut, _ = case.check_class()
    step = T.MAX_GROUP[case.f8]
    is_cut = [cut[i // step].splits != 1 for i in range(len(case.shapes))]
    assert any(is_cut) and len(cut) >= 2
    buf, reported = guarded_workspace(dev, case)
    # outputs: slices of one NaN-filled buffer, 16-byte aligned, 8 floats apart
    offs, o = [], 0
    for Pn, Q in case.shapes:
        offs.append(o)
        o += -(-(Pn * Q) // 4) * 4 + 8
    big = torch.empty(o, device=dev)
    gaps = torch.ones(o, dtype=torch.bool)
    for off, (Pn, Q) in zip(offs, case.shapes):
        gaps[off:off + Pn * Q] = False
    for kind in ("exact", "randn"):
        A, B, probs_h = T.group_operands(case, kind)
        Ad, Bd = A.to(dev), B.to(dev)
        probs, keep = [], []
        for (a, b, _, _, sa, sb), off, (Pn, Q) in zip(probs_h, offs, case.shapes):
            oa, ob = a.storage_offset(), b.storage_offset()
            p = (Ad[:, oa:oa + Pn], Bd[:, ob:ob + Q], big[off:off + Pn * Q], Pn, Q)
            if case.f8:
                keep += [sa.to(dev), sb.to(dev)]
                p += (keep[-2], keep[-1])
            probs.append(p)
        arr, code = ops._tn_problem_array(probs)
        runs = []
        for ws in (None, buf, buf, buf):
            big.fill_(NAN)
            call_grouped(arr, len(probs), code, ws, reported)
            got = big.cpu()
            assert bool(torch.isnan(got[gaps]).all()), f"{name} {kind}: written between the outputs"
            runs.append(got[~gaps])
            use = 0.0
            for i, ((_, _, ref, mag, _, _), off, (Pn, Q)) in enumerate(zip(probs_h, offs, case.shapes)):
                o_i = got[off:off + Pn * Q].view(Pn, Q)
                what = f"{name} {kind} problem {i} ({Pn} x {Q}, launch {i // step}, {'workspace' if ws is not None else 'no workspace'})"
                if kind == "exact":
                    bad = o_i.double() != ref
                    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements differ from the exact product, first at {tuple(int(j) for j in bad.nonzero()[0])}"
                elif case.f8:
                    assert rel(o_i, ref) < 4e-5, (what, rel(o_i, ref))
                    use = max(use, rel(o_i, ref) / 4e-5)
                else:
                    K = case.R + 1 if ws is not None and is_cut[i] else case.R
                    use = max(use, P.assert_within_rounding(o_i, ref, mag * (K * 2.0 ** -24), ulps=0, name=what))
            if kind == "randn":
                _note(("grouped fp8, whole-problem error / 4e-5" if case.f8 else "grouped bf16") + (" halves" if ws is not None else ""), use)
        assert torch.equal(runs[1], runs[2]) and torch.equal(runs[2], runs[3]), f"{name} {kind}: runs on one workspace differ"
        assert status(buf, reported) == 0
        assert guard_untouched(buf, reported), f"{name}: bytes behind the reported workspace size were written"
