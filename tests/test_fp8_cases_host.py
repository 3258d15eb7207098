"""tests/fp8_cases.py on the CPU: the hand-written OCP encoder against torch's cast (two independent implementations of the
rounding), the kernel names the library's launch plan can return against the hipLaunchKernelGGL targets of csrc/fp8.hip (read
from the source text), the case tables of tests/test_gpu_fp8_casts.py against that plan (every branch is reached by a named case), the comparison the GPU test judges with against planted
defects (each one must be refused), and the scale rule of dg_fp8_scale_of over a sweep of amax."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp8_cases as F  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TORCH_FMT = {F.E4M3: torch.float8_e4m3fn, F.E5M2: torch.float8_e5m2}


def _src(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _torch_codes(w, fmt):
    return torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32)).to(TORCH_FMT[fmt]).view(torch.uint8).numpy()


# --------------------------------------------------------------------------------------------------------------------- encoder
@pytest.mark.parametrize("fmt", F.FORMATS)
def test_encoder_equals_torch_cast(fmt):
    """every finite bf16 pattern at three scales and the whole boundary set: not one byte differs"""
    fmax = F.FMAX[fmt]
    x = F.to_f32(F.bf16_patterns())
    assert x.size == 65280 and np.all(np.isfinite(x))
    n = 0
    for amax in (fmax, fmax * 2.0 ** -7, fmax * 0.3, float(x.max())):
        with np.errstate(over="ignore"):
            w = F.clamp(x * F.scale_of(amax, fmax), fmax)
        got, ref = F.encode(w, fmt), _torch_codes(w, fmt)
        assert np.array_equal(got, ref), np.nonzero(got != ref)[0][:5]
        n += 1
    assert n >= 3
    t = F.boundary_targets(fmt).numpy()
    w = F.clamp(t, fmax)
    got, ref = F.encode(w, fmt), _torch_codes(w, fmt)
    assert np.array_equal(got, ref), [(float(w[i]), int(got[i]), int(ref[i])) for i in np.nonzero(got != ref)[0][:5]]
    # the set does hold what it is for: exact ties, both neighbours of each, FMAX, the smallest subnormal's half, both zeros
    pts = F.code_points(fmt)
    assert pts[-1] == fmax and len(pts) == (126 if fmt == F.E4M3 else 123)
    ties = (pts[:-1] + pts[1:]) / 2
    assert np.all(np.isin(ties.astype(np.float32), t)) and np.float32(pts[0] / 2) in t and np.float32(-fmax) in t
    assert np.any((t == 0) & np.signbit(t)) and np.any((t == 0) & ~np.signbit(t))
    # a tie goes to the even code, its neighbours to their own side; zero keeps its sign; NaN is the format's NaN
    lo = F.encode(np.nextafter(ties.astype(np.float32), np.float32(0)), fmt)
    hi = F.encode(np.nextafter(ties.astype(np.float32), np.float32(np.inf)), fmt)
    mid = F.encode(ties.astype(np.float32), fmt)
    assert np.all(hi == lo + 1) and np.all((mid == lo) | (mid == hi)) and np.all(mid % 2 == 0)
    assert F.encode(np.float32([0.0, -0.0]), fmt).tolist() == [0x00, 0x80]
    assert F.is_nan_code(F.encode(np.float32([np.nan]), fmt), fmt).all()
    assert np.array_equal(F.decode(F.encode(pts.astype(np.float32), fmt), fmt), pts)


def test_planted_encoders_differ_from_the_real_one():
    for fmt in F.FORMATS:
        w = F.clamp(F.boundary_targets(fmt).numpy(), F.FMAX[fmt])
        real = F.encode(w, fmt)
        for kw in (dict(rounding="trunc"), dict(rounding="away"), dict(fnuz=True)):
            assert np.any(F.encode(w, fmt, **kw) != real), kw


# --------------------------------------------------------------------------------------------------------------------- the plan
def test_plan_kernel_names_are_the_launch_targets():
    hip = _src("drakegpt_amd", "csrc", "fp8.hip")
    targets = set(re.findall(r"hipLaunchKernelGGL\(\(?(fp8_\w+)", hip))
    assert targets == {"fp8_amax_kernel", "fp8_quantize_kernel", "fp8_quantize_delayed_kernel"}
    names = {F.amax_geometry(d, 1003).kernel for d in F.DTYPES} | {F.quantize_geometry(d, 16).kernel for d in F.DTYPES}
    names |= {F.quantize_geometry(F.BF16, 32, [(0, 16), (16, 16)]).kernel} | {F.delayed_geometry(d, 16).kernel for d in F.DTYPES}
    assert names == targets
    # the launch sites take their geometry from the plan: one launch per entry, each behind a call of fp8_plan
    entries = ["dg_fp8_amax", "dg_fp8_quantize", "dg_fp8_quantize_delayed", "dg_debug_fp8_plan"]
    at = [hip.index(f'extern "C" int {e}(') for e in entries]
    assert at == sorted(at)
    for e, lo, hi, kernel in zip(entries, at, at[1:], ("fp8_amax_kernel", "fp8_quantize_kernel", "fp8_quantize_delayed_kernel")):
        body = hip[lo:hi]
        assert "fp8_plan(" in body and "fp8_check(" in body and re.findall(r"hipLaunchKernelGGL\(\(?(fp8_\w+)", body) == [kernel], e
        assert "dim3(pl.grid), dim3(pl.block)" in body, e
    assert hip.count("hipLaunchKernelGGL") == 3 and "fp8_plan(" in hip[at[3]:]
    # the ABI constant, and the constants of the scale rule as the library holds them
    assert int(re.search(r"#define DG_FP8_AMAX_PARTS (\d+)", _src("include", "drakegpt_hip.h")).group(1)) == F.AMAX_PARTS
    assert F.delayed_geometry(F.BF16, 16).grid == F.AMAX_PARTS == F.amax_geometry(F.BF16, 16).wgs
    assert F.constants() == (np.float32(F.FMAX[F.E4M3]), np.float32(F.FMAX[F.E5M2]), F.SCALE_CAP)


def test_plan_values():
    g = F.quantize_geometry(F.BF16, 16 * 1024 * 2 + 16, q_off=8)
    assert g[:2] + g[3:] == (5, 0, "fp8_quantize_kernel", 256, 5)
    assert g.segs == (F.SegGeo(0, 32784, False, ("q_align",), 4098, 4, 5, 0),)
    g = F.delayed_geometry(F.F32, 2 ** 22 + 2 ** 15 + 16)
    assert g[:2] + g[3:] == (256, 0, "fp8_quantize_delayed_kernel", 1024, 256)
    assert g.segs == (F.SegGeo(0, 4227088, True, (), 264193, 2, 256, 0),)
    g = F.amax_geometry(F.F32, 1003)
    assert g == F.AmaxGeo(256, (F.AmaxSeg(0, 1003, 4, 250, 3, 1, 255),), "fp8_amax_kernel", 256, 256)
    g = F.quantize_geometry(F.F32, 4096, [(8, 1024), (2048, 2048)])
    assert (g.grid, g.bps, g.wgs) == (2, 1, 1) and [s.why for s in g.segs] == [("first", "q_align"), ()]
    assert F.amax_geometry(F.BF16, 4096, [(8, 1024), (2048, 2048)]).grid == 2 * F.AMAX_PARTS
    # a real address decides as an offset does
    assert F.quantize_geometry(F.BF16, 32, x_addr=4096, q_addr=4104).segs[0].why == ("q_align",)


# --------------------------------------------------------------------------------------------------------------------- coverage
def test_every_branch_is_reached_by_a_named_case():
    reached = set()
    qc, dc, ac = F.quantize_cases(), F.delayed_cases(), F.amax_cases()
    assert len({c.name for c in qc + dc + ac}) == len(qc + dc + ac)
    for c in qc:
        geo = F.geometry_of(c)
        if c.seg is None:
            s, e = geo.segs[0], c.expect
            assert (s.wide, s.why, s.trips, geo.grid) == (e["wide"], e["why"], e["trips"], e["grid"]), (c.name, geo)
            reached.add(("quantize", c.dtype, c.fmt, "wide" if s.wide else "narrow:" + "+".join(s.why)))
            if s.trips > 1:
                reached.add(("quantize", c.dtype, c.fmt, "wide second trip" if s.wide else "narrow second trip"))
            if geo.grid > 1:
                reached.add(("quantize", c.dtype, c.fmt, "several workgroups"))
            if s.units % geo.block and geo.grid > 1:
                reached.add(("quantize", c.dtype, c.fmt, "ragged last workgroup"))
        else:
            layout, n = F.seg_layout(c.seg)
            kinds = [k for k, *_ in layout]
            assert kinds == [k for k, *_ in (F.SEG_SPEC[::-1] if c.seg else F.SEG_SPEC)] and n == c.n
            by = dict(zip(kinds, geo.segs))
            assert by["wide"].wide and by["wide_100x"].wide and by["wide_after"].wide
            # (a start at 8 mod 16 moves the output of that segment off the 16-byte boundary with it: both terms are false)
            assert by["narrow_first"].why == ("first", "q_align") and by["narrow_first"].len % 16 == 0
            assert by["narrow_len"].why == ("len",) and by["eight"].why == ("len",) and by["eight"].len == 8
            assert by["wide_100x"].len == 100 * by["wide"].len
            # blocks_per_seg follows the mean: the large segment takes many trips, the small ones leave whole workgroups idle
            assert geo.bps == 3 and geo.grid == geo.bps * 6                  # (neither clamp of blocks_per_seg: the header names both)
            assert by["wide_100x"].trips >= 8 and by["wide_100x"].idle == 0
            assert all(by[k].idle == geo.bps - 1 for k in kinds if k != "wide_100x")
            # gaps: segments do not touch where a gap was asked for, and never overlap
            ends = [0] + [f + l for _, f, l, _ in layout]
            assert all(f >= e for (_, f, _, _), e in zip(layout, ends)) and any(f > e for (_, f, _, _), e in zip(layout, ends))
            order = ["wide" if s.wide else "narrow" for s in geo.segs]
            reached.add(("segments", c.dtype, c.fmt, "reversed" if c.seg else "forward"))
            if "narrow" in order[order.index("wide"):] and "wide" in order[order.index("narrow"):]:
                reached.add(("segments", c.dtype, c.fmt, "wide and narrow in both orders"))
            reached.add(("segments", c.dtype, c.fmt, "many trips next to idle workgroups"))
            reached |= {("segments", c.dtype, c.fmt, "narrow:" + s.why[0]) for s in geo.segs if not s.wide}
    for c in dc:
        geo = F.geometry_of(c)
        s, e = geo.segs[0], c.expect
        assert (s.wide, s.why, s.trips, s.idle) == (e["wide"], e["why"], e["trips"], e["idle"]), (c.name, geo)
        if "second" in e:        # workgroups whose threads make a second trip
            assert F._cdiv(s.units - geo.wgs * geo.block, geo.block) == e["second"]
        assert c.step in F.STEPS
        reached.add(("delayed", c.dtype, c.fmt, "wide" if s.wide else "narrow:" + "+".join(s.why)))
        if s.trips > 1:
            reached.add(("delayed", c.dtype, c.fmt, "wide second trip" if s.wide else "narrow second trip"))
        if s.idle:
            reached.add(("delayed", c.dtype, c.fmt, "idle workgroups"))
        reached.add(("delayed step", c.step))
    for c in ac:
        s = F.geometry_of(c).segs[0]
        at = F.amax_where(c.dtype, c.n, c.expect)
        assert s.tail, c.name                                    # every n of the table leaves a tail
        if c.expect == "tail":
            assert at >= s.nv * s.vec
        elif c.expect == "last_vector" and s.nv:
            assert s.nv * s.vec - s.vec <= at < s.nv * s.vec
        reached.add(("amax", c.dtype, "tail"))
        reached.add(("amax", c.dtype, "no vector" if s.nv == 0 else "second trip" if s.trips > 1 else "one trip"))
        if s.idle:
            reached.add(("amax", c.dtype, "idle workgroups"))
    want = set()
    for dtype in F.DTYPES:
        for fmt in F.FORMATS:
            want |= {("quantize", dtype, fmt, b) for b in ("wide", "narrow:len", "narrow:q_align", "wide second trip", "narrow second trip",
                                                         "several workgroups", "ragged last workgroup")}
            want |= {("segments", dtype, fmt, b) for b in ("forward", "reversed", "wide and narrow in both orders",
                                                         "many trips next to idle workgroups", "narrow:first", "narrow:len")}
            want |= {("delayed", dtype, fmt, b) for b in ("wide", "narrow:len", "narrow:q_align", "wide second trip", "narrow second trip",
                                                        "idle workgroups")}
        want |= {("amax", dtype, b) for b in ("tail", "no vector", "one trip", "second trip", "idle workgroups")}
    want |= {("delayed step", s) for s in F.STEPS}
    assert want <= reached, sorted(map(str, want - reached))
    # the step words: parity 0, 1, 1 and the wrap to 0
    assert [s & 1 for s in F.STEPS] == [0, 1, 1] and (F.STEPS[2] + 1) & 0xFFFFFFFF == 0


def test_geometry_refuses_what_the_entries_refuse():
    for bad in (dict(n=12), dict(n=16, q_off=4), dict(n=16, x_off=8)):
        with pytest.raises(AssertionError):
            F.quantize_geometry(F.BF16, **bad)
        with pytest.raises(AssertionError):
            F.delayed_geometry(F.F32, **bad)
        # the refusal is the entry's own return code, from the checks the entries themselves run
        n, x, q = bad["n"], F.BASE + bad.get("x_off", 0), F.BASE + bad.get("q_off", 0)
        assert F.plan_rc("quantize", F.BF16, n, None, x, q)[0] == F.DG_ERR_ARG and F.plan_rc("delayed", F.F32, n, None, x, q)[0] == F.DG_ERR_ARG
    assert F.plan_rc("quantize", F.BF16, 16)[0] == 0 and F.plan_rc("delayed", F.F32, 16, None, F.BASE, F.BASE + 8)[0] == 0
    assert F.plan_rc("amax", F.BF16, 12)[0] == 0 and F.plan_rc("amax", F.BF16, 16, None, F.BASE + 8)[0] == F.DG_ERR_ARG


def test_partials_model_follows_the_loops():
    """the per-workgroup maxima against a plain loop over (workgroup, thread, trip) at a small size"""
    g = torch.Generator().manual_seed(2)
    x = torch.randn(8 * 1024 * 3 + 8 * 5, generator=g).numpy()
    geo = F.delayed_geometry(F.F32, x.size)
    assert not geo.segs[0].wide
    ref = np.zeros(F.AMAX_PARTS, dtype=np.float32)
    for i in range(x.size // 8):
        b = (i // 1024) % F.AMAX_PARTS
        ref[b] = max(ref[b], np.abs(x[i * 8:i * 8 + 8]).max())
    assert np.array_equal(F.delayed_partials(x, geo), ref)
    y = x[:1003]
    ageo = F.amax_geometry(F.F32, y.size)
    sg = ageo.segs[0]
    ref = np.zeros(F.AMAX_PARTS, dtype=np.float32)
    for i in range(sg.nv):
        b = (i // 256) % F.AMAX_PARTS
        ref[b] = max(ref[b], np.abs(y[i * 4:i * 4 + 4]).max())
    ref[0] = max(ref[0], np.abs(y[sg.nv * 4:]).max())
    assert np.array_equal(F.amax_partials(y, sg, ageo), ref)
    assert F.amax_bits(np.float32([-0.0, -0.0])).view(np.uint32) == 0
    assert np.isnan(F.amax_bits(np.float32([1.0, np.inf, -np.nan]))) and np.isinf(F.amax_bits(np.float32([1.0, -np.inf])))


# --------------------------------------------------------------------------------------------------------------------- planted defects
def _got(want):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in want.items() if k not in ("amax", "idle", "q_start")}


def _refused(got, want, fmt):
    with pytest.raises(AssertionError):
        F.compare(got, want, fmt, "planted")


@pytest.mark.parametrize("fmt", F.FORMATS)
def test_planted_defects_are_refused(fmt):
    # rounding: the boundary set through the delayed entry's model, scale 2^7
    _, amax, p2 = F.boundary_amaxes(fmt)[1]
    xb = F.boundary_sources(fmt, amax, p2)
    prev = F.read_slot(amax)
    want = F.expect_delayed(xb, fmt, 0, prev)
    assert F.compare(_got(want), want, fmt)                     # the model itself passes, scale_inv exact
    for kw in (dict(rounding="trunc"), dict(rounding="away"), dict(fnuz=True)):
        got = _got(want)
        got["q"] = F.expect_delayed(xb, fmt, 0, prev, **kw)["q"]
        _refused(got, want, fmt)
    # stores: one 8-byte store skipped, one 16-byte store 8 bytes late (in the middle, and the last one: into the guard band)
    x, _ = F.planted_source(F.BF16, 4096, 3)
    want = F.expect_delayed(x, fmt, 0, prev)
    s = F.BAND
    got = _got(want)
    got["q"][s + 80:s + 88] = F.Q_SENTINEL
    _refused(got, want, fmt)
    for at in (s + 256, s + 4096 - 16):
        got = _got(want)
        chunk = want["q"][at:at + 16].copy()
        got["q"][at:at + 8] = F.Q_SENTINEL
        got["q"][at + 8:at + 24] = chunk
        _refused(got, want, fmt)
    # the history: a zero partial in the recorded slot (the one that holds the maximum, and another one), the read slot overwritten
    x2, _ = F.planted_source(F.F32, 8 * 1024 * 4 + 8, 4)
    want = F.expect_delayed(x2, fmt, 0, prev)
    assert np.count_nonzero(want["written"]) == 5 and want["idle"] == 251
    for b in (int(np.argmax(want["written"])), int(np.argmin(want["written"][:5]))):
        got = _got(want)
        got["written"][b] = 0.0
        _refused(got, want, fmt)
    got = _got(want)
    got["written"][200] = want["written"][0] * 0.5              # an idle workgroup that recorded something
    _refused(got, want, fmt)
    got = _got(want)
    got["read"][:] = want["written"]
    _refused(got, want, fmt)
    got = _got(want)
    got["read"][5] = np.nextafter(got["read"][5], np.float32(0))
    _refused(got, want, fmt)
    # segments: a segment scaled with its neighbour's amax, scale_inv of the wrong segment, a stray write into a gap
    xs, table, amaxes = F.seg_source(F.BF16)
    want = F.expect_quantize(xs, fmt, 0, table)
    assert np.array_equal(want["scale_inv"], [F.scale_inv_of(F.scale_of(a, F.FMAX[fmt])) for a in amaxes])
    assert F.compare(_got(want), want, fmt)
    (f0, l0), (f1, l1) = table[0], table[1]
    got = _got(want)
    got["q"][s + f0:s + f0 + l0] = F.model_cast(F.to_f32(xs[f0:f0 + l0]), amaxes[1], fmt)[0]
    _refused(got, want, fmt)
    got = _got(want)
    got["scale_inv"][[0, 1]] = got["scale_inv"][[1, 0]]
    _refused(got, want, fmt)
    got = _got(want)
    got["q"][s + f0 + l0] = 0
    _refused(got, want, fmt)
    got = _got(want)
    got["parts"][F.AMAX_PARTS * 2 + 9] = 1.0e6                   # a filler leaked into a partial
    _refused(got, want, fmt)
    got = _got(want)
    got["x"][7] ^= 1
    _refused(got, want, fmt)
    # scale_inv two ulps off is refused, one ulp is not (and is reported as inexact)
    got = _got(want)
    got["scale_inv"][3] = np.nextafter(np.nextafter(got["scale_inv"][3], np.float32(1)), np.float32(1))
    _refused(got, want, fmt)
    got = _got(want)
    got["scale_inv"][3] = np.nextafter(got["scale_inv"][3], np.float32(1))
    assert F.compare(got, want, fmt) is False
    # tiny amax: the scale without its cap turns 0 into NaN, everything else into +-FMAX, scale_inv into 0
    for name, dtype, f, amax in F.tiny_cases():
        if f != fmt:
            continue
        xt, held = F.tiny_source(amax, dtype)
        assert held == amax and F.amax_bits(F.to_f32(xt)) == amax
        want = F.expect_quantize(xt, fmt)
        view = want["q"][s:s + xt.numel()]
        zeros = F.to_f32(xt) == 0
        assert zeros.sum() >= 8 and np.all((view[zeros] & 0x7F) == 0) and not F.is_nan_code(view, fmt).any()
        assert np.isfinite(want["scale_inv"][0]) and want["scale_inv"][0] >= np.finfo(np.float32).tiny
        got = _got(want)
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            inf_scale = np.float32(F.FMAX[fmt]) / amax
            assert np.isinf(inf_scale)
            got["q"][s:s + xt.numel()] = F.encode(F.clamp(F.to_f32(xt) * inf_scale, F.FMAX[fmt]), fmt)
        assert F.is_nan_code(got["q"][s:s + xt.numel()][zeros], fmt).all()
        _refused(got, want, fmt)
        got = _got(want)
        got["scale_inv"][0] = 0.0
        _refused(got, want, fmt)


# --------------------------------------------------------------------------------------------------------------------- scale rule
@pytest.mark.parametrize("fmt", F.FORMATS)
def test_scale_rule_over_a_sweep_of_amax(fmt):
    fmax = np.float32(F.FMAX[fmt])
    flt_max, tiny = np.finfo(np.float32).max, np.finfo(np.float32).tiny
    edge = fmax / flt_max
    with np.errstate(over="ignore"):
        assert np.isinf(fmax / np.nextafter(edge, np.float32(0))) and np.isfinite(fmax / np.nextafter(edge, np.float32(1)))
    assert F.scale_of(0.0, fmax) == 1 and F.scale_of(-0.0, fmax) == 1
    assert np.isnan(F.scale_of(np.inf, fmax)) and np.isnan(F.scale_of(np.nan, fmax))
    sweep = [np.float32(1e-45), np.float32(1e-40), np.nextafter(tiny, np.float32(0)), tiny, np.float32(1e-37),
             np.nextafter(edge, np.float32(0)), edge, np.nextafter(edge, np.float32(1)), fmax * np.float32(2.0 ** -126),
             np.nextafter(fmax * np.float32(2.0 ** -126), np.float32(1)), np.float32(1.0), fmax, flt_max]
    for a in [np.float32(0.0), np.float32(-0.0), np.float32(np.inf), np.float32(np.nan)] + sweep:      # the library's own function, bit for bit
        assert F.lib_scale_of(a, fmt).view(np.uint32) == np.float32(F.scale_of(a, fmax)).view(np.uint32) or (np.isnan(F.lib_scale_of(a, fmt)) and np.isnan(F.scale_of(a, fmax))), a
    for a in sweep:
        sc = F.scale_of(a, fmax)
        si = F.scale_inv_of(sc)
        assert np.isfinite(sc) and 0 < sc <= F.SCALE_CAP, (a, sc)
        assert np.isfinite(si) and si >= tiny, (a, si)                      # a positive NORMAL dequantisation factor
        with np.errstate(over="ignore"):
            q = fmax / a
        if a >= fmax * np.float32(2.0 ** -126):
            assert sc.view(np.uint32) == q.view(np.uint32), a               # at and above FMAX * 2^-126: bit-identical to the quotient
        else:
            assert sc == F.SCALE_CAP and q > F.SCALE_CAP
        assert a * sc <= fmax and np.float32(0.0) * sc == 0                  # amax lands inside the range, zero stays zero
    assert np.all(np.diff([F.scale_of(a, fmax) for a in sweep]) <= 0)       # monotone: a larger amax never gets a larger scale
