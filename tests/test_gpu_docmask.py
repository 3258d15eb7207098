"""Document-masked attention on the device: dg_doc_starts, dg_attn_fwd_doc and dg_attn_bwd_doc (ops.doc_starts, ops.attn_fwd /
ops.attn_bwd with doc_starts=) against the stitched fp64 reference of tests/docmask_cases.py, for the bf16 MFMA instances (DOC
template flag of attn_fwd_mfma_kernel and attn_bwd_dq_mfma_kernel, per-wave and shared dQ form, with and without keep bits, with
the fp8 copies) and for the generic kernels (fp32, and bf16 shapes the MFMA family does not cover).

Bounds: the project's own (oracle/parity.py), as in tests/test_gpu_attention_instances.py -- forward 8e-3 per (row, head) and
inside attention_fwd_envelope, lse to 1e-5, dead rows exactly zero; backward per group BWD_MARGIN x the rounding model's worst
group nearby, "nearby" taken over the offset inside the document (docmask_cases.bwd_bounds_by_offset, and why).  Each case
asserts, with the device's CU count, the block order it is named for.  The structural tests need no reference: one document is
the plain entry, a (batch, head) slab is a launch of its own, nothing before a boundary reaches anything behind it (bit for
bit), and on the generic kernels every document is bit for bit the plain launch on that document alone.

measured on MI355X (256 CUs), worst (row, head) kernel / CPU rounding model, "use" = largest error / bound over the groups
(elements for the forward envelope), < 1 passes; the tiles and the keep-bits form agree to the digits shown; lse within 2e-7:
  case (B, T, NH, p)              forward (env. use)  dq                       dk                       dv
  doc-one-tile (2, 32, 3, 0)      2.8e-3 (0.84)       5.5e-2 / 5.5e-2 (0.33)   1.0e-2 / 1.7e-2 (0.20)   3.5e-3 / 3.5e-3 (0.33)
  doc-one-tile (2, 32, 3, 0.2)    4.1e-3 (0.83)       2.1e-1 / 2.1e-1 (0.33)   3.0e-1 / 3.0e-1 (0.33)   4.1e-3 / 4.1e-3 (0.33)
  doc-ragged (3, 66, 3, 0)        2.8e-3 (0.75)       5.5e-2 / 1.2e-1 (0.23)   5.2e-2 / 1.3e-1 (0.28)   3.8e-3 / 3.8e-3 (0.33)
  doc-ragged (3, 66, 3, 0.2)      3.5e-3 (0.75)       1.3e-1 / 1.5e-1 (0.31)   1.8e-1 / 1.8e-1 (0.33)   4.0e-3 / 4.0e-3 (0.33)
  doc-pairs (2, 128, 3, 0)        2.9e-3 (0.68)       1.5e-1 / 7.8e-2 (0.63)   6.8e-3 / 9.5e-3 (0.32)   4.0e-3 / 4.0e-3 (0.33)
  doc-pairs (2, 128, 3, 0.2)      3.9e-3 (0.82)       1.4e-1 / 1.4e-1 (0.33)   1.1e-2 / 1.0e-2 (0.46)   3.9e-3 / 3.9e-3 (0.33)
  doc-heavy (1, 512, 3, 0)        3.1e-3 (0.66)       8.1e-2 / 1.3e-1 (0.44)   5.9e-3 / 7.0e-3 (0.38)   4.1e-3 / 4.1e-3 (0.33)
  doc-heavy (1, 512, 3, 0.2)      3.4e-3 (0.69)       2.0e-1 / 2.0e-1 (0.37)   4.0e-2 / 4.0e-2 (0.41)   3.8e-3 / 3.8e-3 (0.33)
(dk's worst groups are the last keys of a document, dq's the first queries: one or two terms, the near-cancellation of
oracle/parity.py's attention_bwd_bounds_by_position.)  Generic kernels at p = 0.1: fp32 forward 2e-7 .. 7e-7, backward <= 2.3e-5
(use <= 0.51); bf16 (2, 255, 2, 64): forward 2.2e-3, backward use <= 0.31."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_cases as A  # noqa: E402
import docmask_cases as D  # noqa: E402
from oracle import parity as P  # noqa: E402
from oracle import rng_ref  # noqa: E402

pytestmark = pytest.mark.gpu

H = A.HD
E4, E5 = torch.float8_e4m3fn, torch.float8_e5m2
FORMS = ("tiles", "keep_bits")                 # (the recompute form has no document variant: refused)


def _ops():
    from drakegpt_amd import ops
    return ops


def _report(msg):
    if os.environ.get("DG_TEST_REPORT"):
        print("[parity] " + msg, flush=True)


def _case(dev, name):
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    c = D.case(name)
    assert A.supported(c.B, c.T, c.NH) and _ops().attn_fp8_out_supported(c.B, c.T, c.NH, H, torch.bfloat16)        # the MFMA family runs
    assert A.order(c.B, c.T, c.NH, ncu)[0] == c.order, (c, ncu)
    assert A.plan(A.call(0, c.B, c.T, c.NH, ncu=0)).rot_div == ncu           # the library plans for this device
    # the document-mask instances: the shared dQ form in the heavy-first order only, the shared tile pass in the balanced orders
    b = lambda x: "true" if x else "false"
    for p in D.PS:
        for form in FORMS:
            kb = form == "keep_bits" and p > 0
            assert A.instances(c.B, c.T, c.NH, p, ncu, form, doc=True) == (
                f"attn_fwd_mfma_kernel<{b(p > 0)},{b(kb)},false,true>", f"attn_bwd_dq_mfma_kernel<true,{b(kb)},false,{b(c.order == 2)},true>",
                "attn_bwd_dkv_tiles_shared_kernel" if c.order else "attn_bwd_dkv_tiles_kernel"), (c, p, form)
        assert A.instances(c.B, c.T, c.NH, p, ncu, "keep_bits" if p > 0 else "tiles", "both", doc=True) == (
            f"attn_fwd_mfma_kernel<{b(p > 0)},{b(p > 0)},true,true>", f"attn_bwd_dq_mfma_kernel<true,{b(p > 0)},true,{b(c.order == 2)},true>",
            "attn_bwd_dkv_tiles_shared_f8_kernel" if c.order else "attn_bwd_dkv_tiles_f8_kernel"), (c, p)
    return c


def _rng(dev, p, step=A.STEP):
    return _ops().new_rng_state(A.SEED, dev, step) if p > 0 else None


def _poison(dev, *shapes):
    """as tests/test_gpu_attention_instances.py: NaN-filled tensors of the outputs' sizes, released just before the launch"""
    for shape, dtype in shapes:
        torch.full(shape, float("nan"), dtype=dtype, device=dev)
    torch.cuda.synchronize()


def _same_up_to_contraction(a, b):
    """the criterion of the keep-bits form against the hashed form (tests/test_gpu_attention_instances.py)"""
    a, b = a.float(), b.float()
    assert bool(((a - b).abs() <= 2.0 ** -6 * torch.maximum(a.abs(), b.abs()) + 1e-6 * b.abs().max()).all())
    r = ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()
    assert r < 2e-4, r


def _forward(dev, c, p, R):
    ops = _ops()
    B, T, NH = c.B, c.T, c.NH
    tag = f"docmask {c.name} {(B, T, NH, H, p)}"
    qkv, st = R["qkv"].to(dev), R["starts"].to(dev)
    _poison(dev, ((B * T, NH * H), torch.bfloat16), ((B, NH, T), torch.float32))
    out, lse = ops.attn_fwd(qkv, B, T, NH, H, H ** -0.5, p, _rng(dev, p), A.SITE, doc_starts=st)
    assert getattr(out, "dg_keep", None) is None
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(lse).all())
    wf = P.assert_rowwise(out, R["out"], H, 8e-3, f"{tag} forward", T)
    uf = P.assert_within_rounding(out, R["out"], R["env"], 1, f"{tag} forward")
    el = ((lse.double().cpu() - R["lse"]).abs() / R["lse"].abs().clamp_min(1)).max().item()
    print(f"{tag} forward: worst group {wf:.3e} (bound 8e-3), envelope use {uf:.3f}, lse {el:.2e} (bound 1e-5)")
    assert el < 1e-5, el
    if p > 0:
        dead = R["dead"]
        assert torch.all(out.float().cpu().view(B, T, NH, H).permute(0, 2, 1, 3)[dead] == 0)
        out_k, lse_k = ops.attn_fwd(qkv, B, T, NH, H, H ** -0.5, p, _rng(dev, p), A.SITE, keep=True, doc_starts=st)
        assert out_k.dg_keep.numel() == B * NH * (A.blocks(T) * (A.blocks(T) + 1) // 2) * 128
        assert torch.equal(out_k, out)
        assert ((lse_k.double() - lse.double()).norm() / lse.double().norm()).item() < 1e-6
    _report(f"{tag} forward: worst group {wf:.2e}, envelope use {uf:.2f}, lse {el:.1e}")


def _backward_of(dev, c, p, R, form):
    ops = _ops()
    B, T, NH = c.B, c.T, c.NH
    qkv, dout, st = R["qkv"].to(dev), R["dout"].to(dev), R["starts"].to(dev)
    out, lse = ops.attn_fwd(qkv, B, T, NH, H, H ** -0.5, p, _rng(dev, p), A.SITE, keep=form == "keep_bits", doc_starts=st)
    bits = getattr(out, "dg_keep", None)
    assert (bits is not None) == (form == "keep_bits" and p > 0)
    _poison(dev, (tuple(qkv.shape), torch.bfloat16))
    return ops.attn_bwd(qkv, out, dout, lse, B, T, NH, H, H ** -0.5, p, _rng(dev, p), A.SITE, keep_bits=bits, doc_starts=st)


def _backward(dev, c, p, R, form):
    B, T, NH = c.B, c.T, c.NH
    C = NH * H
    tag = f"docmask {c.name} {(B, T, NH, H, p)} backward ({form})"
    dqkv = _backward_of(dev, c, p, R, form)
    assert bool(torch.isfinite(dqkv.float()).all())
    for i, n in enumerate(("dq", "dk", "dv")):
        got = dqkv.view(B * T, 3, C)[:, i]
        e = P.rowwise_rel(got, R[n], H, R["floors"][n])
        print(f"{tag} {n}: worst group {e.max().item():.3e}, model's worst {R['model_worst'][n]:.3e}, "
              f"largest error / bound {(e / R['bounds'][n].clamp_min(1e-300)).max().item():.3f}")
        P.assert_rowwise_each(got, R[n], H, R["bounds"][n], f"{tag} {n}", T, floor=R["floors"][n])


CHECKS = [(name, p, what) for name, p in D.CASE_P for what in ("forward",) + FORMS + (("keep_bits_against_hashed",) if p > 0 else ())]


@pytest.mark.parametrize("name,p,what", CHECKS, ids=[f"{n}-p{p:g}-{w}" for n, p, w in CHECKS])
def test_case(dev, name, p, what):
    """one parametrisation per (case, p, check), case-major: the checks of a case share its CPU reference"""
    c = _case(dev, name)
    R = D.reference(name, p)
    if what == "forward":
        _forward(dev, c, p, R)
    elif what == "keep_bits_against_hashed":
        _same_up_to_contraction(_backward_of(dev, c, p, R, "keep_bits"), _backward_of(dev, c, p, R, "tiles"))
    else:
        _backward(dev, c, p, R, what)


def test_recompute_form_is_refused_with_doc_starts(dev):
    """the recompute dK/dV kernel has no document variant: ops raises ValueError, the C entry returns DG_ERR_ARG; the generic
    kernels (no tile scratch at all) take doc_starts with either setting"""
    from drakegpt_amd import _lib
    ops = _ops()
    c = _case(dev, "doc-pairs")
    B, T, NH = c.B, c.T, c.NH
    qkv, dout = (t.to(dev) for t in A.operands(B, T, NH, c.draw))
    st = D.starts_tensor(B, T, c.firsts).to(dev)
    out, lse = ops.attn_fwd(qkv, B, T, NH, H, H ** -0.5, 0.0, None, A.SITE, doc_starts=st)
    with pytest.raises(ValueError):
        ops.attn_bwd(qkv, out, dout, lse, B, T, NH, H, H ** -0.5, 0.0, None, A.SITE, tile_scratch=False, doc_starts=st)
    dqkv = torch.empty_like(qkv)
    ws = torch.empty(B * NH * T * 4, dtype=torch.uint8, device=dev)
    args = (qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dqkv.data_ptr(), ws.data_ptr(), ws.numel(), B, T, NH, H,
            H ** -0.5, 0.0, None, A.SITE, ops.dt_code(torch.bfloat16), None, 0, None)
    assert _lib.lib.dg_attn_bwd_doc(*args, st.data_ptr(), None) == -1          # DG_ERR_ARG, before any launch
    torch.cuda.synchronize()
    q32, d32 = qkv.float(), dout.float()
    o32, l32 = ops.attn_fwd(q32, B, T, NH, H, H ** -0.5, 0.0, None, A.SITE, doc_starts=st)
    a = ops.attn_bwd(q32, o32, d32, l32, B, T, NH, H, H ** -0.5, 0.0, None, A.SITE, tile_scratch=False, doc_starts=st)
    b = ops.attn_bwd(q32, o32, d32, l32, B, T, NH, H, H ** -0.5, 0.0, None, A.SITE, doc_starts=st)
    assert torch.equal(a, b)


@pytest.mark.parametrize("name,p", [("doc-ragged", 0.2), ("doc-pairs", 0.0), ("doc-heavy", 0.2)])
def test_one_document_is_the_plain_entry(dev, name, p):
    """starts all zero: out bit for bit and lse within 1e-6 relative of the plain entry, dqkv up to contraction (other template
    instances of the same fp32 expressions)"""
    ops = _ops()
    c = _case(dev, name)
    B, T, NH = c.B, c.T, c.NH
    qkv, dout = (t.to(dev) for t in A.operands(B, T, NH, c.draw))
    st = torch.zeros(B * T, dtype=torch.int32, device=dev)
    o0, l0 = ops.attn_fwd(qkv, B, T, NH, H, H ** -0.5, p, _rng(dev, p), A.SITE, keep=True)
    g0 = ops.attn_bwd(qkv, o0, dout, l0, B, T, NH, H, H ** -0.5, p, _rng(dev, p), A.SITE)
    _poison(dev, ((B * T, NH * H), torch.bfloat16), ((B, NH, T), torch.float32))
    o1, l1 = ops.attn_fwd(qkv, B, T, NH, H, H ** -0.5, p, _rng(dev, p), A.SITE, keep=True, doc_starts=st)
    _poison(dev, (tuple(qkv.shape), torch.bfloat16))
    g1 = ops.attn_bwd(qkv, o1, dout, l1, B, T, NH, H, H ** -0.5, p, _rng(dev, p), A.SITE, doc_starts=st)
    assert torch.equal(o1, o0)
    assert ((l1.double() - l0.double()).abs() / l0.double().abs().clamp_min(1e-30)).max().item() < 1e-6
    _same_up_to_contraction(g1, g0)


def test_every_batch_row_reads_its_own_starts(dev):
    """three different layouts in one launch (catches starts[t] read for starts[b*T + t]): each (b, h) slab equals a (1, T, 1)
    launch with its own starts -- out and lse bit for bit, dqkv up to contraction; the pattern of
    test_a_head_does_not_depend_on_the_launch_around_it"""
    ops = _ops()
    B, T, NH = 3, 128, 2
    layouts = [(0, 40, 64, 100), (0, 1, 33, 127), (0, 96)]
    qkv, dout = (t.to(dev) for t in A.operands(B, T, NH, 2))
    st = torch.cat([D.starts_tensor(1, T, f) for f in layouts]).to(dev)
    _poison(dev, ((B * T, NH * H), torch.bfloat16), ((B, NH, T), torch.float32))
    out, lse = ops.attn_fwd(qkv, B, T, NH, H, H ** -0.5, 0.0, None, A.SITE, doc_starts=st)
    _poison(dev, (tuple(qkv.shape), torch.bfloat16))
    dqkv = ops.attn_bwd(qkv, out, dout, lse, B, T, NH, H, H ** -0.5, 0.0, None, A.SITE, doc_starts=st)
    for b in range(B):
        s1 = st.view(B, T)[b].contiguous()
        for h in range(NH):
            q1, d1 = A.slab(qkv, B, T, NH, b, h, 3), A.slab(dout, B, T, NH, b, h, 1)
            o1, l1 = ops.attn_fwd(q1, 1, T, 1, H, H ** -0.5, 0.0, None, A.SITE, doc_starts=s1)
            g1 = ops.attn_bwd(q1, o1, d1, l1, 1, T, 1, H, H ** -0.5, 0.0, None, A.SITE, doc_starts=s1)
            assert torch.equal(o1, A.slab(out, B, T, NH, b, h, 1)), (b, h)
            assert torch.equal(l1.view(T), lse[b, h]), (b, h)
            _same_up_to_contraction(A.slab(dqkv, B, T, NH, b, h, 3), g1)
    # and the layouts do differ in what they compute
    assert not torch.equal(out.view(B, T, -1)[0], out.view(B, T, -1)[1])


@pytest.mark.parametrize("dtype,B,T,NH,Hh,firsts,a,p", [(torch.bfloat16, 2, 128, 2, 64, (0, 40, 64, 100), 64, 0.2),
                                                        (torch.bfloat16, 1, 512, 2, 64, (0, 130, 256, 300, 511), 300, 0.2),
                                                        (torch.float32, 2, 37, 2, 16, (0, 1, 20, 36), 20, 0.1)],
                         ids=["bf16-pairs", "bf16-shared-dq", "fp32"])
def test_nothing_leaks_across_a_boundary(dev, dtype, B, T, NH, Hh, firsts, a, p):
    """K and V rows before the boundary ``a`` replaced with other finite values: out, lse and dq of every row behind the
    boundary, and dk and dv of every key behind it, do not change by a bit"""
    ops = _ops()
    C = NH * Hh
    g = torch.Generator().manual_seed(T + Hh)
    qkv = torch.randn(B * T, 3 * C, generator=g).to(dtype).to(dev)
    dout = torch.randn(B * T, C, generator=g).to(dtype).to(dev)
    other = qkv.clone()
    other.view(B, T, 3, C)[:, :a, 1:] = (torch.randn(B, a, 2, C, generator=g) * 3 + 1).to(dtype).to(dev)
    st = D.starts_tensor(B, T, firsts).to(dev)
    res = []
    for x in (qkv, other):
        out, lse = ops.attn_fwd(x, B, T, NH, Hh, Hh ** -0.5, p, _rng(dev, p), A.SITE, keep=True, doc_starts=st)
        dqkv = ops.attn_bwd(x, out, dout, lse, B, T, NH, Hh, Hh ** -0.5, p, _rng(dev, p), A.SITE, doc_starts=st)
        res.append((out.view(B, T, C)[:, a:], lse[:, :, a:], dqkv.view(B, T, 3 * C)[:, a:]))
    for x, y in zip(*res):
        assert bool(torch.isfinite(x.float()).all()) and torch.equal(x, y)
    # (the rows before the boundary did change: the replacement is seen where it may be)
    assert not torch.equal(ops.attn_fwd(qkv, B, T, NH, Hh, Hh ** -0.5, 0.0, None, A.SITE, doc_starts=st)[0].view(B, T, C)[:, :a],
                           ops.attn_fwd(other, B, T, NH, Hh, Hh ** -0.5, 0.0, None, A.SITE, doc_starts=st)[0].view(B, T, C)[:, :a])


# the generic kernels: fp32, and bf16 at an odd T.  Boundaries include 0, 1 and T - 1; one document longer than a wave (64 keys);
# in the bf16 case every document has an odd length, so that the plain launch on it takes the generic kernels as well
GENERIC = [(torch.float32, 2, 8, 4, 8, (0, 1, 4, 7)), (torch.float32, 3, 37, 2, 16, (0, 1, 20, 36)),
           (torch.float32, 2, 130, 2, 64, (0, 1, 50, 129)), (torch.bfloat16, 2, 255, 2, 64, (0, 1, 100, 253, 254))]
GENERIC_IDS = ["fp32-T8-H8", "fp32-T37-H16", "fp32-T130-H64", "bf16-T255-H64"]


@pytest.mark.parametrize("dtype,B,T,NH,Hh,firsts", GENERIC, ids=GENERIC_IDS)
def test_generic_kernels_run_each_document_as_a_sequence_of_its_own(dev, dtype, B, T, NH, Hh, firsts):
    """p = 0: each document's slice of out, lse and dqkv is bit for bit the plain launch on that document alone (lane assignment
    and summation order are relative to the document's first key)"""
    ops = _ops()
    C = NH * Hh
    assert not (dtype == torch.bfloat16 and A.supported(B, T, NH, Hh))
    g = torch.Generator().manual_seed(T * 7 + Hh)
    qkv = torch.randn(B * T, 3 * C, generator=g).to(dtype).to(dev)
    dout = torch.randn(B * T, C, generator=g).to(dtype).to(dev)
    st = D.starts_tensor(B, T, firsts).to(dev)
    _poison(dev, ((B * T, C), dtype), ((B, NH, T), torch.float32))
    out, lse = ops.attn_fwd(qkv, B, T, NH, Hh, Hh ** -0.5, 0.0, None, A.SITE, doc_starts=st)
    _poison(dev, (tuple(qkv.shape), dtype))
    dqkv = ops.attn_bwd(qkv, out, dout, lse, B, T, NH, Hh, Hh ** -0.5, 0.0, None, A.SITE, doc_starts=st)
    for a, b in D.documents(T, firsts):
        L = b - a
        assert not (dtype == torch.bfloat16 and A.supported(B, L, NH, Hh))
        q1 = qkv.view(B, T, 3 * C)[:, a:b].reshape(B * L, 3 * C).contiguous()
        d1 = dout.view(B, T, C)[:, a:b].reshape(B * L, C).contiguous()
        o1, l1 = ops.attn_fwd(q1, B, L, NH, Hh, Hh ** -0.5, 0.0, None, A.SITE)
        g1 = ops.attn_bwd(q1, o1, d1, l1, B, L, NH, Hh, Hh ** -0.5, 0.0, None, A.SITE)
        assert torch.equal(out.view(B, T, C)[:, a:b].reshape(B * L, C), o1), (a, b)
        assert torch.equal(lse[:, :, a:b], l1), (a, b)
        assert torch.equal(dqkv.view(B, T, 3 * C)[:, a:b].reshape(B * L, 3 * C), g1), (a, b)


@pytest.mark.parametrize("dtype,B,T,NH,Hh,firsts", GENERIC, ids=GENERIC_IDS)
def test_generic_kernels_against_the_stitched_reference(dev, dtype, B, T, NH, Hh, firsts):
    """p = 0.1 against the stitched fp64 reference at the tolerances tests/test_gpu_ops.py uses for these kernels: fp32 forward
    2e-5 and backward by the model-"fp32" bound with at_least = 3e-5; bf16 forward 8e-3 inside the envelope and backward by the bf16
    rounding model's bound"""
    ops = _ops()
    p, C = 0.1, NH * Hh
    lowp = dtype == torch.bfloat16
    g = torch.Generator().manual_seed(T * 7 + Hh)
    qkv = torch.randn(B * T, 3 * C, generator=g).to(dtype)
    dout = torch.randn(B * T, C, generator=g).to(dtype)
    keep = torch.from_numpy(rng_ref.keep_mask(A.SEED, A.STEP, A.SITE, p, B * NH * T * T).reshape(B, NH, T, T)).double()
    R = D.stitched(qkv, dout, B, T, NH, Hh, firsts, keep, p)
    M = D.stitched(qkv, dout, B, T, NH, Hh, firsts, keep, p, model=True if lowp else "fp32")
    # (T = 8 in four documents: most groups of dq are exact zeros in fp64 and their median is no scale -- floored as in
    # attention_cases.reference)
    floors = {k: P.structured_floor(R, k, Hh) if R[k].reshape(-1, Hh).norm(dim=1).median().item() == 0 else 0.0 for k in ("dq", "dk", "dv")}
    bounds = D.bwd_bounds_by_offset(R, M, B, T, NH, Hh, firsts, at_least=0.0 if lowp else 3e-5, floors=floors)
    tag = f"docmask generic {'bf16' if lowp else 'fp32'} {(B, T, NH, Hh, p)}"
    st = D.starts_tensor(B, T, firsts).to(dev)
    _poison(dev, ((B * T, C), dtype), ((B, NH, T), torch.float32))
    out, lse = ops.attn_fwd(qkv.to(dev), B, T, NH, Hh, Hh ** -0.5, p, _rng(dev, p), A.SITE, doc_starts=st)
    tol = 8e-3 if lowp else 2e-5
    wf = P.assert_rowwise(out, R["out"], Hh, tol, f"{tag} forward", T)
    if lowp:
        P.assert_within_rounding(out, R["out"], P.attention_fwd_envelope(R), 1, f"{tag} forward")
    el = ((lse.double().cpu() - R["lse"]).abs() / R["lse"].abs().clamp_min(1)).max().item()
    assert el < 1e-5, el
    dead = (keep * D.mask(T, firsts).double()).sum(-1) == 0
    assert int(dead.sum()) > 0                                              # (documents of length 1: dropped with probability p)
    assert torch.all(out.float().cpu().view(B, T, NH, Hh).permute(0, 2, 1, 3)[dead] == 0)
    _poison(dev, (tuple(qkv.shape), dtype))
    dqkv = ops.attn_bwd(qkv.to(dev), out, dout.to(dev), lse, B, T, NH, Hh, Hh ** -0.5, p, _rng(dev, p), A.SITE, doc_starts=st)
    print(f"{tag} forward: worst group {wf:.3e} (bound {tol:g}), lse {el:.2e}")
    for i, n in enumerate(("dq", "dk", "dv")):
        got = dqkv.view(B * T, 3, C)[:, i]
        e = P.rowwise_rel(got, R[n], Hh, floors[n])
        print(f"{tag} {n}: worst group {e.max().item():.3e}, largest error / bound {(e / bounds[n].clamp_min(1e-300)).max().item():.3f}")
        P.assert_rowwise_each(got, R[n], Hh, bounds[n], f"{tag} {n}", T, floor=floors[n])


@pytest.mark.parametrize("name,p", [("doc-pairs", 0.0), ("doc-heavy", 0.2)])
def test_fp8_entry_points(dev, name, p):
    """as test_fp8_entry_points of tests/test_gpu_attention_instances.py, with the document mask: the bf16 outputs are bit for bit
    those with fp8 = NULL, the fp8 bytes are the saturating cast of those values with last step's maximum"""
    ops = _ops()
    c = _case(dev, name)
    B, T, NH = c.B, c.T, c.NH
    qkv, dout = (t.to(dev) for t in A.operands(B, T, NH, c.draw))
    dout = (dout.float() * 0.3).bfloat16()
    st = D.starts_tensor(B, T, c.firsts).to(dev)
    for step in (6, 7, 8):
        state = ops.new_rng_state(A.SEED, dev, step)
        rng = state if p > 0 else None
        o_ref, lse_ref = ops.attn_fwd(qkv, B, T, NH, H, H ** -0.5, p, rng, A.SITE, keep=True, doc_starts=st)
        d_ref = ops.attn_bwd(qkv, o_ref, dout, lse_ref, B, T, NH, H, H ** -0.5, p, rng, A.SITE, doc_starts=st)
        a_o, a_d = o_ref.float().abs().max(), d_ref.float().abs().max()
        seed_o = (a_o * 0.37).reshape(1)
        hist = ops.new_attn_fp8_history(seed_o)
        hist.view(3, 64, 32)[(step + 1) % 3, :, 0] = 123.0                 # must be cleared
        o, lse = ops.attn_fwd(qkv, B, T, NH, H, H ** -0.5, p, rng, A.SITE, keep=True, fp8_out=(hist, state), doc_starts=st)
        q8, sinv = o.dg_fp8
        torch.cuda.synchronize()
        assert torch.equal(o, o_ref) and torch.equal(lse, lse_ref)
        sc = torch.tensor(448.0) / seed_o.cpu()
        want = (o_ref.cpu().float() * sc).clamp(-448, 448).to(E4)
        assert torch.equal(q8.cpu().view(torch.uint8), want.view(torch.uint8))
        assert (q8.cpu().float().abs() == 448).sum() > 0
        assert abs(sinv.item() * sc.item() - 1.0) < 1e-6
        h3 = hist.view(3, 64, 32)[:, :, 0].cpu()
        assert h3[step % 3].max().item() == a_o.item()
        assert (h3[(step + 1) % 3] == 0).all() and (h3[(step + 2) % 3] == seed_o.item()).all()
        seed_d = (a_d * 1.5).reshape(1)
        for only in (False, True):
            hist = ops.new_attn_fp8_history(seed_d)
            hist.view(3, 64, 32)[step % 3] = 0.0                           # (as the previous step leaves it)
            d = ops.attn_bwd(qkv, o, dout, lse, B, T, NH, H, H ** -0.5, p, rng, A.SITE, fp8_out=(hist, state), fp8_out_only=only,
                             doc_starts=st)
            d8, dsinv = d.dg_fp8
            torch.cuda.synchronize()
            if only:
                assert getattr(d, "dg_unwritten", False)
            else:
                assert torch.equal(d, d_ref)
            sc = torch.tensor(57344.0) / seed_d.cpu()
            want = (d_ref.cpu().float() * sc).clamp(-57344, 57344).to(E5)
            assert torch.equal(d8.cpu().view(torch.uint8), want.view(torch.uint8))
            assert abs(dsinv.item() * sc.item() - 1.0) < 1e-6
            h3 = hist.view(3, 64, 32)[:, :, 0].cpu()
            assert h3[step % 3].max().item() == a_d.item() and (h3[(step + 1) % 3] == 0).all()


def _starts_np(ids, sep):
    """numpy restatement of dg_doc_starts: starts[b, t] = 1 + max{ j < t : ids[b, j] == sep }, or 0"""
    B, T = ids.shape
    out = np.zeros((B, T), dtype=np.int32)
    for b in range(B):
        s = 0
        for t in range(T):
            out[b, t] = s
            if ids[b, t] == sep:
                s = t + 1
    return out.reshape(-1)


def test_doc_starts_kernel(dev):
    from drakegpt_amd import _lib
    ops = _ops()
    sep = 5

    def check(ids, what):
        got = ops.doc_starts(ids.to(dev), sep)
        assert got.dtype == torch.int32 and got.shape == (ids.numel(),)
        assert np.array_equal(got.cpu().numpy(), _starts_np(ids.numpy(), sep)), what

    check(torch.tensor([[sep]]), "T = 1, a separator")
    check(torch.tensor([[3]]), "T = 1, none")
    x = torch.full((1, 70), 3, dtype=torch.int64)
    check(x, "no separator")
    y = x.clone(); y[0, 0] = sep; y[0, 69] = sep
    check(y, "separator at 0 and at T - 1")
    z = x.clone(); z[0, 10:14] = sep; z[0, 63:66] = sep
    check(z, "consecutive separators, across a 64-position round")
    g = torch.Generator().manual_seed(0)
    big = torch.randint(0, 40, (2, 1025), generator=g)
    assert int((big == sep).sum()) > 10
    check(big, "T = 1025")
    rows = torch.randint(0, 9, (3, 200), generator=g)
    assert len({tuple(r.tolist()) for r in rows}) == 3
    check(rows, "B = 3 with different rows")
    # ld_ids > T: the first 100 columns of a wider batch
    wide = torch.randint(0, 9, (3, 260), generator=g).to(dev)
    view = wide[:, :100]
    assert view.stride(0) == 260
    got = ops.doc_starts(view, sep)
    assert np.array_equal(got.cpu().numpy(), _starts_np(view.cpu().numpy(), sep))
    # refused arguments: NULL pointers, B or T <= 0, ld_ids < T
    ids = rows.to(dev)
    out = torch.empty(600, dtype=torch.int32, device=dev)
    f = _lib.lib.dg_doc_starts
    assert f(ids.data_ptr(), 200, 3, 200, sep, out.data_ptr(), None) == 0
    assert f(None, 200, 3, 200, sep, out.data_ptr(), None) == -1
    assert f(ids.data_ptr(), 200, 3, 200, sep, None, None) == -1
    assert f(ids.data_ptr(), 200, 0, 200, sep, out.data_ptr(), None) == -1
    assert f(ids.data_ptr(), 200, 3, 0, sep, out.data_ptr(), None) == -1
    assert f(ids.data_ptr(), 199, 3, 200, sep, out.data_ptr(), None) == -1
    torch.cuda.synchronize()
