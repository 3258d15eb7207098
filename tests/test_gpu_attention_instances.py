"""csrc/attention_mfma.hip, every block order, slot rotation and template instance against fp64: the cases of
tests/attention_cases.py (the dispatch read from the library's launch plan; tests/test_attention_cases_host.py holds that plan
to a recording of the dispatch it replaced and shows that the table reaches every (order, reason, rotation) and every (order,
instance) pair).  Each case asserts first, from the plan for the CU count of the device, that it is the case it is named for.

Bounds: the project's own (oracle/parity.py).  Forward: per (row, head) 8e-3, element-wise inside the derived envelope, lse to
1e-5; rows whose kept probabilities were all dropped exactly zero.  Backward, separately for the three forms (tiles from the dQ
pass, scores recomputed, keep bits from the forward): per (row, head) and gradient third inside BWD_MARGIN x the CPU rounding
model's worst group around the same position.  A wrong slot, pair index, class, kmin or tile / keep record index damages
whole (batch, head, block) groups: at least 32 rows x 64 columns of one gradient, each of which has its own bound here.

Which groups a defect would hit (argued from attention_cases.item, not planted on the device):
  * a wrong slot in rotation 1 or 2 ({1,0,2,3}: one nibble of 0x3201; {1,2,3,0}: (wave + 1) & 3): the table is no permutation
    any more, two waves of a workgroup take the same block and another 32-row block of that (batch, head) is never written -- of
    out and lse, of dq, and (the key blocks) of dk and dv.  Only workgroups with blockIdx >= #CUs rotate: the "rotation" case
    has 256 of them in rotation 1 and 130 in rotation 2 (642 in all at 256 CUs), each leaving one block whose groups all carry
    an error of order 1 against bounds of ~1e-2 (the outputs are allocated over NaN: _poison), and the invariance test
    compares a (batch, head) that rotation 2 serves bit for bit with a launch of its own, which runs rotation 0.  (A table
    that is a DIFFERENT permutation changes the balance between the SIMDs and no result: no test can see it, and none needs to.)
  * kmin too large by one in the shared dK/dV pass (a wave left out of the minimum, or the minimum taken over blocks that are
    not this workgroup's): the wave with the lowest key block starts behind its diagonal query tile and never loads its first
    P | dS record -- dk and dv of those 32 keys lose their largest term -- in every workgroup of every case of orders 1 and 2.
    Too small by one only adds an idle iteration where kmin >= 1; at kmin = 0 it reads before the tensors, which no parity
    test promises to notice.
  * a wrong pair index j or class index in orders 1 and 2: a block computed twice and one never, as above; "pairs-small" and
    "heavy-size-4" have wpq = 1, "rotation" and "heavy-size-8" wpq = 2, the two "heavy-length" cases wpq = 4.
  * a wrong tile or keep record index (attn_tile_index, attn_keep_index): the dK/dV pass reads another tile's P | dS, or the dQ
    pass another tile's keep decisions -- the tiles and the keep-bits forms are checked separately from the recompute form,
    which uses neither, and the keep-bits form against the hashed one.

Operands: iid N(0, 1), one draw per case.  With few (batch, head) pairs a bound is the maximum over few draws of the rounding
model; attention_cases.dq_conditioning (read from the reference alone; tests/test_attention_cases_host.py) rejects a draw
in which a near-cancelled group of dq inherits more error from delta's rounding than such a bound allows for, and
attention_cases.DRAW records the one case (1, 482, 3) where the first draw was such.

measured on MI355X (256 CUs), worst (row, head) kernel / CPU rounding model, "use" = largest error / bound over the groups
(elements for the forward envelope), < 1 passes; the three backward forms agree to the digits shown; lse within 2e-7:
  case (B, T, NH, p)                    forward (env. use)  dq                       dk                       dv
  one-tile-2 (1, 2, 1, 0)               1.7e-3 (0.45)    1.7e-3 / 1.7e-3 (0.33)   1.8e-3 / 1.8e-3 (0.33)   1.9e-3 / 1.9e-3 (0.33)
  one-tile-2 (1, 2, 1, 0.2)             2.0e-3 (0.52)    4.7e-3 / 4.7e-3 (0.33)   5.2e-3 / 5.2e-3 (0.33)   1.9e-3 / 1.9e-3 (0.33)
  one-tile-32 (2, 32, 3, 0)             2.9e-3 (0.64)    2.4e-2 / 2.6e-2 (0.30)   5.8e-3 / 5.9e-3 (0.35)   3.7e-3 / 3.7e-3 (0.33)
  one-tile-32 (2, 32, 3, 0.2)           3.2e-3 (0.80)    2.0e-1 / 2.0e-1 (0.33)   1.4e-2 / 1.4e-2 (0.33)   3.5e-3 / 3.5e-3 (0.33)
  plain-ragged (3, 66, 3, 0.2)          3.7e-3 (0.78)    1.6e-1 / 1.6e-1 (0.41)   8.5e-3 / 8.6e-3 (0.42)   3.8e-3 / 3.8e-3 (0.33)
  plain-5-blocks (2, 160, 2, 0)         2.9e-3 (0.74)    1.3e-2 / 1.1e-2 (0.41)   4.6e-3 / 6.2e-3 (0.38)   3.8e-3 / 3.8e-3 (0.33)
  plain-5-blocks (2, 160, 2, 0.2)       3.0e-3 (0.76)    2.1e-1 / 2.1e-1 (0.33)   7.0e-3 / 7.1e-3 (0.37)   3.9e-3 / 3.9e-3 (0.33)
  pairs-small (2, 128, 3, 0)            2.9e-3 (0.59)    1.6e-1 / 8.2e-2 (0.65)   6.1e-3 / 7.2e-3 (0.34)   4.2e-3 / 4.2e-3 (0.33)
  rotation (107, 250, 3, 0.2)           4.1e-3 (0.89)    5.3e-1 / 5.3e-1 (0.37)   1.0e-2 / 1.7e-2 (0.62)   4.5e-3 / 4.5e-3 (0.33)
  heavy-size-4 (37, 126, 23, 0.2)       4.4e-3 (0.91)    4.1e-1 / 4.7e-1 (0.33)   2.2e-2 / 2.3e-2 (0.53)   4.9e-3 / 4.9e-3 (0.33)
  heavy-size-8 (141, 256, 3, 0)         3.8e-3 (0.79)    2.9e-1 / 2.1e-1 (0.59)   9.5e-3 / 1.3e-2 (0.33)   4.8e-3 / 4.8e-3 (0.33)
  heavy-length (1, 512, 3, 0)           3.3e-3 (0.62)    8.3e-3 / 7.2e-3 (0.42)   5.5e-3 / 6.5e-3 (0.39)   4.0e-3 / 4.0e-3 (0.33)
  heavy-length (1, 512, 3, 0.2)         3.3e-3 (0.57)    5.1e-1 / 5.1e-1 (0.36)   6.2e-3 / 5.3e-3 (0.39)   4.1e-3 / 4.1e-3 (0.33)
  heavy-length-ragged (1, 482, 3, 0)    3.1e-3 (0.59)    2.9e-2 / 2.9e-2 (0.41)   4.6e-3 / 7.8e-3 (0.36)   4.2e-3 / 4.2e-3 (0.33)
  heavy-length-ragged (1, 482, 3, 0.2)  3.2e-3 (0.61)    2.1e-1 / 2.1e-1 (0.60)   4.2e-3 / 4.2e-3 (0.38)   4.4e-3 / 4.4e-3 (0.33)
(dq's worst groups are the first query rows, as in tests/test_gpu_ops.py; dv equals the rounding model's to the last digit.)
The first draw of (1, 482, 3) at p = 0: dq of head 2, query row 1 at 6.2e-2 against a bound of 4.9e-2 and the model's 1.1e-2, in
all three forms; every other group of that run inside its bound."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_cases as A  # noqa: E402
from oracle import parity as P  # noqa: E402

pytestmark = pytest.mark.gpu

H = A.HD
E4, E5 = torch.float8_e4m3fn, torch.float8_e5m2


def _ops():
    from drakegpt_amd import ops
    return ops


def _report(msg):
    if os.environ.get("DG_TEST_REPORT"):
        print("[parity] " + msg, flush=True)


def _case(dev, name):
    """the case for this device's CU count, after checking that it is what its name says"""
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    c = A.case(name, ncu)
    assert A.supported(c.B, c.T, c.NH) and _ops().attn_fp8_out_supported(c.B, c.T, c.NH, H, torch.bfloat16)        # the MFMA family runs
    assert A.order(c.B, c.T, c.NH, ncu) == (c.order, c.reason), (c, ncu)
    assert A.rotations(c.B, c.T, c.NH, ncu) == c.rotations, (c, ncu)
    assert A.plan(A.call(0, c.B, c.T, c.NH, ncu=0)).rot_div == ncu           # the library plans for this device
    return c


def _rng(dev, p, step=A.STEP):
    return _ops().new_rng_state(A.SEED, dev, step) if p > 0 else None


def _poison(dev, *shapes):
    """the entry points allocate their outputs with torch.empty, and the caching allocator tends to hand back the block a tensor
    of the same size has just left -- after an earlier test of the same case, one full of correct values.  NaN-filled tensors of
    the outputs' sizes, released just before the launch, take that place (best effort: the allocator promises nothing), so that
    a block no wave writes is seen as NaN, not as the last launch's result."""
    for shape, dtype in shapes:
        torch.full(shape, float("nan"), dtype=dtype, device=dev)
    torch.cuda.synchronize()


def _same_up_to_contraction(a, b):
    """the criterion of the keep-bits form against the hashed form (tests/test_gpu_ops.py): a wrong decision or a wrong tile moves
    an element by many bf16 ulps, two builds of the same fp32 expression by one at most"""
    a, b = a.float(), b.float()
    assert bool(((a - b).abs() <= 2.0 ** -6 * torch.maximum(a.abs(), b.abs()) + 1e-6 * b.abs().max()).all())
    r = ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()
    assert r < 2e-4, r


def _forward(dev, c, p, R):
    ops = _ops()
    B, T, NH = c.B, c.T, c.NH
    tag = f"attention instances {c.name} {(B, T, NH, H, p)}"
    qkv = R["qkv"].to(dev)
    _poison(dev, ((B * T, NH * H), torch.bfloat16), ((B, NH, T), torch.float32))
    out, lse = ops.attn_fwd(qkv, B, T, NH, H, H ** -0.5, p, _rng(dev, p), A.SITE)
    assert getattr(out, "dg_keep", None) is None
    wf = P.assert_rowwise(out, R["out"], H, 8e-3, f"{tag} forward", T)
    uf = P.assert_within_rounding(out, R["out"], R["env"], 1, f"{tag} forward")
    el = ((lse.double().cpu() - R["lse"]).abs() / R["lse"].abs().clamp_min(1)).max().item()
    assert el < 1e-5, el
    if p > 0:
        dead = R["dead"]
        assert int(dead.sum()) > 0 or B * NH <= 3                      # (P(row 0 dropped) = p per head)
        assert torch.all(out.float().cpu().view(B, T, NH, H).permute(0, 2, 1, 3)[dead] == 0)
        # the instance that also leaves the keep decisions: the same output bit for bit (lse: an ulp between the two builds)
        out_k, lse_k = ops.attn_fwd(qkv, B, T, NH, H, H ** -0.5, p, _rng(dev, p), A.SITE, keep=True)
        assert out_k.dg_keep.numel() == B * NH * (A.blocks(T) * (A.blocks(T) + 1) // 2) * 128
        assert torch.equal(out_k, out)
        assert ((lse_k.double().cpu() - R["lse"]).abs() / R["lse"].abs().clamp_min(1)).max().item() < 1e-5
        assert ((lse_k.double() - lse.double()).norm() / lse.double().norm()).item() < 1e-6
    _report(f"{tag} forward: worst group {wf:.2e}, envelope use {uf:.2f}, lse {el:.1e}")


def _backward_of(dev, c, p, R, form):
    """(dqkv of the form, out it was computed from)"""
    ops = _ops()
    B, T, NH = c.B, c.T, c.NH
    qkv, dout = R["qkv"].to(dev), R["dout"].to(dev)
    out, lse = ops.attn_fwd(qkv, B, T, NH, H, H ** -0.5, p, _rng(dev, p), A.SITE, keep=form == "keep_bits")
    bits = getattr(out, "dg_keep", None)
    assert (bits is not None) == (form == "keep_bits" and p > 0)
    _poison(dev, (tuple(qkv.shape), torch.bfloat16))
    return ops.attn_bwd(qkv, out, dout, lse, B, T, NH, H, H ** -0.5, p, _rng(dev, p), A.SITE, keep_bits=bits, tile_scratch=form != "recompute")


def _backward(dev, c, p, R, form):
    B, T, NH = c.B, c.T, c.NH
    C = NH * H
    tag = f"attention instances {c.name} {(B, T, NH, H, p)} backward ({form})"
    dqkv = _backward_of(dev, c, p, R, form)
    ref = torch.stack([R["dq"], R["dk"], R["dv"]], 1).reshape(B * T, 3 * C)
    assert P.rel(dqkv, ref) < 2e-2, P.rel(dqkv, ref)                # the whole-tensor tolerance of tests/test_gpu_ops.py
    for i, n in enumerate(("dq", "dk", "dv")):
        got = dqkv.view(B * T, 3, C)[:, i]
        use = P.assert_rowwise_each(got, R[n], H, R["bounds"][n], f"{tag} {n}", T, floor=R["floors"][n])
        _report(f"{tag} {n}: worst group {P.rowwise_rel(got, R[n], H, R['floors'][n]).max().item():.2e}, model's worst {R['model_worst'][n]:.2e}, "
                f"largest error / bound {use:.2f}")


def _keep_bits_against_hashed(dev, c, p, R):
    _same_up_to_contraction(_backward_of(dev, c, p, R, "keep_bits"), _backward_of(dev, c, p, R, "tiles"))


CHECKS = [(name, p, what) for name, p in A.CASE_P for what in ("forward",) + A.FORMS + (("keep_bits_against_hashed",) if p > 0 else ())]


@pytest.mark.parametrize("name,p,what", CHECKS, ids=[f"{n}-p{p:g}-{w}" for n, p, w in CHECKS])
def test_case(dev, name, p, what):
    """one parametrisation per (case, p, check), case-major: the checks of a case share its CPU reference"""
    c = _case(dev, name)
    assert p in c.ps
    R = A.reference(c.B, c.T, c.NH, p, c.draw)
    if what == "forward":
        _forward(dev, c, p, R)
    elif what == "keep_bits_against_hashed":
        _keep_bits_against_hashed(dev, c, p, R)
    else:
        _backward(dev, c, p, R, what)


FP8_CASES = [(n, p) for n, p in A.CASE_P if A.case(n, 256).fp8]


@pytest.mark.parametrize("name,p", FP8_CASES, ids=[f"{n}-p{p:g}" for n, p in FP8_CASES])
def test_fp8_entry_points(dev, name, p):
    """as test_attention_kernels_leave_fp8_copies (tests/test_gpu_fp8.py): the bf16 outputs of the fp8 entry points are those of
    the plain ones bit for bit, the fp8 bytes are the saturating cast of those values with last step's maximum, with and
    without the bf16 dqkv (fp8_out_only)"""
    ops = _ops()
    c = _case(dev, name)
    B, T, NH = c.B, c.T, c.NH
    assert A.runs(p, True)[3:] == [("keep_bits" if p > 0 else "tiles", "both"), ("keep_bits" if p > 0 else "tiles", "only8")]
    qkv, dout = (t.to(dev) for t in A.operands(B, T, NH, c.draw))
    dout = (dout.float() * 0.3).bfloat16()
    for step in (6, 7, 8):
        state = ops.new_rng_state(A.SEED, dev, step)
        rng = state if p > 0 else None
        o_ref, lse_ref = ops.attn_fwd(qkv, B, T, NH, H, H ** -0.5, p, rng, A.SITE, keep=True)
        d_ref = ops.attn_bwd(qkv, o_ref, dout, lse_ref, B, T, NH, H, H ** -0.5, p, rng, A.SITE)
        a_o, a_d = o_ref.float().abs().max(), d_ref.float().abs().max()
        seed_o = (a_o * 0.37).reshape(1)
        hist = ops.new_attn_fp8_history(seed_o)
        hist.view(3, 64, 32)[(step + 1) % 3, :, 0] = 123.0                 # must be cleared
        o, lse = ops.attn_fwd(qkv, B, T, NH, H, H ** -0.5, p, rng, A.SITE, keep=True, fp8_out=(hist, state))
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
            d = ops.attn_bwd(qkv, o, dout, lse, B, T, NH, H, H ** -0.5, p, rng, A.SITE, fp8_out=(hist, state), fp8_out_only=only)
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


@pytest.mark.parametrize("name", ["rotation", "heavy-size-4", "heavy-size-8"])
def test_a_head_does_not_depend_on_the_launch_around_it(dev, name):
    """The kernels treat (batch, head) pairs independently.  Without dropout, the lowest, a middle and the highest (batch, head)
    of the large launch, each run alone as a (1, T, 1) launch (order 1, rotation 0, one or two workgroups): out and lse bit for
    bit -- both launches run attn_fwd_mfma_kernel<false,false,false>, every wave keeps its own K / V images and no arithmetic
    depends on the block order --, dqkv up to the contraction of the per-wave and the shared dQ builds."""
    ops = _ops()
    c = _case(dev, name)
    B, T, NH = c.B, c.T, c.NH
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    assert A.order(1, T, 1, ncu) == (1, None) and A.rotations(1, T, 1, ncu) == {0}
    qkv, dout = (t.to(dev) for t in A.operands(B, T, NH, c.draw))
    _poison(dev, ((B * T, NH * H), torch.bfloat16), ((B, NH, T), torch.float32))
    out, lse = ops.attn_fwd(qkv, B, T, NH, H, H ** -0.5, 0.0, None, A.SITE)
    _poison(dev, (tuple(qkv.shape), torch.bfloat16))
    dqkv = ops.attn_bwd(qkv, out, dout, lse, B, T, NH, H, H ** -0.5, 0.0, None, A.SITE)
    for bh in (0, (B * NH) // 2, B * NH - 1):
        b, h = divmod(bh, NH)
        q1, d1 = A.slab(qkv, B, T, NH, b, h, 3), A.slab(dout, B, T, NH, b, h, 1)
        o1, l1 = ops.attn_fwd(q1, 1, T, 1, H, H ** -0.5, 0.0, None, A.SITE)
        g1 = ops.attn_bwd(q1, o1, d1, l1, 1, T, 1, H, H ** -0.5, 0.0, None, A.SITE)
        assert torch.equal(o1, A.slab(out, B, T, NH, b, h, 1)), (name, bh)
        assert torch.equal(l1.view(T), lse[b, h]), (name, bh)
        _same_up_to_contraction(A.slab(dqkv, B, T, NH, b, h, 3), g1)
