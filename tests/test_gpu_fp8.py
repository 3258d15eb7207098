"""fp8 path (precision = "fp8", BASELINE.json configs[4]): operand preparation and the block-scaled MFMA GEMM against fp64
math on the DEQUANTISED operands.  The reference has no reduced precision (every nn.Linear of src/model_component.py:320-325,
392-393,404,454 is fp32), so the kernel-level oracle is: exact arithmetic on the very fp8 values the kernel multiplies."""
import pytest
import torch

pytestmark = pytest.mark.gpu

E4, E5 = torch.float8_e4m3fn, torch.float8_e5m2
FMAX = {E4: 448.0, E5: 57344.0}


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


@pytest.mark.parametrize("fmt", [E4, E5])
@pytest.mark.parametrize("src", [torch.bfloat16, torch.float32])
def test_fp8_quantize_matches_ocp_rounding(dev, fmt, src):
    """q = fp8(x * FMAX / amax): the bytes equal torch's OCP conversion (round to nearest even, e4m3fn / e5m2 -- gfx950's
    encodings, not MI300's fnuz) of the same scaled values, the dequantisation factor is amax / FMAX, amax lands on +-FMAX."""
    from drakegpt_amd import ops
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(1000, 264, generator=g) * torch.logspace(-3, 1, 264)).to(src)
    x[17, 5] = -37.5                                          # the amax element
    q, sinv = ops.fp8_quantize(x.to(dev), fmt)
    torch.cuda.synchronize()
    amax = x.float().abs().max()
    assert amax.item() == 37.5
    scale = torch.tensor(FMAX[fmt], dtype=torch.float32) / amax
    want = (x.float() * scale).clamp(-FMAX[fmt], FMAX[fmt]).to(fmt)
    assert q.dtype == fmt and q.shape == x.shape
    assert torch.equal(q.cpu().view(torch.uint8), want.view(torch.uint8))
    assert abs(sinv.item() - (1.0 / scale).item()) <= 1e-7 * sinv.item()
    assert q.cpu().float()[17, 5].item() == -FMAX[fmt]
    # all zeros: scale 1, zeros out
    z, zs = ops.fp8_quantize(torch.zeros(64, 128, dtype=src, device=dev), fmt)
    assert zs.item() == 1.0 and torch.all(z.view(torch.uint8) == 0)


def test_fp8_quantize_segments(dev):
    """one launch pair over a flat buffer with a segment table (the weight matrices of a step): per-segment amax and scale"""
    from drakegpt_amd import ops
    g = torch.Generator().manual_seed(5)
    sizes = [384 * 384, 64, 1152 * 384, 80 * 384, 8]
    gaps = [0, 64, 0, 128, 0]
    flat, table, pos = [], [], 0
    for n, gap, amp in zip(sizes, gaps, [0.02, 3.0, 0.5, 1e-4, 100.0]):
        flat.append(torch.randn(n, generator=g) * amp)
        table.append([pos, n])
        pos += n
        if gap:
            flat.append(torch.full((gap,), 1e6))             # padding between segments must not leak into any amax
            pos += gap
    x = torch.cat(flat).bfloat16()
    seg = torch.tensor(table, dtype=torch.int64)
    q, sinv = ops.fp8_quantize(x.to(dev), E4, seg=seg.to(dev), n_seg=len(sizes))
    torch.cuda.synchronize()
    for i, (first, n) in enumerate(table):
        xs = x[first:first + n].float()
        scale = torch.tensor(448.0) / xs.abs().max()
        want = (xs * scale).clamp(-448, 448).to(E4)
        assert torch.equal(q[first:first + n].cpu().view(torch.uint8), want.view(torch.uint8)), i
        assert abs(sinv[i].item() * scale.item() - 1.0) < 1e-6, i


def _rand_fp8(shape, fmt, g, amp):
    return (torch.randn(*shape, generator=g) * amp).clamp(-FMAX[fmt], FMAX[fmt]).to(fmt)


@pytest.mark.parametrize("a_fmt", [E4, E5])
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M,N,K", [(128, 128, 256), (256, 384, 256), (1000, 1152, 384), (2048, 1024, 4096), (300, 200, 1024), (16384, 192, 256)])
def test_gemm_nt_fp8_plain(dev, a_fmt, out_dtype, M, N, K):
    """C = sa * sb * A B^T with e4m3 / e5m2 A and e4m3 B against fp64 on the same fp8 values -- 128 x 128 and 128 x 192 tiles,
    ragged M and N, K = 2 .. 32 steps of 128.  Measured 1.1e-5 (e5m2) / 1.4e-5 (e4m3) relative, the same at every K: the
    128-term dot product inside v_mfma_f32_16x16x128_f8f6f4 is summed with a narrower adder tree than fp32 (a property of the
    instruction; the bf16 MFMA gives 2e-7 here) -- three orders of magnitude below the fp8 quantisation error of the operands."""
    from drakegpt_amd import ops
    g = torch.Generator().manual_seed(M + N + K)
    A = _rand_fp8((M, K), a_fmt, g, 2.0 if a_fmt == E4 else 30.0)
    B = _rand_fp8((N, K), E4, g, 1.5)
    sa, sb = torch.tensor([0.0371]), torch.tensor([1.7e-3])
    ref = (A.double() @ B.double().T) * (sa.double() * sb.double())
    out = ops.gemm_nt(A.to(dev), B.to(dev), out_dtype, scale_a=sa.to(dev), scale_b=sb.to(dev))
    torch.cuda.synchronize()
    assert out.dtype == out_dtype
    assert rel(out, ref) < (4e-5 if out_dtype == torch.float32 else 3e-3), rel(out, ref)
    if out_dtype == torch.bfloat16:
        # every element: one bf16 rounding of fp64 on the dequantised operands plus the accumulation envelope (oracle/parity.py)
        from oracle import parity as P
        P.assert_within_rounding(out, ref, P.gemm_envelope(A, B, K, scale=(sa.double() * sb.double()).item()), 1, "fp8 gemm, bf16 out")


def test_gemm_nt_fp8_asymmetric_identity(dev):
    """A = I (exact in e4m3) against an asymmetric B: catches a transposed C/D map or a k permutation that differs between the
    two operands of v_mfma_f32_16x16x128_f8f6f4"""
    from drakegpt_amd import ops
    K = 256
    A = torch.eye(K).to(E4)
    vals = torch.tensor([0.5, 1.0, 1.5, 2.0, 3.0, -0.75, -4.0, 6.0])
    B = vals[(torch.arange(96 * K) * 7 % 8)].reshape(96, K) * (1 + (torch.arange(96)[:, None] % 3))
    Bq = B.to(E4)
    assert torch.equal(Bq.float(), B)                          # exactly representable
    one = torch.ones(1, device=dev)
    out = ops.gemm_nt(A.to(dev), Bq.to(dev), torch.float32, scale_a=one, scale_b=one)
    assert torch.equal(out.cpu(), B.T.contiguous())


@pytest.mark.parametrize("M,N,K", [(512, 384, 256), (1100, 1024, 512), (256, 1536, 384)])
def test_gemm_nt_fp8_epilogues(dev, M, N, K):
    """the epilogue forms the fp8 step uses: bias + ReLU + sign-bit emission (FeedForward's first Linear), the sign-bit-masked
    dX with column sums (its backward, e5m2 gradients), bias + dropout + residual and bias + residual (proj / second Linear)"""
    from oracle import parity as P
    from oracle import rng_ref
    from drakegpt_amd import ops
    g = torch.Generator().manual_seed(K)
    A = _rand_fp8((M, K), E4, g, 2.0)
    B = _rand_fp8((N, K), E4, g, 1.0)
    G = _rand_fp8((M, N), E5, g, 20.0)                        # a gradient of the [M, N] output
    Bt = _rand_fp8((K, N), E4, g, 1.0)                        # "W^T" for the dX direction: [K out, N contraction]
    bias = torch.randn(N, generator=g)
    resid = torch.randn(M, N, generator=g)
    sa, sb = torch.tensor([0.01]), torch.tensor([0.02])
    d = lambda t: t.to(dev)
    ss = (sa.double() * sb.double()).item()                  # the fp32 scales as the kernel reads them
    acc = (A.double() @ B.double().T) * (0.01 * 0.02)
    # bias + ReLU + sign bits, then consume the bits in the dX form
    sup = ops.gemm_nt_sign_bits_supported(torch.bfloat16, N, K, in_dtype=E4) and ops.gemm_nt_sign_bits_supported(torch.bfloat16, N, K, in_dtype=E5)
    assert sup and not ops.gemm_nt_sign_bits_supported(torch.bfloat16, N, 192, in_dtype=E4)       # K % 128 == 0, K >= 256
    if sup:
        bits = ops.new_sign_bits(M, N, dev)
        f = ops.gemm_nt(d(A), d(B), torch.bfloat16, bias=d(bias), relu=True, sign_bits_out=bits, scale_a=d(sa), scale_b=d(sb))
        ref_f = torch.relu(acc + bias.double())
        assert rel(f, ref_f) < 3e-3
        env = P.gemm_envelope(A, B, K, bias, scale=ss)
        decided = P.mask_margin(acc + bias.double(), env)
        P.assert_within_rounding(f, ref_f, env, 1, "fp8 bias + relu + sign bits out", where=decided)
        # dX of the Linear that consumed f ... here just the masking semantics: out[m, n] = (G2 B2^T)[m, n] where f[m, n] > 0
        G2 = _rand_fp8((M, K), E5, g, 10.0)
        B2 = _rand_fp8((N, K), E4, g, 1.0)
        rows = ops.gemm_nt_colsum_rows(torch.bfloat16, M, N, K, in_dtype=E5)
        cs = torch.full((max(rows, 1), N), float("nan"), device=dev)
        out = ops.gemm_nt(d(G2), d(B2), torch.bfloat16, sign_bits=bits, scale_a=d(sa), scale_b=d(sb), colsum_part=cs if rows else None)
        ref = (G2.double() @ B2.double().T) * (0.01 * 0.02) * (f.double().cpu() > 0)
        assert rel(out, ref) < 3e-3
        P.assert_within_rounding(out, ref, P.gemm_envelope(G2, B2, K, scale=ss) * (f.double().cpu() > 0), 1, "fp8 sign bits in")
        if rows:
            assert rel(cs.sum(0), ref.sum(0)) < 1e-4
    # bias + dropout + residual (fp32 out) with the shared keep-mask, and bias + residual
    rng = ops.new_rng_state(99, dev, 4)
    keep = torch.from_numpy(rng_ref.keep_mask(99, 4, 7, 0.2, M * N).reshape(M, N)).double()
    y = ops.gemm_nt(d(A), d(B), torch.float32, bias=d(bias), dropout_p=0.2, rng_state=rng, site=7, residual=d(resid), scale_a=d(sa), scale_b=d(sb))
    assert rel(y, (acc + bias.double()) * keep / 0.8 + resid.double()) < 4e-5
    y0 = ops.gemm_nt(d(A), d(B), torch.float32, bias=d(bias), residual=d(resid), scale_a=d(sa), scale_b=d(sb))
    assert rel(y0, acc + bias.double() + resid.double()) < 4e-5
    # e5m2 gradient x e4m3 W^T, plain bf16 out (dX of proj / QKV / first FFN Linear)
    dx = ops.gemm_nt(d(G), d(Bt), torch.bfloat16, scale_a=d(sa), scale_b=d(sb))
    assert rel(dx, (G.double() @ Bt.double().T) * (0.01 * 0.02)) < 3e-3
    P.assert_within_rounding(dx, (G.double() @ Bt.double().T) * ss, P.gemm_envelope(G, Bt, N, scale=ss), 1, "fp8 dX, bf16 out")


@pytest.mark.parametrize("M,N,K", [(4096, 1536, 256), (8192, 1024, 384)])
def test_gemm_nt_fp8_out_from_the_epilogue(dev, M, N, K):
    """fp8_out: the bias + ReLU + sign-bit GEMM also leaves its output as e4m3 with delayed scaling (what a dg_fp8_quantize_delayed
    launch on the output would produce, minus the launch and its re-read).  Against exact arithmetic: q8 = e4m3(out * 448 / amax_prev)
    of the fp32 output; the slot of this step receives max(out); scale_inv = amax_prev / 448; the bf16 output and the sign bits
    are those of the call without fp8_out, bit for bit; the next step (parity flipped) scales by the maximum just recorded."""
    from drakegpt_amd import ops
    g = torch.Generator().manual_seed(N + K)
    A = _rand_fp8((M, K), E4, g, 2.0)
    B = _rand_fp8((N, K), E4, g, 1.0)
    bias = torch.randn(N, generator=g)
    sa, sb = torch.tensor([0.013]), torch.tensor([0.021])
    d = lambda t: t.to(dev)
    assert ops.gemm_nt_fp8_out_supported(M, N, K) and not ops.gemm_nt_fp8_out_supported(M - 128, 128, K)
    ref = torch.relu((A.double() @ B.double().T) * (0.013 * 0.021) + bias.double())
    bits0 = ops.new_sign_bits(M, N, dev)
    f0 = ops.gemm_nt(d(A), d(B), torch.bfloat16, bias=d(bias), relu=True, sign_bits_out=bits0, scale_a=d(sa), scale_b=d(sb))
    P = ops.FP8_AMAX_PARTS
    parts2 = torch.zeros(2 * P, device=dev)
    amax_prev = 0.8 * ref.max().item()                        # last step's range was smaller: the top of this one clips
    parts2[P:] = torch.rand(P, generator=g).to(dev) * 0.1
    parts2[P + 17] = amax_prev                                # step 4 is even: slot 1 is read, slot 0 written
    parts2[:P] = 123.0                                        # stale values in the slot to be written
    st = ops.new_rng_state(1, dev, 4)
    q8 = torch.zeros((M, N), dtype=E4, device=dev)
    sinv = torch.zeros(1, device=dev)
    bits = ops.new_sign_bits(M, N, dev)
    f = ops.gemm_nt(d(A), d(B), torch.bfloat16, bias=d(bias), relu=True, sign_bits_out=bits, scale_a=d(sa), scale_b=d(sb),
                    fp8_out=(q8, parts2, st, sinv))
    torch.cuda.synchronize()
    assert torch.equal(f, f0) and torch.equal(bits, bits0)
    assert abs(sinv.item() - amax_prev / 448.0) < 1e-6 * amax_prev
    got = q8.float().double().cpu() * sinv.item()
    want = ref.clamp(max=amax_prev)
    # e4m3: 3 mantissa bits -> half an ulp is 2^-4 relative; subnormals below 2^-6 of the scaled range are absolute
    err = (got - want).abs()
    tol = want.abs() * (2.0 ** -4 + 1e-5) + amax_prev / 448.0 * 2.0 ** -10 + 4e-5 * ref.abs().max().item()
    assert (err <= tol).all(), (err - tol).max()
    assert rel(got, want) < 0.04
    rec = parts2[:P]
    assert abs(rec.max().item() - ref.max().item()) < 1e-5 * ref.max().item() and rec.min().item() >= 0.0
    assert torch.equal(parts2[P:].cpu()[17:18], torch.tensor([amax_prev], dtype=torch.float32))       # the read slot is untouched
    # the cast launch on the bf16 output agrees up to the bf16 rounding of its input
    q_ref, s_ref = ops.fp8_quantize_delayed(f0, E4, torch.cat([torch.zeros(P, device=dev), parts2[P:]]), st)
    assert abs(s_ref.item() - sinv.item()) < 1e-7 and (q_ref.view(torch.uint8) != q8.view(torch.uint8)).float().mean().item() < 0.02
    # next step: parity flips, the maximum recorded above is the scale
    ops.state_advance(st)
    ops.gemm_nt(d(A), d(B), torch.bfloat16, bias=d(bias), relu=True, sign_bits_out=bits, scale_a=d(sa), scale_b=d(sb), fp8_out=(q8, parts2, st, sinv))
    assert abs(sinv.item() - ref.max().item() / 448.0) < 1e-5 * ref.max().item()
    assert rel(q8.float().double().cpu() * sinv.item(), ref) < 0.04
    with pytest.raises(RuntimeError):                        # not offered without the sign bits / for ragged shapes
        ops.gemm_nt(d(A), d(B), torch.bfloat16, bias=d(bias), relu=True, scale_a=d(sa), scale_b=d(sb), fp8_out=(q8, parts2, st, sinv))


@pytest.mark.parametrize("M,N,K", [(4096, 1536, 384), (8192, 1024, 256)])
def test_gemm_nt_fp8_out_dx_form(dev, M, N, K):
    """fp8_out in the dX direction: the sign-bit-masked GEMM with column sums (e5m2 gradient x e4m3 W^T) also leaves its output
    as e5m2 with delayed scaling -- signed values, |.| for the maximum, both clamps; bf16 output and column sums unchanged"""
    from drakegpt_amd import ops
    g = torch.Generator().manual_seed(M + K)
    d = lambda t: t.to(dev)
    A0 = _rand_fp8((M, K), E4, g, 2.0)
    B0 = _rand_fp8((N, K), E4, g, 1.0)
    one = torch.ones(1)
    bits = ops.new_sign_bits(M, N, dev)
    f = ops.gemm_nt(d(A0), d(B0), torch.bfloat16, bias=d(torch.zeros(N)), relu=True, sign_bits_out=bits, scale_a=d(one * 0.01), scale_b=d(one * 0.02))
    G2 = _rand_fp8((M, K), E5, g, 10.0)
    B2 = _rand_fp8((N, K), E4, g, 1.0)
    sa, sb = d(one * 0.01), d(one * 0.02)
    rows = ops.gemm_nt_colsum_rows(torch.bfloat16, M, N, K, in_dtype=E5)
    assert rows and ops.gemm_nt_fp8_out_supported(M, N, K, grad=True)
    cs0 = torch.zeros((rows, N), device=dev)
    out0 = ops.gemm_nt(d(G2), d(B2), torch.bfloat16, sign_bits=bits, scale_a=sa, scale_b=sb, colsum_part=cs0)
    ref = (G2.double() @ B2.double().T) * (0.01 * 0.02) * (f.double().cpu() > 0)
    P = ops.FP8_AMAX_PARTS
    parts2 = torch.zeros(2 * P, device=dev)
    amax_prev = 0.7 * ref.abs().max().item()
    parts2[:P] = amax_prev * torch.rand(P, generator=g).to(dev)
    parts2[3] = amax_prev                                      # step 5 is odd: slot 0 is read, slot 1 written
    parts2[P:] = 55.0
    st = ops.new_rng_state(1, dev, 5)
    q8 = torch.zeros((M, N), dtype=E5, device=dev)
    sinv = torch.zeros(1, device=dev)
    cs = torch.zeros((rows, N), device=dev)
    out = ops.gemm_nt(d(G2), d(B2), torch.bfloat16, sign_bits=bits, scale_a=sa, scale_b=sb, colsum_part=cs, fp8_out=(q8, parts2, st, sinv))
    torch.cuda.synchronize()
    assert torch.equal(out, out0) and torch.equal(cs, cs0)
    assert abs(sinv.item() - amax_prev / 57344.0) < 1e-6 * amax_prev
    got = q8.float().double().cpu() * sinv.item()
    want = ref.clamp(min=-amax_prev, max=amax_prev)
    err = (got - want).abs()
    # e5m2: 2 mantissa bits, subnormal step 2^-16; + the GEMM's own accumulation error (4e-5 of the operand scale, see
    # test_gemm_nt_fp8_plain), which is all there is to an output that nearly cancels
    tol = want.abs() * (2.0 ** -3 + 1e-5) + amax_prev / 57344.0 * 2.0 ** -16 + 4e-5 * ref.abs().max().item()
    bad = (err > tol).nonzero()
    assert bad.numel() == 0, (bad[:3], [(got[i, j].item(), want[i, j].item(), out0[i, j].item()) for i, j in bad[:3].tolist()])
    assert rel(got, want) < 0.08
    assert abs(parts2[P:].max().item() - ref.abs().max().item()) < 1e-5 * ref.abs().max().item() and parts2[P:].min().item() >= 0.0
    assert parts2[3].item() == pytest.approx(amax_prev)


@pytest.mark.parametrize("M,C", [(8192, 1024), (16384, 384), (3000, 768)])
def test_layernorm_bwd_fused_fp8_emits_the_next_gradient_operand(dev, M, C):
    """the fused LayerNorm backward of the bf16 gradient stream also leaves g = dropout_bwd(dx) as e5m2 with delayed scaling
    (the operand of the fp8 dX GEMM that runs next): dx, g and every partial row bit-identical to the call without fp8_out;
    g8 = e5m2(g * 57344 / amax_prev) of the returned bf16 g (bit for bit in tests/test_gpu_layernorm.py); one partial maximum per workgroup (exactly 256 of them)"""
    from oracle import rng_ref
    from drakegpt_amd import ops
    G, site, seed, step, p = ops.FP8_AMAX_PARTS, 5, 11, 8, 0.2
    gen = torch.Generator().manual_seed(M + C)
    x = torch.randn(M, C, generator=gen)
    w, b = torch.randn(C, generator=gen), torch.randn(C, generator=gen)
    dy = torch.randn(M, C, generator=gen).bfloat16()
    dres = torch.randn(M, C, generator=gen).bfloat16()
    d = lambda t: t.to(dev)
    _, mean, rstd = ops.layernorm_fwd(d(x), d(w), d(b), torch.float32)
    rng = ops.new_rng_state(seed, dev, step)
    P0 = [torch.full((G, C), float("nan"), device=dev) for _ in range(3)]
    dx0, g0 = ops.layernorm_bwd_fused(d(dy), d(x), d(w), mean, rstd, d(dres), P0[0], P0[1], C, G, torch.bfloat16, p, rng, site, P0[2], stream_dtype=torch.bfloat16)
    xd = x.double().requires_grad_(True)
    torch.nn.functional.layer_norm(xd, (C,), w.double(), b.double(), 1e-5).backward(dy.double())
    keep = torch.from_numpy(rng_ref.keep_mask(seed, step, site, p, M * C).reshape(M, C)).double()
    g_ref = (xd.grad + dres.double()) * keep / (1.0 - p)
    gmax = g_ref.abs().max().item()
    P = ops.FP8_AMAX_PARTS
    parts2 = torch.zeros(2 * P, device=dev)
    amax_prev = 0.8 * gmax
    parts2[P:] = amax_prev * torch.rand(P, generator=gen).to(dev)            # step 8 is even: slot 1 read, slot 0 written
    parts2[P + 9] = amax_prev
    parts2[:P] = 321.0
    P1 = [torch.full((G, C), float("nan"), device=dev) for _ in range(3)]
    dx, g, g8, sinv = ops.layernorm_bwd_fused(d(dy), d(x), d(w), mean, rstd, d(dres), P1[0], P1[1], C, G, torch.bfloat16, p, rng, site, P1[2],
                                               stream_dtype=torch.bfloat16, fp8_out=(parts2, rng))
    torch.cuda.synchronize()
    assert torch.equal(dx, dx0) and torch.equal(g, g0) and all(torch.equal(a, b_) for a, b_ in zip(P0, P1))
    assert g8.dtype == E5 and abs(sinv.item() - amax_prev / 57344.0) < 1e-6 * amax_prev
    got = g8.float().double().cpu() * sinv.item()
    want = g_ref.clamp(min=-amax_prev, max=amax_prev)
    tol = want.abs() * (2.0 ** -3 + 1e-4) + amax_prev / 57344.0 * 2.0 ** -16 + 2e-6 * gmax
    assert ((got - want).abs() <= tol).all()
    assert torch.all(got[keep == 0] == 0)
    assert abs(parts2[:P].max().item() - gmax) < 1e-5 * gmax and parts2[:P].min().item() >= 0 and parts2[P + 9].item() == pytest.approx(amax_prev)
    with pytest.raises(RuntimeError):                                        # one partial maximum per workgroup: exactly 256
        ops.layernorm_bwd_fused(d(dy), d(x), d(w), mean, rstd, d(dres), P1[0][:24], P1[1][:24], C, 24, torch.bfloat16, p, rng, site, P1[2][:24],
                                stream_dtype=torch.bfloat16, fp8_out=(parts2, rng))


def test_gemm_nt_fp8_argument_validation(dev):
    from drakegpt_amd import ops
    A = torch.zeros(128, 256, dtype=E4, device=dev)
    one = torch.ones(1, device=dev)
    with pytest.raises(TypeError):
        ops.gemm_nt(A, A, torch.float32)                                        # no scales
    with pytest.raises(TypeError):
        ops.gemm_nt(A, A.to(E5), torch.float32, scale_a=one, scale_b=one)       # B must be e4m3
    with pytest.raises(RuntimeError):
        ops.gemm_nt(A[:, :192].contiguous(), A[:, :192].contiguous(), torch.float32, scale_a=one, scale_b=one)   # K % 128
    with pytest.raises(RuntimeError):
        ops.fp8_quantize(torch.zeros(100, 3, dtype=torch.bfloat16, device=dev), E4)                              # numel % 8


# ------------------------------------------------------------------------------------------------ model level
def _scaled(dev, precision, seed=42, p=None, L=None):
    import drakegpt_amd as D
    from oracle import drake_ref as R
    cfg = R.SCALED
    torch.manual_seed(seed)
    return D.TransformerLM(80, cfg["embedding_dim"], cfg["context_length"], cfg["num_heads"], L or cfg["num_layers"],
                           cfg["dropout"] if p is None else p, precision=precision).to(dev).train(), cfg


def test_fp8_engine_step_against_bf16_engine_and_oracle(dev):
    """TransformerLM_scaled, B = 8, dropout 0.2, one captured engine step in precision "fp8" (QKV / proj / FFN Linears forward on
    e4m3 x e4m3, their dX on e5m2 x e4m3, since round 3 their dW on the same e5m2 / e4m3 copies; attention, lm_head, LayerNorm
    as in "bf16") against (a) the same step in "bf16"
    and (b) the reference arithmetic with the same keep-masks.  fp8 operands carry 2^-4 (e4m3) / 2^-3 (e5m2) relative
    rounding per element, so the bounds are those of the number format (measured values in the assertions' comments), not
    of a kernel defect: the kernels themselves are held to 4e-5 against exact arithmetic on the fp8 values above."""
    import os
    from drakegpt_amd.engine import TrainEngine
    from oracle import drake_ref as R
    from oracle import rng_ref
    B, T, seed = 8, 256, 777
    g = torch.Generator().manual_seed(1)
    x = torch.randint(0, 80, (B, T), generator=g)
    y = torch.randint(0, 80, (B, T), generator=g)
    out = {}
    for prec in ("bf16", "fp8"):
        m, cfg = _scaled(dev, prec)
        sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
        eng = TrainEngine(m, B, T, lr=cfg["base_lr"], betas=cfg["betas"], seed=seed, use_graph=True)
        assert eng.fp8 == (prec == "fp8")
        eng.keep_logits = True
        eng.set_batch(x.to(dev), y.to(dev))
        loss = eng.step().item()
        torch.cuda.synchronize()
        out[prec] = (loss, eng.last_logits.float().cpu(), torch.cat([v.reshape(-1).double().cpu() for v in eng.named_grads().values()]),
                     {k: v.detach().clone().cpu() for k, v in eng.named_grads().items()})
        keys = list(eng.named_grads().keys())
    C, NH, L, p = cfg["embedding_dim"], cfg["num_heads"], cfg["num_layers"], cfg["dropout"]
    masks = rng_ref.transformer_masks(seed, 0, p, B, T, C, NH, L)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    lo, ls, gr = R.loss_and_grads("TransformerLM", sd, x, y, p=p, training=True, masks=masks)
    ref_flat = torch.cat([gr[k].reshape(-1).double() for k in keys])
    e = {}
    for prec in ("bf16", "fp8"):
        loss, logits, flat, _ = out[prec]
        e[prec] = (abs(loss - ls.item()) / ls.item(), rel(logits, lo), rel(flat, ref_flat))
    e["fp8_vs_bf16"] = (abs(out["fp8"][0] - out["bf16"][0]) / out["bf16"][0], rel(out["fp8"][1], out["bf16"][1]), rel(out["fp8"][2], out["bf16"][2]))
    if os.environ.get("DG_TEST_REPORT"):
        print("[parity] fp8 engine (loss, logits, flat gradient): " + ", ".join(f"{k}: {v[0]:.2e} {v[1]:.2e} {v[2]:.2e}" for k, v in e.items()), flush=True)
        per = {k: rel(out["fp8"][3][k], gr[k]) for k in keys}
        print("[parity] fp8 worst tensors vs reference: " + str(sorted(per.items(), key=lambda kv: -kv[1])[:4]), flush=True)
    assert e["bf16"][1] < 6e-3 and e["bf16"][2] < 2e-2
    # measured (round 3, fp8 dW): fp8 vs the reference arithmetic: loss 9.2e-5, logits 2.3e-2, flat gradient 7.0e-2 (6.1e-2 with
    # bf16 dW in round 2; worst tensors, the LayerNorm-2 gains and W1: 0.18); bf16 on the same step: 1.3e-5, 2.8e-3, 1.3e-2
    assert e["fp8"][0] < 1e-3 and e["fp8"][1] < 5e-2 and e["fp8"][2] < 0.12, e
    assert e["fp8_vs_bf16"][1] < 5e-2 and e["fp8_vs_bf16"][2] < 0.12, e


def test_fp8_module_path_equals_engine(dev):
    """precision "fp8" behind the nn.Module surface (autograd path, weights quantised per call) == the engine (persistent fp8
    shadows refreshed by the optimizer step): same kernels on the same fp8 values"""
    from drakegpt_amd.engine import TrainEngine
    B, T = 4, 256
    m, cfg = _scaled(dev, "fp8", p=0.0, L=2)
    g = torch.Generator().manual_seed(2)
    x = torch.randint(0, 80, (B, T), generator=g).to(dev)
    y = torch.randint(0, 80, (B, T), generator=g).to(dev)
    logits, loss = m(x, y)
    loss.backward()
    ref = {k: q.grad.detach().clone() for k, q in m.named_parameters() if q.grad is not None}
    m.zero_grad(set_to_none=True)
    # as the module path keeps it: fp32 gradient stream, weight gradients on the bf16 operands (the engine's default since round 3
    # is the grouped dW GEMM on the fp8 copies -- fp8_dw -- which the autograd path's per-matrix split-K GEMMs do not have)
    eng = TrainEngine(m, B, T, lr=0.0, weight_decay=0.0, use_graph=False, grad_stream="fp32", fp8_dw=False)
    eng.keep_logits = True
    eng.set_batch(x, y)
    l2 = eng.step().item()
    assert abs(l2 - loss.item()) < 1e-5 * abs(l2) and rel(eng.last_logits, logits) < 1e-6
    got = eng.named_grads()
    worst = max(((k, rel(got[k], ref[k])) for k in ref), key=lambda kv: kv[1])
    assert worst[1] < 4e-3, worst


def test_fp8_training_tracks_bf16(dev):
    """40 optimizer steps on a learnable synthetic stream (a noisy periodic sequence): the fp8 run's loss falls like the bf16
    run's -- the property that matters for a training precision (final losses within 3 %, both well below the initial loss)"""
    from drakegpt_amd.engine import TrainEngine
    B, T = 16, 256
    g = torch.Generator().manual_seed(0)
    base = torch.arange(300_000) * 7 % 23
    noise = torch.randint(0, 80, (300_000,), generator=g)
    corpus = torch.where(torch.rand(300_000, generator=g) < 0.1, noise, base)
    offs = torch.randint(300_000 - T - 1, (40, B), generator=g).to(dev)
    final = {}
    for prec in ("bf16", "fp8"):
        m, cfg = _scaled(dev, prec, L=2)
        eng = TrainEngine(m, B, T, lr=1e-3, betas=cfg["betas"], seed=5)
        eng.set_corpus(corpus)
        ls = []
        for i in range(40):
            eng.set_offsets(offs[i])
            ls.append(eng.step().item())
        eng.check_status()
        final[prec] = (ls[0], sum(ls[-5:]) / 5)
    assert final["bf16"][1] < 0.6 * final["bf16"][0] and final["fp8"][1] < 0.6 * final["fp8"][0], final
    assert abs(final["fp8"][1] - final["bf16"][1]) < 0.03 * final["bf16"][1], final


def test_fp8_quantize_delayed_uses_last_steps_amax(dev):
    """one-pass delayed scaling: the scale comes from the slot the previous step wrote (step parity from the device-side step
    word), this tensor's amax goes to the other slot; values beyond last step's range saturate instead of overflowing"""
    from drakegpt_amd import ops
    P = ops.FP8_AMAX_PARTS
    g = torch.Generator().manual_seed(9)
    x1 = (torch.randn(512, 1024, generator=g) * 0.7).bfloat16()
    x2 = (torch.randn(512, 1024, generator=g) * 1.9).bfloat16()
    state = ops.new_rng_state(1, dev, 6)                           # step 6: writes slot 0, reads slot 1
    parts2 = torch.zeros(2 * P, device=dev)
    _, _ = ops.fp8_quantize(x1.to(dev), E4, amax=parts2[P:])       # seed slot 1 with amax(x1), as the engine's warm-up does
    q, sinv = ops.fp8_quantize_delayed(x2.to(dev), E4, parts2, state)
    torch.cuda.synchronize()
    a1, a2 = x1.float().abs().max(), x2.float().abs().max()
    scale = torch.tensor(448.0) / a1
    want = (x2.float() * scale).clamp(-448, 448).to(E4)
    assert torch.equal(q.cpu().view(torch.uint8), want.view(torch.uint8))
    assert (q.cpu().float().abs() == 448).sum() > 0                # x2 outgrew x1's range: clipped, finite
    assert abs(sinv.item() * scale.item() - 1.0) < 1e-6
    assert parts2[:P].max().item() == a2.item() and parts2[P:].max().item() == a1.item()
    ops.state_advance(state)                                       # step 7: reads slot 0 (amax of x2), writes slot 1
    q3, s3 = ops.fp8_quantize_delayed(x1.to(dev), E5, parts2, state)
    want3 = (x1.float() * (torch.tensor(57344.0) / a2)).clamp(-57344, 57344).to(E5)
    assert torch.equal(q3.cpu().view(torch.uint8), want3.view(torch.uint8))
    assert parts2[P:].max().item() == a1.item() and abs(s3.item() * (57344.0 / a2.item()) - 1.0) < 1e-6


@pytest.mark.parametrize("B,T,NH,p", [(2, 256, 4, 0.1), (1, 1024, 2, 0.1), (3, 128, 2, 0.0)])
def test_attention_kernels_leave_fp8_copies(dev, B, T, NH, p):
    """dg_attn_fwd_fp8 / dg_attn_bwd_fp8: the bf16 outputs are those of the plain entry points bit for bit; the fp8 copies are the
    saturating cast of those bf16 values with LAST step's maximum (history slot (step + 2) % 3); this step's maximum lands in slot
    step % 3, slot (step + 1) % 3 is cleared; only8 leaves the same bytes and no bf16 dqkv.  ref: Head2.forward
    src/model_component.py:392-405 (o feeds MultiHeadAttention3.proj, :454; dqkv feeds autograd of the packed QKV Linears)."""
    from drakegpt_amd import ops
    H = 64
    assert ops.attn_fp8_out_supported(B, T, NH, H, torch.bfloat16)
    g = torch.Generator().manual_seed(B * 1000 + T)
    qkv = torch.randn(B * T, 3 * NH * H, generator=g).bfloat16().to(dev)
    dout = (torch.randn(B * T, NH * H, generator=g) * 0.3).bfloat16().to(dev)
    for step in (6, 7, 8):
        state = ops.new_rng_state(77, dev, step)
        rng = state if p > 0 else None
        o_ref, lse_ref = ops.attn_fwd(qkv, B, T, NH, H, H ** -0.5, p, rng, 5, keep=True)
        d_ref = ops.attn_bwd(qkv, o_ref, dout, lse_ref, B, T, NH, H, H ** -0.5, p, rng, 5)
        a_o, a_d = o_ref.float().abs().max(), d_ref.float().abs().max()
        # forward: last step's maximum smaller than this tensor's -> some elements saturate
        seed_o = (a_o * 0.37).reshape(1)
        hist = ops.new_attn_fp8_history(seed_o)
        hist.view(3, 64, 32)[(step + 1) % 3, :, 0] = 123.0                 # must be cleared
        o, lse = ops.attn_fwd(qkv, B, T, NH, H, H ** -0.5, p, rng, 5, keep=True, fp8_out=(hist, state))
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
        # backward, with and without the bf16 form
        seed_d = (a_d * 1.5).reshape(1)
        for only in (False, True):
            hist = ops.new_attn_fp8_history(seed_d)
            hist.view(3, 64, 32)[step % 3] = 0.0                           # (as the previous step leaves it)
            d = ops.attn_bwd(qkv, o, dout, lse, B, T, NH, H, H ** -0.5, p, rng, 5, fp8_out=(hist, state), fp8_out_only=only)
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


def test_gpt2_medium_shape_fp8_engine_steps(dev):
    """BASELINE.json configs[4]: GPT-2-medium shape (V 50257, C 1024, T 1024, 16 heads, 24 layers), precision "fp8", B = 1.
    Two captured engine steps: loss finite and near ln V at init, falling after one AdamW step on the same batch; against the
    SAME step in "bf16" (same weights, batch and dropout masks) the loss and the flat gradient stay inside the fp8 number
    format's bounds; size-independent properties of the gradient.  (The oracle cannot run this shape in test time; the fp8
    engine is tied to the oracle at the scaled configuration above.)  ref: src/model.py:558-609, src/model_component.py:320-325."""
    import math
    import os
    import drakegpt_amd as D
    from drakegpt_amd.config import GPT2_MEDIUM as cfg
    from drakegpt_amd.engine import TrainEngine
    V, C, T, NH, L, p, B = cfg["vocab_size"], cfg["embedding_dim"], cfg["context_length"], cfg["num_heads"], cfg["num_layers"], cfg["dropout"], 1
    g = torch.Generator().manual_seed(13)
    x = torch.randint(0, V, (B, T), generator=g).to(dev)
    y = torch.randint(0, V, (B, T), generator=g).to(dev)
    res = {}
    for prec in ("bf16", "fp8"):
        torch.manual_seed(42)
        m = D.TransformerLM(V, C, T, NH, L, p, precision=prec).to(dev).train()
        assert sum(q.numel() for q in m.parameters()) == 2 * V * C + V + T * C + L * (12 * C * C + 10 * C) + 2 * C == 406262865
        eng = TrainEngine(m, B, T, lr=cfg["base_lr"], betas=cfg["betas"], seed=2024, use_graph=True)
        assert eng.fp8 == (prec == "fp8") and eng.grouped_dw and eng.bf16_logits
        if prec == "fp8":
            assert len(eng.fp8_sites) == 0                     # seeded by the first execution
        eng.set_batch(x, y)
        l0 = eng.step().item()
        torch.cuda.synchronize()
        eng.check_status()
        if prec == "fp8":
            # every Linear of every block, forward and dX operands (+ the input of the fp8 lm_head); round 3: + the two LayerNorm
            # launches per block that emit their output as e4m3 themselves (their own history format: one partial per workgroup)
            # and the two attention call sites per block whose fp8 copies leave the attention kernels (three-slot history)
            assert sum(1 for k in eng.fp8_sites if "#" not in k) == 8 * L + int(eng.fp8_head)
            assert sum(1 for k in eng.fp8_sites if k.endswith("#attn")) == 2 * L
            assert sum(1 for k in eng.fp8_sites if k.endswith("#ln")) == 2 * L
        grads = {k: v.detach().clone() for k, v in eng.named_grads().items()}
        l1 = eng.step().item()                                 # same batch again, after one AdamW step: a graph replay
        assert math.isfinite(l0) and math.log(V) - 0.5 < l0 < math.log(V) + 3.0, l0
        assert math.isfinite(l1) and l1 < l0, (l0, l1)
        assert eng.step_count() == 2
        res[prec] = (l0, grads)
        del eng, m
        torch.cuda.empty_cache()
    (lb, gb), (l8, g8) = res["bf16"], res["fp8"]
    keys = list(gb)
    flat_b = torch.cat([gb[k].reshape(-1).double() for k in keys])
    flat_8 = torch.cat([g8[k].reshape(-1).double() for k in keys])
    e_flat = ((flat_8 - flat_b).norm() / flat_b.norm()).item()
    worst = max(((k, rel(g8[k], gb[k])) for k in keys), key=lambda kv: kv[1])
    if os.environ.get("DG_TEST_REPORT"):
        print(f"[parity] gpt2-medium fp8 vs bf16 engine: loss {abs(l8 - lb) / lb:.2e}, flat gradient {e_flat:.3e}, worst tensor {worst}", flush=True)
    # measured (round 2): loss 7.3e-6, flat gradient 0.111, worst tensor 0.23 (a LayerNorm-2 gain, as at the scaled configuration)
    assert abs(l8 - lb) < 1e-3 * lb and e_flat < 0.2 and worst[1] < 0.4, (l8, lb, e_flat, worst)
    bias = g8["lm_head.bias"].double()
    assert abs(bias.sum().item()) < 1e-3 * bias.abs().sum().item()            # softmax-minus-one-hot rows sum to zero
    gt = g8["token_embedding_table.weight"]
    unseen = torch.ones(V, dtype=torch.bool, device=dev)
    unseen[x.reshape(-1)] = False
    assert torch.all(gt[unseen] == 0) and torch.all(gt[~unseen].abs().sum(1) > 0)
    assert torch.all(g8["position_embedding_table.weight"].abs().sum(1) > 0)


@pytest.mark.parametrize("fmt", [torch.float8_e4m3fn, torch.float8_e5m2])
def test_fp8_casts_propagate_non_finite_values(dev, fmt):
    """fmaxf drops a NaN from the recorded amax and the min / max clamp turns a NaN element into -FMAX, so a diverging
    fp8 run trained on saturated values.  Now a NaN / Inf element poisons the recorded maximum (integer max on |x| bit patterns),
    a poisoned maximum makes the scale NaN, and a NaN element stays NaN through the cast."""
    from drakegpt_amd import ops
    g = torch.Generator().manual_seed(9)
    x = torch.randn(64, 256, generator=g).bfloat16().to(dev)
    # just-in-time scaling: the NaN reaches amax, scale_inv and therefore every element
    xn = x.clone()
    xn[3, 17] = float("nan")
    q, sinv = ops.fp8_quantize(xn, fmt)
    assert torch.isnan(sinv).all() and torch.isnan(q.float()).all()
    xi = x.clone()
    xi[5, 1] = float("inf")
    q, sinv = ops.fp8_quantize(xi, fmt)
    assert torch.isnan(sinv).all()
    # delayed scaling: step k casts with step k-1's (finite) maximum -- the NaN element itself stays NaN, the others are cast
    # normally -- and records a NaN maximum; step k+1 then has a NaN scale
    parts2 = torch.zeros(2 * ops.FP8_AMAX_PARTS, device=dev)
    state = ops.new_rng_state(1, dev, 0)
    ops.fp8_quantize(x, fmt, amax=parts2[:ops.FP8_AMAX_PARTS])
    parts2[ops.FP8_AMAX_PARTS:].copy_(parts2[:ops.FP8_AMAX_PARTS])
    q0, s0 = ops.fp8_quantize_delayed(x, fmt, parts2, state)
    assert torch.isfinite(s0).all() and torch.isfinite(q0.float()).all()
    ops.state_advance(state)
    q1, s1 = ops.fp8_quantize_delayed(xn, fmt, parts2, state)
    f1 = q1.float()
    assert torch.isfinite(s1).all() and torch.isnan(f1[3, 17]) and int(torch.isnan(f1).sum()) == 1
    ops.state_advance(state)
    q2, s2 = ops.fp8_quantize_delayed(x, fmt, parts2, state)
    assert torch.isnan(s2).all() and torch.isnan(q2.float()).all()
    # ... and the GEMM carries it into its output (what turns the loss NaN)
    w = torch.randn(128, 256, generator=g).bfloat16().to(dev)
    wq, ws = ops.fp8_quantize(w, torch.float8_e4m3fn)
    out = ops.gemm_nt(q1, wq, torch.bfloat16, scale_a=s1, scale_b=ws)
    assert torch.isnan(out[3].float()).all() and torch.isfinite(out[4].float()).all()


@pytest.mark.parametrize("with_short", [True, False])
def test_gemm_tn_grouped_fp8(dev, with_short):
    """round 3: the grouped dW GEMM on OCP fp8 operands (A = dY e5m2, B = X e4m3, ds_read_b64_tr_b8 + v_mfma_f32_16x16x128_f8f6f4)
    against EXACT arithmetic on the same fp8 values times the two dequantisation factors (ref: autograd's dW = dY^T X of every
    nn.Linear, src/model_component.py:321-323,392-393,454): many problems of different shapes and contraction lengths in one
    launch, ragged P / Q, padded leading dimensions, more tiles than CUs; whole tiles, then K halves chained through the
    workspace twice (the flags reset themselves, results run-to-run identical)."""
    from drakegpt_amd import ops
    g = torch.Generator().manual_seed(12)
    shapes = [(1024, 384, 384), (1024, 1152, 384), (1024, 384, 1536), (1024, 1536, 384), (128 if with_short else 384, 200, 72),
              (2048, 1024, 1024), (512, 128, 128), (256, 264, 520), (8192, 1024, 256)] * 2
    shapes += [(256, 2048, 2048)]
    probs, refs, outs = [], [], []
    for i, (R, P, Q) in enumerate(shapes):
        lda = (P + 15) // 16 * 16 + (16 if i % 3 == 0 else 0)
        ldb = (Q + 15) // 16 * 16
        A = torch.zeros(R, lda)
        A[:, :P] = torch.randn(R, P, generator=g) * 3.0
        B = torch.zeros(R, ldb)
        B[:, :Q] = torch.randn(R, Q, generator=g)
        Aq, Bq = A.to(torch.float8_e5m2), B.to(torch.float8_e4m3fn)
        sa, sb = torch.tensor([0.37 + 0.01 * i]), torch.tensor([1.9 - 0.02 * i])
        refs.append((Aq[:, :P].double().T @ Bq[:, :Q].double()) * (sa.double() * sb.double()))
        out = torch.full((P * Q,), float("nan"), device=dev)
        outs.append(out)
        Ad, Bd = Aq.to(dev), Bq.to(dev)
        probs.append((Ad[:, :P] if lda != P else Ad, Bd[:, :Q] if ldb != Q else Bd, out, P, Q, sa.to(dev), sb.to(dev)))
    assert sum(((P + 255) // 256) * ((Q + 127) // 128) for _, P, Q in shapes) > 256
    ws = ops.gemm_tn_grouped_workspace(probs, dev)
    first = None
    for workspace in (None, ws, ws):
        for out in outs:
            out.fill_(float("nan"))
        ops.gemm_tn_grouped(probs, workspace)
        torch.cuda.synchronize()
        for out, ref, (R, P, Q) in zip(outs, refs, shapes):
            # the 128-term dot product inside the instruction is summed with a narrower adder tree than fp32 (1.1-1.4e-5 measured
            # for the NT form): 4e-5 as there
            assert rel(out.view(P, Q), ref) < 4e-5, (workspace is not None, R, P, Q, rel(out.view(P, Q), ref))
        if workspace is not None:
            if first is None:
                first = [o.clone() for o in outs]
            else:
                assert all(torch.equal(a, b) for a, b in zip(first, outs))
    assert int(ws[-16:].view(torch.int32)[0].item()) == 0
    z8a = torch.zeros(192, 64, dtype=torch.float8_e5m2, device=dev)
    z8b = torch.zeros(192, 64, dtype=torch.float8_e4m3fn, device=dev)
    one = torch.ones(1, device=dev)
    with pytest.raises(RuntimeError):                   # contraction length must be a multiple of 128
        ops.gemm_tn_grouped([(z8a, z8b, torch.zeros(64 * 64, device=dev), 64, 64, one, one)])
    with pytest.raises(RuntimeError):                   # the two operand kinds do not mix in one launch
        ops.gemm_tn_grouped([(z8a[:128], z8b[:128], torch.zeros(64 * 64, device=dev), 64, 64, one, one),
                             (z8a[:128].bfloat16(), z8b[:128].bfloat16(), torch.zeros(64 * 64, device=dev), 64, 64)])


def test_cross_entropy_fp8_gradient_copy(dev):
    """round 3 (fp8 lm_head): the loss kernel on bf16 logits writes its gradient in place (bf16) AND as e5m2 with the a-priori scale
    57344 / grad_scale -- |softmax - onehot| <= 1 bounds |dlogits| by grad_scale (ref: F.cross_entropy, src/model.py:604-607).  The
    e5m2 copy times grad_scale / 57344 is the fp64 gradient to e5m2 rounding (2^-3 relative per element, far less in norm), equals the
    OCP rounding of the very value the bf16 path rounds, pad columns are zero, losses and the bf16 gradient are those of
    dg_cross_entropy."""
    from drakegpt_amd import ops
    M, V, ld = 64, 50257, 50304
    g = torch.Generator().manual_seed(3)
    buf = torch.zeros(M, ld, dtype=torch.bfloat16)
    buf[:, :V] = (torch.randn(M, V, generator=g) * 3).bfloat16()
    tgt = torch.randint(0, V, (M,), generator=g)
    x = buf[:, :V].double()
    ref = (torch.softmax(x, 1) - torch.nn.functional.one_hot(tgt, V)) / M
    ref_rows = torch.logsumexp(x, 1) - x[torch.arange(M), tgt]
    a, b = buf.to(dev), buf.to(dev)
    rows0 = ops.cross_entropy(a[:, :V], tgt.to(dev), V, dlogits=a, grad_scale=1.0 / M)
    q8 = torch.full((M, ld), 7.0, device=dev).to(torch.float8_e5m2)
    rows1 = ops.cross_entropy_fp8(b[:, :V], tgt.to(dev), V, b, 1.0 / M, q8)
    torch.cuda.synchronize()
    assert torch.equal(rows0, rows1) and torch.equal(a, b) and rel(rows1, ref_rows) < 1e-6
    deq = q8.float().cpu().double() * (1.0 / M / 57344.0)
    assert torch.all(deq[:, V:] == 0)
    assert rel(deq[:, :V], ref) < 4e-2, rel(deq[:, :V], ref)
    el = ((deq[:, :V] - ref).abs() / ref.abs().clamp_min(1e-30))
    big = ref.abs() > 1e-4 / M                     # above e5m2's subnormal range at this scale
    assert el[big].max().item() <= 2 ** -3 * 1.02, el[big].max().item()
    with pytest.raises(RuntimeError):              # ld8 must be a multiple of 16 and within the gradient's leading dimension
        ops.cross_entropy_fp8(b[:, :V], tgt.to(dev), V, b, 1.0 / M, torch.zeros((M, 50264), device=dev).to(torch.float8_e5m2))


def test_fp8_head_engine_step(dev):
    """the fp8 lm_head inside the engine (V 50257, T 1024, C 1024, L 1, B 1): forward on e4m3 x e4m3, dX on the loss kernel's e5m2
    gradient x the e4m3 W^T shadow (K = 50304), dW in the fp8 grouped launch -- against the same engine with the bf16 head
    (DG_FP8_HEAD=0): loss, the head's gradients and the gradient that enters the blocks."""
    import os
    import drakegpt_amd as D
    from drakegpt_amd.engine import TrainEngine
    V, C, T, NH, L, B = 50257, 1024, 1024, 16, 1, 1
    g = torch.Generator().manual_seed(8)
    x = torch.randint(0, V, (B, T), generator=g).to(dev)
    y = torch.randint(0, V, (B, T), generator=g).to(dev)
    out = {}
    for mode in ("1", "0"):
        os.environ["DG_FP8_HEAD"] = mode
        try:
            torch.manual_seed(42)
            m = D.TransformerLM(V, C, T, NH, L, 0.0, precision="fp8").to(dev).train()
            eng = TrainEngine(m, B, T, lr=1e-4, seed=3, use_graph=True)
        finally:
            os.environ.pop("DG_FP8_HEAD", None)
        assert eng.fp8_head == (mode == "1") and eng.bf16_logits
        eng.set_batch(x, y)
        loss = eng.step().item()
        torch.cuda.synchronize()
        eng.check_status()
        out[mode] = (loss, {k: v.detach().float().clone() for k, v in eng.named_grads().items()})
    (l1, g1), (l0, g0) = out["1"], out["0"]
    e = {k: rel(g1[k], g0[k]) for k in ("lm_head.weight", "lm_head.bias", "blocks.0.ffwd.net.2.weight", "blocks.0.sa_head.proj.weight")}
    if os.environ.get("DG_TEST_REPORT"):
        print(f"[parity] fp8 head vs bf16 head: loss {abs(l1 - l0) / l0:.2e}, " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()), flush=True)
    # measured (round 3): loss 1.5e-5, lm_head.weight 2.7e-2, lm_head.bias 3.5e-4, block gradients 6.1e-2 / 6.7e-2 (e5m2 dlogits: 2 mantissa bits)
    assert abs(l1 - l0) < 2e-3 * l0 and e["lm_head.weight"] < 0.1 and e["lm_head.bias"] < 2e-2
    assert e["blocks.0.ffwd.net.2.weight"] < 0.15 and e["blocks.0.sa_head.proj.weight"] < 0.15, e


def test_fp8_only_outputs_equal_the_written_ones(dev):
    """round 3: in precision fp8 with the fp8 dW launch the FFN hidden layer, its gradient and the LayerNorm backward's gradient operand
    are read as fp8 ONLY (by the next GEMM and by the grouped dW launch), so their bf16 form is not written any more (dg_gemm_nt
    fp8_out_only, dg_layernorm_bwd_fused_fp8 g8_only).  Same fp8 values either way: three captured steps with and without the stores
    (DG_FP8_ONLY=0) give the same loss and the same gradient bit for bit; an unwritten tensor refuses a bf16 consumer."""
    import os
    import drakegpt_amd as D
    from drakegpt_amd import sublayers as S
    from drakegpt_amd.engine import TrainEngine
    V, C, T, NH, L, B = 80, 384, 256, 6, 2, 8
    g = torch.Generator().manual_seed(21)
    xs = [torch.randint(0, V, (B, T), generator=g).to(dev) for _ in range(3)]
    ys = [torch.randint(0, V, (B, T), generator=g).to(dev) for _ in range(3)]
    out = {}
    for mode in ("1", "0"):
        os.environ["DG_FP8_ONLY"] = mode
        try:
            torch.manual_seed(42)
            m = D.TransformerLM(V, C, T, NH, L, 0.1, precision="fp8").to(dev).train()
            eng = TrainEngine(m, B, T, lr=1e-3, seed=5, use_graph=True)
            res = []
            for x, y in zip(xs, ys):
                eng.set_batch(x, y)
                loss = eng.step().item()
                res.append((loss, torch.cat([v.reshape(-1).float() for v in eng.named_grads().values()]).clone()))
            eng.check_status()
        finally:
            os.environ.pop("DG_FP8_ONLY", None)
        out[mode] = res
    for (l1, g1), (l0, g0) in zip(out["1"], out["0"]):
        assert l1 == l0 and torch.equal(g1, g0)
    t = torch.zeros(4, 4, device=dev, dtype=torch.bfloat16)
    t.dg_unwritten = True
    with pytest.raises(RuntimeError):
        S._refuse_unwritten(t)


@pytest.mark.parametrize("M,C", [(8192, 1024), (1000, 384), (64, 768)])
def test_layernorm_fwd_fp8_equals_layernorm_plus_delayed_cast(dev, M, C):
    """dg_layernorm_fwd_fp8 (round 3; ref: nn.LayerNorm at src/model_component.py:488-489, :505-506): the LayerNorm output as e4m3 with
    delayed scaling from the LayerNorm launch itself, one partial maximum per workgroup -- against dg_layernorm_fwd followed by a cast
    with the same scale (the previous slot's maximum): identical bytes, statistics and bf16 output, the recorded maximum = the
    output's, the other slot untouched; with want_bf16=False the bf16 form is left alone and the tensor is marked."""
    from drakegpt_amd import ops
    g = torch.Generator().manual_seed(M + C)
    x = (torch.randn(M, C, generator=g) * 1.7 + 0.3).to(dev)
    gam, bet = (1 + 0.1 * torch.randn(C, generator=g)).to(dev), (0.1 * torch.randn(C, generator=g)).to(dev)
    n = ops.layernorm_fwd_fp8_parts(M)
    state = ops.new_rng_state(5, dev, 6)                      # step word 6: slot 0 is written, slot 1 read
    y0, mean0, rstd0 = ops.layernorm_fwd(x, gam, bet, torch.bfloat16)
    prev_amax = 3.0
    parts2 = torch.zeros(2 * n, device=dev)
    parts2[n:] = torch.rand(n, generator=g).to(dev) * prev_amax
    parts2[n + 7 % n] = prev_amax
    before = parts2.clone()
    y, mean, rstd, q8, sinv = ops.layernorm_fwd_fp8(x, gam, bet, parts2, state)
    torch.cuda.synchronize()
    assert torch.equal(y, y0) and torch.equal(mean, mean0) and torch.equal(rstd, rstd0)
    sc = 448.0 / prev_amax
    assert abs(sinv.item() - 1.0 / sc) < 1e-7
    ref = (y0.float() * torch.tensor(sc, device=dev)).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    assert torch.equal(q8.view(torch.uint8), ref.view(torch.uint8))
    assert torch.equal(parts2[n:], before[n:])                                # the slot that was read
    assert parts2[:n].max().item() == y0.float().abs().max().item()
    y2, _, _, q8b, _ = ops.layernorm_fwd_fp8(x, gam, bet, before.clone(), state, want_bf16=False)
    assert getattr(y2, "dg_unwritten", False) and torch.equal(q8b.view(torch.uint8), q8.view(torch.uint8))
    with pytest.raises(RuntimeError):
        ops.layernorm_fwd_fp8(x, gam, bet, parts2[:-1], state)


@pytest.mark.parametrize("R,Cc,ldo", [(1024, 4096, 1024), (384, 1152, 384), (80, 384, 128), (50257, 64, 50304), (130, 200, 144)])
def test_transpose_u8_batched(dev, R, Cc, ldo):
    """dg_transpose_u8_batched (round 3): the e4m3 W^T shadows as byte transpositions of the e4m3 W shadows -- exact, for whole and
    ragged 128 x 128 tiles, a padded leading dimension (rows of the output beyond R written as zeros), several matrices per launch."""
    from drakegpt_amd import ops
    g = torch.Generator().manual_seed(R + Cc)
    a = torch.randint(0, 256, (R, Cc), generator=g, dtype=torch.uint8).to(dev)
    b = torch.randint(0, 256, (R // 2 + 1, 48), generator=g, dtype=torch.uint8).to(dev)
    at = torch.full((Cc, ldo), 7, dtype=torch.uint8, device=dev)
    bt = torch.full((48, R // 2 + 1), 7, dtype=torch.uint8, device=dev)
    table = ops.make_transpose_u8_table([(a, at), (b, bt)], dev)
    ops.transpose_u8_batched(*table)
    torch.cuda.synchronize()
    assert torch.equal(at[:, :R], a.t()) and torch.all(at[:, R:] == 0)
    assert torch.equal(bt, b.t())
