// Split-bf16 instantiations of the wave-specialised persistent NT GEMM (gemm_nt_ws.h, F8 = 3): fp32 operands in memory, split
// in registers after the LDS read into hi = bf16(x) and lo = bf16(x - hi), contracted as lo.hi + hi.lo + hi.hi on
// v_mfma_f32_16x16x32_bf16 with fp32 accumulation -- precision "bf16x3" (fp32-grade logits at bf16 matrix-core rates).
// fp32 output only, and only the epilogues the fp32 engine program asks for: plain, bias, bias + residual, bias + dropout +
// residual, and everything else (ReLU, fp32 relu_mask, residual without bias) through the generic form.
// A translation unit of its own so that its kernel variants compile beside gemm.hip's.
#include "gemm_nt_ws.h"

// Returns 0 when a variant was launched.
int dg_gemm_nt_x3_launch(const NtParams& p, bool wide, int epi, dim3 pgrid, hipStream_t s) {
    const dim3 wsb(512 + 64 * WS_NLOAD);
#define L(NJ_, EPI_) hipLaunchKernelGGL((gemm_nt_ws_kernel<float, false, NJ_, EPI_, 3>), pgrid, wsb, 0, s, p)
#define X3(NJ_) do { \
        if (epi == 1) L(NJ_, 1); \
        else if (epi == 3) L(NJ_, 3); \
        else if (epi == 5) L(NJ_, 5); \
        else if (epi == 7) L(NJ_, 7); \
        else if (epi == 0) L(NJ_, 0); \
        else return DG_ERR_ARG; } while (0)
    if (wide) X3(6); else X3(4);
#undef L
#undef X3
    return DG_OK;
}
