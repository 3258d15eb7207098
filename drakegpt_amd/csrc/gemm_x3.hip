// Split-bf16 instantiations of the wave-specialised persistent NT GEMM (gemm_nt_ws.h, F8 = 3): fp32 operands in memory, split
// in registers after the LDS read into hi = bf16(x) and lo = bf16(x - hi), contracted as lo.hi + hi.lo + hi.hi on
// v_mfma_f32_16x16x32_bf16 with fp32 accumulation -- precision "bf16x3" (fp32-grade logits at bf16 matrix-core rates).
// fp32 output only, and only the epilogues the fp32 engine program asks for: plain, bias, bias + residual, bias + dropout +
// residual, and everything else (ReLU, fp32 relu_mask, residual without bias) through the generic form.
// A translation unit of its own so that its kernel variants compile beside gemm.hip's.
#include "gemm_nt_ws.h"

const char* dg_nt_ws_x3(const NtWsKey& k, const NtParams* p, int grid, hipStream_t s) {
    static const NtWsInstance rows[] = {NT_WS_INSTANCES_X3(NT_WS_ROW)};
    for (const NtWsInstance& r : rows) {
        if (!(r.key == k)) continue;
        if (p) hipLaunchKernelGGL(r.kernel, dim3(grid), dim3(NT_WS_BLOCK), 0, s, *p);
        return r.name;
    }
    return nullptr;
}
