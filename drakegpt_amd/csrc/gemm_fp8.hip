// fp8 instantiations of the wave-specialised persistent NT GEMM (gemm_nt_ws.h): OCP e4m3 weights x e4m3 activations (forward
// Linears) and e4m3 W^T x e5m2 gradients (dX), v_mfma_f32_16x16x128_f8f6f4, fp32 accumulation, per-tensor scales applied in the
// epilogue.  Replaces the operand type of the bf16 contractions behind every nn.Linear of the residual blocks
// (ref: src/model_component.py:320-325,392-393,404,454) for precision = "fp8" (BASELINE.json configs[4]).
// A translation unit of its own so that its ~30 kernel variants compile beside gemm.hip's.
#include "gemm_nt_ws.h"

// F8 = 1: A e4m3, F8 = 2: A e5m2 (B is always e4m3)
const char* dg_nt_ws_fp8(const NtWsKey& k, const NtParams* p, int grid, hipStream_t s) {
    static const NtWsInstance rows[] = {NT_WS_INSTANCES_E4M3(NT_WS_ROW) NT_WS_INSTANCES_E5M2(NT_WS_ROW)};
    for (const NtWsInstance& r : rows) {
        if (!(r.key == k)) continue;
        if (p) hipLaunchKernelGGL(r.kernel, dim3(grid), dim3(NT_WS_BLOCK), 0, s, *p);
        return r.name;
    }
    return nullptr;
}
