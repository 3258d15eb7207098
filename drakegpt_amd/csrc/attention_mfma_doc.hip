// The document-mask (DOC) instances of the bf16 MFMA attention kernels and their launches: attn_fwd_mfma_kernel<.., DOC = true> and
// attn_bwd_dq_mfma_kernel<TILES = true, .., DOC = true>.  The kernels are the templates of attention_mfma.hip, compiled here a
// second time for these instances only; that file's host dispatch (dg_attn_fwd_mfma, dg_attn_bwd_mfma) fills the launch parameters,
// calls in here for the one launch that differs and launches the unchanged dK/dV tile kernels itself.
// ref: Head2.forward src/model_component.py:392-405 with the tril mask of :401 cut at the document starts (dg_doc_starts).
#define DG_ATTN_MFMA_DOC_TU
#include "attention_mfma.hip"

int dg_attn_fwd_mfma_doc(const AttnP& p, bool f8, dim3 grid, hipStream_t s) {
    const dim3 block(256);
    if (f8 && p.drop) hipLaunchKernelGGL((attn_fwd_mfma_kernel<true, true, true, true>), grid, block, 4 * WAVE_LDS_FWD, s, p);
    else if (f8) hipLaunchKernelGGL((attn_fwd_mfma_kernel<false, false, true, true>), grid, block, 4 * WAVE_LDS_FWD, s, p);
    else if (p.drop && p.keep) hipLaunchKernelGGL((attn_fwd_mfma_kernel<true, true, false, true>), grid, block, 4 * WAVE_LDS_FWD, s, p);
    else if (p.drop) hipLaunchKernelGGL((attn_fwd_mfma_kernel<true, false, false, true>), grid, block, 4 * WAVE_LDS_FWD, s, p);
    else hipLaunchKernelGGL((attn_fwd_mfma_kernel<false, false, false, true>), grid, block, 4 * WAVE_LDS_FWD, s, p);
    DG_LAUNCH_CHECK();
    return DG_OK;
}

// the shared dQ form in the heavy-first order, the per-wave form elsewhere: the rule of attn_dq_launch
template <bool KB, bool F8>
static void dq_launch_doc(const AttnP& p, dim3 grid, hipStream_t s) {
    if (p.balance == 2) hipLaunchKernelGGL((attn_bwd_dq_mfma_kernel<true, KB, F8, true, true>), grid, dim3(256), WG_LDS_DQS, s, p);
    else hipLaunchKernelGGL((attn_bwd_dq_mfma_kernel<true, KB, F8, false, true>), grid, dim3(256), 4 * WAVE_LDS_DQ, s, p);
}

void dg_attn_dq_mfma_doc(const AttnP& p, bool kb, bool f8, dim3 grid, hipStream_t s) {
    if (!f8) (kb ? dq_launch_doc<true, false> : dq_launch_doc<false, false>)(p, grid, s);
    else (kb ? dq_launch_doc<true, true> : dq_launch_doc<false, true>)(p, grid, s);
}
