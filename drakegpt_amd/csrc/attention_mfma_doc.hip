// The document-mask (DOC) instances of the bf16 MFMA attention kernels and their launches: attn_fwd_mfma_kernel<.., DOC = true> and
// attn_bwd_dq_mfma_kernel<TILES = true, .., DOC = true>.  The kernels are the templates of attention_mfma.hip, compiled here a
// second time for these instances only; that file's dg_attn_mfma_launch fills the launch parameters, looks the one launch that
// differs up in here (attn_row, attention_plan.h) and launches the unchanged dK/dV tile kernels itself.
// ref: Head2.forward src/model_component.py:392-405 with the tril mask of :401 cut at the document starts (dg_doc_starts).
#define DG_ATTN_MFMA_DOC_TU
#include "attention_mfma.hip"

#define ATTN_DOC_FWD_ROW(DROP, KEEP, F8) \
    {ATTN_FWD_KEY(DROP, KEEP, F8, true), "attn_fwd_mfma_kernel<" #DROP "," #KEEP "," #F8 ",true>", attn_fwd_mfma_kernel<DROP, KEEP, F8, true>, 4 * WAVE_LDS_FWD},
#define ATTN_DOC_DQ_ROW(TILES, KB, F8, SH) \
    {ATTN_DQ_KEY(TILES, KB, F8, SH, true), "attn_bwd_dq_mfma_kernel<" #TILES "," #KB "," #F8 "," #SH ",true>", attn_bwd_dq_mfma_kernel<TILES, KB, F8, SH, true>, ATTN_DQ_LDS(SH)},

const AttnRow* dg_attn_mfma_doc_fwd(int key, const AttnP* p, unsigned grid, hipStream_t s) {
    static const AttnRow rows[] = {ATTN_FWD_INSTANCES(ATTN_DOC_FWD_ROW)};
    const AttnRow* r = attn_find(rows, key);
    if (r && p) hipLaunchKernelGGL(r->kernel, dim3(grid), dim3(256), r->lds, s, *p);
    return r;
}
const AttnRow* dg_attn_mfma_doc_dq(int key, const AttnP* p, unsigned grid, hipStream_t s) {
    static const AttnRow rows[] = {ATTN_DQ_TILE_INSTANCES(ATTN_DOC_DQ_ROW)};
    const AttnRow* r = attn_find(rows, key);
    if (r && p) hipLaunchKernelGGL(r->kernel, dim3(grid), dim3(256), r->lds, s, *p);
    return r;
}
