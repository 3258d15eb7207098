// The launch plan of an attention call.  attn_plan (attention.hip) decides everything about a call of the six launch entries:
// return code, kernel family, block order, grid, the instance and dynamic LDS of every launch, every host-set kernel parameter
// that is not a caller's pointer, and what the query entries answer.  The entries launch what it returns (dg_attn_mfma_launch,
// dg_attn_simple_launch), the queries read it and dg_debug_attn_plan reports it.
#pragma once
#include "common.h"

// one of the six launch entries' arguments (forward: out and lse are written; dout, dqkv and the workspace are the backward's)
struct AttnCall {
    bool bwd;
    const void* qkv; const void* out; const void* dout; const float* lse; void* dqkv; void* workspace; int64_t workspace_bytes;
    int B, T, NH, H; float scale, dropout_p; const uint32_t* rng_state; uint32_t site; int dtype;
    const void* keep_bits; int64_t keep_bits_bytes; const dg_attn_fp8_out* fp8; const int32_t* starts;
};

enum { ATTN_F_SIMPLE = 0, ATTN_F_MFMA };              // attention_simple.hip, attention_mfma.hip + attention_mfma_doc.hip
enum { ATTN_FWD = 0, ATTN_DQ, ATTN_DKV };             // the passes: a forward call launches the first, a backward call the other two
enum { ATTN_BY_LENGTH = 1, ATTN_BY_SIZE };            // why the heavy-first order (balance 2) was chosen

struct AttnLaunch {
    int pass, key;             // key: ATTN_*_KEY of the MFMA instance; the generic family: 2 * dtype + (document mask)
    const char* name;
    int lds;                   // dynamic LDS bytes
    bool sinv;                 // the launch gets the fp8 copy's scale_inv pointer (the dK/dV pass does not: written by the dQ pass)
};
struct AttnPlan {
    int rc;                    // what the entry returns; only the query answers mean anything without DG_OK (n_launch = 0)
    int family;
    // the query entries: these read B, T, NH, H and dtype, nothing else.  mfma_ok: the shape fits the MFMA kernels (whatever the
    // dtype); delta_bytes: the [B,NH,T] delta floats at the head of the workspace, rounded up to 256 -- the offset of the tiles
    bool mfma_ok, fp8_out_ok;
    int64_t keep_bytes, workspace_bytes, delta_bytes;
    // MFMA family: AttnP's host-set fields; keep / tiles: AttnP::keep / AttnP::tiles are set; dq_no_drop: without dropout the dQ
    // pass runs with threshold 0, scale 1, site 0 and its key read from qkv
    int nblk; int64_t n_items;
    int balance, reason, rot_div;
    bool keep, tiles, dq_no_drop;
    // both families
    int drop; uint32_t thr; float inv_keep;
    unsigned grid;             // workgroups of 256 threads
    int n_launch; AttnLaunch launch[2];
};

// MFMA instances: a translation unit lists the instances it compiles as rows whose name and kernel address come out of one
// expansion, and has one lookup-and-launch function per pass.  Keys: the template arguments as bits.
struct AttnP;
struct AttnRow { int key; const char* name; void (*kernel)(AttnP); int lds; };
#define ATTN_DOC_BIT 32
#define ATTN_FWD_KEY(DROP, KEEP, F8, DOC) ((DROP) | (KEEP) << 1 | (F8) << 2 | (DOC) * ATTN_DOC_BIT)
#define ATTN_DQ_KEY(TILES, KB, F8, SH, DOC) ((TILES) | (KB) << 1 | (F8) << 2 | (SH) << 3 | (DOC) * ATTN_DOC_BIT)
#define ATTN_DKV_KEY(TILES, SHARED, X) ((TILES) | (SHARED) << 1 | (X) << 2)      // X: F8 with tiles, DROP without
template <size_t N>
inline const AttnRow* attn_find(const AttnRow (&rows)[N], int key) {
    for (const AttnRow& r : rows)
        if (r.key == key) return &r;
    return nullptr;
}
// The row of `key` in the unit's table, nullptr when there is none; with p, the instance is launched.
const AttnRow* dg_attn_mfma_fwd(int key, const AttnP* p, unsigned grid, hipStream_t s);        // attention_mfma.hip
const AttnRow* dg_attn_mfma_dq(int key, const AttnP* p, unsigned grid, hipStream_t s);
const AttnRow* dg_attn_mfma_dkv(int key, const AttnP* p, unsigned grid, hipStream_t s);
const AttnRow* dg_attn_mfma_doc_fwd(int key, const AttnP* p, unsigned grid, hipStream_t s);    // attention_mfma_doc.hip
const AttnRow* dg_attn_mfma_doc_dq(int key, const AttnP* p, unsigned grid, hipStream_t s);
inline const AttnRow* attn_row(int pass, int key, const AttnP* p, unsigned grid, hipStream_t s) {
    if (pass == ATTN_DKV) return dg_attn_mfma_dkv(key, p, grid, s);
    if (key & ATTN_DOC_BIT) return (pass == ATTN_FWD ? dg_attn_mfma_doc_fwd : dg_attn_mfma_doc_dq)(key, p, grid, s);
    return (pass == ATTN_FWD ? dg_attn_mfma_fwd : dg_attn_mfma_dq)(key, p, grid, s);
}

int dg_attn_mfma_launch(const AttnPlan& pl, const AttnCall& c, hipStream_t s);       // attention_mfma.hip
int dg_attn_simple_launch(const AttnPlan& pl, const AttnCall& c, hipStream_t s);     // attention_simple.hip
