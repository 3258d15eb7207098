// dg_attn_fwd / dg_attn_bwd and their fp8 / document-mask forms: the launch plan (attention_plan.h) between the generic VALU
// kernels (attention_simple.hip) and the bf16 MFMA flash kernels (attention_mfma.hip, attention_mfma_doc.hip; head size 64).
#include "attention_plan.h"

// the generic kernels by pass and 2 * dtype + (document mask)
#define ATTN_SIMPLE_NAMES(K) {K "<float,false>", K "<float,true>", K "<bf16_t,false>", K "<bf16_t,true>"}
static const char* const attn_simple_names[3][4] = {ATTN_SIMPLE_NAMES("attn_fwd_simple_kernel"), ATTN_SIMPLE_NAMES("attn_bwd_dq_simple_kernel"),
                                                    ATTN_SIMPLE_NAMES("attn_bwd_dkv_simple_kernel")};

// Pure host code: no pointer of the call is dereferenced but c.fp8 (a host struct), and the CU count comes in.
// Refusals: DG_ERR_ARG for everything but a keep_bits pointer off 16 bytes in a backward call on the MFMA kernels (DG_ERR_ALIGN;
// the forward call answers DG_ERR_ARG for the same pointer, as every misaligned operand or workspace does) and a dtype the
// generic kernels do not have (DG_ERR_DTYPE, after every other check of that family).
static AttnPlan attn_plan(const AttnCall& c, int ncu) {
    constexpr int HD = 64, TILE = 32;
    AttnPlan pl = {};
    const int B = c.B, T = c.T, NH = c.NH, H = c.H;
    const float dp = c.dropout_p;
    const bool pos = B > 0 && T > 0 && NH > 0, doc = c.starts != nullptr, f8 = c.fp8 != nullptr;
    auto refuse = [&pl](int rc) { pl.rc = rc; pl.n_launch = 0; return pl; };
    // the MFMA kernels: head size 64; T even: a lane's adjacent keys then form the element pairs that share a dropout hash;
    // 32-bit dropout element index; row offsets inside a batch slab are 24 x 24 -> 32-bit products (row_off)
    pl.mfma_ok = H == HD && pos && T % 2 == 0 && (int64_t)B * NH * T * T < ((int64_t)1 << 32) && T < (1 << 24) &&
                 3 * (int64_t)NH * HD < (1 << 24) && (int64_t)T * 3 * NH * HD < ((int64_t)1 << 32);
    pl.family = c.dtype == DG_BF16 && pl.mfma_ok ? ATTN_F_MFMA : ATTN_F_SIMPLE;
    const bool mfma = pl.family == ATTN_F_MFMA;
    pl.fp8_out_ok = mfma;
    // keep masks: 128 bytes per unmasked 32 x 32 tile; workspace: [B,NH,T] floats (delta), then -- MFMA family only, optional --
    // the P|dS tile scratch of the dQ pass, 4096 bytes per tile
    const int nblk = (T + TILE - 1) / TILE;
    const int64_t n_tiles = (int64_t)B * NH * ((int64_t)nblk * (nblk + 1) / 2);
    pl.delta_bytes = (((int64_t)B * NH * T * 4) + 255) / 256 * 256;
    pl.keep_bytes = mfma ? n_tiles * 128 : 0;
    pl.workspace_bytes = pos ? pl.delta_bytes + (mfma ? n_tiles * 4096 : 0) : 0;

    if (!c.qkv || !c.out || !c.lse || (c.bwd && (!c.dout || !c.dqkv || !c.workspace))) return refuse(DG_ERR_ARG);
    if (f8 && (!pl.fp8_out_ok || (c.bwd && c.workspace_bytes < pl.workspace_bytes))) return refuse(DG_ERR_ARG);
    if (c.keep_bits && c.keep_bits_bytes < pl.keep_bytes) return refuse(DG_ERR_ARG);
    if (c.bwd && (!pos || c.workspace_bytes < (int64_t)B * NH * T * 4 || !dg_aligned16(c.workspace))) return refuse(DG_ERR_ARG);
    pl.drop = (dp > 0.f && c.rng_state) ? 1 : 0;
    pl.thr = dg_drop_threshold(dp);
    pl.inv_keep = 1.f / (1.f - dp);
    pl.n_launch = c.bwd ? 2 : 1;
    for (int i = 0; i < pl.n_launch; ++i) pl.launch[i].pass = c.bwd + i;

    if (!mfma) {
        if (!pos || H <= 0 || H > 256 || T > 4096 || dp < 0.f || dp >= 1.f) return refuse(DG_ERR_ARG);
        if ((int64_t)B * NH * T * T >= ((int64_t)1 << 32)) return refuse(DG_ERR_ARG);   // 32-bit dropout element index
        if (c.dtype != DG_BF16 && c.dtype != DG_F32) return refuse(DG_ERR_DTYPE);
        pl.grid = (unsigned)(((int64_t)B * NH * T + 3) / 4);                             // one wave per row
        const int rows[3] = {T + H, T + 2 * H, 2 * T + 2 * H};                           // floats of LDS per wave, by pass
        for (int i = 0; i < pl.n_launch; ++i) {
            AttnLaunch& l = pl.launch[i];
            l.key = 2 * c.dtype + doc;
            l.name = attn_simple_names[l.pass][l.key];
            l.lds = 4 * rows[l.pass] * (int)sizeof(float);
        }
        return pl;
    }

    if (dp < 0.f || dp >= 1.f || !dg_aligned16(c.qkv) || !dg_aligned16(c.out)) return refuse(DG_ERR_ARG);
    if (c.bwd) {
        if (!dg_aligned16(c.dout) || !dg_aligned16(c.dqkv)) return refuse(DG_ERR_ARG);
        pl.tiles = c.workspace_bytes >= pl.workspace_bytes;       // (16-byte aligned with the workspace: delta_bytes % 256 == 0)
        if (doc && !pl.tiles) return refuse(DG_ERR_ARG);          // (the recompute form has no document variant)
        if (c.keep_bits && !dg_aligned16(c.keep_bits)) return refuse(DG_ERR_ALIGN);
        // keep masks: the tile form only (the recompute form's dQ loop would spill 16 registers with them; it hashes instead)
        pl.keep = c.keep_bits && pl.drop && pl.tiles;
    } else {
        if (c.keep_bits && !dg_aligned16(c.keep_bits)) return refuse(DG_ERR_ARG);
        pl.keep = c.keep_bits != nullptr;
        if (f8 && pl.drop && !pl.keep) return refuse(DG_ERR_ARG);
    }
    if (f8) {
        const dg_attn_fp8_out& o = *c.fp8;
        if (!o.q8 || !o.hist3 || !o.step_state || !o.scale_inv || !dg_aligned16(o.q8) || !dg_aligned16(o.hist3)) return refuse(DG_ERR_ARG);
        if (!c.bwd && o.only8) return refuse(DG_ERR_ARG);         // (the dQ pass reads the bf16 output: delta = rowsum(dO o))
    }
    pl.nblk = nblk;
    pl.n_items = (int64_t)B * NH * nblk;
    pl.grid = (unsigned)((pl.n_items + 3) / 4);                    // one wave per 32-row block
    pl.rot_div = ncu;
    // Block order: 0 plain, 1 = equal-cost pairs (nblk % 4 == 0), 2 = heavy first: when the launch is more than one residency (three
    // 256-thread workgroups per CU), and from 16 blocks on (T >= 512) at any size: with the K / V and Q / dO tiles shared by a
    // workgroup's waves the consecutive blocks of this order beat the equal-cost pairs at one residency too (GPT-2-small B = 8:
    // 11.75 / 11.65 -> 11.66 / 11.56 ms; no difference at the headline shape's 8 blocks)
    pl.balance = pl.nblk % 4 == 0 ? 1 : 0;
    if (pl.balance && pl.nblk >= 16) pl.reason = ATTN_BY_LENGTH;
    else if (pl.balance && (int64_t)B * NH * (pl.nblk / 4) > (int64_t)3 * ncu * 11 / 10) pl.reason = ATTN_BY_SIZE;
    if (pl.reason) pl.balance = 2;
    pl.dq_no_drop = !pl.drop;
    for (int i = 0; i < pl.n_launch; ++i) {
        AttnLaunch& l = pl.launch[i];
        // The dQ pass with shared K / V tiles (SH): the heavy-first order only, where a workgroup's four query blocks are CONSECUTIVE
        // (the shared loop runs to the last of them: three idle tiles at most).  In the equal-cost order (blocks j and nblk - 1 - j in
        // one workgroup) the short waves would sit at the barriers of the long ones: measured slower at the headline shape (2.326 /
        // 2.336 -> 2.344 / 2.342 ms) and no better at GPT-2-small B = 8.  The recompute form (no tiles) has the per-wave form only.
        // The tile pass with Q / dO tiles shared by a workgroup's waves: the balanced orders (a workgroup = four key blocks of ONE
        // (batch, head)).
        if (l.pass == ATTN_FWD) l.key = ATTN_FWD_KEY(pl.drop, pl.drop && pl.keep, f8, doc);
        else if (l.pass == ATTN_DQ) l.key = ATTN_DQ_KEY(pl.tiles, pl.keep, f8, pl.tiles && pl.balance == 2, doc);
        else l.key = pl.tiles ? ATTN_DKV_KEY(1, pl.balance != 0, f8) : ATTN_DKV_KEY(0, 0, pl.drop);
        l.sinv = f8 && l.pass != ATTN_DKV;
        const AttnRow* r = attn_row(l.pass, l.key, nullptr, 0, nullptr);
        if (!r) return refuse(DG_ERR_ARG);                        // no such instance: never a fallback
        l.name = r->name;
        l.lds = r->lds;
    }
    return pl;
}

static int attn_run(const AttnCall& c, void* stream) {
    const AttnPlan pl = attn_plan(c, dg_num_cus());
    if (pl.rc != DG_OK) return pl.rc;
    return (pl.family == ATTN_F_MFMA ? dg_attn_mfma_launch : dg_attn_simple_launch)(pl, c, (hipStream_t)stream);
}
// the query entries: fields of the plan of a call with these B, T, NH, H and dtype
static AttnPlan attn_query(int B, int T, int NH, int H, int dtype) {
    AttnCall c = {};
    c.B = B; c.T = T; c.NH = NH; c.H = H; c.dtype = dtype;
    return attn_plan(c, dg_num_cus());
}
extern "C" int64_t dg_attn_keep_bits_bytes(int B, int T, int NH, int H, int dtype) { return attn_query(B, T, NH, H, dtype).keep_bytes; }
extern "C" int dg_attn_fp8_out_supported(int B, int T, int NH, int H, int dtype) { return attn_query(B, T, NH, H, dtype).fp8_out_ok; }
extern "C" int64_t dg_attn_bwd_workspace_bytes(int B, int T, int NH, int H, int dtype) { return attn_query(B, T, NH, H, dtype).workspace_bytes; }

// The six launch entries: the parameters and arguments the three of a direction share, written once.  No fp8 / no starts: NULL.
#define ATTN_FWD_PARAMS const void* qkv, void* out, float* lse, int B, int T, int NH, int H, float scale, float dropout_p, \
                        const uint32_t* rng_state, uint32_t site, int dtype, void* keep_bits, int64_t keep_bits_bytes
#define ATTN_BWD_PARAMS const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, void* workspace, int64_t workspace_bytes, \
                        int B, int T, int NH, int H, float scale, float dropout_p, const uint32_t* rng_state, uint32_t site, int dtype, \
                        const void* keep_bits, int64_t keep_bits_bytes
#define ATTN_TAIL B, T, NH, H, scale, dropout_p, rng_state, site, dtype, keep_bits, keep_bits_bytes
extern "C" int dg_attn_fwd_doc(ATTN_FWD_PARAMS, const dg_attn_fp8_out* fp8, const int32_t* starts, void* stream) {
    return attn_run({false, qkv, out, nullptr, lse, nullptr, nullptr, 0, ATTN_TAIL, fp8, starts}, stream);
}
extern "C" int dg_attn_fwd_fp8(ATTN_FWD_PARAMS, const dg_attn_fp8_out* fp8, void* stream) {
    return attn_run({false, qkv, out, nullptr, lse, nullptr, nullptr, 0, ATTN_TAIL, fp8, nullptr}, stream);
}
extern "C" int dg_attn_fwd(ATTN_FWD_PARAMS, void* stream) {
    return attn_run({false, qkv, out, nullptr, lse, nullptr, nullptr, 0, ATTN_TAIL, nullptr, nullptr}, stream);
}
// With starts, a shape on the MFMA kernels needs the tile scratch (DG_ERR_ARG without).
extern "C" int dg_attn_bwd_doc(ATTN_BWD_PARAMS, const dg_attn_fp8_out* fp8, const int32_t* starts, void* stream) {
    return attn_run({true, qkv, out, dout, lse, dqkv, workspace, workspace_bytes, ATTN_TAIL, fp8, starts}, stream);
}
extern "C" int dg_attn_bwd_fp8(ATTN_BWD_PARAMS, const dg_attn_fp8_out* fp8, void* stream) {
    return attn_run({true, qkv, out, dout, lse, dqkv, workspace, workspace_bytes, ATTN_TAIL, fp8, nullptr}, stream);
}
extern "C" int dg_attn_bwd(ATTN_BWD_PARAMS, void* stream) {
    return attn_run({true, qkv, out, dout, lse, dqkv, workspace, workspace_bytes, ATTN_TAIL, nullptr, nullptr}, stream);
}

// diagnostic only (tests/attention_cases.py): the plan of the forward (bwd = 0: dout, dqkv and the workspace are ignored) or
// backward entry for these arguments on `ncu` compute units (0: the device's, 256 without one).  Pure host code that never launches
// and dereferences none of the pointers but fp8; not part of the public header.  out32: rc, family, mfma_ok, fp8_out_ok,
// keep_bytes, workspace_bytes, nblk, n_items, balance, reason, rot_div, grid, block, n_launch, drop, thr, inv_keep (bits), keep,
// tiles, tile offset, dq_no_drop, then per launch pass, key, lds, sinv.
extern "C" int dg_debug_attn_plan(int bwd, const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, void* workspace,
                                  int64_t workspace_bytes, int B, int T, int NH, int H, float dropout_p, const uint32_t* rng_state, int dtype,
                                  const void* keep_bits, int64_t keep_bits_bytes, const dg_attn_fp8_out* fp8, const int32_t* starts, int ncu,
                                  int64_t* out32, const char** names2) {
    if (ncu < 0 || !out32 || !names2) return DG_ERR_ARG;
    const AttnPlan pl = attn_plan({bwd != 0, qkv, out, dout, lse, dqkv, workspace, workspace_bytes, B, T, NH, H, 1.f, dropout_p, rng_state, 0, dtype,
                                   keep_bits, keep_bits_bytes, fp8, starts}, ncu > 0 ? ncu : dg_num_cus());
    const int64_t v[21] = {pl.rc, pl.family, pl.mfma_ok, pl.fp8_out_ok, pl.keep_bytes, pl.workspace_bytes, pl.nblk, pl.n_items, pl.balance,
                           pl.reason, pl.rot_div, pl.grid, 256, pl.n_launch, pl.drop, pl.thr, __builtin_bit_cast(uint32_t, pl.inv_keep), pl.keep,
                           pl.tiles, pl.tiles ? pl.delta_bytes : -1, pl.dq_no_drop};
    for (int i = 0; i < 32; ++i) out32[i] = i < 21 ? v[i] : 0;
    for (int i = 0; i < 2; ++i) {
        const AttnLaunch& l = pl.launch[i];
        const int64_t w[4] = {l.pass, l.key, l.lds, l.sinv};
        for (int j = 0; j < 4; ++j) out32[21 + 4 * i + j] = w[j];
        names2[i] = l.name ? l.name : "";
    }
    return DG_OK;
}
