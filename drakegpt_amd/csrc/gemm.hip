// MFMA GEMMs for gfx950 (wave64): every nn.Linear forward, dX and dW of the training step.
//
//   dg_gemm_nt : C[M,N] = epi(A[M,K] . B[N,K]^T)  -- both operands K-contiguous, which is exactly
//                the 16x16 MFMA A/B fragment shape (8 bf16 / 4 f32 consecutive k per lane), so
//                fragments are single 16-byte LDS reads.  Forward Linears use B = W [out,in];
//                dX GEMMs use B = W^T (kept as a second shadow copy, refreshed by the optimizer).
//   dg_gemm_tn(_grouped) : dW[P,Q] = sum_r A[r,P] B[r,Q]  -- contraction over the strided row index;
//                bf16 fragments come from ds_read_b64_tr_b16 (hardware transpose read), f32 fragments
//                from plain 4-byte reads.
//
// Kernels in this file:
//   gemm_nt_ws_kernel          bf16, the default: persistent, 4 LDS-DMA loader waves + 8 MFMA waves per CU,
//                              128x192 / 128x128 tiles, register-only epilogue with compile-time variants
//   gemm_nt_kernel             fp32 parity mode (v_mfma_f32_16x16x4_f32 = exact fp32 FMA accumulation) and bf16
//                              shapes the default does not cover: 128x128 tile / 256 threads, register-prefetched
//                              global -> LDS staging, double-buffered XOR-swizzled LDS, LDS-staged epilogue
//   gemm_tn_grouped256_kernel  all dW of a backward pass in one launch, 256x128 tiles, chained K halves (bf16 and fp8)
//   gemm_tn_ws_kernel, gemm_tn_bf16_kernel, gemm_tn_f32_kernel   one dW per launch, split-K fp32 slabs
//   gemm_nt_x3_kernel, gemm_tn_x3_kernel   precision "bf16x3": fp32 operands split into bf16 hi + lo in registers,
//                              3 bf16 MFMAs per block (gemm_nt_kernel / gemm_tn_f32_kernel geometry); the wave-specialised
//                              split NT form is instantiated in gemm_x3.hip
// Earlier variants that were measured slower (LDS-DMA without loader waves, one tile per workgroup, 256x128 NT
// tiles, two co-resident workgroups per CU, 128x128 grouped dW tiles, 128x64 grouped dW wave tiles) are in the history
// of this file and listed in DESIGN.md section 4.  The kernel choice follows from the call's arguments alone.
#include "common.h"

#include "gemm_nt_ws.h"
#define NT_LDS_BYTES (4 * 64 * EPI_PITCH * 4)  // 69632: four 64x68 fp32 staging slices >= the 4 x 16 KB operand buffers


// Row-wise epilogue over a wave's staged fp32 tile (ROWS x 64, pitch EPI_PITCH floats): every lane
// handles 4 consecutive columns, so the global stores are whole 128/256-byte row segments instead of
// the MFMA C/D map's 2/4-byte scatter.  Order: +bias, ReLU, ReLU-mask, dropout, +residual, cast.
template <typename T, typename TO, int ROWS>
__device__ __forceinline__ void nt_epilogue(const float* stage, int row_base, int col_base, const NtParams& p, int lane) {
    uint32_t key = 0;
    if (p.drop) key = dg_site_key_dev(p.rng_state, p.site);
    TO* Cp = (TO*)p.C;
    const int ch = lane & 15;
    const int col = col_base + ch * 4;
    f32x4 bv = {0.f, 0.f, 0.f, 0.f};
    if (p.bias) {
#pragma unroll
        for (int e = 0; e < 4; ++e) bv[e] = (col + e < p.N) ? p.bias[col + e] : 0.f;
    }
    const bool full = p.vec_ok && (col + 3 < p.N);
#pragma unroll 4
    for (int it = 0; it < ROWS / 4; ++it) {
        const int lrow = it * 4 + (lane >> 4);
        const int row = row_base + lrow;
        if (row >= p.M || col >= p.N) continue;
        f32x4 v = *(const f32x4*)(&stage[lrow * EPI_PITCH + ch * 4]);
        v += bv;
        if (p.relu) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
        }
        if (p.relu_mask) {
            const T* mp = (const T*)p.relu_mask + (int64_t)row * p.ldmask + col;
            if (full && p.mask_vec_ok) {
                typedef T TV4 __attribute__((ext_vector_type(4)));
                const TV4 mk = *(const TV4*)mp;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = to_f32<T>(mk[e]) > 0.f ? v[e] : 0.f;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (col + e < p.N) v[e] = to_f32<T>(mp[e]) > 0.f ? v[e] : 0.f;
            }
        }
        if (p.drop) {
            const uint32_t i0 = (uint32_t)row * (uint32_t)p.N + (uint32_t)col;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = dg_keep(key, i0 + (uint32_t)e, p.thr) ? v[e] * p.inv_keep : 0.f;
        }
        if (p.residual) {
            const float* rp = p.residual + (int64_t)row * p.ldr + col;
            if (full) v += *(const f32x4*)rp;
            else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (col + e < p.N) v[e] += rp[e];
            }
        }
        TO* cp = Cp + (int64_t)row * p.ldc + col;
        if (full) {
            if (sizeof(TO) == 4) *(f32x4*)cp = v;
            else {
                bf16x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = (bf16_t)v[e];
                *(bf16x4*)cp = o;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (col + e < p.N) cp[e] = from_f32<TO>(v[e]);
        }
    }
}

// X3: fp32 operands contracted as split bf16 (precision "bf16x3"): a K step's two 16-byte chunks g and 4 + g of a row form one
// 8-float 16x16x32 fragment per lane (the same k set for A and B), split into hi / lo after the LDS read, 3 bf16 MFMAs per block
template <typename T, typename TO, bool X3>
__device__ __forceinline__ void gemm_nt_body(const NtParams& p) {
    static_assert(!X3 || sizeof(T) == 4, "split-bf16 operands are fp32");
    constexpr int EPC = MmaTraits<T>::EPC;
    constexpr int BK = 8 * EPC;                      // elements of K per step (128 bytes)
    __shared__ __attribute__((aligned(16))) char lds_raw[NT_LDS_BYTES];   // operands [buf][A|B][16 KB]; the epilogue staging reuses it
    char (*lds)[2][BM * 128] = reinterpret_cast<char (*)[2][BM * 128]>(lds_raw);

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform -> SGPR
    const int wm = wave >> 1, wn = wave & 1;
    const int tile = dg_xcd_remap(blockIdx.x, p.n_tiles);
    const int m0 = (tile / p.tiles_n) * BM, n0 = (tile % p.tiles_n) * BN;

    // staging map: 4 rows x 1 chunk per thread for A and for B
    const int ld_chunk = tid & 7, ld_row = tid >> 3;          // rows ld_row + 32*i
    const int nk = (p.K + BK - 1) / BK;

    u32x4 ra[4], rb[4];
    auto load_tile = [&](int kt) {
        const int k_el = kt * BK + ld_chunk * EPC;
        const bool kok = k_el < p.K;
        const int64_t kbyte = (int64_t)k_el * (int64_t)sizeof(T);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int r = ld_row + 32 * i;
            int gm = m0 + r, gn = n0 + r;
            ra[i] = (kok && gm < p.M) ? *(const u32x4*)(p.A + (int64_t)gm * p.lda_b + kbyte) : (u32x4){0u, 0u, 0u, 0u};
            rb[i] = (kok && gn < p.N) ? *(const u32x4*)(p.B + (int64_t)gn * p.ldb_b + kbyte) : (u32x4){0u, 0u, 0u, 0u};
        }
    };
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int r = ld_row + 32 * i;
            *(u32x4*)(&lds[buf][0][nt_lds_off(r, ld_chunk)]) = ra[i];
            *(u32x4*)(&lds[buf][1][nt_lds_off(r, ld_chunk)]) = rb[i];
        }
    };

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    load_tile(0);
    store_tile(0);
    __syncthreads();

    const int fr = lane & 15, fg = lane >> 4;
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) load_tile(kt + 1);              // in flight under the MFMAs below
        if constexpr (X3) {
            bf16x8 ah[4], al[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = wm * 64 + i * 16 + fr;
                dg_split_bf16(*(const u32x4*)(&lds[buf][0][nt_lds_off(r, fg)]), *(const u32x4*)(&lds[buf][0][nt_lds_off(r, 4 + fg)]),
                              ah[i], al[i]);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int r = wn * 64 + j * 16 + fr;
                bf16x8 bh, bl;
                dg_split_bf16(*(const u32x4*)(&lds[buf][1][nt_lds_off(r, fg)]), *(const u32x4*)(&lds[buf][1][nt_lds_off(r, 4 + fg)]),
                              bh, bl);
#pragma unroll
                for (int i = 0; i < 4; ++i) dg_mma16_x3(ah[i], al[i], bh, bl, acc[i][j]);
            }
        } else {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                u32x4 fa[4], fb[4];
                const int chunk = ks * 4 + fg;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    fa[i] = *(const u32x4*)(&lds[buf][0][nt_lds_off(wm * 64 + i * 16 + fr, chunk)]);
                    fb[i] = *(const u32x4*)(&lds[buf][1][nt_lds_off(wn * 64 + i * 16 + fr, chunk)]);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) mma16<T>(fa[i], fb[j], acc[i][j]);
            }
        }
        if (kt + 1 < nk) store_tile(buf ^ 1);
        __syncthreads();
    }

    // epilogue: each wave parks its 64x64 fp32 accumulator tile in a private LDS slice (the operand
    // buffers are free after the last barrier) and reads it back by rows (nt_epilogue).
    float* stage = (float*)lds_raw + wave * (64 * EPI_PITCH);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) stage[(i * 16 + fg * 4 + r) * EPI_PITCH + j * 16 + fr] = acc[i][j][r];
    __builtin_amdgcn_wave_barrier();
    nt_epilogue<T, TO, 64>(stage, m0 + wm * 64, n0 + wn * 64, p, lane);
}

template <typename T, typename TO>
__global__ __launch_bounds__(256) void gemm_nt_kernel(NtParams p) { gemm_nt_body<T, TO, false>(p); }
// precision "bf16x3": every shape the wave-specialised split form does not take (K % 32 != 0 or K < 128)
__global__ __launch_bounds__(256) void gemm_nt_x3_kernel(NtParams p) { gemm_nt_body<float, float, true>(p); }

static unsigned long long* g_stamp_buffer = nullptr;
// diagnostic only (tools/gemm_stamps.py): not part of the public header
extern "C" void dg_debug_set_stamp_buffer(void* p) { g_stamp_buffer = (unsigned long long*)p; }

// ---------------------------------------------------------------------------------------------
// NT launch plan.  Every decision of a dg_gemm_nt call, in one place: dg_gemm_nt launches what nt_plan returns, the query entries
// read the same plan and dg_debug_nt_plan reports it.  Pure host code: the CU count and whether a stamp buffer is set come in.
const char* dg_nt_ws_bf16(const NtWsKey& k, const NtParams* p, int grid, hipStream_t s) {
    static const NtWsInstance rows[] = {NT_WS_INSTANCES_BF16(NT_WS_ROW)};
    for (const NtWsInstance& r : rows) {
        if (!(r.key == k)) continue;
        if (p) hipLaunchKernelGGL(r.kernel, dim3(grid), dim3(NT_WS_BLOCK), 0, s, *p);
        return r.name;
    }
    return nullptr;
}
static const char* nt_ws_instance(const NtWsKey& k, const NtParams* p, int grid, hipStream_t s) {
    return k.f8 == 0 ? dg_nt_ws_bf16(k, p, grid, s) : (k.f8 == 3 ? dg_nt_ws_x3(k, p, grid, s) : dg_nt_ws_fp8(k, p, grid, s));
}
// the register-staged kernels, by (operands bf16) + (output bf16), and the split-bf16 one
#define NT_STAGED_ROW(...) {#__VA_ARGS__, __VA_ARGS__}
static const struct { const char* name; void (*kernel)(NtParams); } nt_staged[] = {
    NT_STAGED_ROW(gemm_nt_kernel<float,float>), NT_STAGED_ROW(gemm_nt_kernel<bf16_t,float>),
    NT_STAGED_ROW(gemm_nt_kernel<bf16_t,bf16_t>), NT_STAGED_ROW(gemm_nt_x3_kernel)};

// the options of a call that are present, as one mask
enum { NT_BIAS = 1, NT_RELU = 2, NT_MASK = 4, NT_DROP = 8, NT_RES = 16, NT_BITS_IN = 32, NT_BITS_OUT = 64, NT_COLSUM = 128, NT_FP8_OUT = 256,
       NT_VALUE_OPTS = 127 };                                   // the seven that change the output's values
// The specialised epilogues (what each one is: the EPI parameter of gemm_nt_ws_kernel, gemm_nt_ws.h) as data.  A call takes the
// form whose `need` options are all present and whose `never` options are all absent -- every value option the form does not
// name is in `never` --, with a bf16 output / the mask prefetch where the form asks for it; any other call, and every stamped
// run, takes EPI 0.
struct NtEpiForm { int epi, need, never; bool bf16_out, pf; };
static constexpr NtEpiForm nt_form(int epi, int need, int never_too, bool bf16_out, bool pf) {
    return {epi, need, (NT_VALUE_OPTS & ~need) | never_too, bf16_out, pf};
}
static constexpr NtEpiForm nt_epi_forms[] = {
    nt_form(1, 0, 0, false, false),
    nt_form(2, NT_BIAS | NT_RELU | NT_BITS_OUT, NT_FP8_OUT, true, false),
    nt_form(8, NT_BIAS | NT_RELU | NT_BITS_OUT | NT_FP8_OUT, 0, true, false),
    nt_form(3, NT_BIAS | NT_DROP | NT_RES, 0, false, false),
    nt_form(4, NT_BITS_IN, NT_COLSUM, true, true),
    nt_form(6, NT_BITS_IN | NT_COLSUM, NT_FP8_OUT, true, true),
    nt_form(9, NT_BITS_IN | NT_COLSUM | NT_FP8_OUT, 0, true, true),
    nt_form(5, NT_BIAS, 0, false, false),
    nt_form(7, NT_BIAS | NT_RES, 0, false, false),
};

// bytes of the lane-ordered bit mask: one bit per element of every (whole) output tile of the kernel that will run
static int64_t nt_sign_bits_bytes(int M, int N) {
    if (M <= 0 || N <= 0) return 0;
    const int bn = N % 192 == 0 ? 192 : 128;
    return (int64_t)((M + BM - 1) / BM) * ((N + bn - 1) / bn) * (BM * bn / 8);
}
// Column sums, one partial row per (workgroup, wave row) instead of one per 32 rows of C.  Tile t of workgroup b of G is
// remap(b + t G) = base(b % 8) + b / 8 + t G / 8, so with (G / 8) % tiles_n == 0 all tiles of a workgroup share one column block
// and it writes ONE partial row per wave row at the end: 4 G / tiles_n rows, indexed 4 rank + wave row with rank = (b % 8)
// (G / 8 / tiles_n) + (b / 8) / tiles_n, which numbers the workgroups of one column block 0 .. G / tiles_n - 1.
static bool nt_cs_accum(int G, int tiles_n) { return G % 8 == 0 && (G / 8) % tiles_n == 0; }

enum { NT_F_WS = 0, NT_F_STAGED, NT_F_X3 };                     // gemm_nt_ws_kernel, gemm_nt_kernel, gemm_nt_x3_kernel
struct NtPlan {
    int rc;                            // what dg_gemm_nt returns; everything down to q8_only is set only with DG_OK
    int family, staged;                // staged: row of nt_staged (families 1 and 2)
    NtWsKey inst;                      // family 0: the instance that runs (after the fallback rule below)
    const char* name;
    int grid, block;
    int esz, K, tiles_n, n_tiles, cs_accum, vec_ok, mask_vec_ok, warm_b, drop, q8_only;     // NtParams (K: in the kernel's units)
    // what the query entries report; these read M, N, K, ldc, the dtypes, C and which options are present, nothing else
    int bn;                            // tile width
    int sign_ok, colsum_ok, colsum_rows, fp8_out_ok;
    int64_t sign_bits_bytes;
};

static NtPlan nt_plan(const dg_gemm_nt_args& a, int ncu, bool stamps) {
    NtPlan pl = {};
    const bool bf16 = a.in_dtype == DG_BF16, e4m3 = a.in_dtype == DG_FP8_E4M3, e5m2 = a.in_dtype == DG_FP8_E5M2;
    const bool fp8 = e4m3 || e5m2, x3 = a.in_dtype == DG_F32X3, out_bf16 = a.out_dtype == DG_BF16;
    const int esz = fp8 ? 1 : (bf16 ? 2 : 4), osz = out_bf16 ? 2 : 4, epc = 16 / esz;
    const bool drop = a.dropout_p > 0.f && a.rng_state;
    const int opts = (a.bias ? NT_BIAS : 0) | (a.relu ? NT_RELU : 0) | (a.relu_mask ? NT_MASK : 0) | (drop ? NT_DROP : 0) |
                     (a.residual ? NT_RES : 0) | (a.sign_bits ? NT_BITS_IN : 0) | (a.sign_bits_out ? NT_BITS_OUT : 0) |
                     (a.colsum_part ? NT_COLSUM : 0) | (a.fp8_out ? NT_FP8_OUT : 0);

    // ---- what is offered
    const bool wide = a.N % 192 == 0;                           // 128 x 192 tiles of the wave-specialised kernel (otherwise 128 x 128)
    pl.bn = wide ? 192 : 128;
    pl.sign_bits_bytes = nt_sign_bits_bytes(a.M, a.N);
    pl.sign_ok = a.N > 0 && a.N % 8 == 0 && (bf16 ? a.K % 64 == 0 && a.K >= 128 : fp8 && a.K % 128 == 0 && a.K >= 256);
    // column sums and the fp8 copy: bf16 output, every tile whole and on the vector path, no stamp buffer
    const bool whole = pl.sign_ok && out_bf16 && !stamps && a.M % BM == 0 && a.N % pl.bn == 0 && a.ldc % 8 == 0 && dg_aligned16(a.C);
    // column sums: only the sign-bit-masked dX form (the one whose output is the pre-activation gradient a bias gradient is the
    // column sum of)
    pl.colsum_ok = whole && (opts & NT_VALUE_OPTS) == NT_BITS_IN;
    if (pl.colsum_ok) {
        const int tiles_n = a.N / pl.bn, n_tiles = (a.M / BM) * tiles_n, G = n_tiles < ncu ? n_tiles : ncu;
        pl.colsum_rows = nt_cs_accum(G, tiles_n) ? 4 * G / tiles_n : a.M / 32;
    }
    // fp8 copy of the output: (EPI 8) the bias + ReLU + sign-bit form with e4m3 operands -> e4m3 copy, or (EPI 9) the sign-bit-masked
    // dX form with column sums and e5m2 gradients -> e5m2 copy; exactly DG_FP8_AMAX_PARTS persistent workgroups (one partial maximum each)
    pl.fp8_out_ok = whole && ncu == DG_FP8_AMAX_PARTS && (int64_t)(a.M / BM) * (a.N / pl.bn) >= DG_FP8_AMAX_PARTS &&
                    (e4m3 ? (opts & ~NT_FP8_OUT) == (NT_BIAS | NT_RELU | NT_BITS_OUT) && dg_aligned16(a.bias)
                          : e5m2 && a.colsum_part && pl.colsum_ok);
    const NtPlan offers = pl;
    auto refuse = [&](int rc) { NtPlan r = offers; r.rc = rc; return r; };

    // ---- is the call valid
    if (!a.A || !a.B || !a.C || a.M <= 0 || a.N <= 0 || a.K <= 0) return refuse(DG_ERR_ARG);
    if (!bf16 && a.in_dtype != DG_F32 && !fp8 && !x3) return refuse(DG_ERR_DTYPE);
    if (!out_bf16 && a.out_dtype != DG_F32) return refuse(DG_ERR_DTYPE);
    if ((a.in_dtype == DG_F32 || x3) && out_bf16) return refuse(DG_ERR_DTYPE);
    if (fp8) {
        // B (the weight operand) is e4m3; per-tensor dequantisation factors are mandatory; only the LDS-DMA kernel has an fp8 form
        if (a.b_dtype != DG_FP8_E4M3 || !a.scale_a || !a.scale_b || a.relu_mask) return refuse(DG_ERR_ARG);
        if (a.K % 128 || a.K < 256) return refuse(DG_ERR_ARG);
    } else if (a.b_dtype != 0 && a.b_dtype != a.in_dtype && !(x3 && a.b_dtype == DG_F32)) return refuse(DG_ERR_DTYPE);
    if (a.K % epc || a.lda % epc || a.ldb % epc || !dg_aligned16(a.A) || !dg_aligned16(a.B)) return refuse(DG_ERR_ALIGN);
    if (a.lda < a.K || a.ldb < a.K || a.ldc < a.N) return refuse(DG_ERR_ARG);
    if (a.dropout_p < 0.f || a.dropout_p >= 1.f) return refuse(DG_ERR_ARG);
    if ((opts & (NT_BITS_IN | NT_BITS_OUT)) &&
        (!pl.sign_ok || a.sign_bits_bytes < pl.sign_bits_bytes || (a.sign_bits && a.relu_mask))) return refuse(DG_ERR_ARG);
    if (a.colsum_part && (!pl.colsum_ok || a.colsum_rows < pl.colsum_rows || a.colsum_ld < a.N || a.colsum_ld % 4 ||
                          !dg_aligned16(a.colsum_part))) return refuse(DG_ERR_ARG);
    if (a.fp8_out && (!pl.fp8_out_ok || !a.fp8_out_parts2 || !a.fp8_out_step || !a.fp8_out_scale_inv || a.ld_fp8_out < a.N ||
                      a.ld_fp8_out % 8 || (((uintptr_t)a.fp8_out) & 7))) return refuse(DG_ERR_ARG);

    // ---- what runs
    // split form (x3_ws): the wave-specialised kernel where K is whole 128-byte steps, at least two; the generic one otherwise
    const bool x3_ws = x3 && a.K % 32 == 0 && a.K >= 128;
    pl.esz = esz;
    pl.K = fp8 ? a.K / 2 : (x3_ws ? 2 * a.K : a.K);            // fp8 / split: K in 2-byte units, the kernel's K step is 128 BYTES
    pl.drop = drop;
    pl.q8_only = (a.fp8_out && a.fp8_out_only) ? 1 : 0;
    pl.vec_ok = (a.ldc % 4 == 0) && ((((uintptr_t)a.C) % (4 * osz)) == 0) &&
                (!a.residual || ((a.ldr % 4 == 0) && dg_aligned16(a.residual)));
    pl.mask_vec_ok = a.relu_mask && (a.ldmask % 4 == 0) && ((((uintptr_t)a.relu_mask) % (4 * esz)) == 0);
    {   // weights of at most 2 MB (every block Linear of the scaled model; not lm_head at the GPT-2 vocabulary), one touch per
        // lane (headline step: 2.498 -> 2.478 ms); warm_b = touch rounds of 2 MB each
        const int64_t wbytes = (int64_t)a.N * a.ldb * esz;
        pl.warm_b = (wbytes <= ((int64_t)2 << 20) && (a.ldb * esz) % 128 == 0 && (((uintptr_t)a.B) & 127) == 0) ? (int)((wbytes + (2 << 20) - 1) >> 21) : 0;
    }
    const int tiles_m = (a.M + BM - 1) / BM;
    if (!(fp8 || x3_ws || (bf16 && a.K % 64 == 0 && a.K >= 128))) {      // register-staged: one 128 x 128 tile per workgroup
        pl.family = x3 ? NT_F_X3 : NT_F_STAGED;
        pl.staged = x3 ? 3 : (bf16 ? 1 : 0) + (out_bf16 ? 1 : 0);
        pl.name = nt_staged[pl.staged].name;
        pl.tiles_n = (a.N + BN - 1) / BN;
        pl.n_tiles = tiles_m * pl.tiles_n;
        pl.grid = pl.n_tiles; pl.block = 256;
        return pl;
    }
    pl.family = NT_F_WS;
    pl.tiles_n = (a.N + pl.bn - 1) / pl.bn;
    pl.n_tiles = tiles_m * pl.tiles_n;
    pl.grid = pl.n_tiles < ncu ? pl.n_tiles : ncu;              // persistent: one workgroup per CU
    pl.block = NT_WS_BLOCK;
    pl.cs_accum = nt_cs_accum(pl.grid, pl.tiles_n) ? 1 : 0;
    // the mask bits of the sign-bit dX form are prefetched ahead of the epilogue
    const bool pf = a.sign_bits && pl.vec_ok && (!a.bias || dg_aligned16(a.bias)) && (a.ldc * osz) % 16 == 0 && dg_aligned16(a.C);
    if (pf && e4m3) return refuse(DG_ERR_ARG);                  // the mask-prefetch form only exists for the dX direction
    int epi = 0;
    for (const NtEpiForm& f : nt_epi_forms)
        if (!stamps && (opts & f.need) == f.need && !(opts & f.never) && (!f.bf16_out || out_bf16) && (!f.pf || pf)) epi = f.epi;
    // Fallback rule: the exact instance; else the same with EPI 0; else that without the prefetch.  (bf16 and split operands
    // always find the exact one: their lists hold every form their calls can classify as -- a split call cannot ask for a form
    // with a bf16 output.  fp8: fp32 output of forms 1 and 5, forward forms on e5m2 operands -> EPI 0; e5m2, prefetch, fp32
    // output -> EPI 0 without it.)
    pl.inst = {a.out_dtype, pf, wide ? 6 : 4, epi, e4m3 ? 1 : (e5m2 ? 2 : (x3 ? 3 : 0))};
    pl.name = nt_ws_instance(pl.inst, nullptr, 0, nullptr);
    if (!pl.name) { pl.inst.epi = 0; pl.name = nt_ws_instance(pl.inst, nullptr, 0, nullptr); }
    if (!pl.name) { pl.inst.pf = 0; pl.name = nt_ws_instance(pl.inst, nullptr, 0, nullptr); }
    return pl.name ? pl : refuse(DG_ERR_ARG);
}

// the query entries: fields of the plan of the call they are asked about
extern "C" int dg_gemm_nt_sign_bits_supported(const dg_gemm_nt_args* a) {
    return a ? nt_plan(*a, dg_num_cus(), g_stamp_buffer != nullptr).sign_ok : 0;
}
extern "C" int dg_gemm_nt_fp8_out_supported(const dg_gemm_nt_args* a) {
    return a ? nt_plan(*a, dg_num_cus(), g_stamp_buffer != nullptr).fp8_out_ok : 0;
}
extern "C" int dg_gemm_nt_colsum_supported(const dg_gemm_nt_args* a) {
    return a ? nt_plan(*a, dg_num_cus(), g_stamp_buffer != nullptr).colsum_ok : 0;
}
// number of partial rows the call writes (0 = not supported)
extern "C" int dg_gemm_nt_colsum_rows(const dg_gemm_nt_args* a) {
    return a ? nt_plan(*a, dg_num_cus(), g_stamp_buffer != nullptr).colsum_rows : 0;
}
extern "C" int64_t dg_gemm_nt_sign_bits_bytes(int M, int N) { return nt_sign_bits_bytes(M, N); }

extern "C" int dg_gemm_nt(const dg_gemm_nt_args* a, void* stream) {
    if (!a) return DG_ERR_ARG;
    const NtPlan pl = nt_plan(*a, dg_num_cus(), g_stamp_buffer != nullptr);
    if (pl.rc != DG_OK) return pl.rc;
    NtParams p;
    p.A = (const char*)a->A; p.lda_b = a->lda * pl.esz;
    p.B = (const char*)a->B; p.ldb_b = a->ldb * pl.esz;
    p.C = a->C; p.ldc = a->ldc;
    p.M = a->M; p.N = a->N; p.K = pl.K;
    p.bias = a->bias; p.relu = a->relu;
    p.relu_mask = a->relu_mask; p.ldmask = a->ldmask;
    p.bits_out = a->sign_bits_out; p.bits_in = a->sign_bits;
    p.colsum_part = a->colsum_part; p.colsum_ld = a->colsum_ld; p.cs_accum = pl.cs_accum;
    p.residual = a->residual; p.ldr = a->ldr;
    p.inv_keep = 1.f / (1.f - a->dropout_p);
    p.thr = dg_drop_threshold(a->dropout_p);
    p.drop = pl.drop;
    p.rng_state = a->rng_state; p.site = a->site;
    p.tiles_n = pl.tiles_n; p.n_tiles = pl.n_tiles;
    p.vec_ok = pl.vec_ok; p.mask_vec_ok = pl.mask_vec_ok;
    p.stamps = g_stamp_buffer;
    p.scale_a = a->scale_a; p.scale_b = a->scale_b;
    p.warm_b = pl.warm_b;
    p.q8 = (unsigned char*)a->fp8_out; p.ldq8 = a->ld_fp8_out; p.q8_only = pl.q8_only;
    p.q_parts2 = a->fp8_out_parts2; p.q_step = a->fp8_out_step; p.q_scale_inv = a->fp8_out_scale_inv;
    hipStream_t s = (hipStream_t)stream;
    if (pl.family == NT_F_WS) nt_ws_instance(pl.inst, &p, pl.grid, s);
    else hipLaunchKernelGGL(nt_staged[pl.staged].kernel, dim3(pl.grid), dim3(pl.block), 0, s, p);
    DG_LAUNCH_CHECK();
    return DG_OK;
}

// diagnostic only (tests/nt_cases.py): the plan of dg_gemm_nt(a) with `ncu` compute units (0: the device's, 256 without one) and
// a stamp buffer set or not.  Pure host code that never launches, not part of the public header.  out24: rc, family, the
// instance's out_dtype, PF, NJ, EPI, F8, grid, block, K, tiles_n, n_tiles, cs_accum, vec_ok, mask_vec_ok, warm_b, drop, q8_only,
// tile width, sign bits / column sums offered, colsum_rows, fp8 copy offered, sign_bits_bytes.
extern "C" int dg_debug_nt_plan(const dg_gemm_nt_args* a, int ncu, int stamps, int64_t* out24, const char** kernel_name) {
    if (!a || ncu < 0 || !out24) return DG_ERR_ARG;
    const NtPlan pl = nt_plan(*a, ncu > 0 ? ncu : dg_num_cus(), stamps != 0);
    const int64_t v[24] = {pl.rc, pl.family, pl.inst.out_dtype, pl.inst.pf, pl.inst.nj, pl.inst.epi, pl.inst.f8, pl.grid, pl.block,
                           pl.K, pl.tiles_n, pl.n_tiles, pl.cs_accum, pl.vec_ok, pl.mask_vec_ok, pl.warm_b, pl.drop, pl.q8_only,
                           pl.bn, pl.sign_ok, pl.colsum_ok, pl.colsum_rows, pl.fp8_out_ok, pl.sign_bits_bytes};
    for (int i = 0; i < 24; ++i) out24[i] = v[i];
    if (kernel_name) *kernel_name = pl.name ? pl.name : "";
    return DG_OK;
}

// =============================================================================================
// TN: out[P,Q] = sum_r A[r,P] * B[r,Q]
struct TnParams {
    const char* A; int64_t lda_b;
    const char* B; int64_t ldb_b;
    float* out; int64_t ldo; int64_t split_stride;
    int R, P, Q;
    int tiles_q, n_tiles;
    int r_per_split;
    int n_splits, xcd_map;     // xcd_map: 1-D grid, every split's tiles on one XCD (they share the same rows)
};

// (tile, split) of a workgroup.  Workgroups are dealt round-robin over the 8 XCDs (id % 8 labels the
// XCD group), and all tiles of one split read the same R rows of both operands: keeping a split on one
// XCD makes those rows L2 hits for every tile after the first.  Speed only, never correctness.
__device__ __forceinline__ void tn_work(const TnParams& p, int& tile, int& split) {
    if (!p.xcd_map) { tile = dg_xcd_remap(blockIdx.x, p.n_tiles); split = blockIdx.y; return; }
    const int id = blockIdx.x, x = id & 7, rest = id >> 3;
    if (p.n_splits >= 8) {
        const int g = p.n_splits >> 3;
        split = x + 8 * (rest % g);
        tile = rest / g;
    } else {
        const int share = 8 / p.n_splits;                    // XCDs per split
        split = x % p.n_splits;
        tile = rest * share + x / p.n_splits;
    }
}

// ---- bf16: [64 r][128 cols] tiles, 256-byte rows, dual-use image (b) of the guide (T10):
//      off(row, ch) = 256*row + 16*(ch ^ (((row&3)<<2) | ((row>>2)&3))),  ch = 16-byte chunk 0..15
__device__ __forceinline__ int tn_off_bf16(int row, int ch) {
    return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
}
// A 16(cols) x 8(r) fragment for the 16x16x32 MFMA, lane group g = lane>>4 supplying k = 8g..8g+7:
// two transposed reads of 4(r) x 16(cols) blocks.  col0 is a multiple of 16.
__device__ __forceinline__ u32x4 tn_frag_bf16(const char* tile, int r0, int col0, int lane) {
    const int i = lane & 15, q = i >> 2, pp = i & 3;
    const int c0 = col0 >> 3;
    typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
    const char* a0 = tile + tn_off_bf16(r0 + q, c0 + (pp >> 1)) + 8 * (pp & 1);
    const char* a1 = tile + tn_off_bf16(r0 + 4 + q, c0 + (pp >> 1)) + 8 * (pp & 1);
    bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)a0);
    bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)a1);
    bf16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(u32x4, v);
}

__global__ __launch_bounds__(256) void gemm_tn_bf16_kernel(TnParams p) {
    constexpr int BR = 64;
    __shared__ __attribute__((aligned(16))) char lds[2][2][BR * 256];      // 64 KB
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform -> SGPR
    const int wp = wave >> 1, wq = wave & 1;
    int tile, split;
    tn_work(p, tile, split);
    if (tile >= p.n_tiles) return;                          // padding of the 1-D grid (whole workgroup)
    const int p0 = (tile / p.tiles_q) * 128, q0 = (tile % p.tiles_q) * 128;
    const int r_begin = split * p.r_per_split;
    int r_end = r_begin + p.r_per_split; if (r_end > p.R) r_end = p.R;
    const int nk = r_end > r_begin ? (r_end - r_begin + BR - 1) / BR : 0;

    const int ld_ch = tid & 15, ld_row = tid >> 4;          // rows ld_row + 16*i, i < 4
    const bool a_ok = (p0 + ld_ch * 8) < p.P, b_ok = (q0 + ld_ch * 8) < p.Q;
    u32x4 ra[4], rb[4];
    auto load_tile = [&](int kt) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int r = r_begin + kt * BR + ld_row + 16 * i;
            bool rok = r < r_end;
            ra[i] = (rok && a_ok) ? *(const u32x4*)(p.A + (int64_t)r * p.lda_b + (int64_t)(p0 + ld_ch * 8) * 2) : (u32x4){0u, 0u, 0u, 0u};
            rb[i] = (rok && b_ok) ? *(const u32x4*)(p.B + (int64_t)r * p.ldb_b + (int64_t)(q0 + ld_ch * 8) * 2) : (u32x4){0u, 0u, 0u, 0u};
        }
    };
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int r = ld_row + 16 * i;
            *(u32x4*)(&lds[buf][0][tn_off_bf16(r, ld_ch)]) = ra[i];
            *(u32x4*)(&lds[buf][1][tn_off_bf16(r, ld_ch)]) = rb[i];
        }
    };

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    if (nk > 0) { load_tile(0); store_tile(0); }
    __syncthreads();
    const int fg = lane >> 4;
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) load_tile(kt + 1);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            u32x4 fa[4], fb[4];
            const int r0 = ks * 32 + fg * 8;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                fa[i] = tn_frag_bf16(&lds[buf][0][0], r0, wp * 64 + i * 16, lane);
                fb[i] = tn_frag_bf16(&lds[buf][1][0], r0, wq * 64 + i * 16, lane);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) mma16<bf16_t>(fa[i], fb[j], acc[i][j]);
        }
        if (kt + 1 < nk) store_tile(buf ^ 1);
        __syncthreads();
    }
    float* out = p.out + (int64_t)split * p.split_stride;
    const int fr = lane & 15;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = q0 + wq * 64 + j * 16 + fr;
        if (col >= p.Q) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = p0 + wp * 64 + i * 16 + fg * 4 + r;
                if (row < p.P) out[(int64_t)row * p.ldo + col] = acc[i][j][r];
            }
    }
}

// ---- bf16, wave-specialised LDS-DMA form (as gemm_nt_ws_kernel): 8 MFMA waves (4 x 2 of 32 x 64) + 4 loader waves
// ---- (description of the shared structure:) 8 waves (4 x 2 of 32 x 64), 4 stages of [64 r][128 cols] x 2 operands,
//      global_load_lds writes image (b) directly (per-lane SOURCE chunk = slot ^ f(row)), counted
//      vmcnt + one raw barrier per K step, fragments of the next half step always in flight.
//      Requires whole 64-row steps (R % 64 == 0); column tails read clamped (finite) data that only
//      reaches outputs which are not stored.  Accumulators transposed (mfma(B, A)): 16-byte stores.
__global__ __launch_bounds__(768) void gemm_tn_ws_kernel(TnParams p) {
    __shared__ __attribute__((aligned(16))) char lds[GL_NST * GL_STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform -> SGPR
    const int wp = wave >> 1, wq = wave & 1;
    int tile, split;
    tn_work(p, tile, split);
    if (tile >= p.n_tiles) return;                          // padding of the 1-D grid (whole workgroup)
    const int p0 = (tile / p.tiles_q) * 128, q0 = (tile % p.tiles_q) * 128;
    const int r_begin = split * p.r_per_split;
    int r_end = r_begin + p.r_per_split; if (r_end > p.R) r_end = p.R;
    const int nk = r_end > r_begin ? (r_end - r_begin) / 64 : 0;

    // piece = 1 KB = 4 rows x 256 B; this wave moves pieces 2w, 2w+1 of A and of B per stage
    const int prow = lane >> 4, slot = lane & 15;
    const bool loader = wave >= 8;
    const int lw = wave - 8;
    const char* srcA[4];
    const char* srcB[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int q = 4 * (loader ? lw : 0) + i;
        const int row = 4 * q + prow;
        const int chunk = slot ^ ((prow << 2) | (q & 3));           // f(row) of image (b): ((row&3)<<2)|((row>>2)&3)
        int ca = p0 + chunk * 8; if (ca + 8 > p.lda_b / 2) ca = 0;   // past the leading dimension: clamp
        int cb = q0 + chunk * 8; if (cb + 8 > p.ldb_b / 2) cb = 0;
        srcA[i] = p.A + (int64_t)(r_begin + row) * p.lda_b + (int64_t)ca * 2;
        srcB[i] = p.B + (int64_t)(r_begin + row) * p.ldb_b + (int64_t)cb * 2;
    }
    auto issue = [&](int kt) {
        char* base = lds + (kt & (GL_NST - 1)) * GL_STAGE + (4 * lw) * 1024;
        const int64_t ra = (int64_t)kt * 64 * p.lda_b, rb = (int64_t)kt * 64 * p.ldb_b;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            __builtin_amdgcn_global_load_lds((gptr_t)(srcA[i] + ra), (lptr_t)(base + i * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((gptr_t)(srcB[i] + rb), (lptr_t)(base + 16384 + i * 1024), 16, 0, 0);
        }
    };
    if (loader) {
        if (nk > 0) {
            const int npre = nk < GL_NST - 1 ? nk : GL_NST - 1;
            for (int g = 0; g < npre; ++g) issue(g);
            if (npre >= 3) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
            else if (npre == 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            for (int g = 0; g + 1 < nk; ++g) {
                int issued = g + GL_NST - 1; if (issued > nk) issued = nk;
                if (issued - (g + 2) >= 1) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                if (g + GL_NST - 1 < nk) issue(g + GL_NST - 1);
            }
        }
        return;
    }
    f32x4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int fr = lane & 15, fg = lane >> 4;
    auto read_frags = [&](u32x4 (&fa)[2], u32x4 (&fb)[4], const char* buf, int ks) {
        const int r0 = ks * 32 + fg * 8;
#pragma unroll
        for (int i = 0; i < 2; ++i) fa[i] = tn_frag_bf16(buf, r0, wp * 32 + i * 16, lane);
#pragma unroll
        for (int j = 0; j < 4; ++j) fb[j] = tn_frag_bf16(buf + 16384, r0, wq * 64 + j * 16, lane);
    };
    auto mma_all = [&](const u32x4 (&fa)[2], const u32x4 (&fb)[4]) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) mma16<bf16_t>(fb[j], fa[i], acc[i][j]);
    };
    if (nk > 0) {
        u32x4 fa0[2], fb0[4], fa1[2], fb1[4];
        __builtin_amdgcn_s_barrier();                              // stage 0 published by the loaders
        read_frags(fa0, fb0, lds, 0);
        for (int g = 0; g < nk; ++g) {
            const char* buf = lds + (g & (GL_NST - 1)) * GL_STAGE;
            read_frags(fa1, fb1, buf, 1);
            mma_all(fa0, fb0);
            if (g + 1 < nk) {
                __builtin_amdgcn_s_barrier();
                read_frags(fa0, fb0, lds + ((g + 1) & (GL_NST - 1)) * GL_STAGE, 0);
            }
            mma_all(fa1, fb1);
        }
    }
    float* out = p.out + (int64_t)split * p.split_stride;
    const bool vec = (p.ldo % 4 == 0) && ((((uintptr_t)out) & 15) == 0);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = p0 + wp * 32 + i * 16 + fr;
        if (row >= p.P) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = q0 + wq * 64 + j * 16 + 4 * fg;
            float* op = out + (int64_t)row * p.ldo + col;
            if (vec && col + 3 < p.Q) *(f32x4*)op = acc[i][j];
            else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (col + e < p.Q) op[e] = acc[i][j][e];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Grouped dW GEMM: every weight gradient of the step in one persistent launch.  Same stage format,
// loader / MFMA wave split and fragment reads as gemm_tn_ws_kernel, but a workgroup walks its tiles
// (of any problem of the group) with ONE continuous stage pipeline and each tile runs over the whole
// contraction, so there are no split-K slabs to write, re-read and reduce (they were ~790 MB per step)
// and no per-matrix launch: 651 tiles of 256 K steps instead of 25 launches of <= 256 short workgroups.
#define TN_MAX_GROUP 64                       // 40 + 64 x 56 = 3624 B of kernel arguments (limit 4 KB): GPT-2-small's 49 matrices in one launch
struct TnProblem {
    const char* A; const char* B; float* out;
    int lda_b, ldb_b, ldo;                    // byte strides of A and B (< 2 GB), element stride of out
    int P, Q, R, tiles_q, tile_begin;
};
// ws: split-K workspace, [total_tiles][8 waves][16 KB] fp32 partials of THIS launch; flags: [total_tiles][8] hand-over words at a
// place every launch of the call shares -- behind the partial area of the call's LARGEST launch (tn_group_most_tiles), so that
// no launch's flags lie in bytes another launch of the same call uses for partials
struct TnGroup { int n, total_tiles; int splits, tiles_pad; char* ws; unsigned* flags; unsigned* err; TnProblem pr[TN_MAX_GROUP]; };
// fp8 operands (round 3): e5m2 dY x e4m3 X with one dequantisation factor per operand (device scalars).  Two more pointers per
// problem: 48 problems per launch keep the kernel arguments under 4 KB (40 + 48 x 72 = 3496 B; GPT-2-medium's 96 block matrices:
// two launches).
#define TN_MAX_GROUP8 48
struct TnProblem8 {
    const char* A; const char* B; float* out;
    const float* sa; const float* sb;         // dW = sa[0] * sb[0] * sum_r qA qB
    int lda_b, ldb_b, ldo;
    int P, Q, R, tiles_q, tile_begin;
};
struct TnGroup8 { int n, total_tiles; int splits, tiles_pad; char* ws; unsigned* flags; unsigned* err; TnProblem8 pr[TN_MAX_GROUP8]; };
static_assert(sizeof(TnGroup) <= 4096 && sizeof(TnGroup8) <= 4096, "kernel arguments: 4 KB");
template <bool F8> struct TnGroupOf { typedef TnGroup type; };
template <> struct TnGroupOf<true> { typedef TnGroup8 type; };

// ---------------------------------------------------------------------------------------------
// 256 x 128 output tiles for the grouped dW GEMM: 8 MFMA waves in 4 x 2, wave tile 64 x 64, two MFMA waves per SIMD, each
// reading a whole stage and then issuing its 32 MFMAs.  The dW K step is bound by the transposed LDS reads
// (ds_read_b64_tr_b16: ~5 cycles each; tools/fillbench.hip): 256 per K step and CU against 1024 MFMA cycles.  A 64 x 64 wave
// tile needs 32 of them per 32 MFMAs where a 32 x 64 one (128 x 128 output tiles) needs 24 per 16.  Stage = three
// [64 r][128 cols] images (A columns 0..127, A columns 128..255, B) = 48 KB, three stages.  The kernel is also closer to its
// HBM bound than to its LDS bound: 1.87 GB in 455 us = 4.1 TB/s of the ~5.2 TB/s the chip sustains.
// The straight K loop below overlaps by itself: the two MFMA waves of a SIMD drift apart and one's reads run under the other's
// MFMAs.  The alternatives measured slower (128 x 64 wave tiles on 4 MFMA waves, the NT kernel's barrier-in-the-middle loop,
// 128 x 128 output tiles) are listed in DESIGN.md section 4.
#define TN2_STAGE 49152
#define TN2_NST 3
// F8 (round 3): OCP fp8 operands -- A = dY as e5m2, B = X as e4m3, the copies the fp8 forward / dX GEMMs already made of
// them.  A stage is 128 rows of the contraction instead of 64 at the same 48 KB (three [128 r][128 B] images), read with
// ds_read_b64_tr_b8 (per 16-lane group an 8-row x 16-byte-column block, lane i receiving column i's eight rows; lane 2 r + h
// supplies row r, bytes 8 h .. 8 h + 7 -- probed with tools/tr8_probe.hip) and multiplied with ONE v_mfma_f32_16x16x128_f8f6f4
// per 16 x 16 block: per 128 rows the same 32 transposed reads per wave as the bf16 form needs for 64, half the operand bytes from
// HBM, 16 MFMAs instead of 32.  Swizzle of the image: physical 16-byte chunk = chunk ^ (((row >> 1) & 3) | (((row >> 5) & 1) << 2))
// -- rows two apart share their banks (128-byte rows, 64 banks), the two 16-lane groups of a half-wave read rows 32 apart.
// WT is always 0 (64 x 64 wave tiles): it stays a template parameter only to keep the kernel symbol that bench.py's labels name.
template <int WT, bool F8 = false>
__global__ __launch_bounds__(768) void gemm_tn_grouped256_kernel(typename TnGroupOf<F8>::type gp) {
    static_assert(WT == 0, "64 x 64 wave tiles only");
    constexpr int KROWS = F8 ? 128 : 64;           // rows of the contraction per stage
    __shared__ __attribute__((aligned(16))) char lds[TN2_NST * TN2_STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform -> SGPR
    const int G = gridDim.x;
    // Work items: (tile, K half).  With splits == 2 every tile is cut into two K halves handled by different workgroups one
    // round apart (all first halves come first in the item order): 381 tiles on 256 CUs then cost 3 rounds of 128 K steps
    // instead of 2 rounds of 256.  The first half publishes its accumulators (per wave: 16 KB + a flag, agent-scope
    // release); the second half adds them after its own K range -- first + second, a fixed order -- and stores.
    // splits == 3 ("split the leftover only"): with T = q G + r tiles, every workgroup runs q whole tiles and only the r
    // leftover tiles are cut in two.  The role goes by XCD (b & 7): even XCDs run the first half of a leftover tile FIRST and
    // then their whole tiles, odd XCDs their whole tiles and the second half LAST -- the partial is published a whole tile
    // before it is needed, and all workgroups of one XCD stay at the same K offset of neighbouring tiles (role by workgroup
    // parity put neighbours 128 K steps apart: no operand sharing in L2, +15 us).  XCD pair (2m, 2m+1), workgroup j = b >> 3
    // of it: leftover tile 8 (j >> 1) + 2m + (j & 1), i.e. 16 consecutive tiles of each of the two tile ranges.  For the
    // scaled model (384 tiles, 256 CUs) that is the same 384 K steps per workgroup as cutting every tile, with a third of
    // the partial traffic (128 instead of 384 tiles x 128 KB written and read back) and a third of the hand-overs.
    const int q_whole = gp.total_tiles / G;
    const int lo_x = (int)blockIdx.x & 7, lo_j = (int)blockIdx.x >> 3;
    const int lo_tile = (gp.splits == 3) ? q_whole * G + 8 * (lo_j >> 1) + 2 * (lo_x >> 1) + (lo_j & 1) : 0;
    const bool lo_have = gp.splits == 3 && lo_tile < gp.total_tiles;
    const int lo_half = lo_x & 1;
    const int n_items = gp.splits == 3 ? 0 : gp.splits * gp.tiles_pad;
    const int my_items = gp.splits == 3 ? q_whole + (lo_have ? 1 : 0) : (n_items - (int)blockIdx.x + G - 1) / G;
    struct Item { int pi, p0, q0, ka, kb, tile, half; };         // half: 0 first (publishes), 1 second (adds, stores), 2 whole tile
    auto item = [&](int ii, Item& x) -> bool {                   // false: padding item (nothing to do)
        int tl;
        if (gp.splits == 3) {
            const bool is_half = lo_have && (lo_half == 0 ? ii == 0 : ii == q_whole);
            if (is_half) { x.half = lo_half; tl = lo_tile; }
            else { x.half = 2; tl = (int)blockIdx.x + (ii - ((lo_have && lo_half == 0) ? 1 : 0)) * G; }
        } else {
            const int it = (int)blockIdx.x + ii * G;
            x.half = it / gp.tiles_pad;
            tl = it - x.half * gp.tiles_pad;
            if (gp.splits == 1) x.half = 2;
        }
        if (tl >= gp.total_tiles) return false;
        x.tile = dg_xcd_remap(tl, gp.total_tiles);
        int pi = 0;
        for (int i = 1; i < gp.n; ++i)
            if (x.tile >= gp.pr[i].tile_begin) pi = i;
        const int local = x.tile - gp.pr[pi].tile_begin;
        x.pi = pi;
        x.p0 = (local / gp.pr[pi].tiles_q) * 256; x.q0 = (local % gp.pr[pi].tiles_q) * 128;
        const int nk = gp.pr[pi].R / KROWS, mid = nk / 2;
        x.ka = x.half == 1 ? mid : 0; x.kb = x.half == 0 ? mid : nk;
        return true;
    };
    int total = 0;
    for (int ii = 0; ii < my_items; ++ii) {
        Item x;
        if (item(ii, x)) total += x.kb - x.ka;
    }
    if (total == 0) return;

    if (wave >= 8) {
        // ---- loader role: 48 pieces of 1 KB (4 rows x 256 B) per stage, 12 per wave: pieces 0-15 -> image A0, 16-31 -> A1, 32-47 -> B
        const int lw = wave - 8;
        const int prow = lane >> 4, slot = lane & 15;
        const char* src[12];
        int64_t step[12];
        int nk_iss = 1, iss_item = -1;
        auto set_src = [&]() {                                    // advance to the next real item
            Item x;
            do { if (++iss_item >= my_items) return; } while (!item(iss_item, x));
            const auto& pr = gp.pr[x.pi];
            nk_iss = x.kb - x.ka;
            if constexpr (F8) {
                // piece = 8 rows x 128 B of one image: lane (row-in-piece, physical chunk) fetches the logical chunk the swizzle puts there
                const int prow8 = lane >> 3, slot8 = lane & 7;
#pragma unroll
                for (int i = 0; i < 12; ++i) {
                    const int pc = 12 * lw + i, img = pc >> 4, q = pc & 15;
                    const int rloc = 8 * q + prow8;
                    const int chunk = slot8 ^ (((rloc >> 1) & 3) | (((rloc >> 5) & 1) << 2));
                    const bool isB = img == 2;
                    const int64_t ld_b = isB ? pr.ldb_b : pr.lda_b;
                    int c = (isB ? x.q0 : x.p0 + img * 128) + chunk * 16;
                    if (c + 16 > ld_b) c = 0;                     // past the leading dimension: clamp
                    src[i] = (isB ? pr.B : pr.A) + (int64_t)(x.ka * 128 + rloc) * ld_b + c;
                    step[i] = 128 * ld_b;
                }
                return;
            }
#pragma unroll
            for (int i = 0; i < 12; ++i) {
                const int pc = 12 * lw + i, img = pc >> 4, q = pc & 15;
                const int row = x.ka * 64 + 4 * q + prow;
                const int chunk = slot ^ ((prow << 2) | (q & 3));
                const bool isB = img == 2;
                const int64_t ld_b = isB ? pr.ldb_b : pr.lda_b;
                int c = (isB ? x.q0 : x.p0 + img * 128) + chunk * 8;
                if (c + 8 > ld_b / 2) c = 0;                      // past the leading dimension: clamp
                src[i] = (isB ? pr.B : pr.A) + (int64_t)row * ld_b + (int64_t)c * 2;
                step[i] = 64 * ld_b;
            }
        };
        int iss_kt = 0, iss_buf = 0;
        auto issue = [&]() {
            char* base = lds + iss_buf * TN2_STAGE + (12 * lw) * 1024;
#pragma unroll
            for (int i = 0; i < 12; ++i)
                __builtin_amdgcn_global_load_lds((gptr_t)(src[i] + (int64_t)iss_kt * step[i]), (lptr_t)(base + i * 1024), 16, 0, 0);
            if (++iss_buf == TN2_NST) iss_buf = 0;
            if (++iss_kt == nk_iss) { iss_kt = 0; set_src(); }
        };
        // All three buffers stay busy: the consumers read BOTH K halves of stage g right after barrier g-1, so its buffer is
        // free again at barrier g and stage g+3 is issued there -- two K steps before it is needed.
        set_src();
        const int npre = total < TN2_NST ? total : TN2_NST;
        for (int g = 0; g < npre; ++g) issue();
        if (npre >= 3) asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
        else if (npre == 2) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                              // stage 0 published
        for (int g = 0; g + 1 < total; ++g) {
            int issued = g + TN2_NST; if (issued > total) issued = total;
            if (issued - (g + 2) >= 1) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");   // stage g+1 landed, g+2 may fly
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();                          // publishes stage g+1; stage g's buffer is free
            if (g + TN2_NST < total) issue();
        }
        return;
    }

    // ---- MFMA role
    const int wp = wave >> 1, wq = wave & 1;       // wp 0..3: 64 rows each
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int fr = lane & 15, fg = lane >> 4;
    const int aimg = (wp >> 1) * 16384, acol = (wp & 1) * 64;
    // The same addresses as tn_frag_bf16(buf + image, ks * 32 + fg * 8, col0 + 16 i, lane), from four per-lane offsets instead
    // of sixteen: a wave's col0 is a multiple of 64 and 16 i only sets bits 1, 2 of the chunk index, which the swizzle XORs, so
    // fragment i lies at (fragment 0) ^ 32 i -- taken after the stage offset (a multiple of 16 KB) is added, so that the sixteen
    // addresses are not hoisted out of the K loop as invariants again -- and ks adds 32 rows (8 KB).
    int offA[2], offB[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int row = fg * 8 + 4 * h + (fr >> 2), sub = ((fr & 3) >> 1), byte = 8 * (fr & 1);
        offA[h] = aimg + tn_off_bf16(row, (acol >> 3) + sub) + byte;
        offB[h] = 32768 + tn_off_bf16(row, wq * 8 + sub) + byte;
    }
    auto read_frags = [&](u32x4 (&fa)[4], u32x4 (&fb)[4], int stage_off, int ks) {
        typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
        auto frag = [&](int lo_off, int hi_off) -> u32x4 {
            bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(lds + lo_off));
            bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(lds + hi_off));
            return __builtin_bit_cast(u32x4, (bf16x8)__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
        };
#pragma unroll
        for (int i = 0; i < 4; ++i)
            fa[i] = frag(((stage_off + offA[0]) ^ (32 * i)) + ks * 8192, ((stage_off + offA[1]) ^ (32 * i)) + ks * 8192);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            fb[j] = frag(((stage_off + offB[0]) ^ (32 * j)) + ks * 8192, ((stage_off + offB[1]) ^ (32 * j)) + ks * 8192);
    };
    auto mma_all = [&](const u32x4 (&fa)[4], const u32x4 (&fb)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) mma16<bf16_t>(fb[j], fa[i], acc[i][j]);
    };
    Item cx;
    int cur_item = -1;
    auto next_item = [&]() {
        do { if (++cur_item >= my_items) return; } while (!item(cur_item, cx));
    };
    next_item();
    auto store_tile = [&]() {
        const auto& pr = gp.pr[cx.pi];
        if (cx.half != 2) {
            // per wave 4 x 4 accumulators of 1 KB (64 lanes x 16 B): 16 KB
            float* part = (float*)(gp.ws + ((size_t)cx.tile * 8 + wave) * 16384);
            unsigned* flag = gp.flags + cx.tile * 8 + wave;
            // The partials move as (64 lanes x 16 B) pieces with the sc0 sc1 cache bits: system-scope write-through
            // stores and L2-bypassing loads, i.e. coherent between XCDs without any cache-wide maintenance.  (One relaxed
            // agent-scope atomic per float -- the portable spelling -- cost ~30 us per hand-over.)
            char* pw = (char*)part + lane * 16;
            if (cx.half == 0) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" :: "v"(pw + (i * 4 + j) * 1024), "v"(acc[i][j]) : "memory");
                    }
                // the flag is an agent-scope atomic too, so ordering needs only "my stores have been acknowledged": a
                // workgroup-scope fence.  An agent-scope release / acquire pair would write back and invalidate the whole L2
                // of the XCD on every hand-over, which made this kernel 2x slower than not splitting at all.
                // The accumulators pass through the wait: that keeps their registers allocated and untouched until every
                // store has read its data (the hazard logic that protects a store's data registers does not see through
                // inline asm -- without this the compiler recycled them for the next store's address).
                asm volatile("s_waitcnt vmcnt(0)"
                             : "+v"(acc[0][0]), "+v"(acc[0][1]), "+v"(acc[0][2]), "+v"(acc[0][3]), "+v"(acc[1][0]), "+v"(acc[1][1]),
                               "+v"(acc[1][2]), "+v"(acc[1][3]), "+v"(acc[2][0]), "+v"(acc[2][1]), "+v"(acc[2][2]), "+v"(acc[2][3]),
                               "+v"(acc[3][0]), "+v"(acc[3][1]), "+v"(acc[3][2]), "+v"(acc[3][3])
                             :: "memory");
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                if (lane == 0) __hip_atomic_store(flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
                return;
            }
            // Bounded wait (~1 s): the producer is an earlier item of a LOWER-numbered workgroup that never waits itself (see the
            // launch rules in dg_gemm_tn_grouped), so under in-order dispatch this resolves in microseconds.  If it ever does
            // not (CU mask, a broken build), give up instead of hanging the GPU: the sticky error word marks the result invalid.
            for (unsigned spin = 0; __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u; ++spin) {
                if (spin >= (1u << 22)) { if (lane == 0) __hip_atomic_store(gp.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break; }
                __builtin_amdgcn_s_sleep(8);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#pragma unroll
            for (int c = 0; c < 2; ++c) {                      // eight 1 KB pieces at a time (32 registers)
                f32x4 t[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1" : "=v"(t[k]) : "v"(pw + (c * 8 + k) * 1024) : "memory");
                // one wait for all eight; the values pass through it so that nothing reads them earlier
                asm volatile("s_waitcnt vmcnt(0)"
                             : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]), "+v"(t[4]), "+v"(t[5]), "+v"(t[6]), "+v"(t[7])
                             :: "memory");
#pragma unroll
                for (int k = 0; k < 8; ++k) acc[2 * c + (k >> 2)][k & 3] += t[k];
            }
            __builtin_amdgcn_wave_barrier();
            if (lane == 0) __hip_atomic_store(flag, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
        }
        float* out = pr.out;
        const bool vec = (pr.ldo % 4 == 0) && ((((uintptr_t)out) & 15) == 0);
        if constexpr (F8) {
            const float sab = pr.sa[0] * pr.sb[0];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] *= sab;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = cx.p0 + wp * 64 + i * 16 + fr;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int col = cx.q0 + wq * 64 + j * 16 + 4 * fg;
                if (row < pr.P) {
                    float* op = out + (int64_t)row * pr.ldo + col;
                    if (vec && col + 3 < pr.Q) *(f32x4*)op = acc[i][j];
                    else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (col + e < pr.Q) op[e] = acc[i][j][e];
                    }
                }
                acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
        }
    };
    u32x4 fa0[4], fb0[4], fa1[4], fb1[4];
    __builtin_amdgcn_s_barrier();                                  // stage 0 published by the loaders
    int kt = 0, buf_i = 0;
    if constexpr (F8) {
        typedef int i32x2 __attribute__((ext_vector_type(2)));
        typedef int i32x8 __attribute__((ext_vector_type(8)));
        typedef __attribute__((address_space(3))) i32x2 lds_i32x2;
        typedef __attribute__((address_space(3))) char lds_char8;
        lds_char8* const lbase = (lds_char8*)lds;
        // lane l of a 16-lane group supplies row (l >> 1), byte 8 (l & 1) of the group's 8 x 16 block; group fg takes rows 32 fg ..
        // 32 fg + 31 of the stage in four blocks of eight (+ 1024 bytes each): its lane then holds 32 consecutive k of one column
        const int l16 = lane & 15, swz = ((l16 >> 2) & 3) | ((fg & 1) << 2);
        const int rowbase = (32 * fg + (l16 >> 1)) * 128 + 8 * (l16 & 1);
        const int abase = (wp >> 1) * 16384 + rowbase, bbase = 32768 + rowbase;
        auto frag8 = [&](int a) -> i32x8 {
            i32x2 v0 = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_i32x2*)(lbase + a));
            i32x2 v1 = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_i32x2*)(lbase + a + 1024));
            i32x2 v2 = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_i32x2*)(lbase + a + 2048));
            i32x2 v3 = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_i32x2*)(lbase + a + 3072));
            return (i32x8){v0[0], v0[1], v1[0], v1[1], v2[0], v2[1], v3[0], v3[1]};
        };
        for (int g = 0; g < total; ++g) {
            const int sb = buf_i * TN2_STAGE;
            i32x8 fa[4], fb[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) fa[i] = frag8(sb + abase + ((((wp & 1) * 4 + i) ^ swz) << 4));
#pragma unroll
            for (int j = 0; j < 4; ++j) fb[j] = frag8(sb + bbase + (((wq * 4 + j) ^ swz) << 4));
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)      // first operand X (e4m3: cbsz 0), second dY (e5m2: blgp 1), unit block scales
                    acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fb[j], fa[i], acc[i][j], 0, 1, 0, 0, 0, 0);
            if (++buf_i == TN2_NST) buf_i = 0;
            if (++kt == cx.kb - cx.ka) {
                store_tile();
                kt = 0;
                next_item();
            }
            if (g + 1 < total) {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // every read of stage g has returned: the loaders refill its buffer
                __builtin_amdgcn_s_barrier();
            }
        }
    } else {
        // One counted loop per item inside the loop over all stages: the same stages, barriers and stores in the same order as one
        // flat loop with an item counter.  Together with the four-offset fragment addresses above it is what lets the register
        // allocator keep the 64 accumulators in place across the item switch: 166 VGPRs and no scratch, where the flat loop
        // with sixteen hoisted addresses spilled 218 registers and reloaded accumulators between the stores of every
        // epilogue (460 -> 422 us per launch at the headline shapes).
        for (int g = 0; g < total;) {
            const int nkc = cx.kb - cx.ka;
            for (int k = 0; k < nkc; ++k) {
                read_frags(fa0, fb0, buf_i * TN2_STAGE, 0);
                read_frags(fa1, fb1, buf_i * TN2_STAGE, 1);
                mma_all(fa0, fb0);
                mma_all(fa1, fb1);
                if (++buf_i == TN2_NST) buf_i = 0;
                if (k + 1 == nkc) {
                    store_tile();
                    next_item();
                }
                if (++g < total) {
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // every read of stage g has returned: the loaders refill its buffer
                    __builtin_amdgcn_s_barrier();
                }
            }
            if (nkc <= 0) next_item();                             // (the host never builds an empty K range)
        }
    }
}

// ---- f32: [32 r][128 cols] tiles with 144-float row pitch (pad 16 floats: rows r, r+1 of one
//      ds_read_b32 half-wave land on different banks)
#define TNF_PITCH 144
// X3 (precision "bf16x3"): the 32 rows of a stage are ONE 16x16x32 bf16 k block.  Lane group g supplies rows 4e + g (e < 8) of its
// column -- 8 scalar LDS reads per fragment, the f32 kernel's count per row, and rows 4 apart per group keep the reads of a wave
// on distinct banks as there -- split into hi / lo, 3 bf16 MFMAs per block.  Same k permutation for A and B.
template <bool X3>
__device__ __forceinline__ void gemm_tn_f32_body(const TnParams& p) {
    constexpr int BR = 32;
    __shared__ __attribute__((aligned(16))) float lds[2][2][BR * TNF_PITCH];     // 73.7 KB
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform -> SGPR
    const int wp = wave >> 1, wq = wave & 1;
    int tile, split;
    tn_work(p, tile, split);
    if (tile >= p.n_tiles) return;                          // padding of the 1-D grid (whole workgroup)
    const int p0 = (tile / p.tiles_q) * 128, q0 = (tile % p.tiles_q) * 128;
    const int r_begin = split * p.r_per_split;
    int r_end = r_begin + p.r_per_split; if (r_end > p.R) r_end = p.R;
    const int nk = r_end > r_begin ? (r_end - r_begin + BR - 1) / BR : 0;

    const int ld_ch = tid & 31, ld_row = tid >> 5;          // rows ld_row + 8*i, i < 4
    const bool a_ok = (p0 + ld_ch * 4) < p.P, b_ok = (q0 + ld_ch * 4) < p.Q;
    u32x4 ra[4], rb[4];
    auto load_tile = [&](int kt) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int r = r_begin + kt * BR + ld_row + 8 * i;
            bool rok = r < r_end;
            ra[i] = (rok && a_ok) ? *(const u32x4*)(p.A + (int64_t)r * p.lda_b + (int64_t)(p0 + ld_ch * 4) * 4) : (u32x4){0u, 0u, 0u, 0u};
            rb[i] = (rok && b_ok) ? *(const u32x4*)(p.B + (int64_t)r * p.ldb_b + (int64_t)(q0 + ld_ch * 4) * 4) : (u32x4){0u, 0u, 0u, 0u};
        }
    };
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int r = ld_row + 8 * i;
            *(u32x4*)(&lds[buf][0][r * TNF_PITCH + ld_ch * 4]) = ra[i];
            *(u32x4*)(&lds[buf][1][r * TNF_PITCH + ld_ch * 4]) = rb[i];
        }
    };
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    if (nk > 0) { load_tile(0); store_tile(0); }
    __syncthreads();
    const int fr = lane & 15, fg = lane >> 4;
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) load_tile(kt + 1);
        if constexpr (X3) {
            bf16x8 ah[4], al[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float x[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) x[e] = lds[buf][0][(4 * e + fg) * TNF_PITCH + wp * 64 + i * 16 + fr];
                dg_split_bf16(x, ah[i], al[i]);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float x[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) x[e] = lds[buf][1][(4 * e + fg) * TNF_PITCH + wq * 64 + j * 16 + fr];
                bf16x8 bh, bl;
                dg_split_bf16(x, bh, bl);
#pragma unroll
                for (int i = 0; i < 4; ++i) dg_mma16_x3(ah[i], al[i], bh, bl, acc[i][j]);
            }
        } else {
#pragma unroll
            for (int ks = 0; ks < BR / 4; ++ks) {
                float fa[4], fb[4];
                const int r = ks * 4 + fg;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    fa[i] = lds[buf][0][r * TNF_PITCH + wp * 64 + i * 16 + fr];
                    fb[i] = lds[buf][1][r * TNF_PITCH + wq * 64 + i * 16 + fr];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
            }
        }
        if (kt + 1 < nk) store_tile(buf ^ 1);
        __syncthreads();
    }
    float* out = p.out + (int64_t)split * p.split_stride;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = q0 + wq * 64 + j * 16 + fr;
        if (col >= p.Q) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = p0 + wp * 64 + i * 16 + fg * 4 + r;
                if (row < p.P) out[(int64_t)row * p.ldo + col] = acc[i][j][r];
            }
    }
}

__global__ __launch_bounds__(256) void gemm_tn_f32_kernel(TnParams p) { gemm_tn_f32_body<false>(p); }
__global__ __launch_bounds__(256) void gemm_tn_x3_kernel(TnParams p) { gemm_tn_f32_body<true>(p); }

// Every decision of a dg_gemm_tn launch, in one place: dg_gemm_tn launches what this returns and dg_debug_tn_plan reports it.
enum { TN_K_WS = 0, TN_K_BF16, TN_K_F32, TN_K_X3 };
static const char* const tn_kernel_names[] = {"gemm_tn_ws_kernel", "gemm_tn_bf16_kernel", "gemm_tn_f32_kernel", "gemm_tn_x3_kernel"};
struct TnPlan { int kernel, xcd_map, grid_x, grid_y, block, r_per_split, tiles_q, n_tiles; };
static TnPlan tn_plan(int R, int P, int Q, int n_splits, int dtype, int ncu) {
    TnPlan pl;
    pl.tiles_q = (Q + 127) / 128;
    pl.n_tiles = ((P + 127) / 128) * pl.tiles_q;
    const int br = dtype == DG_BF16 ? 64 : 32;
    const int per = (R + n_splits - 1) / n_splits;
    pl.r_per_split = ((per + br - 1) / br) * br;
    pl.xcd_map = (n_splits % 8 == 0 || n_splits == 1 || n_splits == 2 || n_splits == 4) ? 1 : 0;
    pl.grid_x = pl.n_tiles; pl.grid_y = n_splits;
    if (pl.xcd_map) {
        const int per_x = n_splits >= 8 ? pl.n_tiles * (n_splits / 8) : (pl.n_tiles + (8 / n_splits) - 1) / (8 / n_splits);
        pl.grid_x = per_x * 8; pl.grid_y = 1;
    }
    // the LDS-DMA kernel owns a CU (128 KB LDS): use it when the launch fits one wave of workgroups,
    // otherwise two register-staged workgroups per CU finish sooner than a second round
    const bool one_round = (int64_t)pl.n_tiles * n_splits <= ncu;
    if (dtype == DG_BF16) pl.kernel = (R % 64 == 0 && one_round) ? TN_K_WS : TN_K_BF16;
    else pl.kernel = dtype == DG_F32X3 ? TN_K_X3 : TN_K_F32;
    pl.block = pl.kernel == TN_K_WS ? 768 : 256;
    return pl;
}

extern "C" int dg_gemm_tn(const void* A, int64_t lda, const void* B, int64_t ldb,
                          float* out, int64_t ldo, int64_t split_stride, int n_splits,
                          int R, int P, int Q, int dtype, void* stream) {
    if (!A || !B || !out || R <= 0 || P <= 0 || Q <= 0 || n_splits <= 0) return DG_ERR_ARG;
    if (dtype != DG_BF16 && dtype != DG_F32 && dtype != DG_F32X3) return DG_ERR_DTYPE;
    const int esz = dtype == DG_BF16 ? 2 : 4, epc = 16 / esz;
    if (lda % epc || ldb % epc || !dg_aligned16(A) || !dg_aligned16(B)) return DG_ERR_ALIGN;
    if (lda < P || ldb < Q || ldo < Q) return DG_ERR_ARG;
    if (((P + epc - 1) / epc) * epc > lda || ((Q + epc - 1) / epc) * epc > ldb) return DG_ERR_ARG;
    if (n_splits > 1 && split_stride < (int64_t)(P - 1) * ldo + Q) return DG_ERR_ARG;
    const TnPlan pl = tn_plan(R, P, Q, n_splits, dtype, dg_num_cus());
    TnParams p;
    p.A = (const char*)A; p.lda_b = lda * esz;
    p.B = (const char*)B; p.ldb_b = ldb * esz;
    p.out = out; p.ldo = ldo; p.split_stride = split_stride;
    p.R = R; p.P = P; p.Q = Q;
    p.tiles_q = pl.tiles_q;
    p.n_tiles = pl.n_tiles;
    p.r_per_split = pl.r_per_split;
    p.n_splits = n_splits;
    p.xcd_map = pl.xcd_map;
    const dim3 grid(pl.grid_x, pl.grid_y), block(pl.block);
    hipStream_t s = (hipStream_t)stream;
    switch (pl.kernel) {
    case TN_K_WS: hipLaunchKernelGGL(gemm_tn_ws_kernel, grid, block, 0, s, p); break;
    case TN_K_BF16: hipLaunchKernelGGL(gemm_tn_bf16_kernel, grid, block, 0, s, p); break;
    case TN_K_X3: hipLaunchKernelGGL(gemm_tn_x3_kernel, grid, block, 0, s, p); break;
    default: hipLaunchKernelGGL(gemm_tn_f32_kernel, grid, block, 0, s, p); break;
    }
    DG_LAUNCH_CHECK();
    return DG_OK;
}

// diagnostic only (tests/tn_cases.py): the plan dg_gemm_tn would launch with `ncu` compute units (0: the device's).  Pure host
// code, not part of the public header.  out8: kernel, xcd_map, grid_x, grid_y, block, r_per_split, tiles_q, n_tiles.
extern "C" int dg_debug_tn_plan(int R, int P, int Q, int n_splits, int dtype, int ncu, int* out8, const char** kernel_name) {
    if (R <= 0 || P <= 0 || Q <= 0 || n_splits <= 0 || ncu < 0 || !out8) return DG_ERR_ARG;
    if (dtype != DG_BF16 && dtype != DG_F32 && dtype != DG_F32X3) return DG_ERR_DTYPE;
    const TnPlan pl = tn_plan(R, P, Q, n_splits, dtype, ncu > 0 ? ncu : dg_num_cus());
    out8[0] = pl.kernel; out8[1] = pl.xcd_map; out8[2] = pl.grid_x; out8[3] = pl.grid_y;
    out8[4] = pl.block; out8[5] = pl.r_per_split; out8[6] = pl.tiles_q; out8[7] = pl.n_tiles;
    if (kernel_name) *kernel_name = tn_kernel_names[pl.kernel];
    return DG_OK;
}

static int64_t tn_group_tiles(const dg_tn_problem* problems, int n) {
    int64_t tiles = 0;
    for (int i = 0; i < n; ++i) tiles += (int64_t)((problems[i].P + 255) / 256) * ((problems[i].Q + 127) / 128);
    return tiles;
}
// tiles of the largest launch of a call, whichever operand kind it is made with: the function below has no dtype argument, and
// bf16 calls are cut into launches of TN_MAX_GROUP problems, fp8 calls into launches of TN_MAX_GROUP8
static int64_t tn_group_most_tiles(const dg_tn_problem* problems, int n) {
    int64_t most = 0;
    for (int maxg : {TN_MAX_GROUP, TN_MAX_GROUP8})
        for (int base = 0; base < n; base += maxg) {
            const int64_t t = tn_group_tiles(problems + base, n - base < maxg ? n - base : maxg);
            if (t > most) most = t;
        }
    return most;
}
#define TN_PART_BYTES (8 * 16384)             // partials per 256 x 128 tile: 8 MFMA waves x 16 KB
// split-K workspace of a call: [most][8 x 16 KB] wave partials, [most][8] flags, the sticky error word (last 16 bytes), with
// most = the tiles of the call's largest launch.  Every launch of the call puts its partials at the front and its flags at
// most * TN_PART_BYTES (tn_grouped_plan), wherever its own partials end.
extern "C" int64_t dg_gemm_tn_grouped_workspace_bytes(const dg_tn_problem* problems, int n) {
    if (!problems || n <= 0) return 0;
    return tn_group_most_tiles(problems, n) * (TN_PART_BYTES + 8 * 4) + 16;
}

// Every decision of ONE launch of a dg_gemm_tn_grouped call (problems [first, first + count)), in one place: tn_grouped_launch
// launches what this returns and dg_debug_tn_grouped_plan reports it.  flag_offset / ws_need: bytes from the workspace's start
// (ws_need: how far this launch reads or writes it, the error word included; 0 for a launch that is not cut).
struct TnGroupPlan { int first, count, tiles, tiles_pad, splits, grid; int64_t flag_offset, ws_need; };
static TnGroupPlan tn_grouped_plan(const dg_tn_problem* problems, int n, int first, bool f8, bool with_ws, int ncu) {
    const int maxg = f8 ? TN_MAX_GROUP8 : TN_MAX_GROUP, krows = f8 ? 128 : 64;
    TnGroupPlan pl;
    pl.first = first;
    pl.count = n - first < maxg ? n - first : maxg;
    int nk_min = 1 << 30, nk_max = 0;
    for (int i = 0; i < pl.count; ++i) {
        const int nk = problems[first + i].R / krows;
        if (nk < nk_min) nk_min = nk;
        if (nk > nk_max) nk_max = nk;
    }
    const int tiles = (int)tn_group_tiles(problems + first, pl.count);
    pl.tiles = tiles;
    pl.tiles_pad = (tiles + 7) / 8 * 8;
    pl.splits = 1;
    if (with_ws && nk_min >= 2) {
        // two K halves per tile when that shortens the schedule: rounds x steps per round
        const int64_t whole = (int64_t)((tiles + ncu - 1) / ncu) * nk_max;
        const int64_t halves = (int64_t)((2 * pl.tiles_pad + ncu - 1) / ncu) * ((nk_max + 1) / 2);
        // Cutting EVERY tile is only taken when each workgroup gets one item (2 tiles_pad <= #CUs): the second half of tile t
        // (workgroup tiles_pad + t) then waits for workgroup t, a lower-numbered one that never waits -- safe whatever part of
        // the grid is resident.  With several items per workgroup the second halves of tiles [G - tiles_pad % G, G) would sit
        // on LOWER-numbered workgroups than their producers: a deadlock as soon as fewer than G workgroups are resident.
        // (With a CU count that is a multiple of 16 the leftover cut below is at least as short whenever cutting every tile
        // would shorten a multi-round schedule, so the guard only decides on other CU counts.)
        if (halves < whole && 2 * pl.tiles_pad <= ncu) pl.splits = 2;
        // cut only the leftover tiles when their halves fit into one half round (see the kernel)
        const int r = tiles % ncu;
        if (tiles > ncu && ncu % 16 == 0 && r > 0 && 16 * ((r + 7) / 8) <= ncu) {
            const int64_t lo = (int64_t)(tiles / ncu) * nk_max + (nk_max + 1) / 2;
            if (lo <= (pl.splits == 2 ? halves : whole)) pl.splits = 3;
        }
    }
    const int items = pl.splits == 3 ? tiles : pl.splits * pl.tiles_pad;
    pl.grid = items < ncu ? items : ncu;
    pl.flag_offset = tn_group_most_tiles(problems, n) * TN_PART_BYTES;
    // a cut launch uses its partials (tiles <= most: they end at or before flag_offset), its flags and the error word at the
    // very end of the call's workspace; an uncut one touches none of it
    pl.ws_need = pl.splits == 1 ? 0 : dg_gemm_tn_grouped_workspace_bytes(problems, n);
    return pl;
}

// diagnostic only (tests/tn_cases.py): the launches of dg_gemm_tn_grouped(problems, n, dtype, workspace or NULL) with `ncu`
// compute units (0: the device's), one row of 8 int64 per launch: first problem, problems, tiles, tiles_pad, splits, grid,
// flag offset, workspace bytes needed.  Reads R, P, Q of the problems only; pure host code, not part of the public header.
// Returns the number of launches (at most max_rows are written), or a negative error code.
extern "C" int dg_debug_tn_grouped_plan(const dg_tn_problem* problems, int n, int dtype, int with_workspace, int ncu,
                                        int64_t* rows8, int max_rows) {
    if (!problems || n <= 0 || ncu < 0 || (!rows8 && max_rows > 0)) return DG_ERR_ARG;
    const bool f8 = dtype == DG_FP8_E5M2;
    if (dtype != DG_BF16 && !f8) return DG_ERR_DTYPE;
    for (int i = 0; i < n; ++i)
        if (problems[i].R <= 0 || problems[i].P <= 0 || problems[i].Q <= 0 || problems[i].R % (f8 ? 128 : 64)) return DG_ERR_ARG;
    int launches = 0;
    for (int base = 0; base < n; base += f8 ? TN_MAX_GROUP8 : TN_MAX_GROUP, ++launches) {
        if (launches >= max_rows) continue;
        const TnGroupPlan pl = tn_grouped_plan(problems, n, base, f8, with_workspace != 0, ncu > 0 ? ncu : dg_num_cus());
        int64_t* o = rows8 + 8 * launches;
        o[0] = pl.first; o[1] = pl.count; o[2] = pl.tiles; o[3] = pl.tiles_pad; o[4] = pl.splits; o[5] = pl.grid;
        o[6] = pl.flag_offset; o[7] = pl.ws_need;
    }
    return launches;
}

template <typename GroupT, typename ProbT, bool F8, int MAXG>
static int tn_grouped_launch(const dg_tn_problem* problems, int n, void* workspace, int64_t workspace_bytes, hipStream_t s) {
    constexpr int ESZ = F8 ? 1 : 2;
    static_assert(MAXG == (F8 ? TN_MAX_GROUP8 : TN_MAX_GROUP), "tn_grouped_plan cuts the call the same way");
    const int ncu = dg_num_cus();
    // nothing is launched unless every launch of the call has its room
    for (int base = 0; base < n; base += MAXG)
        if (tn_grouped_plan(problems, n, base, F8, workspace != nullptr, ncu).ws_need > workspace_bytes) return DG_ERR_ARG;
    for (int base = 0; base < n; base += MAXG) {
        const TnGroupPlan pl = tn_grouped_plan(problems, n, base, F8, workspace != nullptr, ncu);
        GroupT gp;
        gp.n = pl.count;
        int tiles = 0;
        for (int i = 0; i < gp.n; ++i) {
            const dg_tn_problem& q = problems[base + i];
            ProbT& t = gp.pr[i];
            t.A = (const char*)q.A; t.B = (const char*)q.B; t.out = q.out;
            t.lda_b = (int)(q.lda * ESZ); t.ldb_b = (int)(q.ldb * ESZ); t.ldo = (int)q.ldo;
            t.P = q.P; t.Q = q.Q; t.R = q.R;
            if constexpr (F8) { t.sa = q.scale_a; t.sb = q.scale_b; }
            t.tiles_q = (q.Q + 127) / 128;
            t.tile_begin = tiles;
            tiles += ((q.P + 255) / 256) * t.tiles_q;
        }
        if (tiles != pl.tiles) return DG_ERR_ARG;          // (the plan counts tiles with the same formula)
        gp.total_tiles = pl.tiles;
        gp.tiles_pad = pl.tiles_pad;
        gp.splits = pl.splits;
        const bool cut = pl.splits != 1;
        gp.ws = cut ? (char*)workspace : nullptr;
        gp.flags = cut ? (unsigned*)((char*)workspace + pl.flag_offset) : nullptr;
        gp.err = workspace ? (unsigned*)((char*)workspace + dg_gemm_tn_grouped_workspace_bytes(problems, n) - 16) : nullptr;
        hipLaunchKernelGGL((gemm_tn_grouped256_kernel<0, F8>), dim3(pl.grid), dim3(768), 0, s, gp);
        DG_LAUNCH_CHECK();
    }
    return DG_OK;
}

extern "C" int dg_gemm_tn_grouped(const dg_tn_problem* problems, int n, int dtype, void* workspace, int64_t workspace_bytes,
                                  void* stream) {
    if (!problems || n <= 0) return DG_ERR_ARG;
    const bool f8 = dtype == DG_FP8_E5M2;         // named after the A operand (dY: e5m2); B (X) is e4m3
    if (dtype != DG_BF16 && !f8) return DG_ERR_DTYPE;
    const int g = f8 ? 16 : 8, kr = f8 ? 128 : 64;
    for (int i = 0; i < n; ++i) {
        const dg_tn_problem& q = problems[i];
        if (!q.A || !q.B || !q.out || q.R <= 0 || q.P <= 0 || q.Q <= 0 || q.R % kr) return DG_ERR_ARG;
        if (q.lda % g || q.ldb % g || !dg_aligned16(q.A) || !dg_aligned16(q.B)) return DG_ERR_ALIGN;
        if (q.lda < q.P || q.ldb < q.Q || q.ldo < q.Q) return DG_ERR_ARG;
        if (q.lda >= (1 << 30) || q.ldb >= (1 << 30) || q.ldo >= (1ll << 31)) return DG_ERR_ARG;
        if (((q.P + g - 1) / g) * g > q.lda || ((q.Q + g - 1) / g) * g > q.ldb) return DG_ERR_ARG;
        if (f8 && (!q.scale_a || !q.scale_b)) return DG_ERR_ARG;
    }
    if (workspace && (!dg_aligned16(workspace) || workspace_bytes < dg_gemm_tn_grouped_workspace_bytes(problems, n))) return DG_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (f8) return tn_grouped_launch<TnGroup8, TnProblem8, true, TN_MAX_GROUP8>(problems, n, workspace, workspace_bytes, s);
    return tn_grouped_launch<TnGroup, TnProblem, false, TN_MAX_GROUP>(problems, n, workspace, workspace_bytes, s);
}
