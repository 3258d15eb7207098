// Token sampling on the device for generate() -- ref: src/model.py:625-635 (F.softmax at :631, torch.multinomial at :633).
// One workgroup per row of fp32 logits; the row (201 KB at V = 50257) does not fit LDS, so the kernel makes a few passes over
// the L2-resident row:
//   1. max z and its lowest index (z = logit * inv_temp; coalesced)            -> greedy ends here
//   2. top-k only: radix select of the k-th largest z on order-preserving 32-bit keys, 4 passes of 8 bits, LDS histograms
//      with INTEGER atomics (counts do not depend on arrival order)
//   3. blocked scan: thread t owns the contiguous chunk [t * chunk, (t + 1) * chunk); its e_j = exp(z_j - max) (fp64 exp of the
//      fp32 difference) are summed in index order in fp64, the chunk sums are scanned (wave shuffles, then the wave totals in
//      wave order), S = the last prefix
//   4. the thread whose prefix interval holds u * S walks its chunk again and writes the token; all threads write probs
// z and z - max are single fp32 roundings (__fmul_rn / __fsub_rn: never contracted into an fma), so a host restatement can match.
//   2b. dg_sample_rows_nucleus only (four-word params): min-p keeps e_j >= min_p; top-p finds tau_p by a second radix descent whose
//      LDS histograms hold INTEGER masses w_j = rint(e_j * 2^40) (64-bit integer atomics: sums do not depend on arrival order).
//      Neither costs a pass when it is off: min-p alone is one more compare in passes 3 and 4.
//   0. dg_sample_rows_control only: every pass reads y_i in the place of the logit -- the repetition / presence / frequency
//      penalties on the row's token counts and the logit bias, four single fp32 roundings, recomputed by each pass from
//      (logit, count, bias) (no scratch row: the three operands are L2-resident like the row itself).  The thread that writes the
//      token also does counts[row, token] += 1 and, at a stop token, lengths[row] = L + 1; a row that arrives finished writes pad_id
//      and returns before it reads a logit.
//      dg_sample_rows_ragged only (prompts of different lengths walked by one shared L): a row whose span {first, end} has
//      L < first is forced -- its prompt token is already at ids[row, L] -- and returns next, having read and written nothing; a
//      row that writes the last token of its budget (L + 1 >= end) marks itself finished like a row at a stop token.
// No floating-point atomics anywhere: tokens and probs are a pure function of (logits, state, params, row).
// exp and the prefix sums are fp64: with a few terms kept by top-k the errors of an fp32 expf do not average out of S (measured:
// probs off by 4.5 x 2^-24 at k = 40), and fp64 is cheap here -- a few passes over one row.  The CDF is then exact to ~1e-14.
#include "common.h"

#define DG_SITE_SAMPLE 0x53414D50u      // "SAMP": not of the form 4 * layer + k for any layer a model can have

struct SampleParams { float inv_temp; int32_t top_k; };
struct SampleParamsEx { float inv_temp; int32_t top_k; float top_p; float min_p; };      // dg_sample_rows_nucleus: the same first two words
// dg_sample_rows_control: the 16-word control block (device) and the launch arguments that come with it
struct SampleControl {
    float inv_rep, rep, presence, frequency;
    int32_t use_bias, n_stop, pad_id, reserved;
    int32_t stop[DG_SAMPLE_MAX_STOP];
};
struct SampleCtlArgs { const SampleControl* control; const float* bias; int32_t* counts; int64_t ldc; int32_t* lengths; };
struct SampleRagArgs : SampleCtlArgs { const int32_t* spans; };      // dg_sample_rows_ragged: + {first, end} per row
struct SampleNoCtl {};
template <bool CTL, bool RAG> using SampleCtlOf = std::conditional_t<RAG, SampleRagArgs, std::conditional_t<CTL, SampleCtlArgs, SampleNoCtl>>;

__device__ __forceinline__ uint32_t f32_key(float z) {          // a < b  <=>  key(a) < key(b)  (no NaNs)
    const uint32_t b = __float_as_uint(z);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_f32(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// The adjustment of dg_sample_rows_control: four fp32 roundings, one instruction each.  Contraction is off for the whole function --
// left on, x * inv_rep - presence becomes one fma with a single rounding, which no host restatement reproduces.
__device__ __forceinline__ float adjust_logit(float x, int32_t c, float inv_rep, float rep, float presence, float frequency,
                                              const float* __restrict__ bias, int i) {
#pragma clang fp contract(off)
    float y = x;
    if (c > 0) y = y > 0.f ? y * inv_rep : y * rep;
    y = y - (c > 0 ? presence : 0.f);
    const float f = frequency * (float)c;
    y = y - f;
    if (bias) y = y + bias[i];
    return y;
}

// EXT: params is a SampleParamsEx and the top-p / min-p stage exists; !EXT is dg_sample_rows as it always was
// CTL: dg_sample_rows_control -- `ctl` holds the control block, bias, counts and lengths; !CTL: an empty struct, no code
// RAG: dg_sample_rows_ragged -- CTL with the rows' spans in `ctl` (the launch has checked ids, ld_ids > 0 and lengths); !RAG: no code
template <int NT, bool EXT, bool CTL = false, bool RAG = false>
__global__ __launch_bounds__(NT) void sample_rows_kernel(const float* __restrict__ logits, int64_t ldl, int M, int V,
                                                         const uint32_t* __restrict__ state, const SampleParams* __restrict__ params,
                                                         int64_t* __restrict__ ids, int64_t ld_ids, float* __restrict__ probs,
                                                         int64_t ldp, SampleCtlOf<CTL, RAG> ctl) {
    static_assert(CTL || !RAG, "the ragged entry is a control entry");
    constexpr int NW = NT / 64;
    __shared__ float s_mx[NW];
    __shared__ int s_ix[NW];
    __shared__ int s_hist[256];
    __shared__ uint32_t s_sel[2];          // {key prefix, k still to find below it}
    __shared__ double s_wtot[NW];
    __shared__ int s_owner, s_last;
    __shared__ unsigned long long s_mass[EXT ? 256 : 1];
    __shared__ uint32_t s_psel[2];         // {key prefix of tau_p, a bin was found}
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int row = blockIdx.x;
    const float* x = logits + (int64_t)row * ldl;
    float* prow = probs ? probs + (int64_t)row * ldp : nullptr;
    const float inv_temp = params->inv_temp;
    int top_k = params->top_k;
    const bool greedy = !(inv_temp > 0.f);
    const float sc = greedy ? 1.f : inv_temp;

    // ---- pass 0 (CTL): finished rows leave here; everything below reads zat(i) = y_i * sc in the place of logit_i * sc
    float inv_rep = 1.f, rpen = 1.f, presence = 0.f, frequency = 0.f;
    const float* bias = nullptr; int32_t* crow = nullptr;
    if constexpr (CTL) {
        if (ctl.lengths && ids && ld_ids > 0 && ctl.lengths[row] != 0) {          // uniform per workgroup, before any barrier
            const uint32_t Lf = state[2];
            if (tid == 0 && (int64_t)Lf < ld_ids) ids[(int64_t)row * ld_ids + Lf] = (int64_t)ctl.control->pad_id;
            return;
        }
        if constexpr (RAG) {          // forced: uniform per workgroup, before any barrier; nothing is read but the span, nothing written
            if ((int64_t)state[2] < (int64_t)ctl.spans[2 * row]) return;
        }
        inv_rep = ctl.control->inv_rep; rpen = ctl.control->rep;
        presence = ctl.control->presence; frequency = ctl.control->frequency;
        if (ctl.control->use_bias != 0) bias = ctl.bias;
        if (ctl.counts) crow = ctl.counts + (int64_t)row * ctl.ldc;
    }
    auto zat = [&](int i) -> float {
        float y = x[i];
        if constexpr (CTL) y = adjust_logit(y, crow ? crow[i] : 0, inv_rep, rpen, presence, frequency, bias, i);
        return __fmul_rn(y, sc);
    };

    // ---- pass 1: max and the lowest index that attains it
    float mx = -INFINITY; int ix = V;
    for (int i = tid; i < V; i += NT) {
        const float z = zat(i);
        if (ix == V || z > mx) { mx = z; ix = i; }              // strict: a thread keeps the lowest of its equal maxima
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(mx, o, 64); const int oi = __shfl_xor(ix, o, 64);
        if (om > mx || (om == mx && oi < ix)) { mx = om; ix = oi; }
    }
    if (lane == 0) { s_mx[w] = mx; s_ix[w] = ix; }
    if (tid == 0) { s_owner = NT; s_last = -1; }
    __syncthreads();
    mx = s_mx[0]; ix = s_ix[0];
#pragma unroll
    for (int v = 1; v < NW; ++v) {
        const float om = s_mx[v]; const int oi = s_ix[v];
        if (om > mx || (om == mx && oi < ix)) { mx = om; ix = oi; }
    }
    if (ix >= V) ix = V - 1;
    const uint32_t L = state ? state[2] : 0u;
    const bool write_tok = ids != nullptr && (ld_ids == 0 || (int64_t)L < ld_ids);
    int64_t* tok_out = ids ? (ld_ids == 0 ? ids + row : ids + (int64_t)row * ld_ids + L) : nullptr;
    // the one thread that has the token writes it and (CTL) keeps the row's books: every read of counts is behind it by then
    auto emit = [&](int tok) {
        *tok_out = tok;
        if constexpr (CTL) {
            if (crow) crow[tok] = crow[tok] + 1;
            bool stopped = false;
            if (ctl.lengths && ld_ids > 0) {
                const int ns = min(ctl.control->n_stop, DG_SAMPLE_MAX_STOP);
                for (int q = 0; q < ns; ++q)
                    if (ctl.control->stop[q] == tok) { ctl.lengths[row] = (int32_t)(L + 1u); stopped = true; break; }
            }
            if constexpr (RAG) {      // the last token of the row's budget: finished from the next position on
                if (!stopped && (int64_t)L + 1 >= (int64_t)ctl.spans[2 * row + 1]) ctl.lengths[row] = (int32_t)(L + 1u);
            }
        }
    };

    if (greedy) {
        if (tid == 0 && write_tok) emit(ix);
        if (prow) for (int i = tid; i < V; i += NT) prow[i] = i == ix ? 1.f : 0.f;
        return;
    }

    // ---- pass 2: tau = the k-th largest z (ties at tau are all kept; -inf never is)
    float tau = -INFINITY;
    if (top_k > V) top_k = V;
    if (top_k > 0 && top_k < V) {
        if (tid == 0) { s_sel[0] = 0u; s_sel[1] = (uint32_t)top_k; }
        for (int shift = 24; shift >= 0; shift -= 8) {
            for (int i = tid; i < 256; i += NT) s_hist[i] = 0;
            __syncthreads();
            const uint32_t prefix = s_sel[0];
            const uint32_t himask = shift == 24 ? 0u : (0xFFFFFFFFu << (shift + 8));
            for (int i = tid; i < V; i += NT) {
                const uint32_t key = f32_key(zat(i));
                if (((key ^ prefix) & himask) == 0u) atomicAdd(&s_hist[(key >> shift) & 255u], 1);
            }
            __syncthreads();
            if (w == 0) {
                // lane l owns bins 4l .. 4l + 3; `above` = keys in the bins of higher lanes
                const int c0 = s_hist[4 * lane], c1 = s_hist[4 * lane + 1], c2 = s_hist[4 * lane + 2], c3 = s_hist[4 * lane + 3];
                const int c = c0 + c1 + c2 + c3;
                int suf = c;                                   // inclusive suffix sum over lanes >= lane
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_down(suf, o, 64); if (lane + o < 64) suf += t; }
                int above = suf - c;
                const int k = (int)s_sel[1];
                if (above < k && k <= suf) {                   // exactly one lane
                    int bin = 4 * lane + 3;
                    if (above + c3 >= k) bin = 4 * lane + 3;
                    else if ((above += c3, above + c2 >= k)) bin = 4 * lane + 2;
                    else if ((above += c2, above + c1 >= k)) bin = 4 * lane + 1;
                    else { above += c1; bin = 4 * lane; }
                    s_sel[0] = prefix | ((uint32_t)bin << shift);
                    s_sel[1] = (uint32_t)(k - above);
                }
            }
            __syncthreads();
        }
        tau = key_f32(s_sel[0]);
    }

    // kept before top-p (K1 of the header): z >= tau, never -inf, and with min-p e >= min_p; e is computed on the way
    double minp = 0.0; bool use_minp = false;
    auto kept = [&](float z, double& e) -> bool {
        if (!(z >= tau && z > -INFINITY)) return false;
        e = exp((double)__fsub_rn(z, mx));
        if constexpr (EXT) { if (use_minp && !(e >= minp)) return false; }
        return true;
    };

    // ---- pass 2b: tau_p = the lowest z whose mass above it, G(z) = sum { w_i : z_i > z }, is < T = top_p * S1 (as doubles)
    if constexpr (EXT) {
        const SampleParamsEx* px = (const SampleParamsEx*)params;
        const float top_p = px->top_p, min_p = px->min_p;
        use_minp = min_p > 0.f;
        minp = (double)fminf(min_p, 1.f);                       // the maximum (e = 1) always stays
        if (top_p > 0.f && top_p < 1.f) {
            // The same 4 x 8-bit descent as top-k, over histograms of mass.  A bin holds a kept key iff its mass is > 0 and the
            // mass above the bin is < T: its highest key with mass has exactly that G.  Keys with w = 0 need no count of their own:
            // every key below them has w = 0 too, so their G is S1, and (double)S1 > T for any fp32 top_p < 1.
            // Level 0 sees every element of K1, so its histogram total is S1: no pass of its own.
            if (tid == 0) { s_psel[0] = 0u; s_psel[1] = 0u; }
            double T = 0.0; unsigned long long carried = 0ull;      // live in wave 0 only
            for (int shift = 24; shift >= 0; shift -= 8) {
                for (int i = tid; i < 256; i += NT) s_mass[i] = 0ull;
                __syncthreads();
                const uint32_t prefix = s_psel[0];
                const uint32_t himask = shift == 24 ? 0u : (0xFFFFFFFFu << (shift + 8));
                for (int i = tid; i < V; i += NT) {
                    const float z = zat(i);
                    const uint32_t key = f32_key(z);
                    double e;
                    if (((key ^ prefix) & himask) == 0u && kept(z, e)) {
                        const unsigned long long wj = (unsigned long long)rint(e * 0x1p40);
                        if (wj) atomicAdd(&s_mass[(key >> shift) & 255u], wj);
                    }
                }
                __syncthreads();
                if (w == 0) {
                    // lane l owns bins 4l .. 4l + 3; a3 .. a0 = the mass above each of them
                    const unsigned long long m0 = s_mass[4 * lane], m1 = s_mass[4 * lane + 1], m2 = s_mass[4 * lane + 2],
                                             m3 = s_mass[4 * lane + 3];
                    const unsigned long long m = m0 + m1 + m2 + m3;
                    unsigned long long suf = m;                // inclusive suffix sum over lanes >= lane
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) { const unsigned long long t = __shfl_down(suf, o, 64); if (lane + o < 64) suf += t; }
                    if (shift == 24) T = (double)top_p * (double)__shfl(suf, 0, 64);
                    const unsigned long long a3 = carried + (suf - m), a2 = a3 + m3, a1 = a2 + m2, a0 = a1 + m1;
                    int bin = -1; unsigned long long A = 0ull;  // this lane's lowest bin that holds a kept key
                    if (m0 && (double)a0 < T) { bin = 4 * lane; A = a0; }
                    else if (m1 && (double)a1 < T) { bin = 4 * lane + 1; A = a1; }
                    else if (m2 && (double)a2 < T) { bin = 4 * lane + 2; A = a2; }
                    else if (m3 && (double)a3 < T) { bin = 4 * lane + 3; A = a3; }
                    const unsigned long long have = __ballot(bin >= 0);
                    if (have) {                                 // none: no finite logit in the row -- no filter, as without top-p
                        const int src = __ffsll(have) - 1;
                        carried = __shfl(A, src, 64);
                        if (lane == src) { s_psel[0] = prefix | ((uint32_t)bin << shift); s_psel[1] = 1u; }
                    }
                }
                __syncthreads();
            }
            if (s_psel[1]) tau = fmaxf(tau, key_f32(s_psel[0]));
        }
    }

    // ---- pass 3: chunk sums in index order, fp64, and their scan
    const int chunk = (V + NT - 1) / NT;
    const int j0 = min(tid * chunk, V), j1 = min(j0 + chunk, V);
    double csum = 0.0; int last = -1;
    for (int j = j0; j < j1; ++j) {
        const float z = zat(j);
        double e;
        if (kept(z, e)) { csum += e; last = j; }
    }
    double incl = csum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const double t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
    if (lane == 63) s_wtot[w] = incl;
    if (last >= 0) atomicMax(&s_last, last);
    __syncthreads();
    double woff = 0.0, S = 0.0;
    for (int v = 0; v < NW; ++v) { if (v == w) woff = S; S += s_wtot[v]; }
    incl += woff;
    double excl = __shfl_up(incl, 1, 64);
    if (lane == 0) excl = woff;                                // == the last inclusive prefix of wave w - 1, bit for bit

    if (prow) {
        for (int i = tid; i < V; i += NT) {
            const float z = zat(i);
            double e;
            prow[i] = kept(z, e) ? (float)(e / S) : 0.f;
        }
    }
    if (!write_tok) return;

    // ---- pass 4: the smallest n with sum_{j <= n} e_j > u * S
    const uint32_t h = dg_hash_w(dg_site_key(state[0], state[1], L, DG_SITE_SAMPLE), (uint32_t)row * DG_WEYL);
    const double target = (double)((float)(h >> 8) * 0x1p-24f) * S;
    if (incl > target && !(excl > target)) atomicMin(&s_owner, tid);     // excl(t) == incl(t - 1): at most one thread
    __syncthreads();
    const int owner = s_owner;
    if (owner == NT) {                                         // rounding (or an empty / non-finite row) left no such n
        if (tid == 0) { const int l = s_last; emit(l >= 0 ? l : ix); }
        return;
    }
    if (tid != owner) return;
    double run = excl; int tok = last;                         // last: if re-adding from excl rounds below target
    for (int j = j0; j < j1; ++j) {
        const float z = zat(j);
        double e;
        if (kept(z, e)) {
            run += e;
            if (run > target) { tok = j; break; }
        }
    }
    emit(tok);
}

template <bool EXT, bool CTL = false, bool RAG = false>
static int sample_rows_launch(const float* logits, int64_t ldl, int M, int V, const uint32_t* state, const void* params,
                              int64_t* ids, int64_t ld_ids, float* probs, int64_t ldp, void* stream,
                              SampleCtlOf<CTL, RAG> ctl = {}) {
    if (!logits || !params || M <= 0 || V <= 0 || V > (1 << 20) || ldl < V || ld_ids < 0) return DG_ERR_ARG;
    if (!ids && !probs) return DG_ERR_ARG;
    if (ids && !state) return DG_ERR_ARG;
    if (probs && ldp < V) return DG_ERR_ARG;
    if constexpr (CTL) {
        if (!ctl.control) return DG_ERR_ARG;
        if (ctl.counts && ctl.ldc < V) return DG_ERR_ARG;
        if (ctl.lengths && (!ids || ld_ids == 0)) return DG_ERR_ARG;
    }
    if constexpr (RAG) {
        if (!ctl.spans || !ctl.lengths || !ids || ld_ids == 0) return DG_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    const SampleParams* p = (const SampleParams*)params;
    // a chunk of at most 32 (small rows) or V / 1024 (52 at V = 53248) elements per thread
    if (V <= 8192)
        hipLaunchKernelGGL((sample_rows_kernel<256, EXT, CTL, RAG>), dim3(M), dim3(256), 0, s, logits, ldl, M, V, state, p, ids, ld_ids, probs, ldp, ctl);
    else
        hipLaunchKernelGGL((sample_rows_kernel<1024, EXT, CTL, RAG>), dim3(M), dim3(1024), 0, s, logits, ldl, M, V, state, p, ids, ld_ids, probs, ldp, ctl);
    DG_LAUNCH_CHECK();
    return DG_OK;
}

extern "C" int dg_sample_rows(const float* logits, int64_t ldl, int M, int V, const uint32_t* state, const void* params,
                              int64_t* ids, int64_t ld_ids, float* probs, int64_t ldp, void* stream) {
    return sample_rows_launch<false>(logits, ldl, M, V, state, params, ids, ld_ids, probs, ldp, stream);
}

extern "C" int dg_sample_rows_nucleus(const float* logits, int64_t ldl, int M, int V, const uint32_t* state, const void* params,
                                      int64_t* ids, int64_t ld_ids, float* probs, int64_t ldp, void* stream) {
    return sample_rows_launch<true>(logits, ldl, M, V, state, params, ids, ld_ids, probs, ldp, stream);
}

extern "C" int dg_sample_rows_control(const float* logits, int64_t ldl, int M, int V, const uint32_t* state, const void* params,
                                      int64_t* ids, int64_t ld_ids, float* probs, int64_t ldp, const void* control,
                                      const float* bias, int32_t* counts, int64_t ldc, int32_t* lengths, void* stream) {
    return sample_rows_launch<true, true>(logits, ldl, M, V, state, params, ids, ld_ids, probs, ldp, stream,
                                          SampleCtlArgs{(const SampleControl*)control, bias, counts, ldc, lengths});
}

extern "C" int dg_sample_rows_ragged(const float* logits, int64_t ldl, int M, int V, const uint32_t* state, const void* params,
                                     int64_t* ids, int64_t ld_ids, float* probs, int64_t ldp, const void* control,
                                     const float* bias, int32_t* counts, int64_t ldc, int32_t* lengths, const int32_t* spans,
                                     void* stream) {
    return sample_rows_launch<true, true, true>(logits, ldl, M, V, state, params, ids, ld_ids, probs, ldp, stream,
                                                SampleRagArgs{{(const SampleControl*)control, bias, counts, ldc, lengths}, spans});
}

// counts[m, clamp(ids[m, j])] += 1 for j < n: one workgroup per row; !accumulate zeroes the row's V counts first, and the barrier
// of that same workgroup orders the zeroes before its own atomics -- no grid-wide ordering is needed
__device__ __forceinline__ void token_counts_row(const int64_t* __restrict__ ids, int64_t ld_ids, int n, int V,
                                                 int32_t* __restrict__ counts, int64_t ldc, int accumulate, int row) {
    int32_t* crow = counts + (int64_t)row * ldc;
    if (!accumulate) {
        for (int i = threadIdx.x; i < V; i += 256) crow[i] = 0;
        __syncthreads();
    }
    const int64_t* irow = ids + (int64_t)row * ld_ids;
    for (int j = threadIdx.x; j < n; j += 256) {
        int64_t v = irow[j];
        v = v < 0 ? 0 : (v >= V ? V - 1 : v);
        atomicAdd(&crow[v], 1);
    }
}

__global__ __launch_bounds__(256) void token_counts_kernel(const int64_t* __restrict__ ids, int64_t ld_ids, int n, int V,
                                                           int32_t* __restrict__ counts, int64_t ldc, int accumulate) {
    token_counts_row(ids, ld_ids, n, V, counts, ldc, accumulate, blockIdx.x);
}

// dg_token_counts_rows: row m counts its own prefix, n = clamp(n_rows[m * n_stride], 0, ld_ids)
__global__ __launch_bounds__(256) void token_counts_rows_kernel(const int64_t* __restrict__ ids, int64_t ld_ids,
                                                                const int32_t* __restrict__ n_rows, int64_t n_stride, int V,
                                                                int32_t* __restrict__ counts, int64_t ldc, int accumulate) {
    const int row = blockIdx.x;
    const int64_t n = n_rows[(int64_t)row * n_stride];
    token_counts_row(ids, ld_ids, (int)(n < 0 ? 0 : (n > ld_ids ? ld_ids : n)), V, counts, ldc, accumulate, row);
}

extern "C" int dg_token_counts(const int64_t* ids, int64_t ld_ids, int M, int n, int V, int32_t* counts, int64_t ldc,
                               int accumulate, void* stream) {
    if (!ids || !counts || M <= 0 || n < 0 || V <= 0 || ld_ids < n || ldc < V) return DG_ERR_ARG;
    hipLaunchKernelGGL(token_counts_kernel, dim3(M), dim3(256), 0, (hipStream_t)stream, ids, ld_ids, n, V, counts, ldc, accumulate);
    DG_LAUNCH_CHECK();
    return DG_OK;
}

extern "C" int dg_token_counts_rows(const int64_t* ids, int64_t ld_ids, int M, const int32_t* n_rows, int64_t n_stride, int V,
                                    int32_t* counts, int64_t ldc, int accumulate, void* stream) {
    if (!ids || !counts || !n_rows || M <= 0 || V <= 0 || ld_ids < 0 || ld_ids > INT32_MAX || n_stride < 0 || ldc < V) return DG_ERR_ARG;
    hipLaunchKernelGGL(token_counts_rows_kernel, dim3(M), dim3(256), 0, (hipStream_t)stream, ids, ld_ids, n_rows, n_stride, V, counts,
                       ldc, accumulate);
    DG_LAUNCH_CHECK();
    return DG_OK;
}
