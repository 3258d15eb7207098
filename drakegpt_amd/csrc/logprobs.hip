// Token log-probabilities for generate(return_logprobs=) and score() -- dg_token_logprobs (include/drakegpt_hip.h has the contract).
// One workgroup per row of logits (fp32, or bf16 widened exactly).  A row (201 KB in fp32 at V = 50257) fits neither the registers
// of a sensible workgroup nor LDS, so the kernel re-reads the L2-resident row, as the sampler does (sample.hip):
//   1. strided, coalesced: m* = max x, and with x_t known up front (one broadcast load) the rank counts of the token in the SAME
//      pass -- the rank needs x_t, not the maximum
//   2. top_n > 0 only: radix select of the n-th largest x on order-preserving 32-bit keys, 4 passes of 8 bits, LDS histograms with
//      INTEGER atomics (the sampler's top-k pass)
//   3. blocked: thread t owns the chunk [t * chunk, (t + 1) * chunk); e_j = exp((double)(x_j - m*)) summed in index order in fp64,
//      the chunk sums scanned per wave (shfl_up, offsets 1, 2, .., 32) and the wave totals added in wave order: Z.  This is the
//      sampler's scheme for S, order for order.  With top_n > 0 the same walk counts the chunk's entries above and at the threshold;
//      an integer scan of those counts gives every survivor its slot (ties at the threshold: lowest index first), and the threads
//      that own one walk their chunk once more to file it.  At most 20 survivors are then ranked by one wave.
// So two passes at top_n = 0, and four short ones plus a refile with top-n.  No floating-point atomics: every output is a pure
// function of (logits, tokens, state, lengths, spans, top_n).
#include "common.h"

__device__ __forceinline__ uint32_t lp_key(float z) {           // a < b  <=>  key(a) < key(b)  (no NaNs)
    const uint32_t b = __float_as_uint(z);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float lp_unkey(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}
#define LP_KEY_NEG_INF 0x007FFFFFu                              // lp_key(-inf): below every other key

template <int NT, typename T>
__global__ __launch_bounds__(NT) void token_logprobs_kernel(const T* __restrict__ logits, int64_t ldl, int M, int V,
                                                            const int64_t* __restrict__ tokens, int64_t ld_tok,
                                                            const uint32_t* __restrict__ state, const int32_t* __restrict__ lengths,
                                                            const int32_t* __restrict__ spans, const int32_t* __restrict__ top_n_dev,
                                                            float* __restrict__ tok_lp, int32_t* __restrict__ tok_rank,
                                                            int32_t* __restrict__ top_ids, float* __restrict__ top_lp) {
    constexpr int NW = NT / 64;
    constexpr int TOP = DG_LOGPROBS_MAX_TOP;
    __shared__ float s_mx[NW];
    __shared__ int s_cnt[NW];
    __shared__ int s_hist[256];
    __shared__ uint32_t s_sel[2];          // {key prefix, k still to find below it}
    __shared__ double s_wtot[NW];
    __shared__ uint32_t s_scan[NW];
    __shared__ uint32_t s_lkey[TOP];
    __shared__ int s_lidx[TOP];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int row = blockIdx.x;

    // ---- which token, which output element; skipped rows leave here (uniform per workgroup, before any barrier)
    int64_t e = row;
    if (ld_tok > 0) {
        const int64_t L = (int64_t)state[2];
        if (L >= ld_tok) return;
        if (lengths) { const int32_t n = lengths[row]; if (n != 0 && L >= (int64_t)n) return; }
        if (spans && L < (int64_t)spans[2 * row]) return;
        e = (int64_t)row * ld_tok + L;
    }
    int64_t t64 = tokens[e];
    const int t = (int)(t64 < 0 ? 0 : (t64 >= V ? V - 1 : t64));
    const T* x = logits + (int64_t)row * ldl;
    const float xt = to_f32<T>(x[t]);
    int top_n = (top_ids && top_n_dev) ? *top_n_dev : 0;
    top_n = top_n < 0 ? 0 : (top_n > TOP ? TOP : top_n);
    const int k = top_n > V ? V : top_n;

    // ---- pass 1: the maximum, and the token's rank counts
    float mx = -INFINITY; int cnt = 0;
    for (int i = tid; i < V; i += NT) {
        const float v = to_f32<T>(x[i]);
        if (v > mx) mx = v;
        cnt += (v > xt || (v == xt && i < t)) ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        cnt += __shfl_xor(cnt, o, 64);
    }
    if (lane == 0) { s_mx[w] = mx; s_cnt[w] = cnt; }
    if (tid == 0) { s_sel[0] = 0u; s_sel[1] = (uint32_t)k; }
    __syncthreads();
    mx = s_mx[0]; cnt = s_cnt[0];
#pragma unroll
    for (int v = 1; v < NW; ++v) { mx = fmaxf(mx, s_mx[v]); cnt += s_cnt[v]; }

    // ---- pass 2 (top_n > 0): tau = the k-th largest x, k <= V
    uint32_t tau_key = 0u;
    if (k > 0) {
        for (int shift = 24; shift >= 0; shift -= 8) {
            for (int i = tid; i < 256; i += NT) s_hist[i] = 0;
            __syncthreads();
            const uint32_t prefix = s_sel[0];
            const uint32_t himask = shift == 24 ? 0u : (0xFFFFFFFFu << (shift + 8));
            for (int i = tid; i < V; i += NT) {
                const uint32_t key = lp_key(to_f32<T>(x[i]));
                if (((key ^ prefix) & himask) == 0u) atomicAdd(&s_hist[(key >> shift) & 255u], 1);
            }
            __syncthreads();
            if (w == 0) {
                // lane l owns bins 4l .. 4l + 3; `above` = keys in the bins of higher lanes
                const int c0 = s_hist[4 * lane], c1 = s_hist[4 * lane + 1], c2 = s_hist[4 * lane + 2], c3 = s_hist[4 * lane + 3];
                const int c = c0 + c1 + c2 + c3;
                int suf = c;                                   // inclusive suffix sum over lanes >= lane
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_down(suf, o, 64); if (lane + o < 64) suf += u; }
                int above = suf - c;
                const int kk = (int)s_sel[1];
                if (above < kk && kk <= suf) {                 // exactly one lane
                    int bin;
                    if (above + c3 >= kk) bin = 4 * lane + 3;
                    else if ((above += c3, above + c2 >= kk)) bin = 4 * lane + 2;
                    else if ((above += c2, above + c1 >= kk)) bin = 4 * lane + 1;
                    else { above += c1; bin = 4 * lane; }
                    s_sel[0] = prefix | ((uint32_t)bin << shift);
                    s_sel[1] = (uint32_t)(kk - above);
                }
            }
            __syncthreads();
        }
        tau_key = s_sel[0];
    }

    // ---- pass 3: chunk sums in index order, fp64, and their scan; with top-n the chunk's counts above / at tau ride along
    const int chunk = (V + NT - 1) / NT;
    const int j0 = min(tid * chunk, V), j1 = min(j0 + chunk, V);
    double csum = 0.0; uint32_t mine = 0u;                     // mine = (#above tau) << 24 | #at tau: < 20 and <= 2^20
    for (int j = j0; j < j1; ++j) {
        const float v = to_f32<T>(x[j]);
        csum += exp((double)__fsub_rn(v, mx));
        if (k > 0) {
            const uint32_t key = lp_key(v);
            if (key > LP_KEY_NEG_INF) mine += key > tau_key ? (1u << 24) : (key == tau_key ? 1u : 0u);
        }
    }
    double incl = csum; uint32_t sc = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double u = __shfl_up(incl, o, 64); const uint32_t us = __shfl_up(sc, o, 64);
        if (lane >= o) { incl += u; sc += us; }
    }
    if (lane == 63) { s_wtot[w] = incl; s_scan[w] = sc; }
    __syncthreads();
    double Z = 0.0; uint32_t before = 0u, total = 0u;
    for (int v = 0; v < NW; ++v) { if (v == w) before = total; Z += s_wtot[v]; total += s_scan[v]; }
    const double logZ = log(Z);
    auto lp_of = [&](float v) -> float { return (float)((double)__fsub_rn(v, mx) - logZ); };

    if (tid == 0) {
        if (tok_lp) tok_lp[e] = lp_of(xt);
        if (tok_rank) tok_rank[e] = cnt;
    }
    if (!top_ids) return;

    // ---- the survivors take their slots: those above tau in index order, then the ties at tau, lowest index first
    const int n_gt = (int)(total >> 24), n_eq = (int)(total & 0xFFFFFFu);
    const int n_top = k > 0 ? min(k, n_gt + n_eq) : 0;         // < k only when the row has fewer than k finite entries
    if (mine != 0u) {
        const uint32_t ex = before + sc - mine;                // exclusive prefix of this thread
        int g = (int)(ex >> 24), q = n_gt + (int)(ex & 0xFFFFFFu);
        for (int j = j0; j < j1; ++j) {
            const uint32_t key = lp_key(to_f32<T>(x[j]));
            if (key <= LP_KEY_NEG_INF) continue;
            if (key > tau_key) { if (g < TOP) { s_lkey[g] = key; s_lidx[g] = j; } ++g; }
            else if (key == tau_key) { if (q < n_top) { s_lkey[q] = key; s_lidx[q] = j; } ++q; }
        }
    }
    __syncthreads();
    if (w != 0 || lane >= TOP) return;
    // one wave ranks them: descending x, ties by lowest index; the slots beyond n_top get the sentinels
    int32_t* oid = top_ids + e * TOP; float* olp = top_lp + e * TOP;
    if (lane >= n_top) { oid[lane] = -1; olp[lane] = -INFINITY; return; }
    const uint32_t key = s_lkey[lane]; const int idx = s_lidx[lane];
    int pos = 0;
    for (int j = 0; j < n_top; ++j) {
        const uint32_t kj = s_lkey[j]; const int ij = s_lidx[j];
        pos += (kj > key || (kj == key && ij < idx)) ? 1 : 0;
    }
    oid[pos] = idx; olp[pos] = lp_of(lp_unkey(key));
}

extern "C" int dg_token_logprobs(const void* logits, int logits_dtype, int64_t ldl, int M, int V, const int64_t* tokens,
                                 int64_t ld_tok, const uint32_t* state, const int32_t* lengths, const int32_t* spans,
                                 const int32_t* top_n, float* tok_lp, int32_t* tok_rank, int32_t* top_ids, float* top_lp,
                                 void* stream) {
    if (!logits || !tokens || M <= 0 || V <= 0 || V > (1 << 20) || ldl < V || ld_tok < 0) return DG_ERR_ARG;
    if (!dg_is_float_dtype(logits_dtype)) return DG_ERR_ARG;
    if (ld_tok > 0 && !state) return DG_ERR_ARG;
    if (ld_tok == 0 && (lengths || spans)) return DG_ERR_ARG;
    if ((top_ids == nullptr) != (top_lp == nullptr)) return DG_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    dg_with_dtype(logits_dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        // the sampler's split: a chunk of at most 32 (small rows) or V / 1024 elements per thread
        if (V <= 8192)
            hipLaunchKernelGGL((token_logprobs_kernel<256, T>), dim3(M), dim3(256), 0, s, (const T*)logits, ldl, M, V, tokens, ld_tok,
                               state, lengths, spans, top_n, tok_lp, tok_rank, top_ids, top_lp);
        else
            hipLaunchKernelGGL((token_logprobs_kernel<1024, T>), dim3(M), dim3(1024), 0, s, (const T*)logits, ldl, M, V, tokens, ld_tok,
                               state, lengths, spans, top_n, tok_lp, tok_rank, top_ids, top_lp);
    });
    DG_LAUNCH_CHECK();
    return DG_OK;
}
