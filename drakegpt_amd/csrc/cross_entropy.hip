// Fused row-wise cross entropy forward + backward (ref: F.cross_entropy at src/model.py:604-607).
// HBM-bound.  Small vocabularies (the reference's 80 characters): one wave64 per row, the row re-read from L2 for the
// max, sum and gradient passes.  Large vocabularies (GPT-2's 50257: 201 KB per row, 1.65 GB of logits at M = 8192): one
// 1024-thread workgroup per row that keeps the whole row in registers, so the logits are read from HBM exactly once.
// Algorithmic bytes per row: V*4 read (+ V*sizeof(dlogits) written when training).
#include "common.h"
#include <float.h>
#include <type_traits>

// Loss options, a compile-time switch of every kernel below: the kernels end in a parameter pack `O... o` that is either empty (the
// plain mean NLL: the code and the kernel arguments it always had) or one CeOpt (OPT below):
// label smoothing eps in [0, 1) and the z-loss coefficient zeta >= 0.  Per row, with lse = mx + log s and p = softmax(x):
//   objective  l   = lse - (1 - eps) x_t - (eps / V) sum_{i < V} x_i + zeta lse^2
//   gradient   g_i = grad_scale (p_i (1 + 2 zeta lse) - (1 - eps) [i == t] - eps / V)
// The cross-entropy part is evaluated as log s + (1 - eps)(mx - x_t) + (eps / V) sum_{i < V} (mx - x_i): every term is non-negative
// and nothing rounds at the size of mx (see the comment in cross_entropy_row_bf16_kernel).  The sum runs over the V logits only:
// neither the -inf that fills padding lanes nor the memory of columns V .. ldl - 1 enters it.  With zeta > 0 a gradient row sums to
// 2 zeta lse grad_scale, not to zero.
struct CeOpt { float eps, zeta; };
// ignore_index, a second member the pack may end in (IGN below; alone or behind a CeOpt): a row whose target equals ignore_index is
// left out -- its loss_rows entry and its dlogits row (padding columns included, and in place over its own logits) are STORED as
// exact zeros, and its target is recognised before any logit is read, a wave- / workgroup-uniform exit in the wave-per-row and
// workgroup-per-row kernels.  The other rows' gradients are scaled by inv_count[0] = 1 / N, N the number of rows that count, which
// only the device knows (dg_ce_count_valid writes it); the mean of loss_rows takes the same factor (dg_reduce_sum_scaled, or the
// fused kernel's last workgroup).  N = 0: inv_count is +inf, nothing is multiplied by it, every gradient row is zeros.
struct CeIgn { int64_t ignore_index; const float* inv_count; };
// The pack resolved (dg_pack_has / dg_pack_get of common.h): every kernel opens with `const CePack<O...> p(o...)` and hands p.OPT, p.IGN,
// p.opt and p.ign to the row math below, which takes and returns values.  An absent CeOpt reads as both options zero.
template <typename... O> struct CePack {
    static constexpr bool OPT = dg_pack_has<CeOpt, O...>::value, IGN = dg_pack_has<CeIgn, O...>::value;
    CeOpt opt;
    CeIgn ign;
    __device__ __forceinline__ explicit CePack(O... o) : opt(dg_pack_get(CeOpt{0.f, 0.f}, o...)), ign(dg_pack_get(CeIgn{0, nullptr}, o...)) {}
};
// The row loss from mx, logs = log s, xt = x_t and sd = sum_{i < V} (mx - x_i) (read under OPT only).  The plain instantiations keep
// mx + log s - x_t, the code they always had.  The ignore forms without a CeOpt write log s + (mx - x_t), the order the options use
// (nothing rounds at the size of mx: logits shifted by +1000 keep 1e-6).  The bf16 whole-row kernel has an order of its own.
__device__ __forceinline__ float ce_objective(float mx, float logs, float xt, float sd, int V, CeOpt opt) {
    const float lse = mx + logs;
    return logs + (1.f - opt.eps) * (mx - xt) + opt.eps / (float)V * sd + opt.zeta * lse * lse;
}
template <bool OPT, bool IGN>
__device__ __forceinline__ float ce_row_loss(float mx, float logs, float xt, float sd, int V, CeOpt opt) {
    return OPT ? ce_objective(mx, logs, xt, sd, V, opt) : IGN ? logs + (mx - xt) : mx + logs - xt;
}
// The gradient element is (e_i inv - (1 - eps) [i == t] - unif) scale with e_i = exp(x_i - mx), inv = ce_inv(), unif = ce_unif():
// p_i enters the gradient times 1 + 2 zeta lse; the target's one-hot weighs 1 - eps; every column gives up eps / V
__device__ __forceinline__ float ce_pscale(float mx, float logs, CeOpt opt) { return 1.f + 2.f * opt.zeta * (mx + logs); }
template <bool OPT> __device__ __forceinline__ float ce_inv(float mx, float logs, float s, CeOpt opt) {
    return OPT ? ce_pscale(mx, logs, opt) / s : 1.f / s;
}
template <bool OPT> __device__ __forceinline__ float ce_unif(int V, CeOpt opt) { return OPT ? opt.eps / (float)V : 0.f; }
template <bool OPT> __device__ __forceinline__ float ce_grad(float p, bool hot, float unif, CeOpt opt, float grad_scale) {
    return OPT ? (p - (hot ? 1.f - opt.eps : 0.f) - unif) * grad_scale : (p - (hot ? 1.f : 0.f)) * grad_scale;
}
__device__ __forceinline__ int64_t ce_clamp_target(int64_t t, int V) { return t < 0 ? 0 : (t >= V ? V - 1 : t); }
// An ignored row: loss 0 and, where there is a gradient, exact zeros over all ldd columns of its row; the thread stores columns
// first, first + stride, ...  The 16-byte form for bf16x8 rows follows.  (The two rows-in-registers kernels store their <= 8 columns
// per lane unrolled, the fused one inside its row loop.)
template <typename TD>
__device__ __forceinline__ void ce_zero_row(float* loss_rows, TD* dlogits, int64_t ldd, int row, int first, int stride) {
    if (first == 0) loss_rows[row] = 0.f;
    if (dlogits)
        for (int i = first; i < (int)ldd; i += stride) dlogits[(int64_t)row * ldd + i] = from_f32<TD>(0.f);
}
__device__ __forceinline__ void ce_zero_row_x8(float* loss_rows, bf16_t* dlogits, int64_t ldd, int row, int first, int stride) {
    if (first == 0) loss_rows[row] = 0.f;
    if (!dlogits) return;
    bf16x8 z;
#pragma unroll
    for (int e = 0; e < 8; ++e) z[e] = (bf16_t)0.f;
    for (int c = first; c < (int)(ldd / 8); c += stride) *(bf16x8*)(dlogits + (int64_t)row * ldd + c * 8) = z;
}

template <typename TD, typename TL = float, typename... O>
__global__ void cross_entropy_kernel(const TL* __restrict__ logits, int64_t ldl, const int64_t* __restrict__ targets,
                                     float* __restrict__ loss_rows, TD* __restrict__ dlogits, int64_t ldd,
                                     float grad_scale, const float* __restrict__ gs_dev, int M, int V, O... o) {
    const CePack<O...> p(o...);
    constexpr bool OPT = p.OPT, IGN = p.IGN;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= M) return;
    if (IGN && targets[row] == p.ign.ignore_index)           // (wave-uniform: no logit of the row is read)
        return ce_zero_row(loss_rows, dlogits, ldd, row, lane, 64);
    const TL* x = logits + (int64_t)row * ldl;
    float mx = -INFINITY;
    for (int i = lane; i < V; i += 64) mx = fmaxf(mx, (float)x[i]);
    mx = wave_max(mx);
    float s = 0.f, sd = 0.f;
    for (int i = lane; i < V; i += 64) {
        s += expf((float)x[i] - mx);
        if (OPT) sd += mx - (float)x[i];
    }
    s = wave_sum(s);
    if (OPT) sd = wave_sum(sd);
    const int64_t t = ce_clamp_target(targets[row], V);
    if (lane == 0) loss_rows[row] = ce_row_loss<OPT, IGN>(mx, logf(s), (float)x[t], sd, V, p.opt);
    if (dlogits) {
        TD* d = dlogits + (int64_t)row * ldd;
        const float inv = ce_inv<OPT>(mx, logf(s), s, p.opt), unif = ce_unif<OPT>(V, p.opt);
        if (gs_dev) grad_scale *= gs_dev[0];
        if (IGN) grad_scale *= p.ign.inv_count[0];
        for (int i = lane; i < (int)ldd; i += 64) {
            float g = 0.f;
            if (i < V) g = ce_grad<OPT>(expf((float)x[i] - mx) * inv, i == (int)t, unif, p.opt, grad_scale);
            d[i] = from_f32<TD>(g);
        }
    }
}


// Small vocabularies (V <= 128: the character-level model): 16 lanes per row, four rows per wave, the row held in registers
// (the wave-per-row kernel above left 3/4 of its lanes idle at V = 80 and read the row three times: 12 us for 8 MB).
// Its 16-lane row body (load, max, shuffle, exp, sum, shuffle) stands again in the fused kernel below, on purpose: as one function,
// whether it returns a struct or fills references, the compiler orders the operands of the sums differently and, in the forms with a
// CeOpt, turns selects into branches -- all 16 instantiations come out as other code.
template <typename TD, typename... O>
__global__ __launch_bounds__(256) void cross_entropy_small_kernel(const float* __restrict__ logits, int64_t ldl, const int64_t* __restrict__ targets,
                                                                  float* __restrict__ loss_rows, TD* __restrict__ dlogits, int64_t ldd,
                                                                  float grad_scale, const float* __restrict__ gs_dev, int M, int V, O... o) {
    const CePack<O...> p(o...);
    constexpr bool OPT = p.OPT, IGN = p.IGN;
    const int sub = threadIdx.x & 15;
    const int row = blockIdx.x * 16 + (threadIdx.x >> 4);
    const bool ok = row < M;
    const float* x = logits + (int64_t)(ok ? row : 0) * ldl;
    // an ignored row keeps its 16 lanes in the shuffles below on zeros that it never loaded, and stores zeros
    const bool skip = IGN && ok && targets[row] == p.ign.ignore_index;
    float v[8];
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int i = sub + 16 * k;
        v[k] = i < V ? (IGN && skip ? 0.f : x[i]) : -INFINITY;
        mx = fmaxf(mx, v[k]);
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    float s = 0.f, sd = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (OPT && sub + 16 * k < V) sd += mx - v[k];            // (the -inf of a padding lane stays out)
        v[k] = expf(v[k] - mx); s += v[k];
    }
#pragma unroll
    for (int sh = 8; sh > 0; sh >>= 1) s += __shfl_xor(s, sh, 64);
    if (OPT) {
#pragma unroll
        for (int sh = 8; sh > 0; sh >>= 1) sd += __shfl_xor(sd, sh, 64);
    }
    if (!ok) return;
    if (IGN && skip) {
        if (sub == 0) loss_rows[row] = 0.f;
        if (dlogits) {
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (sub + 16 * k < (int)ldd) dlogits[(int64_t)row * ldd + sub + 16 * k] = from_f32<TD>(0.f);
        }
        return;
    }
    const int64_t t = ce_clamp_target(targets[row], V);
    if (sub == 0) loss_rows[row] = ce_row_loss<OPT, IGN>(mx, logf(s), x[t], sd, V, p.opt);
    if (dlogits) {
        TD* d = dlogits + (int64_t)row * ldd;
        const float inv = ce_inv<OPT>(mx, logf(s), s, p.opt), unif = ce_unif<OPT>(V, p.opt);
        if (gs_dev) grad_scale *= gs_dev[0];
        if (IGN) grad_scale *= p.ign.inv_count[0];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int i = sub + 16 * k;
            if (i < (int)ldd) d[i] = from_f32<TD>(i >= V ? 0.f : ce_grad<OPT>(v[k] * inv, i == (int)t, unif, p.opt, grad_scale));
        }
    }
}

// The same rows-in-registers scheme as a whole loss head for the engine's step (V <= 128): workgroup b takes rows
// [b * rows_per, (b + 1) * rows_per), writes the gradient rows, partial row b of the column sums of the gradient (the lm_head
// bias gradient, fp32 values before rounding, row groups added in a fixed order) and its share of the loss; the workgroup that
// arrives last at the counter adds the shares up in index order and writes loss_out = scale * sum -- the mean loss without a
// reduction launch, bit-identical from run to run.  Shares and counter travel as agent-scope atomics (the per-XCD L2s are not
// coherent); the counter is back at zero when the launch ends.
struct CeFuse {
    float* colsum_part; int64_t part_stride; int rows_per;
    float* loss_part; unsigned* counter; float* loss_out; float loss_scale;
};
#define CEF_THREADS 1024                  // 64 row groups of 16 lanes: a 64-row share of the batch is in flight at once
#define CEF_RG (CEF_THREADS / 16)
template <typename TD, typename... O>
__global__ __launch_bounds__(CEF_THREADS) void cross_entropy_small_fused_kernel(const float* __restrict__ logits, int64_t ldl, const int64_t* __restrict__ targets,
                                                                        float* __restrict__ loss_rows, TD* __restrict__ dlogits, int64_t ldd,
                                                                        float grad_scale, int M, int V, CeFuse fz, O... o) {
    const CePack<O...> p(o...);
    constexpr bool OPT = p.OPT, IGN = p.IGN;
    __shared__ float red[CEF_RG][128];
    __shared__ float lred[CEF_RG];
    __shared__ unsigned last_flag;
    const int tid = threadIdx.x, sub = tid & 15, rg = tid >> 4;
    const int m_begin = blockIdx.x * fz.rows_per;
    int m_end = m_begin + fz.rows_per; if (m_end > M) m_end = M;
    float cacc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) cacc[k] = 0.f;
    float lsum = 0.f;
    if (IGN) grad_scale *= p.ign.inv_count[0];
    for (int r0 = m_begin; r0 < m_end; r0 += CEF_RG) {            // (uniform trip count: the shuffles below need every lane)
        const int row = r0 + rg;
        const bool ok = row < m_end;
        const float* x = logits + (int64_t)(ok ? row : m_begin) * ldl;
        // an ignored row group stays in the trip and in the shuffles on zeros that it never loaded: it stores zeros and adds
        // nothing to the column sums or to the loss share
        const bool skip = IGN && ok && targets[row] == p.ign.ignore_index;
        float v[8];
        float mx = -INFINITY;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int i = sub + 16 * k;
            v[k] = i < V ? (IGN && skip ? 0.f : x[i]) : -INFINITY;
            mx = fmaxf(mx, v[k]);
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        float s = 0.f, sd = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (OPT && sub + 16 * k < V) sd += mx - v[k];            // (the -inf of a padding lane stays out)
            v[k] = expf(v[k] - mx); s += v[k];
        }
#pragma unroll
        for (int sh = 8; sh > 0; sh >>= 1) s += __shfl_xor(s, sh, 64);
        if (OPT) {
#pragma unroll
            for (int sh = 8; sh > 0; sh >>= 1) sd += __shfl_xor(sd, sh, 64);
        }
        if (!ok) continue;
        if (IGN && skip) {
            if (sub == 0) loss_rows[row] = 0.f;
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (sub + 16 * k < (int)ldd) dlogits[(int64_t)row * ldd + sub + 16 * k] = from_f32<TD>(0.f);
            continue;
        }
        const int64_t t = ce_clamp_target(targets[row], V);
        const float lr = ce_row_loss<OPT, IGN>(mx, logf(s), x[t], sd, V, p.opt);
        if (sub == 0) { loss_rows[row] = lr; lsum += lr; }
        TD* d = dlogits + (int64_t)row * ldd;
        const float inv = ce_inv<OPT>(mx, logf(s), s, p.opt), unif = ce_unif<OPT>(V, p.opt);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int i = sub + 16 * k;
            // (with zeta > 0 a row no longer sums to zero: cacc stays the column sum of exactly what is written)
            const float gk = i >= V ? 0.f : ce_grad<OPT>(v[k] * inv, i == (int)t, unif, p.opt, grad_scale);
            cacc[k] += gk;
            if (i < (int)ldd) d[i] = from_f32<TD>(gk);
        }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) red[rg][sub + 16 * k] = cacc[k];
    if (sub == 0) lred[rg] = lsum;
    __syncthreads();
    if (fz.colsum_part && tid < V) {
        float c = 0.f;
#pragma unroll 8
        for (int r = 0; r < CEF_RG; ++r) c += red[r][tid];
        fz.colsum_part[(int64_t)blockIdx.x * fz.part_stride + tid] = c;
    }
    if (!fz.loss_out) return;
    if (tid == 0) {
        float b = 0.f;
#pragma unroll 8
        for (int r = 0; r < CEF_RG; ++r) b += lred[r];
        __hip_atomic_store(fz.loss_part + blockIdx.x, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // the share must be ACKNOWLEDGED by L2 before the counter moves: a workgroup-scope release does not wait on vmcnt on gfx9
        // (no tgsplit), and an agent-scope release would write the whole L2 back; the explicit wait is what the dW hand-over uses
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned prev = __hip_atomic_fetch_add(fz.counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last_flag = prev == gridDim.x - 1 ? 1u : 0u;
    }
    __syncthreads();
    if (!last_flag) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    // the last workgroup: every share is in memory; thread i fetches shares i, i + 256, ...; added up in index order
    float* sh = &red[0][0];                                              // >= 2048 floats
    for (int i = tid; i < (int)gridDim.x; i += CEF_THREADS) sh[i] = __hip_atomic_load(fz.loss_part + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (tid == 0) {
        float tot = 0.f;
        for (int i = 0; i < (int)gridDim.x; ++i) tot += sh[i];
        fz.loss_out[0] = IGN ? tot * (fz.loss_scale * p.ign.inv_count[0]) : tot * fz.loss_scale;
        __hip_atomic_store(fz.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

#define CE_BLOCK 1024
#define CE_MAXK 52                    // values per thread (128-VGPR budget at 16 waves per workgroup): rows up to 53248 logits
// The reductions of the two whole-row kernels over the 16 waves of a workgroup, once every wave's leader has stored its value to red
// (and, under OPT, its sd to red2).  The leaders' stores stay in the kernels: as part of these helpers their basic blocks land in front
// of the unrolled load loop and the kernels come out one or two instructions longer.
// The maximum: its second barrier frees red for the sums.
__device__ __forceinline__ float ce_block_max(const float* red) {
    __syncthreads();
    float mx = red[0];
#pragma unroll
    for (int k = 1; k < 16; ++k) mx = fmaxf(mx, red[k]);
    __syncthreads();
    return mx;
}
// s and sd together: one store phase, ONE barrier, then both sums, red2 touched only under OPT.  (Two phases with a barrier each took
// the CeOpt forms, which sit at the register limit, from 16 to 176 bytes of scratch.)
struct CeSums { float s, sd; };
template <bool OPT> __device__ __forceinline__ CeSums ce_block_sums(const float* red, const float* red2) {
    __syncthreads();
    float s = red[0], sd = 0.f;
#pragma unroll
    for (int k = 1; k < 16; ++k) s += red[k];             // fixed order
    if (OPT) {
        sd = red2[0];
#pragma unroll
        for (int k = 1; k < 16; ++k) sd += red2[k];
    }
    return CeSums{s, sd};
}

// TL: logits type.  bf16 logits (the engine at the GPT-2 vocabulary: 0.82 GB instead of 1.65 GB written by lm_head and read here)
// may be overwritten IN PLACE by their own gradient (dlogits == logits, ldd == ldl): a workgroup holds its whole row in
// registers before it stores anything.
template <typename TD, typename TL = float, typename... O>
__global__ __launch_bounds__(CE_BLOCK) void cross_entropy_row_kernel(const TL* logits, int64_t ldl, const int64_t* __restrict__ targets,
                                                                      float* __restrict__ loss_rows, TD* dlogits, int64_t ldd,   // (may alias)
                                                                      float grad_scale, const float* __restrict__ gs_dev, int M, int V, O... o) {
    const CePack<O...> p(o...);
    constexpr bool OPT = p.OPT, IGN = p.IGN;
    __shared__ float red[16];
    __shared__ float red2[OPT ? 16 : 1];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int row = blockIdx.x;
    const TL* x = logits + (int64_t)row * ldl;
    int64_t t = targets[row];
    if (IGN && t == p.ign.ignore_index)                  // (workgroup-uniform, before any load of the row and any barrier)
        return ce_zero_row(loss_rows, dlogits, ldd, row, tid, CE_BLOCK);
    float v[CE_MAXK];
    float mx = -INFINITY;
    t = ce_clamp_target(t, V);
    const float xt = (float)x[t];                        // before any store of this row (in-place gradient)
#pragma unroll
    for (int k = 0; k < CE_MAXK; ++k) {
        const int i = k * CE_BLOCK + tid;
        v[k] = i < V ? (float)x[i] : -INFINITY;
        mx = fmaxf(mx, v[k]);
    }
    mx = wave_max(mx);
    if (lane == 0) red[w] = mx;
    mx = ce_block_max(red);
    float s = 0.f, sd = 0.f;
#pragma unroll
    for (int k = 0; k < CE_MAXK; ++k) {
        if (OPT && k * CE_BLOCK + tid < V) sd += mx - v[k];      // (the -inf of a padding lane stays out)
        v[k] = expf(v[k] - mx);                          // exp(-inf) = 0 for the padding
        s += v[k];
    }
    s = wave_sum(s);
    if (OPT) sd = wave_sum(sd);
    if (lane == 0) red[w] = s;
    if (OPT && lane == 0) red2[w] = sd;
    const CeSums sums = ce_block_sums<OPT>(red, red2);
    s = sums.s; sd = sums.sd;
    if (tid == 0) loss_rows[row] = ce_row_loss<OPT, IGN>(mx, logf(s), xt, sd, V, p.opt);
    if (dlogits) {
        TD* d = dlogits + (int64_t)row * ldd;
        const float inv = ce_inv<OPT>(mx, logf(s), s, p.opt), unif = ce_unif<OPT>(V, p.opt);
        if (gs_dev) grad_scale *= gs_dev[0];
        if (IGN) grad_scale *= p.ign.inv_count[0];
#pragma unroll
        for (int k = 0; k < CE_MAXK; ++k) {
            const int i = k * CE_BLOCK + tid;
            if (i < (int)ldd) d[i] = from_f32<TD>(i >= V ? 0.f : ce_grad<OPT>(v[k] * inv, i == (int)t, unif, p.opt, grad_scale));
        }
    }
}

// bf16 logits, vectorised: a thread owns 16-byte chunks (8 logits) c = tid + 1024 j of its row, j < CE_MAXC: 16-byte loads and
// stores (the 2-byte-per-lane form of the generic kernel ran at half the rate of the fp32 one: 1240 us instead of 636 us for
// M = 8192 rows of 50257).  ldl % 8 == 0 and a 16-byte aligned base; may run in place (dlogits == logits).
#define CE_MAXC 7                     // 7 x 1024 x 8 = 57344 >= 53248
// exp(x - mx) as ONE v_exp_f32 behind one fused multiply-add: exp2(x log2(e) - mx log2(e)).  expf() is ~12 instructions here (range
// reduction, ldexp, the overflow / underflow selects) and this kernel evaluates it twice per logit: the instruction stream, not the
// 1.65 GB, was what bounded it (~36 executed VALU instructions per logit, two thirds of them in the two exponentials).  The argument
// is <= 0, results below 2^-126 flush to zero; relative error <= 2^-23 + |x - mx| 2^-24 log2(e) (2e-6 at x - mx = -20), three orders of
// magnitude below the bf16 rounding of the gradient this kernel writes.  The fp32-logits kernels keep expf (the parity mode).
#define CE_LOG2E 1.4426950408889634f
__device__ __forceinline__ float ce_exp_fast(float x, float mxl) { return __builtin_amdgcn_exp2f(__builtin_fmaf(x, CE_LOG2E, -mxl)); }
// The row stays in registers as the bf16 words it was loaded as (28 registers per thread instead of 56 fp32 values): at <= 64
// registers TWO workgroups are resident per CU and one's loads run beside the other's stores (one resident workgroup
// alternated between a load phase and a store phase: 570 us = 2.9 TB/s at M = 8192, V = 50257).  The exponentials are
// computed twice (sum pass, gradient pass) -- 0.8 G quarter-rate instructions, ~25 us of a kernel that moves 1.65 GB.
// q8 (nullable; round 3, precision "fp8"): the gradient a second time as OCP e5m2 with the A-PRIORI scale q8_scale = 57344 /
// grad_scale (|softmax - onehot| <= 1, so |dlogits| <= grad_scale: no amax pass, no history) -- the A operand of lm_head's fp8 dX
// GEMM and the dY operand of its fp8 dW; columns V .. ldq8 - 1 are written as zeros (the dX contraction runs over the padded width).
// With label smoothing alone the bound stands (|p_i - eps / V| < 1, |p_t - (1 - eps) - eps / V| < 1); with zeta > 0 it does not (a row
// sums to 2 zeta lse grad_scale), so the launcher gives q8 to the options only at zeta = 0.
template <typename... O>
__global__ __launch_bounds__(CE_BLOCK, 8) void cross_entropy_row_bf16_kernel(const bf16_t* logits, int64_t ldl, const int64_t* __restrict__ targets,
                                                                              float* __restrict__ loss_rows, bf16_t* dlogits, int64_t ldd,
                                                                              float grad_scale, const float* __restrict__ gs_dev, int M, int V,
                                                                              unsigned char* __restrict__ q8, int64_t ldq8, float q8_scale, O... o) {
    const CePack<O...> p(o...);
    constexpr bool OPT = p.OPT, IGN = p.IGN;
    __shared__ float red[16];
    __shared__ float red2[OPT ? 16 : 1];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int row = blockIdx.x;
    const bf16_t* x = logits + (int64_t)row * ldl;
    int64_t t = targets[row];
    if (IGN && t == p.ign.ignore_index)                  // (workgroup-uniform, before any load of the row and any barrier; never with q8)
        return ce_zero_row_x8(loss_rows, dlogits, ldd, row, tid, CE_BLOCK);
    t = ce_clamp_target(t, V);
    const float xt = (float)x[t];                        // before any store of this row (in-place gradient)
    const int nchunk = (int)((dlogits && ldd > V ? ldd : (int64_t)V) + 7) / 8;      // chunks that exist in memory (ldl >= that * 8)
    bf16x8 q[CE_MAXC];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < CE_MAXC; ++j) {
        const int c = tid + CE_BLOCK * j;
        if (c < nchunk && c * 8 < V) {
            q[j] = *(const bf16x8*)(x + c * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (c * 8 + e < V) mx = fmaxf(mx, (float)q[j][e]);
        }
    }
    mx = wave_max(mx);
    if (lane == 0) red[w] = mx;
    mx = ce_block_max(red);
    const float mxl = mx * CE_LOG2E;
    float s = 0.f, sd = 0.f;
#pragma unroll
    for (int j = 0; j < CE_MAXC; ++j) {
        const int c = tid + CE_BLOCK * j;
        if (c < nchunk && c * 8 < V) {
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (c * 8 + e < V) {
                    s += ce_exp_fast((float)q[j][e], mxl);
                    if (OPT) sd += mx - (float)q[j][e];
                }
        }
    }
    s = wave_sum(s);
    if (OPT) sd = wave_sum(sd);
    if (lane == 0) red[w] = s;
    if (OPT && lane == 0) red2[w] = sd;
    const CeSums sums = ce_block_sums<OPT>(red, red2);
    s = sums.s; sd = sums.sd;
    // (mx - xt first: exact for bf16 logits within 2^16 of each other, so a target at the row maximum gives logf(s) itself.  mx + logf(s)
    // rounds at the size of mx -- 2^-24 |mx| = 1.2e-4 at |mx| = 2000 -- on top of the 2^-24 |mx| that the rounding of mx log2(e) already
    // costs through ce_exp_fast: tests/test_gpu_conditioning.py, logit range 2000)
    if (tid == 0) loss_rows[row] = OPT ? ce_objective(mx, logf(s), xt, sd, V, p.opt) : (mx - xt) + logf(s);
    if (dlogits) {
        bf16_t* d = dlogits + (int64_t)row * ldd;
        const float inv = ce_inv<OPT>(mx, logf(s), s, p.opt), unif = ce_unif<OPT>(V, p.opt);
        if (gs_dev) grad_scale *= gs_dev[0];
        if (IGN) grad_scale *= p.ign.inv_count[0];
        const int dchunk = (int)(ldd / 8);
#pragma unroll
        for (int j = 0; j < CE_MAXC; ++j) {
            const int c = tid + CE_BLOCK * j;
            if (c < dchunk) {
                bf16x8 o;
                float gv[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int i = c * 8 + e;
                    gv[e] = i >= V ? 0.f : ce_grad<OPT>(ce_exp_fast((float)q[j][e], mxl) * inv, i == (int)t, unif, p.opt, grad_scale);
                    o[e] = (bf16_t)gv[e];
                }
                *(bf16x8*)(d + c * 8) = o;
                if (q8 && c * 8 < ldq8) {                                 // (uniform per launch; ldq8 % 8 == 0)
                    int lo = 0, hi = 0;
                    lo = __builtin_amdgcn_cvt_pk_bf8_f32(gv[0] * q8_scale, gv[1] * q8_scale, lo, false);
                    lo = __builtin_amdgcn_cvt_pk_bf8_f32(gv[2] * q8_scale, gv[3] * q8_scale, lo, true);
                    hi = __builtin_amdgcn_cvt_pk_bf8_f32(gv[4] * q8_scale, gv[5] * q8_scale, hi, false);
                    hi = __builtin_amdgcn_cvt_pk_bf8_f32(gv[6] * q8_scale, gv[7] * q8_scale, hi, true);
                    typedef int i32x2 __attribute__((ext_vector_type(2)));
                    *(i32x2*)(q8 + (int64_t)row * ldq8 + c * 8) = (i32x2){lo, hi};
                }
            }
        }
    }
}

// {(float)N, 1.0f / (float)N}, N the number of targets that are not ignore_index: one workgroup, an integer sum (no order to fix), the
// reciprocal one correctly rounded fp32 division (+inf at N = 0).  Everything the ignore forms need to know about the batch.
__global__ __launch_bounds__(1024) void ce_count_valid_kernel(const int64_t* __restrict__ targets, int M, int64_t ignore_index, float* __restrict__ out) {
    __shared__ int red[16];
    int n = 0;
    for (int i = threadIdx.x; i < M; i += 1024) n += targets[i] != ignore_index ? 1 : 0;
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) n += __shfl_xor(n, sh, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) tot += red[k];
        const float nf = (float)tot;
        out[0] = nf;
        out[1] = __fdiv_rn(1.0f, nf);
    }
}

// ---------------------------------------------------------------------------------------------
// Host side.  The one place that chooses the pack: launch() with nothing (both options zero, no ign: the plain kernels), a CeOpt, a
// CeIgn (both options zero: the CeIgn alone), or a CeOpt and a CeIgn.
// eps in [0, 1), zeta >= 0, both finite (a NaN fails every comparison)
static bool ce_opt_ok(float eps, float zeta) { return eps >= 0.f && eps < 1.f && zeta >= 0.f && zeta <= FLT_MAX; }
template <typename F> static int ce_with_options(float eps, float zeta, const CeIgn* ign, F&& launch) {
    if (!ce_opt_ok(eps, zeta) || (ign && !ign->inv_count)) return DG_ERR_ARG;
    const bool plain = eps == 0.f && zeta == 0.f;
    if (ign) return plain ? launch(*ign) : launch(CeOpt{eps, zeta}, *ign);
    return plain ? launch() : launch(CeOpt{eps, zeta});
}
// The gradient's type: launch(d) with dlogits as a bf16_t* or a float*, whichever dtype names
template <typename F> static int ce_with_grad_type(int dtype, void* dlogits, F&& launch) {
    if (dtype == DG_BF16) launch((bf16_t*)dlogits);
    else if (dtype == DG_F32) launch((float*)dlogits);
    else return DG_ERR_DTYPE;
    DG_LAUNCH_CHECK();
    return DG_OK;
}
template <typename P> using ce_pointee = std::remove_pointer_t<P>;

// ign: null, or the CeIgn of an _ignore entry point; q8: null but for the _fp8 entry points
static int ce_rows(const void* logits_v, int logits_dtype, int64_t ldl, const int64_t* targets, float* loss_rows, void* dlogits, int64_t ldd,
                   int dtype, float grad_scale, const float* grad_scale_dev, int M, int V, unsigned char* q8, int64_t ldq8, float q8_scale,
                   float eps, float zeta, const CeIgn* ign, void* stream) {
    return ce_with_options(eps, zeta, ign, [&](auto... opt) -> int {
        if (!logits_v || !targets || !loss_rows || M <= 0 || V <= 0 || ldl < V) return DG_ERR_ARG;
        if (dlogits && ldd < V) return DG_ERR_ARG;
        if (ign && q8) return DG_ERR_ARG;                    // (the e5m2 scale rests on |dlogits| <= 1 / M: see dg_cross_entropy_fp8)
        if (logits_dtype != DG_F32 && logits_dtype != DG_BF16) return DG_ERR_DTYPE;
        hipStream_t s = (hipStream_t)stream;
        const int64_t width = dlogits && ldd > V ? ldd : V;
        if (logits_dtype == DG_BF16) {
            // bf16 logits: the whole-row kernel only (its in-place form is what they exist for); gradient in bf16
            if (width > (int64_t)CE_BLOCK * CE_MAXK) return DG_ERR_ARG;
            if (dlogits && dtype != DG_BF16) return DG_ERR_DTYPE;
            if (dlogits == logits_v && ldd != ldl) return DG_ERR_ARG;
            const bool vec = ldl % 8 == 0 && dg_aligned16(logits_v) && (!dlogits || (ldd % 8 == 0 && dg_aligned16(dlogits))) &&
                             (int64_t)((V + 7) / 8) * 8 <= ldl && width <= (int64_t)CE_BLOCK * CE_MAXC * 8;
            if (q8 && !vec) return DG_ERR_ARG;
            if (vec)
                hipLaunchKernelGGL((cross_entropy_row_bf16_kernel<decltype(opt)...>), dim3(M), dim3(CE_BLOCK), 0, s, (const bf16_t*)logits_v, ldl,
                                   targets, loss_rows, (bf16_t*)dlogits, ldd, grad_scale, grad_scale_dev, M, V, q8, ldq8, q8_scale, opt...);
            else
                hipLaunchKernelGGL((cross_entropy_row_kernel<bf16_t, bf16_t, decltype(opt)...>), dim3(M), dim3(CE_BLOCK), 0, s, (const bf16_t*)logits_v,
                                   ldl, targets, loss_rows, (bf16_t*)dlogits, ldd, grad_scale, grad_scale_dev, M, V, opt...);
            DG_LAUNCH_CHECK();
            return DG_OK;
        }
        const float* logits = (const float*)logits_v;
        if (dlogits == logits_v) return DG_ERR_ARG;          // in place only with bf16 logits
        return ce_with_grad_type(dtype, dlogits, [&](auto* d) {
            using TD = ce_pointee<decltype(d)>;
            if (width <= 128)
                hipLaunchKernelGGL((cross_entropy_small_kernel<TD, decltype(opt)...>), dim3((M + 15) / 16), dim3(256), 0, s, logits, ldl, targets, loss_rows,
                                   d, ldd, grad_scale, grad_scale_dev, M, V, opt...);
            else if (V > 4096 && width <= (int64_t)CE_BLOCK * CE_MAXK)
                hipLaunchKernelGGL((cross_entropy_row_kernel<TD, float, decltype(opt)...>), dim3(M), dim3(CE_BLOCK), 0, s, logits, ldl, targets, loss_rows,
                                   d, ldd, grad_scale, grad_scale_dev, M, V, opt...);
            else
                hipLaunchKernelGGL((cross_entropy_kernel<TD, float, decltype(opt)...>), dim3((M + 3) / 4), dim3(256), 0, s, logits, ldl, targets, loss_rows,
                                   d, ldd, grad_scale, grad_scale_dev, M, V, opt...);
        });
    });
}

static int ce_fused(const float* logits, int64_t ldl, const int64_t* targets, float* loss_rows, void* dlogits, int64_t ldd, int dtype, float grad_scale,
                    int M, int V, float* colsum_part, int64_t part_stride, int n_partials, float* loss_part, uint32_t* loss_counter, float* loss_out,
                    float loss_scale, float eps, float zeta, const CeIgn* ign, void* stream) {
    return ce_with_options(eps, zeta, ign, [&](auto... opt) -> int {
        if (!logits || !targets || !loss_rows || !dlogits || M <= 0 || V <= 0 || ldl < V || ldd < V) return DG_ERR_ARG;
        if (ldd > 128 || n_partials <= 0 || n_partials > 2048) return DG_ERR_ARG;     // rows in registers; shares summed out of 8 KB of LDS
        if (colsum_part && part_stride < V) return DG_ERR_ARG;
        if ((loss_out != nullptr) != (loss_part != nullptr) || (loss_out != nullptr) != (loss_counter != nullptr)) return DG_ERR_ARG;
        const int rows_per = (M + n_partials - 1) / n_partials;
        const CeFuse fz{colsum_part, part_stride, rows_per, loss_part, (unsigned*)loss_counter, loss_out, loss_scale};
        return ce_with_grad_type(dtype, dlogits, [&](auto* d) {
            hipLaunchKernelGGL((cross_entropy_small_fused_kernel<ce_pointee<decltype(d)>, decltype(opt)...>), dim3(n_partials), dim3(CEF_THREADS), 0,
                               (hipStream_t)stream, logits, ldl, targets, loss_rows, d, ldd, grad_scale, M, V, fz, opt...);
        });
    });
}

extern "C" int dg_cross_entropy(const void* logits_v, int logits_dtype, int64_t ldl, const int64_t* targets, float* loss_rows,
                                void* dlogits, int64_t ldd, int dtype, float grad_scale, const float* grad_scale_dev, int M, int V, void* stream) {
    return ce_rows(logits_v, logits_dtype, ldl, targets, loss_rows, dlogits, ldd, dtype, grad_scale, grad_scale_dev, M, V, nullptr, 0, 0.f, 0.f, 0.f,
                   nullptr, stream);
}

extern "C" int dg_cross_entropy_smooth(const void* logits_v, int logits_dtype, int64_t ldl, const int64_t* targets, float* loss_rows,
                                       void* dlogits, int64_t ldd, int dtype, float grad_scale, const float* grad_scale_dev, int M, int V,
                                       float label_smoothing, float z_loss, void* stream) {
    return ce_rows(logits_v, logits_dtype, ldl, targets, loss_rows, dlogits, ldd, dtype, grad_scale, grad_scale_dev, M, V, nullptr, 0, 0.f,
                   label_smoothing, z_loss, nullptr, stream);
}

// rows whose target equals ignore_index left out; inv_count: device, 1 / N (the second word of dg_ce_count_valid's output)
extern "C" int dg_cross_entropy_ignore(const void* logits_v, int logits_dtype, int64_t ldl, const int64_t* targets, float* loss_rows,
                                       void* dlogits, int64_t ldd, int dtype, float grad_scale, const float* grad_scale_dev, int M, int V,
                                       float label_smoothing, float z_loss, int64_t ignore_index, const float* inv_count, void* stream) {
    const CeIgn ign{ignore_index, inv_count};
    return ce_rows(logits_v, logits_dtype, ldl, targets, loss_rows, dlogits, ldd, dtype, grad_scale, grad_scale_dev, M, V, nullptr, 0, 0.f,
                   label_smoothing, z_loss, &ign, stream);
}

// bf16 logits (the whole-row kernel, 16-byte accesses) with the gradient ALSO as e5m2: dlogits_fp8 [M, ld8] = e5m2(dlogits * 57344 /
// grad_scale), dequantisation factor grad_scale / 57344 (a constant the caller knows); ld8 % 16 == 0, ld8 >= V, columns beyond V zero.
// Label smoothing only: |g_i| <= grad_scale, on which the a-priori scale rests, does not survive a z-loss
extern "C" int dg_cross_entropy_fp8_smooth(const void* logits, int64_t ldl, const int64_t* targets, float* loss_rows, void* dlogits, int64_t ldd,
                                           float grad_scale, int M, int V, void* dlogits_fp8, int64_t ld8, float label_smoothing, void* stream) {
    if (!ce_opt_ok(label_smoothing, 0.f)) return DG_ERR_ARG;
    if (!dlogits || !dlogits_fp8 || ld8 < V || ld8 % 16 || ld8 > ldd || !dg_aligned16(dlogits_fp8) || !(grad_scale > 0.f)) return DG_ERR_ARG;
    if (ldl % 8 || ldd % 8 || !dg_aligned16(logits) || !dg_aligned16(dlogits) || (int64_t)((V + 7) / 8) * 8 > ldl) return DG_ERR_ALIGN;
    return ce_rows(logits, DG_BF16, ldl, targets, loss_rows, dlogits, ldd, DG_BF16, grad_scale, nullptr, M, V, (unsigned char*)dlogits_fp8, ld8,
                   57344.f / grad_scale, label_smoothing, 0.f, nullptr, stream);
}

extern "C" int dg_cross_entropy_fp8(const void* logits, int64_t ldl, const int64_t* targets, float* loss_rows, void* dlogits, int64_t ldd,
                                    float grad_scale, int M, int V, void* dlogits_fp8, int64_t ld8, void* stream) {
    return dg_cross_entropy_fp8_smooth(logits, ldl, targets, loss_rows, dlogits, ldd, grad_scale, M, V, dlogits_fp8, ld8, 0.f, stream);
}

extern "C" int dg_cross_entropy_fused(const float* logits, int64_t ldl, const int64_t* targets, float* loss_rows, void* dlogits, int64_t ldd,
                                      int dtype, float grad_scale, int M, int V, float* colsum_part, int64_t part_stride, int n_partials,
                                      float* loss_part, uint32_t* loss_counter, float* loss_out, float loss_scale, void* stream) {
    return ce_fused(logits, ldl, targets, loss_rows, dlogits, ldd, dtype, grad_scale, M, V, colsum_part, part_stride, n_partials, loss_part, loss_counter,
                    loss_out, loss_scale, 0.f, 0.f, nullptr, stream);
}

extern "C" int dg_cross_entropy_fused_smooth(const float* logits, int64_t ldl, const int64_t* targets, float* loss_rows, void* dlogits, int64_t ldd,
                                             int dtype, float grad_scale, int M, int V, float* colsum_part, int64_t part_stride, int n_partials,
                                             float* loss_part, uint32_t* loss_counter, float* loss_out, float loss_scale,
                                             float label_smoothing, float z_loss, void* stream) {
    return ce_fused(logits, ldl, targets, loss_rows, dlogits, ldd, dtype, grad_scale, M, V, colsum_part, part_stride, n_partials, loss_part, loss_counter,
                    loss_out, loss_scale, label_smoothing, z_loss, nullptr, stream);
}

// loss_out = loss_scale * inv_count[0] * sum(rows); the column-sum partials hold the rows that count only
extern "C" int dg_cross_entropy_fused_ignore(const float* logits, int64_t ldl, const int64_t* targets, float* loss_rows, void* dlogits, int64_t ldd,
                                             int dtype, float grad_scale, int M, int V, float* colsum_part, int64_t part_stride, int n_partials,
                                             float* loss_part, uint32_t* loss_counter, float* loss_out, float loss_scale,
                                             float label_smoothing, float z_loss, int64_t ignore_index, const float* inv_count, void* stream) {
    const CeIgn ign{ignore_index, inv_count};
    return ce_fused(logits, ldl, targets, loss_rows, dlogits, ldd, dtype, grad_scale, M, V, colsum_part, part_stride, n_partials, loss_part, loss_counter,
                    loss_out, loss_scale, label_smoothing, z_loss, &ign, stream);
}

extern "C" int dg_ce_count_valid(const int64_t* targets, int M, int64_t ignore_index, float* out, void* stream) {
    if (!targets || !out || M <= 0) return DG_ERR_ARG;
    hipLaunchKernelGGL(ce_count_valid_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, targets, M, ignore_index, out);
    DG_LAUNCH_CHECK();
    return DG_OK;
}
