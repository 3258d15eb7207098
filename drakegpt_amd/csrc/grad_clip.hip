// Global-norm gradient clipping (ref: torch.nn.utils.clip_grad_norm_(params, max_norm), norm_type 2) in two launches:
//   1. sumsq_partials_kernel: sum of squares of a flat fp32 buffer, one fp64 partial per workgroup;
//   2. grad_norm_finalize_kernel: ONE workgroup sums the partials in a fixed order and writes {total_norm, coef}.
// Deterministic by construction: the grid depends on n alone (never on the CU count), every thread walks a fixed index set, the
// wave / workgroup sums run in a fixed tree, and the partials are summed by one workgroup in index order -- no float atomics, no
// arrival order.  The coefficient is applied inside the AdamW launch
// (dg_adamw_step_clip), so the stored gradient stays unclipped.
#include "common.h"

#define DG_SUMSQ_WG 256
#define DG_SUMSQ_MAX_GRID 2048
#define DG_SUMSQ_UNROLL 4         // 16-B loads in flight per lane and loop trip

static int64_t sumsq_grid(int64_t n) {
    // one workgroup per DG_SUMSQ_UNROLL x 256 x 4 floats, at most DG_SUMSQ_MAX_GRID (8 per CU: enough loads in flight to stream)
    int64_t per = (int64_t)DG_SUMSQ_UNROLL * DG_SUMSQ_WG * 4;
    int64_t g = (n + per - 1) / per;
    return g < 1 ? 1 : (g > DG_SUMSQ_MAX_GRID ? DG_SUMSQ_MAX_GRID : g);
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// fixed-order sum over the 256 threads of a workgroup: wave butterflies, then the 4 wave sums as (w0 + w1) + (w2 + w3)
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
    v = wave_sum_f64(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ __forceinline__ float sq4(f32x4 a) { return (a[0] * a[0] + a[1] * a[1]) + (a[2] * a[2] + a[3] * a[3]); }

__global__ __launch_bounds__(DG_SUMSQ_WG) void sumsq_partials_kernel(const float* __restrict__ g, int64_t n, double* __restrict__ part) {
    __shared__ double red[DG_SUMSQ_WG / 64];
    const int64_t gs = (int64_t)gridDim.x * DG_SUMSQ_WG;
    const int64_t n4 = n / 4;
    const f32x4* g4 = (const f32x4*)g;
    double acc = 0.0;
    int64_t i = (int64_t)blockIdx.x * DG_SUMSQ_WG + threadIdx.x;
    for (; i + (DG_SUMSQ_UNROLL - 1) * gs < n4; i += DG_SUMSQ_UNROLL * gs) {
        f32x4 a[DG_SUMSQ_UNROLL];
#pragma unroll
        for (int u = 0; u < DG_SUMSQ_UNROLL; ++u) a[u] = g4[i + u * gs];
#pragma unroll
        for (int u = 0; u < DG_SUMSQ_UNROLL; ++u) acc += (double)sq4(a[u]);
    }
    for (; i < n4; i += gs) acc += (double)sq4(g4[i]);
    // the 0..3 elements past the last whole float4: the first lanes of workgroup 0
    if (blockIdx.x == 0 && threadIdx.x < n - n4 * 4) {
        const float t = g[n4 * 4 + threadIdx.x];
        acc += (double)(t * t);
    }
    const double s = block_sum_f64(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// total_norm = grad_scale * sqrt(sum), rounded to fp32 once; coef as torch evaluates it in fp32:
// clamp(max_norm / (total_norm + 1e-6), max = 1) -- a NaN norm gives a NaN coefficient (the comparison below keeps it)
// G = FinalizeGuard, the update guard: the same workgroup, the same sum and the same {total_norm, coef} bits (max_norm may then be
// null: no coefficient is written), and the decision whether the optimizer update of this step is applied, in
// guard = {apply, total skipped, consecutive skipped, spare}:
//   apply = total_norm <= limit[0] && (loss == nullptr || isfinite(loss[0]))
// A NaN or Inf norm fails the comparison against any finite limit (FLT_MAX guards non-finite gradients alone; +inf would let an
// Inf norm through).  sumsq_partials_kernel squares in fp32, so a finite element beyond 1.8e19 in magnitude gives an Inf norm and
// reads as non-finite too.  Thread 0 moves the counters with plain stores; dg_adamw_step_guard reads guard[0] in the next launch.
// The pack is empty or one FinalizeGuard; the coefficient is written once for both.  The guard is taken with the fold `(gd, ...)`,
// not with dg_pack_get: copied straight from the kernel argument its pointers count as never clobbered and guard[1] is read with a
// scalar load, through the getter it is not.
struct FinalizeGuard { const float* limit; const float* loss; uint32_t* guard; };
template <typename... G>
__global__ __launch_bounds__(DG_SUMSQ_WG) void grad_norm_finalize_kernel(const double* __restrict__ part, int n_parts, float grad_scale,
                                                                         const float* __restrict__ max_norm, float* __restrict__ out, G... gd) {
    __shared__ double red[DG_SUMSQ_WG / 64];
    double acc = 0.0;
    for (int i0 = 0; i0 < n_parts; i0 += 8 * DG_SUMSQ_WG) {        // 8 independent loads in flight per lane, then a fixed-order sum
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = i0 + u * DG_SUMSQ_WG + threadIdx.x;
            v[u] = i < n_parts ? part[i] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += v[u];
    }
    const double s = block_sum_f64(acc, red);
    if (threadIdx.x == 0) {
        const float total = (float)(sqrt(s) * (double)grad_scale);
        constexpr bool GUARD = sizeof...(G) != 0;
        out[0] = total;
        if (!GUARD || max_norm) {
            const float c = max_norm[0] / (total + 1e-6f);
            out[1] = c > 1.f ? 1.f : c;
        }
        if constexpr (GUARD) {
            const FinalizeGuard fg = (gd, ...);
            bool apply = total <= fg.limit[0];
            if (fg.loss) apply = apply && isfinite(fg.loss[0]);
            fg.guard[0] = apply ? 1u : 0u;
            fg.guard[1] += apply ? 0u : 1u;
            fg.guard[2] = apply ? 0u : fg.guard[2] + 1u;
        }
    }
}

extern "C" int64_t dg_sumsq_parts(int64_t n) { return n > 0 ? sumsq_grid(n) : 0; }

extern "C" int dg_sumsq_partials(const float* g, int64_t n, double* part, void* stream) {
    if (!g || !part || n <= 0) return DG_ERR_ARG;
    if (!dg_aligned16(g)) return DG_ERR_ALIGN;
    hipLaunchKernelGGL(sumsq_partials_kernel, dim3((unsigned)sumsq_grid(n)), dim3(DG_SUMSQ_WG), 0, (hipStream_t)stream, g, n, part);
    DG_LAUNCH_CHECK();
    return DG_OK;
}

extern "C" int dg_grad_norm_finalize(const double* part, int n_parts, float grad_scale, const float* max_norm, float* out, void* stream) {
    if (!part || !max_norm || !out || n_parts <= 0) return DG_ERR_ARG;
    hipLaunchKernelGGL(grad_norm_finalize_kernel<>, dim3(1), dim3(DG_SUMSQ_WG), 0, (hipStream_t)stream, part, n_parts, grad_scale, max_norm, out);
    DG_LAUNCH_CHECK();
    return DG_OK;
}

extern "C" int dg_grad_norm_finalize_guard(const double* part, int n_parts, float grad_scale, const float* max_norm, float* out,
                                           const float* limit, const float* loss, uint32_t* guard, void* stream) {
    if (!part || !out || !limit || !guard || n_parts <= 0) return DG_ERR_ARG;
    hipLaunchKernelGGL(grad_norm_finalize_kernel<FinalizeGuard>, dim3(1), dim3(DG_SUMSQ_WG), 0, (hipStream_t)stream, part, n_parts, grad_scale, max_norm,
                       out, FinalizeGuard{limit, loss, guard});
    DG_LAUNCH_CHECK();
    return DG_OK;
}
