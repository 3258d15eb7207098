// Gradient accumulation over micro-batches (ref: k x `(loss / k).backward()` summing into p.grad between two optimizer.step()
// calls): one streaming pass per micro-step that adds the micro-batch's flat gradient into a flat fp32 accumulator.
//   ctl = {j, k, arrival counter, 0}: j is the micro-step inside the current optimizer step, k = accum_steps.
//   j == 0: acc = g  (acc is not read: no zero-fill launch anywhere, 8 B/param);   j > 0: acc = acc + g  (12 B/param).
// One fp32 add per element, no scale and no FMA: a host restatement (tests/accum_model.py) is bit-exact.
// The launch also moves both counters on, by dg_adamw_step's protocol: every workgroup reads j, k and the micro-step word first
// thing and registers at the arrival counter when it is done; the last one to arrive clears the counter and writes
// ctl[0] = (j + 1) mod k and rng_state[2] = step + 1.  Nothing behind this launch in a micro-step reads either word.
#include "common.h"

#define DG_ACCUM_WG 256
#define DG_ACCUM_MAX_GRID 2048

__global__ __launch_bounds__(DG_ACCUM_WG) void grad_accumulate_kernel(float* __restrict__ acc, const float* __restrict__ g, int64_t n,
                                                                      uint32_t* ctl, const float* __restrict__ loss, float* loss_out,
                                                                      uint32_t* rng_state) {
    const uint32_t j = ctl[0], k = ctl[1];
    const uint32_t step_now = rng_state ? rng_state[2] : 0u;
    const int64_t gs = (int64_t)gridDim.x * DG_ACCUM_WG;
    const int64_t n4 = n / 4;
    const int64_t i0 = (int64_t)blockIdx.x * DG_ACCUM_WG + threadIdx.x;
    if (j == 0) {
        for (int64_t i = i0; i < n4; i += gs) ((f32x4*)acc)[i] = ((const f32x4*)g)[i];
        for (int64_t i = n4 * 4 + i0; i < n; i += gs) acc[i] = g[i];
    } else {
        for (int64_t i = i0; i < n4; i += gs) {
            const f32x4 a = ((const f32x4*)acc)[i], b = ((const f32x4*)g)[i];
            ((f32x4*)acc)[i] = a + b;
        }
        for (int64_t i = n4 * 4 + i0; i < n; i += gs) acc[i] = acc[i] + g[i];
    }
    if (loss && blockIdx.x == 0 && threadIdx.x == 0) {
        const float s = j == 0 ? loss[0] : loss_out[0] + loss[0];
        loss_out[0] = s;
        if (j + 1u == k) loss_out[1] = s / (float)k;
    }
    __syncthreads();                                       // (every wave of this workgroup has read j, k and the step word long ago)
    if (threadIdx.x == 0) {
        const unsigned prev = __hip_atomic_fetch_add(ctl + 2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (prev == gridDim.x - 1) {
            __hip_atomic_store(ctl + 2, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(ctl + 0, j + 1u == k ? 0u : j + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (rng_state) __hip_atomic_store(rng_state + 2, step_now + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

extern "C" int dg_grad_accumulate(float* acc, const float* g, int64_t n, uint32_t* ctl, const float* loss, float* loss_out,
                                  uint32_t* rng_state, void* stream) {
    if (!acc || !g || !ctl || n <= 0) return DG_ERR_ARG;
    if ((loss != nullptr) != (loss_out != nullptr)) return DG_ERR_ARG;
    if (!dg_aligned16(acc) || !dg_aligned16(g)) return DG_ERR_ALIGN;
    int64_t grid = (n / 4 + DG_ACCUM_WG - 1) / DG_ACCUM_WG;          // the grid cap of dg_adamw_step
    if (grid < 1) grid = 1;
    if (grid > DG_ACCUM_MAX_GRID) grid = DG_ACCUM_MAX_GRID;
    hipLaunchKernelGGL(grad_accumulate_kernel, dim3((unsigned)grid), dim3(DG_ACCUM_WG), 0, (hipStream_t)stream, acc, g, n, ctl, loss,
                       loss_out, rng_state);
    DG_LAUNCH_CHECK();
    return DG_OK;
}
