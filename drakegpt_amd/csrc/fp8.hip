// fp8 operand preparation for the block-scaled MFMA GEMM path (precision = "fp8", BASELINE.json configs[4]).
// OCP encodings (gfx950): e4m3fn (max 448) for forward operands, e5m2 (max 57344) for gradients.
// Per-tensor scaling, just in time: amax(x) -> scale = FMAX / amax -> q = cvt_fp8(x * scale) and the dequantisation factor
// 1 / scale goes to the GEMM epilogue (dg_gemm_nt: scale_a, scale_b).  The reference has no reduced precision at all (every
// nn.Linear of src/model_component.py:320-325,392-393,404,454 is fp32); this path replaces the operand type of those
// contractions, nothing else.  HBM-bound: 2 B read + 1 B written per element (+ 2 B read for the amax pass).
#include "common.h"

#define FP8_E4M3_MAX 448.0f
#define FP8_E5M2_MAX 57344.0f
#define FP8_BLOCK 256             // fp8_amax_kernel, fp8_quantize_kernel (= DG_FP8_AMAX_PARTS: one partial per thread)
#define FP8_DELAYED_BLOCK 1024    // fp8_quantize_delayed_kernel
template <bool BF8> constexpr float fp8_fmax = BF8 ? FP8_E5M2_MAX : FP8_E4M3_MAX;

// the maximum of |v| over a workgroup of WAVES waves, to every thread (dg_amax_nan: a NaN / Inf wins); red is free again after
// the caller's next barrier
template <int WAVES>
__device__ __forceinline__ float fp8_block_amax(float v, float (&red)[WAVES]) {
    v = wave_amax_nan(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float m = 0.f;
#pragma unroll
    for (int i = 0; i < WAVES; ++i) m = dg_amax_nan(m, red[i]);
    return m;
}

// ---------------------------------------------------------------------------------------------
// amax, without atomics and without a zero-fill launch: DG_FP8_AMAX_PARTS workgroups per segment each write the maximum of
// |x| over their share to parts[seg * PARTS + b]; the quantise kernel reduces the PARTS values of its segment itself.
// seg table: n_seg x 2 int64 {first element (multiple of 8), number of elements (multiple of 8)}; NULL = one segment.
template <typename T>
__global__ __launch_bounds__(FP8_BLOCK) void fp8_amax_kernel(const T* __restrict__ x, int64_t n, const int64_t* __restrict__ seg,
                                                             float* __restrict__ parts) {
    __shared__ float red[FP8_BLOCK / 64];
    const int s = blockIdx.x / DG_FP8_AMAX_PARTS, b = blockIdx.x % DG_FP8_AMAX_PARTS;
    const int64_t first = seg ? seg[2 * s] : 0, len = seg ? seg[2 * s + 1] : n;
    float m = 0.f;
    constexpr int V = 16 / sizeof(T);
    typedef T TV __attribute__((ext_vector_type(V)));
    const int64_t nv = len / V;
    const TV* xv = (const TV*)(x + first);
    for (int64_t i = (int64_t)b * FP8_BLOCK + threadIdx.x; i < nv; i += (int64_t)DG_FP8_AMAX_PARTS * FP8_BLOCK) {
        const TV v = xv[i];
#pragma unroll
        for (int e = 0; e < V; ++e) m = dg_amax_nan(m, (float)v[e]);
    }
    for (int64_t i = nv * V + (int64_t)b * FP8_BLOCK + threadIdx.x; i < len; i += (int64_t)DG_FP8_AMAX_PARTS * FP8_BLOCK) m = dg_amax_nan(m, (float)x[first + i]);
    m = fp8_block_amax(m, red);
    if (threadIdx.x == 0) parts[blockIdx.x] = m;
}

template <typename T>
__device__ __forceinline__ void fp8_load8(const T* p, float (&v)[8]) {
    if constexpr (sizeof(T) == 2) {
        const bf16x8 t = *(const bf16x8*)p;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (float)t[e];
    } else {
        const f32x4 t0 = *(const f32x4*)p, t1 = *(const f32x4*)(p + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[e] = t0[e]; v[4 + e] = t1[e]; }
    }
}

// Which terms keep a span of `len` elements that starts at element `first` of its tensor from the wide loop below; 0 = wide.
// x_addr / q_addr: the byte addresses of the span's first source and output element.  The kernels and fp8_plan's report ask here.
enum { FP8_NARROW_FIRST = 1, FP8_NARROW_LEN = 2, FP8_NARROW_Q = 4, FP8_NARROW_X = 8 };
__host__ __device__ __forceinline__ int fp8_narrow_terms(int64_t first, int64_t len, uintptr_t x_addr, uintptr_t q_addr) {
    return ((first & 15) ? FP8_NARROW_FIRST : 0) | ((len & 15) ? FP8_NARROW_LEN : 0) | ((q_addr & 15) ? FP8_NARROW_Q : 0) |
           ((x_addr & 15) ? FP8_NARROW_X : 0);
}

// q[i] = cvt(clamp(x[i] * sc)) over the span x[0 .. len) (x, q: the span's base, element `first` of the tensor), in units of 16 or
// 8 elements: this thread takes units unit0, unit0 + stride, ...  RECORD: the maximum of |x| over its units is returned.
// Sixteen elements per thread and trip where the span allows it (start and length multiples of 16: every weight matrix):
// ONE 16-byte store per lane instead of two 8-byte ones -- 8-byte stores run at half the rate of 16-byte ones on this part
// (DESIGN section 4), and the quantise kernel sat at 1.6 TB/s.  Odd chunk counts and unaligned spans keep the 8-element form:
// 16 B in (bf16) / 2 x 16 B (f32), 8 B out.
template <typename T, bool BF8, bool RECORD>
__device__ __forceinline__ float fp8_cast_span(const T* __restrict__ x, uint8_t* __restrict__ q, int64_t first, int64_t len,
                                               int64_t unit0, int64_t stride, float sc) {
    typedef int i32x2 __attribute__((ext_vector_type(2)));
    typedef int i32x4 __attribute__((ext_vector_type(4)));
    constexpr float fmax = fp8_fmax<BF8>;
    float m = 0.f;
    if (fp8_narrow_terms(first, len, (uintptr_t)x, (uintptr_t)q) == 0) {
        const int64_t n16 = len / 16;
        for (int64_t i = unit0; i < n16; i += stride) {
            float v0[8], v1[8];
            fp8_load8<T>(x + i * 16, v0);
            fp8_load8<T>(x + i * 16 + 8, v1);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (RECORD) { m = dg_amax_nan(m, v0[e]); m = dg_amax_nan(m, v1[e]); }
                v0[e] = dg_fp8_clamp(v0[e] * sc, fmax); v1[e] = dg_fp8_clamp(v1[e] * sc, fmax);
            }
            int a, b, c, d;
            dg_fp8_pack8<BF8>(v0, a, b);
            dg_fp8_pack8<BF8>(v1, c, d);
            *(i32x4*)(q + i * 16) = (i32x4){a, b, c, d};
        }
        return m;
    }
    const int64_t n8 = len / 8;
    for (int64_t i = unit0; i < n8; i += stride) {
        float v[8];
        fp8_load8<T>(x + i * 8, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (RECORD) m = dg_amax_nan(m, v[e]);
            v[e] = dg_fp8_clamp(v[e] * sc, fmax);
        }
        int lo, hi;
        dg_fp8_pack8<BF8>(v, lo, hi);
        *(i32x2*)(q + i * 8) = (i32x2){lo, hi};
    }
    return m;
}

// ---------------------------------------------------------------------------------------------
// q = cvt(clamp(x * scale)), scale = FMAX / amax (amax == 0: scale 1); scale_inv[seg] = 1 / scale is written by block 0 of
// the segment for the consumer.
template <typename T, bool BF8>
__global__ __launch_bounds__(FP8_BLOCK) void fp8_quantize_kernel(const T* __restrict__ x, uint8_t* __restrict__ q, int64_t n,
                                                                 const int64_t* __restrict__ seg, int n_seg, const float* __restrict__ parts,
                                                                 float* __restrict__ scale_inv, int blocks_per_seg) {
    __shared__ float red[FP8_BLOCK / 64];
    const int s = seg ? blockIdx.x / blocks_per_seg : 0;
    const int64_t first = seg ? seg[2 * s] : 0, len = seg ? seg[2 * s + 1] : n;
    const int b = seg ? blockIdx.x % blocks_per_seg : blockIdx.x;
    const int nb = seg ? blocks_per_seg : gridDim.x;
    // the segment's amax from its DG_FP8_AMAX_PARTS (= 256 = blockDim) partial maxima
    const float sc = dg_fp8_scale_of(fp8_block_amax(parts[(int64_t)s * DG_FP8_AMAX_PARTS + threadIdx.x], red), fp8_fmax<BF8>);
    if (b == 0 && threadIdx.x == 0 && scale_inv) scale_inv[s] = 1.f / sc;
    fp8_cast_span<T, BF8, false>(x + first, q + first, first, len, (int64_t)b * FP8_BLOCK + threadIdx.x, (int64_t)nb * FP8_BLOCK, sc);
}

// ---------------------------------------------------------------------------------------------
// Delayed scaling, ONE pass: q = cvt(clamp(x * FMAX / amax_prev)) with amax_prev = the maximum this call site saw one step ago,
// while the maximum of THIS tensor is recorded for the next step.  parts2 = [2][DG_FP8_AMAX_PARTS] floats owned by the call
// site: slot (step & 1) is written, slot ((step & 1) ^ 1) is read -- step is the device-side step word of the dropout / AdamW
// state (rng_state[2]), so a captured graph alternates the slots by itself and no block can read a value another block of the
// same launch is writing.  The caller seeds both slots with a just-in-time amax before the first use.  Saturating cast: a
// tensor that outgrows last step's range clips instead of overflowing.  Exactly DG_FP8_AMAX_PARTS workgroups of 1024.
template <typename T, bool BF8>
__global__ __launch_bounds__(FP8_DELAYED_BLOCK) void fp8_quantize_delayed_kernel(const T* __restrict__ x, uint8_t* __restrict__ q, int64_t n,
                                                                                 float* __restrict__ parts2, const uint32_t* __restrict__ step_word,
                                                                                 float* __restrict__ scale_inv) {
    __shared__ float red[FP8_DELAYED_BLOCK / 64];
    const DgFp8Slots slot = dg_fp8_slots(parts2, step_word, DG_FP8_AMAX_PARTS);
    const float am = fp8_block_amax(threadIdx.x < DG_FP8_AMAX_PARTS ? slot.prev[threadIdx.x] : 0.f, red);
    __syncthreads();                                   // red is used again below
    const float sc = dg_fp8_scale_of(am, fp8_fmax<BF8>);
    if (blockIdx.x == 0 && threadIdx.x == 0) scale_inv[0] = 1.f / sc;
    float m = fp8_cast_span<T, BF8, true>(x, q, 0, n, (int64_t)blockIdx.x * FP8_DELAYED_BLOCK + threadIdx.x,
                                          (int64_t)DG_FP8_AMAX_PARTS * FP8_DELAYED_BLOCK, sc);
    m = fp8_block_amax(m, red);
    if (threadIdx.x == 0) slot.next[blockIdx.x] = m;
}

// ---------------------------------------------------------------------------------------------
// The host side.  Every decision of a launch of the three entries, in one place: the entries launch what fp8_plan returns and
// dg_debug_fp8_plan reports it.  n_seg: the rows of the segment table, 0 without one.  A thread's units (vectors for the amax
// kernel) are `stride` apart: the workgroups that share a segment times the block.
enum { FP8_AMAX = 0, FP8_QUANTIZE, FP8_DELAYED };
static const char* const fp8_kernel_names[] = {"fp8_amax_kernel", "fp8_quantize_kernel", "fp8_quantize_delayed_kernel"};
struct Fp8Plan { int grid, block, blocks_per_seg, wgs_per_seg; int64_t stride; };
static Fp8Plan fp8_plan(int kind, int64_t n, int n_seg) {
    Fp8Plan pl;
    pl.block = kind == FP8_DELAYED ? FP8_DELAYED_BLOCK : FP8_BLOCK;
    pl.blocks_per_seg = 0;
    pl.wgs_per_seg = DG_FP8_AMAX_PARTS;
    pl.grid = (n_seg ? n_seg : 1) * DG_FP8_AMAX_PARTS;
    if (kind == FP8_QUANTIZE && n_seg) {               // sized by the mean segment: 32 elements per thread
        int64_t bps = (n / n_seg + FP8_BLOCK * 32 - 1) / (FP8_BLOCK * 32);
        pl.wgs_per_seg = pl.blocks_per_seg = (int)(bps < 1 ? 1 : (bps > 128 ? 128 : bps));
        pl.grid = pl.blocks_per_seg * n_seg;
    } else if (kind == FP8_QUANTIZE) {                 // four 8-element chunks per thread
        const int64_t g = (n / 8 + FP8_BLOCK * 4 - 1) / (FP8_BLOCK * 4);
        pl.wgs_per_seg = pl.grid = (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
    }
    pl.stride = (int64_t)pl.wgs_per_seg * pl.block;
    return pl;
}

// what the three entries refuse, in their order; `rest`: the entry's other pointers are all there.  The amax entry has no
// output, no format and takes any n.
static int fp8_check(int kind, const void* x, const void* q, bool rest, int64_t n, const int64_t* seg, int n_seg, int dtype, int fmt) {
    const bool casts = kind != FP8_AMAX;
    if (!x || !rest || n <= 0 || (seg && n_seg <= 0) || !dg_aligned16(x)) return DG_ERR_ARG;
    if (casts && (!q || n % 8 || (((uintptr_t)q) & 7))) return DG_ERR_ARG;
    if (!dg_is_float_dtype(dtype)) return DG_ERR_DTYPE;
    if (casts && fmt != DG_FP8_E4M3 && fmt != DG_FP8_E5M2) return DG_ERR_DTYPE;
    return DG_OK;
}

// dtype x format -> f(dg_type<T>, std::bool_constant<BF8>) (both codes checked by fp8_check)
template <typename F> static void fp8_with_types(int dtype, int fmt, F&& f) {
    dg_with_dtype(dtype, [&](auto t) {
        if (fmt == DG_FP8_E5M2) f(t, std::true_type{});
        else f(t, std::false_type{});
    });
}

extern "C" int dg_fp8_amax(const void* x, int dtype, int64_t n, const int64_t* seg, int n_seg, float* amax_parts, void* stream) {
    if (const int rc = fp8_check(FP8_AMAX, x, nullptr, amax_parts, n, seg, n_seg, dtype, 0)) return rc;
    const Fp8Plan pl = fp8_plan(FP8_AMAX, n, seg ? n_seg : 0);
    dg_with_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL(fp8_amax_kernel<T>, dim3(pl.grid), dim3(pl.block), 0, (hipStream_t)stream, (const T*)x, n, seg, amax_parts);
    });
    DG_LAUNCH_CHECK();
    return DG_OK;
}

extern "C" int dg_fp8_quantize(const void* x, int dtype, void* q, int fmt, int64_t n, const int64_t* seg, int n_seg,
                               const float* amax_parts, float* scale_inv, void* stream) {
    if (const int rc = fp8_check(FP8_QUANTIZE, x, q, amax_parts, n, seg, n_seg, dtype, fmt)) return rc;
    const Fp8Plan pl = fp8_plan(FP8_QUANTIZE, n, seg ? n_seg : 0);
    fp8_with_types(dtype, fmt, [&](auto t, auto bf8) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((fp8_quantize_kernel<T, decltype(bf8)::value>), dim3(pl.grid), dim3(pl.block), 0, (hipStream_t)stream, (const T*)x,
                           (uint8_t*)q, n, seg, seg ? n_seg : 1, amax_parts, scale_inv, pl.blocks_per_seg);
    });
    DG_LAUNCH_CHECK();
    return DG_OK;
}

extern "C" int dg_fp8_quantize_delayed(const void* x, int dtype, void* q, int fmt, int64_t n, float* parts2,
                                       const uint32_t* rng_state, float* scale_inv, void* stream) {
    if (const int rc = fp8_check(FP8_DELAYED, x, q, parts2 && rng_state && scale_inv, n, nullptr, 0, dtype, fmt)) return rc;
    const Fp8Plan pl = fp8_plan(FP8_DELAYED, n, 0);
    fp8_with_types(dtype, fmt, [&](auto t, auto bf8) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((fp8_quantize_delayed_kernel<T, decltype(bf8)::value>), dim3(pl.grid), dim3(pl.block), 0, (hipStream_t)stream,
                           (const T*)x, (uint8_t*)q, n, parts2, rng_state, scale_inv);
    });
    DG_LAUNCH_CHECK();
    return DG_OK;
}

// diagnostic only (tests/fp8_cases.py), pure host code, not part of the public header: the launch entry `kind` (FP8_AMAX /
// FP8_QUANTIZE / FP8_DELAYED) makes for a tensor of `n` elements of `dtype` at byte address x_addr, output at q_addr, with the
// HOST copy `seg` of its segment table (NULL: none), or the entry's refusal.  launch6: grid, block, blocks_per_seg, workgroups per
// segment, stride, segments.  rows: per segment {first, len, narrow terms (fp8_narrow_terms; 0 for amax), unit (elements: 16 / 8, the
// vector for amax), units, elements behind the last unit (amax: the scalar tail of workgroup 0), trips of the busiest thread, busy
// workgroups, idle workgroups}; as many as fit max_rows.
extern "C" int dg_debug_fp8_plan(int kind, int dtype, int64_t n, const int64_t* seg, int n_seg, uint64_t x_addr, uint64_t q_addr,
                                 int64_t* launch6, int64_t* rows, int max_rows, const char** kernel_name) {
    if (kind < FP8_AMAX || kind > FP8_DELAYED || !launch6 || (kind == FP8_DELAYED && seg)) return DG_ERR_ARG;
    if (const int rc = fp8_check(kind, (const void*)(uintptr_t)x_addr, (const void*)(uintptr_t)q_addr, true, n, seg, n_seg, dtype, DG_FP8_E4M3)) return rc;
    const Fp8Plan pl = fp8_plan(kind, n, seg ? n_seg : 0);
    const int ns = seg ? n_seg : 1, esz = dtype == DG_BF16 ? 2 : 4;
    launch6[0] = pl.grid; launch6[1] = pl.block; launch6[2] = pl.blocks_per_seg; launch6[3] = pl.wgs_per_seg; launch6[4] = pl.stride; launch6[5] = ns;
    if (kernel_name) *kernel_name = fp8_kernel_names[kind];
    for (int s = 0; rows && s < ns && s < max_rows; ++s) {
        const int64_t first = seg ? seg[2 * s] : 0, len = seg ? seg[2 * s + 1] : n;
        const int terms = kind == FP8_AMAX ? 0 : fp8_narrow_terms(first, len, (uintptr_t)x_addr + first * esz, (uintptr_t)q_addr + first);
        const int64_t unit = kind == FP8_AMAX ? 16 / esz : (terms ? 8 : 16), units = len / unit, tail = len - units * unit;
        int64_t busy = (units + pl.block - 1) / pl.block;          // workgroup b starts at unit b * block
        if (busy > pl.wgs_per_seg) busy = pl.wgs_per_seg;
        if (kind == FP8_AMAX && tail && busy < 1) busy = 1;
        int64_t* r = rows + 9 * s;
        r[0] = first; r[1] = len; r[2] = terms; r[3] = unit; r[4] = units; r[5] = tail;
        r[6] = (units + pl.stride - 1) / pl.stride; r[7] = busy; r[8] = pl.wgs_per_seg - busy;
    }
    return DG_OK;
}

// diagnostic only: the constants of the scale rule {FP8_E4M3_MAX, FP8_E5M2_MAX, DG_FP8_SCALE_CAP}, and the rule itself on the host
extern "C" void dg_debug_fp8_constants(float* out3) { out3[0] = FP8_E4M3_MAX; out3[1] = FP8_E5M2_MAX; out3[2] = DG_FP8_SCALE_CAP; }
extern "C" float dg_debug_fp8_scale(float amax, int fmt) { return dg_fp8_scale_of(amax, fmt == DG_FP8_E5M2 ? FP8_E5M2_MAX : FP8_E4M3_MAX); }
