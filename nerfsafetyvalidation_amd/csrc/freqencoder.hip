// freqencoder.hip -- the frequency (positional) encoding [x | sin(2^0 x) | cos(2^0 x) | sin(2^1 x) | cos(2^1 x) | ...] for gfx950.
// Line references are to the reference's freqencoder/src/freqencoder.cu.
//
// Layout as the reference (:28-58): outputs [B, C] row-major, C = D + 2 D deg, column D + (2 f + k) D + d holds sin (k = 0) or
// cos (k = 1) of 2^f x[b, d].  Values NOT as the reference: it writes the cosine as __sinf(2^f x + pi/2) (:55-56), which rounds the
// sum to float at arguments in the hundreds (4.8e-4 off at degree 16) on top of the fast sine's own error.  Here both come from the
// exact argument (freq_math.hpp: one range reduction per input value, one polynomial pair per frequency that feeds both columns).
//
// Shape.  A workgroup owns `rows` consecutive rows: rows * C contiguous floats of the output (the forward) or of the incoming gradient
// (the backward).  Its threads take the (row, dim) pairs -- an input value each, read as consecutive words -- and exchange the wide
// rows with global memory through LDS, so that consecutive lanes move consecutive words whatever C is; a thread per output element
// (:36-57) would evaluate every sine twice and a thread per row would store 4 bytes every 4 C.  The backward recomputes sin and cos
// from the inputs instead of reading saved outputs (:87): 4 (C + 2 D) bytes per row instead of 4 (2 C + D), and nothing of size C
// kept alive between the passes.  Its sum over f runs in ascending order in one thread: no atomics, the same bits on every run.
// Rows wider than the staging buffer (C > 5120: D in the hundreds) take the same code with the rows in global memory.
#include "ngp_common.hpp"
#include "freq_math.hpp"

namespace ngp {
namespace {

// 128 rows of C <= 40 words (D = 3: degree 6 has C = 39) in 20 KiB: eight workgroups, 32 waves, per CU.  Measured against 256 rows in
// 40 KiB (four workgroups: 15 % slower), 85 rows (a (row, dim) pair per thread, runs that start off a 16-byte boundary: 8 % slower) and
// 512 threads on 256 rows (5 % slower): DESIGN.md "Frequency encoder".
constexpr int kFreqBlock = 256;
constexpr uint32_t kFreqStageWords = 5120;
constexpr uint32_t kFreqMaxRows = 128;

// `words` consecutive floats between the staging buffer and global memory: 16 bytes per lane from the first 16-byte boundary of the
// global side on (a workgroup's run starts wherever first * C puts it), single words before it and for the last words % 4
__device__ __forceinline__ uint32_t freq_head(const float* global, uint32_t words) {
    const uint32_t head = (uint32_t)((0 - (uintptr_t)global) & 15) >> 2;
    return head < words ? head : words;
}
__device__ __forceinline__ void freq_store_rows(float* __restrict__ out, const float* stage, uint32_t words) {
    const uint32_t head = freq_head(out, words), quads = (words - head) / 4;
    if (threadIdx.x < head) out[threadIdx.x] = stage[threadIdx.x];
    for (uint32_t q = threadIdx.x; q < quads; q += kFreqBlock) {
        const uint32_t i = head + 4 * q;
        *reinterpret_cast<float4*>(out + i) = make_float4(stage[i], stage[i + 1], stage[i + 2], stage[i + 3]);
    }
    for (uint32_t w = head + 4 * quads + threadIdx.x; w < words; w += kFreqBlock) out[w] = stage[w];
}
__device__ __forceinline__ void freq_load_rows(float* stage, const float* __restrict__ g, uint32_t words) {
    const uint32_t head = freq_head(g, words), quads = (words - head) / 4;
    if (threadIdx.x < head) stage[threadIdx.x] = g[threadIdx.x];
    for (uint32_t q = threadIdx.x; q < quads; q += kFreqBlock) {
        const uint32_t i = head + 4 * q;
        const float4 v = *reinterpret_cast<const float4*>(g + i);
        stage[i] = v.x; stage[i + 1] = v.y; stage[i + 2] = v.z; stage[i + 3] = v.w;
    }
    for (uint32_t w = head + 4 * quads + threadIdx.x; w < words; w += kFreqBlock) stage[w] = g[w];
}

// sin, cos of 2^f x: f counts up by one per call, u carries 2^f x in quarter turns
__device__ __forceinline__ void freq_next(float x, bool fast, uint32_t f, double& u, float& s, float& c) {
    if (fast) {
        freq_sincos_quarter(u, s, c);
        u += u;
    } else {
        sincosf(ldexpf(x, (int)f), &s, &c);         // |x| > 1024, inf, nan: the library's reduction (Payne-Hanek), argument still exact
    }
}

struct FreqBlock {
    size_t first;           // first row
    uint32_t here;          // rows of this workgroup
};
__device__ __forceinline__ FreqBlock freq_block(uint32_t B, uint32_t rows) {
    FreqBlock k;
    k.first = (size_t)blockIdx.x * rows;            // (< B: the grid covers B)
    const size_t left = (size_t)B - k.first;
    k.here = left < rows ? (uint32_t)left : rows;
    return k;
}

template <bool STAGED>
__global__ void __launch_bounds__(kFreqBlock) k_freq_forward(const float* __restrict__ inputs, float* __restrict__ outputs, uint32_t B, uint32_t D,
                                                             uint32_t deg, uint32_t rows) {
    __shared__ float stage[STAGED ? kFreqStageWords : 1];
    const uint32_t C = D + 2 * D * deg;
    const FreqBlock k = freq_block(B, rows);
    const float* in = inputs + k.first * D;
    float* out = outputs + k.first * C;
    const uint32_t items = k.here * D;               // (<= rows * C <= kFreqStageWords when staged; D when not: rows = 1)
    for (uint32_t i = threadIdx.x; i < items; i += kFreqBlock) {
        const uint32_t r = i / D, d = i - r * D;
        const float x = in[i];
        float* o = (STAGED ? stage : out) + (size_t)r * C + d;
        *o = x;
        const bool fast = fabsf(x) <= kFreqFastMax;
        double u = freq_quarter_turns(x);
        for (uint32_t f = 0; f < deg; f++) {
            float s, c;
            freq_next(x, fast, f, u, s, c);
            o += D;
            *o = s;
            o += D;
            *o = c;
        }
    }
    if (STAGED) {
        __syncthreads();
        freq_store_rows(out, stage, k.here * C);
    }
}

template <bool STAGED>
__global__ void __launch_bounds__(kFreqBlock) k_freq_backward(const float* __restrict__ grad, const float* __restrict__ inputs, uint32_t B, uint32_t D,
                                                              uint32_t deg, uint32_t rows, float* __restrict__ grad_inputs) {
    __shared__ float stage[STAGED ? kFreqStageWords : 1];
    const uint32_t C = D + 2 * D * deg;
    const FreqBlock k = freq_block(B, rows);
    const float* in = inputs + k.first * D;
    const float* g = grad + k.first * C;
    float* gin = grad_inputs + k.first * D;
    if (STAGED) {
        freq_load_rows(stage, g, k.here * C);
        __syncthreads();
    }
    const uint32_t items = k.here * D;
    for (uint32_t i = threadIdx.x; i < items; i += kFreqBlock) {
        const uint32_t r = i / D, d = i - r * D;
        const float x = in[i];
        const float* gp = (STAGED ? (const float*)stage : g) + (size_t)r * C + d;
        float acc = *gp;
        const bool fast = fabsf(x) <= kFreqFastMax;
        double u = freq_quarter_turns(x);
        float scale = 1.0f;                          // 2^f
        for (uint32_t f = 0; f < deg; f++) {
            float s, c;
            freq_next(x, fast, f, u, s, c);
            gp += D;
            const float gs = *gp;
            gp += D;
            const float gc = *gp;
            acc = fmaf(scale, fmaf(gs, c, -(gc * s)), acc);       // d sin = cos, d cos = -sin, both times 2^f (:87)
            scale += scale;
        }
        gin[i] = acc;
    }
}

// rows per workgroup: 0 = the rows do not fit the staging buffer (one row per workgroup, no staging)
uint32_t freq_rows(uint32_t C) {
    if (C > kFreqStageWords) return 0;
    const uint32_t fit = kFreqStageWords / C;
    return fit < kFreqMaxRows ? fit : kFreqMaxRows;
}

constexpr uint32_t kFreqMaxGrid = 0x7FFFFFFFu;
uint32_t freq_grid(uint32_t B, uint32_t rows) { return rows ? (uint32_t)(((uint64_t)B + rows - 1) / rows) : B; }      // (B + rows - 1 may pass 2^32)

int freq_check(const char* what, uint32_t D, uint32_t deg) {
    NGP_REQUIRE(D >= 1, "%s: input dim must be at least 1", what);
    NGP_REQUIRE(deg <= kFreqMaxDegree, "%s: degree %u is above %u", what, deg, kFreqMaxDegree);
    NGP_REQUIRE((uint64_t)D * (1 + 2 * deg) <= 0x7FFFFFFFull, "%s: D (1 + 2 degree) must stay below 2^31", what);
    return NGP_OK;
}

}  // namespace
}  // namespace ngp

using namespace ngp;

extern "C" {

int ngp_freq_encode_forward(const float* inputs, float* outputs, uint32_t B, uint32_t D, uint32_t deg, ngp_stream_t stream) {
    if (int rc = freq_check("freq_encode_forward", D, deg)) return rc;
    if (B == 0) return NGP_OK;
    NGP_REQUIRE(inputs && outputs, "freq_encode_forward: null pointer");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("freq_encode_forward", s, B);
    const uint32_t rows = freq_rows(D + 2 * D * deg), grid = freq_grid(B, rows);
    NGP_REQUIRE(grid <= kFreqMaxGrid, "freq_encode_forward: too many rows (%u) for this width", B);
    if (rows) k_freq_forward<true><<<grid, kFreqBlock, 0, s>>>(inputs, outputs, B, D, deg, rows);
    else k_freq_forward<false><<<grid, kFreqBlock, 0, s>>>(inputs, outputs, B, D, deg, 1);
    return check_launch("freq_encode_forward");
}

int ngp_freq_encode_backward(const float* grad, const float* inputs, uint32_t B, uint32_t D, uint32_t deg, float* grad_inputs,
                             ngp_stream_t stream) {
    if (int rc = freq_check("freq_encode_backward", D, deg)) return rc;
    if (B == 0) return NGP_OK;
    NGP_REQUIRE(grad && inputs && grad_inputs, "freq_encode_backward: null pointer");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("freq_encode_backward", s, B);
    const uint32_t rows = freq_rows(D + 2 * D * deg), grid = freq_grid(B, rows);
    NGP_REQUIRE(grid <= kFreqMaxGrid, "freq_encode_backward: too many rows (%u) for this width", B);
    if (rows) k_freq_backward<true><<<grid, kFreqBlock, 0, s>>>(grad, inputs, B, D, deg, rows, grad_inputs);
    else k_freq_backward<false><<<grid, kFreqBlock, 0, s>>>(grad, inputs, B, D, deg, 1, grad_inputs);
    return check_launch("freq_encode_backward");
}

}  // extern "C"
