// Cross-lane arithmetic of libngp_hip's kernels (gfx950, wave64): the one definition of every reduction and scan over lanes.
// The ORDER of the additions decides output bits, and tests pin those bits: each function names its order, and that order is the
// function's contract (DESIGN.md "Cross-lane arithmetic").  A group is W consecutive lanes aligned to W; `l` is the lane's index
// within its group, of whichever integer type the caller holds it in.
#pragma once
#include "ngp_common.hpp"

namespace ngp {

struct AddOp { template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; } };
struct MulOp { template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a * b; } };

// Sum of a group, the same bits in every lane of it.  Order: xor butterfly, offsets W/2, W/4, .. 1.
template <int W = 64, typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = W / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, W);
    return v;
}
// Sum of the wave, complete in lane 0 ONLY (the step in front of a per-wave LDS slot).  Order: __shfl_down tree, offsets 32, 16, .. 1.
template <typename T>
__device__ __forceinline__ T wave_sum_lane0(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}
// Smallest value of a group, the same in every lane of it (integers, or floats without NaN: the order then decides nothing).
template <int W = 64, typename T>
__device__ __forceinline__ T wave_min(T v) {
#pragma unroll
    for (int off = W / 2; off > 0; off >>= 1) {
        const T u = __shfl_xor(v, off, W);
        v = u < v ? u : v;
    }
    return v;
}
// The four quads of sixteen lanes added up: lane l ends with lanes l % 16 + {0, 16, 32, 48}.  Order: xor 16, then xor 32.
template <typename T>
__device__ __forceinline__ T quad_sum(T v) {
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

// Inclusive scan of a group: lane l gets Op over lanes 0 .. l.  Order: Hillis-Steele over __shfl_up, offsets 1, 2, .. W/2.
template <class Op, int W = 64, typename T, typename L>
__device__ __forceinline__ T scan_inclusive(T v, L l) {
#pragma unroll
    for (int off = 1; off < W; off <<= 1) {
        const T u = __shfl_up(v, off, W);
        if (l >= (L)off) v = Op()(v, u);
    }
    return v;
}
// Its mirror: lane l gets Op over lanes l .. W - 1.  Order: Hillis-Steele over __shfl_down, offsets 1, 2, .. W/2.
template <class Op, int W = 64, typename T, typename L>
__device__ __forceinline__ T scan_suffix(T v, L l) {
#pragma unroll
    for (int off = 1; off < W; off <<= 1) {
        const T u = __shfl_down(v, off, W);
        if (l + (L)off < (L)W) v = Op()(v, u);
    }
    return v;
}
// Inclusive -> exclusive: the lower neighbour's value, `first` (the identity, or a carry) in lane 0 of the group.
template <int W = 64, typename T, typename L>
__device__ __forceinline__ T shifted_in(T inclusive, L l, T first) {
    const T u = __shfl_up(inclusive, 1, W);
    return l == 0 ? first : u;
}
// A group's last / first lane, to every lane of it: what a chunk of a scan (a suffix scan) carries into the next chunk.
template <int W = 64, typename T>
__device__ __forceinline__ T last_lane(T v) { return __shfl(v, W - 1, W); }
template <int W = 64, typename T>
__device__ __forceinline__ T first_lane(T v) { return __shfl(v, 0, W); }

// ---- the fixed-order mean of N floats (DESIGN.md "Cross-lane arithmetic"): its order is a function of N alone.  value(i) is element
// i for i < N and +0 beyond.  (1) the 64 elements of a group by wave_sum, in float; (2) lane l of ONE wave adds the groups l, l + 64,
// ... in double, in that order; (3) wave_sum over those 64 doubles; (4) / N in double, rounded to float.
__device__ __forceinline__ void final_mean(const float* groups, uint32_t n_groups, uint32_t N, float* mean) {      // one whole wave
    const uint32_t lane = threadIdx.x & 63;
    double acc = 0.0;
    for (uint32_t g = lane; g < n_groups; g += 64) acc += (double)groups[g];
    acc = wave_sum(acc);
    if (lane == 0) *mean = (float)(acc / (double)N);
}
// N <= kMeanOneBlockRays: one workgroup of kMeanOneBlockThreads forms the whole mean.
template <class F>
__device__ __forceinline__ void mean_one_block(F value, uint32_t N, float* mean) {
    __shared__ float s_groups[kMeanOneBlockRays / 64];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t rounds = (N + kMeanOneBlockThreads - 1) / kMeanOneBlockThreads;
    for (uint32_t r = 0; r < rounds; r++) {
        const float v = wave_sum(value(r * kMeanOneBlockThreads + threadIdx.x));
        if (lane == 0) s_groups[r * (kMeanOneBlockThreads / 64) + wave] = v;
    }
    __syncthreads();
    if (wave == 0) final_mean(s_groups, (N + 63) / 64, N, mean);
}
// Above: workgroups of kMeanGroupThreads write step (1) to groups[(N + 63) / 64]; mean_of_groups (ngp_common.hpp) finishes.
template <class F>
__device__ __forceinline__ void mean_groups(F value, uint32_t N, float* groups) {
    const uint32_t i = blockIdx.x * kMeanGroupThreads + threadIdx.x;
    const float v = wave_sum(value(i));
    if ((threadIdx.x & 63) == 0 && (i >> 6) < (N + 63) / 64) groups[i >> 6] = v;
}

}  // namespace ngp
