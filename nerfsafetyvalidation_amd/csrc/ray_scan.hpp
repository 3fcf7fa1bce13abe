// ray_scan.hpp -- what the per-ray loss kernels share (distortion.hip, depth_loss.hip): a row of the ray table, the input stage of one
// 64-sample chunk with its two prefix sums, and the chain from a gradient in the weights to one in sigma.  One WAVE per ray, lane l on
// sample base + l of a chunk; inside a chunk the prefixes are wave_ops.hpp's scans, between chunks the running values travel in
// registers.  No LDS, no atomics: a ray's sums are formed by its own wave in an order that depends on its sample count alone.
// The ORDER of every operation here decides output bits that tests pin (DESIGN.md "Cross-lane arithmetic").
#pragma once
#include "ngp_common.hpp"
#include "wave_ops.hpp"

namespace ngp {

constexpr int kRayBlock = 256;                      // four waves = four rays
constexpr float kStopT = 1e-4f;                     // composite_rays_train's early stop (raymarching.cu:560)
constexpr uint32_t kRayMaxRays = 0x3FFFFFFFu;       // 3 N and 4 N stay 32-bit

// The arrays of one call.  FROM_SIGMA: a = sigmas [M], b = deltas [M,2], c = scale per ray (indexed by the table's `index`; NULL = 1).
// Otherwise: a = w [M], b = m [M], c = interval [M] (NULL: the scalar cs for every sample).
struct RayIn {
    const float* a;
    const float* b;
    const float* c;
    float cs;
};

struct RayRun {                 // what a ray carries from one chunk to the next
    float T, t, W, WM;
    bool stopped;
};

struct RayChunk {               // lane l's sample of a chunk; a lane past the ray's live samples holds exact zeros in w, m, delta
    float w, m, delta, wm;
    float Wpre, WMpre;          // sums over the ray's samples before this one
    float dt, T_next;           // FROM_SIGMA only: the sample's dt and the transmittance behind it (T_{i+1})
    bool live;
};

// One chunk: the input stage, then the two prefix sums every caller needs.  `row` is the ray's first packed row, `scale` its factor.
// FROM_SIGMA forms T as the PRODUCT of the (1 - alpha), multiplied in the scan's tree order inside a chunk and onto the carried product
// between chunks (not exp of a summed optical depth); the ray stops behind the first sample whose T_{i+1} < 1e-4, that sample included.
template <bool FROM_SIGMA>
__device__ __forceinline__ RayChunk ray_chunk(const RayIn& in, size_t row, uint32_t base, uint32_t count, float scale, uint32_t lane, RayRun& run) {
    const uint32_t i = base + lane;
    const bool on = i < count;
    RayChunk q;
    if (FROM_SIGMA) {
        const float sg = on ? in.a[row + i] : 0.0f;
        const float2 d = on ? reinterpret_cast<const float2*>(in.b)[row + i] : make_float2(0.0f, 0.0f);
        const float alpha = 1.0f - expf(-sg * d.x);                  // (a lane that is off: exp(-0) = 1, alpha = 0)
        const float P = scan_inclusive<MulOp>(1.0f - alpha, lane);
        const float T_before = run.T * shifted_in(P, lane, 1.0f);
        q.T_next = run.T * P;
        const unsigned long long crossed = __ballot(on && q.T_next < kStopT);
        const uint32_t stop_lane = crossed ? (uint32_t)__ffsll((long long)crossed) - 1u : 64u;
        q.live = on && lane <= stop_lane;
        const float t = run.t + scan_inclusive<AddOp>(d.y, lane);
        q.w = q.live ? alpha * T_before : 0.0f;
        q.m = q.live ? scale * t : 0.0f;
        q.delta = q.live ? scale * d.x : 0.0f;
        q.dt = d.x;
        run.T = last_lane(q.T_next);
        run.t = last_lane(t);
        run.stopped = crossed != 0ull;
    } else {
        q.live = on;
        q.w = on ? in.a[row + i] : 0.0f;
        q.m = on ? in.b[row + i] : 0.0f;
        q.delta = on ? (in.c ? in.c[row + i] : in.cs) : 0.0f;
        q.dt = 0.0f;
        q.T_next = 0.0f;
    }
    q.wm = q.w * q.m;
    const float W = scan_inclusive<AddOp>(q.w, lane), WM = scan_inclusive<AddOp>(q.wm, lane);
    q.Wpre = run.W + shifted_in(W, lane, 0.0f);
    q.WMpre = run.WM + shifted_in(WM, lane, 0.0f);
    run.W += last_lane(W);
    run.WM += last_lane(WM);
    return q;
}

// A row of the table -> (index, first row, samples), or false when the ray takes no part: no samples, a slot outside the table, or
// rows the arrays do not hold.  The packed training layout keeps composite_rays_train's rule (offset + count >= M drops the ray,
// raymarching.cu:523); given arrays may end with their last ray's last sample.
template <bool FROM_SIGMA>
__device__ __forceinline__ bool ray_of(const int32_t* __restrict__ rays, uint32_t n, uint32_t M, uint32_t N, uint32_t& index, uint32_t& offset,
                                       uint32_t& count, bool& slot_ok) {
    index = (uint32_t)rays[n * 3];
    offset = (uint32_t)rays[n * 3 + 1];
    count = (uint32_t)rays[n * 3 + 2];
    slot_ok = index < N;
    const uint64_t end = (uint64_t)offset + count;
    return slot_ok && count != 0 && (FROM_SIGMA ? end < (uint64_t)M : end <= (uint64_t)M);
}

// The chain to sigma of one chunk: with g the gradient in this lane's weight, gw = g * w and S_total = sum over the ray's live samples of g_k w_k,
//   dL / dsigma_i = dt_i (g_i T_{i+1} - sum_{k>i} g_k w_k),
// the suffix sum formed as the total minus the prefix (S_run carries the prefix across chunks).  Exact for every live sample, the one
// that stops the ray included.
__device__ __forceinline__ float sigma_chain(const RayChunk& q, float g, float gw, float S_total, float& S_run, uint32_t lane) {
    const float S = scan_inclusive<AddOp>(gw, lane);
    const float S_after = S_total - (S_run + S);          // sum_{i>k} g_i w_i
    S_run += last_lane(S);
    return q.dt * (g * q.T_next - S_after);
}

}  // namespace ngp
