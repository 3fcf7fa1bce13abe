// distortion.hip -- the distortion regulariser (mip-NeRF 360, in the O(n) prefix-sum form) on a ray table, for gfx950.
//
//   L_ray = 2 sum_i w_i (m_i Wpre_i - WMpre_i) + (1/3) sum_i w_i^2 delta_i,     Wpre_i = sum_{j<i} w_j,  WMpre_i = sum_{j<i} w_j m_j
//   g_i   = dL_ray / dw_i = 2 (m_i (Wpre_i - Wsuf_i) + (WMsuf_i - WMpre_i)) + (2/3) delta_i w_i
//
// Two input stages feed ONE scan routine (ray_chunk): the packed training layout, where w comes from sigma and dt by the forward rule
// of composite_rays_train and m from the running sum of deltas[1]; and given per-sample w, m, interval.  Two output stages: the chain
// to sigma, or g itself.  DESIGN.md "Distortion regulariser" has the definitions.
//
// One WAVE per ray (four rays per 256-thread workgroup), lane l on sample base + l of a 64-sample chunk: the loads of a chunk are
// consecutive addresses.  Inside a chunk the prefixes are wave_ops.hpp's scans over the 64 lanes; between chunks the running values
// travel in registers.  Bandwidth- and latency-bound: no LDS, no matrix pipe.  No atomics: a ray's sums are formed by its own wave in an
// order that depends on its sample count alone, the mean over the rays by mean_of_rays, the fixed-order mean (DESIGN.md "Cross-lane
// arithmetic") -- two runs on the same inputs give the same bits, and so does any order of the table's rows.
#include "ngp_common.hpp"
#include "wave_ops.hpp"

namespace ngp {
namespace {

constexpr int kDistBlock = 256;                     // four waves = four rays
constexpr float kStopT = 1e-4f;                     // composite_rays_train's early stop (raymarching.cu:560)

// The arrays of one call.  FROM_SIGMA: a = sigmas [M], b = deltas [M,2], c = scale per ray (indexed by the table's `index`; NULL = 1).
// Otherwise: a = w [M], b = m [M], c = interval [M] (NULL: the scalar cs for every sample).
struct DistIn {
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
__device__ __forceinline__ RayChunk ray_chunk(const DistIn& in, size_t row, uint32_t base, uint32_t count, float scale, uint32_t lane, RayRun& run) {
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

__device__ __forceinline__ float weight_gradient(const RayChunk& q, float W_total, float WM_total) {
    const float Wsuf = W_total - (q.Wpre + q.w), WMsuf = WM_total - (q.WMpre + q.wm);
    return 2.0f * (q.m * (q.Wpre - Wsuf) + (WMsuf - q.WMpre)) + (2.0f / 3.0f) * q.delta * q.w;      // (0 on a dead lane only after `* w`)
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

template <bool FROM_SIGMA>
__global__ void __launch_bounds__(kDistBlock) k_distortion_fwd(DistIn in, const int32_t* __restrict__ rays, uint32_t M, uint32_t N,
                                                               float* __restrict__ loss_rays, float* __restrict__ totals) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t n = blockIdx.x * (kDistBlock / 64) + (threadIdx.x >> 6);      // one wave per ray
    if (n >= N) return;
    uint32_t index, offset, count;
    bool slot_ok;
    if (!ray_of<FROM_SIGMA>(rays, n, M, N, index, offset, count, slot_ok)) {
        if (slot_ok && lane == 0) { loss_rays[index] = 0.0f; totals[index * 2] = 0.0f; totals[index * 2 + 1] = 0.0f; }
        return;
    }
    const float scale = FROM_SIGMA && in.c ? in.c[index] : 1.0f;
    RayRun run = {1.0f, 0.0f, 0.0f, 0.0f, false};
    float acc = 0.0f;
    for (uint32_t base = 0; base < count && !run.stopped; base += 64) {
        const RayChunk q = ray_chunk<FROM_SIGMA>(in, offset, base, count, scale, lane, run);
        acc += 2.0f * q.w * (q.m * q.Wpre - q.WMpre) + (1.0f / 3.0f) * (q.w * q.w) * q.delta;
    }
    acc = wave_sum(acc);
    if (lane == 0) { loss_rays[index] = acc; totals[index * 2] = run.W; totals[index * 2 + 1] = run.WM; }
}

// FROM_SIGMA: grad[offset + k] = (*grad_loss / N) dt_k (g_k T_{k+1} - sum_{i>k} g_i w_i) for every live sample, the one that stops the
// ray included.  Otherwise grad[offset + k] = (*grad_loss / N) g_k.  Rows of dead samples and of rays that take no part are not written.
template <bool FROM_SIGMA>
__global__ void __launch_bounds__(kDistBlock) k_distortion_bwd(const float* __restrict__ grad_loss, DistIn in, const int32_t* __restrict__ rays,
                                                               const float* __restrict__ totals, uint32_t M, uint32_t N, float* __restrict__ grad) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t n = blockIdx.x * (kDistBlock / 64) + (threadIdx.x >> 6);
    if (n >= N) return;
    uint32_t index, offset, count;
    bool slot_ok;
    if (!ray_of<FROM_SIGMA>(rays, n, M, N, index, offset, count, slot_ok)) return;
    const float scale = FROM_SIGMA && in.c ? in.c[index] : 1.0f;
    const float W_total = totals[index * 2], WM_total = totals[index * 2 + 1];
    const float seed = *grad_loss, rays_f = (float)N;
    const RayRun start = {1.0f, 0.0f, 0.0f, 0.0f, false};
    float S_total = 0.0f;
    if (FROM_SIGMA && count > 64) {          // a first sweep for sum_i g_i w_i (a ray of one chunk forms it in the sweep below)
        RayRun run = start;
        float acc = 0.0f;
        for (uint32_t base = 0; base < count && !run.stopped; base += 64) {
            const RayChunk q = ray_chunk<true>(in, offset, base, count, scale, lane, run);
            acc += weight_gradient(q, W_total, WM_total) * q.w;
        }
        S_total = wave_sum(acc);
    }
    RayRun run = start;
    float S_run = 0.0f;
    for (uint32_t base = 0; base < count && !run.stopped; base += 64) {
        const RayChunk q = ray_chunk<FROM_SIGMA>(in, offset, base, count, scale, lane, run);
        const float g = weight_gradient(q, W_total, WM_total);
        if (FROM_SIGMA) {
            const float gw = g * q.w;
            if (count <= 64) S_total = wave_sum(gw);
            const float S = scan_inclusive<AddOp>(gw, lane);
            const float S_after = S_total - (S_run + S);          // sum_{i>k} g_i w_i
            S_run += last_lane(S);
            if (q.live) grad[(size_t)offset + base + lane] = (seed * (q.dt * (g * q.T_next - S_after))) / rays_f;
        } else {
            if (q.live) grad[(size_t)offset + base + lane] = (seed * g) / rays_f;
        }
    }
}

constexpr uint32_t kDistMaxRays = 0x3FFFFFFFu;      // 3 N and 4 N stay 32-bit

}  // namespace
}  // namespace ngp

using namespace ngp;

extern "C" {

size_t ngp_distortion_workspace(uint32_t N) { return mean_workspace(N); }

int ngp_distortion_train_forward(const float* sigmas, const float* deltas, const int32_t* rays, const float* scale, uint32_t M, uint32_t N,
                                 float* loss_rays, float* totals, float* loss, void* workspace, size_t workspace_bytes, ngp_stream_t stream) {
    if (N == 0) return NGP_OK;
    NGP_REQUIRE(sigmas && deltas && rays && loss_rays && totals && loss, "distortion_train_forward: null pointer");
    NGP_REQUIRE(N <= kDistMaxRays, "distortion_train_forward: too many rays");
    NGP_REQUIRE(((uintptr_t)deltas & 7) == 0, "distortion_train_forward: deltas must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("distortion_train_forward", s, M);
    const DistIn in = {sigmas, deltas, scale, 0.0f};
    k_distortion_fwd<true><<<div_up(N, kDistBlock / 64), kDistBlock, 0, s>>>(in, rays, M, N, loss_rays, totals);
    return mean_of_rays(loss_rays, N, loss, workspace, workspace_bytes, s, "distortion_train_forward");
}

int ngp_distortion_train_backward(const float* grad_loss, const float* sigmas, const float* deltas, const int32_t* rays, const float* scale,
                                  const float* totals, uint32_t M, uint32_t N, float* grad_sigmas, ngp_stream_t stream) {
    if (N == 0) return NGP_OK;
    NGP_REQUIRE(grad_loss && sigmas && deltas && rays && totals && grad_sigmas, "distortion_train_backward: null pointer");
    NGP_REQUIRE(N <= kDistMaxRays, "distortion_train_backward: too many rays");
    NGP_REQUIRE(((uintptr_t)deltas & 7) == 0, "distortion_train_backward: deltas must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("distortion_train_backward", s, M);
    const DistIn in = {sigmas, deltas, scale, 0.0f};
    k_distortion_bwd<true><<<div_up(N, kDistBlock / 64), kDistBlock, 0, s>>>(grad_loss, in, rays, totals, M, N, grad_sigmas);
    return check_launch("distortion_train_backward");
}

int ngp_distortion_forward(const float* w, const float* m, const float* interval, float interval_scalar, const int32_t* rays, uint32_t M,
                           uint32_t N, float* loss_rays, float* totals, float* loss, void* workspace, size_t workspace_bytes,
                           ngp_stream_t stream) {
    if (N == 0) return NGP_OK;
    NGP_REQUIRE(w && m && rays && loss_rays && totals && loss, "distortion_forward: null pointer");
    NGP_REQUIRE(N <= kDistMaxRays, "distortion_forward: too many rays");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("distortion_forward", s, M);
    const DistIn in = {w, m, interval, interval_scalar};
    k_distortion_fwd<false><<<div_up(N, kDistBlock / 64), kDistBlock, 0, s>>>(in, rays, M, N, loss_rays, totals);
    return mean_of_rays(loss_rays, N, loss, workspace, workspace_bytes, s, "distortion_forward");
}

int ngp_distortion_backward(const float* grad_loss, const float* w, const float* m, const float* interval, float interval_scalar,
                            const int32_t* rays, const float* totals, uint32_t M, uint32_t N, float* grad_w, ngp_stream_t stream) {
    if (N == 0) return NGP_OK;
    NGP_REQUIRE(grad_loss && w && m && rays && totals && grad_w, "distortion_backward: null pointer");
    NGP_REQUIRE(N <= kDistMaxRays, "distortion_backward: too many rays");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("distortion_backward", s, M);
    const DistIn in = {w, m, interval, interval_scalar};
    k_distortion_bwd<false><<<div_up(N, kDistBlock / 64), kDistBlock, 0, s>>>(grad_loss, in, rays, totals, M, N, grad_w);
    return check_launch("distortion_backward");
}

}  // extern "C"
