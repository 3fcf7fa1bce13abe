// distortion.hip -- the distortion regulariser (mip-NeRF 360, in the O(n) prefix-sum form) on a ray table, for gfx950.
//
//   L_ray = 2 sum_i w_i (m_i Wpre_i - WMpre_i) + (1/3) sum_i w_i^2 delta_i,     Wpre_i = sum_{j<i} w_j,  WMpre_i = sum_{j<i} w_j m_j
//   g_i   = dL_ray / dw_i = 2 (m_i (Wpre_i - Wsuf_i) + (WMsuf_i - WMpre_i)) + (2/3) delta_i w_i
//
// Two input stages feed ONE scan routine (ray_chunk): the packed training layout, where w comes from sigma and dt by the forward rule
// of composite_rays_train and m from the running sum of deltas[1]; and given per-sample w, m, interval.  Two output stages: the chain
// to sigma, or g itself.  DESIGN.md "Distortion regulariser" has the definitions.  The input stage, the table's row rule and the
// sigma chain live in ray_scan.hpp, which depth_loss.hip includes too.
//
// One WAVE per ray (four rays per 256-thread workgroup), lane l on sample base + l of a 64-sample chunk: the loads of a chunk are
// consecutive addresses.  Inside a chunk the prefixes are wave_ops.hpp's scans over the 64 lanes; between chunks the running values
// travel in registers.  Bandwidth- and latency-bound: no LDS, no matrix pipe.  No atomics: a ray's sums are formed by its own wave in an
// order that depends on its sample count alone, the mean over the rays by mean_of_rays, the fixed-order mean (DESIGN.md "Cross-lane
// arithmetic") -- two runs on the same inputs give the same bits, and so does any order of the table's rows.
#include "ray_scan.hpp"

namespace ngp {
namespace {

__device__ __forceinline__ float weight_gradient(const RayChunk& q, float W_total, float WM_total) {
    const float Wsuf = W_total - (q.Wpre + q.w), WMsuf = WM_total - (q.WMpre + q.wm);
    return 2.0f * (q.m * (q.Wpre - Wsuf) + (WMsuf - q.WMpre)) + (2.0f / 3.0f) * q.delta * q.w;      // (0 on a dead lane only after `* w`)
}

template <bool FROM_SIGMA>
__global__ void __launch_bounds__(kRayBlock) k_distortion_fwd(RayIn in, const int32_t* __restrict__ rays, uint32_t M, uint32_t N,
                                                               float* __restrict__ loss_rays, float* __restrict__ totals) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t n = blockIdx.x * (kRayBlock / 64) + (threadIdx.x >> 6);      // one wave per ray
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
__global__ void __launch_bounds__(kRayBlock) k_distortion_bwd(const float* __restrict__ grad_loss, RayIn in, const int32_t* __restrict__ rays,
                                                               const float* __restrict__ totals, uint32_t M, uint32_t N, float* __restrict__ grad) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t n = blockIdx.x * (kRayBlock / 64) + (threadIdx.x >> 6);
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
            const float chain = sigma_chain(q, g, gw, S_total, S_run, lane);
            if (q.live) grad[(size_t)offset + base + lane] = (seed * chain) / rays_f;
        } else {
            if (q.live) grad[(size_t)offset + base + lane] = (seed * g) / rays_f;
        }
    }
}

}  // namespace
}  // namespace ngp

using namespace ngp;

extern "C" {

size_t ngp_distortion_workspace(uint32_t N) { return mean_workspace(N); }

int ngp_distortion_train_forward(const float* sigmas, const float* deltas, const int32_t* rays, const float* scale, uint32_t M, uint32_t N,
                                 float* loss_rays, float* totals, float* loss, void* workspace, size_t workspace_bytes, ngp_stream_t stream) {
    if (N == 0) return NGP_OK;
    NGP_REQUIRE(sigmas && deltas && rays && loss_rays && totals && loss, "distortion_train_forward: null pointer");
    NGP_REQUIRE(N <= kRayMaxRays, "distortion_train_forward: too many rays");
    NGP_REQUIRE(((uintptr_t)deltas & 7) == 0, "distortion_train_forward: deltas must be 8-byte aligned");
    int rc = check_workspace("distortion_train_forward", workspace, workspace_bytes, mean_workspace(N), alignof(float));      // before anything is launched
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("distortion_train_forward", s, M);
    const RayIn in = {sigmas, deltas, scale, 0.0f};
    k_distortion_fwd<true><<<div_up(N, kRayBlock / 64), kRayBlock, 0, s>>>(in, rays, M, N, loss_rays, totals);
    return mean_of_rays(loss_rays, N, loss, workspace, workspace_bytes, s, "distortion_train_forward");
}

int ngp_distortion_train_backward(const float* grad_loss, const float* sigmas, const float* deltas, const int32_t* rays, const float* scale,
                                  const float* totals, uint32_t M, uint32_t N, float* grad_sigmas, ngp_stream_t stream) {
    if (N == 0) return NGP_OK;
    NGP_REQUIRE(grad_loss && sigmas && deltas && rays && totals && grad_sigmas, "distortion_train_backward: null pointer");
    NGP_REQUIRE(N <= kRayMaxRays, "distortion_train_backward: too many rays");
    NGP_REQUIRE(((uintptr_t)deltas & 7) == 0, "distortion_train_backward: deltas must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("distortion_train_backward", s, M);
    const RayIn in = {sigmas, deltas, scale, 0.0f};
    k_distortion_bwd<true><<<div_up(N, kRayBlock / 64), kRayBlock, 0, s>>>(grad_loss, in, rays, totals, M, N, grad_sigmas);
    return check_launch("distortion_train_backward");
}

int ngp_distortion_forward(const float* w, const float* m, const float* interval, float interval_scalar, const int32_t* rays, uint32_t M,
                           uint32_t N, float* loss_rays, float* totals, float* loss, void* workspace, size_t workspace_bytes,
                           ngp_stream_t stream) {
    if (N == 0) return NGP_OK;
    NGP_REQUIRE(w && m && rays && loss_rays && totals && loss, "distortion_forward: null pointer");
    NGP_REQUIRE(N <= kRayMaxRays, "distortion_forward: too many rays");
    int rc = check_workspace("distortion_forward", workspace, workspace_bytes, mean_workspace(N), alignof(float));      // before anything is launched
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("distortion_forward", s, M);
    const RayIn in = {w, m, interval, interval_scalar};
    k_distortion_fwd<false><<<div_up(N, kRayBlock / 64), kRayBlock, 0, s>>>(in, rays, M, N, loss_rays, totals);
    return mean_of_rays(loss_rays, N, loss, workspace, workspace_bytes, s, "distortion_forward");
}

int ngp_distortion_backward(const float* grad_loss, const float* w, const float* m, const float* interval, float interval_scalar,
                            const int32_t* rays, const float* totals, uint32_t M, uint32_t N, float* grad_w, ngp_stream_t stream) {
    if (N == 0) return NGP_OK;
    NGP_REQUIRE(grad_loss && w && m && rays && totals && grad_w, "distortion_backward: null pointer");
    NGP_REQUIRE(N <= kRayMaxRays, "distortion_backward: too many rays");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("distortion_backward", s, M);
    const RayIn in = {w, m, interval, interval_scalar};
    k_distortion_bwd<false><<<div_up(N, kRayBlock / 64), kRayBlock, 0, s>>>(grad_loss, in, rays, totals, M, N, grad_w);
    return check_launch("distortion_backward");
}

}  // extern "C"
