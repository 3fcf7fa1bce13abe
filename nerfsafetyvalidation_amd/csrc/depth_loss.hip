// depth_loss.hip -- depth supervision on a ray table, for gfx950 (DESIGN.md "Depth supervision"; include/ngp_hip.h has the definitions).
//
//   z = target[index]:   z == 0, NaN or negative   no measurement: L_ray = 0, no gradient
//                        0 < z < +inf              a surface at z:  d = sum_live w_i t_i,  A = sum_{live, t_i < z - margin} w_i,
//                                                  L_ray = a (scale (d - z))^2 + b A
//                        z == +inf                 known empty ray: A = sum_live w_i,  L_ray = b A
//   g_i = dL_ray / dw_i = 2 a scale^2 (d - z) t_i + b [t_i < z - margin]
//
// The shape is distortion.hip's, and the input stage (ray_chunk), the table's row rule (ray_of) and the chain to sigma (sigma_chain)
// are the SAME code, ray_scan.hpp: one wave per ray, lane l on sample base + l of a 64-sample chunk, prefixes by wave scans, running
// values in registers between chunks.  No LDS, no atomics; the mean over the slots is the fixed-order mean.  Two runs on the same
// inputs, and any order of the table's rows, give the same bits.  The chunk is formed with scale 1, so that its m is t and its running
// sum of w m is d; the ray's scale enters the loss's coefficient alone.
#include "ray_scan.hpp"

namespace ngp {
namespace {

struct DepthArgs {
    const float* target;        // [N], read at `index`
    const float* scale;         // [N] or NULL = 1, read at `index`
    float margin, a, b;
};

// The ray's target -> does it take part, is it the known-empty case, and the threshold the front set is cut at (+inf: every sample).
__device__ __forceinline__ bool depth_target(float z, float margin, bool& empty, float& front_end) {
    if (!(z > 0.0f)) return false;                  // 0, negative, NaN
    empty = z == __builtin_inff();
    front_end = z - margin;                         // (+inf stays +inf)
    return true;
}

template <bool FROM_SIGMA>
__global__ void __launch_bounds__(kRayBlock) k_depth_loss_fwd(RayIn in, DepthArgs args, const int32_t* __restrict__ rays, uint32_t M, uint32_t N,
                                                              float* __restrict__ loss_rays, float* __restrict__ parts) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t n = blockIdx.x * (kRayBlock / 64) + (threadIdx.x >> 6);      // one wave per ray
    if (n >= N) return;
    uint32_t index, offset, count;
    bool slot_ok, empty = false;
    float front_end = 0.0f;
    const bool takes_part = ray_of<FROM_SIGMA>(rays, n, M, N, index, offset, count, slot_ok);
    if (!slot_ok) return;                                                        // (target and scale are read at a valid index only)
    const float z = args.target[index];
    if (!takes_part || !depth_target(z, args.margin, empty, front_end)) {
        if (lane == 0) { loss_rays[index] = 0.0f; parts[index * 2] = 0.0f; parts[index * 2 + 1] = 0.0f; }
        return;
    }
    const float scale = args.scale ? args.scale[index] : 1.0f;
    RayRun run = {1.0f, 0.0f, 0.0f, 0.0f, false};
    float front = 0.0f;
    for (uint32_t base = 0; base < count && !run.stopped; base += 64) {
        const RayChunk q = ray_chunk<FROM_SIGMA>(in, offset, base, count, 1.0f, lane, run);
        front += q.live && q.m < front_end ? q.w : 0.0f;
    }
    const float A = wave_sum(front), d = run.WM;
    const float miss = empty ? 0.0f : scale * (d - z);
    if (lane == 0) {
        loss_rays[index] = args.a * (miss * miss) + args.b * A;
        parts[index * 2] = d;
        parts[index * 2 + 1] = A;
    }
}

// FROM_SIGMA: grad[offset + k] = (*grad_loss / N) dt_k (g_k T_{k+1} - sum_{i>k} g_i w_i) for every live sample, the one that stops the
// ray included; the sum over all live samples is 2 a scale^2 (d - z) d + b A, from the forward's parts.  Otherwise
// grad[offset + k] = (*grad_loss / N) g_k.  Rows of dead samples and of rays that take no part are not written.
template <bool FROM_SIGMA>
__global__ void __launch_bounds__(kRayBlock) k_depth_loss_bwd(const float* __restrict__ grad_loss, RayIn in, DepthArgs args,
                                                              const int32_t* __restrict__ rays, const float* __restrict__ parts, uint32_t M,
                                                              uint32_t N, float* __restrict__ grad) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t n = blockIdx.x * (kRayBlock / 64) + (threadIdx.x >> 6);
    if (n >= N) return;
    uint32_t index, offset, count;
    bool slot_ok, empty = false;
    float front_end = 0.0f;
    if (!ray_of<FROM_SIGMA>(rays, n, M, N, index, offset, count, slot_ok)) return;
    const float z = args.target[index];
    if (!depth_target(z, args.margin, empty, front_end)) return;
    const float scale = args.scale ? args.scale[index] : 1.0f;
    const float d = parts[index * 2], A = parts[index * 2 + 1];
    const float pull = empty ? 0.0f : 2.0f * args.a * (scale * scale) * (d - z);
    const float S_total = pull * d + args.b * A;
    const float seed = *grad_loss, rays_f = (float)N;
    RayRun run = {1.0f, 0.0f, 0.0f, 0.0f, false};
    float S_run = 0.0f;
    for (uint32_t base = 0; base < count && !run.stopped; base += 64) {
        const RayChunk q = ray_chunk<FROM_SIGMA>(in, offset, base, count, 1.0f, lane, run);
        const float g = pull * q.m + (q.m < front_end ? args.b : 0.0f);
        if (FROM_SIGMA) {
            const float chain = sigma_chain(q, g, g * q.w, S_total, S_run, lane);
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

size_t ngp_depth_loss_workspace(uint32_t N) { return mean_workspace(N); }

int ngp_depth_loss_train_forward(const float* sigmas, const float* deltas, const int32_t* rays, const float* target, const float* scale,
                                 float margin, float weight_depth, float weight_free, uint32_t M, uint32_t N, float* loss_rays, float* parts,
                                 float* loss, void* workspace, size_t workspace_bytes, ngp_stream_t stream) {
    if (N == 0) return NGP_OK;
    NGP_REQUIRE(sigmas && deltas && rays && target && loss_rays && parts && loss, "depth_loss_train_forward: null pointer");
    NGP_REQUIRE(N <= kRayMaxRays, "depth_loss_train_forward: too many rays");
    NGP_REQUIRE(((uintptr_t)deltas & 7) == 0, "depth_loss_train_forward: deltas must be 8-byte aligned");
    int rc = check_workspace("depth_loss_train_forward", workspace, workspace_bytes, mean_workspace(N), alignof(float));      // before anything is launched
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("depth_loss_train_forward", s, M);
    const RayIn in = {sigmas, deltas, nullptr, 0.0f};
    const DepthArgs args = {target, scale, margin, weight_depth, weight_free};
    k_depth_loss_fwd<true><<<div_up(N, kRayBlock / 64), kRayBlock, 0, s>>>(in, args, rays, M, N, loss_rays, parts);
    return mean_of_rays(loss_rays, N, loss, workspace, workspace_bytes, s, "depth_loss_train_forward");
}

int ngp_depth_loss_train_backward(const float* grad_loss, const float* sigmas, const float* deltas, const int32_t* rays, const float* target,
                                  const float* scale, float margin, float weight_depth, float weight_free, const float* parts, uint32_t M,
                                  uint32_t N, float* grad_sigmas, ngp_stream_t stream) {
    if (N == 0) return NGP_OK;
    NGP_REQUIRE(grad_loss && sigmas && deltas && rays && target && parts && grad_sigmas, "depth_loss_train_backward: null pointer");
    NGP_REQUIRE(N <= kRayMaxRays, "depth_loss_train_backward: too many rays");
    NGP_REQUIRE(((uintptr_t)deltas & 7) == 0, "depth_loss_train_backward: deltas must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("depth_loss_train_backward", s, M);
    const RayIn in = {sigmas, deltas, nullptr, 0.0f};
    const DepthArgs args = {target, scale, margin, weight_depth, weight_free};
    k_depth_loss_bwd<true><<<div_up(N, kRayBlock / 64), kRayBlock, 0, s>>>(grad_loss, in, args, rays, parts, M, N, grad_sigmas);
    return check_launch("depth_loss_train_backward");
}

int ngp_depth_loss_forward(const float* w, const float* t, const int32_t* rays, const float* target, const float* scale, float margin,
                           float weight_depth, float weight_free, uint32_t M, uint32_t N, float* loss_rays, float* parts, float* loss,
                           void* workspace, size_t workspace_bytes, ngp_stream_t stream) {
    if (N == 0) return NGP_OK;
    NGP_REQUIRE(w && t && rays && target && loss_rays && parts && loss, "depth_loss_forward: null pointer");
    NGP_REQUIRE(N <= kRayMaxRays, "depth_loss_forward: too many rays");
    int rc = check_workspace("depth_loss_forward", workspace, workspace_bytes, mean_workspace(N), alignof(float));      // before anything is launched
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("depth_loss_forward", s, M);
    const RayIn in = {w, t, nullptr, 0.0f};
    const DepthArgs args = {target, scale, margin, weight_depth, weight_free};
    k_depth_loss_fwd<false><<<div_up(N, kRayBlock / 64), kRayBlock, 0, s>>>(in, args, rays, M, N, loss_rays, parts);
    return mean_of_rays(loss_rays, N, loss, workspace, workspace_bytes, s, "depth_loss_forward");
}

int ngp_depth_loss_backward(const float* grad_loss, const float* w, const float* t, const int32_t* rays, const float* target,
                            const float* scale, float margin, float weight_depth, float weight_free, const float* parts, uint32_t M, uint32_t N,
                            float* grad_w, ngp_stream_t stream) {
    if (N == 0) return NGP_OK;
    NGP_REQUIRE(grad_loss && w && t && rays && target && parts && grad_w, "depth_loss_backward: null pointer");
    NGP_REQUIRE(N <= kRayMaxRays, "depth_loss_backward: too many rays");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("depth_loss_backward", s, M);
    const RayIn in = {w, t, nullptr, 0.0f};
    const DepthArgs args = {target, scale, margin, weight_depth, weight_free};
    k_depth_loss_bwd<false><<<div_up(N, kRayBlock / 64), kRayBlock, 0, s>>>(grad_loss, in, args, rays, parts, M, N, grad_w);
    return check_launch("depth_loss_backward");
}

}  // extern "C"
