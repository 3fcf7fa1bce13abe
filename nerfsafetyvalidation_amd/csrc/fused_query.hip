// fused_query.hip -- the network on explicit points rather than along rays: NeRFNetwork.forward / .density on a point list
// (nerf/network_ff.py:51-90) and the density's gradient with respect to the points, the collision map's per-cell maximum density
// (collision.py, occupancy_from_density), and the trajectory planner's collision term with its backward (nav/quad_plot.py:216-249).
// Every kernel is a template over the network policy of fused_net.hpp and is instantiated here only.
#include "fused_net.hpp"
#include "wave_ops.hpp"

namespace ngp {

// ------------------------------------------------------------------------------------------
// NeRFNetwork.forward on an explicit point list (network_ff.py:51-75)
// ------------------------------------------------------------------------------------------
template <class NET>
__global__ void __launch_bounds__(256) k_network_forward(NetArgs na, GridLevels lv, const float* __restrict__ xyzs,
                                                         const float* __restrict__ dirs, uint32_t M, float* __restrict__ sigmas,
                                                         float* __restrict__ rgbs) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const char* Wlds = smem;
    LevelTab* lt = reinterpret_cast<LevelTab*>(smem + NET::w_bytes(na));
    stage_block(na, lv, smem, lt, NET::w_bytes(na));
    const uint32_t lane = threadIdx.x & 63, c = lane & 15;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    const uint32_t n_tiles = (M + 15) / 16;
    for (uint32_t tile = wave; tile < n_tiles; tile += n_waves) {
        const uint32_t m = tile * 16 + c;
        const uint32_t mm = m < M ? m : M - 1;
        float sg, r, g, b;
        typename NET::geo_t s16[4];
        NET::density(na, Wlds, *lt, lane, xyzs[(size_t)mm * 3], xyzs[(size_t)mm * 3 + 1], xyzs[(size_t)mm * 3 + 2], sg, s16);
        NET::color(na, Wlds, lane, dirs[(size_t)mm * 3], dirs[(size_t)mm * 3 + 1], dirs[(size_t)mm * 3 + 2], s16, r, g, b);
        if (lane < 16 && m < M) {
            sigmas[m] = sg;
            rgbs[(size_t)m * 3] = r;
            rgbs[(size_t)m * 3 + 1] = g;
            rgbs[(size_t)m * 3 + 2] = b;
        }
    }
}

// the density half alone (NeRFNetwork.density, network_ff.py:77-90): what the density-grid maintenance queries (renderer.py:487,526)
// geo (optional, [M, 15] f32): the geometry features = the sigma net's outputs 1..15 (what density() returns next to sigma)
template <class NET>
__global__ void __launch_bounds__(256) k_network_density(NetArgs na, GridLevels lv, const float* __restrict__ xyzs, uint32_t M,
                                                         float* __restrict__ sigmas, float* __restrict__ geo) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const char* Wlds = smem;
    LevelTab* lt = reinterpret_cast<LevelTab*>(smem + NET::w_bytes(na));
    stage_block(na, lv, smem, lt, NET::w_bytes(na));
    const uint32_t lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    const uint32_t n_tiles = (M + 15) / 16;
    for (uint32_t tile = wave; tile < n_tiles; tile += n_waves) {
        const uint32_t m = tile * 16 + c;
        const uint32_t mm = m < M ? m : M - 1;
        float sg;
        typename NET::geo_t s16[4];
        NET::density(na, Wlds, *lt, lane, xyzs[(size_t)mm * 3], xyzs[(size_t)mm * 3 + 1], xyzs[(size_t)mm * 3 + 2], sg, s16);
        if (lane < 16 && m < M) sigmas[m] = sg;
        if (geo && m < M) {
#pragma unroll
            for (int r = 0; r < 4; r++)
                if (4 * q + r > 0) geo[(size_t)m * 15 + 4 * q + r - 1] = (float)s16[r];
        }
    }
}

// The collision map's density (collision.py, occupancy_from_density): for cell (i, j, k) of an X x Y x Z box the s^3 sub-sample points
// p = start + (cell + (sub + 0.5) / s) / granularity (fp32, IEEE division, no contraction), in the NeRF's axes x = p @ rot as
// plan_point forms them, through the density half -> out[i, j, k] = the largest raw sigma.  Each lane of a 16-point tile owns one
// cell and walks its sub-samples with a running max: no cross-lane reduction, no atomics, and every sigma is the one
// k_network_density computes for the same fp32 point.
struct CellArgs {
    float start[3];
    float granularity;
    float rot[9];
    uint32_t X, Y, Z, s;
};

__device__ __forceinline__ float cell_coord(float start, uint32_t cell, uint32_t sub, float s, float g) {
    return start + ((float)cell + ((float)sub + 0.5f) / s) / g;
}

template <class NET>
__global__ void __launch_bounds__(256) k_cell_max_density(NetArgs na, GridLevels lv, CellArgs ca, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const char* Wlds = smem;
    LevelTab* lt = reinterpret_cast<LevelTab*>(smem + NET::w_bytes(na));
    stage_block(na, lv, smem, lt, NET::w_bytes(na));
    const uint32_t lane = threadIdx.x & 63, c = lane & 15;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    const uint32_t M = ca.X * ca.Y * ca.Z;
    const uint32_t n_tiles = (M + 15) / 16;
    const float fs = (float)ca.s;
    for (uint32_t tile = wave; tile < n_tiles; tile += n_waves) {
        const uint32_t m = tile * 16 + c;
        const uint32_t mm = m < M ? m : M - 1;
        const uint32_t k = mm % ca.Z, j = (mm / ca.Z) % ca.Y, i = mm / (ca.Z * ca.Y);
        float mx = 0.0f;
        for (uint32_t a = 0; a < ca.s; a++) {
            const float w0 = cell_coord(ca.start[0], i, a, fs, ca.granularity);
            for (uint32_t b = 0; b < ca.s; b++) {
                const float w1 = cell_coord(ca.start[1], j, b, fs, ca.granularity);
                for (uint32_t e = 0; e < ca.s; e++) {
                    const float w2 = cell_coord(ca.start[2], k, e, fs, ca.granularity);
                    float x[3];
#pragma unroll
                    for (int d = 0; d < 3; d++) x[d] = w0 * ca.rot[d] + w1 * ca.rot[3 + d] + w2 * ca.rot[6 + d];
                    float sg;
                    typename NET::geo_t s16[4];
                    NET::density(na, Wlds, *lt, lane, x[0], x[1], x[2], sg, s16);
                    mx = (a | b | e) == 0 ? sg : fmaxf(mx, sg);
                }
            }
        }
        if (lane < 16 && m < M) out[m] = mx;
    }
}

// Vector-Jacobian product of the density half with respect to the POINTS, map frozen: what the trajectory planner differentiates
// (nav/quad_plot.py:223-249: density_fn on S x 500 body points, 250 Adam steps per simulator step).  Upstream gradients of sigma [M]
// and (optional) of the geometry features [M, 15] -> grad_xyzs [M, 3].  One pass: forward with kept activations, trunc_exp backward
// (activation.py:12-17), the transposed sigma net, the hash grid's input derivative, d u / d x = 1 / (2 bound).
template <class NET>
__global__ void __launch_bounds__(256) k_network_density_bwd(NetArgs na, GridLevels lv, const char* __restrict__ packed_bwd,
                                                             const float* __restrict__ xyzs, uint32_t M, const float* __restrict__ g_sigma,
                                                             const float* __restrict__ g_geo, float* __restrict__ grad_xyzs) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const size_t w_bytes = NET::w_bytes(na);
    const size_t ws_bytes = NET::kF32 ? (size_t)bwd_floats(na.sig_mm) * 4 : (size_t)bwd_halfs(na.sig_mm) * 2;   // the sigma net's transposed fragments only
    const char* Wlds = smem;
    char* Wb = smem + w_bytes;
    LevelTab* lt = reinterpret_cast<LevelTab*>(smem + w_bytes + ws_bytes);
    {
        const uint4* src = reinterpret_cast<const uint4*>(packed_bwd);
        uint4* dst = reinterpret_cast<uint4*>(Wb);
        for (uint32_t i = threadIdx.x; i < ws_bytes / 16; i += blockDim.x) dst[i] = src[i];
    }
    stage_block(na, lv, smem, lt, w_bytes);
    const uint32_t lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    const uint32_t n_tiles = (M + 15) / 16;
    for (uint32_t tile = wave; tile < n_tiles; tile += n_waves) {
        const uint32_t m = tile * 16 + c;
        const bool valid = m < M;
        const uint32_t mm = valid ? m : M - 1;
        typename NET::Tape tape;
        typename NET::geo_t s16[4];
        NET::density_tape(na, Wlds, *lt, lane, xyzs[(size_t)mm * 3], xyzs[(size_t)mm * 3 + 1], xyzs[(size_t)mm * 3 + 2], tape, s16);
        f32x4 gso = {0, 0, 0, 0};
        if (valid) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const uint32_t o = 4 * q + r;
                if (o == 0) gso[r] = g_sigma ? g_sigma[m] * expf(fminf(15.0f, fmaxf(-15.0f, (float)s16[0]))) : 0.0f;
                else gso[r] = g_geo ? g_geo[(size_t)m * 15 + o - 1] : 0.0f;
            }
        }
        float gx[3];
        NET::density_vjp(na, Wb, lane, tape, gso, gx);
#pragma unroll
        for (int d = 0; d < 3; d++) {
            gx[d] = quad_sum(gx[d]);
        }
        if (lane < 16 && valid) {
#pragma unroll
            for (int d = 0; d < 3; d++) grad_xyzs[(size_t)m * 3 + d] = gx[d] * na.inv_two_bound;
        }
    }
}

// ------------------------------------------------------------------------------------------
// The trajectory planner's collision term (nav/quad_plot.py:216-241 through validate.py:288's density_fn): for planned state s the
// B body points b go to the world (w = R_s b + p_s), to the NeRF's axes (x = w @ rot), through hash grid + sigma net + trunc_exp,
// and out[s] = mean_b sigma^2.  One workgroup per state; its waves take 16-point tiles in turn, and every sum runs in a fixed order
// (tiles of a lane, then lanes, then waves through LDS): no atomics, the same bits on every call and on every graph replay.
// ------------------------------------------------------------------------------------------
struct PlanArgs {
    const float* rot_matrix;   // [S,3,3]
    const float* pos;          // [S,3]
    const float* body;         // [B,3]
    const float* rot;          // [3,3]
    uint32_t S, B;
};

constexpr uint32_t kPlanThreads = 256;

// sum of lanes 0..15 (every other lane holds 0), complete in lane 0.  (wave_sum<16>'s order, but with shuffle width 64 -- the other
// lanes take part with their zeros -- and kept as written: with the header's width-16 form the planner kernels are scheduled differently)
__device__ __forceinline__ float plan_lane_sum(float v) {
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ void plan_load_rot(const PlanArgs& pa, float (&rot)[9]) {
#pragma unroll
    for (int i = 0; i < 9; i++) rot[i] = pa.rot[i];
}

// body point b of state s: its world point w and the density query's input x = w @ rot
__device__ __forceinline__ void plan_point(const PlanArgs& pa, const float (&rot)[9], uint32_t s, uint32_t b, float (&bp)[3], float (&x)[3]) {
    const float* R = pa.rot_matrix + (size_t)s * 9;
    const float* p = pa.pos + (size_t)s * 3;
#pragma unroll
    for (int k = 0; k < 3; k++) bp[k] = pa.body[(size_t)b * 3 + k];
    float w[3];
#pragma unroll
    for (int i = 0; i < 3; i++) w[i] = R[3 * i] * bp[0] + R[3 * i + 1] * bp[1] + R[3 * i + 2] * bp[2] + p[i];
#pragma unroll
    for (int j = 0; j < 3; j++) x[j] = w[0] * rot[j] + w[1] * rot[3 + j] + w[2] * rot[6 + j];
}

template <class NET>
__global__ void __launch_bounds__(kPlanThreads) k_planner_collision(NetArgs na, GridLevels lv, PlanArgs pa, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const size_t w_bytes = NET::w_bytes(na);
    const char* Wlds = smem;
    LevelTab* lt = reinterpret_cast<LevelTab*>(smem + w_bytes);
    float* red = reinterpret_cast<float*>(smem + w_bytes + sizeof(LevelTab));          // [waves]
    stage_block(na, lv, smem, lt, w_bytes);
    float rot[9];
    plan_load_rot(pa, rot);
    const uint32_t s = blockIdx.x;
    const uint32_t lane = threadIdx.x & 63, c = lane & 15, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    const uint32_t n_tiles = (pa.B + 15) / 16;
    float acc = 0.0f;
    for (uint32_t tile = wave; tile < n_tiles; tile += n_waves) {
        const uint32_t b = tile * 16 + c;
        const bool valid = b < pa.B;
        float bp[3], x[3];
        plan_point(pa, rot, s, valid ? b : pa.B - 1, bp, x);
        float sg;
        typename NET::geo_t s16[4];
        NET::density(na, Wlds, *lt, lane, x[0], x[1], x[2], sg, s16);
        if (valid && lane < 16) acc += sg * sg;          // (sigma is meaningful in the lanes of quarter 0)
    }
    acc = plan_lane_sum(lane < 16 ? acc : 0.0f);
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float sum = 0.0f;
        for (uint32_t w = 0; w < n_waves; w++) sum += red[w];
        out[s] = sum / (float)pa.B;
    }
}

// g [S] = dL/d out -> grad_pos [S,3], grad_rot_matrix [S,3,3] (overwritten).  The forward again with kept activations, then per point
// dL/d sigma = (g / B) * (2 sigma) (mean, then pow), trunc_exp's backward, the sigma net and hash grid (NET::density_vjp, as
// k_network_density_bwd), d x / d w = rot^T and d w / d (p, R) = (1, b^T).
template <class NET>
__global__ void __launch_bounds__(kPlanThreads) k_planner_collision_bwd(NetArgs na, GridLevels lv, const char* __restrict__ packed_bwd,
                                                                        PlanArgs pa, const float* __restrict__ g, float* __restrict__ grad_pos,
                                                                        float* __restrict__ grad_rot_matrix) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const size_t w_bytes = NET::w_bytes(na);
    const size_t ws_bytes = NET::kF32 ? (size_t)bwd_floats(na.sig_mm) * 4 : (size_t)bwd_halfs(na.sig_mm) * 2;   // sigma net's transposed fragments
    const char* Wlds = smem;
    char* Wb = smem + w_bytes;
    LevelTab* lt = reinterpret_cast<LevelTab*>(smem + w_bytes + ws_bytes);
    float* red = reinterpret_cast<float*>(smem + w_bytes + ws_bytes + sizeof(LevelTab));   // [waves][12]
    {
        const uint4* src = reinterpret_cast<const uint4*>(packed_bwd);
        uint4* dst = reinterpret_cast<uint4*>(Wb);
        for (uint32_t i = threadIdx.x; i < ws_bytes / 16; i += blockDim.x) dst[i] = src[i];
    }
    stage_block(na, lv, smem, lt, w_bytes);
    float rot[9];
    plan_load_rot(pa, rot);
    const uint32_t s = blockIdx.x;
    const uint32_t lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    const uint32_t n_tiles = (pa.B + 15) / 16;
    const float g_mean = g[s] / (float)pa.B;
    float acc[12];                                       // d/d p (3), then d/d R row-major (9)
#pragma unroll
    for (int i = 0; i < 12; i++) acc[i] = 0.0f;
    for (uint32_t tile = wave; tile < n_tiles; tile += n_waves) {
        const uint32_t b = tile * 16 + c;
        const bool valid = b < pa.B;
        float bp[3], x[3];
        plan_point(pa, rot, s, valid ? b : pa.B - 1, bp, x);
        typename NET::Tape tape;
        typename NET::geo_t s16[4];
        NET::density_tape(na, Wlds, *lt, lane, x[0], x[1], x[2], tape, s16);
        f32x4 gso = {0, 0, 0, 0};
        if (valid && q == 0) {
            const float h = (float)s16[0];
            const float sigma = expf(h);
            gso[0] = (g_mean * (2.0f * sigma)) * expf(fminf(15.0f, fmaxf(-15.0f, h)));
        }
        float gx[3];
        NET::density_vjp(na, Wb, lane, tape, gso, gx);
#pragma unroll
        for (int d = 0; d < 3; d++) {
            gx[d] = quad_sum(gx[d]);
        }
        if (valid && lane < 16) {
            float gxr[3], gw[3];
#pragma unroll
            for (int d = 0; d < 3; d++) gxr[d] = gx[d] * na.inv_two_bound;
#pragma unroll
            for (int i = 0; i < 3; i++) gw[i] = rot[3 * i] * gxr[0] + rot[3 * i + 1] * gxr[1] + rot[3 * i + 2] * gxr[2];
#pragma unroll
            for (int i = 0; i < 3; i++) {
                acc[i] += gw[i];
#pragma unroll
                for (int k = 0; k < 3; k++) acc[3 + 3 * i + k] += gw[i] * bp[k];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 12; i++) {
        const float v = plan_lane_sum(lane < 16 ? acc[i] : 0.0f);
        if (lane == 0) red[wave * 12 + i] = v;
    }
    __syncthreads();
    if (threadIdx.x < 12) {
        float sum = 0.0f;
        for (uint32_t w = 0; w < n_waves; w++) sum += red[w * 12 + threadIdx.x];
        if (threadIdx.x < 3) grad_pos[(size_t)s * 3 + threadIdx.x] = sum;
        else grad_rot_matrix[(size_t)s * 9 + threadIdx.x - 3] = sum;
    }
}

}  // namespace ngp

using namespace ngp;

extern "C" {

int ngp_network_density(const ngp_model* model, const float* xyzs, uint32_t M, float* sigmas, float* geo_feat, ngp_stream_t stream) {
    if (M == 0) return NGP_OK;
    NGP_REQUIRE(xyzs && sigmas, "network_density: null pointer");
    NGP_REQUIRE(model && model->packed_weights, "network_density: model->packed_weights is NULL (ngp_pack_weights fills it)");
    hipStream_t s = (hipStream_t)stream;
    NetArgs na;
    GridLevels lv;
    int rc = fill_net(model, (const _Float16*)model->packed_weights, na, lv);
    if (rc) return rc;
    const size_t lds = weights_bytes(na) + sizeof(LevelTab);
    NGP_REQUIRE(lds <= 96 * 1024, "network_density: the packed weights need %zu bytes of LDS", lds);
    uint32_t blocks = div_up(div_up(M, 16), 4);
    if (blocks > resident_blocks(lds)) blocks = resident_blocks(lds);
    ProfScope prof("network_density", s, M);
    NGP_WITH_NET(net_variant(na, lv), {
        ensure_dynamic_lds(reinterpret_cast<const void*>(k_network_density<NET>), 96 * 1024);
        k_network_density<NET><<<blocks, 256, lds, s>>>(na, lv, xyzs, M, sigmas, geo_feat);
    });
    return check_launch("network_density");
}

int ngp_cell_max_density(const ngp_model* model, const float* start_host, float granularity, uint32_t X, uint32_t Y, uint32_t Z, uint32_t s,
                         const float* rot_host, float* out_max_sigma, ngp_stream_t stream) {
    NGP_REQUIRE(start_host && rot_host && out_max_sigma, "cell_max_density: null pointer");
    NGP_REQUIRE(model && model->packed_weights, "cell_max_density: model->packed_weights is NULL (ngp_pack_weights fills it)");
    NGP_REQUIRE(s >= 1 && s <= 16, "cell_max_density: 1 <= samples per axis <= 16 (got %u)", s);
    NGP_REQUIRE(granularity > 0.0f, "cell_max_density: granularity must be > 0");
    const uint64_t M = (uint64_t)X * Y * Z;
    NGP_REQUIRE(M < ((uint64_t)1 << 31), "cell_max_density: X * Y * Z must be < 2^31");
    if (M == 0) return NGP_OK;
    hipStream_t st = (hipStream_t)stream;
    NetArgs na;
    GridLevels lv;
    int rc = fill_net(model, (const _Float16*)model->packed_weights, na, lv);
    if (rc) return rc;
    const size_t lds = weights_bytes(na) + sizeof(LevelTab);
    NGP_REQUIRE(lds <= 96 * 1024, "cell_max_density: the packed weights need %zu bytes of LDS", lds);
    CellArgs ca;
    for (int d = 0; d < 3; d++) ca.start[d] = start_host[d];
    for (int d = 0; d < 9; d++) ca.rot[d] = rot_host[d];
    ca.granularity = granularity;
    ca.X = X; ca.Y = Y; ca.Z = Z; ca.s = s;
    uint32_t blocks = div_up(div_up((uint32_t)M, 16), 4);
    if (blocks > resident_blocks(lds)) blocks = resident_blocks(lds);
    ProfScope prof("cell_max_density", st, (double)M * s * s * s);
    NGP_WITH_NET(net_variant(na, lv), {
        ensure_dynamic_lds(reinterpret_cast<const void*>(k_cell_max_density<NET>), 96 * 1024);
        k_cell_max_density<NET><<<blocks, 256, lds, st>>>(na, lv, ca, out_max_sigma);
    });
    return check_launch("cell_max_density");
}

int ngp_network_density_backward(const ngp_model* model, const void* packed_weights_bwd, const float* xyzs, uint32_t M, const float* grad_sigmas,
                                 const float* grad_geo_feat, float* grad_xyzs, ngp_stream_t stream) {
    if (M == 0) return NGP_OK;
    NGP_REQUIRE(xyzs && grad_xyzs && (grad_sigmas || grad_geo_feat), "network_density_backward: null pointer");
    NGP_REQUIRE(model && model->packed_weights && packed_weights_bwd, "network_density_backward: packed weights missing (ngp_pack_weights / ngp_pack_weights_bwd)");
    hipStream_t s = (hipStream_t)stream;
    NetArgs na;
    GridLevels lv;
    int rc = fill_net(model, (const _Float16*)model->packed_weights, na, lv);
    if (rc) return rc;
    NGP_REQUIRE(bwd_shape_ok(na), "network_density_backward: the fp32 form supports at most 1 hidden matmul in the sigma net (got %u)", na.sig_mm);
    const size_t ws = na.f32() ? (size_t)bwd_floats(na.sig_mm) * 4 : (size_t)bwd_halfs(na.sig_mm) * 2;
    const size_t lds = weights_bytes(na) + ws + sizeof(LevelTab);
    NGP_REQUIRE(lds <= 160 * 1024, "network_density_backward: LDS budget exceeded (%zu bytes)", lds);
    uint32_t blocks = div_up(div_up(M, 16), 4);
    if (blocks > resident_blocks(lds)) blocks = resident_blocks(lds);
    ProfScope prof("network_density_backward", s, M);
    NGP_WITH_NET(net_variant(na, lv), {
        ensure_dynamic_lds(reinterpret_cast<const void*>(k_network_density_bwd<NET>), 160 * 1024);
        k_network_density_bwd<NET><<<blocks, 256, lds, s>>>(na, lv, (const char*)packed_weights_bwd, xyzs, M, grad_sigmas, grad_geo_feat, grad_xyzs);
    });
    return check_launch("network_density_backward");
}

int ngp_planner_collision(const ngp_model* model, const float* rot_matrix, const float* pos, const float* body, const float* rot, uint32_t S,
                          uint32_t B, float* out, ngp_stream_t stream) {
    if (S == 0) return NGP_OK;
    NGP_REQUIRE(rot_matrix && pos && body && rot && out, "planner_collision: null pointer");
    NGP_REQUIRE(B > 0, "planner_collision: no body points");
    NGP_REQUIRE(model && model->packed_weights, "planner_collision: model->packed_weights is NULL (ngp_pack_weights fills it)");
    hipStream_t s = (hipStream_t)stream;
    NetArgs na;
    GridLevels lv;
    int rc = fill_net(model, (const _Float16*)model->packed_weights, na, lv);
    if (rc) return rc;
    const size_t lds = weights_bytes(na) + sizeof(LevelTab) + (kPlanThreads / 64) * sizeof(float);
    NGP_REQUIRE(lds <= 96 * 1024, "planner_collision: the packed weights need %zu bytes of LDS", lds);
    const PlanArgs pa{rot_matrix, pos, body, rot, S, B};
    ProfScope prof("planner_collision", s, (size_t)S * B);
    NGP_WITH_NET(net_variant(na, lv), {
        ensure_dynamic_lds(reinterpret_cast<const void*>(k_planner_collision<NET>), 96 * 1024);
        k_planner_collision<NET><<<S, kPlanThreads, lds, s>>>(na, lv, pa, out);
    });
    return check_launch("planner_collision");
}

int ngp_planner_collision_backward(const ngp_model* model, const void* packed_weights_bwd, const float* rot_matrix, const float* pos,
                                   const float* body, const float* rot, uint32_t S, uint32_t B, const float* grad_out, float* grad_pos,
                                   float* grad_rot_matrix, ngp_stream_t stream) {
    if (S == 0) return NGP_OK;
    NGP_REQUIRE(rot_matrix && pos && body && rot && grad_out && grad_pos && grad_rot_matrix, "planner_collision_backward: null pointer");
    NGP_REQUIRE(B > 0, "planner_collision_backward: no body points");
    NGP_REQUIRE(model && model->packed_weights && packed_weights_bwd,
                "planner_collision_backward: packed weights missing (ngp_pack_weights / ngp_pack_weights_bwd)");
    hipStream_t s = (hipStream_t)stream;
    NetArgs na;
    GridLevels lv;
    int rc = fill_net(model, (const _Float16*)model->packed_weights, na, lv);
    if (rc) return rc;
    NGP_REQUIRE(bwd_shape_ok(na), "planner_collision_backward: the fp32 form supports at most 1 hidden matmul in the sigma net (got %u)", na.sig_mm);
    const size_t ws = na.f32() ? (size_t)bwd_floats(na.sig_mm) * 4 : (size_t)bwd_halfs(na.sig_mm) * 2;
    const size_t lds = weights_bytes(na) + ws + sizeof(LevelTab) + (kPlanThreads / 64) * 12 * sizeof(float);
    NGP_REQUIRE(lds <= 160 * 1024, "planner_collision_backward: LDS budget exceeded (%zu bytes)", lds);
    const PlanArgs pa{rot_matrix, pos, body, rot, S, B};
    ProfScope prof("planner_collision_backward", s, (size_t)S * B);
    NGP_WITH_NET(net_variant(na, lv), {
        ensure_dynamic_lds(reinterpret_cast<const void*>(k_planner_collision_bwd<NET>), 160 * 1024);
        k_planner_collision_bwd<NET><<<S, kPlanThreads, lds, s>>>(na, lv, (const char*)packed_weights_bwd, pa, grad_out, grad_pos, grad_rot_matrix);
    });
    return check_launch("planner_collision_backward");
}

int ngp_network_forward(const ngp_model* model, const float* xyzs, const float* dirs, uint32_t M, float* sigmas, float* rgbs,
                        ngp_stream_t stream) {
    if (M == 0) return NGP_OK;
    NGP_REQUIRE(xyzs && dirs && sigmas && rgbs, "network_forward: null pointer");
    hipStream_t s = (hipStream_t)stream;
    // No scratch of the library's own: the fragment-major weights are the caller's, packed once per parameter version
    // (a process-wide buffer here would be shared by calls that run concurrently on different streams with different models)
    NGP_REQUIRE(model && model->packed_weights, "network_forward: model->packed_weights is NULL (ngp_pack_weights fills it)");
    NetArgs na;
    GridLevels lv;
    int rc = fill_net(model, (const _Float16*)model->packed_weights, na, lv);
    if (rc) return rc;
    const size_t lds = weights_bytes(na) + sizeof(LevelTab);
    NGP_REQUIRE(lds <= 96 * 1024, "network_forward: the packed weights need %zu bytes of LDS", lds);
    const uint32_t n_tiles = div_up(M, 16);
    uint32_t blocks = div_up(n_tiles, 4);
    if (blocks > resident_blocks(lds)) blocks = resident_blocks(lds);
    ProfScope prof("network_forward", s, M);
    NGP_WITH_NET(net_variant(na, lv), {
        ensure_dynamic_lds(reinterpret_cast<const void*>(k_network_forward<NET>), 96 * 1024);
        k_network_forward<NET><<<blocks, 256, lds, s>>>(na, lv, xyzs, dirs, M, sigmas, rgbs);
    });
    return check_launch("network_forward");
}

}  // extern "C"
