// sigma_fit.hip -- the Bayesian-Laplace fit's objective on cached encoder features (uncertainty/quantification/bayesian_laplace.py:38-53):
//   L(theta) = 0.5 sum_j (theta_j - mu)^2 / s^2 + 0.5 sum_i (y_i - sigma_i)^2,  sigma_i = exp(h_i0),  h_i = W2 relu(W1 f_i)
// theta = [W1 (64 x 32) | W2 (16 x 64)] in nn.Linear order.  The parameters sit AFTER the hash grid, so the features of a frame's
// points are encoded once per perturbation and every one of the fit's evaluations is this fp32 MLP plus a reduction over n points.
//
// k_sigma_fit: persistent workgroups of 4 waves, one 16-point tile per wave and iteration (a workgroup steps through 64-point tiles).
// theta is staged in LDS once, then every lane keeps its W1 fragments and its slice of W2's row 0 in registers for all its tiles.
//   forward   Hid [point][unit] = F W1^T on v_mfma_f32_16x16x4_f32: A = the lane's feature row (point c = lane & 15, features
//             8 q .. 8 q + 7, q = lane >> 4: two 16-byte loads), B = W1[16 ub + c][8 q + j].  The accumulator of block ub holds
//             Hid[point 4 q + r][unit 16 ub + c]; h_0 of the lane's four points is a 4-term fmaf chain over ub and a butterfly over c.
//   backward  dh_0 = (sigma - y) exp(clamp(h_0, -15, 15)) (trunc_exp's backward, activation.py); dW2[0][unit] accumulates in registers;
//             dHid (unit on lane & 15, point on (q, r)) is directly the A operand of dW1 += dHid^T F, whose B operand is the tile's
//             features read a second time with the point on (q, r) (the lines are in L1 from the forward read).  dW1 stays in 32
//             accumulator registers across all of a wave's tiles.
// Rows 1..15 of W2 never reach the loss: their gradient is the prior term alone.
// Reduction order (no atomics, the same bits on every call): lanes -> wave (butterflies), the 4 waves in index order through LDS,
// one partial per workgroup in the caller's workspace; k_sigma_fit_reduce sums the partials of workgroups w = seg, seg + 4, ... in
// double per segment, the four segments in order, adds the prior terms and rounds once.  The loss is accumulated in double throughout.
#include "fused_net.hpp"
#include "wave_ops.hpp"

namespace ngp {

constexpr uint32_t kFitThreads = 256, kFitTile = 64;
constexpr uint32_t kFitDefaultWG = 512, kFitMaxWG = 4096;        // default: two workgroups per CU of an MI355X
constexpr uint32_t kFitTheta = 3072, kFitW1 = 2048;
constexpr uint32_t kFitPartial = kFitW1 + 64;                    // floats per workgroup: dW1 [64][32] | dW2[0] [64]

static uint32_t fit_workgroups(uint32_t n, uint32_t max_workgroups) {
    const uint32_t cap = max_workgroups ? max_workgroups : kFitDefaultWG;
    const uint32_t tiles = (uint32_t)(((uint64_t)n + kFitTile - 1) / kFitTile);
    return tiles < 1 ? 1 : tiles < cap ? tiles : cap;
}

template <bool GRAD>
__global__ void __launch_bounds__(kFitThreads) k_sigma_fit(const float* __restrict__ features, const float* __restrict__ y, uint32_t n,
                                                           const float* __restrict__ theta, double* __restrict__ part_loss,
                                                           float* __restrict__ part_grad) {
    __shared__ float lds[4 * kFitPartial];                       // theta (3072 floats) first, the waves' partial gradients at the end
    __shared__ double lds_loss[4];
    for (uint32_t i = threadIdx.x; i < kFitTheta; i += kFitThreads) lds[i] = theta[i];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
    float w1[4][8], w2[4];
#pragma unroll
    for (int ub = 0; ub < 4; ub++) {
#pragma unroll
        for (int j = 0; j < 8; j++) w1[ub][j] = lds[(16 * ub + c) * 32 + 8 * q + j];
        w2[ub] = lds[kFitW1 + 16 * ub + c];
    }
    __syncthreads();                                             // (the LDS image is overwritten by the reduction below)

    f32x4 dw1[4][2];
    float dw2[4] = {0, 0, 0, 0};
#pragma unroll
    for (int ub = 0; ub < 4; ub++) dw1[ub][0] = dw1[ub][1] = (f32x4){0, 0, 0, 0};
    double loss = 0.0;

    const uint64_t tiles16 = ((uint64_t)n + 15) / 16;
    for (uint64_t t = (uint64_t)blockIdx.x * 4 + wave; t < tiles16; t += (uint64_t)gridDim.x * 4) {
        const uint64_t base = t * 16;
        float xa[8];
        {
            float4 a0 = {0, 0, 0, 0}, a1 = {0, 0, 0, 0};
            if (base + c < n) {                                  // a point past the end is a zero row, and is masked out below
                const float4* src = reinterpret_cast<const float4*>(features + (base + c) * 32 + 8 * q);
                a0 = src[0];
                a1 = src[1];
            }
            xa[0] = a0.x; xa[1] = a0.y; xa[2] = a0.z; xa[3] = a0.w; xa[4] = a1.x; xa[5] = a1.y; xa[6] = a1.z; xa[7] = a1.w;
        }
        f32x4 hid[4];
#pragma unroll
        for (int ub = 0; ub < 4; ub++) hid[ub] = (f32x4){0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 8; j++)
#pragma unroll
            for (int ub = 0; ub < 4; ub++) hid[ub] = mfma4(xa[j], w1[ub][j], hid[ub]);

        float h0[4], dh0[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            float p = 0.0f;
#pragma unroll
            for (int ub = 0; ub < 4; ub++) p = fmaf(w2[ub], fmaxf(hid[ub][r], 0.0f), p);
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) p += __shfl_xor(p, off, 64);      // every lane of the q group ends with the same bits (ASCENDING offsets: not the order of wave_ops.hpp's wave_sum<16>)
            h0[r] = p;
        }
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const uint64_t idx = base + 4 * q + r;
            const bool valid = idx < n;
            const float yv = valid ? y[idx] : 0.0f;
            const float sig = expf(h0[r]);                       // trunc_exp forward (activation.py:8-10)
            const float res = yv - sig;
            if (valid && c == 0) loss += 0.5 * (double)res * (double)res;
            dh0[r] = valid ? (sig - yv) * expf(clampf(h0[r], -15.0f, 15.0f)) : 0.0f;
        }
        if (GRAD) {
            float xb[4][2];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const uint64_t idx = base + 4 * q + r;
#pragma unroll
                for (int fb = 0; fb < 2; fb++) xb[r][fb] = idx < n ? features[idx * 32 + 16 * fb + c] : 0.0f;
            }
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int ub = 0; ub < 4; ub++) {
                    const bool on = hid[ub][r] > 0.0f;
                    dw2[ub] = fmaf(dh0[r], on ? hid[ub][r] : 0.0f, dw2[ub]);
                    const float dhid = on ? w2[ub] * dh0[r] : 0.0f;
                    dw1[ub][0] = mfma4(dhid, xb[r][0], dw1[ub][0]);
                    dw1[ub][1] = mfma4(dhid, xb[r][1], dw1[ub][1]);
                }
        }
    }

    // ---- lanes -> wave -> workgroup, fixed order
    loss = wave_sum_lane0(loss);
    if (lane == 0) lds_loss[wave] = loss;
    if (GRAD) {
        float* buf = lds + wave * kFitPartial;
#pragma unroll
        for (int ub = 0; ub < 4; ub++) {
            float v = dw2[ub];      // (wave_ops.hpp's quad_sum, written out: as a call k_sigma_fit<true> compiles to other instructions)
            v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 32, 64);
            if (q == 0) buf[kFitW1 + 16 * ub + c] = v;
#pragma unroll
            for (int fb = 0; fb < 2; fb++)
#pragma unroll
                for (int r = 0; r < 4; r++) buf[(16 * ub + 4 * q + r) * 32 + 16 * fb + c] = dw1[ub][fb][r];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) part_loss[blockIdx.x] = ((lds_loss[0] + lds_loss[1]) + lds_loss[2]) + lds_loss[3];
    if (GRAD) {
        float* out = part_grad + (size_t)blockIdx.x * kFitPartial;
        for (uint32_t j = threadIdx.x; j < kFitPartial; j += kFitThreads)
            out[j] = ((lds[j] + lds[kFitPartial + j]) + lds[2 * kFitPartial + j]) + lds[3 * kFitPartial + j];
    }
}

// blocks [0, grad_blocks): 64 gradient entries each (mode 1: the prior term alone, exactly (theta - mu) / s^2; mode 2: + the summed
// partials); the last block: the loss, and the fit's bookkeeping when its pointers are given.
__global__ void __launch_bounds__(kFitThreads) k_sigma_fit_reduce(const double* __restrict__ part_loss, const float* __restrict__ part_grad,
                                                                  uint32_t wgs, const float* __restrict__ theta, float mu, float var,
                                                                  double var_d, int mode, uint32_t grad_blocks, float* __restrict__ grad,
                                                                  double* __restrict__ loss_out, float* __restrict__ history,
                                                                  float* __restrict__ min_loss, int32_t* __restrict__ improved) {
    __shared__ double red[kFitThreads];
    if (blockIdx.x < grad_blocks) {
        const uint32_t e = blockIdx.x * 64 + (threadIdx.x & 63), seg = threadIdx.x >> 6;
        double s = 0.0;
        if (mode == 2 && e < kFitPartial)                        // theta[0, 2112) = W1 and row 0 of W2 = the partial's layout
            for (uint32_t w = seg; w < wgs; w += 4) s += (double)part_grad[(size_t)w * kFitPartial + e];
        red[threadIdx.x] = s;
        __syncthreads();
        if (seg == 0) {
            const float prior = (theta[e] - mu) / var;
            const double lik = ((red[threadIdx.x] + red[64 + threadIdx.x]) + red[128 + threadIdx.x]) + red[192 + threadIdx.x];
            grad[e] = mode == 2 ? (float)((double)prior + lik) : prior;
        }
        return;
    }
    double acc = 0.0;
    for (uint32_t j = threadIdx.x; j < kFitTheta; j += kFitThreads) {
        const double d = (double)theta[j] - (double)mu;
        acc += d * d;
    }
    acc = 0.5 * acc / var_d;
    for (uint32_t w = threadIdx.x; w < wgs; w += kFitThreads) acc += part_loss[w];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (uint32_t half = kFitThreads / 2; half > 0; half >>= 1) {
        if (threadIdx.x < half) red[threadIdx.x] += red[threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double loss = red[0];
        const float l32 = (float)loss;
        if (loss_out) *loss_out = loss;
        if (history) *history = l32;
        if (min_loss && l32 < *min_loss) {                       // `if loss < minLoss` (:79): a NaN never improves
            *min_loss = l32;
            if (improved) *improved = 1;
        }
    }
}

struct FitWs {
    double* part_loss;      // [wgs] one partial loss per workgroup
    float* part_grad;       // [wgs][kFitPartial] and its partial gradient
    uint32_t wgs;
};
static FitWs fit_layout(Carver& c, uint32_t n, uint32_t max_workgroups) {
    const uint32_t wgs = fit_workgroups(n, max_workgroups);
    return {c.take<double>(wgs), c.take<float>((size_t)wgs * kFitPartial), wgs};
}

static int fit_launch(const float* features, const float* y, uint32_t n, const float* theta, float prior_mean, double prior_var, int mode,
                      uint32_t max_workgroups, void* workspace, size_t workspace_bytes, double* loss, float* grad, float* history,
                      float* min_loss, int32_t* improved, hipStream_t s) {
    NGP_REQUIRE(features && y && theta, "sigma_fit: null pointer");
    NGP_REQUIRE(n >= 1, "sigma_fit: no points");
    NGP_REQUIRE(mode >= 0 && mode <= 2, "sigma_fit: mode must be 0 (loss), 1 (loss + prior gradient) or 2 (loss + full gradient)");
    NGP_REQUIRE(mode == 0 || grad, "sigma_fit: mode %d needs a gradient buffer", mode);
    NGP_REQUIRE(max_workgroups <= kFitMaxWG, "sigma_fit: max_workgroups %u > %u", max_workgroups, kFitMaxWG);
    NGP_REQUIRE(prior_var > 0.0, "sigma_fit: the prior's variance must be positive");
    NGP_REQUIRE(((uintptr_t)features & 15) == 0, "sigma_fit: features must be 16-byte aligned");
    int rc = check_workspace("sigma_fit", workspace, workspace_bytes, ngp_sigma_fit_workspace(n, max_workgroups), 8);
    if (rc) return rc;
    Carver c(workspace);
    const FitWs w = fit_layout(c, n, max_workgroups);
    ProfScope prof(mode == 2 ? "sigma_fit_grad" : "sigma_fit_loss", s, (double)n);
    if (mode == 2)
        k_sigma_fit<true><<<w.wgs, kFitThreads, 0, s>>>(features, y, n, theta, w.part_loss, w.part_grad);
    else
        k_sigma_fit<false><<<w.wgs, kFitThreads, 0, s>>>(features, y, n, theta, w.part_loss, w.part_grad);
    rc = check_launch("sigma_fit");
    if (rc) return rc;
    const uint32_t grad_blocks = mode == 0 ? 0 : kFitTheta / 64;
    k_sigma_fit_reduce<<<grad_blocks + 1, kFitThreads, 0, s>>>(w.part_loss, w.part_grad, w.wgs, theta, prior_mean, (float)prior_var, prior_var, mode,
                                                              grad_blocks, grad, loss, history, min_loss, improved);
    return check_launch("sigma_fit (reduce)");
}

}  // namespace ngp

using namespace ngp;

extern "C" {

size_t ngp_sigma_fit_workspace(uint32_t n, uint32_t max_workgroups) {
    if (max_workgroups > kFitMaxWG) return 0;
    Carver c; fit_layout(c, n, max_workgroups); return c.bytes();
}

int ngp_sigma_fit_eval(const float* features, const float* y, uint32_t n, const float* theta, float prior_mean, double prior_var, int mode,
                       uint32_t max_workgroups, void* workspace, size_t workspace_bytes, double* loss, float* grad, ngp_stream_t stream) {
    NGP_REQUIRE(loss, "sigma_fit_eval: null loss");
    return fit_launch(features, y, n, theta, prior_mean, prior_var, mode, max_workgroups, workspace, workspace_bytes, loss, grad, nullptr,
                      nullptr, nullptr, (hipStream_t)stream);
}

int ngp_sigma_fit_step(const float* features, const float* y, uint32_t n, float* theta, float prior_mean, double prior_var, int mode,
                       uint32_t max_workgroups, void* workspace, size_t workspace_bytes, float* grad, float* exp_avg, float* exp_avg_sq,
                       float lr, uint32_t step, float* min_loss, int32_t* improved, float* history, uint32_t history_index,
                       ngp_stream_t stream) {
    NGP_REQUIRE(mode == 1 || mode == 2, "sigma_fit_step: mode must be 1 (prior gradient) or 2 (full gradient)");
    NGP_REQUIRE(exp_avg && exp_avg_sq && min_loss && improved && history, "sigma_fit_step: null pointer");
    NGP_REQUIRE(step >= 1, "sigma_fit_step: step counts from 1");
    int rc = fit_launch(features, y, n, theta, prior_mean, prior_var, mode, max_workgroups, workspace, workspace_bytes, nullptr, grad,
                        history + history_index, min_loss, improved, (hipStream_t)stream);
    if (rc) return rc;
    // torch.optim.Adam's defaults (bayesian_laplace.py:71), the host-stepped kernel of the optimiser: the step count is the loop index
    return ngp_adam_step(theta, grad, exp_avg, exp_avg_sq, kFitTheta, lr, 0.9f, 0.999f, 1e-8f, step, 1.0f, stream);
}

}  // extern "C"
