// The data side of a training / evaluation step (reference: nerf/provider.py:311-316, nerf/utils.py:426-480): ground-truth colours out
// of the resident image store, the per-ray MSE with its mean and the error-map update, and the loss's gradient.  The reference spends a
// dozen small torch operators and autograd nodes on this per step; here it is one launch each way.  Wave64, vector loads and stores only.
#include "ngp_common.hpp"
#include "wave_ops.hpp"

namespace ngp {

constexpr uint32_t kStoreF32 = 0, kStoreF16 = 1, kStoreU8 = 2;

__device__ __forceinline__ float round_half(float x) { return (float)(_Float16)x; }

// One stored channel as the float the provider yields.  uint8: table[k] when a table is given (colour channels, linear space), else k / 255.
template <uint32_t DT>
__device__ __forceinline__ float load_channel(const void* store, size_t at, const float* table) {
    if (DT == kStoreF32) return ((const float*)store)[at];
    if (DT == kStoreF16) return (float)((const _Float16*)store)[at];
    const uint32_t code = ((const uint8_t*)store)[at];
    return table ? table[code] : (float)code / 255.0f;
}

template <uint32_t DT, uint32_t C, bool HALF>
__global__ void __launch_bounds__(256) k_train_targets(const void* __restrict__ store, uint64_t frame_base, uint32_t n_pix,
                                                       const int64_t* __restrict__ inds, uint32_t N, const float* __restrict__ bg,
                                                       const float* __restrict__ table, float* __restrict__ gt) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int64_t pix = inds ? inds[i] : (int64_t)i;
    float* out = gt + (size_t)i * 3;
    if (pix < 0 || pix >= (int64_t)n_pix) {      // torch.gather would raise; nothing is read, the target is NaN
        out[0] = out[1] = out[2] = __builtin_nanf("");
        return;
    }
    const size_t at = ((size_t)frame_base + (size_t)pix) * C;
    float rgb[3];
#pragma unroll
    for (uint32_t c = 0; c < 3; c++) {
        rgb[c] = load_channel<DT>(store, at + c, table);
        if (HALF) rgb[c] = round_half(rgb[c]);
    }
    if (C == 4) {
        float a = load_channel<DT>(store, at + 3, nullptr);
        if (HALF) a = round_half(a);
        // images[..., :3] * images[..., 3:] + bg_color * (1 - images[..., 3:])   (utils.py:442): four operators, four roundings
        float rest = 1.0f - a;
        if (HALF) rest = round_half(rest);
#pragma unroll
        for (uint32_t c = 0; c < 3; c++) {
            float b = bg ? bg[(size_t)i * 3 + c] : 1.0f;
            float front = rgb[c] * a, back = b * rest;
            if (HALF) { front = round_half(front); back = round_half(back); }
            rgb[c] = front + back;
            if (HALF) rgb[c] = round_half(rgb[c]);
        }
    }
    out[0] = rgb[0];
    out[1] = rgb[1];
    out[2] = rgb[2];
}

// ---- depth targets ----------------------------------------------------------------------------------------------------------------
// The chosen pixels' ray distances out of the 16-bit depth store (nerf/targets.py DepthStore), one thread per ray:
//   code 0 -> 0 (no measurement), 65535 -> +inf (known empty), else t = ((float)code * unit) * |dir|,
//   dir = ((i + 0.5 - cx) / fx, (j + 0.5 - cy) / fy, 1), the direction get_rays forms for pixel (i, j) before it normalises it.
// Every operation is one fp32 operation.  An id outside [0, n_pix) reads nothing and gives 0.
__global__ void __launch_bounds__(256) k_train_depth_targets(const uint16_t* __restrict__ store, uint64_t frame_base, uint32_t n_pix, uint32_t W,
                                                             const int64_t* __restrict__ inds, uint32_t N, float fx, float fy, float cx, float cy,
                                                             float unit, float* __restrict__ out) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= N) return;
    const int64_t pix = inds ? inds[k] : (int64_t)k;
    if (pix < 0 || pix >= (int64_t)n_pix) { out[k] = 0.0f; return; }
    const uint32_t code = store[(size_t)frame_base + (size_t)pix];
    if (code == 0u) { out[k] = 0.0f; return; }
    if (code == 65535u) { out[k] = __builtin_inff(); return; }
    const float x = (((float)((uint32_t)pix % W) + 0.5f) - cx) / fx;
    const float y = (((float)((uint32_t)pix / W) + 0.5f) - cy) / fy;
    out[k] = ((float)code * unit) * sqrtf((x * x + y * y) + 1.0f);
}

// ---- photometric loss -------------------------------------------------------------------------------------------------------------
// The mean over the rays is the fixed-order mean (DESIGN.md "Cross-lane arithmetic"), fused with the pass that forms the per-ray losses.
template <typename P>
__device__ __forceinline__ float ray_loss(const P* __restrict__ pred, const float* __restrict__ gt, uint32_t i, uint32_t N, float* __restrict__ per_ray,
                                          float* __restrict__ error_row, uint32_t map_len, const int64_t* __restrict__ inds_coarse) {
    if (i >= N) return 0.0f;            // (+0 leaves a sum of non-negative terms unchanged)
    const size_t at = (size_t)i * 3;
    const float d0 = (float)pred[at] - gt[at], d1 = (float)pred[at + 1] - gt[at + 1], d2 = (float)pred[at + 2] - gt[at + 2];
    const float loss = ((d0 * d0 + d1 * d1) + d2 * d2) / 3.0f;
    per_ray[i] = loss;
    if (error_row) {
        const int64_t cell = inds_coarse[i];
        if (cell >= 0 && cell < (int64_t)map_len) error_row[cell] = 0.1f * error_row[cell] + 0.9f * loss;     // distinct ids (header)
    }
    return loss;
}

template <typename P>
__global__ void __launch_bounds__(kMeanOneBlockThreads) k_photo_loss_one_block(const P* __restrict__ pred, const float* __restrict__ gt, uint32_t N,
                                                                              float* __restrict__ per_ray, float* __restrict__ mean,
                                                                              float* __restrict__ error_row, uint32_t map_len,
                                                                              const int64_t* __restrict__ inds_coarse) {
    mean_one_block([&](uint32_t i) { return ray_loss(pred, gt, i, N, per_ray, error_row, map_len, inds_coarse); }, N, mean);
}

template <typename P>
__global__ void __launch_bounds__(kMeanGroupThreads) k_photo_loss_groups(const P* __restrict__ pred, const float* __restrict__ gt, uint32_t N,
                                                                         float* __restrict__ per_ray, float* __restrict__ error_row, uint32_t map_len,
                                                                         const int64_t* __restrict__ inds_coarse, float* __restrict__ groups) {
    mean_groups([&](uint32_t i) { return ray_loss(pred, gt, i, N, per_ray, error_row, map_len, inds_coarse); }, N, groups);
}

// ---- the same mean over a plain float[N] (the distortion loss's per-ray values) ----
__global__ void __launch_bounds__(kMeanOneBlockThreads) k_mean_one_block(const float* __restrict__ values, uint32_t N, float* __restrict__ mean) {
    mean_one_block([&](uint32_t i) { return i < N ? values[i] : 0.0f; }, N, mean);
}

__global__ void __launch_bounds__(kMeanGroupThreads) k_mean_groups(const float* __restrict__ values, uint32_t N, float* __restrict__ groups) {
    mean_groups([&](uint32_t i) { return i < N ? values[i] : 0.0f; }, N, groups);
}

__global__ void __launch_bounds__(64) k_mean_final(const float* __restrict__ groups, uint32_t n_groups, uint32_t N, float* __restrict__ mean) {
    final_mean(groups, n_groups, N, mean);
}

int mean_of_groups(const float* groups, uint32_t N, float* mean, hipStream_t s, const char* what) {
    k_mean_final<<<1, 64, 0, s>>>(groups, div_up(N, 64), N, mean);
    return check_launch(what);
}

int mean_of_rays(const float* values, uint32_t N, float* mean, void* workspace, size_t workspace_bytes, hipStream_t s, const char* what) {
    const size_t need = mean_workspace(N);
    int rc = check_workspace(what, workspace, workspace_bytes, need, alignof(float));
    if (rc) return rc;
    if (!need) {
        k_mean_one_block<<<1, kMeanOneBlockThreads, 0, s>>>(values, N, mean);
        return check_launch(what);
    }
    Carver c(workspace);
    float* const groups = mean_layout(c, N);
    k_mean_groups<<<div_up(N, kMeanGroupThreads), kMeanGroupThreads, 0, s>>>(values, N, groups);
    return mean_of_groups(groups, N, mean, s, what);
}

template <typename P>
__global__ void __launch_bounds__(256) k_photo_loss_backward(const P* __restrict__ pred, const float* __restrict__ gt, uint32_t n3, float three_n,
                                                             const float* __restrict__ g, P* __restrict__ grad) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n3) return;
    grad[k] = (P)(*g * (2.0f * ((float)pred[k] - gt[k])) / three_n);
}

}  // namespace ngp

using namespace ngp;

template <uint32_t DT, uint32_t C>
static void launch_targets(bool half, const void* store, uint64_t frame_base, uint32_t n_pix, const int64_t* inds, uint32_t N, const float* bg,
                           const float* table, float* gt, hipStream_t s) {
    const uint32_t blocks = div_up(N, 256);
    if (half)
        k_train_targets<DT, C, true><<<blocks, 256, 0, s>>>(store, frame_base, n_pix, inds, N, bg, table, gt);
    else
        k_train_targets<DT, C, false><<<blocks, 256, 0, s>>>(store, frame_base, n_pix, inds, N, bg, table, gt);
}

extern "C" {

int ngp_train_targets(const void* store, int store_dtype, uint32_t C, uint64_t frame_base, uint32_t n_pix, const int64_t* inds, uint32_t N,
                      const float* bg, const float* table, int round_half, float* gt_rgb, ngp_stream_t stream) {
    if (N == 0) return NGP_OK;
    NGP_REQUIRE(store && gt_rgb, "train_targets: null pointer");
    NGP_REQUIRE(C == 3 || C == 4, "train_targets: C must be 3 or 4 (got %u)", C);
    NGP_REQUIRE(store_dtype >= 0 && store_dtype <= 2, "train_targets: store dtype must be 0 (f32), 1 (f16) or 2 (uint8)");
    NGP_REQUIRE(!table || store_dtype == (int)kStoreU8, "train_targets: the code table needs a uint8 store");
    NGP_REQUIRE(inds || N <= n_pix, "train_targets: %u rays in pixel order but the frame has %u pixels", N, n_pix);
    hipStream_t s = (hipStream_t)stream;
    const bool half = round_half != 0 || store_dtype == (int)kStoreF16;
    ProfScope prof("train_targets", s, (double)N);
#define NGP_TARGETS(DT)                                                                          \
    if (C == 3) launch_targets<DT, 3>(half, store, frame_base, n_pix, inds, N, bg, table, gt_rgb, s); \
    else launch_targets<DT, 4>(half, store, frame_base, n_pix, inds, N, bg, table, gt_rgb, s)
    if (store_dtype == (int)kStoreF32) { NGP_TARGETS(kStoreF32); }
    else if (store_dtype == (int)kStoreF16) { NGP_TARGETS(kStoreF16); }
    else { NGP_TARGETS(kStoreU8); }
#undef NGP_TARGETS
    return check_launch("train_targets");
}

int ngp_train_depth_targets(const uint16_t* store, uint64_t frame_base, uint32_t n_pix, uint32_t W, const int64_t* inds, uint32_t N, float fx,
                            float fy, float cx, float cy, float unit, float* target, ngp_stream_t stream) {
    if (N == 0) return NGP_OK;
    NGP_REQUIRE(store && target, "train_depth_targets: null pointer");
    NGP_REQUIRE(W > 0 && n_pix % W == 0, "train_depth_targets: %u pixels are no whole rows of %u", n_pix, W);
    NGP_REQUIRE(inds || N <= n_pix, "train_depth_targets: %u rays in pixel order but the frame has %u pixels", N, n_pix);
    NGP_REQUIRE(((uintptr_t)store & 1) == 0, "train_depth_targets: the store must be 2-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("train_depth_targets", s, (double)N);
    k_train_depth_targets<<<div_up(N, 256), 256, 0, s>>>(store, frame_base, n_pix, W, inds, N, fx, fy, cx, cy, unit, target);
    return check_launch("train_depth_targets");
}

size_t ngp_photo_loss_workspace(uint32_t N) { return mean_workspace(N); }

int ngp_photo_loss_forward(const void* pred, int pred_dtype, const float* gt, uint32_t N, float* per_ray, float* mean, float* error_row,
                           uint32_t map_len, const int64_t* inds_coarse, void* workspace, size_t workspace_bytes, ngp_stream_t stream) {
    NGP_REQUIRE(N > 0, "photo_loss_forward: no rays");
    NGP_REQUIRE(N <= 0xFFFFFF00u, "photo_loss_forward: too many rays");
    NGP_REQUIRE(pred && gt && per_ray && mean, "photo_loss_forward: null pointer");
    NGP_REQUIRE(pred_dtype == 0 || pred_dtype == 1, "photo_loss_forward: pred dtype must be 0 (f32) or 1 (f16)");
    NGP_REQUIRE(!error_row || inds_coarse, "photo_loss_forward: an error-map row needs inds_coarse");
    const size_t need = ngp_photo_loss_workspace(N);
    int rc = check_workspace("photo_loss_forward", workspace, workspace_bytes, need, alignof(float));
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("photo_loss", s, (double)N);
    if (!need) {
        if (pred_dtype == 0)
            k_photo_loss_one_block<float><<<1, kMeanOneBlockThreads, 0, s>>>((const float*)pred, gt, N, per_ray, mean, error_row, map_len, inds_coarse);
        else
            k_photo_loss_one_block<_Float16><<<1, kMeanOneBlockThreads, 0, s>>>((const _Float16*)pred, gt, N, per_ray, mean, error_row, map_len, inds_coarse);
        return check_launch("photo_loss_forward");
    }
    Carver c(workspace);
    float* const groups = mean_layout(c, N);
    const uint32_t blocks = div_up(N, kMeanGroupThreads);
    if (pred_dtype == 0)
        k_photo_loss_groups<float><<<blocks, kMeanGroupThreads, 0, s>>>((const float*)pred, gt, N, per_ray, error_row, map_len, inds_coarse, groups);
    else
        k_photo_loss_groups<_Float16><<<blocks, kMeanGroupThreads, 0, s>>>((const _Float16*)pred, gt, N, per_ray, error_row, map_len, inds_coarse, groups);
    rc = check_launch("photo_loss_forward");
    if (rc) return rc;
    return mean_of_groups(groups, N, mean, s, "photo_loss_forward (final)");
}

int ngp_photo_loss_backward(const void* pred, int pred_dtype, const float* gt, uint32_t N, const float* g, void* grad_pred, ngp_stream_t stream) {
    if (N == 0) return NGP_OK;
    NGP_REQUIRE(pred && gt && g && grad_pred, "photo_loss_backward: null pointer");
    NGP_REQUIRE(pred_dtype == 0 || pred_dtype == 1, "photo_loss_backward: pred dtype must be 0 (f32) or 1 (f16)");
    NGP_REQUIRE(N <= 0xFFFFFFFFu / 3, "photo_loss_backward: too many rays");
    hipStream_t s = (hipStream_t)stream;
    const uint32_t n3 = N * 3;
    const float three_n = (float)(3.0 * (double)N);
    ProfScope prof("photo_loss_backward", s, (double)N);
    if (pred_dtype == 0)
        k_photo_loss_backward<float><<<div_up(n3, 256), 256, 0, s>>>((const float*)pred, gt, n3, three_n, g, (float*)grad_pred);
    else
        k_photo_loss_backward<_Float16><<<div_up(n3, 256), 256, 0, s>>>((const _Float16*)pred, gt, n3, three_n, g, (_Float16*)grad_pred);
    return check_launch("photo_loss_backward");
}

}  // extern "C"
