// Image-quality sums of one batch of frames in one pass (reference: uncertainty/evaluation/image_metrics.py:79-135): the SSIM map of
// torchmetrics' structural_similarity_index_measure(data_range, return_full_image=True) -- 11-tap Gaussian window of sigma 1.5, both
// images reflect-padded by 5 -- averaged over the three channels, its masked sum, and the masked squared error per channel that PSNR
// needs.  The reference pads, concatenates five images, runs a grouped 11x11 convolution and a dozen elementwise operators per frame;
// here every pixel is read once (plus the halo) and every sum leaves the kernel in double.  Wave64, vector loads and stores only.
//
// One workgroup of 256 threads owns a kTileH x kTileW tile of the map.  Per channel: (1) the tile and its 5-pixel halo of both images go
// to LDS through the reflected index; (2) 11 taps along x give the five windowed row sums (p, t, p^2, t^2, p t) of every halo row;
// (3) 11 taps along y finish them, each thread for two vertically adjacent pixels (12 rows read for 2 x 11 taps).  All window sums are
// double: a float product is exact in double, so the cancellation in E[p^2] - mu^2 (against c2 = 9e-4) costs nothing (DESIGN.md
// "Image-quality metrics").  -ffp-contract=off: the only fused multiply-adds are the explicit fma() calls.
#include "ngp_common.hpp"
#include "wave_ops.hpp"

namespace ngp {

constexpr int kIqTileH = 16, kIqTileW = 32, kIqHalo = 5, kIqTaps = 2 * kIqHalo + 1;
constexpr int kIqHaloH = kIqTileH + 2 * kIqHalo, kIqHaloW = kIqTileW + 2 * kIqHalo;      // 26 x 42
constexpr int kIqThreads = 256;
constexpr int kIqSums = 5;          // per workgroup: sum mask * ssim, sum mask, sum mask * err^2 of the three channels
// LDS: 2 x 26 x 42 floats + 5 x 26 x 32 doubles + 4 x 5 doubles = 42 176 B: three workgroups per CU inside 160 KB
static_assert(kIqThreads == kIqTileW * kIqTileH / 2, "a thread owns two vertically adjacent pixels");

// Type of the window sums.  double is the build; -DNGP_IQ_FLOAT_SUMS (scripts/build_variant.sh) is the float form, kept to measure what
// the doubles cost and what they buy (DESIGN.md "Image-quality metrics").  The SSIM formula and every sum over pixels stay double.
#ifdef NGP_IQ_FLOAT_SUMS
typedef float IqAcc;
#else
typedef double IqAcc;
#endif

struct IqParams {
    double g[kIqTaps];              // the normalised 1-D window
    double c1, c2;
};

// torch's 'reflect' padding: -k -> k, n-1+k -> n-1-k.  The last tile of a row or column reaches past the padded image: those entries
// feed only outputs outside the image, which nobody keeps -- the clamp is there so that they read inside the image too.
__device__ __forceinline__ int reflect(int i, int n) {
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * (n - 1) - i : i;
    return min(max(i, 0), n - 1);
}

__global__ void __launch_bounds__(kIqThreads) k_image_quality(const float* __restrict__ pred, const float* __restrict__ target,
                                                              const float* __restrict__ mask, int H, int W, int64_t stride_b, int64_t stride_c,
                                                              int64_t stride_y, int64_t stride_x, IqParams prm, float* __restrict__ ssim_map,
                                                              double* __restrict__ partials) {
    __shared__ float s_p[kIqHaloH][kIqHaloW], s_t[kIqHaloH][kIqHaloW];
    __shared__ IqAcc s_row[5][kIqHaloH][kIqTileW];
    __shared__ double s_red[kIqThreads / 64][kIqSums];

    const int tid = threadIdx.x;
    const int b = blockIdx.z, y0 = blockIdx.y * kIqTileH, x0 = blockIdx.x * kIqTileW;
    const int tx = tid & (kIqTileW - 1), ty = (tid / kIqTileW) * 2;       // this thread's pixels: (y0 + ty, x0 + tx) and the one below
    const int px = x0 + tx;
    const bool in0 = px < W && y0 + ty < H, in1 = px < W && y0 + ty + 1 < H;
    const float* pb = pred + (int64_t)b * stride_b;
    const float* tb = target + (int64_t)b * stride_b;

    double ssim0 = 0.0, ssim1 = 0.0, err[3] = {0.0, 0.0, 0.0};
    float m0 = in0 ? 1.0f : 0.0f, m1 = in1 ? 1.0f : 0.0f;
    if (mask) {
        const size_t at = ((size_t)b * H + (y0 + ty)) * W + px;
        if (in0) m0 = mask[at];
        if (in1) m1 = mask[at + W];
    }

    for (int c = 0; c < 3; c++) {
        // (1) tile + halo of both images, x fastest
        for (int i = tid; i < kIqHaloH * kIqHaloW; i += kIqThreads) {
            const int hy = i / kIqHaloW, hx = i - hy * kIqHaloW;
            const int64_t at = (int64_t)c * stride_c + (int64_t)reflect(y0 + hy - kIqHalo, H) * stride_y + (int64_t)reflect(x0 + hx - kIqHalo, W) * stride_x;
            s_p[hy][hx] = pb[at];
            s_t[hy][hx] = tb[at];
        }
        __syncthreads();
        // (2) 11 taps along x for every halo row
        for (int i = tid; i < kIqHaloH * kIqTileW; i += kIqThreads) {
            const int hy = i / kIqTileW, x = i & (kIqTileW - 1);
            IqAcc a_p = 0, a_t = 0, a_pp = 0, a_tt = 0, a_pt = 0;
#pragma unroll
            for (int k = 0; k < kIqTaps; k++) {
                const IqAcc p = (IqAcc)s_p[hy][x + k], t = (IqAcc)s_t[hy][x + k], g = (IqAcc)prm.g[k];
                a_p = fma(g, p, a_p);
                a_t = fma(g, t, a_t);
                a_pp = fma(g, p * p, a_pp);
                a_tt = fma(g, t * t, a_tt);
                a_pt = fma(g, p * t, a_pt);
            }
            s_row[0][hy][x] = a_p;
            s_row[1][hy][x] = a_t;
            s_row[2][hy][x] = a_pp;
            s_row[3][hy][x] = a_tt;
            s_row[4][hy][x] = a_pt;
        }
        __syncthreads();
        // (3) 11 taps along y for two pixels: rows ty .. ty+10 for the upper one, ty+1 .. ty+11 for the lower one
        IqAcc up[5] = {0, 0, 0, 0, 0}, lo[5] = {0, 0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k <= kIqTaps; k++) {
#pragma unroll
            for (int q = 0; q < 5; q++) {
                const IqAcc v = s_row[q][ty + k][tx];
                if (k < kIqTaps) up[q] = fma((IqAcc)prm.g[k], v, up[q]);
                if (k > 0) lo[q] = fma((IqAcc)prm.g[k - 1], v, lo[q]);
            }
        }
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const double s[5] = {(double)(r ? lo : up)[0], (double)(r ? lo : up)[1], (double)(r ? lo : up)[2], (double)(r ? lo : up)[3],
                                 (double)(r ? lo : up)[4]};
            const double mu_pp = s[0] * s[0], mu_tt = s[1] * s[1], mu_pt = s[0] * s[1];
            const double var_p = fmax(s[2] - mu_pp, 0.0), var_t = fmax(s[3] - mu_tt, 0.0), cov = s[4] - mu_pt;
            const double v = ((2.0 * mu_pt + prm.c1) * (2.0 * cov + prm.c2)) / ((mu_pp + mu_tt + prm.c1) * (var_p + var_t + prm.c2));
            if (r) ssim1 += v; else ssim0 += v;
        }
        // squared error of the two pixels themselves (float difference, exact square, double sum)
        const float d0 = s_p[ty + kIqHalo][tx + kIqHalo] - s_t[ty + kIqHalo][tx + kIqHalo];
        const float d1 = s_p[ty + 1 + kIqHalo][tx + kIqHalo] - s_t[ty + 1 + kIqHalo][tx + kIqHalo];
        if (in0) err[c] += (double)m0 * ((double)d0 * (double)d0);
        if (in1) err[c] += (double)m1 * ((double)d1 * (double)d1);
        __syncthreads();            // the next channel overwrites the tiles
    }

    ssim0 /= 3.0;
    ssim1 /= 3.0;
    if (ssim_map) {
        const size_t at = ((size_t)b * H + (y0 + ty)) * W + px;
        if (in0) ssim_map[at] = (float)ssim0;
        if (in1) ssim_map[at + W] = (float)ssim1;
    }
    double sums[kIqSums];
    sums[0] = (in0 ? (double)m0 * ssim0 : 0.0) + (in1 ? (double)m1 * ssim1 : 0.0);
    sums[1] = (double)m0 + (double)m1;
    sums[2] = err[0];
    sums[3] = err[1];
    sums[4] = err[2];
    // fixed order: the 64 lanes of a wave by the xor butterfly, then the four waves in order
#pragma unroll
    for (int q = 0; q < kIqSums; q++) {
        const double v = wave_sum(sums[q]);
        if ((tid & 63) == 0) s_red[tid >> 6][q] = v;
    }
    __syncthreads();
    if (tid < kIqSums) {
        const uint32_t tiles = gridDim.x * gridDim.y, tile = blockIdx.y * gridDim.x + blockIdx.x;
        partials[((size_t)b * kIqSums + tid) * tiles + tile] = ((s_red[0][tid] + s_red[1][tid]) + s_red[2][tid]) + s_red[3][tid];
    }
}

// One workgroup per image, wave q sums quantity q: lane l adds the tiles l, l + 64, ... in that order, then the butterfly.
__global__ void __launch_bounds__(64 * kIqSums) k_image_quality_final(const double* __restrict__ partials, uint32_t tiles, double hw,
                                                                      double* __restrict__ stats) {
    const uint32_t b = blockIdx.x, q = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double* src = partials + ((size_t)b * kIqSums + q) * tiles;
    double acc = 0.0;
    for (uint32_t i = lane; i < tiles; i += 64) acc += src[i];
    acc = wave_sum(acc);
    if (lane == 0) stats[(size_t)b * 8 + q] = acc;
    if (threadIdx.x < 3) stats[(size_t)b * 8 + 5 + threadIdx.x] = threadIdx.x == 0 ? hw : 0.0;
}

static inline uint32_t iq_tiles(uint32_t H, uint32_t W) { return div_up(H, kIqTileH) * div_up(W, kIqTileW); }

// [B][kIqSums][tiles] partial sums, one per tile and quantity
static double* iq_layout(Carver& c, uint32_t B, uint32_t H, uint32_t W) { return c.take<double>((size_t)B * kIqSums * iq_tiles(H, W)); }

}  // namespace ngp

using namespace ngp;

extern "C" {

size_t ngp_image_quality_workspace(uint32_t B, uint32_t H, uint32_t W) {
    if (B == 0 || B > 65535 || H < 6 || W < 6 || H > 32768 || W > 32768) return 0;
    Carver c; iq_layout(c, B, H, W); return c.bytes();
}

int ngp_image_quality(const float* pred, const float* target, const float* mask, uint32_t B, uint32_t H, uint32_t W, int64_t stride_b,
                      int64_t stride_c, int64_t stride_y, int64_t stride_x, float data_range, float* ssim_map, double* stats, void* workspace,
                      size_t workspace_bytes, ngp_stream_t stream) {
    NGP_REQUIRE(pred && target && stats, "image_quality: null pointer");
    NGP_REQUIRE(H >= 6 && W >= 6, "image_quality: a reflect pad of 5 needs H, W >= 6 (got %u x %u)", H, W);
    NGP_REQUIRE(H <= 32768 && W <= 32768, "image_quality: frame too large (%u x %u)", H, W);
    NGP_REQUIRE(B >= 1 && B <= 65535, "image_quality: batch size must be in [1, 65535] (got %u)", B);
    NGP_REQUIRE(data_range > 0.0f, "image_quality: data_range must be positive");     // (false for NaN as well)
    NGP_REQUIRE(stride_b >= 0 && stride_c >= 0 && stride_y >= 0 && stride_x >= 0, "image_quality: negative stride");
    int rc = check_workspace("image_quality", workspace, workspace_bytes, ngp_image_quality_workspace(B, H, W), 8);
    if (rc) return rc;
    Carver c(workspace);
    double* const partial = iq_layout(c, B, H, W);
    IqParams prm;
    double sum = 0.0;
    for (int k = 0; k < kIqTaps; k++) {
        const double d = (double)(k - kIqHalo) / 1.5;
        prm.g[k] = exp(-0.5 * d * d);
        sum += prm.g[k];
    }
    for (int k = 0; k < kIqTaps; k++) prm.g[k] /= sum;
    prm.c1 = (0.01 * (double)data_range) * (0.01 * (double)data_range);
    prm.c2 = (0.03 * (double)data_range) * (0.03 * (double)data_range);

    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("image_quality", s, (double)B * H * W);
    const dim3 grid(div_up(W, kIqTileW), div_up(H, kIqTileH), B);
    k_image_quality<<<grid, kIqThreads, 0, s>>>(pred, target, mask, (int)H, (int)W, stride_b, stride_c, stride_y, stride_x, prm, ssim_map,
                                                partial);
    rc = check_launch("image_quality");
    if (rc) return rc;
    k_image_quality_final<<<B, 64 * kIqSums, 0, s>>>(partial, iq_tiles(H, W), (double)H * (double)W, stats);
    return check_launch("image_quality (final)");
}

}  // extern "C"
