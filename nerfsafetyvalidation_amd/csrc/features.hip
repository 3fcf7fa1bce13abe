// features.hip -- the detection stage of SIFT (Lowe 2004, as cv2.SIFT_create() parameterises it) and the dilated interest mask the
// state estimator samples its pixels from (nav/estimator_helpers.py find_POI + estimate_relative_pose's mask, nerfsafetyvalidation_amd/
// nav/features.py).  Only what the estimator consumes is computed: the integer keypoint positions and the dilated mask -- no
// orientations, no descriptors (orientation copies of a keypoint share its position).
//
// The arithmetic is written to be restated bit for bit by a float32 numpy program (nav/sift_numpy.py): every blur sum runs in a
// fixed tap order with plain mul / add (-ffp-contract=off) and host-supplied float32 weights; the refinement solves its 3x3 system
// with one explicit cofactor formula; float division is IEEE (hipcc's default correctly rounded division).
//
//   k_sift_base        RGB -> gray (BGR2GRAY's fixed-point weights applied to R, G, B: the reference passes RGB to an OpenCV call
//                      that assumes BGR), x2 bilinear upsample with half-pixel centres (replicated border)
//   k_sift_blur_rows   one pass of a separable Gaussian along rows, the row segment and its apron staged in LDS (reflect-101)
//   k_sift_blur_cols   the pass along columns, one thread per output, coalesced across x
//   k_sift_decimate    the next octave's base: every second pixel of layer 3
//   k_sift_dog         the 5 difference-of-Gaussian layers of an octave
//   k_sift_extrema     candidates of DoG layers 1..3, Newton refinement, contrast and edge tests; an accepted keypoint sets its
//                      truncated position in the point mask (the same byte may be set twice: harmless, no sort needed) and counts
//   k_sift_dilate      separable max filter (cv2.dilate with a k x k box, `iter` times: pixels outside the image do not contribute)
#include <algorithm>
#include <cmath>

#include "ngp_common.hpp"

namespace ngp {

constexpr uint32_t kSiftBlock = 256;
constexpr int kSiftMaxTaps = 63;
constexpr int kSiftLayers = 3;                 // nOctaveLayers
constexpr int kSiftGauss = kSiftLayers + 3;    // Gaussian layers per octave
constexpr int kSiftDog = kSiftLayers + 2;      // DoG layers per octave
constexpr int kSiftBorder = 5;                 // SIFT_IMG_BORDER
constexpr int kSiftMaxInterp = 5;              // SIFT_MAX_INTERP_STEPS
constexpr int kSiftMaxOctaves = 32;

struct SiftTaps {
    float w[kSiftMaxTaps];
    int n;
};

// cv::borderInterpolate(p, len, BORDER_REFLECT_101)
__host__ __device__ inline int sift_reflect101(int p, int len) {
    if (len == 1) return 0;
    while ((unsigned)p >= (unsigned)len) p = p < 0 ? -p : 2 * len - 2 - p;
    return p;
}

__global__ void __launch_bounds__(kSiftBlock) k_sift_base(const uint8_t* __restrict__ rgb, uint32_t H, uint32_t W, float* __restrict__ out) {
    const uint32_t W2 = 2 * W, n = 4 * H * W;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int Y = (int)(i / W2), X = (int)(i % W2);
        // source sample (X + 0.5) / 2 - 0.5: even X -> 0.25 of X/2 - 1 and 0.75 of X/2; odd -> 0.75 of (X-1)/2 and 0.25 of the next
        const int xl = (X & 1) ? (X >> 1) : (X >> 1) - 1, yl = (Y & 1) ? (Y >> 1) : (Y >> 1) - 1;
        const float wxl = (X & 1) ? 0.75f : 0.25f, wyl = (Y & 1) ? 0.75f : 0.25f;
        const float wxh = (X & 1) ? 0.25f : 0.75f, wyh = (Y & 1) ? 0.25f : 0.75f;
        const int x0 = min(max(xl, 0), (int)W - 1), x1 = min(max(xl + 1, 0), (int)W - 1);
        const int y0 = min(max(yl, 0), (int)H - 1), y1 = min(max(yl + 1, 0), (int)H - 1);
        float g[4];
        const int ys[2] = {y0, y1}, xs[2] = {x0, x1};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint8_t* p = rgb + ((size_t)ys[k >> 1] * W + xs[k & 1]) * 3;
            g[k] = (float)((1868 * (int)p[0] + 9617 * (int)p[1] + 4899 * (int)p[2] + 8192) >> 14);
        }
        const float top = wxl * g[0] + wxh * g[1];
        const float bot = wxl * g[2] + wxh * g[3];
        out[i] = wyl * top + wyh * bot;
    }
}

__global__ void __launch_bounds__(kSiftBlock) k_sift_blur_rows(const float* __restrict__ src, float* __restrict__ dst, int rows, int cols,
                                                               SiftTaps taps) {
    __shared__ float tile[kSiftBlock + kSiftMaxTaps];
    const int r = taps.n / 2;
    const int y = blockIdx.y, x0 = blockIdx.x * kSiftBlock;
    const float* row = src + (size_t)y * cols;
    for (int i = threadIdx.x; i < (int)kSiftBlock + 2 * r; i += kSiftBlock) tile[i] = row[sift_reflect101(x0 + i - r, cols)];
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x >= cols) return;
    float acc = 0.0f;
    for (int k = 0; k < taps.n; k++) acc = acc + taps.w[k] * tile[threadIdx.x + k];
    dst[(size_t)y * cols + x] = acc;
}

__global__ void __launch_bounds__(kSiftBlock) k_sift_blur_cols(const float* __restrict__ src, float* __restrict__ dst, int rows, int cols,
                                                               SiftTaps taps) {
    const int x = blockIdx.x * kSiftBlock + threadIdx.x, y = blockIdx.y;
    if (x >= cols) return;
    const int r = taps.n / 2;
    float acc = 0.0f;
    for (int k = 0; k < taps.n; k++) acc = acc + taps.w[k] * src[(size_t)sift_reflect101(y + k - r, rows) * cols + x];
    dst[(size_t)y * cols + x] = acc;
}

__global__ void __launch_bounds__(kSiftBlock) k_sift_decimate(const float* __restrict__ src, int src_cols, float* __restrict__ dst, int rows,
                                                              int cols) {
    const uint32_t n = (uint32_t)rows * cols;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t y = i / cols, x = i % cols;
        dst[i] = src[(size_t)(2 * y) * src_cols + 2 * x];
    }
}

__global__ void __launch_bounds__(kSiftBlock) k_sift_dog(const float* __restrict__ gauss, float* __restrict__ dog, uint32_t plane) {
    const uint32_t n = plane * kSiftDog;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) dog[i] = gauss[i + plane] - gauss[i];
}

// one octave's candidates: (layer 1..3, r, c) with r, c in [border, size - border)
__global__ void __launch_bounds__(kSiftBlock) k_sift_extrema(const float* __restrict__ dog, int rows, int cols, int octave, uint32_t H,
                                                             uint32_t W, uint8_t* __restrict__ points, uint32_t* __restrict__ count) {
    const int ir = rows - 2 * kSiftBorder, ic = cols - 2 * kSiftBorder;
    if (ir <= 0 || ic <= 0) return;
    const uint32_t n = (uint32_t)kSiftLayers * ir * ic;
    const size_t plane = (size_t)rows * cols;
    const float img_scale = 1.0f / 255.0f;
    const float deriv_scale = img_scale * 0.5f, second_scale = img_scale, cross_scale = img_scale * 0.25f;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        int layer = 1 + (int)(i / (uint32_t)(ir * ic));
        const uint32_t rem = i % (uint32_t)(ir * ic);
        int r = kSiftBorder + (int)(rem / ic), c = kSiftBorder + (int)(rem % ic);
        {
            const float* cur = dog + layer * plane + (size_t)r * cols + c;
            const float val = *cur;
            if (!(fabsf(val) > 1.0f)) continue;       // floor(0.5 * 0.04 / 3 * 255) = 1
            bool is_max = val > 0.0f, is_min = val < 0.0f;
            for (int dl = -1; dl <= 1; dl++)
                for (int dy = -1; dy <= 1; dy++)
                    for (int dx = -1; dx <= 1; dx++) {
                        if (dl == 0 && dy == 0 && dx == 0) continue;
                        const float v = cur[(ptrdiff_t)dl * (ptrdiff_t)plane + dy * cols + dx];
                        is_max = is_max && val >= v;
                        is_min = is_min && val <= v;
                    }
            if (!is_max && !is_min) continue;
        }
        // Newton refinement of the 3-D quadratic (adjustLocalExtrema)
        float xc = 0.0f, xr = 0.0f, xi = 0.0f, dx = 0.0f, dy = 0.0f, ds = 0.0f;
        bool ok = false;
        for (int step = 0; step < kSiftMaxInterp; step++) {
            const float* img = dog + layer * plane;
            const float* prv = img - plane;
            const float* nxt = img + plane;
            const size_t o = (size_t)r * cols + c;
            dx = (img[o + 1] - img[o - 1]) * deriv_scale;
            dy = (img[o + cols] - img[o - cols]) * deriv_scale;
            ds = (nxt[o] - prv[o]) * deriv_scale;
            const float v2 = img[o] * 2.0f;
            const float dxx = (img[o + 1] + img[o - 1] - v2) * second_scale;
            const float dyy = (img[o + cols] + img[o - cols] - v2) * second_scale;
            const float dss = (nxt[o] + prv[o] - v2) * second_scale;
            const float dxy = (img[o + cols + 1] - img[o + cols - 1] - img[o - cols + 1] + img[o - cols - 1]) * cross_scale;
            const float dxs = (nxt[o + 1] - nxt[o - 1] - prv[o + 1] + prv[o - 1]) * cross_scale;
            const float dys = (nxt[o + cols] - nxt[o - cols] - prv[o + cols] + prv[o - cols]) * cross_scale;
            // X = H^-1 (dx, dy, ds) by cofactors, H = [[dxx dxy dxs] [dxy dyy dys] [dxs dys dss]]
            const float c00 = dyy * dss - dys * dys, c01 = dys * dxs - dxy * dss, c02 = dxy * dys - dyy * dxs;
            const float c11 = dxx * dss - dxs * dxs, c12 = dxy * dxs - dxx * dys, c22 = dxx * dyy - dxy * dxy;
            const float det = dxx * c00 + dxy * c01 + dxs * c02;
            if (det == 0.0f) break;
            xc = -((c00 * dx + c01 * dy + c02 * ds) / det);
            xr = -((c01 * dx + c11 * dy + c12 * ds) / det);
            xi = -((c02 * dx + c12 * dy + c22 * ds) / det);
            if (fabsf(xi) < 0.5f && fabsf(xr) < 0.5f && fabsf(xc) < 0.5f) {
                ok = true;
                break;
            }
            const float lim = (float)(INT32_MAX / 3);
            if (!(fabsf(xi) <= lim && fabsf(xr) <= lim && fabsf(xc) <= lim)) break;
            c += (int)rintf(xc);
            r += (int)rintf(xr);
            layer += (int)rintf(xi);
            if (layer < 1 || layer > kSiftLayers || c < kSiftBorder || c >= cols - kSiftBorder || r < kSiftBorder || r >= rows - kSiftBorder)
                break;
        }
        if (!ok) continue;
        const float* img = dog + layer * plane;
        const size_t o = (size_t)r * cols + c;
        const float t = dx * xc + dy * xr + ds * xi;
        const float contr = img[o] * img_scale + t * 0.5f;
        if (fabsf(contr) * (float)kSiftLayers < 0.04f) continue;
        const float v2 = img[o] * 2.0f;
        const float dxx = (img[o + 1] + img[o - 1] - v2) * second_scale;
        const float dyy = (img[o + cols] + img[o - cols] - v2) * second_scale;
        const float dxy = (img[o + cols + 1] - img[o + cols - 1] - img[o - cols + 1] + img[o - cols - 1]) * cross_scale;
        const float tr = dxx + dyy, det = dxx * dyy - dxy * dxy;
        if (det <= 0.0f || tr * tr * 10.0f >= 121.0f * det) continue;
        const float scale = (float)(1 << octave);
        const float px = ((float)c + xc) * scale * 0.5f, py = ((float)r + xr) * scale * 0.5f;
        const int ix = (int)px, iy = (int)py;                     // astype(int): truncation
        if (ix < 0 || iy < 0 || ix >= (int)W || iy >= (int)H) continue;
        points[(size_t)ix * H + iy] = 1;                          // [x][y], the reference's interest_regions[POI[:,0], POI[:,1]]
        atomicAdd(count, 1u);
    }
}

// max over [i - lo, i + hi] along one axis of a [X][Y] byte mask; axis 1 (contiguous) or 0
__global__ void __launch_bounds__(kSiftBlock) k_sift_dilate(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, uint32_t X, uint32_t Y,
                                                            int axis, int lo, int hi) {
    const uint32_t n = X * Y;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int x = (int)(i / Y), y = (int)(i % Y);
        const int p = axis ? y : x, len = axis ? (int)Y : (int)X;
        const int a = max(p - lo, 0), b = min(p + hi, len - 1);
        uint8_t m = 0;
        for (int q = a; q <= b; q++) m = max(m, axis ? src[(size_t)x * Y + q] : src[(size_t)q * Y + y]);
        dst[i] = m;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
struct SiftGeometry {
    int n_octaves;
    int rows[kSiftMaxOctaves], cols[kSiftMaxOctaves];
    size_t offset[kSiftMaxOctaves];      // bytes: the octave's 6 Gaussian then 5 DoG planes
    size_t scratch;                      // two planes of octave 0 (upsampled base, blur intermediate)
    size_t dilate_tmp;                   // H * W bytes
    size_t total;
};

static bool sift_geometry(uint32_t H, uint32_t W, SiftGeometry& g) {
    if (H < 8 || W < 8 || H > 16384 || W > 16384) return false;
    if ((uint64_t)4 * H * W * kSiftDog >= ((uint64_t)1 << 32)) return false;     // 32-bit element counts of octave 0's DoG planes
    const int r0 = 2 * (int)H, c0 = 2 * (int)W;
    g.n_octaves = (int)lrint(std::log((double)std::min(r0, c0)) / std::log(2.0) - 2) + 1;
    if (g.n_octaves < 1 || g.n_octaves > kSiftMaxOctaves) return false;
    size_t off = 0;
    int rows = r0, cols = c0;
    for (int o = 0; o < g.n_octaves; o++) {
        if (rows < 1 || cols < 1) return false;
        g.rows[o] = rows;
        g.cols[o] = cols;
        g.offset[o] = off;
        off += (size_t)(kSiftGauss + kSiftDog) * rows * cols * sizeof(float);
        rows /= 2;
        cols /= 2;
    }
    g.scratch = off;
    off += 2 * (size_t)r0 * c0 * sizeof(float);
    g.dilate_tmp = off;
    off += ((size_t)H * W + 255) & ~(size_t)255;
    g.total = off;
    return true;
}

// getGaussianKernel(round(8 sigma + 1) | 1, sigma, CV_32F): float64 weights, normalised, then float32
static bool sift_taps(double sigma, SiftTaps& t) {
    const int n = ((int)lrint(sigma * 8 + 1)) | 1;
    if (n > kSiftMaxTaps) return false;
    double w[kSiftMaxTaps], sum = 0;
    const double scale2x = -0.5 / (sigma * sigma);
    for (int i = 0; i < n; i++) {
        const double x = i - (n - 1) * 0.5;
        w[i] = std::exp(scale2x * x * x);
        sum += w[i];
    }
    sum = 1.0 / sum;
    for (int i = 0; i < n; i++) t.w[i] = (float)(w[i] * sum);
    t.n = n;
    return true;
}

static uint32_t sift_blocks(size_t n) {
    const size_t b = (n + kSiftBlock - 1) / kSiftBlock;
    return (uint32_t)(b > 8192 ? 8192 : (b ? b : 1));
}

static void sift_blur(const float* src, float* tmp, float* dst, int rows, int cols, const SiftTaps& taps, hipStream_t s) {
    const dim3 grid(div_up((uint32_t)cols, kSiftBlock), (uint32_t)rows);
    k_sift_blur_rows<<<grid, kSiftBlock, 0, s>>>(src, tmp, rows, cols, taps);
    k_sift_blur_cols<<<grid, kSiftBlock, 0, s>>>(tmp, dst, rows, cols, taps);
}

}  // namespace ngp

using namespace ngp;

extern "C" {

size_t ngp_sift_workspace(uint32_t H, uint32_t W) {
    SiftGeometry g;
    return sift_geometry(H, W, g) ? g.total : 0;
}

size_t ngp_sift_layer_offset(uint32_t H, uint32_t W, int octave, int index) {
    SiftGeometry g;
    if (!sift_geometry(H, W, g) || octave < 0 || octave >= g.n_octaves || index < 0 || index >= kSiftGauss + kSiftDog) return (size_t)-1;
    return g.offset[octave] + (size_t)index * g.rows[octave] * g.cols[octave] * sizeof(float);
}

int ngp_sift_octaves(uint32_t H, uint32_t W) {
    SiftGeometry g;
    return sift_geometry(H, W, g) ? g.n_octaves : 0;
}

int ngp_sift_interest_mask(const uint8_t* rgb, uint32_t H, uint32_t W, uint32_t kernel_size, uint32_t dil_iter, uint8_t* points,
                           uint8_t* mask, uint32_t* count, void* workspace, size_t workspace_bytes, ngp_stream_t stream) {
    SiftGeometry g;
    NGP_REQUIRE(sift_geometry(H, W, g), "sift_interest_mask: H and W must be in [8, 16384] with H * W < 2^32 / 20 (got %u x %u)", H, W);
    NGP_REQUIRE(rgb && points && mask && count, "sift_interest_mask: null pointer");
    NGP_REQUIRE(kernel_size >= 1 && kernel_size <= 255 && dil_iter <= 255, "sift_interest_mask: kernel_size in [1, 255], dil_iter <= 255");
    int rc = check_workspace("sift_interest_mask", workspace, workspace_bytes, g.total, 4);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    Carver c(workspace);
    char* const ws = c.take<char>(g.total);      // SiftGeometry's offsets are into this
    float* base = reinterpret_cast<float*>(ws + g.scratch);
    float* tmp = base + (size_t)g.rows[0] * g.cols[0];
    uint8_t* dtmp = reinterpret_cast<uint8_t*>(ws + g.dilate_tmp);
    ProfScope prof("sift_interest_mask", s, (double)H * W);

    // per-layer sigmas (createInitialImage / buildGaussianPyramid): 1.6 at layer 0, then the increments to 1.6 * 2^(i/3)
    const double sigma = 1.6;
    SiftTaps taps[kSiftGauss], taps0;
    bool fits = sift_taps(std::sqrt(std::max(sigma * sigma - 1.0, 0.01)), taps0);
    const double k = std::pow(2.0, 1.0 / kSiftLayers);
    for (int i = 1; i < kSiftGauss; i++) {
        const double prev = std::pow(k, (double)(i - 1)) * sigma, total = prev * k;
        fits = fits && sift_taps(std::sqrt(total * total - prev * prev), taps[i]);
    }
    NGP_REQUIRE(fits, "sift_interest_mask: Gaussian kernel longer than %d taps", kSiftMaxTaps);

    (void)hipMemsetAsync(points, 0, (size_t)H * W, s);
    (void)hipMemsetAsync(count, 0, sizeof(uint32_t), s);
    const size_t n0 = (size_t)g.rows[0] * g.cols[0];
    k_sift_base<<<sift_blocks(n0), kSiftBlock, 0, s>>>(rgb, H, W, base);
    for (int o = 0; o < g.n_octaves; o++) {
        const int rows = g.rows[o], cols = g.cols[o];
        const size_t plane = (size_t)rows * cols;
        float* gauss = reinterpret_cast<float*>(ws + g.offset[o]);
        float* dog = gauss + kSiftGauss * plane;
        if (o == 0) {
            sift_blur(base, tmp, gauss, rows, cols, taps0, s);
        } else {
            const float* prev3 = reinterpret_cast<const float*>(ws + g.offset[o - 1]) + (size_t)kSiftLayers * g.rows[o - 1] * g.cols[o - 1];
            k_sift_decimate<<<sift_blocks(plane), kSiftBlock, 0, s>>>(prev3, g.cols[o - 1], gauss, rows, cols);
        }
        for (int i = 1; i < kSiftGauss; i++) sift_blur(gauss + (i - 1) * plane, tmp, gauss + i * plane, rows, cols, taps[i], s);
        k_sift_dog<<<sift_blocks(plane * kSiftDog), kSiftBlock, 0, s>>>(gauss, dog, (uint32_t)plane);
        const int ir = rows - 2 * kSiftBorder, ic = cols - 2 * kSiftBorder;
        if (ir > 0 && ic > 0)
            k_sift_extrema<<<sift_blocks((size_t)kSiftLayers * ir * ic), kSiftBlock, 0, s>>>(dog, rows, cols, o, H, W, points, count);
    }
    // cv2.dilate(points, ones(k, k), iterations=dil_iter): anchor k/2, the window [p - anchor * iter, p + (k - 1 - anchor) * iter]
    const int lo = (int)(kernel_size / 2) * (int)dil_iter, hi = (int)(kernel_size - 1 - kernel_size / 2) * (int)dil_iter;
    k_sift_dilate<<<sift_blocks((size_t)H * W), kSiftBlock, 0, s>>>(points, dtmp, W, H, 1, lo, hi);
    k_sift_dilate<<<sift_blocks((size_t)H * W), kSiftBlock, 0, s>>>(dtmp, mask, W, H, 0, lo, hi);
    return check_launch("sift_interest_mask");
}

}  // extern "C"
