// occupancy.hip -- the derived copies of the occupancy bits (occupancy.hpp): the kernels that build them and the host helper that decides
// whether a grid has them and launches the build, for march_rays_train, ngp_build_occupancy_lin and the render loop with their own caps.
#include "occupancy.hpp"

namespace ngp {

// one bit per aligned 8-byte word (= 64 Morton-consecutive cells = one 4x4x4 block) of the occupancy bitfield
__global__ void __launch_bounds__(256) k_build_coarse(const unsigned long long* __restrict__ bitfield64, uint32_t n_words,
                                                       unsigned long long* __restrict__ coarse) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const bool any = i < n_words && bitfield64[i] != 0ull;
    const unsigned long long m = __ballot(any);
    if ((threadIdx.x & 63) == 0 && i < n_words) coarse[i >> 6] = m;
}

// Linear re-layout of the occupancy bits (power-of-two H): bit (level, z, y, x) of `lin` = bit level*H^3 + morton3D(x, y, z)
// of the bitfield (raymarching.cu:381).  One thread per output word (32 consecutive x).
__global__ void __launch_bounds__(256) k_build_linear(const uint8_t* __restrict__ bitfield, uint32_t cascade, uint32_t logH,
                                                      uint32_t* __restrict__ lin) {
    const uint32_t w = blockIdx.x * 256 + threadIdx.x;
    const uint32_t words_per_level = 1u << (3 * logH - 5);
    if (w >= cascade * words_per_level) return;
    const uint32_t level = w / words_per_level, c0 = (w % words_per_level) * 32;
    const uint32_t H1 = (1u << logH) - 1;
    const uint32_t x0 = c0 & H1, y = (c0 >> logH) & H1, z = c0 >> (2 * logH);
    const uint32_t n = H1 + 1 < 32 ? H1 + 1 : 32;   // H < 32: a word spans several rows
    uint32_t out = 0;
    for (uint32_t i = 0; i < 32; i++) {
        const uint32_t c = c0 + i;
        const uint32_t xi = n == 32 ? x0 + i : (c & H1), yi = n == 32 ? y : ((c >> logH) & H1), zi = n == 32 ? z : (c >> (2 * logH));
        const uint32_t m = (level << (3 * logH)) + morton3D_cell(xi, yi, zi);
        out |= (uint32_t)((bitfield[m >> 3] >> (m & 7u)) & 1u) << i;
    }
    lin[w] = out;
}

// coarse bits in the same x-fastest order: bit (level, bz, by, bx) = any cell of the 4x4x4 block set
__global__ void __launch_bounds__(256) k_build_coarse_linear(const unsigned long long* __restrict__ bitfield64, uint32_t cascade, uint32_t logH,
                                                             unsigned long long* __restrict__ coarse) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const uint32_t lb = logH - 2, per_level = 1u << (3 * lb), B1 = (1u << lb) - 1;
    bool any = false;
    if (i < cascade * per_level) {
        const uint32_t level = i / per_level, r = i % per_level;
        const uint32_t bx = r & B1, by = (r >> lb) & B1, bz = r >> (2 * lb);
        any = bitfield64[(size_t)level * per_level + morton3D_cell(bx, by, bz)] != 0ull;   // 64 Morton-consecutive cells = one block
    }
    const unsigned long long m = __ballot(any);
    if ((threadIdx.x & 63) == 0 && i < cascade * per_level) coarse[i >> 6] = m;
}

static uint32_t log2_of(uint32_t H) {
    uint32_t logH = 0;
    while ((1u << logH) < H) logH++;
    return logH;
}

// (the C and H ranges are the entry points' own: ngp_render_rays and ngp_march_rays_train refuse anything else before they ask)
bool occupancy_lin_fits(uint32_t C, uint32_t H, const uint8_t* grid, size_t lin_cap_bytes, size_t coarse_cap_bytes) {
    if (C < 1 || C > 8 || H < 8 || H > 1024 || (H & (H - 1)) || ((uintptr_t)grid & 7)) return false;
    const size_t cells = (size_t)C * H * H * H;
    return cells % 4096 == 0 && cells / 8 <= lin_cap_bytes && cells / 64 / 8 <= coarse_cap_bytes;
}

OccupancyLin occupancy_lin_view(uint32_t C, uint32_t H, const void* lin, const void* coarse) {
    const size_t cells = (size_t)C * H * H * H;
    return {(const uint32_t*)lin, (const uint32_t*)coarse, (uint32_t)(cells / 64 / 32), log2_of(H)};
}

OccupancyLin build_occupancy_lin(const uint8_t* grid, uint32_t C, uint32_t H, void* lin_out, void* coarse_out, hipStream_t stream) {
    const size_t cells = (size_t)C * H * H * H;
    const OccupancyLin ol = occupancy_lin_view(C, H, lin_out, coarse_out);
    k_build_linear<<<div_up((uint32_t)(cells / 32), 256), 256, 0, stream>>>(grid, C, ol.logH, (uint32_t*)lin_out);
    k_build_coarse_linear<<<div_up((uint32_t)(cells / 64), 256), 256, 0, stream>>>((const unsigned long long*)grid, C, ol.logH,
                                                                                   (unsigned long long*)coarse_out);
    return ol;
}

}  // namespace ngp
