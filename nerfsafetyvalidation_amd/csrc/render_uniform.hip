// render_uniform.hip -- NeRFRenderer.run (nerf/renderer.py:125-258), the renderer without an occupancy grid: uniform samples along
// every ray, optionally the importance resampling of sample_pdf (:12-46, :172-204), and the vector-Jacobian product with respect to
// the rays that the state estimator differentiates (nav/estimator_helpers.py:191-225).  The network comes from fused_net.hpp.
#include <stdlib.h>

#include "fused_net.hpp"
#include "wave_ops.hpp"

namespace ngp {

// ------------------------------------------------------------------------------------------
// The steps of NeRFRenderer.run's sampling and compositing (nerf/renderer.py:150-244) that the kernels below share, each stated once.
// ------------------------------------------------------------------------------------------
struct RaySetup {
    float ox, oy, oz, dx, dy, dz, near, span, sample_dist;
    __device__ __forceinline__ float z_at(const float* lin, uint32_t i) const { return near + span * lin[i]; }   // :150 (mul, then add: eager torch does not fuse)
    __device__ __forceinline__ float depth_ratio(float zv) const { return (zv - near) / span; }   // :227; 0/0 = NaN for rays that miss the box
};
// ORIGIN = false: a kernel that evaluates no position (rays_o is not read)
template <bool ORIGIN = true>
__device__ __forceinline__ RaySetup load_ray(const float* rays_o, const float* rays_d, const float* nears, const float* fars, uint32_t ray, uint32_t T) {
    float ox = 0, oy = 0, oz = 0;
    if constexpr (ORIGIN) { ox = rays_o[(size_t)ray * 3]; oy = rays_o[(size_t)ray * 3 + 1]; oz = rays_o[(size_t)ray * 3 + 2]; }
    const float dx = rays_d[(size_t)ray * 3], dy = rays_d[(size_t)ray * 3 + 1], dz = rays_d[(size_t)ray * 3 + 2];
    const float near = nears[ray], far = fars[ray], span = far - near;
    return {ox, oy, oz, dx, dy, dz, near, span, span * (1.0f / (float)T)};      // :153 (tensor / Python scalar on the GPU = multiplication with the fp32 reciprocal)
}
__device__ __forceinline__ void sample_point(const RaySetup& r, float zv, float lo, float hi, float& x, float& y, float& z) {   // :159-160, :181-182
    x = clampf(r.ox + r.dx * zv, lo, hi);
    y = clampf(r.oy + r.dy * zv, lo, hi);
    z = clampf(r.oz + r.dz * zv, lo, hi);
}
__device__ __forceinline__ float sample_alpha(float delta, float density_scale, float sigma) { return 1.0f - expf(((-delta) * density_scale) * sigma); }   // :208
__device__ __forceinline__ float alpha_survival(float alpha) { return (1.0f - alpha) + 1e-15f; }                                                       // :209
__device__ __forceinline__ bool weight_masked(float w) { return w > 1e-4f; }      // :216, the samples whose colour the reference evaluates
// a ray stops where its transmittance falls below this: everything further down is weighted by less, below fp32 resolution of the
// O(1) sums
constexpr float kSpentTransmittance = 1e-10f;

// cumprod(1 - alpha + 1e-15) of :209-210 over a tile of W samples, lane = sample: the transmittance in front of the lane's sample, given
// `carry` = the product over the earlier tiles; tile_product is what the tile multiplies into carry
// (the scan of k_trans_weights' chunk in sampling.hip, not shared with it: there the chunk also forms p from its arrays and is always
// 64 wide; here the callers form p, W is 16 or 64, and carry moves on in the caller, which may stop the ray on it first.  The shift
// and the broadcast stay written out: with the header's shifted_in / last_lane the compiler schedules the callers differently.)
template <int W>
__device__ __forceinline__ float tile_transmittance(float p, float carry, uint32_t l, float& tile_product) {
    const float incl = scan_inclusive<MulOp, W>(p, l);
    const float excl = __shfl_up(incl, 1, W);
    tile_product = __shfl(incl, W - 1, W);
    return carry * (l == 0 ? 1.0f : excl);
}

// colour of a tile's samples from the sigma net's outputs s16, evaluated (by the whole wave) only when `any` holds for some lane -- the
// reference's masked colour query (:216-218); lanes that are not `masked` read zero
template <class NET>
__device__ __forceinline__ void masked_color(const NetArgs& na, const char* Wlds, uint32_t lane, const RaySetup& r, const typename NET::geo_t (&s16)[4],
                                             bool any, bool masked, float& cr, float& cg, float& cb) {
    cr = 0; cg = 0; cb = 0;
    if (__ballot(any) != 0ull) {
        NET::color(na, Wlds, lane, r.dx, r.dy, r.dz, s16, cr, cg, cb);
        if (!masked) { cr = 0; cg = 0; cb = 0; }
    }
}

// one of the per-sample rows the reference returns for the last ray chunk
__device__ __forceinline__ void dump_sample(float* sigmas, float* rgbs, size_t row, float sigma, float cr, float cg, float cb) {
    sigmas[row] = sigma;
    rgbs[row * 3] = cr; rgbs[row * 3 + 1] = cg; rgbs[row * 3 + 2] = cb;
}

// a lane's partial sums of the four per-ray outputs
struct RaySums {
    float ws, dep, r, g, b, agg;
    __device__ __forceinline__ void add(const RaySetup& ray, float zv, float w, float sigma, float cr, float cg, float cb) {
        ws += w;
        const float qz = ray.depth_ratio(zv);
        dep += w * (qz != qz ? qz : fminf(1.0f, fmaxf(0.0f, qz)));                   // torch.clamp keeps the NaN, as the reference does
        r += w * cr; g += w * cg; b += w * cb;                                       // :231
        agg += w * sigma;                                                            // :244
    }
    __device__ __forceinline__ void reduce16() {
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) {      // six wave_sum<16> (wave_ops.hpp) interleaved step by step; as six calls the callers are scheduled differently
            ws += __shfl_xor(ws, off, 16); dep += __shfl_xor(dep, off, 16); agg += __shfl_xor(agg, off, 16);
            r += __shfl_xor(r, off, 16); g += __shfl_xor(g, off, 16); b += __shfl_xor(b, off, 16);
        }
    }
    __device__ __forceinline__ void store(uint32_t ray, float* weights_sum, float* depth, float* image, float* aggregated_density) const {
        weights_sum[ray] = ws; depth[ray] = dep; aggregated_density[ray] = agg;
        image[(size_t)ray * 3] = r; image[(size_t)ray * 3 + 1] = g; image[(size_t)ray * 3 + 2] = b;
    }
};

// ray -> (group of sixteen, slot in the group) as the across-ray kernels form their groups: 1x16 strips, or 4x4-pixel blocks of row-major
// frames `frame_w` wide (frame_w % 4 == 0, N % (4 * frame_w) == 0: checked on the host)
__device__ __forceinline__ void ray_slot(uint32_t ray, uint32_t frame_w, uint32_t& grp, uint32_t& c) {
    if (frame_w) {
        const uint32_t row = ray / frame_w, col = ray - row * frame_w;
        grp = (row >> 2) * (frame_w >> 2) + (col >> 2);
        c = (row & 3u) * 4u + (col & 3u);
    } else {
        grp = ray >> 4;
        c = ray & 15u;
    }
}
// (group, slot) -> ray, the inverse of ray_slot; the slots past the last ray of a ragged last group give a ray >= N
__device__ __forceinline__ uint32_t group_ray(uint32_t grp, uint32_t c, uint32_t frame_w) {
    uint32_t ray = grp * 16 + c;
    if (frame_w) {
        const uint32_t bpr = frame_w >> 2, by = grp / bpr, bx = grp - by * bpr;
        ray = (by * 4 + (c >> 2)) * frame_w + bx * 4 + (c & 3);
    }
    return ray;
}

// ------------------------------------------------------------------------------------------
// NeRFRenderer.run, uniform sampling without upsampling (nerf/renderer.py:125-258): the path validate.py -O executes
// (cuda_ray = False, num_steps = 512).  One wave walks one ray 16 samples at a time: positions from the linspace table,
// fused hash-grid + sigma net, in-wave transmittance scan (alphas * cumprod(1 - alphas + 1e-15), :206-210), colour net only
// for tiles that contain a sample with weight > 1e-4 (the reference's masked colour query, :216-218), running sums of
// weights, depth, colour and weights * sigma.  None of the reference's [N, T, *] intermediates exists in memory; the
// per-sample sigmas / rgbs it returns for the LAST ray chunk are written only for rays >= dump_begin.
// ------------------------------------------------------------------------------------------
template <class NET>
__global__ void __launch_bounds__(256, NET::kF32 ? 2 : 4) k_render_uniform(NetArgs na, GridLevels lv, const float* __restrict__ rays_o,
                                                           const float* __restrict__ rays_d, const float* __restrict__ nears,
                                                           const float* __restrict__ fars, uint32_t N, uint32_t T,
                                                           const float* __restrict__ lin, float* __restrict__ weights_sum,
                                                           float* __restrict__ depth, float* __restrict__ image,
                                                           float* __restrict__ aggregated_density, uint32_t dump_begin,
                                                           float* __restrict__ sigmas, float* __restrict__ rgbs, float aabb_lo, float aabb_hi) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const char* Wlds = smem;
    LevelTab* lt = reinterpret_cast<LevelTab*>(smem + NET::w_bytes(na));
    stage_block(na, lv, smem, lt, NET::w_bytes(na));
    const uint32_t lane = threadIdx.x & 63, c = lane & 15;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t ray = wave; ray < N; ray += n_waves) {
        const RaySetup r = load_ray(rays_o, rays_d, nears, fars, ray, T);
        const bool dump = sigmas != nullptr && ray >= dump_begin;
        float carry = 1.0f;                                                          // cumprod of (1 - alpha + 1e-15) over earlier tiles
        RaySums sums = {};                                                           // per-lane partial sums (lanes 0..15)
        for (uint32_t i0 = 0; i0 < T; i0 += 16) {
            const uint32_t idx = i0 + c;
            const bool valid = idx < T;
            const uint32_t ii = valid ? idx : T - 1;
            const float zv = r.z_at(lin, ii);
            float x, y, z;
            sample_point(r, zv, aabb_lo, aabb_hi, x, y, z);
            float sigma;
            typename NET::geo_t s16[4];
            NET::density(na, Wlds, *lt, lane, x, y, z, sigma, s16);
            // ---- lanes 0..15 hold sigma of samples i0..i0+15 (the other quarters compute along with them; only lane < 16 results are used)
            const float z_next = (ii + 1 < T) ? r.z_at(lin, ii + 1) : 0.0f;
            const float delta = (ii + 1 < T) ? z_next - zv : r.sample_dist;         // :206-207
            const float alpha = valid ? sample_alpha(delta, na.density_scale, sigma) : 0.0f;
            float tile_product;
            const float Tr = tile_transmittance<16>(alpha_survival(alpha), carry, c, tile_product);
            const float w = alpha * Tr;                                              // :210
            const bool masked = valid && weight_masked(w);
            float cr, cg, cb;
            masked_color<NET>(na, Wlds, lane, r, s16, masked && lane < 16, masked, cr, cg, cb);
            if (lane < 16 && valid) {
                sums.add(r, zv, w, sigma, cr, cg, cb);
                if (dump) dump_sample(sigmas, rgbs, (size_t)(ray - dump_begin) * T + idx, sigma, cr, cg, cb);
            }
            // (lanes 16..63 evaluate other rows of the sigma net in `sigma`: only quarter 0's transmittance is the ray's.  The exit
            //  below must be taken by the WHOLE wave at once -- a quarter that left early would stop gathering its levels -- hence
            //  the broadcast of lane 0's value)
            carry = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(carry * tile_product)));
            if (!dump && carry < kSpentTransmittance) break;
        }
        sums.reduce16();
        if (lane == 0) sums.store(ray, weights_sum, depth, image, aggregated_density);
    }
}

// The same computation with the samples of a tile taken ACROSS sixteen neighbouring rays (consecutive pixels of a row) at one
// depth index instead of along one ray: neighbouring pixels at equal depth are ~4x closer than consecutive samples of a ray
// (d / 1111 against span / 512), so the sixteen samples of a tile share cells -- and cache lines -- down to finer levels, as the
// tiles of k_render_iter do; and the transmittance becomes a per-lane running product (no in-tile scan).  Lane c of every quarter
// walks ray 16 g + c; a ray whose transmittance is spent idles until the last ray of its group is (neighbouring pixels end at
// similar depths).  Per-sample granularity of the stop: a ray ends after the first sample that leaves carry < 1e-10.
constexpr uint32_t kUniformX16MinRays = 65536;      // (measured: section 4 of DESIGN.md)
template <class NET>
__global__ void __launch_bounds__(256, NET::kF32 ? 2 : 4) k_render_uniform_x16(NetArgs na, GridLevels lv, const float* __restrict__ rays_o,
                                                               const float* __restrict__ rays_d, const float* __restrict__ nears,
                                                               const float* __restrict__ fars, uint32_t N, uint32_t T,
                                                               const float* __restrict__ lin, float* __restrict__ weights_sum,
                                                               float* __restrict__ depth, float* __restrict__ image,
                                                               float* __restrict__ aggregated_density, uint32_t dump_begin,
                                                               float* __restrict__ sigmas, float* __restrict__ rgbs, float aabb_lo, float aabb_hi,
                                                               uint32_t frame_w, unsigned long long* __restrict__ stamps) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const char* Wlds = smem;
    LevelTab* lt = reinterpret_cast<LevelTab*>(smem + NET::w_bytes(na));
    stage_block(na, lv, smem, lt, NET::w_bytes(na));
    const uint32_t lane = threadIdx.x & 63, c = lane & 15;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    const uint32_t n_groups = (N + 15) / 16;
    for (uint32_t grp = wave; grp < n_groups; grp += n_waves) {
        const uint32_t ray_raw = group_ray(grp, c, frame_w);
        const bool live = ray_raw < N;
        const uint32_t ray = live ? ray_raw : N - 1;      // (slots past the last ray read the last ray)
        const RaySetup r = load_ray(rays_o, rays_d, nears, fars, ray, T);
        const bool dump = live && sigmas != nullptr && ray >= dump_begin;
        float carry = 1.0f;
        RaySums sums = {};
        bool running = live;
        uint32_t n_iter = 0, n_counted = 0;
        float zv = r.z_at(lin, 0);
        for (uint32_t i = 0; i < T; i++) {
            n_iter++;
            const float z_next = (i + 1 < T) ? r.z_at(lin, i + 1) : 0.0f;
            float x, y, z;
            sample_point(r, zv, aabb_lo, aabb_hi, x, y, z);
            float sigma;
            typename NET::geo_t s16[4];
            NET::density(na, Wlds, *lt, lane, x, y, z, sigma, s16);
            // (quarter 0 holds sigma; the other quarters evaluate other rows of the sigma net in `sigma` and follow quarter 0's
            //  decisions through the ballots below)
            const float delta = (i + 1 < T) ? z_next - zv : r.sample_dist;           // :206-207
            const float alpha = sample_alpha(delta, na.density_scale, sigma);
            const float w = alpha * carry;                                           // :210
            const bool counted = running && lane < 16;
            const bool masked = counted && weight_masked(w);
            float cr, cg, cb;
            masked_color<NET>(na, Wlds, lane, r, s16, masked, masked, cr, cg, cb);
            if (counted) {
                n_counted++;
                sums.add(r, zv, w, sigma, cr, cg, cb);
                if (dump) dump_sample(sigmas, rgbs, (size_t)(ray - dump_begin) * T + i, sigma, cr, cg, cb);
                carry *= alpha_survival(alpha);
                if (!dump && carry < kSpentTransmittance) running = false;
            }
            if (__ballot(running && lane < 16) == 0ull) break;
            zv = z_next;
        }
        if (lane < 16 && live) sums.store(ray, weights_sum, depth, image, aggregated_density);
        if (stamps) {    // diagnostics (ngp_debug_set_stamps): depth indices walked by the group x 16 lanes, and those that carried a running ray
            const uint32_t mine = wave_sum<16>(lane < 16 ? n_counted : 0u);
            if (lane == 0) { atomicAdd(stamps + 12, (unsigned long long)n_iter * 16ull); atomicAdd(stamps + 13, (unsigned long long)mine); }
        }
    }
}

// The density pass alone, tiles across sixteen rays as in k_render_uniform_x16 (fp16 network): sigma of T samples of every ray, no
// colour, no sums, no early stop -- the two density launches of the large-batch importance resampling.  z_in = NULL: the uniform depths;
// else the resampled ones.  z_in, sigmas and geo_out are GROUP-major, [group][sample][ray of the group]: the sixteen rays' values of
// one sample are 64 (sigma, depth) or 512 (geo) contiguous bytes.
template <class NET>
__global__ void __launch_bounds__(256, 4) k_density_x16(NetArgs na, GridLevels lv, const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                        const float* __restrict__ nears, const float* __restrict__ fars, uint32_t N, uint32_t T,
                                                        const float* __restrict__ lin, const float* __restrict__ z_in, float* __restrict__ sigmas,
                                                        _Float16* __restrict__ geo_out, float aabb_lo, float aabb_hi, uint32_t frame_w) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const char* Wlds = smem;
    LevelTab* lt = reinterpret_cast<LevelTab*>(smem + NET::w_bytes(na));
    stage_block(na, lv, smem, lt, NET::w_bytes(na));
    const uint32_t lane = threadIdx.x & 63, c = lane & 15;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    const uint32_t n_groups = (N + 15) / 16;
    for (uint32_t grp = wave; grp < n_groups; grp += n_waves) {
        const uint32_t ray_raw = group_ray(grp, c, frame_w);
        const bool live = ray_raw < N;
        const uint32_t ray = live ? ray_raw : N - 1;      // (slots past the last ray read the last ray)
        const RaySetup r = load_ray(rays_o, rays_d, nears, fars, ray, T);
        for (uint32_t i = 0; i < T; i++) {
            const size_t at = ((size_t)grp * T + i) * 16 + c;
            const float zs = z_in ? (live ? z_in[at] : 0.0f) : r.z_at(lin, i);    // (slots past the last ray were never written)
            float x, y, z;
            sample_point(r, zs, aabb_lo, aabb_hi, x, y, z);
            float sigma;
            _Float16 s16[4];
            NET::density(na, Wlds, *lt, lane, x, y, z, sigma, s16);
            if (lane < 16) sigmas[at] = sigma;
            // the sigma net's sixteen outputs (sigma's pre-activation + the 15 geometry features), 4 per quarter: what the colour
            // net of the compositing launch needs of this sample
            if (geo_out) {
                half4 h4 = {s16[0], s16[1], s16[2], s16[3]};
                *reinterpret_cast<half4*>(geo_out + at * 16 + (lane >> 4) * 4) = h4;
            }
        }
    }
}

// The last launch of the large-batch importance resampling: merge + compositing ACROSS the sixteen rays of a group.  Every lane walks
// its ray's two ascending runs -- the T uniform depths (computed) and the U resampled ones (group-major scratch) -- with two
// pointers (coarse first on ties: the order k_merge_sorted / torch.sort of the concatenation give), so the merge costs no search and
// no LDS; sigma and, for tiles that hold a sample with weight > 1e-4, the sigma net's outputs come from the density launches'
// scratch, and only the colour net is evaluated here.  Transmittance is a per-lane running product, as in k_render_uniform_x16.
template <int MODE>
__global__ void __launch_bounds__(256, 4) k_composite_merged_x16(NetArgs na, GridLevels lv, const float* __restrict__ rays_d,
                                                                 const float* __restrict__ nears, const float* __restrict__ fars, uint32_t N,
                                                                 uint32_t T, uint32_t U, const float* __restrict__ lin,
                                                                 const float* __restrict__ sc, const float* __restrict__ zf,
                                                                 const float* __restrict__ sf, const _Float16* __restrict__ geo_c,
                                                                 const _Float16* __restrict__ geo_f, float* __restrict__ weights_sum,
                                                                 float* __restrict__ depth, float* __restrict__ image,
                                                                 float* __restrict__ aggregated_density, uint32_t dump_begin,
                                                                 float* __restrict__ sigmas, float* __restrict__ rgbs, uint32_t frame_w) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    _Float16* Wlds = reinterpret_cast<_Float16*>(smem);
    LevelTab* lt = reinterpret_cast<LevelTab*>(smem + net_w_bytes_f16(na));
    stage_block(na, lv, Wlds, lt, net_w_bytes_f16(na));
    const uint32_t lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    const uint32_t n_groups = (N + 15) / 16, Tm = T + U;
    const float inf = __builtin_huge_valf();
    for (uint32_t grp = wave; grp < n_groups; grp += n_waves) {
        const uint32_t ray_raw = group_ray(grp, c, frame_w);
        const bool live = ray_raw < N;
        const uint32_t ray = live ? ray_raw : N - 1;      // (slots past the last ray read the last ray)
        const RaySetup r = load_ray<false>(nullptr, rays_d, nears, fars, ray, T);
        const bool dump = live && sigmas != nullptr && ray >= dump_begin;
        const size_t cbase = (size_t)grp * T * 16 + c, fbase = (size_t)grp * U * 16 + c;
        uint32_t i = 0, j = 0;                                                       // next coarse / fine sample of this lane's ray
        float zci = r.z_at(lin, 0), zfj = live ? zf[fbase] : 0.0f;                   // (slots past the last ray were never written)
        float carry = 1.0f;
        RaySums sums = {};
        bool running = live;
        for (uint32_t m = 0; m < Tm; m++) {
            const bool from_c = zci <= zfj;                                          // (an exhausted run holds +inf; both cannot be)
            const float zv = from_c ? zci : zfj;
            const size_t at = from_c ? cbase + (size_t)i * 16 : fbase + (size_t)j * 16;
            const float sigma = (from_c ? sc : sf)[at];
            const _Float16* gp = (from_c ? geo_c : geo_f) + at * 16 + q * 4;
            if (from_c) { i++; zci = i < T ? r.z_at(lin, i) : inf; }
            else { j++; zfj = j < U ? (live ? zf[fbase + (size_t)j * 16] : 0.0f) : inf; }
            const float z_next = zci <= zfj ? zci : zfj;
            const float delta = (m + 1 < Tm) ? z_next - zv : r.sample_dist;          // :206-207
            const float alpha = sample_alpha(delta, na.density_scale, sigma);
            const float w = alpha * carry;                                           // :210
            const bool counted = running && lane < 16;
            const bool masked = counted && weight_masked(w);
            float cr = 0, cg = 0, cb = 0;
            if (__ballot(masked) != 0ull) {      // (as masked_color does, on the sigma net's outputs that the density launches kept)
                const half4 h4 = *reinterpret_cast<const half4*>(gp);
                const _Float16 s16[4] = {h4[0], h4[1], h4[2], h4[3]};
                net_color(na, Wlds, lane, r.dx, r.dy, r.dz, s16, cr, cg, cb);
                if (!masked) { cr = 0; cg = 0; cb = 0; }
            }
            if (counted) {
                sums.add(r, zv, w, sigma, cr, cg, cb);
                if (dump) dump_sample(sigmas, rgbs, (size_t)(ray - dump_begin) * Tm + m, sigma, cr, cg, cb);
                carry *= alpha_survival(alpha);
                if (!dump && carry < kSpentTransmittance) running = false;
            }
            if (__ballot(running && lane < 16) == 0ull) break;
        }
        if (lane < 16 && live) sums.store(ray, weights_sum, depth, image, aggregated_density);
    }
}

// ------------------------------------------------------------------------------------------
// NeRFRenderer.run WITH the NeRF-style importance resampling (nerf/renderer.py:172-204, sample_pdf :12-46), evaluation mode
// (`det`: the u of the inverse-CDF draw are the fixed linspace of :26).  One wave walks one ray; everything the reference keeps
// in [N, T, *] / [N, T + U, *] tensors -- coarse depths and densities, their weights, the CDF, the U resampled depths, the
// merged order -- lives in a few KB of LDS per wave:
//   1. coarse pass: T uniform samples, fused hash grid + sigma net                                   (:148-170)
//   2. weights of the coarse samples (:176-180), CDF over the T - 1 mid points of weights[1:-1] + 1e-5 (:17-22), U inverse-CDF
//      samples by binary search (:29-44)
//   3. fine pass: sigma at the U new depths                                                          (:181-184)
//   4. merge of the two ascending runs (the sort + gathers of :187-193; coarse first on ties)
//   5. compositing over the T + U merged samples exactly as k_render_uniform does; a tile that holds a sample with weight > 1e-4
//      re-evaluates the sigma net for its geometry features (bit-identical to the first evaluation) and runs the colour net.
// ------------------------------------------------------------------------------------------
template <int MODE, bool CLAMPED = false>
__global__ void __launch_bounds__(256) k_render_upsample(NetArgs na, GridLevels lv, const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                         const float* __restrict__ nears, const float* __restrict__ fars, uint32_t N, uint32_t T,
                                                         uint32_t U, const float* __restrict__ lin, const float* __restrict__ u_det,
                                                         float* __restrict__ weights_sum, float* __restrict__ depth, float* __restrict__ image,
                                                         float* __restrict__ aggregated_density, uint32_t dump_begin, float* __restrict__ sigmas,
                                                         float* __restrict__ rgbs, float aabb_lo, float aabb_hi,
                                                         const float* __restrict__ sc_in, float* __restrict__ zf_out, uint32_t frame_w) {
    // sc_in: sigma of the uniform samples, evaluated by k_density_x16 (tiles across rays);  zf_out: stop after the resampling
    // and hand the new depths over.  Both group-major (frame_w as in that launch): the middle launch of the large-batch form.
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const size_t w_bytes = net_w_bytes_f16(na);
    _Float16* Wlds = reinterpret_cast<_Float16*>(smem);
    LevelTab* lt = reinterpret_cast<LevelTab*>(smem + w_bytes);
    stage_block(na, lv, Wlds, lt, w_bytes);
    const uint32_t lane = threadIdx.x & 63, c = lane & 15, wid = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    const uint32_t Tm = T + U;
    float* zc = reinterpret_cast<float*>(smem + w_bytes + sizeof(LevelTab)) + (size_t)wid * (5 * T + 4 * U);
    float* sc = zc + T;
    float* cdf = sc + T;          // first the coarse weights, then (in place) the CDF
    float* zf = cdf + T;
    float* sf = zf + U;
    float* zm = sf + U;
    float* sm = zm + Tm;
#define NGP_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)
    for (uint32_t ray = blockIdx.x * wpb + wid; ray < N; ray += gridDim.x * wpb) {
        const RaySetup r = load_ray(rays_o, rays_d, nears, fars, ray, T);
        const bool dump = sigmas != nullptr && ray >= dump_begin;
        uint32_t g_grp, g_c;
        ray_slot(ray, frame_w, g_grp, g_c);
        // ---- 1. / 3. sigma along the ray: the T uniform depths, then (after the resampling below) the U new ones
        for (int phase = 0; phase < 2; phase++) {
            const uint32_t n = phase ? U : T;
            float* zdst = phase ? zf : zc;
            float* sdst = phase ? sf : sc;
            if (!phase && sc_in) {  // the coarse pass was evaluated across rays: take its sigma
                for (uint32_t i = lane; i < n; i += 64) {
                    zdst[i] = r.z_at(lin, i);
                    sdst[i] = sc_in[((size_t)g_grp * T + i) * 16 + g_c];
                }
            } else
            for (uint32_t i0 = 0; i0 < n; i0 += 16) {
                const uint32_t idx = i0 + c;
                const bool valid = idx < n;
                const uint32_t ii = valid ? idx : n - 1;
                const float zv = phase ? zf[ii] : r.z_at(lin, ii);
                float x, y, z;
                sample_point(r, zv, aabb_lo, aabb_hi, x, y, z);
                float sigma;
                _Float16 s16[4];
                net_density<MODE, false, CLAMPED>(na, Wlds, *lt, lane, x, y, z, sigma, s16);
                if (lane < 16 && valid) { zdst[idx] = zv; sdst[idx] = sigma; }
            }
            NGP_WAVE_SYNC();
            if (phase) break;
            // ---- 2. coarse weights (:176-180), lane = sample
            float carry = 1.0f;
            for (uint32_t t0 = 0; t0 < T; t0 += 64) {
                const uint32_t t = t0 + lane;
                const bool on = t < T;
                const uint32_t tt = on ? t : T - 1;
                const float delta = tt + 1 < T ? zc[tt + 1] - zc[tt] : r.sample_dist;
                const float alpha = on ? sample_alpha(delta, na.density_scale, sc[tt]) : 0.0f;
                float tile_product;
                const float Tr = tile_transmittance<64>(on ? alpha_survival(alpha) : 1.0f, carry, lane, tile_product);
                if (on) cdf[t] = alpha * Tr;
                carry *= tile_product;
            }
            NGP_WAVE_SYNC();
            // sample_pdf(bins = mid points [T - 1], weights[1:-1] [T - 2]) (:12-46): cdf[k], k = 0 .. T - 2, in place of weights[k]
            const uint32_t Tb = T - 1, Tw = T - 2;
            float sum = 0.0f;
            for (uint32_t t = lane; t < Tw; t += 64) sum += cdf[t + 1] + 1e-5f;      // :19-20
#pragma unroll      // (wave_ops.hpp's wave_sum, and last_lane below, written out: as calls k_render_upsample compiles to other instructions)
            for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
            float run = 0.0f;
            for (uint32_t t0 = 0; t0 < Tw; t0 += 64) {
                const uint32_t t = t0 + lane;
                const float pdf = t < Tw ? (cdf[t + 1] + 1e-5f) / sum : 0.0f;
                const float incl = scan_inclusive<AddOp>(pdf, lane);
                if (t < Tw) cdf[t + 1] = run + incl;                                 // :21
                run += __shfl(incl, 63, 64);
            }
            if (lane == 0) cdf[0] = 0.0f;                                            // :22
            NGP_WAVE_SYNC();
            for (uint32_t sI = lane; sI < U; sI += 64) {
                const float us = u_det[sI];
                uint32_t lo = 0, hi = Tb;                                            // searchsorted(cdf, u, right=True)
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (cdf[mid] > us) hi = mid; else lo = mid + 1;
                }
                const uint32_t below = lo > 0 ? lo - 1 : 0, above = lo < Tb - 1 ? lo : Tb - 1;   // :33-34
                float denom = cdf[above] - cdf[below];                               // :41
                if (denom < 1e-5f) denom = 1.0f;                                     // :42
                const float tq = (us - cdf[below]) / denom;                          // :43
                const float b0 = zc[below] + 0.5f * (zc[below + 1] - zc[below]);     // :174 mid points
                const float b1 = zc[above] + 0.5f * (zc[above + 1] - zc[above]);
                zf[sI] = b0 + tq * (b1 - b0);                                        // :44
                if (zf_out) zf_out[((size_t)g_grp * U + sI) * 16 + g_c] = zf[sI];
            }
            NGP_WAVE_SYNC();
            if (zf_out) break;
        }
        if (zf_out) { NGP_WAVE_SYNC(); continue; }
        // ---- 4. merge: rank of every element in the other run (coarse first on ties)
        for (uint32_t k = lane; k < Tm; k += 64) {
            float v, sg;
            uint32_t pos;
            if (k < T) {
                v = zc[k]; sg = sc[k];
                uint32_t lo = 0, hi = U;
                while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (zf[mid] < v) lo = mid + 1; else hi = mid; }
                pos = k + lo;
            } else {
                v = zf[k - T]; sg = sf[k - T];
                uint32_t lo = 0, hi = T;
                while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (zc[mid] <= v) lo = mid + 1; else hi = mid; }
                pos = (k - T) + lo;
            }
            zm[pos] = v; sm[pos] = sg;
        }
        NGP_WAVE_SYNC();
        // ---- 5. compositing over the merged samples (:206-244)
        float carry = 1.0f;
        RaySums sums = {};
        for (uint32_t i0 = 0; i0 < Tm; i0 += 16) {
            const uint32_t idx = i0 + c;
            const bool valid = idx < Tm;
            const uint32_t ii = valid ? idx : Tm - 1;
            const float zv = zm[ii], sigma = sm[ii];
            const float delta = (ii + 1 < Tm) ? zm[ii + 1] - zv : r.sample_dist;     // :206-207
            const float alpha = valid ? sample_alpha(delta, na.density_scale, sigma) : 0.0f;
            float tile_product;
            const float w = alpha * tile_transmittance<16>(alpha_survival(alpha), carry, c, tile_product);   // :210
            const bool masked = valid && weight_masked(w);
            float cr = 0, cg = 0, cb = 0;
            if (__ballot(masked) != 0ull) {      // (as masked_color does, with the sigma net evaluated again for the geometry features it did not keep)
                float x, y, z, s_again;
                sample_point(r, zv, aabb_lo, aabb_hi, x, y, z);
                _Float16 s16[4];
                net_density<MODE, false, CLAMPED>(na, Wlds, *lt, lane, x, y, z, s_again, s16);
                net_color(na, Wlds, lane, r.dx, r.dy, r.dz, s16, cr, cg, cb);
                if (!masked) { cr = 0; cg = 0; cb = 0; }
            }
            if (lane < 16 && valid) {
                sums.add(r, zv, w, sigma, cr, cg, cb);
                if (dump) dump_sample(sigmas, rgbs, (size_t)(ray - dump_begin) * Tm + idx, sigma, cr, cg, cb);
            }
            carry = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(carry * tile_product)));
            if (!dump && carry < kSpentTransmittance) break;
        }
        sums.reduce16();
        if (lane == 0) sums.store(ray, weights_sum, depth, image, aggregated_density);
        NGP_WAVE_SYNC();      // the next ray overwrites the arrays
    }
#undef NGP_WAVE_SYNC
}

// ==========================================================================================
// Differentiable `run`: the vector-Jacobian product of k_render_uniform with respect to the RAYS, map frozen.
// What nav/estimator_helpers.py:191-225 (measurement_fn) differentiates -- <= 1024 chosen pixels x 512 samples, 100 Adam steps per
// simulator step -- is d(image, depth) / d(rays_o, rays_d) through sampling -> hash grid -> sigma net -> SH -> colour net ->
// compositing, with table and weights constant.  The reference (and this package's operator path) gets it from autograd over
// ~60 kernels and [N, T, *] saved tensors; here it is ONE launch, one wave per ray, nothing saved by the forward pass:
//
//   pass 1  forward over the ray's tiles (as k_render_uniform): per sample sigma, transmittance T_i and the upstream gradient
//           of its weight, g_i = dL/dw_i = G_img . rgb_i [w_i > 1e-4] + G_depth rel_i + G_ws + G_agg sigma_i, into LDS;
//   scan    reverse scan over the samples: dL/dalpha_j = g_j T_j - (sum_{i>j} g_i w_i) / p_j  ->  dL/dsigma_j, in place;
//   pass 2  per tile, recompute the network keeping every layer's activations in registers and walk it backwards with the
//           TRANSPOSED weights (packed as MFMA A fragments by k_pack_weights_bwd: dH_prev^T = W^T dH^T, the same accumulator ->
//           B-fragment trick as forward, so gradients never leave registers either): colour net -> (SH', geo) -> sigma net ->
//           hash-grid input derivative from the corners already gathered -> clip -> (grad o, grad d), reduced over the ray.
//
// Rounding points follow the operator path: fp16 activations and activation gradients, fp32 MFMA accumulation, fp32 everywhere
// outside the MLPs.
// ==========================================================================================
struct GradArgs {
    const float *rays_o, *rays_d, *nears, *fars, *lin;
    const float *g_image, *g_depth, *g_ws, *g_agg;      // upstream gradients of the four per-ray outputs (g_depth / g_ws / g_agg may be NULL)
    float *grad_o, *grad_d;
    const void* packed_bwd;
    uint32_t N, T;
    float aabb_lo, aabb_hi;
    float* dump;    // diagnostics (ngp_debug_set_grad_dump): [N][T][4] = sigma, transmittance, dL/dw, dL/dsigma per sample; NULL = off
};

constexpr int kGradWaves = 8;
constexpr uint32_t kGradMaxT = 1024;

// GW waves (= rays in flight) per workgroup, one workgroup per CU: 8, or 4 -- one wave per SIMD with the whole register file, which the
// fp32 form needs (its tape is twice the size) and which also spreads a small batch over all CUs (the pose estimator's 1024 rays are
// 128 workgroups of 8 but 256 of 4)
template <class NET, int GW>
__global__ void __launch_bounds__(GW * 64, 1) k_render_uniform_bwd(NetArgs na, GridLevels lv, GradArgs ga) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const size_t w_bytes = NET::w_bytes(na);
    const size_t wb_bytes = NET::wb_bytes(na);
    const char* Wlds = smem;
    char* Wb = smem + w_bytes;
    LevelTab* lt = reinterpret_cast<LevelTab*>(smem + w_bytes + wb_bytes);
    float* store = reinterpret_cast<float*>(smem + w_bytes + wb_bytes + sizeof(LevelTab));
    {   // transposed fragments next to the forward ones
        const uint4* src = reinterpret_cast<const uint4*>(ga.packed_bwd);
        uint4* dst = reinterpret_cast<uint4*>(Wb);
        for (uint32_t i = threadIdx.x; i < wb_bytes / 16; i += blockDim.x) dst[i] = src[i];
    }
    stage_block(na, lv, smem, lt, w_bytes);
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
    const uint32_t T = ga.T;
    float* s_sig = store + (size_t)wid * 3 * T;      // pass 1: sigma (raw);  after the scan: dL/dsigma
    float* s_g = s_sig + T;                          // pass 1: dL/dw;        after the scan: w [w > 1e-4] (the scale of dL/drgb)
    float* s_T = s_g + T;                            // transmittance before the sample

    for (uint32_t ray = blockIdx.x * GW + wid; ray < ga.N; ray += gridDim.x * GW) {
        const RaySetup r = load_ray(ga.rays_o, ga.rays_d, ga.nears, ga.fars, ray, T);
        const float Gi0 = ga.g_image[(size_t)ray * 3], Gi1 = ga.g_image[(size_t)ray * 3 + 1], Gi2 = ga.g_image[(size_t)ray * 3 + 2];
        const float Gd = ga.g_depth ? ga.g_depth[ray] : 0.0f, Gw = ga.g_ws ? ga.g_ws[ray] : 0.0f, Ga = ga.g_agg ? ga.g_agg[ray] : 0.0f;
        // ---------------- pass 1: forward, k_render_uniform's tile loop from the same helpers ----------------
        float carry = 1.0f;
        uint32_t t_end = T;                                           // samples >= t_end carry no weight (transmittance below 1e-10)
        for (uint32_t i0 = 0; i0 < T; i0 += 16) {
            const uint32_t idx = i0 + c;
            const bool valid = idx < T;
            const uint32_t ii = valid ? idx : T - 1;
            const float zv = r.z_at(ga.lin, ii);
            float x, y, z;
            sample_point(r, zv, ga.aabb_lo, ga.aabb_hi, x, y, z);
            float sigma;
            typename NET::geo_t s16[4];
            NET::density(na, Wlds, *lt, lane, x, y, z, sigma, s16);
            const float z_next = (ii + 1 < T) ? r.z_at(ga.lin, ii + 1) : 0.0f;
            const float delta = (ii + 1 < T) ? z_next - zv : r.sample_dist;
            const float alpha = valid ? sample_alpha(delta, na.density_scale, sigma) : 0.0f;
            float tile_product;
            const float Tr = tile_transmittance<16>(alpha_survival(alpha), carry, c, tile_product);
            const float w = alpha * Tr;
            const bool masked = valid && weight_masked(w);
            float cr, cg, cb;
            masked_color<NET>(na, Wlds, lane, r, s16, masked && lane < 16, masked, cr, cg, cb);
            if (lane < 16 && valid) {     // (instead of the forward's sums: the sample's state for the reverse scan; a NaN depth ratio has no gradient)
                const float qz = r.depth_ratio(zv);
                const float rel = qz != qz ? 0.0f : fminf(1.0f, fmaxf(0.0f, qz));
                s_sig[idx] = sigma;
                s_T[idx] = Tr;
                s_g[idx] = fmaf(Gi0, cr, fmaf(Gi1, cg, Gi2 * cb)) + Gd * rel + Gw + Ga * sigma;
            }
            carry = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(carry * tile_product)));              // quarter 0's value, for the whole wave
            if (carry < kSpentTransmittance) { t_end = (i0 + 16 < T) ? i0 + 16 : T; break; }
        }
        __builtin_amdgcn_wave_barrier();
        // ---------------- reverse scan: dL/dsigma_j and the colour scale w_j [w_j > 1e-4] ----------------
        float suffix = 0.0f;
        for (uint32_t c0 = ((t_end + 63) / 64) * 64; c0 > 0; c0 -= 64) {
            const uint32_t t = c0 - 64 + lane;
            const bool on = t < t_end;
            const uint32_t tt = on ? t : t_end - 1;
            const float zv = r.z_at(ga.lin, tt);
            const float delta = (tt + 1 < T) ? r.z_at(ga.lin, tt + 1) - zv : r.sample_dist;
            const float sg = s_sig[tt], Tr = s_T[tt];
            const float e = expf(((-delta) * na.density_scale) * sg);               // (sample_alpha's exponential, kept for its derivative)
            const float alpha = 1.0f - e, p = alpha_survival(alpha), w = alpha * Tr;
            const float g = on ? s_g[tt] : 0.0f;
            const float gw = on ? g * w : 0.0f;
            float inc = gw;      // (scan_suffix<AddOp> and first_lane, and quad_sum in pass 2, written out: as calls k_render_uniform_bwd compiles to other instructions)
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const float o = __shfl_down(inc, off, 64);
                if (lane + (uint32_t)off < 64) inc += o;
            }
            const float later = suffix + (inc - gw);
            suffix += __shfl(inc, 0, 64);
            __builtin_amdgcn_wave_barrier();
            if (on) {
                const float dsg = (g * Tr - later / p) * ((delta * na.density_scale) * e) + Ga * w;
                if (ga.dump) {
                    float* o4 = ga.dump + ((size_t)ray * T + t) * 4;
                    o4[0] = sg; o4[1] = Tr; o4[2] = g; o4[3] = dsg;
                }
                s_sig[t] = dsg;
                s_g[t] = weight_masked(w) ? w : 0.0f;
            }
        }
        __builtin_amdgcn_wave_barrier();
        // ---------------- pass 2: network backward per tile ----------------
        float a_o[3] = {0, 0, 0}, a_d[3] = {0, 0, 0};
        const float G[3] = {Gi0, Gi1, Gi2};
        for (uint32_t i0 = 0; i0 < t_end; i0 += 16) {
            const uint32_t idx = i0 + c;
            const bool valid = idx < t_end;
            const uint32_t ii = valid ? idx : t_end - 1;
            const float zv = r.z_at(ga.lin, ii);
            const float ux = r.ox + r.dx * zv, uy = r.oy + r.dy * zv, uz = r.oz + r.dz * zv;   // before the clip (for its derivative)
            const float x = clampf(ux, ga.aabb_lo, ga.aabb_hi), y = clampf(uy, ga.aabb_lo, ga.aabb_hi), z = clampf(uz, ga.aabb_lo, ga.aabb_hi);
            // ---- forward recompute, keeping corners and activations
            typename NET::Tape tape;
            typename NET::geo_t s16[4];
            NET::density_tape(na, Wlds, *lt, lane, x, y, z, tape, s16);
            const float wscale = valid ? s_g[ii] : 0.0f;            // w [w > 1e-4]: zero when the reference does not evaluate the colour
            const float dsig = valid ? s_sig[ii] : 0.0f;
            f32x4 gso = {0, 0, 0, 0};                               // dL/d(sigma-net outputs 4q .. 4q+3) of sample c
            float gdir[3] = {0, 0, 0};
            if (__ballot(wscale != 0.0f && lane < 16) != 0ull) {
                const float wsc = __shfl(wscale, c, 64);             // lanes 0..15 hold the per-sample values: broadcast to the sample's 4 lanes
                NET::color_vjp(na, Wlds, Wb, lane, r.dx, r.dy, r.dz, s16, wsc, G, gdir, gso);
            }
            // ---- sigma: trunc_exp backward (activation.py:12-17) on output 0
            {
                const float ds = __shfl(dsig, c, 64);
                if (q == 0) gso[0] = ds * expf(fminf(15.0f, fmaxf(-15.0f, (float)s16[0])));
            }
            float gx[3];
            NET::density_vjp(na, Wb, lane, tape, gso, gx);
            // reduce the four level groups of a sample, then x = clip(o + d z): (x + bound) / (2 bound) upstream
#pragma unroll
            for (int d = 0; d < 3; d++) {
                gx[d] += __shfl_xor(gx[d], 16, 64);
                gx[d] += __shfl_xor(gx[d], 32, 64);
                gdir[d] += __shfl_xor(gdir[d], 16, 64);
                gdir[d] += __shfl_xor(gdir[d], 32, 64);
            }
            if (lane < 16 && valid) {
                const float uu[3] = {ux, uy, uz};
#pragma unroll
                for (int d = 0; d < 3; d++) {
                    const float a = uu[d] > ga.aabb_lo ? 1.0f : (uu[d] == ga.aabb_lo ? 0.5f : 0.0f);
                    const float v = fmaxf(uu[d], ga.aabb_lo);
                    const float b = v < ga.aabb_hi ? 1.0f : (v == ga.aabb_hi ? 0.5f : 0.0f);
                    const float gxd = gx[d] * na.inv_two_bound * (a * b);
                    a_o[d] += gxd;
                    a_d[d] = fmaf(gxd, zv, a_d[d]) + gdir[d];       // the direction also enters through SH (dirs = rays_d per sample)
                }
            }
        }
#pragma unroll
        for (int d = 0; d < 3; d++) {
#pragma unroll
            for (int off = 8; off > 0; off >>= 1) { a_o[d] += __shfl_xor(a_o[d], off, 16); a_d[d] += __shfl_xor(a_d[d], off, 16); }      // two wave_sum<16>, interleaved (as reduce16)
            if (lane == 0) { ga.grad_o[(size_t)ray * 3 + d] = a_o[d]; ga.grad_d[(size_t)ray * 3 + d] = a_d[d]; }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

}  // namespace ngp

using namespace ngp;

// frame_width (scheduling hint, results do not depend on it): the rays are the pixels of row-major frames this wide -> a group of the
// across-ray kernels is a 4x4-pixel block instead of a 1x16 strip (its sixteen rays are closer together and end at more similar
// depths).  0 where the rays are not whole rows of 4x4 blocks.
static uint32_t usable_frame_width(uint32_t frame_width, uint32_t N) {
    return frame_width && (frame_width % 4 != 0 || N % (4 * frame_width) != 0) ? 0 : frame_width;
}

// runs STMT with MODE bound to the grid variant `mode` of the fp16 network (net_density<MODE>), as NGP_WITH_NET does with NET
#define NGP_WITH_MODE(mode, ...)                                   \
    switch (mode) {                                                \
        case 1: { constexpr int MODE = 1; __VA_ARGS__; } break;    \
        case 2: { constexpr int MODE = 2; __VA_ARGS__; } break;    \
        default: { constexpr int MODE = 0; __VA_ARGS__; } break;   \
    }
// The forward kernels of this unit clamp every position to [-bound, bound] (sample_point), so when 2*bound is a power of two
// (clamped_exact) they take the instantiation without the encoder's out-of-range test: CL / the third parameter of the NET policy.
#define NGP_WITH_CLAMPED(clamped, ...)                             \
    if (clamped) { constexpr bool CL = true; __VA_ARGS__; }        \
    else { constexpr bool CL = false; __VA_ARGS__; }
#define NGP_WITH_NET_CLAMPED(variant, ...)                                         \
    switch (variant) {                                                             \
        case 0: { using NET = NetF16<0, false, true>; __VA_ARGS__; } break;        \
        case 1: { using NET = NetF16<1, false, true>; __VA_ARGS__; } break;        \
        case 2: { using NET = NetF16<2, false, true>; __VA_ARGS__; } break;        \
        case 3: { using NET = NetF32<0, true>; __VA_ARGS__; } break;               \
        case 4: { using NET = NetF32<1, true>; __VA_ARGS__; } break;               \
        case 5: { using NET = NetF16<0, true, true>; __VA_ARGS__; } break;         \
        case 6: { using NET = NetF16<1, true, true>; __VA_ARGS__; } break;         \
        default: { using NET = NetF16<2, true, true>; __VA_ARGS__; } break;        \
    }

extern "C" {

int ngp_render_uniform(const ngp_model* model, const float* rays_o, const float* rays_d, const float* nears, const float* fars, uint32_t N,
                       uint32_t T, const float* lin, float* weights_sum, float* depth, float* image, float* aggregated_density,
                       uint32_t dump_begin, float* sigmas, float* rgbs, uint32_t frame_width, ngp_stream_t stream) {
    if (N == 0) return NGP_OK;
    NGP_REQUIRE(rays_o && rays_d && nears && fars && lin && weights_sum && depth && image && aggregated_density, "render_uniform: null pointer");
    NGP_REQUIRE((sigmas == nullptr) == (rgbs == nullptr), "render_uniform: sigmas and rgbs must both be given or both NULL");
    NGP_REQUIRE(T >= 1, "render_uniform: num_steps must be positive");
    hipStream_t s = (hipStream_t)stream;
    // No scratch of the library's own: the fragment-major weights are the caller's, packed once per parameter version
    // (a process-wide buffer here would be shared by calls that run concurrently on different streams with different models)
    NGP_REQUIRE(model && model->packed_weights, "render_uniform: model->packed_weights is NULL (ngp_pack_weights fills it)");
    NetArgs na;
    GridLevels lv;
    const DebugState dbg = debug_snapshot();
    int rc = fill_net(model, (const _Float16*)model->packed_weights, na, lv);
    if (rc) return rc;
    const size_t lds = weights_bytes(na) + sizeof(LevelTab);
    NGP_REQUIRE(lds <= 96 * 1024, "render_uniform: the packed weights need %zu bytes of LDS", lds);
    const int variant = net_variant(na, lv);
    const bool clamped = clamped_exact(na);     // the kernels below clamp to [-bound, bound]: see NGP_WITH_NET_CLAMPED
    uint32_t blocks = div_up(N, 4);
    if (blocks > resident_blocks(lds)) blocks = resident_blocks(lds);   // each wave strides over rays
    ProfScope prof("render_uniform", s, (double)N * T);
    // tiles across sixteen neighbouring rays (twice the per-sample rate) once there are enough groups of sixteen to occupy the chip;
    // a pose-estimator batch (1024 scattered pixels, every ray dumped) keeps one ray per wave
    const bool per_ray = env_set("NGP_UNIFORM_PER_RAY");    // diagnostics (read per call: tests switch it): tiles along one ray for every size
    if (!per_ray && N >= kUniformX16MinRays) {
        const uint32_t fw = usable_frame_width(frame_width, N);
        uint32_t gb = div_up(div_up(N, 16), 4);
        // as many workgroups as are RESIDENT at once (each strides over the groups): four per CU, or what the LDS holds -- the fp32
        // weights take 40 KB per workgroup, three fit, and with 1024 workgroups the fourth of every CU ran as a second round at a third
        // of the occupancy (800x800 x 512 samples, fp32: 8.01 -> 7.56 ms)
        const uint32_t gb_cap = resident_blocks(lds);
        if (gb > gb_cap) gb = gb_cap;
#define NGP_LAUNCH_X16                                                                                                                          \
    {                                                                                                                                           \
        ensure_dynamic_lds(reinterpret_cast<const void*>(k_render_uniform_x16<NET>), 96 * 1024);                                                \
        k_render_uniform_x16<NET><<<gb, 256, lds, s>>>(na, lv, rays_o, rays_d, nears, fars, N, T, lin, weights_sum, depth, image, aggregated_density, \
                                                       dump_begin, sigmas, rgbs, -model->bound, model->bound, fw, dbg.stamps);                 \
    }
        if (clamped) { NGP_WITH_NET_CLAMPED(variant, NGP_LAUNCH_X16); }
        else { NGP_WITH_NET(variant, NGP_LAUNCH_X16); }
#undef NGP_LAUNCH_X16
        return check_launch("render_uniform");
    }
#define NGP_LAUNCH_PER_RAY                                                                                                                      \
    {                                                                                                                                           \
        ensure_dynamic_lds(reinterpret_cast<const void*>(k_render_uniform<NET>), 96 * 1024);                                                    \
        k_render_uniform<NET><<<blocks, 256, lds, s>>>(na, lv, rays_o, rays_d, nears, fars, N, T, lin, weights_sum, depth, image, aggregated_density, \
                                                       dump_begin, sigmas, rgbs, -model->bound, model->bound);                                 \
    }
    if (clamped) { NGP_WITH_NET_CLAMPED(variant, NGP_LAUNCH_PER_RAY); }
    else { NGP_WITH_NET(variant, NGP_LAUNCH_PER_RAY); }
#undef NGP_LAUNCH_PER_RAY
    return check_launch("render_uniform");
}

// group-major arrays over Np rays, whole groups of sixteen (see k_density_x16)
struct UpsampleWs {
    float *sc, *zf, *sf;      // sigma of the coarse pass [Np, T]; depths and sigma of the fine pass [Np, U] each
    _Float16 *gc, *gf;        // the sigma net's outputs of both passes [Np, T, 16], [Np, U, 16]
};
static UpsampleWs upsample_layout(Carver& c, uint32_t N, uint32_t T, uint32_t U) {
    const size_t Np = ((size_t)N + 15) / 16 * 16;
    return {c.take<float>(Np * T), c.take<float>(Np * U), c.take<float>(Np * U), c.take<_Float16>(Np * T * 16), c.take<_Float16>(Np * U * 16)};
}
static size_t upsample_workspace_bytes(uint32_t N, uint32_t T, uint32_t U) { Carver c; upsample_layout(c, N, T, U); return c.bytes(); }
size_t ngp_render_upsample_workspace(uint32_t N, uint32_t T, uint32_t U) {
    return N >= kUniformX16MinRays ? upsample_workspace_bytes(N, T, U) : 0;
}

int ngp_render_upsample(const ngp_model* model, const float* rays_o, const float* rays_d, const float* nears, const float* fars, uint32_t N,
                        uint32_t T, uint32_t U, const float* lin, const float* u, float* weights_sum, float* depth, float* image,
                        float* aggregated_density, uint32_t dump_begin, float* sigmas, float* rgbs, uint32_t frame_width, void* workspace,
                        size_t workspace_bytes, ngp_stream_t stream) {
    if (N == 0) return NGP_OK;
    NGP_REQUIRE(rays_o && rays_d && nears && fars && lin && u && weights_sum && depth && image && aggregated_density, "render_upsample: null pointer");
    NGP_REQUIRE((sigmas == nullptr) == (rgbs == nullptr), "render_upsample: sigmas and rgbs must both be given or both NULL");
    NGP_REQUIRE(T >= 3 && U >= 1, "render_upsample: num_steps >= 3 and upsample_steps >= 1 (got %u, %u)", T, U);
    hipStream_t s = (hipStream_t)stream;
    NGP_REQUIRE(model && model->packed_weights, "render_upsample: model->packed_weights is NULL (ngp_pack_weights fills it)");
    NetArgs na;
    GridLevels lv;
    int rc = fill_net(model, (const _Float16*)model->packed_weights, na, lv);
    if (rc) return rc;
    NGP_REQUIRE(!na.f32(), "render_upsample: built for the fp16 network (ngp_model::precision == NGP_PREC_F16)");
    const size_t fixed = weights_bytes(na) + sizeof(LevelTab), per_wave = ((size_t)5 * T + (size_t)4 * U) * sizeof(float);
    const size_t budget = 160 * 1024 - 1024;
    NGP_REQUIRE(fixed + per_wave <= budget, "render_upsample: num_steps %u + upsample_steps %u need %zu bytes of LDS per ray, %zu are available", T, U,
                per_wave, budget - fixed);
    uint32_t waves = (uint32_t)((budget - fixed) / per_wave);
    waves = waves > 4 ? 4 : waves;
    const size_t lds = fixed + waves * per_wave;
    uint32_t blocks = div_up(N, waves);
    if (blocks > 1024) blocks = 1024;
    ProfScope prof("render_upsample", s, (double)N * (T + U));
    const int mode = needs_generic(lv) ? 1 : (na.cells ? 2 : 0);
    const bool clamped = clamped_exact(na);
    const uint32_t fw = usable_frame_width(frame_width, N);
    auto per_ray = [&](const float* sc_in, float* zf_out) {
        NGP_WITH_MODE(mode, NGP_WITH_CLAMPED(clamped, {
            ensure_dynamic_lds(reinterpret_cast<const void*>(k_render_upsample<MODE, CL>), 160 * 1024);
            k_render_upsample<MODE, CL><<<blocks, 64 * waves, lds, s>>>(na, lv, rays_o, rays_d, nears, fars, N, T, U, lin, u, weights_sum, depth, image,
                                                                        aggregated_density, dump_begin, sigmas, rgbs, -model->bound, model->bound, sc_in, zf_out, fw);
        }));
    };
    const size_t need = upsample_workspace_bytes(N, T, U);
    if (!(workspace && workspace_bytes >= need && N >= kUniformX16MinRays && !env_set("NGP_UPSAMPLE_PER_RAY"))) {
        per_ray(nullptr, nullptr);      // everything along the ray in one launch
        return check_launch("render_upsample");
    }
    // Large batches: four launches through the caller's scratch (group-major arrays, see k_density_x16).  The two density
    // passes take their tiles ACROSS sixteen neighbouring rays (twice the per-sample rate of tiles along a ray) and keep the sigma
    // net's outputs; the per-ray kernel resamples between them; merge + compositing run across the rays as well, colour net only.
    Carver carver(workspace);
    const UpsampleWs w = upsample_layout(carver, N, T, U);
    float *sc = w.sc, *zf = w.zf, *sf = w.sf;
    _Float16 *gc = w.gc, *gf = w.gf;
    uint32_t gb = div_up(div_up(N, 16), 4);
    if (gb > 1024) gb = 1024;
    auto density = [&](uint32_t n, const float* z_in, float* out, _Float16* geo) {
        NGP_WITH_MODE(mode, NGP_WITH_CLAMPED(clamped, {
            using NET = NetF16<MODE, false, CL>;
            ensure_dynamic_lds(reinterpret_cast<const void*>(k_density_x16<NET>), 96 * 1024);
            k_density_x16<NET><<<gb, 256, fixed, s>>>(na, lv, rays_o, rays_d, nears, fars, N, n, lin, z_in, out, geo, -model->bound, model->bound, fw);
        }));
    };
    density(T, nullptr, sc, gc);
    per_ray(sc, zf);
    density(U, zf, sf, gf);
    NGP_WITH_MODE(mode, {
        ensure_dynamic_lds(reinterpret_cast<const void*>(k_composite_merged_x16<MODE>), 96 * 1024);
        k_composite_merged_x16<MODE><<<gb, 256, fixed, s>>>(na, lv, rays_d, nears, fars, N, T, U, lin, sc, zf, sf, gc, gf, weights_sum, depth, image,
                                                            aggregated_density, dump_begin, sigmas, rgbs, fw);
    });
    return check_launch("render_upsample");
}

size_t ngp_render_uniform_backward_lds(const ngp_model* model, uint32_t T) {
    if (!model) return 0;
    NetArgs na = {};
    na.sig_mm = model->sigma_hidden_mm; na.col_mm = model->color_hidden_mm; na.prec_bits = model->precision == NGP_PREC_F32 ? 256u : 0u;
    if (!bwd_shape_ok(na)) return (size_t)-1;
    const size_t wb = na.f32() ? NetF32<0>::wb_bytes(na) : NetF16<0>::wb_bytes(na);
    return net_w_bytes(na) + wb + sizeof(LevelTab) + (size_t)(na.f32() ? 4 : kGradWaves) * 3 * T * 4;
}

int ngp_render_uniform_backward(const ngp_model* model, const void* packed_weights_bwd, const float* rays_o, const float* rays_d, const float* nears,
                                const float* fars, uint32_t N, uint32_t T, const float* lin, const float* grad_image, const float* grad_depth,
                                const float* grad_weights_sum, const float* grad_aggregated_density, float* grad_rays_o, float* grad_rays_d,
                                ngp_stream_t stream) {
    if (N == 0) return NGP_OK;
    NGP_REQUIRE(rays_o && rays_d && nears && fars && lin && grad_image && grad_rays_o && grad_rays_d, "render_uniform_backward: null pointer");
    NGP_REQUIRE(model && model->packed_weights && packed_weights_bwd, "render_uniform_backward: packed weights missing (ngp_pack_weights / ngp_pack_weights_bwd)");
    NGP_REQUIRE(T >= 1 && T <= kGradMaxT, "render_uniform_backward: 1 <= num_steps <= %u (got %u)", kGradMaxT, T);
    hipStream_t s = (hipStream_t)stream;
    NetArgs na;
    GridLevels lv;
    int rc = fill_net(model, (const _Float16*)model->packed_weights, na, lv);
    if (rc) return rc;
    NGP_REQUIRE(bwd_shape_ok(na), "render_uniform_backward: the fp32 form supports at most 1 / 2 hidden matmuls (got %u / %u)", na.sig_mm, na.col_mm);
    GradArgs ga = {rays_o, rays_d, nears, fars, lin, grad_image, grad_depth, grad_weights_sum, grad_aggregated_density, grad_rays_o, grad_rays_d,
                   packed_weights_bwd, N, T, -model->bound, model->bound, grad_dump()};
    const size_t lds = ngp_render_uniform_backward_lds(model, T);
    NGP_REQUIRE(lds <= 160 * 1024, "render_uniform_backward: LDS budget exceeded (%zu bytes: at most %u samples per ray with this network)", lds, T);
    ProfScope prof("render_uniform_backward", s, (double)N * T);
    // four rays per workgroup: always in fp32; in fp16 while that still gives every CU at most two rounds of work
    const bool four = na.f32() || N <= 2048;
    uint32_t blocks = div_up(N, four ? 4 : kGradWaves);
    if (blocks > 512) blocks = 512;
    NGP_WITH_NET(net_variant(na, lv), {
        if (four) {
            ensure_dynamic_lds(reinterpret_cast<const void*>(k_render_uniform_bwd<NET, 4>), 160 * 1024);
            k_render_uniform_bwd<NET, 4><<<blocks, 4 * 64, lds, s>>>(na, lv, ga);
        } else {
            ensure_dynamic_lds(reinterpret_cast<const void*>(k_render_uniform_bwd<NET, kGradWaves>), 160 * 1024);
            k_render_uniform_bwd<NET, kGradWaves><<<blocks, kGradWaves * 64, lds, s>>>(na, lv, ga);
        }
    });
    return check_launch("render_uniform_backward");
}

}  // extern "C"
