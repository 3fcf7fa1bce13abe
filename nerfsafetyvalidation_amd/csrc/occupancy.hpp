// The occupancy-grid march of march_rays_train, march_rays and the fused renderer: the DDA and its jitter, the derived copies of the
// occupancy bits, the one-wave-per-ray window step, the slot scan.  Included by raymarching.hip, render_fused.hip and occupancy.hip only.
#pragma once
#include "ngp_common.hpp"
#include "wave_ops.hpp"

namespace ngp {

// raymarching.cu:58-83 (expand_bits / morton3D are in ngp_common.hpp: the density grid uses them too)
__device__ __forceinline__ uint32_t morton3D_invert(uint32_t x) {
    x = x & 0x49249249u;
    x = (x | (x >> 2)) & 0xc30c30c3u;
    x = (x | (x >> 4)) & 0x0f00f00fu;
    x = (x | (x >> 8)) & 0xff0000ffu;
    x = (x | (x >> 16)) & 0x0000ffffu;
    return x;
}

// PCG32 (raymarching/src/pcg32.h:44-170), seeded on the host, advanced per ray on device.
struct Pcg32 {
    uint64_t state, inc;
    __host__ __device__ uint32_t next_uint() {
        const uint64_t old = state;
        state = old * 0x5851f42d4c957f2dULL + inc;
        const uint32_t xs = (uint32_t)(((old >> 18u) ^ old) >> 27u);
        const uint32_t rot = (uint32_t)(old >> 59u);
        return (xs >> rot) | (xs << ((~rot + 1u) & 31));
    }
    __host__ __device__ void seed(uint64_t initstate, uint64_t initseq = 1) {
        state = 0u;
        inc = (initseq << 1u) | 1u;
        next_uint();
        state += initstate;
        next_uint();
    }
    __host__ __device__ float next_float() {
        union { uint32_t u; float f; } x;
        x.u = (next_uint() >> 9) | 0x3f800000u;
        return x.f - 1.0f;
    }
    __host__ __device__ void advance(int64_t delta_) {
        uint64_t cur_mult = 0x5851f42d4c957f2dULL, cur_plus = inc, acc_mult = 1u, acc_plus = 0u;
        uint64_t delta = (uint64_t)delta_;
        while (delta > 0) {
            if (delta & 1) { acc_mult *= cur_mult; acc_plus = acc_plus * cur_mult + cur_plus; }
            cur_plus = (cur_mult + 1) * cur_plus;
            cur_mult *= cur_mult;
            delta /= 2;
        }
        state = acc_mult * state + acc_plus;
    }
};

// ---- derived copies of the occupancy bits (power-of-two H): the x-fastest re-layout (k_build_linear: same cells, same bits, read by
// Dda::probe_lin) and its 1:64 reduction, one bit per 4x4x4 block (k_build_coarse_linear), which the kernels stage into LDS.
struct OccupancyLin {
    const uint32_t* lin;
    const uint32_t* coarse;
    uint32_t coarse_words, logH;   // coarse_words == 0: no coarse bits (the probes go unfiltered)
};
constexpr size_t kCoarseMaxBytes = 8192;   // LDS budget of every kernel that stages the coarse bits (C * H^3 / 64 bits)

// block-wide: `coarse` into the caller's LDS array (kCoarseMaxBytes / 4 words); the caller synchronises before the first probe
__device__ __forceinline__ void stage_coarse(const OccupancyLin& ol, uint32_t* coarse_lds, uint32_t block_threads) {
    for (uint32_t i = threadIdx.x; i < ol.coarse_words; i += block_threads) coarse_lds[i] = ol.coarse[i];
}

// host side and the build kernels (occupancy.hip).  A grid has derived copies when H is a power of two >= 8, its bitfield is 8-byte
// aligned and the two copies fit the caller's buffers; the callers differ in those caps (DESIGN.md "Occupancy sources").  `grid` NULL:
// the operator sizes its buffer before it has the bitfield, and requires the alignment when it builds.
bool occupancy_lin_fits(uint32_t C, uint32_t H, const uint8_t* grid, size_t lin_cap_bytes, size_t coarse_cap_bytes);
OccupancyLin occupancy_lin_view(uint32_t C, uint32_t H, const void* lin, const void* coarse);   // the struct over copies that exist
OccupancyLin build_occupancy_lin(const uint8_t* grid, uint32_t C, uint32_t H, void* lin_out, void* coarse_out, hipStream_t stream);
// the Morton-order coarse bits of a grid without a linear copy (Dda::probe): one bit per aligned 8-byte word of the bitfield.  The render
// loop launches it itself; k_build_linear and k_build_coarse_linear are launched by build_occupancy_lin alone.
__global__ void k_build_coarse(const unsigned long long* __restrict__ bitfield64, uint32_t n_words, unsigned long long* __restrict__ coarse);

// ---- the occupancy-grid DDA shared by march_rays_train / march_rays / the fused renderer.
// Follows raymarching.cu:357-404 (identical text at :431-483 and :757-813).
struct Dda {
    float ox, oy, oz, dx, dy, dz, rdx, rdy, rdz;
    float bound, rbound, dt_gamma, dt_min, dt_max, dt_c, rH, H3f, Cf, Hf, Hm1, halfH;
    double Hd;
    bool h_pow2, const_dt;
    int level_dt0;
    float t_fast_min;   // constant-step skips use a closed form for t >= this (see skip_const_dt)
    // fused renderer only (H a power of two): occupancy bits re-laid out x-fastest by k_build_linear (same cells, same bits)
    const uint32_t* grid_lin;
    uint32_t logH;
    int sx, sy, sz;     // 1 where the direction component is >= +0 (signf == +1), else 0
    float two_rH;
    float jump_guard;   // rounding allowance of a block-exit time per unit of |1/d| of the axis it is taken on (see jump_block)
    bool block_jump;    // leave empty 4x4x4 blocks in one step (A/B switch)
    const uint8_t* grid;

    __device__ __forceinline__ void init(const float* o, const float* d, const uint8_t* g, float bound_, float dt_gamma_,
                                         uint32_t max_steps, uint32_t C, uint32_t H) {
        ox = o[0]; oy = o[1]; oz = o[2];
        dx = d[0]; dy = d[1]; dz = d[2];
        rdx = 1 / dx; rdy = 1 / dy; rdz = 1 / dz;
        rH = 1 / (float)H;
        H3f = (float)(H * H * H);
        bound = bound_; rbound = 1 / bound_; dt_gamma = dt_gamma_;
        const float SQRT3 = 1.7320508075688772f;
        dt_min = 2 * SQRT3 / (float)max_steps;
        dt_max = 2 * SQRT3 * (float)(1 << (C - 1)) / (float)H;
        Cf = (float)C; Hf = (float)H; Hm1 = (float)(H - 1); Hd = (double)H;
        h_pow2 = (H & (H - 1)) == 0;
        halfH = 0.5f * Hf;
        grid = g;
        // dt_gamma == 0 (the default): clamp(t * 0, dt_min, dt_max) = fminf(dt_max, fmaxf(0, dt_min)) (:26) for every t, so the step
        // and its mip level are constants -- dt_min normally, dt_max when max_steps is so small that dt_min exceeds it
        const_dt = dt_gamma_ == 0.0f;
        dt_c = fminf(dt_max, fmaxf(0.0f, dt_min));
        level_dt0 = mip_from_dt(dt_c);
        // dt_c = m * 2^(ed-23).  Added to a t of exponent e it is rounded to a multiple of ulp(t) = 2^(e-23); that rounding is a
        // tie (and then depends on the parity of t) only in the one binade e = ed + ctz(m) + 1.  Everywhere above it the rounded
        // step is a per-binade constant.
        const uint32_t b = __float_as_uint(dt_c);
        const uint32_t m = (b & 0x7FFFFFu) | 0x800000u;
        t_fast_min = __uint_as_float(((b >> 23) + (uint32_t)__ffs((int)m) + 1u) << 23);
    }

    __device__ __forceinline__ void init_lin(const uint32_t* lin, uint32_t logH_, bool block_jump_) {
        grid_lin = lin;
        block_jump = block_jump_;
        logH = logH_;
        sx = (int)((__float_as_uint(dx) >> 31) ^ 1u);
        sy = (int)((__float_as_uint(dy) >> 31) ^ 1u);
        sz = (int)((__float_as_uint(dz) >> 31) ^ 1u);
        two_rH = 2.0f * rH;
        jump_guard = bound * 9.5367431640625e-7f;   // 2^-20: eight ulps of a coordinate
    }

    // The preamble of a march: init, the linear copies if the kernel probes through them (`ol` NULL: the Morton-order originals, `block_jump_`
    // unused), and the reference's jitter (:349-352, :733-736).  Returns the start t.  (Not every march opens with it: see k_march_train_count.)
    __device__ __forceinline__ float start(const float* o, const float* d, const uint8_t* g, float bound_, float dt_gamma_, uint32_t max_steps,
                                           uint32_t C, uint32_t H, const OccupancyLin* ol, bool block_jump_, float t, uint32_t perturb, Pcg32 rng,
                                           uint32_t index) {
        init(o, d, g, bound_, dt_gamma_, max_steps, C, H);
        if (ol) init_lin(ol->lin, ol->logH, block_jump_);
        if (perturb) {
            rng.advance((int64_t)index);
            t += dt_min * rng.next_float();
        }
        return t;
    }

    // `do { t += dt_c; } while (t < tt);` (:395-403 with a constant step) without the loop.  Inside one binade above the tie
    // binade every addition advances t by the same d = fl(t + dt_c) - t exactly (t and d are multiples of ulp(t), the sums
    // stay below the next power of two), so the loop ends at the smallest lattice point t1 + k*d >= tt.  k comes from an
    // approximate quotient and is corrected by one step either way; fmaf(k, d, t1) is exact because the true value is
    // representable.  Anything else (binade crossing, tiny t) falls back to the loop.
    __device__ __forceinline__ void skip_const_dt(float& t, float tt) const {
        const float t1 = t + dt_c;
        if (!(t1 < tt)) { t = t1; return; }
        const float d = t1 - t;
        const float r = tt - t1;
        float t2 = fmaf(ceilf(r * __builtin_amdgcn_rcpf(d)), d, t1);
        if (t2 < tt) t2 += d;
        else if (t2 - d >= tt) t2 -= d;
        const bool same_binade = ((__float_as_uint(t2) ^ __float_as_uint(t)) >> 23) == 0;
        if (same_binade && t >= t_fast_min) { t = t2; return; }
        t = t1;
        do { t += dt_c; } while (t < tt);
    }

    __device__ __forceinline__ int mip_from_pos(float x, float y, float z) const {   // :44-49
        const float mx = fmaxf(fabsf(x), fmaxf(fabsf(y), fabsf(z)));
        int e;
        frexpf(mx, &e);
        return (int)fminf(Cf - 1, fmaxf(0.0f, (float)e));
    }
    __device__ __forceinline__ int mip_from_dt(float dt) const {                     // :51-56 (x0.5 in double is exact)
        const float mx = (dt * Hf) * 0.5f;
        int e;
        frexpf(mx, &e);
        return (int)fminf(Cf - 1, fmaxf(0.0f, (float)e));
    }
    // :378-380.  The reference's `0.5 * (...) * H` is a double product; for a power-of-two H it only rescales the
    // float value fmaf(v, rb, 1) by 2^k, which is exact in float as well, so the double detour is skipped.
    // (Every entry point refuses any other H on the host -- grid_size_ok, ngp_common.hpp -- so the double branch is never taken.  It
    // stays: without it the render loop's march kernels compile to other code, measured 1 % slower on the frame benchmark.)
    __device__ __forceinline__ int cell(float v, float mip_rbound) const {
        const float a = fmaf(v, mip_rbound, 1.0f);
        const float s = h_pow2 ? a * halfH : (float)(0.5 * (double)a * Hd);
        return (int)clampf(s, 0.0f, Hm1);
    }

    // True when the 4x4x4 block containing the march position at t is empty according to the coarse occupancy bits
    // (same cell arithmetic as probe()).  Used only to PREDICT that a ray's next march starts with a long skip.
    __device__ __forceinline__ bool coarse_empty_at(float t, const uint32_t* coarse) const {
        const float x = clampf(fmaf(t, dx, ox), -bound, bound);
        const float y = clampf(fmaf(t, dy, oy), -bound, bound);
        const float z = clampf(fmaf(t, dz, oz), -bound, bound);
        const float dt = const_dt ? dt_c : clampf(t * dt_gamma, dt_min, dt_max);
        const int lp = mip_from_pos(x, y, z), ld = const_dt ? level_dt0 : mip_from_dt(dt);
        const int level = lp > ld ? lp : ld;
        const float pw = (float)(1 << level);
        const float mip_rbound = pw <= bound ? __uint_as_float((uint32_t)(127 - level) << 23) : rbound;
        const uint32_t index = (uint32_t)((float)level * H3f + (float)morton3D_cell((uint32_t)cell(x, mip_rbound), (uint32_t)cell(y, mip_rbound),
                                                                                    (uint32_t)cell(z, mip_rbound)));
        // (testing the fine cell as well groups 3x more of the skipping rays -- march lane utilisation 66 % instead of 26 % --
        //  but was measured SLOWER overall: with the march that short, more waves gather at once and thrash L1/L2)
        return ((coarse[index >> 11] >> ((index >> 6) & 31u)) & 1u) == 0;
    }

    // ---- power-of-two H, linear bit layout (fused renderer) -------------------------------------------------------
    // Same decisions and the same t as probe(), with cheaper arithmetic:
    //  * clampf = v_med3_f32 (identical for non-NaN arguments);
    //  * bit index level*H^3 + (z*H + y)*H + x into the re-laid-out copy instead of the Morton index into the original;
    //  * the voxel face ((n + 0.5 + 0.5*sign(d)) / H) * 2 - 1 of :386-388 is (n + s) * (2/H) - 1 with s in {0, 1}: every
    //    intermediate of the reference expression is exact when H is a power of two, so one fma gives the same float.
    __device__ __forceinline__ int cell_pow2(float v, float mip_rbound) const {
        return (int)__builtin_amdgcn_fmed3f(fmaf(v, mip_rbound, 1.0f) * halfH, 0.0f, Hm1);
    }
    __device__ __forceinline__ void locate_lin(float t, float& x, float& y, float& z, float& dt, int& level, float& mip_bound, int& nx, int& ny,
                                               int& nz) const {
        x = __builtin_amdgcn_fmed3f(fmaf(t, dx, ox), -bound, bound);
        y = __builtin_amdgcn_fmed3f(fmaf(t, dy, oy), -bound, bound);
        z = __builtin_amdgcn_fmed3f(fmaf(t, dz, oz), -bound, bound);
        dt = const_dt ? dt_c : clampf(t * dt_gamma, dt_min, dt_max);
        const int lp = mip_from_pos(x, y, z), ld = const_dt ? level_dt0 : mip_from_dt(dt);
        level = lp > ld ? lp : ld;
        const float pw = (float)(1 << level);
        const bool use_pw = pw <= bound;
        mip_bound = use_pw ? pw : bound;
        const float mip_rbound = use_pw ? __uint_as_float((uint32_t)(127 - level) << 23) : rbound;
        nx = cell_pow2(x, mip_rbound); ny = cell_pow2(y, mip_rbound); nz = cell_pow2(z, mip_rbound);
    }
    __device__ __forceinline__ uint32_t coarse_index_lin(int level, int nx, int ny, int nz) const {
        const uint32_t lb = logH - 2;   // log2 of blocks per axis
        return ((uint32_t)level << (3 * lb)) + ((((uint32_t)nz >> 2) << (2 * lb)) | (((uint32_t)ny >> 2) << lb) | ((uint32_t)nx >> 2));
    }
    __device__ __forceinline__ bool coarse_empty_at_lin(float t, const uint32_t* coarse) const {
        float x, y, z, dt, mip_bound;
        int level, nx, ny, nz;
        locate_lin(t, x, y, z, dt, level, mip_bound, nx, ny, nz);
        const uint32_t ci = coarse_index_lin(level, nx, ny, nz);
        return ((coarse[ci >> 5] >> (ci & 31u)) & 1u) == 0;
    }
    // Leaving an EMPTY 4x4x4 block in one step.  The reference walks it cell by cell (:386-403): from a lattice point in an empty
    // cell it goes to the first lattice point at or beyond that cell's exit, and so on; every point it visits inside the block
    // is empty, so nothing is sampled there, and the walk leaves through a face of the last cell that is also a face of the
    // block -- at the first lattice point >= T*, the exit time of the BLOCK.  T* evaluated here and the reference's last-cell exit
    // are the same plane crossing rounded differently, so the shortcut is taken only when no lattice point lies within a
    // generous rounding allowance of T* (then both pick the same point) and the constant-step lattice is exact (one binade,
    // see skip_const_dt); otherwise the caller falls back to the cell walk.  The block must also be "pure": every position in
    // it has to select this cascade level, which can fail only above the step-size level where the block may reach into the
    // next finer cascade's cube.
    __device__ __forceinline__ bool jump_block(float& t, float x, float y, float z, int level, float mip_bound, int nx, int ny, int nz) const {
        const float bx = fmaf((float)((nx & ~3) + 4 * sx), two_rH, -1.0f), by = fmaf((float)((ny & ~3) + 4 * sy), two_rH, -1.0f),
                    bz = fmaf((float)((nz & ~3) + 4 * sz), two_rH, -1.0f);
        if (level > level_dt0) {
            if (mip_bound != (float)(1 << level)) return false;   // top cascade of a non-power-of-two bound: units differ, walk the cells
            // distance of the block from the origin in the max norm, in units of mip_bound: pure iff >= 1/2 (the finer cube's half size)
            const float cell4 = 4.0f * two_rH;
            const float ox_ = sx ? bx - cell4 : bx, oy_ = sy ? by - cell4 : by, oz_ = sz ? bz - cell4 : bz;   // low faces
            const float mx = (ox_ <= 0.0f && ox_ + cell4 >= 0.0f) ? 0.0f : fminf(fabsf(ox_), fabsf(ox_ + cell4));
            const float my = (oy_ <= 0.0f && oy_ + cell4 >= 0.0f) ? 0.0f : fminf(fabsf(oy_), fabsf(oy_ + cell4));
            const float mz = (oz_ <= 0.0f && oz_ + cell4 >= 0.0f) ? 0.0f : fminf(fabsf(oz_), fabsf(oz_ + cell4));
            if (fmaxf(mx, fmaxf(my, mz)) < 0.5f) return false;
        }
        const float tx = fmaf(bx, mip_bound, -x) * rdx, ty = fmaf(by, mip_bound, -y) * rdy, tz = fmaf(bz, mip_bound, -z) * rdz;
        const float tmin = fminf(tx, fminf(ty, tz));
        const float tt = t + fmaxf(0.0f, tmin);
        const float t1 = t + dt_c;
        if (!(t1 < tt)) return false;
        const float d = t1 - t;
        float t2 = fmaf(ceilf((tt - t1) * __builtin_amdgcn_rcpf(d)), d, t1);
        if (t2 < tt) t2 += d;
        else if (t2 - d >= tt) t2 -= d;
        // The allowance: a face-crossing time (face - x) / d carries the coordinate's rounding times |1/d| -- e_a = |1/d_a| * 8 ulp(bound),
        // sixteen times what either side's evaluation can be off by.  Only axes that can be the minimum count: one whose crossing lies
        // beyond the minimum by more than both allowances is not the exit face here, nor in the reference's last cell (its own value of
        // that crossing differs from this one by less than e_a / 8).  A ray almost parallel to an axis (|1/d| in the thousands: two or
        // three pixel columns of a frame) used to have every jump refused on that axis' account and walked 200 cells of empty space
        // one by one -- the launch-wide march lasts as long as its slowest ray.  (infinite / NaN crossings -- d_a = 0 -- fail every
        // comparison below, as they are ignored by fminf on both sides.)
        const float ex = fabsf(rdx) * jump_guard, ey = fabsf(rdy) * jump_guard, ez = fabsf(rdz) * jump_guard;
        const float em = tmin == tx ? ex : (tmin == ty ? ey : ez);
        const float lim = tmin + em;
        float ga = em;
        if (tx - ex <= lim) ga = fmaxf(ga, ex);
        if (ty - ey <= lim) ga = fmaxf(ga, ey);
        if (tz - ez <= lim) ga = fmaxf(ga, ez);
        const float guard = fmaf(t2, 9.5367431640625e-7f, ga);
        const bool clear = (t2 - tt) > guard && (tt - (t2 - d)) > guard;   // false for NaN / infinite allowances as well
        const bool same_binade = ((__float_as_uint(t2) ^ __float_as_uint(t)) >> 23) == 0;
        if (!(clear && same_binade && t >= t_fast_min)) return false;
        t = t2;
        return true;
    }

    // `occupied_until` (optional): when the probe finds its cell occupied, the time up to which every later position of the ray is
    // CERTAIN to be located in this same cell by the reference's arithmetic -- the cell's exit time less the rounding allowance of
    // jump_block (all three axes counted: a generous bound).  A position before it moves towards each exit face and stays eight ulps of a
    // coordinate short of it, so its cell indices are these.  The cascade level must not change inside the cell either: it changes at the
    // cube surfaces |p| = 2^k, and those are faces of this level's cells only when the cells tile the cube of half size 2^level
    // (mip_bound == 2^level: the surfaces lie at cell coordinates H/4, 3H/4, 0 and H).  Where mip_bound is the scene bound instead --
    // the top cascade of a non-power-of-two bound (bound 1.5, H 64: |x| = 1 is at cell coordinate 53.33), or a level above
    // log2(bound), which only a position clamped onto the box selects (bound 8, C 8) -- a surface cuts through cells, the next position
    // may belong to a finer level whose cell is empty, and nothing is certain: *occupied_until = t (jump_block refuses the same case).
    // The march can take its samples up to there without probing (the samples' own arithmetic -- t, dt, t += dt -- is untouched).
    __device__ __forceinline__ bool probe_lin(float& t, float& x, float& y, float& z, float& dt, const uint32_t* coarse,
                                              float* occupied_until = nullptr) const {
        float mip_bound;
        int level, nx, ny, nz;
        locate_lin(t, x, y, z, dt, level, mip_bound, nx, ny, nz);
        const uint32_t ci = coarse_index_lin(level, nx, ny, nz);
        bool occ = false;
        if ((coarse[ci >> 5] >> (ci & 31u)) & 1u) {
            const uint32_t fi = ((uint32_t)level << (3 * logH)) + (((uint32_t)nz << (2 * logH)) | ((uint32_t)ny << logH) | (uint32_t)nx);
            occ = ((grid_lin[fi >> 5] >> (fi & 31u)) & 1u) != 0;
            if (occ && occupied_until) {
                const float tx = fmaf(fmaf((float)(nx + sx), two_rH, -1.0f), mip_bound, -x) * rdx;
                const float ty = fmaf(fmaf((float)(ny + sy), two_rH, -1.0f), mip_bound, -y) * rdy;
                const float tz = fmaf(fmaf((float)(nz + sz), two_rH, -1.0f), mip_bound, -z) * rdz;
                const float tt = t + fminf(tx, fminf(ty, tz));
                const float g = fmaf(tt, 9.5367431640625e-7f, (fabsf(rdx) + fabsf(rdy) + fabsf(rdz)) * jump_guard);
                const float until = tt - g;
                // (NaN / infinite allowances, or a cell that a cascade surface cuts through: nothing is certain)
                *occupied_until = (until > t && mip_bound == (float)(1 << level)) ? until : t;
            }
        } else if (const_dt && block_jump && jump_block(t, x, y, z, level, mip_bound, nx, ny, nz)) {
            return false;
        }
        if (!occ) {
            const float tx = fmaf(fmaf((float)(nx + sx), two_rH, -1.0f), mip_bound, -x) * rdx;
            const float ty = fmaf(fmaf((float)(ny + sy), two_rH, -1.0f), mip_bound, -y) * rdy;
            const float tz = fmaf(fmaf((float)(nz + sz), two_rH, -1.0f), mip_bound, -z) * rdz;
            const float tt = t + fmaxf(0.0f, fminf(tx, fminf(ty, tz)));
            if (const_dt) {
                skip_const_dt(t, tt);
            } else {
                do { t += clampf(t * dt_gamma, dt_min, dt_max); } while (t < tt);
            }
        }
        return occ;
    }

    // Probe at t. Occupied: returns true with x,y,z,dt set (caller advances t += dt).
    // Empty: t is advanced past the next voxel boundary (:386-403) and false is returned.
    // `coarse` (optional, LDS): one bit per 64 consecutive cells of the Morton-ordered bitfield (= a 4x4x4 block); a clear
    // bit proves the probed cell empty without touching global memory.
    __device__ __forceinline__ bool probe(float& t, float& x, float& y, float& z, float& dt, const uint32_t* coarse = nullptr) const {
        x = clampf(fmaf(t, dx, ox), -bound, bound);
        y = clampf(fmaf(t, dy, oy), -bound, bound);
        z = clampf(fmaf(t, dz, oz), -bound, bound);
        dt = const_dt ? dt_c : clampf(t * dt_gamma, dt_min, dt_max);
        const int lp = mip_from_pos(x, y, z), ld = const_dt ? level_dt0 : mip_from_dt(dt);
        const int level = lp > ld ? lp : ld;
        // mip_bound = min(2^level, bound); 1 / mip_bound is exact for the power of two (built from its exponent)
        // and the precomputed 1 / bound otherwise: same values as the reference's IEEE division (:373-374)
        const float pw = (float)(1 << level);
        const bool use_pw = pw <= bound;
        const float mip_bound = use_pw ? pw : bound;
        const float mip_rbound = use_pw ? __uint_as_float((uint32_t)(127 - level) << 23) : rbound;
        const int nx = cell(x, mip_rbound), ny = cell(y, mip_rbound), nz = cell(z, mip_rbound);
        const uint32_t index = (uint32_t)((float)level * H3f + (float)morton3D_cell((uint32_t)nx, (uint32_t)ny, (uint32_t)nz));
        bool occ;
        if (coarse != nullptr && ((coarse[index >> 11] >> ((index >> 6) & 31u)) & 1u) == 0) occ = false;
        else occ = (grid[index >> 3] & (1u << (index & 7u))) != 0;
        if (!occ) {
            const float tx = fmaf(fmaf(0.5f, signf(dx), (float)nx + 0.5f) * rH * 2 - 1, mip_bound, -x) * rdx;
            const float ty = fmaf(fmaf(0.5f, signf(dy), (float)ny + 0.5f) * rH * 2 - 1, mip_bound, -y) * rdy;
            const float tz = fmaf(fmaf(0.5f, signf(dz), (float)nz + 0.5f) * rH * 2 - 1, mip_bound, -z) * rdz;
            const float tt = t + fmaxf(0.0f, fminf(tx, fminf(ty, tz)));
            if (const_dt) {
                skip_const_dt(t, tt);
            } else {
                do { t += clampf(t * dt_gamma, dt_min, dt_max); } while (t < tt);
            }
        }
        return occ;
    }
};

// ---- one wave per ray on the step lattice (k_march_train_count_wave, march_ahead_wave) ------------------------------------------
// With dt_gamma == 0 every t the march visits lies on the lattice t0, t0 + dt, (t0 + dt) + dt, ... of the sequential additions, and inside
// one binade above Dda::t_fast_min those additions are exact: point k is fmaf(k, d, t) with d = fl(t + dt) - t (skip_const_dt's argument).
// Lane l therefore evaluates the probe AT lattice point l of a 64-point window that starts at the march's current t -- the same pure
// function of t the sequential march evaluates, returning whether the cell is occupied and where the march goes next from there (one step
// for a sample, the cell / block exit for an empty cell).  The caller then follows the chain 0 -> j(0) -> j(j(0)) ... through the window
// from registers (v_readlane): the points on it are exactly the ones the sequential march visits, the occupied ones among them its
// samples, in order.  A point the chain cannot vouch for ends the window -- another binade (the step d changes there), t below the exact
// regime, a point at or beyond `far`, a continuation that is not a lattice point: the march goes on from `nxt` of the last point
// visited, the exact t the sequential march would have, and point 0 alone is always valid.
struct LatticeWindow {
    float p, dt, nxt;                  // this lane's lattice point, the step of a sample taken there, and where the march continues from it
    uint32_t j;                        // index of `nxt` in the window; 64: it leaves the window or is not one of its points
    unsigned long long vmask, omask;   // the wave's valid points, and the occupied ones among them
};
__device__ __forceinline__ LatticeWindow probe_window(const Dda& s, float t, float far, uint32_t lane, const uint32_t* coarse) {
    LatticeWindow w;
    const float t1 = t + s.dt_c, d = t1 - t;
    w.p = lane == 0 ? t : fmaf((float)lane, d, t);
    const bool exact = t >= s.t_fast_min && ((__float_as_uint(w.p) ^ __float_as_uint(t)) >> 23) == 0;
    const bool valid = lane == 0 || (exact && w.p < far);
    float x, y, z;
    w.nxt = w.p;
    w.dt = 0.0f;
    w.j = 64;
    bool occ = false;
    if (valid) {
        occ = s.probe_lin(w.nxt, x, y, z, w.dt, coarse);      // empty: nxt moves on to where the march continues
        if (occ) w.nxt = w.p + w.dt;
    }
    if (valid) {      // (a block of its own: merged with the probe's, the compiler schedules both callers differently)
        const float q = rintf((w.nxt - t) * __builtin_amdgcn_rcpf(d));
        if (q >= 1.0f && q < 64.0f && fmaf(q, d, t) == w.nxt) w.j = (uint32_t)q;      // exact when it is a lattice point
    }
    w.vmask = __ballot(valid);
    w.omask = __ballot(occ);
    return w;
}

// ---- per-ray counts -> slots ----------------------------------------------------------------------------------------------------
// Exclusive prefix of one value per thread over a block of THREADS threads (every thread calls; one barrier inside).  `wave_tot`:
// THREADS / 64 words of LDS, free again after the caller's next barrier.
template <int THREADS>
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* wave_tot) {
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint32_t incl = scan_inclusive<AddOp>(v, lane);
    if (lane == 63) wave_tot[wid] = incl;
    __syncthreads();
    uint32_t wave_off = 0;
    for (uint32_t w = 0; w < wid; w++) wave_off += wave_tot[w];
    return wave_off + incl - v;
}
// One 1024-thread block turns sums[0 .. n) into their exclusive prefix in place, 1024 at a time with a carry, and returns the total.
__device__ __forceinline__ uint32_t scan_in_place_1024(uint32_t* __restrict__ sums, uint32_t n) {
    __shared__ uint32_t wave_tot[16];
    __shared__ uint32_t carry_s;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (uint32_t start = 0; start < n; start += 1024) {
        const uint32_t i = start + threadIdx.x;
        const uint32_t v = i < n ? sums[i] : 0;
        const uint32_t excl = block_exclusive_scan<1024>(v, wave_tot);
        const uint32_t carry = carry_s;
        if (i < n) sums[i] = carry + excl;
        __syncthreads();
        if (threadIdx.x == 1023) carry_s = carry + excl + v;
        __syncthreads();
    }
    return carry_s;
}

}  // namespace ngp
