// fused_net.hpp -- the hash-grid + MLP network as the fused kernels evaluate it: one 16-sample tile per wave, activations in
// registers, weights in LDS as ready-made MFMA fragments.  Device side: the fragment orders (perm_*), the fp16 and fp32 MLP layers
// forward and backward, the gathers, and the two policy classes NetF16 / NetF32 that every fused kernel is a template over
// (NeRFNetwork.density / .forward of nerf/network_ff.py and nerf/network.py, gridencoder.cu's encoder, shencoder.cu's SH).
// Host side: what a unit needs to fill NetArgs and pick the kernel variant of a model; defined once, in fused_net.hip.
// Included by fused_net.hip, fused_query.hip, render_uniform.hip and render_fused.hip.
#pragma once
#include <hip/hip_fp16.h>
#include <math.h>

#include "ngp_common.hpp"

namespace ngp {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// per-level table staged in LDS (16 levels)
struct LevelTab {
    float scale[16];
    uint32_t offset[16], size[16];
    uint32_t a1[16], a2[16];   // per-dimension multipliers: the hash primes for hashed levels, the dense strides otherwise
    uint32_t mask[16];         // index reduction as an AND: size-1 (power-of-two size), ~0 (dense: already < size)
    uint32_t flags[16];        // bit0 hashed, bit1 needs a generic modulo (only in the GENERIC kernel variants)
    uint32_t cell_off[16], cell_res[16];   // per-cell corner records (NetArgs::cells): first record and cells per axis
};

struct NetArgs {
    const uint32_t* table;     // fp16 pairs viewed as u32
    const _Float16* packed;    // fragment-major weights (global)
    uint32_t sig_mm, col_mm;   // hidden->hidden matmuls
    float bound, inv_two_bound, density_scale;
    int align_corners;
    // per-cell corner records of the first 4 * cell_steps levels (ngp_build_cell_tables), or null: record (level, cx, cy, cz) =
    // the 8 table entries the cell's corners map to, 32 contiguous bytes instead of 8 gathers from up to 4 cache lines
    const uint4* cells;
    uint32_t cell_steps;
    uint32_t cell_off[16];     // first record of a level
    // bit 8: ngp_model::precision == NGP_PREC_F32 (`table` holds float pairs, `packed` float fragments: NetF32 below); bit 9: ... == NGP_PREC_F16_REF
    // (host side only: selects the HACC kernel instantiations).  (One word: the struct is a kernel argument of the tuned render loop.)
    uint32_t prec_bits;
    __host__ __device__ bool f32() const { return (prec_bits & 256u) != 0; }
    __host__ __device__ bool hacc() const { return (prec_bits & 512u) != 0; }
};

__host__ __device__ inline uint32_t sig_halfs(uint32_t mm) { return 2048 + mm * 4096 + 1024; }
__host__ __device__ inline size_t net_w_bytes_f16(const NetArgs& na) { return (size_t)(sig_halfs(na.sig_mm) + sig_halfs(na.col_mm)) * 2; }
// bytes of the packed forward weights of both nets (the LDS image every fused kernel starts with)
__host__ __device__ inline size_t net_w_bytes(const NetArgs& na) {
    return (size_t)(sig_halfs(na.sig_mm) + sig_halfs(na.col_mm)) * (na.f32() ? 4 : 2);
}

// ------------------------------------------------------------------------------------------
// weight fragment packing.  Source blobs are FFMLP-layout [64 x 32 | mm x 64 x 64 | 16 x 64].
// Destination: for every (layer, 16-row block ob, 32-wide k step s, lane) 8 halfs = the lane's
// A fragment for v_mfma_f32_16x16x32_f16 (row = 16*ob + (lane & 15), k index permuted):
//   first sigma layer : k(q, j) = 2*(q + 4*(j >> 1)) + (j & 1)      (lane q gathers levels q, q+4, q+8, q+12)
//   first colour layer: k(q, j) = j < 4 ? 4q + j                      (SH 4q..4q+3)
//                                : (q == 0 && j == 4) ? 31           (the zero pad feature sits where lane 0 holds sigma)
//                                : 15 + 4q + (j - 4)                  (geo_feat = sigma-net outputs 4q..4q+3, shifted by 15)
//   hidden / output   : k(q, j, s) = 32 s + 16*(j >> 2) + 4q + (j & 3)  (accumulators of row blocks 2s, 2s+1)
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t perm_grid(uint32_t q, uint32_t j) { return 2 * (q + 4 * (j >> 1)) + (j & 1); }
__device__ __forceinline__ uint32_t perm_color(uint32_t q, uint32_t j) {
    return j < 4 ? 4 * q + j : ((q == 0 && j == 4) ? 31u : 15 + 4 * q + (j - 4));
}
__device__ __forceinline__ uint32_t perm_hidden(uint32_t q, uint32_t j, uint32_t s) { return 32 * s + 16 * (j >> 2) + 4 * q + (j & 3); }

// (launched by ngp_pack_weights and, for a model without packed weights, by ngp_render_rays)
__global__ void k_pack_weights(const _Float16* __restrict__ sig, uint32_t sig_mm, const _Float16* __restrict__ col, uint32_t col_mm,
                               _Float16* __restrict__ packed);

// ------------------------------------------------------------------------------------------
// the network on one 16-sample tile.  All 64 lanes participate; lane = (c = sample, q = quarter).
// Returns in lanes with q == 0: sigma (trunc_exp output, unscaled) and rgb (fp16-rounded sigmoid).
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ half8 relu_pack(const f32x4& a, const f32x4& b) {
    half8 h;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const _Float16 x = (_Float16)a[r], y = (_Float16)b[r];
        h[r] = x > (_Float16)0 ? x : (_Float16)0;
        h[4 + r] = y > (_Float16)0 ? y : (_Float16)0;
    }
    return h;
}

__device__ __forceinline__ void mlp_in(const half8* W, uint32_t lane, half8 x, half8 (&h)[2]) {
    f32x4 acc[4];
#pragma unroll
    for (int ob = 0; ob < 4; ob++) acc[ob] = __builtin_amdgcn_mfma_f32_16x16x32_f16(W[ob * 64 + lane], x, (f32x4){0, 0, 0, 0}, 0, 0, 0);
    h[0] = relu_pack(acc[0], acc[1]);
    h[1] = relu_pack(acc[2], acc[3]);
}
__device__ __forceinline__ void mlp_hidden(const half8* W, uint32_t lane, half8 (&h)[2]) {
    f32x4 acc[4];
#pragma unroll
    for (int ob = 0; ob < 4; ob++) {
        acc[ob] = __builtin_amdgcn_mfma_f32_16x16x32_f16(W[(ob * 2 + 0) * 64 + lane], h[0], (f32x4){0, 0, 0, 0}, 0, 0, 0);
        acc[ob] = __builtin_amdgcn_mfma_f32_16x16x32_f16(W[(ob * 2 + 1) * 64 + lane], h[1], acc[ob], 0, 0, 0);
    }
    h[0] = relu_pack(acc[0], acc[1]);
    h[1] = relu_pack(acc[2], acc[3]);
}
__device__ __forceinline__ f32x4 mlp_out(const half8* W, uint32_t lane, const half8 (&h)[2]) {
    f32x4 o = __builtin_amdgcn_mfma_f32_16x16x32_f16(W[lane], h[0], (f32x4){0, 0, 0, 0}, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(W[64 + lane], h[1], o, 0, 0, 0);
}

// degree-4 real SH of a direction, the 4 values index 4q..4q+3 (shencoder.cu:51-70 as products, see shencoder.hip)
__device__ __forceinline__ void sh4_quarter(uint32_t q, float x, float y, float z, float (&o)[4]) {
    const float xy = x * y, xz = x * z, yz = y * z, x2 = x * x, y2 = y * y, z2 = z * z;
    if (q == 0) {
        o[0] = 0.28209479177387814f;
        o[1] = -0.48860251190291987f * y;
        o[2] = 0.48860251190291987f * z;
        o[3] = -0.48860251190291987f * x;
    } else if (q == 1) {
        o[0] = 1.0925484305920792f * xy;
        o[1] = -1.0925484305920792f * yz;
        o[2] = 0.94617469575755997f * z2 - 0.31539156525251999f;
        o[3] = -1.0925484305920792f * xz;
    } else if (q == 2) {
        o[0] = 0.54627421529603959f * x2 - 0.54627421529603959f * y2;
        o[1] = 0.59004358992664352f * y * (-3.0f * x2 + y2);
        o[2] = 2.8906114426405538f * xy * z;
        o[3] = 0.45704579946446572f * y * (1.0f - 5.0f * z2);
    } else {
        o[0] = 0.3731763325901154f * z * (5.0f * z2 - 3.0f);
        o[1] = 0.45704579946446572f * x * (1.0f - 5.0f * z2);
        o[2] = 1.4453057213202769f * z * (x2 - y2);
        o[3] = 0.59004358992664352f * x * (-x2 + 3.0f * y2);
    }
}

// ---- the encoder's per-sample arithmetic, shared by every gather below ------------------------------------------------------------
typedef float f32x2 __attribute__((ext_vector_type(2)));

// Encoder input (x + bound) / (2 bound) (gridencoder/grid.py:144) and the out-of-range test of gridencoder.cu:107-123: an
// out-of-range point gathers at the centre (in range) and has its features zeroed by the callers.
// CLAMPED: a compile-time promise of the call site that (x, y, z) went through clampf(., -bound, bound) AND that 2*bound is a power
// of two (clamped_exact() on the host).  Then x + bound is in [0, 2 bound] (0 and 2 bound exactly at the ends, rounding is
// monotone), the multiplication with the power of two 1 / (2 bound) is exact, so u is in [0, 1]; a NaN does not survive the
// clamp's v_med3_f32.  The test cannot fire and is not compiled: no compares, no selects on u, none on the features.
template <bool CLAMPED = false>
__device__ __forceinline__ void encoder_unit(const NetArgs& na, float x, float y, float z, float (&u)[3], bool& oob) {
    u[0] = (x + na.bound) * na.inv_two_bound; u[1] = (y + na.bound) * na.inv_two_bound; u[2] = (z + na.bound) * na.inv_two_bound;
    if constexpr (CLAMPED) {
        oob = false;
    } else {
        oob = (u[0] < 0 || u[0] > 1) || (u[1] < 0 || u[1] > 1) || (u[2] < 0 || u[2] > 1);
        if (oob) { u[0] = 0.5f; u[1] = 0.5f; u[2] = 0.5f; }
    }
}

// position along an axis in cells -> (cell, fraction): gridencoder.cu's floorf(p), (uint32_t), p - (float)cell in two instructions.
// p = fmaf(u, scale, half_off) with u in [0, 1], scale > 0, half_off >= 0, so p >= 0 and finite: truncation IS the floor, and
// p - floor(p) is exact in fp32 (a suffix of p's significand), which is what v_fract_f32 returns (its clamp below one only acts for
// negative inputs).  A NaN gives cell 0 and fraction NaN in both forms.
__device__ __forceinline__ void cell_frac(float p, uint32_t& cell, float& frac) {
    cell = (uint32_t)p;
    frac = __builtin_amdgcn_fractf(p);
}

// the eight corner weights w[idx] = (wx * wy) * wz in the reference's order (gridencoder.cu:150-160; 1 * wx is exact), corner idx
// bit d set = the upper cell boundary along axis d.  PACKED: the same twelve products in the same order, two per v_pk_mul_f32
// (the four wx * wy, then the eight * wz) -- a packing, not a re-association.  Only the render loop's tile (net_density_piped) asks
// for it: there it takes 46 v_mul_f32 out for 23 v_pk_mul_f32 at unchanged registers, while in net_density, the tape and the fp32
// gather the even-aligned register pairs cost occupancy or scratch in some kernels, so they keep the scalar form.
template <bool PACKED>
__device__ __forceinline__ void corner_weights(const float (&fr)[3], float (&w)[8]) {
    if constexpr (!PACKED) {
#pragma unroll
        for (int idx = 0; idx < 8; idx++) {
            const float wx = (idx & 1) ? fr[0] : 1 - fr[0];
            const float wy = (idx & 2) ? fr[1] : 1 - fr[1];
            const float wz = (idx & 4) ? fr[2] : 1 - fr[2];
            w[idx] = (wx * wy) * wz;
        }
        return;
    }
    const f32x2 wx = {1 - fr[0], fr[0]};
    const float wy0 = 1 - fr[1], wy1 = fr[1], wz0 = 1 - fr[2], wz1 = fr[2];
    const f32x2 xy0 = wx * (f32x2){wy0, wy0}, xy1 = wx * (f32x2){wy1, wy1};
    const f32x2 w01 = xy0 * (f32x2){wz0, wz0}, w23 = xy1 * (f32x2){wz0, wz0}, w45 = xy0 * (f32x2){wz1, wz1}, w67 = xy1 * (f32x2){wz1, wz1};
    w[0] = w01[0]; w[1] = w01[1]; w[2] = w23[0]; w[3] = w23[1];
    w[4] = w45[0]; w[5] = w45[1]; w[6] = w67[0]; w[7] = w67[1];
}

// entry e of the compact table (hashed / dense levels; e counts from the table's start, the level's offset included): the table's
// base stays in SGPRs and the lane supplies a 32-bit byte offset (the global_load saddr form), so no 64-bit vector address is formed.
// fill_net() refuses a table of 4 GiB or more.  (The per-cell records are larger than that and keep 64-bit addresses.)
template <typename T>
__device__ __forceinline__ T table_at(const void* table, uint32_t e) {
    return *reinterpret_cast<const T*>(reinterpret_cast<const char*>(table) + (size_t)(e * (uint32_t)sizeof(T)));
}

// fmaf(w, (float)half, acc) with the half taken from the low / high 16 bits of a packed table entry: one v_fma_mix_f32
// (fp32 arithmetic, the conversion is part of the instruction).  hipcc otherwise converts both halves and uses v_pk_fma_f32.
__device__ __forceinline__ float fma_mix_lo(float w, uint32_t packed, float acc) {
    float r;
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel_hi:[0,1,0]" : "=v"(r) : "v"(w), "v"(packed), "v"(acc));
    return r;
}
__device__ __forceinline__ float fma_mix_hi(float w, uint32_t packed, float acc) {
    float r;
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[0,1,0]" : "=v"(r) : "v"(w), "v"(packed), "v"(acc));
    return r;
}

// HALF_ACC (ngp_model::precision == NGP_PREC_F16_REF, `model.fused_reference_rounding`): the grid_encode operator's arithmetic instead --
// every product rounded to fp16, fp16 running sum (c10::Half, gridencoder.cu:169-172): the features are then bit-identical to the
// reference's, at three VALU instructions per corner and feature instead of one.
template <bool HALF_ACC = false, bool PACKED = false>
__device__ __forceinline__ void corners_to_feature(const float (&fr)[3], const uint32_t (&raw)[8], bool oob, _Float16& f0, _Float16& f1) {
    float a0 = 0.0f, a1 = 0.0f;
    half2v hs = {(_Float16)0, (_Float16)0};
    float cw[8];
    corner_weights<PACKED>(fr, cw);
#pragma unroll
    for (int idx = 0; idx < 8; idx++) {
        const float w = cw[idx];
        if (HALF_ACC) {
            // w * (float)entry in fp32 (x + (-0) = x: the fma with a -0 addend IS the fp32 product, signed zeros included; the
            // conversion of the entry is part of the instruction), rounded to half -- two roundings, as c10::Half's operator* gives,
            // not the single one of v_fma_mixlo_f16 -- then the half running sum of both channels in one packed add
            half2v pr = {(_Float16)fma_mix_lo(w, raw[idx], -0.0f), (_Float16)fma_mix_hi(w, raw[idx], -0.0f)};
            hs = hs + pr;
        } else {
            a0 = fma_mix_lo(w, raw[idx], a0);
            a1 = fma_mix_hi(w, raw[idx], a1);
        }
    }
    f0 = oob ? (_Float16)0 : (HALF_ACC ? hs[0] : (_Float16)a0);
    f1 = oob ? (_Float16)0 : (HALF_ACC ? hs[1] : (_Float16)a1);
}

// density half: hash-grid encode + sigma net.  Returns sigma (meaningful in q == 0) and the sigma-net outputs 4q..4q+3 as fp16.
template <int MODE, bool HACC = false, bool CLAMPED = false>
__device__ __forceinline__ void net_density(const NetArgs& na, const _Float16* Wlds, const LevelTab& lt, uint32_t lane, float x, float y, float z,
                                            float& sigma, _Float16 (&s16)[4]) {
    const uint32_t q = lane >> 4;
    // encoder input: (x + bound) / (2 bound)  (gridencoder/grid.py:144).  torch evaluates a division by a Python scalar on
    // the GPU as a multiplication with the fp32 reciprocal; identical to the division whenever 2*bound is a power of two.
    float u[3];
    bool oob;
    encoder_unit<CLAMPED>(na, x, y, z, u, oob);
    const float u0 = u[0], u1 = u[1], u2 = u[2];
    const float half_off = na.align_corners ? 0.0f : 0.5f;

    // ---- 4 levels x 8 corners: issue all 32 gathers, then interpolate (gridencoder.cu:139-175).
    // Index recipe of get_grid_index (:54-72), branch-free: hashed and dense candidates are both formed from the
    // same two products and selected per level; the modulo is an AND (see LevelTab).
    uint32_t raw[4][8];
    float fr[4][3];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t level = q + 4 * i;
        const float scale = lt.scale[level];
        const uint32_t a1 = lt.a1[level], a2 = lt.a2[level], mask = lt.mask[level], fl = lt.flags[level];
        const bool hashed = (fl & 1u) != 0;
        float p[3] = {fmaf(u0, scale, half_off), fmaf(u1, scale, half_off), fmaf(u2, scale, half_off)};
        uint32_t g[3];
#pragma unroll
        for (int d = 0; d < 3; d++) cell_frac(p[d], g[d], fr[i][d]);
        if (MODE == 2 && i < 3) {   // levels 0..11 from the per-cell records (compile-time: no second code path in the other kernels)
            const uint32_t S = lt.cell_res[level];
            const uint32_t ci = lt.cell_off[level] + g[0] + S * (g[1] + S * g[2]);
            const uint4* rec = na.cells + (size_t)ci * 2;
            const uint4 lo = rec[0], hi = rec[1];
            raw[i][0] = lo.x; raw[i][1] = lo.y; raw[i][2] = lo.z; raw[i][3] = lo.w;
            raw[i][4] = hi.x; raw[i][5] = hi.y; raw[i][6] = hi.z; raw[i][7] = hi.w;
            continue;
        }
        const uint32_t off = lt.offset[level];
        const uint32_t t1[2] = {g[1] * a1, g[1] * a1 + a1};
        const uint32_t t2[2] = {g[2] * a2, g[2] * a2 + a2};
#pragma unroll
        for (int idx = 0; idx < 8; idx++) {
            const uint32_t px = g[0] + (idx & 1), ty = t1[(idx >> 1) & 1], tz = t2[(idx >> 2) & 1];
            uint32_t e = hashed ? (px ^ ty ^ tz) : (px + ty + tz);
            e &= mask;
            if (MODE == 1) {
                if (fl & 2u) e %= lt.size[level];
            }
            raw[i][idx] = table_at<uint32_t>(na.table, off + e);
        }
    }
    half8 feat;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        // The fused path accumulates the 8 corners in fp32 (one v_fma_mix_f32 per corner and feature) and rounds the feature
        // to fp16 once; the grid_encode operator keeps the reference's c10::Half accumulation (8 roundings, :169-172) bit for
        // bit.  The difference is below one fp16 ulp of the feature and inside the fused path's documented tolerance.
        if constexpr (HACC) {        // the reference's c10::Half accumulation (NGP_PREC_F16_REF)
            _Float16 f0, f1;
            corners_to_feature<true>(fr[i], raw[i], oob, f0, f1);
            feat[2 * i] = f0; feat[2 * i + 1] = f1;
            continue;
        }
        float a0 = 0.0f, a1 = 0.0f;
        float cw[8];
        corner_weights<false>(fr[i], cw);     // w = ((1 * wx) * wy) * wz in the reference's order (:150-160)
#pragma unroll
        for (int idx = 0; idx < 8; idx++) {
            a0 = fma_mix_lo(cw[idx], raw[i][idx], a0);
            a1 = fma_mix_hi(cw[idx], raw[i][idx], a1);
        }
        feat[2 * i] = oob ? (_Float16)0 : (_Float16)a0;
        feat[2 * i + 1] = oob ? (_Float16)0 : (_Float16)a1;
    }

    // ---- sigma net: 32 -> 64 (-> 64)* -> 16
    const half8* Ws = reinterpret_cast<const half8*>(Wlds);
    half8 h[2];
    mlp_in(Ws, lane, feat, h);
    for (uint32_t k = 0; k < na.sig_mm; k++) mlp_hidden(Ws + 256 + k * 512, lane, h);
    const f32x4 so = mlp_out(Ws + 256 + na.sig_mm * 512, lane, h);
#pragma unroll
    for (int r = 0; r < 4; r++) s16[r] = (_Float16)so[r];
    sigma = expf((float)s16[0]);  // trunc_exp forward (activation.py:8-10), meaningful in q == 0
}

// ---- MODE 2 inside the render loop: the hashed level of a lane (12 + q) is gathered ONE TILE AHEAD --------------------------------
// With the per-cell records the only loads that still miss far are the 8 gathers of the lane's hashed level.  They are issued for
// the NEXT tile's sample while this tile's records are in flight and its MLPs run, and consumed a tile later from registers
// (`pre`).  Order inside a tile: issue this tile's record loads; interpolate the hashed level from `pre` (loaded a tile ago);
// issue the next tile's hashed gathers into the freed registers; then wait for the records only (vector-memory loads return
// in order, so the younger gathers stay in flight behind them).
template <bool CLAMPED = false>
__device__ __forceinline__ void hashed_gather(const NetArgs& na, const LevelTab& lt, uint32_t level, float x, float y, float z, uint32_t (&out)[8]) {
    float u[3];
    bool oob;
    encoder_unit<CLAMPED>(na, x, y, z, u, oob);
    const float half_off = na.align_corners ? 0.0f : 0.5f, scale = lt.scale[level];
    const uint32_t a1 = lt.a1[level], a2 = lt.a2[level], mask = lt.mask[level], off = lt.offset[level];
    // (cells only: p >= 0, so the truncation is the floor, see cell_frac)
    const uint32_t g0 = (uint32_t)fmaf(u[0], scale, half_off), g1 = (uint32_t)fmaf(u[1], scale, half_off), g2 = (uint32_t)fmaf(u[2], scale, half_off);
    const bool hashed = (lt.flags[level] & 1u) != 0;     // (a tiled grid's fine levels are sums wrapped by the mask, not hashes)
    const uint32_t t1[2] = {g1 * a1, g1 * a1 + a1};
    const uint32_t t2[2] = {g2 * a2, g2 * a2 + a2};
#pragma unroll
    for (int idx = 0; idx < 8; idx++) {
        const uint32_t px = g0 + (idx & 1), ty = t1[(idx >> 1) & 1], tz = t2[(idx >> 2) & 1];
        out[idx] = table_at<uint32_t>(na.table, off + ((hashed ? (px ^ ty ^ tz) : (px + ty + tz)) & mask));
    }
}

// same values and arithmetic as net_density<2>; `pre` holds this tile's hashed-level entries on entry and the next tile's on exit
template <bool HACC = false, bool CLAMPED = false>
__device__ __forceinline__ void net_density_piped(const NetArgs& na, const _Float16* Wlds, const LevelTab& lt, uint32_t lane, float x, float y,
                                                  float z, float nx, float ny, float nz, uint32_t (&pre)[8], float& sigma,
                                                  _Float16 (&s16)[4]) {
    const uint32_t q = lane >> 4;
    float u[3];
    bool oob;
    encoder_unit<CLAMPED>(na, x, y, z, u, oob);
    const float half_off = na.align_corners ? 0.0f : 0.5f;
    uint4 rec[3][2];
    float fr[4][3];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t level = q + 4 * i;
        const float scale = lt.scale[level];
        uint32_t g[3];
#pragma unroll
        for (int d = 0; d < 3; d++) cell_frac(fmaf(u[d], scale, half_off), g[d], fr[i][d]);
        if (i < 3) {
            const uint32_t S = lt.cell_res[level];
            const uint4* r = na.cells + (size_t)(lt.cell_off[level] + g[0] + S * (g[1] + S * g[2])) * 2;
            rec[i][0] = r[0];
            rec[i][1] = r[1];
        }
    }
    half8 feat;
    {
        _Float16 f0, f1;
        corners_to_feature<HACC, true>(fr[3], pre, oob, f0, f1);
        feat[6] = f0; feat[7] = f1;
    }
    // (unconditional: a branch here makes the compiler wait for ALL outstanding loads at the join; the last tile re-gathers its own entries)
    hashed_gather<CLAMPED>(na, lt, q + 12, nx, ny, nz, pre);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const uint32_t raw[8] = {rec[i][0].x, rec[i][0].y, rec[i][0].z, rec[i][0].w, rec[i][1].x, rec[i][1].y, rec[i][1].z, rec[i][1].w};
        _Float16 f0, f1;
        corners_to_feature<HACC, true>(fr[i], raw, oob, f0, f1);
        feat[2 * i] = f0; feat[2 * i + 1] = f1;
    }
    const half8* Ws = reinterpret_cast<const half8*>(Wlds);
    half8 h[2];
    mlp_in(Ws, lane, feat, h);
    for (uint32_t k = 0; k < na.sig_mm; k++) mlp_hidden(Ws + 256 + k * 512, lane, h);
    const f32x4 so = mlp_out(Ws + 256 + na.sig_mm * 512, lane, h);
#pragma unroll
    for (int r = 0; r < 4; r++) s16[r] = (_Float16)so[r];
    sigma = expf((float)s16[0]);
}

// The gather of net_density on its own: a lane's four levels (q, q+4, q+8, q+12) -> 32 raw corner entries, the interpolation
// fractions and the out-of-range flag.  (net_density keeps its own copy of these lines: its instruction schedule is tuned.)
template <int MODE, bool CLAMPED = false>
__device__ __forceinline__ void fused_gather(const NetArgs& na, const LevelTab& lt, uint32_t q, float x, float y, float z, uint32_t (&raw)[4][8],
                                             float (&fr)[4][3], bool& oob) {
    float u[3];
    encoder_unit<CLAMPED>(na, x, y, z, u, oob);
    const float half_off = na.align_corners ? 0.0f : 0.5f;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t level = q + 4 * i;
        const float scale = lt.scale[level];
        uint32_t g[3];
#pragma unroll
        for (int d = 0; d < 3; d++) cell_frac(fmaf(u[d], scale, half_off), g[d], fr[i][d]);
        if (MODE == 2 && i < 3) {
            const uint32_t S = lt.cell_res[level];
            const uint4* rec = na.cells + (size_t)(lt.cell_off[level] + g[0] + S * (g[1] + S * g[2])) * 2;
            const uint4 lo = rec[0], hi = rec[1];
            raw[i][0] = lo.x; raw[i][1] = lo.y; raw[i][2] = lo.z; raw[i][3] = lo.w;
            raw[i][4] = hi.x; raw[i][5] = hi.y; raw[i][6] = hi.z; raw[i][7] = hi.w;
            continue;
        }
        const uint32_t off = lt.offset[level];
        const uint32_t a1 = lt.a1[level], a2 = lt.a2[level], mask = lt.mask[level], fl = lt.flags[level];
        const bool hashed = (fl & 1u) != 0;
        const uint32_t t1[2] = {g[1] * a1, g[1] * a1 + a1}, t2[2] = {g[2] * a2, g[2] * a2 + a2};
#pragma unroll
        for (int idx = 0; idx < 8; idx++) {
            const uint32_t px = g[0] + (idx & 1), ty = t1[(idx >> 1) & 1], tz = t2[(idx >> 2) & 1];
            uint32_t e = hashed ? (px ^ ty ^ tz) : (px + ty + tz);
            e &= mask;
            if (MODE == 1) { if (fl & 2u) e %= lt.size[level]; }
            raw[i][idx] = table_at<uint32_t>(na.table, off + e);
        }
    }
}

// colour half: SH degree 4 + geo_feat -> colour net -> fp16 sigmoid (results in q == 0)
__device__ __forceinline__ void net_color(const NetArgs& na, const _Float16* Wlds, uint32_t lane, float dx, float dy, float dz,
                                          const _Float16 (&s16)[4], float& cr, float& cg, float& cb) {
    const uint32_t q = lane >> 4;
    half8 h[2];
    // ---- colour net input: [SH(16) | geo_feat(15) | 0] in the permuted k order of perm_color
    float sh[4];
    sh4_quarter(q, dx, dy, dz, sh);
    half8 cin;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        cin[r] = (_Float16)sh[r];
        cin[4 + r] = s16[r];
    }
    if (q == 0) cin[4] = (_Float16)0;  // lane 0's accumulator row 0 is sigma, not a feature: this slot carries the zero pad
    const half8* Wc = reinterpret_cast<const half8*>(Wlds + sig_halfs(na.sig_mm));
    mlp_in(Wc, lane, cin, h);
    for (uint32_t k = 0; k < na.col_mm; k++) mlp_hidden(Wc + 256 + k * 512, lane, h);
    const f32x4 co = mlp_out(Wc + 256 + na.col_mm * 512, lane, h);
    // torch.sigmoid on a half tensor: evaluate in fp32, round to fp16
    cr = (float)(_Float16)(1.0f / (1.0f + expf(-(float)(_Float16)co[0])));
    cg = (float)(_Float16)(1.0f / (1.0f + expf(-(float)(_Float16)co[1])));
    cb = (float)(_Float16)(1.0f / (1.0f + expf(-(float)(_Float16)co[2])));
}

template <int MODE>
__device__ __forceinline__ void net_tile(const NetArgs& na, const _Float16* Wlds, const LevelTab& lt, uint32_t lane, float x, float y, float z,
                                         float dx, float dy, float dz, float& sigma, float& cr, float& cg, float& cb) {
    _Float16 s16[4];
    net_density<MODE>(na, Wlds, lt, lane, x, y, z, sigma, s16);
    net_color(na, Wlds, lane, dx, dy, dz, s16, cr, cg, cb);
}

// ---- fp16 backward: what k_pack_weights_bwd (fused_net.hip) writes, then the layers, the ReLU mask and the SH derivative
// Transposed fragments.  Per net: [out layer: ob 4][lane][8] | [hidden layers, LAST first: ob 4][s 2][lane][8] | [in layer: ob 2][s 2][lane][8]
//   out layer   : A[row = unit 16 ob + c][k(q, j)] = j < 4 ? W_out[4q + j][unit] : 0      (B fragment = the lane's own 4 output gradients)
//   hidden layer: A[row = unit 16 ob + c of the layer BELOW][k = perm_hidden(q, j, s)] = W[perm_hidden(q, j, s)][that unit]
//   in layer    : accumulator row 4 q' + r of block ob is the gradient of input feature phi(q', 4 ob + r), phi = perm_grid / perm_color:
//                 A[row i][k = perm_hidden(q, j, s)] = W_in[perm_hidden(q, j, s)][phi(i >> 2, 4 ob + (i & 3))]
__host__ __device__ inline uint32_t bwd_halfs(uint32_t mm) { return 2048 + mm * 4096 + 2048; }

__device__ __forceinline__ void mlp_out_bwd(const half8* Wt, uint32_t lane, half8 g, f32x4 (&acc)[4]) {
#pragma unroll
    for (int ob = 0; ob < 4; ob++) acc[ob] = __builtin_amdgcn_mfma_f32_16x16x32_f16(Wt[ob * 64 + lane], g, (f32x4){0, 0, 0, 0}, 0, 0, 0);
}
__device__ __forceinline__ void mlp_hidden_bwd(const half8* Wt, uint32_t lane, const half8 (&g)[2], f32x4 (&acc)[4]) {
#pragma unroll
    for (int ob = 0; ob < 4; ob++) {
        acc[ob] = __builtin_amdgcn_mfma_f32_16x16x32_f16(Wt[(ob * 2 + 0) * 64 + lane], g[0], (f32x4){0, 0, 0, 0}, 0, 0, 0);
        acc[ob] = __builtin_amdgcn_mfma_f32_16x16x32_f16(Wt[(ob * 2 + 1) * 64 + lane], g[1], acc[ob], 0, 0, 0);
    }
}
__device__ __forceinline__ void mlp_in_bwd(const half8* Wt, uint32_t lane, const half8 (&g)[2], f32x4 (&acc)[2]) {
#pragma unroll
    for (int ob = 0; ob < 2; ob++) {
        acc[ob] = __builtin_amdgcn_mfma_f32_16x16x32_f16(Wt[(ob * 2 + 0) * 64 + lane], g[0], (f32x4){0, 0, 0, 0}, 0, 0, 0);
        acc[ob] = __builtin_amdgcn_mfma_f32_16x16x32_f16(Wt[(ob * 2 + 1) * 64 + lane], g[1], acc[ob], 0, 0, 0);
    }
}
// gradient through ReLU at the layer whose (post-activation) forward values are h: pass where h > 0; fp16 like the operator's buffers
__device__ __forceinline__ void relu_mask_pack(const f32x4 (&acc)[4], const half8 (&h)[2], half8 (&g)[2]) {
#pragma unroll
    for (int st = 0; st < 2; st++)
#pragma unroll
        for (int jj = 0; jj < 8; jj++) {
            const _Float16 v = (_Float16)acc[2 * st + (jj >> 2)][jj & 3];
            g[st][jj] = h[st][jj] > (_Float16)0 ? v : (_Float16)0;
        }
}

// d SH_k / d (x, y, z) for k = 4q .. 4q + 3 contracted with g[4] (the closed forms of sh4_quarter differentiated)
__device__ __forceinline__ void sh4_quarter_vjp(uint32_t q, float x, float y, float z, const float (&g)[4], float (&o)[3]) {
    const float a = 0.48860251190291987f, b = 1.0925484305920792f, c2 = 2.0f * 0.94617469575755997f, e = 0.54627421529603959f,
                f = 0.59004358992664352f, gg = 2.8906114426405538f, h = 0.45704579946446572f, k = 0.3731763325901154f, m = 1.4453057213202769f;
    const float x2 = x * x, y2 = y * y, z2 = z * z;
    if (q == 0) {
        o[0] = -a * g[3]; o[1] = -a * g[1]; o[2] = a * g[2];
    } else if (q == 1) {
        o[0] = b * y * g[0] - b * z * g[3];
        o[1] = b * x * g[0] - b * z * g[1];
        o[2] = -b * y * g[1] + c2 * z * g[2] - b * x * g[3];
    } else if (q == 2) {
        o[0] = 2 * e * x * g[0] - 6 * f * x * y * g[1] + gg * y * z * g[2];
        o[1] = -2 * e * y * g[0] + f * (-3 * x2 + 3 * y2) * g[1] + gg * x * z * g[2] + h * (1 - 5 * z2) * g[3];
        o[2] = gg * x * y * g[2] - 10 * h * y * z * g[3];
    } else {
        o[0] = h * (1 - 5 * z2) * g[1] + 2 * m * x * z * g[2] + f * (-3 * x2 + 3 * y2) * g[3];
        o[1] = -2 * m * y * z * g[2] + 6 * f * x * y * g[3];
        o[2] = k * (15 * z2 - 3) * g[0] - 10 * h * x * z * g[1] + m * (x2 - y2) * g[2];
    }
}

// ==========================================================================================
// The same network in fp32 (ngp_model::precision == NGP_PREC_F32): what validate.py's rollout evaluates.  Its render_fn is a bare
// model.render(...) (validate.py:288-291) -- no autocast context is ever entered on that path (the only ones are inside Trainer
// methods, nerf/utils.py:544-864) -- so the table is read as fp32 (gridencoder/grid.py:36-39 casts only under autocast) and the
// nn.Linear layers of nerf/network.py:33-47 run as fp32 GEMMs.
//
// Same lane mapping as the fp16 form: lane = (sample c, quarter q), a lane gathers levels q, q+4, q+8, q+12 as 8-byte (float2)
// entries and interpolates them with the operator's arithmetic (fmaf(w, entry, acc) over the corners in index order,
// gridencoder.cu:139-175: the features are bit-identical to grid_encode's fp32 output).  The MLPs run on v_mfma_f32_16x16x4_f32
// (f32 in, f32 accumulate: bit for bit a k-ordered fmaf chain, at the fp32 vector rate): H^T = W X^T again, so an accumulator
// (units 16 ob + 4 q + r of sample c) is directly the B operand of the next layer's k-steps -- step (ob, r) takes register r of
// block ob from every lane, i.e. k = q <-> unit 16 ob + 4 q + r -- and the A fragments are stored in that order:
//   in layer  [ob 4][g 2][lane][4]: W_in[16 ob + c][phi(q, 4 g + r)],  phi = perm_grid / perm_color (the lane's own 8 inputs)
//   hidden    [ob 4][g 4][lane][4]: W[16 ob + c][16 g + 4 q + r]
//   out layer        [g 4][lane][4]: W_out[c][16 g + 4 q + r]
// one ds_read_b128 per lane and four MFMAs.  The summation order over k is therefore a permutation of the natural one (fp32
// round-off level, like any GEMM library's).  Source blobs: the FFMLP layout in fp32.
// ==========================================================================================
__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ void relu4(f32x4 (&h)[4]) {
#pragma unroll
    for (int ob = 0; ob < 4; ob++)
#pragma unroll
        for (int r = 0; r < 4; r++) h[ob][r] = h[ob][r] > 0.0f ? h[ob][r] : 0.0f;
}
__device__ __forceinline__ void mlp32_in(const f32x4* W, uint32_t lane, const float (&x)[8], f32x4 (&h)[4]) {
#pragma unroll
    for (int ob = 0; ob < 4; ob++) h[ob] = (f32x4){0, 0, 0, 0};
#pragma unroll
    for (int g = 0; g < 2; g++) {
        f32x4 a[4];
#pragma unroll
        for (int ob = 0; ob < 4; ob++) a[ob] = W[(ob * 2 + g) * 64 + lane];
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int ob = 0; ob < 4; ob++) h[ob] = mfma4(a[ob][r], x[4 * g + r], h[ob]);
    }
    relu4(h);
}
__device__ __forceinline__ void mlp32_hidden_raw(const f32x4* W, uint32_t lane, const f32x4 (&h)[4], f32x4 (&acc)[4]) {
#pragma unroll
    for (int ob = 0; ob < 4; ob++) acc[ob] = (f32x4){0, 0, 0, 0};
#pragma unroll
    for (int g = 0; g < 4; g++) {
        f32x4 a[4];
#pragma unroll
        for (int ob = 0; ob < 4; ob++) a[ob] = W[(ob * 4 + g) * 64 + lane];
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int ob = 0; ob < 4; ob++) acc[ob] = mfma4(a[ob][r], h[g][r], acc[ob]);
    }
}
__device__ __forceinline__ void mlp32_hidden(const f32x4* W, uint32_t lane, f32x4 (&h)[4]) {
    f32x4 acc[4];
    mlp32_hidden_raw(W, lane, h, acc);
#pragma unroll
    for (int ob = 0; ob < 4; ob++) h[ob] = acc[ob];
    relu4(h);
}
__device__ __forceinline__ f32x4 mlp32_out(const f32x4* W, uint32_t lane, const f32x4 (&h)[4]) {
    f32x4 o = {0, 0, 0, 0};
#pragma unroll
    for (int g = 0; g < 4; g++) {
        const f32x4 a = W[g * 64 + lane];
#pragma unroll
        for (int r = 0; r < 4; r++) o = mfma4(a[r], h[g][r], o);
    }
    return o;
}

// a lane's four levels from the fp32 table: 32 eight-byte corner entries, the interpolation fractions, the out-of-range flag
template <int MODE, bool CLAMPED = false>
__device__ __forceinline__ void fused_gather32(const NetArgs& na, const LevelTab& lt, uint32_t q, float x, float y, float z, float2 (&raw)[4][8],
                                               float (&fr)[4][3], bool& oob) {
    float u[3];
    encoder_unit<CLAMPED>(na, x, y, z, u, oob);
    const float half_off = na.align_corners ? 0.0f : 0.5f;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t level = q + 4 * i;
        const float scale = lt.scale[level];
        uint32_t g[3];
#pragma unroll
        for (int d = 0; d < 3; d++) cell_frac(fmaf(u[d], scale, half_off), g[d], fr[i][d]);
        const uint32_t off = lt.offset[level];
        const uint32_t a1 = lt.a1[level], a2 = lt.a2[level], mask = lt.mask[level], fl = lt.flags[level];
        const bool hashed = (fl & 1u) != 0;
        const uint32_t t1[2] = {g[1] * a1, g[1] * a1 + a1}, t2[2] = {g[2] * a2, g[2] * a2 + a2};
#pragma unroll
        for (int idx = 0; idx < 8; idx++) {
            const uint32_t px = g[0] + (idx & 1), ty = t1[(idx >> 1) & 1], tz = t2[(idx >> 2) & 1];
            uint32_t e = hashed ? (px ^ ty ^ tz) : (px + ty + tz);
            e &= mask;
            if (MODE == 1) { if (fl & 2u) e %= lt.size[level]; }
            raw[i][idx] = table_at<float2>(na.table, off + e);
        }
    }
}
// gridencoder.cu:139-175 in fp32: results[ch] += w * grid[index + ch] over the corners in index order (one fma each under nvcc's
// -fmad; the operator and the oracle write it as fmaf) -- bit-identical to grid_encode's fp32 features
__device__ __forceinline__ void corners_to_feature32(const float (&fr)[3], const float2 (&raw)[8], bool oob, float& f0, float& f1) {
    f32x2 acc = {0.0f, 0.0f};                           // both features of a corner in one v_pk_fma_f32 (an IEEE fma per component)
    float cw[8];
    corner_weights<false>(fr, cw);
#pragma unroll
    for (int idx = 0; idx < 8; idx++) {
        const float w = cw[idx];
        acc = __builtin_elementwise_fma((f32x2){w, w}, (f32x2){raw[idx].x, raw[idx].y}, acc);
    }
    const float a0 = acc[0], a1 = acc[1];
    f0 = oob ? 0.0f : a0;
    f1 = oob ? 0.0f : a1;
}
// d feature / d u_gd of one level (gridencoder.cu:177-222) contracted with the feature gradients (g0, g1): += into gx[3]
__device__ __forceinline__ void level_input_grad32(float scale, const float (&fr)[3], const float2 (&raw)[8], float g0, float g1, float (&gx)[3]) {
#pragma unroll
    for (int gd = 0; gd < 3; gd++) {
        float d0 = 0.0f, d1 = 0.0f;
#pragma unroll
        for (int k4 = 0; k4 < 4; k4++) {
            float w = scale;
            int left = 0;
#pragma unroll
            for (int nd = 0; nd < 2; nd++) {
                const int d = (nd >= gd) ? (nd + 1) : nd;
                const int bit = (k4 >> nd) & 1;
                w *= bit ? fr[d] : 1 - fr[d];
                left |= bit << d;
            }
            const int right = left | (1 << gd);
            d0 = fmaf(w, raw[right].x - raw[left].x, d0);
            d1 = fmaf(w, raw[right].y - raw[left].y, d1);
        }
        gx[gd] = fmaf(g0, d0, fmaf(g1, d1, gx[gd]));
    }
}

// backward fragments, fp32.  Per net: [out layer: ob 4][lane][4] | [hidden layers, LAST first: ob 4][g 4][lane][4] | [in layer: ob 2][g 4][lane][4]
//   out layer   : A[row = unit 16 ob + c][k = q] of step r = W_out[4 q + r][unit]            (B operand = the lane's output gradient r)
//   hidden layer: A[row = unit 16 ob + c of the layer BELOW][k = q] of step (g, r) = W[16 g + 4 q + r][that unit]
//   in layer    : accumulator (ob, r) of lane (c, q') = gradient of the lane's own input 4 ob + r, i.e. of feature phi(q', 4 ob + r):
//                 A[row i][k = q] of step (g, r) = W_in[16 g + 4 q + r][phi(i >> 2, 4 ob + (i & 3))]
__host__ __device__ inline uint32_t bwd_floats(uint32_t mm) { return 1024 + mm * 4096 + 2048; }
__device__ __forceinline__ void mlp32_out_bwd(const f32x4* Wt, uint32_t lane, const f32x4& g, f32x4 (&acc)[4]) {
#pragma unroll
    for (int ob = 0; ob < 4; ob++) {
        const f32x4 a = Wt[ob * 64 + lane];
        acc[ob] = (f32x4){0, 0, 0, 0};
#pragma unroll
        for (int r = 0; r < 4; r++) acc[ob] = mfma4(a[r], g[r], acc[ob]);
    }
}
__device__ __forceinline__ void mlp32_in_bwd(const f32x4* Wt, uint32_t lane, const f32x4 (&g)[4], f32x4 (&acc)[2]) {
#pragma unroll
    for (int ob = 0; ob < 2; ob++) acc[ob] = (f32x4){0, 0, 0, 0};
#pragma unroll
    for (int gg = 0; gg < 4; gg++)
#pragma unroll
        for (int ob = 0; ob < 2; ob++) {
            const f32x4 a = Wt[(ob * 4 + gg) * 64 + lane];
#pragma unroll
            for (int r = 0; r < 4; r++) acc[ob] = mfma4(a[r], g[gg][r], acc[ob]);
        }
}
// gradient through ReLU at the layer whose post-activation forward values are h
__device__ __forceinline__ void relu_mask32(const f32x4 (&acc)[4], const f32x4 (&h)[4], f32x4 (&g)[4]) {
#pragma unroll
    for (int ob = 0; ob < 4; ob++)
#pragma unroll
        for (int r = 0; r < 4; r++) g[ob][r] = h[ob][r] > 0.0f ? acc[ob][r] : 0.0f;
}

// stage packed weights + level table into LDS (all threads of the block)
// (w_bytes: the caller's net_w_bytes(na), or the fp16 constant expression in the kernels that only exist for fp16)
__device__ __forceinline__ void stage_block(const NetArgs& na, const GridLevels& lv, void* Wlds, LevelTab* lt, size_t w_bytes) {
    const uint32_t n16 = (uint32_t)(w_bytes / 16);  // 16-byte chunks
    const uint4* src = reinterpret_cast<const uint4*>(na.packed);
    uint4* dst = reinterpret_cast<uint4*>(Wlds);
    for (uint32_t i = threadIdx.x; i < n16; i += blockDim.x) dst[i] = src[i];
    if (threadIdx.x < 16) {
        const uint32_t l = threadIdx.x;
        const uint32_t size = lv.offset[l + 1] - lv.offset[l];
        lt->scale[l] = lv.scale[l];
        lt->offset[l] = lv.offset[l];
        lt->size[l] = size;
        lt->a1[l] = lv.hashed[l] ? 2654435761u : lv.mul1[l];
        lt->a2[l] = lv.hashed[l] ? 805459861u : lv.mul2[l];
        lt->mask[l] = lv.mode[l] == 1 ? size - 1 : 0xFFFFFFFFu;
        lt->flags[l] = (uint32_t)lv.hashed[l] | (lv.mode[l] == 2 ? 2u : 0u);
        lt->cell_off[l] = na.cell_off[l];
        lt->cell_res[l] = lv.resolution[l];
    }
    __syncthreads();
}

// ------------------------------------------------------------------------------------------
// Network policies: what a fused kernel needs of the network, for the two precisions.  `W` is the LDS image of the packed forward
// weights (sigma net, then colour net), `Wb` that of the transposed ones (backward kernels only).
//   density      hash grid + sigma net of the lane's sample -> sigma (trunc_exp output, meaningful in q == 0) and the sigma net's
//                outputs 4q..4q+3 (`geo_t`: fp16 / fp32)
//   color        SH + colour net -> rgb in q == 0
//   density_tape the same forward keeping what its backward needs;  density_vjp: dL/d(sigma-net outputs) -> this lane's part of
//                dL/d(encoder input in [0,1]) (the sample's is the sum over its four lanes)
//   color_vjp    colour net forward + backward for one tile: dL/d rgb = G * wsc * sigmoid' -> this lane's part of dL/d dir (through
//                SH) and dL/d(sigma-net outputs) (through the geometry features)
// ------------------------------------------------------------------------------------------
template <int MODE_, bool HACC_ = false, bool CLAMPED_ = false>
struct NetF16 {
    static constexpr int MODE = MODE_;
    static constexpr bool HACC = HACC_;        // the reference's c10::Half corner accumulation (NGP_PREC_F16_REF)
    static constexpr bool CLAMPED = CLAMPED_;  // `density` only: its callers clamp the position and the host found clamped_exact() (see encoder_unit)
    static constexpr bool kF32 = false;
    typedef _Float16 geo_t;
    static __host__ __device__ size_t w_bytes(const NetArgs& na) { return net_w_bytes_f16(na); }
    static __device__ __forceinline__ void density(const NetArgs& na, const char* W, const LevelTab& lt, uint32_t lane, float x, float y, float z,
                                                   float& sigma, geo_t (&s)[4]) {
        net_density<MODE, HACC, CLAMPED>(na, reinterpret_cast<const _Float16*>(W), lt, lane, x, y, z, sigma, s);
    }
    static __device__ __forceinline__ void color(const NetArgs& na, const char* W, uint32_t lane, float dx, float dy, float dz, const geo_t (&s)[4],
                                                 float& cr, float& cg, float& cb) {
        net_color(na, reinterpret_cast<const _Float16*>(W), lane, dx, dy, dz, s, cr, cg, cb);
    }
    static __host__ __device__ size_t wb_bytes(const NetArgs& na) { return (size_t)(bwd_halfs(na.sig_mm) + bwd_halfs(na.col_mm)) * 2; }

    struct Tape {
        bool oob;
        uint32_t raw[4][8];
        float fr[4][3], scl[4];
        half8 hs[3][2], hs_last[2];        // sigma net: post-activations of the input layer and of each hidden layer
    };
    static __device__ __forceinline__ void density_tape(const NetArgs& na, const char* W, const LevelTab& lt, uint32_t lane, float x, float y,
                                                        float z, Tape& t, geo_t (&s)[4]) {
        const uint32_t q = lane >> 4;
        const half8* Ws = reinterpret_cast<const half8*>(W);
        fused_gather<MODE>(na, lt, q, x, y, z, t.raw, t.fr, t.oob);
#pragma unroll
        for (int i = 0; i < 4; i++) t.scl[i] = lt.scale[q + 4 * i];
        half8 feat;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            _Float16 f0, f1;
            corners_to_feature<HACC>(t.fr[i], t.raw[i], t.oob, f0, f1);
            feat[2 * i] = f0; feat[2 * i + 1] = f1;
        }
        mlp_in(Ws, lane, feat, t.hs[0]);                   // (indices stay compile-time constants: register arrays)
        t.hs_last[0] = t.hs[0][0]; t.hs_last[1] = t.hs[0][1];
#pragma unroll
        for (int k = 0; k < 2; k++)
            if ((uint32_t)k < na.sig_mm) {
                mlp_hidden(Ws + 256 + k * 512, lane, t.hs_last);
                t.hs[k + 1][0] = t.hs_last[0]; t.hs[k + 1][1] = t.hs_last[1];
            }
        const f32x4 so = mlp_out(Ws + 256 + na.sig_mm * 512, lane, t.hs_last);
#pragma unroll
        for (int r = 0; r < 4; r++) s[r] = (_Float16)so[r];
    }
    static __device__ __forceinline__ void density_vjp(const NetArgs& na, const char* Wb, uint32_t lane, const Tape& t, const f32x4& gso,
                                                       float (&gx)[3]) {
        const half8* Bs = reinterpret_cast<const half8*>(Wb);
        half8 gs_out = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int r = 0; r < 4; r++) gs_out[r] = (_Float16)gso[r];
        f32x4 acc[4];
        half8 gsn[2];
        mlp_out_bwd(Bs, lane, gs_out, acc);
        relu_mask_pack(acc, t.hs_last, gsn);
#pragma unroll
        for (int l = 1; l >= 0; l--)
            if ((uint32_t)l < na.sig_mm) {
                mlp_hidden_bwd(Bs + 256 + (na.sig_mm - 1 - l) * 512, lane, gsn, acc);
                relu_mask_pack(acc, t.hs[l], gsn);
            }
        f32x4 gfe[2];
        mlp_in_bwd(Bs + 256 + na.sig_mm * 512, lane, gsn, gfe);
        // accumulator (ob, r) = gradient of feature perm_grid(q, 4 ob + r) = level q + 4 (2 ob + (r >> 1)), channel r & 1
        gx[0] = 0; gx[1] = 0; gx[2] = 0;
        if (!t.oob) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const float g0 = (float)(_Float16)gfe[i >> 1][2 * (i & 1)], g1 = (float)(_Float16)gfe[i >> 1][2 * (i & 1) + 1];
#pragma unroll
                for (int gd = 0; gd < 3; gd++) {              // gridencoder.cu:177-222: d feature / d u_gd = scale * sum_4 w (right - left)
                    float d0 = 0.0f, d1 = 0.0f;
#pragma unroll
                    for (int k4 = 0; k4 < 4; k4++) {
                        float w = t.scl[i];
                        int left = 0;
#pragma unroll
                        for (int nd = 0; nd < 2; nd++) {
                            const int d = (nd >= gd) ? (nd + 1) : nd;
                            const int bit = (k4 >> nd) & 1;
                            w *= bit ? t.fr[i][d] : 1 - t.fr[i][d];
                            left |= bit << d;
                        }
                        const int right = left | (1 << gd);
                        const uint32_t rl = t.raw[i][left], rr = t.raw[i][right];
                        d0 = fmaf(w, (float)__builtin_bit_cast(_Float16, (uint16_t)(rr & 0xffffu)) - (float)__builtin_bit_cast(_Float16, (uint16_t)(rl & 0xffffu)), d0);
                        d1 = fmaf(w, (float)__builtin_bit_cast(_Float16, (uint16_t)(rr >> 16)) - (float)__builtin_bit_cast(_Float16, (uint16_t)(rl >> 16)), d1);
                    }
                    gx[gd] = fmaf(g0, d0, fmaf(g1, d1, gx[gd]));
                }
            }
        }
    }
    static __device__ __forceinline__ void color_vjp(const NetArgs& na, const char* W, const char* Wb, uint32_t lane, float dx, float dy, float dz,
                                                     const geo_t (&s)[4], float wsc, const float (&G)[3], float (&gdir)[3], f32x4& gso) {
        const uint32_t q = lane >> 4;
        const half8* Wc = reinterpret_cast<const half8*>(reinterpret_cast<const _Float16*>(W) + sig_halfs(na.sig_mm));
        const half8* Bc = reinterpret_cast<const half8*>(reinterpret_cast<const _Float16*>(Wb) + bwd_halfs(na.sig_mm));
        // ---- colour net forward with kept activations
        float sh[4];
        sh4_quarter(q, dx, dy, dz, sh);
        half8 cin;
#pragma unroll
        for (int r = 0; r < 4; r++) { cin[r] = (_Float16)sh[r]; cin[4 + r] = s[r]; }
        if (q == 0) cin[4] = (_Float16)0;
        half8 hc[4][2], hc_last[2];
        mlp_in(Wc, lane, cin, hc[0]);
        hc_last[0] = hc[0][0]; hc_last[1] = hc[0][1];
#pragma unroll
        for (int k = 0; k < 3; k++)
            if ((uint32_t)k < na.col_mm) {
                mlp_hidden(Wc + 256 + k * 512, lane, hc_last);
                hc[k + 1][0] = hc_last[0]; hc[k + 1][1] = hc_last[1];
            }
        const f32x4 co = mlp_out(Wc + 256 + na.col_mm * 512, lane, hc_last);
        // ---- backward: sigmoid (on the fp16-rounded value, as torch.sigmoid's backward does), out layer, hidden, in
        half8 gco = {0, 0, 0, 0, 0, 0, 0, 0};
        if (q == 0) {
#pragma unroll
            for (int k3 = 0; k3 < 3; k3++) {
                const float yv = (float)(_Float16)(1.0f / (1.0f + expf(-(float)(_Float16)co[k3])));
                gco[k3] = (_Float16)(G[k3] * wsc * (yv * (1.0f - yv)));
            }
        }
        f32x4 acc[4];
        half8 gc[2];
        mlp_out_bwd(Bc, lane, gco, acc);
        relu_mask_pack(acc, hc_last, gc);
#pragma unroll
        for (int l = 2; l >= 0; l--)                        // through hidden matmul l (input activations hc[l]), last first
            if ((uint32_t)l < na.col_mm) {
                mlp_hidden_bwd(Bc + 256 + (na.col_mm - 1 - l) * 512, lane, gc, acc);
                relu_mask_pack(acc, hc[l], gc);
            }
        f32x4 gin[2];
        mlp_in_bwd(Bc + 256 + na.col_mm * 512, lane, gc, gin);
        // accumulator (ob, r) = gradient of colour input perm_color(q, 4 ob + r): ob 0 -> SH 4q + r, ob 1 -> sigma-net output 4q + r
        const float gsh[4] = {(float)(_Float16)gin[0][0], (float)(_Float16)gin[0][1], (float)(_Float16)gin[0][2], (float)(_Float16)gin[0][3]};
        sh4_quarter_vjp(q, dx, dy, dz, gsh, gdir);
#pragma unroll
        for (int r = 0; r < 4; r++) gso[r] = (float)(_Float16)gin[1][r];
        if (q == 0) gso[0] = 0.0f;                          // that slot was the zero pad, not sigma
    }
};

template <int MODE_, bool CLAMPED_ = false>
struct NetF32 {
    static constexpr int MODE = MODE_;
    static constexpr bool CLAMPED = CLAMPED_;  // `density` only, as in NetF16
    static constexpr bool kF32 = true;
    typedef float geo_t;
    static __host__ __device__ size_t w_bytes(const NetArgs& na) { return 2 * net_w_bytes_f16(na); }
    template <bool CL = false>
    static __device__ __forceinline__ void features(const NetArgs& na, const LevelTab& lt, uint32_t q, float x, float y, float z, float (&feat)[8]) {
        float2 raw[4][8];
        float fr[4][3];
        bool oob;
        fused_gather32<MODE, CL>(na, lt, q, x, y, z, raw, fr, oob);
#pragma unroll
        for (int i = 0; i < 4; i++) corners_to_feature32(fr[i], raw[i], oob, feat[2 * i], feat[2 * i + 1]);
    }
    static __device__ __forceinline__ void density(const NetArgs& na, const char* W, const LevelTab& lt, uint32_t lane, float x, float y, float z,
                                                   float& sigma, geo_t (&s)[4]) {
        const f32x4* Ws = reinterpret_cast<const f32x4*>(W);
        float feat[8];
        features<CLAMPED>(na, lt, lane >> 4, x, y, z, feat);
        f32x4 h[4];
        mlp32_in(Ws, lane, feat, h);
        for (uint32_t k = 0; k < na.sig_mm; k++) mlp32_hidden(Ws + 512 + k * 1024, lane, h);
        const f32x4 so = mlp32_out(Ws + 512 + na.sig_mm * 1024, lane, h);
#pragma unroll
        for (int r = 0; r < 4; r++) s[r] = so[r];
        sigma = expf(so[0]);              // trunc_exp forward (activation.py:8-10), meaningful in q == 0
    }
    static __device__ __forceinline__ void color_input(uint32_t q, float dx, float dy, float dz, const geo_t (&s)[4], float (&cin)[8]) {
        float sh[4];
        sh4_quarter(q, dx, dy, dz, sh);
#pragma unroll
        for (int r = 0; r < 4; r++) { cin[r] = sh[r]; cin[4 + r] = s[r]; }
        if (q == 0) cin[4] = 0.0f;        // lane 0's accumulator row 0 is sigma, not a feature: this slot meets the zero-padded weight column
    }
    static __device__ __forceinline__ void color(const NetArgs& na, const char* W, uint32_t lane, float dx, float dy, float dz, const geo_t (&s)[4],
                                                 float& cr, float& cg, float& cb) {
        const f32x4* Wc = reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(W) + sig_halfs(na.sig_mm));
        float cin[8];
        color_input(lane >> 4, dx, dy, dz, s, cin);
        f32x4 h[4];
        mlp32_in(Wc, lane, cin, h);
        for (uint32_t k = 0; k < na.col_mm; k++) mlp32_hidden(Wc + 512 + k * 1024, lane, h);
        const f32x4 co = mlp32_out(Wc + 512 + na.col_mm * 1024, lane, h);
        cr = 1.0f / (1.0f + expf(-co[0]));                 // torch.sigmoid (nerf/network.py:122)
        cg = 1.0f / (1.0f + expf(-co[1]));
        cb = 1.0f / (1.0f + expf(-co[2]));
    }
    static __host__ __device__ size_t wb_bytes(const NetArgs& na) { return (size_t)(bwd_floats(na.sig_mm) + bwd_floats(na.col_mm)) * 4; }

    // backward kernels: at most 1 hidden matmul in the sigma net and 2 in the colour net (nerf/network.py has 0 and 1)
    static constexpr uint32_t kMaxSigMM = 1, kMaxColMM = 2;
    struct Tape {
        bool oob;
        float2 raw[4][8];
        float fr[4][3], scl[4];
        f32x4 hs[2][4], hs_last[4];
    };
    static __device__ __forceinline__ void density_tape(const NetArgs& na, const char* W, const LevelTab& lt, uint32_t lane, float x, float y,
                                                        float z, Tape& t, geo_t (&s)[4]) {
        const uint32_t q = lane >> 4;
        const f32x4* Ws = reinterpret_cast<const f32x4*>(W);
        fused_gather32<MODE>(na, lt, q, x, y, z, t.raw, t.fr, t.oob);
        float feat[8];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            t.scl[i] = lt.scale[q + 4 * i];
            corners_to_feature32(t.fr[i], t.raw[i], t.oob, feat[2 * i], feat[2 * i + 1]);
        }
        mlp32_in(Ws, lane, feat, t.hs[0]);
#pragma unroll
        for (int ob = 0; ob < 4; ob++) t.hs_last[ob] = t.hs[0][ob];
        if (na.sig_mm > 0) {
            mlp32_hidden(Ws + 512, lane, t.hs_last);
#pragma unroll
            for (int ob = 0; ob < 4; ob++) t.hs[1][ob] = t.hs_last[ob];
        }
        const f32x4 so = mlp32_out(Ws + 512 + na.sig_mm * 1024, lane, t.hs_last);
#pragma unroll
        for (int r = 0; r < 4; r++) s[r] = so[r];
    }
    static __device__ __forceinline__ void density_vjp(const NetArgs& na, const char* Wb, uint32_t lane, const Tape& t, const f32x4& gso,
                                                       float (&gx)[3]) {
        const f32x4* Bs = reinterpret_cast<const f32x4*>(Wb);
        f32x4 acc[4], g[4];
        mlp32_out_bwd(Bs, lane, gso, acc);
        relu_mask32(acc, t.hs_last, g);
        if (na.sig_mm > 0) {
            mlp32_hidden_raw(Bs + 256, lane, g, acc);      // (the transposed fragments have the forward layout: rows = units of the layer below)
            relu_mask32(acc, t.hs[0], g);
        }
        f32x4 gfe[2];
        mlp32_in_bwd(Bs + 256 + na.sig_mm * 1024, lane, g, gfe);
        gx[0] = 0; gx[1] = 0; gx[2] = 0;
        if (!t.oob) {
#pragma unroll
            for (int i = 0; i < 4; i++) level_input_grad32(t.scl[i], t.fr[i], t.raw[i], gfe[i >> 1][2 * (i & 1)], gfe[i >> 1][2 * (i & 1) + 1], gx);
        }
    }
    static __device__ __forceinline__ void color_vjp(const NetArgs& na, const char* W, const char* Wb, uint32_t lane, float dx, float dy, float dz,
                                                     const geo_t (&s)[4], float wsc, const float (&G)[3], float (&gdir)[3], f32x4& gso) {
        const uint32_t q = lane >> 4;
        const f32x4* Wc = reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(W) + sig_halfs(na.sig_mm));
        const f32x4* Bc = reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(Wb) + bwd_floats(na.sig_mm));
        float cin[8];
        color_input(q, dx, dy, dz, s, cin);
        f32x4 hc[3][4], hc_last[4];
        mlp32_in(Wc, lane, cin, hc[0]);
#pragma unroll
        for (int ob = 0; ob < 4; ob++) hc_last[ob] = hc[0][ob];
#pragma unroll
        for (int k = 0; k < 2; k++)
            if ((uint32_t)k < na.col_mm) {
                mlp32_hidden(Wc + 512 + k * 1024, lane, hc_last);
#pragma unroll
                for (int ob = 0; ob < 4; ob++) hc[k + 1][ob] = hc_last[ob];
            }
        const f32x4 co = mlp32_out(Wc + 512 + na.col_mm * 1024, lane, hc_last);
        f32x4 gco = {0, 0, 0, 0};
        if (q == 0) {
#pragma unroll
            for (int k3 = 0; k3 < 3; k3++) {
                const float yv = 1.0f / (1.0f + expf(-co[k3]));
                gco[k3] = G[k3] * wsc * (yv * (1.0f - yv));
            }
        }
        f32x4 acc[4], gc[4];
        mlp32_out_bwd(Bc, lane, gco, acc);
        relu_mask32(acc, hc_last, gc);
#pragma unroll
        for (int l = 1; l >= 0; l--)
            if ((uint32_t)l < na.col_mm) {
                mlp32_hidden_raw(Bc + 256 + (na.col_mm - 1 - l) * 1024, lane, gc, acc);
                relu_mask32(acc, hc[l], gc);
            }
        f32x4 gin[2];
        mlp32_in_bwd(Bc + 256 + na.col_mm * 1024, lane, gc, gin);
        const float gsh[4] = {gin[0][0], gin[0][1], gin[0][2], gin[0][3]};
        sh4_quarter_vjp(q, dx, dy, dz, gsh, gdir);
        gso = gin[1];
        if (q == 0) gso[0] = 0.0f;                          // that slot was the zero pad, not sigma
    }
};

// ---- host side: defined once, in fused_net.hip
// Diagnostics state.  The process-wide setters (ngp_debug_*) only change the DEFAULT; a context can carry its own
// (ngp_render_ctx_set_debug), and every render call takes ONE snapshot when it starts, so concurrent calls on other host threads /
// streams (pipeline.py) never see a half-changed set and never change under a running call.
struct DebugState {
    int flags = 0;
    unsigned long long* stamps = nullptr;
    uint32_t* sample_hash = nullptr;
    bool jump_off() const { return (flags & NGP_DBG_NO_BLOCK_JUMP) != 0; }
    bool coarse_off() const { return (flags & NGP_DBG_NO_COARSE) != 0; }
    bool sort_off() const { return (flags & NGP_DBG_NO_SLOW_SORT) != 0; }
    bool lin_off() const { return (flags & NGP_DBG_NO_LIN) != 0; }
    bool spec_off() const { return (flags & NGP_DBG_ONE_ITER_PER_LAUNCH) != 0; }
    bool tile_off() const { return (flags & NGP_DBG_NO_TILES) != 0; }
    bool pre_verdict_off() const { return (flags & NGP_DBG_NO_PRE_VERDICT) != 0; }
    bool narrow_items_off() const { return (flags & NGP_DBG_WIDE_ITEMS) != 0; }
    bool prefix_replay_off() const { return (flags & NGP_DBG_REPLAY_ONE_ITER) != 0; }
    bool wave_march_off() const { return (flags & NGP_DBG_LANE_MARCH) != 0; }
    bool cell_runs_off() const { return (flags & NGP_DBG_PROBE_PER_SAMPLE) != 0; }
};
DebugState debug_snapshot();   // the process default; a render context may carry its own (render_fused.hip)
bool debug_flags_valid(int flags, const char* who);   // only NGP_DBG_* bits set; else the error text is set (the setters return NGP_EINVAL)
float* grad_dump();             // ngp_debug_set_grad_dump
bool needs_generic(const GridLevels& lv);
int fill_net(const ngp_model* m, const _Float16* packed, NetArgs& na, GridLevels& lv);
size_t weights_bytes(const NetArgs& na);
uint32_t resident_blocks(size_t lds);
int net_variant(const NetArgs& na, const GridLevels& lv);
bool clamped_exact(const NetArgs& na);   // 2*bound is a power of two: the kernels that clamp to [-bound, bound] may instantiate CLAMPED
bool bwd_shape_ok(const NetArgs& na);
// runs STMT with NET bound to the policy class of `variant`
#define NGP_WITH_NET(variant, ...)                                           \
    switch (variant) {                                                       \
        case 0: { using NET = NetF16<0>; __VA_ARGS__; } break;               \
        case 1: { using NET = NetF16<1>; __VA_ARGS__; } break;               \
        case 2: { using NET = NetF16<2>; __VA_ARGS__; } break;               \
        case 3: { using NET = NetF32<0>; __VA_ARGS__; } break;               \
        case 4: { using NET = NetF32<1>; __VA_ARGS__; } break;               \
        case 5: { using NET = NetF16<0, true>; __VA_ARGS__; } break;         \
        case 6: { using NET = NetF16<1, true>; __VA_ARGS__; } break;         \
        default: { using NET = NetF16<2, true>; __VA_ARGS__; } break;        \
    }

}  // namespace ngp
