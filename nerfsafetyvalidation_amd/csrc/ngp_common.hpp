// Shared host/device helpers of libngp_hip (gfx950 only).
//
// Numerics contract (DESIGN.md "Numerics"): every translation unit is compiled with
// -ffp-contract=off; the fused multiply-adds nvcc's default -fmad=true would form in the
// reference's expressions are written explicitly as fmaf().
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string>

#include "../../include/ngp_hip.h"
#include "workspace.hpp"

namespace ngp {

// ---- error plumbing (set_error: declared in workspace.hpp) -----------------------
int check_launch(const char* what);

#define NGP_REQUIRE(cond, ...)                 \
    do {                                       \
        if (!(cond)) {                         \
            ngp::set_error(__VA_ARGS__);       \
            return NGP_EINVAL;                 \
        }                                      \
    } while (0)

// ---- diagnostics switches read from the environment (capi.hip; read on every call, never cached) ----
bool env_set(const char* name);                        // the variable exists
uint32_t env_u32(const char* name, uint32_t dflt);     // its integer value, `dflt` when it does not

// ---- optional per-kernel timing (ngp_prof_*) -----------------------------------
struct ProfScope {
    ProfScope(const char* name, hipStream_t s, double units);
    ~ProfScope();
    int slot;
    hipStream_t stream;
};
bool prof_enabled();
void prof_add_units(const char* name, double units);

static inline uint32_t div_up(uint32_t a, uint32_t b) { return (a + b - 1) / b; }

// ---- the fixed-order mean of N floats (train_data.hip; its order: DESIGN.md "Cross-lane arithmetic", device pieces in wave_ops.hpp) ----
constexpr uint32_t kMeanOneBlockRays = 16384;      // up to here one 1024-thread workgroup forms the mean: one launch, no workspace
constexpr uint32_t kMeanOneBlockThreads = 1024;
constexpr uint32_t kMeanGroupThreads = 256;        // above: 256 values per workgroup into per-64 group sums, then one wave over the groups
// [(N + 63) / 64] group sums; nothing up to kMeanOneBlockRays
static inline float* mean_layout(Carver& c, uint32_t N) { return c.take<float>(N <= kMeanOneBlockRays ? 0 : div_up(N, 64)); }
static inline size_t mean_workspace(uint32_t N) { Carver c; mean_layout(c, N); return c.bytes(); }
// *mean = mean of values[0 .. N); mean_workspace(N) bytes of workspace, 4-byte aligned (check_workspace's codes).  `what` names the caller in errors.
int mean_of_rays(const float* values, uint32_t N, float* mean, void* workspace, size_t workspace_bytes, hipStream_t s, const char* what);
// the last step alone, for a caller that formed the (N + 63) / 64 group sums in a pass of its own (N > kMeanOneBlockRays)
int mean_of_groups(const float* groups, uint32_t N, float* mean, hipStream_t s, const char* what);

// hipFuncSetAttribute(..., hipFuncAttributeMaxDynamicSharedMemorySize, bytes), once per (device, kernel): the attribute belongs to
// the kernel's code object on ONE device, and render calls arrive from several host threads (pipeline.py) -- a plain
// `static bool` guard is neither per device nor safe to race on.
void ensure_dynamic_lds(const void* func, int bytes);

// ---- hash-grid level geometry, evaluated once per call on the host -----------------
// scale / resolution exactly as gridencoder.cu:126-128; the index recipe of get_grid_index
// (gridencoder.cu:54-72) is folded into per-level multipliers so that the device code does
// no data-dependent loop:  index = hashed ? fast_hash(p) : p0 + p1*mul1 + p2*mul2, then
// reduced modulo hashmap_size (mode 0: already < size, 1: size is a power of two, 2: generic %).
constexpr int kMaxLevels = 32;
struct GridLevels {
    float scale[kMaxLevels];
    uint32_t resolution[kMaxLevels];
    uint32_t offset[kMaxLevels + 1];
    uint32_t mul1[kMaxLevels], mul2[kMaxLevels];
    uint8_t hashed[kMaxLevels], mode[kMaxLevels];
};
void fill_levels(GridLevels& lv, const int32_t* offsets_host, uint32_t L, float S, uint32_t H, uint32_t D, uint32_t gridtype,
                 bool align_corners);

// ---- device helpers ---------------------------------------------------------------
// fp16(w * g) with the reference's two roundings (fp32 product, then fp16; c10::Half arithmetic,
// gridencoder.cu:169-172).  The empty asm keeps hipcc from folding the multiply and the conversion
// into v_fma_mixlo_f16, which rounds once and differs in rare tie cases.
__device__ __forceinline__ _Float16 mul_round_f16(float w, _Float16 g) {
    float p = w * (float)g;
    asm volatile("" : "+v"(p));
    return (_Float16)p;
}
__device__ __forceinline__ float clampf(float x, float lo, float hi) { return fminf(hi, fmaxf(lo, x)); }
__device__ __forceinline__ float signf(float x) { return copysignf(1.0f, x); }

// raymarching.cu:58-83
__device__ __forceinline__ uint32_t expand_bits(uint32_t v) {
    v = (v * 0x00010001u) & 0xFF0000FFu;
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}
__device__ __forceinline__ uint32_t morton3D(uint32_t x, uint32_t y, uint32_t z) {
    return expand_bits(x) | (expand_bits(y) << 1) | (expand_bits(z) << 2);
}
// Same function for v < 1024 (grid cell coordinates: H <= 1024): the products above only ever add disjoint bit fields,
// so they are ORs of shifts -- full-rate instructions instead of quarter-rate v_mul_lo_u32.
__device__ __forceinline__ uint32_t expand_bits10(uint32_t v) {
    v = (v | (v << 16)) & 0xFF0000FFu;
    v = (v | (v << 8)) & 0x0F00F00Fu;
    v = (v | (v << 4)) & 0xC30C30C3u;
    v = (v | (v << 2)) & 0x49249249u;
    return v;
}
__device__ __forceinline__ uint32_t morton3D_cell(uint32_t x, uint32_t y, uint32_t z) {
    return expand_bits10(x) | (expand_bits10(y) << 1) | (expand_bits10(z) << 2);
}
// The grid sizes of the occupancy grid and the density grid: a power of two in [2, 1024].  A cell's index is level * H^3 +
// morton3D(x, y, z), and the Morton code stays below H^3 only then (H = 48: morton3D(47, 47, 47) = 233 471 against 110 592 cells), so
// with any other H a march would read, and mark_untrained_grid write, past the level and past the buffer.  The reference has the same
// defect and only ever uses 128; here every entry point refuses on the host.
inline bool grid_size_ok(uint32_t H) { return H >= 2 && H <= 1024 && (H & (H - 1)) == 0; }
#define NGP_GRID_SIZE_RULE "H must be a power of two in [2, 1024]: cells are indexed by morton3D(x, y, z), which exceeds H^3 otherwise"

}  // namespace ngp
