// collision.hip -- the exact 3-D Euclidean distance transform behind the rollout's signed distance field (nerfsafetyvalidation_amd/
// collision.py): the GPU form of validation/utils/createSDF.py's scipy.ndimage.distance_transform_edt(~map).
//
// d2[x,y,z] = min over occupied cells (x',y',z') of (x-x')^2 + (y-y')^2 + (z-z')^2, in integers, as three separable passes over the
// C-order [X,Y,Z] map (Meijster, Roerdink & Hesselink 2000; the lower-envelope phase is Felzenszwalb & Huttenlocher's):
//
//   k_edt_z      along Z, the contiguous axis: the 1-D distance to the nearest occupied cell of the line, squared.  One WAVE per line:
//                lane l takes cell c0 + l of each 64-cell chunk (coalesced byte loads and dword stores), the nearest occupied index
//                to the left is a wave prefix max, the one to the right a suffix min, carried from chunk to chunk.  A thread per line
//                would stride by Z between lanes; staging lines through LDS would cap Z (a 16384-cell line is 64 KiB of int32, and
//                the stacks of the envelope double that), and the two-sweep pass needs no stacks at all -- so the contiguous axis gets
//                the pass that parallelises across a line, and the sequential envelope runs on the two strided axes.
//   k_edt_env    along Y, then along X: the lower envelope of the parabolas (u - i)^2 + f(i) of the line, f = the previous pass.
//                One THREAD per line; consecutive threads take consecutive z, so every load and store of a step is one coalesced
//                row.  The envelope's stacks (apex index s, start t; uint16 since every dimension is <= 16384) live in the workspace
//                as [position][line], coalesced the same way; the top entry is kept in registers.
//
// Integer arithmetic throughout (int64 inside the envelope): every result is exact and independent of scheduling.  kEdtInf marks
// "no occupied cell": it is >= every finite squared distance (3 * 16383^2 < 2^31 - 1), candidates built on it are clamped back
// to it, and a finite optimum is never displaced by one, so the clamp changes no finite result.  A map with no occupied cell
// comes out as kEdtInf everywhere (NGP_EDT_INF).
#include <limits.h>

#include "ngp_common.hpp"

namespace ngp {

constexpr int32_t kEdtInf = NGP_EDT_INF;
constexpr uint32_t kEdtBlock = 256;
constexpr uint32_t kEdtMaxDim = 16384;

// ---- pass 1: along Z, one wave per (x, y) line ------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kEdtBlock) k_edt_z(const uint8_t* __restrict__ occ, uint32_t lines, uint32_t Z, int32_t* __restrict__ out) {
    const int lane = (int)(threadIdx.x & 63);
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t line = wave; line < lines; line += n_waves) {
        const size_t base = (size_t)line * Z;
        // forward: the last occupied index <= z (-1: none), parked in out[] until the backward sweep
        int carry = -1;
        for (uint32_t c0 = 0; c0 < Z; c0 += 64) {
            const uint32_t z = c0 + lane;
            const bool valid = z < Z;
            int v = (valid && occ[base + z]) ? (int)z : -1;
#pragma unroll      // (a max scan, and a min scan below: wave_ops.hpp's scans are add and mul)
            for (int off = 1; off < 64; off <<= 1) {
                const int t = __shfl_up(v, off, 64);
                if (lane >= off) v = max(v, t);
            }
            v = max(v, carry);
            if (valid) out[base + z] = v;
            carry = __shfl(v, 63, 64);
        }
        // backward: the first occupied index >= z (INT_MAX: none), then the squared distance to the nearer of the two
        carry = INT_MAX;
        for (int c0 = (int)((Z - 1) & ~63u); c0 >= 0; c0 -= 64) {
            const uint32_t z = (uint32_t)c0 + lane;
            const bool valid = z < Z;
            int w = (valid && occ[base + z]) ? (int)z : INT_MAX;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int t = __shfl_down(w, off, 64);
                if (lane + off < 64) w = min(w, t);
            }
            w = min(w, carry);
            carry = __shfl(w, 0, 64);
            if (valid) {
                const int left = out[base + z];
                int d = INT_MAX;
                if (left >= 0) d = (int)z - left;
                if (w != INT_MAX) d = min(d, w - (int)z);
                out[base + z] = d == INT_MAX ? kEdtInf : d * d;
            }
        }
    }
}

// ---- passes 2 and 3: lower envelope along a strided axis, one thread per line ------------------------------------------------------
// line L (of n_lines) starts at (L / inner) * outer_stride + L % inner and steps by `stride`; m cells.
__device__ __forceinline__ int64_t edt_floor_div(int64_t a, int64_t b) {   // b > 0
    return a >= 0 ? a / b : -((-a + b - 1) / b);
}

__global__ void __launch_bounds__(kEdtBlock) k_edt_env(const int32_t* __restrict__ in, int32_t* __restrict__ out, uint32_t n_lines, uint32_t inner,
                                                       size_t outer_stride, size_t stride, uint32_t m, uint16_t* __restrict__ stk_s,
                                                       uint16_t* __restrict__ stk_t) {
    for (uint32_t L = blockIdx.x * blockDim.x + threadIdx.x; L < n_lines; L += gridDim.x * blockDim.x) {
        const size_t base = (size_t)(L / inner) * outer_stride + L % inner;
        const int32_t* f = in + base;
        int32_t* o = out + base;
        uint16_t* S = stk_s + L;     // entry q at S[q * n_lines]
        uint16_t* T = stk_t + L;
        // forward scan: the parabolas that form the lower envelope, and from where each one is lowest
        int q = 0;
        int64_t ts = 0, tt = 0, tf = f[0];        // top of the stack: apex index, start, f(apex)
        S[0] = 0;
        T[0] = 0;
        for (uint32_t u = 1; u < m; u++) {
            const int64_t fu = f[(size_t)u * stride];
            while (q >= 0 && (tt - ts) * (tt - ts) + tf > (tt - (int64_t)u) * (tt - (int64_t)u) + fu) {
                if (--q >= 0) {
                    ts = S[(size_t)q * n_lines];
                    tt = T[(size_t)q * n_lines];
                    tf = f[(size_t)ts * stride];
                }
            }
            if (q < 0) {
                q = 0;
                ts = u; tt = 0; tf = fu;
                S[0] = (uint16_t)u;
                T[0] = 0;
            } else {
                // the first cell where u's parabola is strictly lower than the top's: 1 + floor((u^2 - s^2 + f(u) - f(s)) / (2 (u - s)))
                const int64_t w = 1 + edt_floor_div((int64_t)u * u - ts * ts + fu - tf, 2 * ((int64_t)u - ts));
                if (w < (int64_t)m) {
                    q++;
                    ts = u; tt = w; tf = fu;
                    S[(size_t)q * n_lines] = (uint16_t)u;
                    T[(size_t)q * n_lines] = (uint16_t)w;
                }
            }
        }
        // backward scan: every cell takes the envelope's value
        for (int u = (int)m - 1; u >= 0; u--) {
            const int64_t v = ((int64_t)u - ts) * ((int64_t)u - ts) + tf;
            o[(size_t)u * stride] = v >= kEdtInf ? kEdtInf : (int32_t)v;
            if (u == tt && --q >= 0) {
                ts = S[(size_t)q * n_lines];
                tt = T[(size_t)q * n_lines];
                tf = f[(size_t)ts * stride];
            }
        }
    }
}

static uint32_t edt_blocks(uint32_t threads) {
    const uint32_t b = div_up(threads, kEdtBlock);
    return b > 4096 ? 4096 : (b ? b : 1);
}

struct EdtWs {
    int32_t* mid;                  // [n] the middle pass's output
    uint16_t *stk_s, *stk_t;       // [n] each: the envelope's stacks
};
static EdtWs edt_layout(Carver& c, size_t n) {
    const EdtWs w = {c.take<int32_t>(n), c.take<uint16_t>(n), c.take<uint16_t>(n)};
    c.pad(64);                     // no kernel touches it: kept so that the size stays what it was
    return w;
}

}  // namespace ngp

using namespace ngp;

extern "C" {

size_t ngp_edt_sq_workspace(uint32_t X, uint32_t Y, uint32_t Z) {
    Carver c; edt_layout(c, (size_t)X * Y * Z); return c.bytes();
}

int ngp_edt_sq(const uint8_t* occupied, uint32_t X, uint32_t Y, uint32_t Z, int32_t* d2, void* workspace, size_t workspace_bytes,
               ngp_stream_t stream) {
    NGP_REQUIRE(X >= 1 && Y >= 1 && Z >= 1 && X <= kEdtMaxDim && Y <= kEdtMaxDim && Z <= kEdtMaxDim,
                "edt_sq: every dimension must be in [1, %u] (got %u x %u x %u)", kEdtMaxDim, X, Y, Z);
    const size_t n = (size_t)X * Y * Z;
    NGP_REQUIRE(n < ((size_t)1 << 31), "edt_sq: X * Y * Z must be < 2^31 (got %zu)", n);
    NGP_REQUIRE(occupied && d2, "edt_sq: null pointer");
    int rc = check_workspace("edt_sq", workspace, workspace_bytes, ngp_edt_sq_workspace(X, Y, Z), 4);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    Carver c(workspace);
    const EdtWs w = edt_layout(c, n);
    ProfScope prof("edt_sq", s, (double)n);
    // pass 1 (Z) -> d2; pass 2 (Y): d2 -> mid, lines (x, z); pass 3 (X): mid -> d2, lines (y, z)
    const uint32_t zlines = X * Y;
    k_edt_z<<<div_up(zlines, kEdtBlock / 64) > 4096 ? 4096 : div_up(zlines, kEdtBlock / 64), kEdtBlock, 0, s>>>(occupied, zlines, Z, d2);
    k_edt_env<<<edt_blocks(X * Z), kEdtBlock, 0, s>>>(d2, w.mid, X * Z, Z, (size_t)Y * Z, Z, Y, w.stk_s, w.stk_t);
    k_edt_env<<<edt_blocks(Y * Z), kEdtBlock, 0, s>>>(w.mid, d2, Y * Z, Y * Z, n, (size_t)Y * Z, X, w.stk_s, w.stk_t);
    return check_launch("edt_sq");
}

}  // extern "C"
