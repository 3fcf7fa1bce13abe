// overlay.hip -- rays against a list of analytic primitives (capsules, axis-aligned boxes), merged by depth with the mesh cast of
// raycast.hip: the failure view of the replay (nerfsafetyvalidation_amd/replay.py), in the place of the Blender scene that the
// reference's runBlenderOnFailure -> validation/utils/viz_failures_blend.py builds (plans as tubes of radius 0.02, the drone's
// positions as cubes of half extent 0.0125).
//
// The primitive table (8 floats per primitive: kind, a.xyz, b.xyz, r), the hit rule per (ray, primitive), the acceptance and the depth
// merge through t_max[ray] are world.py's docstring ("The overlay's hit rule"); overlay_test is that text in float32 with one rounding
// per operation, in its order (this unit is compiled with -ffp-contract=off, holds no fused multiply-add, and uses the correctly
// rounded division and square root).
//
// k_overlay_cast: one lane per ray, 256-thread workgroups (ray_of_thread: with frame_width a wave takes an 8 x 8 pixel tile).  The
// workgroup stages the table through LDS in chunks of 256 records (8 KB); every lane then walks the chunk reading the same address --
// an LDS broadcast, no bank conflicts.  NO LANE LEAVES BEFORE THE LAST BARRIER: a thread with no ray, or a ray that can no longer be
// hit (t_max <= t_min), stays in the loop masked; the barrier count depends on P alone.  No atomics; the result per ray does not
// depend on the chunking.
#include "cast_common.hpp"

namespace ngp {

constexpr uint32_t kOverlayChunk = 256;      // records per LDS chunk
static_assert(kOverlayChunk == kCastBlock, "the staging loop of k_overlay_cast loads one record per thread of the workgroup");

struct OverlayHit {
    float t, nx, ny, nz;
    int32_t prim;
};

// re-centring on c: t0 = (d . (c - o)) inv_dd, o' = o + t0 d -> p = o' - c (the point of the ray's line closest to c, seen from c)
__device__ __forceinline__ float overlay_recentre(float cx, float cy, float cz, float ox, float oy, float oz, float dx, float dy, float dz,
                                                  float inv_dd, float& px, float& py, float& pz) {
    const float t0 = dot3(dx, dy, dz, cx - ox, cy - oy, cz - oz) * inv_dd;
    px = (ox + t0 * dx) - cx;
    py = (oy + t0 * dy) - cy;
    pz = (oz + t0 * dz) - cz;
    return t0;
}

// the nearer root of the sphere |x - c| = r (a cap of the capsule), re-centred on c itself: two capsules that share a joint compute the
// same bits for it, so the joint goes to the lower index.  Replaces (t, n) when strictly smaller.
__device__ __forceinline__ void overlay_cap(float cx, float cy, float cz, float ox, float oy, float oz, float dx, float dy, float dz, float dd,
                                            float inv_dd, float rr, float& t_best, float& nx, float& ny, float& nz) {
    float px, py, pz;
    const float t0 = overlay_recentre(cx, cy, cz, ox, oy, oz, dx, dy, dz, inv_dd, px, py, pz);
    const float Bs = dot3(dx, dy, dz, px, py, pz);
    const float Cs = dot3(px, py, pz, px, py, pz) - rr;
    const float hs = Bs * Bs - dd * Cs;
    if (hs >= 0.0f) {
        const float tp = (-Bs - sqrtf(hs)) / dd;
        const float t = t0 + tp;
        if (t < t_best) {
            t_best = t;
            nx = px + tp * dx;
            ny = py + tp * dy;
            nz = pz + tp * dz;
        }
    }
}

// the hit rule for one (ray, primitive); updates `best` under (smallest t, then lowest index: the caller walks ascending)
__device__ __forceinline__ void overlay_test(const float4 ka, const float4 br, int32_t index, float ox, float oy, float oz, float dx, float dy,
                                             float dz, float dd, float inv_dd, float t_min, float t_max, OverlayHit& best) {
    const float kind = ka.x, ax = ka.y, ay = ka.z, az = ka.w, bx = br.x, by = br.y, bz = br.z, r = br.w;
    const bool capsule = kind == 0.0f;
    if (!capsule && kind != 1.0f) return;                                  // (the host refuses such a table; never trusted here)
    float t = INFINITY, nx = 0.0f, ny = 0.0f, nz = 0.0f;
    if (capsule) {
        const float mx = (ax + bx) * 0.5f, my = (ay + by) * 0.5f, mz = (az + bz) * 0.5f;
        float qx, qy, qz;                                                  // o' - m
        const float t0 = overlay_recentre(mx, my, mz, ox, oy, oz, dx, dy, dz, inv_dd, qx, qy, qz);
        const float bax = bx - ax, bay = by - ay, baz = bz - az;
        const float oax = qx + (mx - ax), oay = qy + (my - ay), oaz = qz + (mz - az);
        const float baba = dot3(bax, bay, baz, bax, bay, baz), rr = r * r;
        const float ux = bay * dz - baz * dy, uy = baz * dx - bax * dz, uz = bax * dy - bay * dx;
        const float A = dot3(ux, uy, uz, ux, uy, uz);
        if (A > 0.0f) {
            const float wx = bay * oaz - baz * oay, wy = baz * oax - bax * oaz, wz = bax * oay - bay * oax;
            const float B = dot3(ux, uy, uz, wx, wy, wz);
            const float C = dot3(wx, wy, wz, wx, wy, wz) - rr * baba;
            const float h = B * B - A * C;
            if (h >= 0.0f) {
                const float tp = (-B - sqrtf(h)) / A;
                const float y = dot3(bax, bay, baz, oax, oay, oaz) + tp * dot3(bax, bay, baz, dx, dy, dz);
                if (y > 0.0f && y < baba) {
                    t = t0 + tp;
                    nx = (oax + tp * dx) * baba - bax * y;
                    ny = (oay + tp * dy) * baba - bay * y;
                    nz = (oaz + tp * dz) * baba - baz * y;
                }
            }
        }
        overlay_cap(ax, ay, az, ox, oy, oz, dx, dy, dz, dd, inv_dd, rr, t, nx, ny, nz);
        overlay_cap(bx, by, bz, ox, oy, oz, dx, dy, dz, dd, inv_dd, rr, t, nx, ny, nz);
    } else {
        float p[3];
        const float t0 = overlay_recentre(ax, ay, az, ox, oy, oz, dx, dy, dz, inv_dd, p[0], p[1], p[2]);
        const float h[3] = {bx, by, bz}, d[3] = {dx, dy, dz};
        float t_near = -INFINITY, t_far = INFINITY;
        int axis = 0;
        bool miss = false;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            if (d[k] == 0.0f) {
                miss = miss || fabsf(p[k]) > h[k];
            } else {
                const float inv = 1.0f / d[k];
                const float t1 = (-h[k] - p[k]) * inv, t2 = (h[k] - p[k]) * inv;
                const float lo = fminf(t1, t2), hi = fmaxf(t1, t2);
                if (lo > t_near) {
                    t_near = lo;
                    axis = k;
                }
                t_far = fminf(t_far, hi);
            }
        }
        if (!miss && t_near <= t_far) {
            t = t0 + t_near;
            const float s = (axis == 0 ? dx : axis == 1 ? dy : dz) > 0.0f ? -1.0f : 1.0f;
            nx = axis == 0 ? s : 0.0f;
            ny = axis == 1 ? s : 0.0f;
            nz = axis == 2 ? s : 0.0f;
        }
    }
    if (t > t_min && t < t_max && t < best.t) best = OverlayHit{t, nx, ny, nz, index};
}

__global__ void __launch_bounds__(kCastBlock) k_overlay_cast(const float* __restrict__ rays_o, const float* __restrict__ rays_d, uint32_t N,
                                                             const float4* __restrict__ prims, uint32_t P, float t_min,
                                                             const float* __restrict__ t_max, uint32_t frame_width, float* __restrict__ out_t,
                                                             int32_t* __restrict__ out_prim, float* __restrict__ out_normal) {
    __shared__ float4 s_ka[kOverlayChunk], s_br[kOverlayChunk];
    uint32_t r = 0;
    const bool has_ray = ray_of_thread(N, frame_width, r);      // never a reason to return: NO LANE LEAVES BEFORE THE LAST BARRIER
    float o[3] = {0.0f, 0.0f, 0.0f}, d[3] = {0.0f, 0.0f, 0.0f}, far = 0.0f;
    if (has_ray) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            o[k] = rays_o[3 * (size_t)r + k];
            d[k] = rays_d[3 * (size_t)r + k];
        }
        far = t_max ? t_max[r] : INFINITY;
    }
    const bool finite = isfinite(o[0]) && isfinite(o[1]) && isfinite(o[2]) && isfinite(d[0]) && isfinite(d[1]) && isfinite(d[2]);
    const bool moving = d[0] != 0.0f || d[1] != 0.0f || d[2] != 0.0f;
    const bool active = has_ray && finite && moving && far > t_min;      // (masked, not gone: the barriers below need every lane)
    const float dd = dot3(d[0], d[1], d[2], d[0], d[1], d[2]), inv_dd = 1.0f / dd;
    OverlayHit best{INFINITY, 0.0f, 0.0f, 0.0f, -1};

    for (uint32_t base = 0; base < P; base += kOverlayChunk) {           // (uniform: P is the same for every thread)
        const uint32_t n = min(kOverlayChunk, P - base);
        __syncthreads();                                                  // the previous chunk has been read by every lane
        if (threadIdx.x < n) {
            s_ka[threadIdx.x] = prims[2 * (size_t)(base + threadIdx.x)];
            s_br[threadIdx.x] = prims[2 * (size_t)(base + threadIdx.x) + 1];
        }
        __syncthreads();
        if (active) {
            for (uint32_t j = 0; j < n; j++)
                overlay_test(s_ka[j], s_br[j], (int32_t)(base + j), o[0], o[1], o[2], d[0], d[1], d[2], dd, inv_dd, t_min, far, best);
        }
    }
    if (has_ray) {
        out_t[r] = best.t;
        out_prim[r] = best.prim;
        out_normal[3 * (size_t)r] = best.nx;
        out_normal[3 * (size_t)r + 1] = best.ny;
        out_normal[3 * (size_t)r + 2] = best.nz;
    }
}

// where the overlay hit: the primitive's colour times the headlight on the hit's normal over the world's pixel; every other pixel
// keeps its bits
__global__ void __launch_bounds__(kCastBlock) k_overlay_shade(const float* __restrict__ rays_d, const int32_t* __restrict__ prim,
                                                              const float* __restrict__ normal, uint32_t N, const float* __restrict__ colors,
                                                              uint32_t P, float ambient, float* __restrict__ image, uint8_t* __restrict__ image_u8) {
    const uint32_t r = blockIdx.x * kCastBlock + threadIdx.x;
    if (r >= N) return;
    const int32_t f = prim[r];
    if (f < 0 || (uint32_t)f >= P) return;
    const float dx = rays_d[3 * (size_t)r], dy = rays_d[3 * (size_t)r + 1], dz = rays_d[3 * (size_t)r + 2];
    const float nx = normal[3 * (size_t)r], ny = normal[3 * (size_t)r + 1], nz = normal[3 * (size_t)r + 2];
    const float shade = headlight(nx, ny, nz, dx, dy, dz, ambient);
#pragma unroll
    for (int k = 0; k < 3; k++) store_rgb(image, image_u8, r, k, fminf(fmaxf(colors[3 * (size_t)f + k] * shade, 0.0f), 1.0f));
}

}  // namespace ngp

using namespace ngp;

extern "C" {

int ngp_overlay_cast(const float* rays_o, const float* rays_d, uint64_t N, const float* prims_host, const float* prims, uint32_t P, float t_min,
                     const float* t_max, uint32_t frame_width, float* t, int32_t* prim, float* normal, ngp_stream_t stream) {
    NGP_REQUIRE(N < ((uint64_t)1 << 31), "overlay_cast: N must be < 2^31 (got %llu)", (unsigned long long)N);
    NGP_REQUIRE(P < (1u << 31), "overlay_cast: P must be < 2^31 (got %u)", P);
    NGP_REQUIRE(t_min == t_min, "overlay_cast: t_min is NaN");
    NGP_REQUIRE(P == 0 || (prims_host && prims), "overlay_cast: null primitive table");
    for (uint32_t i = 0; i < P; i++) {
        const float* q = prims_host + 8 * (size_t)i;
        NGP_REQUIRE(q[0] == 0.0f || q[0] == 1.0f, "overlay_cast: primitive %u has kind %g (0: capsule, 1: box)", i, (double)q[0]);
        for (int k = 1; k < 8; k++) NGP_REQUIRE(q[k] - q[k] == 0.0f, "overlay_cast: primitive %u has a non-finite field (%d)", i, k);
        NGP_REQUIRE(q[7] > 0.0f, "overlay_cast: primitive %u has r = %g (must be > 0)", i, (double)q[7]);
    }
    if (N == 0) return NGP_OK;
    NGP_REQUIRE(rays_o && rays_d && t && prim && normal, "overlay_cast: null pointer");
    NGP_REQUIRE(((uintptr_t)prims & 15) == 0, "overlay_cast: the primitive table must be 16-byte aligned");
    uint32_t threads;
    const int rc = cast_plan("overlay_cast", N, frame_width, threads);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("overlay_cast", s, (double)N * (double)P);
    k_overlay_cast<<<div_up(threads, kCastBlock), kCastBlock, 0, s>>>(rays_o, rays_d, (uint32_t)N, reinterpret_cast<const float4*>(prims), P,
                                                                     t_min, t_max, frame_width, t, prim, normal);
    return check_launch("overlay_cast");
}

int ngp_overlay_shade(const float* rays_d, const int32_t* prim, const float* normal, uint64_t N, const float* colors, uint32_t P, float ambient,
                      float* image, uint8_t* image_u8, ngp_stream_t stream) {
    NGP_REQUIRE(N < ((uint64_t)1 << 31), "overlay_shade: N must be < 2^31 (got %llu)", (unsigned long long)N);
    NGP_REQUIRE(P < (1u << 31), "overlay_shade: P must be < 2^31 (got %u)", P);
    NGP_REQUIRE(ambient >= 0.0f && ambient <= 1.0f, "overlay_shade: ambient must be in [0, 1]");
    if (N == 0 || P == 0) return NGP_OK;
    NGP_REQUIRE(rays_d && prim && normal && colors && image && image_u8, "overlay_shade: null pointer");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("overlay_shade", s, (double)N);
    k_overlay_shade<<<div_up((uint32_t)N, kCastBlock), kCastBlock, 0, s>>>(rays_d, prim, normal, (uint32_t)N, colors, P, ambient, image,
                                                                          image_u8);
    return check_launch("overlay_shade");
}

}  // extern "C"
