// raycast.hip -- rays against a triangle mesh (nerfsafetyvalidation_amd/world.py): the ground-truth camera of the safety-validation
// loop, in the place of the Blender subprocess of the reference's second simulator (validation/simulators/BlenderSimulator.py:82,102).
//
// The hit rule and the shading are world.py's docstring ("The hit rule", "Shading"); test_triangle and k_raycast_shade are that text in
// float32 with one rounding per operation, in its order (this unit is compiled with -ffp-contract=off and holds no fmaf).  The
// per-triangle data v0, e1, e2 are packed once by the caller, three 16-byte rows per triangle.
// The grid only chooses WHICH triangles a ray is tested against; the arithmetic per (ray, triangle) is fixed.
//
// Acceleration structure: a uniform grid over the (padded) bounding box, built without atomics in the count -> scan -> emit form of
// mesh.hip:
//   k_bin_count   per triangle, the number of cells its bounding box, grown by grid.grow, overlaps
//   (torch)       exclusive scan of the counts
//   k_bin_emit    each triangle writes its (cell, triangle) pairs at its own offset, cells in C order
//   (torch)       stable sort by cell (every cell's list ascending in the triangle index) and the cell start table
// Traversal (k_raycast, one lane per ray): the ray is clipped to the grid box, then a 3-D DDA walks the cells.  The exit parameter
// of a cell is recomputed from the cell index at every step (no accumulated t), the walk ends when the best t is not beyond the
// current cell's exit or the ray leaves the box, and it has a hard bound of nx + ny + nz + 3 cells.  A ray whose origin has a component
// beyond grid.reach, or whose direction has a component outside 2^-40 .. 2^40, is tested against every triangle
// instead (bounded by F): the coverage argument needs the DDA's rounding to stay far below grid.grow, and that holds only for
// ordinary rays near the box.
// With frame_width the 64 lanes of a wave take an 8 x 8 pixel tile of the row-major frame, so a wave's rays walk the same cells.
#include "cast_common.hpp"

namespace ngp {

struct CastHit {
    float t, u, v;
    int32_t prim;
};

// the hit rule for one (ray, triangle); updates `best` under (smallest t, then lowest index)
__device__ __forceinline__ void test_triangle(const Tri& T, int32_t f, float ox, float oy, float oz, float dx, float dy, float dz, float t_min,
                                              float t_max, CastHit& best) {
    const float px = dy * T.e2z - dz * T.e2y, py = dz * T.e2x - dx * T.e2z, pz = dx * T.e2y - dy * T.e2x;
    const float det = dot3(T.e1x, T.e1y, T.e1z, px, py, pz);
    if (det == 0.0f) return;
    const float inv = 1.0f / det;
    const float sx = ox - T.v0x, sy = oy - T.v0y, sz = oz - T.v0z;
    const float u = dot3(sx, sy, sz, px, py, pz) * inv;
    const float qx = sy * T.e1z - sz * T.e1y, qy = sz * T.e1x - sx * T.e1z, qz = sx * T.e1y - sy * T.e1x;
    const float v = dot3(dx, dy, dz, qx, qy, qz) * inv;
    const float t = dot3(T.e2x, T.e2y, T.e2z, qx, qy, qz) * inv;
    if (u >= 0.0f && v >= 0.0f && u + v <= 1.0f && t > t_min && t < t_max) {
        if (t < best.t || (t == best.t && f < best.prim)) best = CastHit{t, u, v, f};
    }
}

// cell range [c0, c1] (inclusive, clamped to the grid) of the interval [lo - grow, hi + grow] on one axis
__device__ __forceinline__ void cell_range(float lo, float hi, float glo, float inv_cell, float grow, uint32_t n, uint32_t& c0, uint32_t& c1) {
    const float top = (float)(n - 1);
    const float a = floorf(((lo - grow) - glo) * inv_cell), b = floorf(((hi + grow) - glo) * inv_cell);
    c0 = (uint32_t)fminf(fmaxf(a, 0.0f), top);       // (fmaxf / fminf drop a NaN: a broken vertex lands in cell 0)
    c1 = (uint32_t)fminf(fmaxf(b, 0.0f), top);
    if (c1 < c0) c1 = c0;
}

struct TriCells {
    uint32_t x0, x1, y0, y1, z0, z1;
};

__device__ __forceinline__ TriCells tri_cells(const Tri& T, const ngp_raycast_grid& G) {
    const float ax = T.v0x + T.e1x, ay = T.v0y + T.e1y, az = T.v0z + T.e1z;
    const float bx = T.v0x + T.e2x, by = T.v0y + T.e2y, bz = T.v0z + T.e2z;
    TriCells c;
    cell_range(fminf(T.v0x, fminf(ax, bx)), fmaxf(T.v0x, fmaxf(ax, bx)), G.lo[0], G.inv_cell[0], G.grow[0], G.n[0], c.x0, c.x1);
    cell_range(fminf(T.v0y, fminf(ay, by)), fmaxf(T.v0y, fmaxf(ay, by)), G.lo[1], G.inv_cell[1], G.grow[1], G.n[1], c.y0, c.y1);
    cell_range(fminf(T.v0z, fminf(az, bz)), fmaxf(T.v0z, fmaxf(az, bz)), G.lo[2], G.inv_cell[2], G.grow[2], G.n[2], c.z0, c.z1);
    return c;
}

__global__ void __launch_bounds__(kCastBlock) k_bin_count(const float4* __restrict__ tri_data, uint32_t F, ngp_raycast_grid G,
                                                          int32_t* __restrict__ counts) {
    const uint32_t f = blockIdx.x * kCastBlock + threadIdx.x;
    if (f >= F) return;
    const TriCells c = tri_cells(load_tri(tri_data, f), G);
    counts[f] = (int32_t)((c.x1 - c.x0 + 1) * (c.y1 - c.y0 + 1) * (c.z1 - c.z0 + 1));      // <= 256^3
}

__global__ void __launch_bounds__(kCastBlock) k_bin_emit(const float4* __restrict__ tri_data, uint32_t F, ngp_raycast_grid G,
                                                         const int64_t* __restrict__ offsets, uint32_t P, int32_t* __restrict__ pair_cell,
                                                         int32_t* __restrict__ pair_tri) {
    const uint32_t f = blockIdx.x * kCastBlock + threadIdx.x;
    if (f >= F) return;
    const TriCells c = tri_cells(load_tri(tri_data, f), G);
    int64_t k = offsets[f];
    if (k < 0) return;
    for (uint32_t x = c.x0; x <= c.x1; x++)
        for (uint32_t y = c.y0; y <= c.y1; y++)
            for (uint32_t z = c.z0; z <= c.z1; z++, k++) {
                if (k >= (int64_t)P) return;          // (P is the caller's: never write past what it describes)
                pair_cell[k] = (int32_t)((x * G.n[1] + y) * G.n[2] + z);
                pair_tri[k] = (int32_t)f;
            }
}

__global__ void __launch_bounds__(kCastBlock) k_raycast(const float* __restrict__ rays_o, const float* __restrict__ rays_d, uint32_t N,
                                                        ngp_raycast_grid G, const int32_t* __restrict__ cell_start,
                                                        const int32_t* __restrict__ pair_tri, uint32_t P, const float4* __restrict__ tri_data,
                                                        uint32_t F, float t_min, float t_max, uint32_t frame_width, float* __restrict__ out_t,
                                                        int32_t* __restrict__ out_prim, float* __restrict__ out_u, float* __restrict__ out_v) {
    uint32_t r;
    if (!ray_of_thread(N, frame_width, r)) return;
    const float o[3] = {rays_o[3 * (size_t)r], rays_o[3 * (size_t)r + 1], rays_o[3 * (size_t)r + 2]};
    const float d[3] = {rays_d[3 * (size_t)r], rays_d[3 * (size_t)r + 1], rays_d[3 * (size_t)r + 2]};
    CastHit best{INFINITY, 0.0f, 0.0f, 0x7FFFFFFF};

    const bool finite = isfinite(o[0]) && isfinite(o[1]) && isfinite(o[2]) && isfinite(d[0]) && isfinite(d[1]) && isfinite(d[2]);
    const bool moving = d[0] != 0.0f || d[1] != 0.0f || d[2] != 0.0f;
    if (finite && moving) {
        // ordinary ray: origin within grid.reach of zero, every non-zero direction component within 2^-40 .. 2^40
        bool ordinary = true;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const float m = fabsf(d[a]);
            ordinary = ordinary && (m == 0.0f || (m >= 0x1p-40f && m <= 0x1p40f)) && fabsf(o[a]) <= G.reach;
        }
        if (!ordinary) {
            for (uint32_t f = 0; f < F; f++) test_triangle(load_tri(tri_data, f), (int32_t)f, o[0], o[1], o[2], d[0], d[1], d[2], t_min, t_max, best);
        } else {
            // clip to the grid box
            float t_in = t_min, t_out = t_max, inv_d[3];
            bool inside = true;
#pragma unroll
            for (int a = 0; a < 3; a++) {
                const float hi = G.lo[a] + (float)G.n[a] * G.cell[a];
                if (d[a] == 0.0f) {
                    inv_d[a] = 0.0f;
                    inside = inside && o[a] >= G.lo[a] && o[a] <= hi;
                } else {
                    inv_d[a] = 1.0f / d[a];
                    const float t0 = (G.lo[a] - o[a]) * inv_d[a], t1 = (hi - o[a]) * inv_d[a];
                    t_in = fmaxf(t_in, fminf(t0, t1));
                    t_out = fminf(t_out, fmaxf(t0, t1));
                }
            }
            if (inside && t_in <= t_out) {
                int32_t c[3], step[3];
                float t_next[3];
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    const float top = (float)(G.n[a] - 1);
                    const float p = d[a] == 0.0f ? o[a] : o[a] + t_in * d[a];
                    c[a] = (int32_t)fminf(fmaxf(floorf((p - G.lo[a]) * G.inv_cell[a]), 0.0f), top);
                    step[a] = d[a] > 0.0f ? 1 : (d[a] < 0.0f ? -1 : 0);
                }
                const uint32_t max_cells = G.n[0] + G.n[1] + G.n[2] + 3;
                for (uint32_t it = 0; it < max_cells; it++) {
                    const uint32_t cell = ((uint32_t)c[0] * G.n[1] + (uint32_t)c[1]) * G.n[2] + (uint32_t)c[2];
                    const uint32_t k0 = min((uint32_t)cell_start[cell], P), k1 = min((uint32_t)cell_start[cell + 1], P);
                    for (uint32_t k = k0; k < k1; k++) {
                        const uint32_t f = (uint32_t)pair_tri[k];
                        if (f >= F) continue;
                        test_triangle(load_tri(tri_data, f), (int32_t)f, o[0], o[1], o[2], d[0], d[1], d[2], t_min, t_max, best);
                    }
                    // the parameter at which the ray leaves this cell, from the cell index (nothing accumulates)
#pragma unroll
                    for (int a = 0; a < 3; a++) {
                        const float plane = G.lo[a] + (float)(c[a] + (step[a] > 0 ? 1 : 0)) * G.cell[a];
                        t_next[a] = step[a] == 0 ? INFINITY : (plane - o[a]) * inv_d[a];
                    }
                    int ax = t_next[0] <= t_next[1] ? 0 : 1;
                    ax = t_next[ax] <= t_next[2] ? ax : 2;
                    const float t_exit = t_next[ax];
                    if (best.t <= t_exit || t_exit > t_out) break;
                    // (a select chain, not c[ax]: a runtime index would put the arrays in scratch)
                    const int32_t n_ax = (int32_t)(ax == 0 ? G.n[0] : ax == 1 ? G.n[1] : G.n[2]);
                    const int32_t nc = (ax == 0 ? c[0] : ax == 1 ? c[1] : c[2]) + (ax == 0 ? step[0] : ax == 1 ? step[1] : step[2]);
                    if (nc < 0 || nc >= n_ax) break;
                    if (ax == 0) c[0] = nc;
                    else if (ax == 1) c[1] = nc;
                    else c[2] = nc;
                }
            }
        }
    }
    const bool hit = best.prim != 0x7FFFFFFF;
    out_t[r] = best.t;
    out_prim[r] = hit ? best.prim : -1;
    out_u[r] = best.u;
    out_v[r] = best.v;
}

// the barycentric blend of the vertex colours (mid-grey without) times the headlight on n = e1 x e2; a miss is the background
__global__ void __launch_bounds__(kCastBlock) k_raycast_shade(const float* __restrict__ rays_d, const int32_t* __restrict__ prim,
                                                              const float* __restrict__ hit_u, const float* __restrict__ hit_v, uint32_t N,
                                                              const float4* __restrict__ tri_data, const int32_t* __restrict__ faces, uint32_t F,
                                                              const float* __restrict__ colors, uint32_t V, float ambient, float bg0, float bg1,
                                                              float bg2, float* __restrict__ image, uint8_t* __restrict__ image_u8) {
    const uint32_t r = blockIdx.x * kCastBlock + threadIdx.x;
    if (r >= N) return;
    float rgb[3] = {bg0, bg1, bg2};
    const int32_t f = prim[r];
    if (f >= 0 && (uint32_t)f < F) {
        const Tri T = load_tri(tri_data, (uint32_t)f);
        const float u = hit_u[r], v = hit_v[r], w = (1.0f - u) - v;
        float col[3] = {0.5f, 0.5f, 0.5f};
        if (colors) {
            const uint32_t i0 = (uint32_t)faces[3 * (size_t)f], i1 = (uint32_t)faces[3 * (size_t)f + 1], i2 = (uint32_t)faces[3 * (size_t)f + 2];
            if (i0 < V && i1 < V && i2 < V) {
#pragma unroll
                for (int k = 0; k < 3; k++) col[k] = (w * colors[3 * (size_t)i0 + k] + u * colors[3 * (size_t)i1 + k]) + v * colors[3 * (size_t)i2 + k];
            }
        }
        const float dx = rays_d[3 * (size_t)r], dy = rays_d[3 * (size_t)r + 1], dz = rays_d[3 * (size_t)r + 2];
        const float nx = T.e1y * T.e2z - T.e1z * T.e2y, ny = T.e1z * T.e2x - T.e1x * T.e2z, nz = T.e1x * T.e2y - T.e1y * T.e2x;
        const float shade = headlight(nx, ny, nz, dx, dy, dz, ambient);
#pragma unroll
        for (int k = 0; k < 3; k++) rgb[k] = fminf(fmaxf(col[k] * shade, 0.0f), 1.0f);
    }
#pragma unroll
    for (int k = 0; k < 3; k++) store_rgb(image, image_u8, r, k, rgb[k]);
}

}  // namespace ngp

using namespace ngp;

extern "C" {

int ngp_raycast_bin_count(const float* tri_data, uint32_t F, const ngp_raycast_grid* grid, int32_t* counts, ngp_stream_t stream) {
    int rc = cast_check_grid("raycast_bin_count", grid);
    if (rc) return rc;
    NGP_REQUIRE(F >= 1 && F < (1u << 31), "raycast_bin_count: 1 <= F < 2^31 (got %u)", F);
    NGP_REQUIRE(tri_data && counts, "raycast_bin_count: null pointer");
    NGP_REQUIRE(((uintptr_t)tri_data & 15) == 0, "raycast_bin_count: tri_data must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("raycast_bin_count", s, (double)F);
    k_bin_count<<<div_up(F, kCastBlock), kCastBlock, 0, s>>>(reinterpret_cast<const float4*>(tri_data), F, *grid, counts);
    return check_launch("raycast_bin_count");
}

int ngp_raycast_bin_emit(const float* tri_data, uint32_t F, const ngp_raycast_grid* grid, const int64_t* offsets, uint64_t P, int32_t* pair_cell,
                         int32_t* pair_tri, ngp_stream_t stream) {
    int rc = cast_check_grid("raycast_bin_emit", grid);
    if (rc) return rc;
    NGP_REQUIRE(F >= 1 && F < (1u << 31), "raycast_bin_emit: 1 <= F < 2^31 (got %u)", F);
    NGP_REQUIRE(P >= 1 && P < ((uint64_t)1 << 31), "raycast_bin_emit: 1 <= pairs < 2^31 (got %llu)", (unsigned long long)P);
    NGP_REQUIRE(tri_data && offsets && pair_cell && pair_tri, "raycast_bin_emit: null pointer");
    NGP_REQUIRE(((uintptr_t)tri_data & 15) == 0, "raycast_bin_emit: tri_data must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("raycast_bin_emit", s, (double)P);
    k_bin_emit<<<div_up(F, kCastBlock), kCastBlock, 0, s>>>(reinterpret_cast<const float4*>(tri_data), F, *grid, offsets, (uint32_t)P, pair_cell,
                                                            pair_tri);
    return check_launch("raycast_bin_emit");
}

int ngp_raycast(const float* rays_o, const float* rays_d, uint64_t N, const ngp_raycast_grid* grid, const int32_t* cell_start,
                const int32_t* pair_tri, uint64_t P, const float* tri_data, uint32_t F, float t_min, float t_max, uint32_t frame_width, float* t,
                int32_t* prim, float* u, float* v, ngp_stream_t stream) {
    int rc = cast_check_grid("raycast", grid);
    if (rc) return rc;
    NGP_REQUIRE(N < ((uint64_t)1 << 31), "raycast: N must be < 2^31 (got %llu)", (unsigned long long)N);
    NGP_REQUIRE(F >= 1 && F < (1u << 31), "raycast: 1 <= F < 2^31 (got %u)", F);
    NGP_REQUIRE(P >= 1 && P < ((uint64_t)1 << 31), "raycast: 1 <= pairs < 2^31 (got %llu)", (unsigned long long)P);
    NGP_REQUIRE(t_min == t_min && t_max == t_max, "raycast: t_min / t_max is NaN");
    if (N == 0) return NGP_OK;
    NGP_REQUIRE(rays_o && rays_d && cell_start && pair_tri && tri_data && t && prim && u && v, "raycast: null pointer");
    NGP_REQUIRE(((uintptr_t)tri_data & 15) == 0, "raycast: tri_data must be 16-byte aligned");
    uint32_t threads;
    rc = cast_plan("raycast", N, frame_width, threads);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("raycast", s, (double)N);
    k_raycast<<<div_up(threads, kCastBlock), kCastBlock, 0, s>>>(rays_o, rays_d, (uint32_t)N, *grid, cell_start, pair_tri, (uint32_t)P,
                                                                 reinterpret_cast<const float4*>(tri_data), F, t_min, t_max, frame_width, t, prim, u, v);
    return check_launch("raycast");
}

int ngp_raycast_shade(const float* rays_d, const int32_t* prim, const float* u, const float* v, uint64_t N, const float* tri_data,
                      const int32_t* faces, uint32_t F, const float* colors, uint32_t V, float ambient, const float* bg_color3_host, float* image,
                      uint8_t* image_u8, ngp_stream_t stream) {
    NGP_REQUIRE(N < ((uint64_t)1 << 31), "raycast_shade: N must be < 2^31 (got %llu)", (unsigned long long)N);
    NGP_REQUIRE(F >= 1 && F < (1u << 31), "raycast_shade: 1 <= F < 2^31 (got %u)", F);
    NGP_REQUIRE(ambient >= 0.0f && ambient <= 1.0f, "raycast_shade: ambient must be in [0, 1]");
    NGP_REQUIRE(bg_color3_host, "raycast_shade: null background");
    if (N == 0) return NGP_OK;
    NGP_REQUIRE(rays_d && prim && u && v && tri_data && image && image_u8, "raycast_shade: null pointer");
    NGP_REQUIRE(!colors || faces, "raycast_shade: vertex colours need the faces");
    NGP_REQUIRE(((uintptr_t)tri_data & 15) == 0, "raycast_shade: tri_data must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("raycast_shade", s, (double)N);
    k_raycast_shade<<<div_up((uint32_t)N, kCastBlock), kCastBlock, 0, s>>>(rays_d, prim, u, v, (uint32_t)N, reinterpret_cast<const float4*>(tri_data),
                                                                          faces, F, colors, V, ambient, bg_color3_host[0], bg_color3_host[1],
                                                                          bg_color3_host[2], image, image_u8);
    return check_launch("raycast_shade");
}

}  // extern "C"
