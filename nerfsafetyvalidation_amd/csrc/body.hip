// body.hip -- the drone's body as an oriented box, tested against the world's triangles and against a collision map's occupied cells
// (nerfsafetyvalidation_amd/world.py MeshWorld.box_overlap, collision.py box_cells): the verdict of a stress test for a body, not
// for its centre point.
//
// The rules -- the box table, the box-triangle test, the box-cell test -- are world.py's docstring ("The body rule"); body_tri_overlaps
// and body_cell_overlaps are that text in float64 with one IEEE rounding per operation, in its order (this unit is compiled with
// -ffp-contract=off and holds no fma).  Every inequality is written as the rule writes it -- "all three p_k > r", never a min or a max --
// so that a NaN (an overflow of a huge box) decides the same way in numpy and here: it separates nothing.  No kernel computes a
// rotation: R comes in the table.
//
// Work split, both kernels: ONE WAVE PER BOX, lanes over the box's candidates, lane-local minimum, then wave_min.  The batches are
// 4 boxes (a rollout step: launch-bound whatever the split) and 10^4..10^6 (a re-judged stress test: waves enough to fill the chip);
// a box in free space has no candidate, one at a wall has hundreds -- with a lane per box the wave would cost its slowest lane, with a
// wave per box the lanes share one box's candidates and boxes of different cost sit in different waves.  No atomics, no LDS, no
// barrier, no workgroup waits for another; every loop is bounded by the inputs (the grid's cells and pairs, the map's cells).
//
// k_box_mesh: the candidates are the pairs of the cast's grid (cell_start, pair_tri) in the cells the box's bounds reach.  Cells of
// one (x, y) row are consecutive in C order, so their pairs are ONE contiguous range of pair_tri: the lanes stride over it.  A
// triangle listed in several cells is tested several times; the minimum makes that harmless.  A triangle whose index is not below the
// lane's best so far is skipped (it cannot lower the minimum).
// Why the range is a superset (world.py states it too).  b_lo..b_hi: the box's world bounds c_a -+ E_a, E_a = (|R_a0| h_0 + |R_a1|
// h_1) + |R_a2| h_2, permuted into the mesh's axes (a copy or a negation: exact), rounded OUTWARD to float32 and grown by grid.grow.
// f(x) = floor((x - grid.lo) * grid.inv_cell) in float32 is non-decreasing in x (every step is), and so is the clamp to 0..n-1.
// Binning lists a triangle with bounds t_lo..t_hi in the cells clamp(f(t_lo - grow)) .. clamp(f(t_hi + grow)).  A triangle that
// overlaps the box shares a point with the box's bounds, so t_lo <= b_hi and t_hi >= b_lo on every axis, hence f(t_lo - grow) <=
// f(b_hi + grow) and f(t_hi + grow) >= f(b_lo - grow): the two cell ranges intersect on every axis, and the triangle is listed in
// every cell of the product of its ranges.  "Overlaps" is decided in float64, whose rounding (2^-52 relative) is far inside the
// growth (>= S 2^-12 on either side).  The range is EMPTY -- not clamped -- when f(b_hi + grow) < 0 or f(b_lo - grow) >= n: then the
// box lies outside the grid's box, which holds every vertex with a padding of 2^-7 of its extent to spare (the rounding of n * cell
// is 2^-22 of it).  A NaN bound (an overflowing row) takes the whole axis.
//
// k_box_cells: the candidates are the cells floor((c_a - E_a - start_a) g) - 1 .. floor((c_a + E_a - start_a) g) + 1 clipped to the
// map (the voxeliser's range rule: an overlapping cell's centre lies within E_a + 0.5 / g of c_a, so its index is inside with most
// of a cell to spare), walked in C order 64 at a time; an empty cell costs one byte load.  The walk ends after the first 64 that hold
// a hit: C order inside the range is C order in the map, so nothing later can be lower.
#include "cast_common.hpp"
#include "wave_ops.hpp"

namespace ngp {

constexpr uint32_t kBodyBlock = 256;                 // four waves: four boxes
constexpr int32_t kBodyNone = 0x7FFFFFFF;

struct BodyBox {
    double c[3], R[3][3], h[3];                      // indexed by constants only (fully unrolled loops): registers, not scratch
    bool valid;                                      // every entry finite and no half extent negative
};

__device__ __forceinline__ BodyBox body_load(const double* __restrict__ boxes, uint32_t b) {
    const double* __restrict__ q = boxes + 15 * (size_t)b;
    BodyBox B;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 15; k++) ok = ok && (q[k] - q[k] == 0.0);
#pragma unroll
    for (int a = 0; a < 3; a++) {
        B.c[a] = q[a];
        B.h[a] = q[12 + a];
        ok = ok && q[12 + a] >= 0.0;
#pragma unroll
        for (int j = 0; j < 3; j++) B.R[a][j] = q[3 + 3 * a + j];
    }
    B.valid = ok;
    return B;
}

// x in the box's frame: column a of R against x - c, (R_0a d_0 + R_1a d_1) + R_2a d_2
__device__ __forceinline__ void body_to_frame(const BodyBox& B, const double x[3], double out[3]) {
    const double d0 = x[0] - B.c[0], d1 = x[1] - B.c[1], d2 = x[2] - B.c[2];
#pragma unroll
    for (int a = 0; a < 3; a++) out[a] = (B.R[0][a] * d0 + B.R[1][a] * d1) + B.R[2][a] * d2;
}

// the box's half extent along world axis a: (|R_a0| h_0 + |R_a1| h_1) + |R_a2| h_2
__device__ __forceinline__ double body_extent(const BodyBox& B, int a) {
    return (fabs(B.R[a][0]) * B.h[0] + fabs(B.R[a][1]) * B.h[1]) + fabs(B.R[a][2]) * B.h[2];
}

__device__ __forceinline__ bool body_all_above(double p0, double p1, double p2, double r) { return p0 > r && p1 > r && p2 > r; }
__device__ __forceinline__ bool body_all_below(double p0, double p1, double p2, double r) { return p0 < r && p1 < r && p2 < r; }

// one of the nine axes u_i x e_j, reduced to its two non-zero components (a1, a2), the matching components (c1, c2) of the vertices in
// the box's frame and the matching half extents
__device__ __forceinline__ bool body_edge_separates(double a1, double a2, double p0c1, double p0c2, double p1c1, double p1c2, double p2c1,
                                                    double p2c2, double h1, double h2) {
    const double p0 = a1 * p0c1 + a2 * p0c2, p1 = a1 * p1c1 + a2 * p1c2, p2 = a1 * p2c1 + a2 * p2c2;
    const double r = h1 * fabs(a1) + h2 * fabs(a2);
    return body_all_above(p0, p1, p2, r) || body_all_below(p0, p1, p2, -r);
}

// the closed box-triangle test of the rule: w[k][a] the triangle's world vertices; true when no axis separates
__device__ __forceinline__ bool body_tri_overlaps(const BodyBox& B, const double w[3][3]) {
    double p[3][3];
#pragma unroll
    for (int k = 0; k < 3; k++) body_to_frame(B, w[k], p[k]);
#pragma unroll
    for (int a = 0; a < 3; a++)
        if (body_all_above(p[0][a], p[1][a], p[2][a], B.h[a]) || body_all_below(p[0][a], p[1][a], p[2][a], -B.h[a])) return false;
    double e[3][3];      // e0 = v1' - v0', e1 = v2' - v1', e2 = v0' - v2'
#pragma unroll
    for (int a = 0; a < 3; a++) {
        e[0][a] = p[1][a] - p[0][a];
        e[1][a] = p[2][a] - p[1][a];
        e[2][a] = p[0][a] - p[2][a];
    }
    const double nx = e[0][1] * e[1][2] - e[0][2] * e[1][1], ny = e[0][2] * e[1][0] - e[0][0] * e[1][2], nz = e[0][0] * e[1][1] - e[0][1] * e[1][0];
    const double d = (nx * p[0][0] + ny * p[0][1]) + nz * p[0][2];
    if (fabs(d) > (B.h[0] * fabs(nx) + B.h[1] * fabs(ny)) + B.h[2] * fabs(nz)) return false;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        // u_0 x e = (0, -ez, ey);  u_1 x e = (ez, 0, -ex);  u_2 x e = (-ey, ex, 0)
        if (body_edge_separates(-e[j][2], e[j][1], p[0][1], p[0][2], p[1][1], p[1][2], p[2][1], p[2][2], B.h[1], B.h[2])) return false;
        if (body_edge_separates(e[j][2], -e[j][0], p[0][0], p[0][2], p[1][0], p[1][2], p[2][0], p[2][2], B.h[0], B.h[2])) return false;
        if (body_edge_separates(-e[j][1], e[j][0], p[0][0], p[0][1], p[1][0], p[1][1], p[2][0], p[2][1], B.h[0], B.h[1])) return false;
    }
    return true;
}

// the closed box-cell test of the rule (15 axes, in the box's frame): m the cell's centre (world), s its half-width
__device__ __forceinline__ bool body_cell_overlaps(const BodyBox& B, const double m[3], double s) {
    double t[3];
    body_to_frame(B, m, t);
    double A[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int a = 0; a < 3; a++) A[i][a] = fabs(B.R[i][a]);
    // the box's axes
#pragma unroll
    for (int a = 0; a < 3; a++)
        if (fabs(t[a]) > B.h[a] + s * ((A[0][a] + A[1][a]) + A[2][a])) return false;
    // the cell's axes: row i of R in the box's frame
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double q = (B.R[i][0] * t[0] + B.R[i][1] * t[1]) + B.R[i][2] * t[2];
        if (fabs(q) > ((B.h[0] * A[i][0] + B.h[1] * A[i][1]) + B.h[2] * A[i][2]) + s) return false;
    }
    // u_a x (row i): for a = 0 (0, -R_i2, R_i1), a = 1 (R_i2, 0, -R_i0), a = 2 (-R_i1, R_i0, 0); b, c the other two box axes
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int j = (i + 1) % 3, k = (i + 2) % 3;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const int b = (a + 1) % 3, c = (a + 2) % 3;
            const double p = B.R[i][b] * t[c] - B.R[i][c] * t[b];
            const double r = (B.h[b] * A[i][c] + B.h[c] * A[i][b]) + s * (A[j][a] + A[k][a]);
            if (fabs(p) > r) return false;
        }
    }
    return true;
}

// float32 not above / not below x
__device__ __forceinline__ float body_f32_down(double x) {
    const float f = (float)x;
    return (double)f > x ? nextafterf(f, -INFINITY) : f;
}
__device__ __forceinline__ float body_f32_up(double x) {
    const float f = (float)x;
    return (double)f < x ? nextafterf(f, INFINITY) : f;
}

struct BodyPerm {
    int32_t axis[3], sign[3];
};

__global__ void __launch_bounds__(kBodyBlock) k_box_mesh(const double* __restrict__ boxes, uint32_t N, ngp_raycast_grid G,
                                                         const int32_t* __restrict__ cell_start, const int32_t* __restrict__ pair_tri, uint32_t P,
                                                         const float4* __restrict__ tri_verts, uint32_t F, BodyPerm M,
                                                         int32_t* __restrict__ out_prim) {
    const uint32_t b = blockIdx.x * (kBodyBlock / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= N) return;                                  // (whole waves leave together)
    const BodyBox B = body_load(boxes, b);
    int32_t best = kBodyNone;
    if (B.valid) {
        // the box's bounds in the mesh's axes, float32, outward, grown; then the grid's cells (the header's superset argument)
        int32_t c0[3], c1[3];
        bool some = true;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const double E = body_extent(B, a);
            const double wlo = B.c[a] - E, whi = B.c[a] + E;
            const float lo = body_f32_down(M.sign[a] < 0 ? -whi : wlo), hi = body_f32_up(M.sign[a] < 0 ? -wlo : whi);
#pragma unroll
            for (int m = 0; m < 3; m++) {                // (M.axis[a] == m for exactly one m: constant indices only)
                if (M.axis[a] == m) {
                    const float top = (float)(G.n[m] - 1);
                    const float v0 = floorf(((lo - G.grow[m]) - G.lo[m]) * G.inv_cell[m]), v1 = floorf(((hi + G.grow[m]) - G.lo[m]) * G.inv_cell[m]);
                    if (v1 < 0.0f || v0 > top) some = false;
                    c0[m] = v0 >= 1.0f ? (int32_t)fminf(v0, top) : 0;              // (NaN: the whole axis)
                    c1[m] = v1 <= top - 1.0f ? (int32_t)fmaxf(v1, 0.0f) : (int32_t)G.n[m] - 1;
                }
            }
        }
        if (some) {
            for (int32_t x = c0[0]; x <= c1[0]; x++) {
                for (int32_t y = c0[1]; y <= c1[1]; y++) {
                    const uint32_t row = ((uint32_t)x * G.n[1] + (uint32_t)y) * G.n[2];
                    const uint32_t k0 = min((uint32_t)cell_start[row + (uint32_t)c0[2]], P), k1 = min((uint32_t)cell_start[row + (uint32_t)c1[2] + 1], P);
                    for (uint32_t k = k0 + lane; k < k1; k += 64) {
                        const uint32_t f = (uint32_t)pair_tri[k];
                        if (f >= F || (int32_t)f >= best) continue;
                        const Tri T = load_tri(tri_verts, f);                      // (v0, v1, v2 under load_tri's names)
                        const float v[3][3] = {{T.v0x, T.v0y, T.v0z}, {T.e1x, T.e1y, T.e1z}, {T.e2x, T.e2y, T.e2z}};
                        double w[3][3];
#pragma unroll
                        for (int q = 0; q < 3; q++)
#pragma unroll
                            for (int a = 0; a < 3; a++) {
                                const float s = M.axis[a] == 0 ? v[q][0] : (M.axis[a] == 1 ? v[q][1] : v[q][2]);
                                w[q][a] = (double)(M.sign[a] < 0 ? -s : s);
                            }
                        if (body_tri_overlaps(B, w)) best = (int32_t)f;
                    }
                }
            }
        }
    }
    best = wave_min(best);
    if (lane == 0) out_prim[b] = best == kBodyNone ? -1 : best;
}

__global__ void __launch_bounds__(kBodyBlock) k_box_cells(const uint8_t* __restrict__ map, ngp_voxel_box V, const double* __restrict__ boxes,
                                                          uint32_t N, int32_t* __restrict__ out_cell) {
    const uint32_t b = blockIdx.x * (kBodyBlock / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= N) return;                                  // (whole waves leave together)
    const BodyBox B = body_load(boxes, b);
    int32_t best = kBodyNone;
    if (B.valid) {
        uint32_t lo[3], n[3];
        bool some = true;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const double E = body_extent(B, a);
            const double top = (double)(V.shape[a] - 1);
            const double l = floor(((B.c[a] - E) - V.start[a]) * V.granularity) - 1.0, h = floor(((B.c[a] + E) - V.start[a]) * V.granularity) + 1.0;
            if (h < 0.0 || l > top) some = false;
            lo[a] = l >= 1.0 ? (uint32_t)fmin(l, top) : 0u;                        // (NaN: the whole axis)
            const uint32_t hi = h <= top - 1.0 ? (uint32_t)fmax(h, 0.0) : V.shape[a] - 1;
            n[a] = hi >= lo[a] ? hi - lo[a] + 1 : 0;
        }
        const uint32_t total = some ? n[0] * n[1] * n[2] : 0;                      // <= X Y Z < 2^31
        const uint32_t nyz = n[1] * n[2];
        const double s = 0.5 / V.granularity;
        for (uint32_t base = 0; base < total; base += 64) {
            const uint32_t j = base + lane;
            if (j < total) {
                const uint32_t ix = lo[0] + j / nyz, iy = lo[1] + (j % nyz) / n[2], iz = lo[2] + j % n[2];
                const uint32_t cell = (ix * V.shape[1] + iy) * V.shape[2] + iz;
                if (map[cell]) {
                    const double m[3] = {V.start[0] + ((double)ix + 0.5) / V.granularity, V.start[1] + ((double)iy + 0.5) / V.granularity,
                                         V.start[2] + ((double)iz + 0.5) / V.granularity};
                    if (body_cell_overlaps(B, m, s)) best = (int32_t)cell;
                }
            }
            best = wave_min(best);                       // (every lane of the wave is here: the loop's bounds are the wave's)
            if (best != kBodyNone) break;
        }
    }
    if (lane == 0) out_cell[b] = best == kBodyNone ? -1 : best;
}

}  // namespace ngp

using namespace ngp;

extern "C" {

int ngp_box_mesh_overlap(const double* boxes, uint64_t N, const ngp_raycast_grid* grid, const int32_t* cell_start, const int32_t* pair_tri,
                         uint64_t P, const float* tri_verts, uint32_t F, const int32_t* axis3_host, const int32_t* sign3_host, int32_t* prim,
                         ngp_stream_t stream) {
    int rc = cast_check_grid("box_mesh_overlap", grid);
    if (rc) return rc;
    NGP_REQUIRE(N < ((uint64_t)1 << 31), "box_mesh_overlap: N must be < 2^31 (got %llu)", (unsigned long long)N);
    NGP_REQUIRE(F >= 1 && F < (1u << 31), "box_mesh_overlap: 1 <= F < 2^31 (got %u)", F);
    NGP_REQUIRE(P >= 1 && P < ((uint64_t)1 << 31), "box_mesh_overlap: 1 <= pairs < 2^31 (got %llu)", (unsigned long long)P);
    NGP_REQUIRE(axis3_host && sign3_host, "box_mesh_overlap: null permutation");
    BodyPerm M;
    uint32_t seen = 0;
    for (int a = 0; a < 3; a++) {
        M.axis[a] = axis3_host[a];
        M.sign[a] = sign3_host[a];
        NGP_REQUIRE(M.axis[a] >= 0 && M.axis[a] <= 2 && (M.sign[a] == 1 || M.sign[a] == -1),
                    "box_mesh_overlap: world axis %d must be plus or minus one of the mesh's axes", a);
        seen |= 1u << M.axis[a];
    }
    NGP_REQUIRE(seen == 7u, "box_mesh_overlap: the three world axes must take three different axes of the mesh");
    if (N == 0) return NGP_OK;
    NGP_REQUIRE(boxes && cell_start && pair_tri && tri_verts && prim, "box_mesh_overlap: null pointer");
    NGP_REQUIRE(((uintptr_t)tri_verts & 15) == 0 && ((uintptr_t)boxes & 7) == 0, "box_mesh_overlap: tri_verts must be 16-byte, boxes 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("box_mesh_overlap", s, (double)N);
    k_box_mesh<<<div_up((uint32_t)N, kBodyBlock / 64), kBodyBlock, 0, s>>>(boxes, (uint32_t)N, *grid, cell_start, pair_tri, (uint32_t)P,
                                                                          reinterpret_cast<const float4*>(tri_verts), F, M, prim);
    return check_launch("box_mesh_overlap");
}

int ngp_box_cells_overlap(const uint8_t* map, const ngp_voxel_box* box, const double* boxes, uint64_t N, int32_t* cell, ngp_stream_t stream) {
    NGP_REQUIRE(box, "box_cells_overlap: null box");
    NGP_REQUIRE(box->granularity > 0.0 && box->granularity <= 1.7e308, "box_cells_overlap: the granularity must be positive and finite");
    for (int a = 0; a < 3; a++) {
        NGP_REQUIRE(box->start[a] - box->start[a] == 0.0, "box_cells_overlap: the map's start must be finite");
        NGP_REQUIRE(box->shape[a] >= 1, "box_cells_overlap: every axis of the map has at least one cell");
    }
    NGP_REQUIRE((uint64_t)box->shape[0] * box->shape[1] * box->shape[2] < ((uint64_t)1 << 31), "box_cells_overlap: X * Y * Z must be < 2^31");
    NGP_REQUIRE(N < ((uint64_t)1 << 31), "box_cells_overlap: N must be < 2^31 (got %llu)", (unsigned long long)N);
    if (N == 0) return NGP_OK;
    NGP_REQUIRE(map && boxes && cell, "box_cells_overlap: null pointer");
    NGP_REQUIRE(((uintptr_t)boxes & 7) == 0, "box_cells_overlap: boxes must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("box_cells_overlap", s, (double)N);
    k_box_cells<<<div_up((uint32_t)N, kBodyBlock / 64), kBodyBlock, 0, s>>>(map, *box, boxes, (uint32_t)N, cell);
    return check_launch("box_cells_overlap");
}

}  // extern "C"
