// voxelize.hip -- the world's triangle mesh as a collision map (nerfsafetyvalidation_amd/world.py, MeshWorld.occupancy): the truth a
// rollout's collisions are judged against, in the place of the reference's validation/utils/createCollisionMap.py.  That script marks
// the cells that hold a mesh VERTEX; this unit marks every cell a TRIANGLE touches (a conservative surface voxelisation), so a
// triangle larger than a cell leaves no hole.
//
// The voxelisation rule -- the signed permutation into the world frame, the 13-axis separating test, the vertex cells, the candidate
// cells -- is world.py's docstring ("The voxelisation rule"); vox_overlaps and vox_range are that text in float64 with one IEEE rounding
// per operation, in its order (this unit is compiled with -ffp-contract=off and holds no fma).  The zero component of an axis u_i x e_j
// drops out of both of its sums exactly, so they are written as the two-term sums they are.
//
// Work is split by (face, candidate cell) pair, not by face -- one face spanning the box does not serialise on a lane:
//   k_voxel_count   one lane per face: its number of candidates; marks its vertices' cells
//   (caller)        inclusive scan of the counts (int64), the total P read back
//   k_voxel_mark    one lane per pair: finds its face in the scanned counts (binary search), its cell in the face's candidate
//                   range (C order), runs the test and stores the byte 1 on overlap
// No atomics: the only writes to the map are byte stores of the constant 1 (several lanes may store it to one cell), after a
// hipMemsetAsync of the whole map on the same stream.
#include "ngp_common.hpp"

namespace ngp {

constexpr uint32_t kVoxBlock = 256;

__device__ __forceinline__ float pick3(float x, float y, float z, int32_t axis) { return axis == 0 ? x : (axis == 1 ? y : z); }

struct VoxTri {
    double v[3][3];      // world vertices [k][a]; indexed by constants only (fully unrolled loops): registers, not scratch
};

// vertex `i` in the world frame: a copy or a negation per axis, then float64
__device__ __forceinline__ void vox_world(const float* __restrict__ vertices, uint32_t i, const ngp_voxel_box& B, double w[3]) {
    const float x = vertices[3 * (size_t)i], y = vertices[3 * (size_t)i + 1], z = vertices[3 * (size_t)i + 2];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float c = pick3(x, y, z, B.axis[a]);
        w[a] = (double)(B.sign[a] < 0 ? -c : c);
    }
}

// the face's vertices; false when an index is outside the V vertices (the face then has no candidates and marks nothing)
__device__ __forceinline__ bool vox_load(const float* __restrict__ vertices, uint32_t V, const int32_t* __restrict__ faces, uint32_t f,
                                         const ngp_voxel_box& B, VoxTri& T) {
    const uint32_t i0 = (uint32_t)faces[3 * (size_t)f], i1 = (uint32_t)faces[3 * (size_t)f + 1], i2 = (uint32_t)faces[3 * (size_t)f + 2];
    if (i0 >= V || i1 >= V || i2 >= V) return false;
    vox_world(vertices, i0, B, T.v[0]);
    vox_world(vertices, i1, B, T.v[1]);
    vox_world(vertices, i2, B, T.v[2]);
    return true;
}

struct VoxRange {
    uint32_t lo[3], n[3];      // first candidate cell and the number of them per axis (n == 0: none)
};

__device__ __forceinline__ VoxRange vox_range(const VoxTri& T, const ngp_voxel_box& B) {
    VoxRange R;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double mn = fmin(T.v[0][a], fmin(T.v[1][a], T.v[2][a])), mx = fmax(T.v[0][a], fmax(T.v[1][a], T.v[2][a]));
        const double top = (double)(B.shape[a] - 1);
        const double lo = floor((mn - B.start[a]) * B.granularity) - 1.0, hi = floor((mx - B.start[a]) * B.granularity) + 1.0;
        if (hi >= 0.0 && lo <= top) {
            const uint32_t l = (uint32_t)fmax(lo, 0.0), h = (uint32_t)fmin(hi, top);
            R.lo[a] = l;
            R.n[a] = h - l + 1;
        } else {
            R.lo[a] = 0;
            R.n[a] = 0;
        }
    }
    return R;
}

// one of the nine axes u_i x e_j, reduced to its two non-zero components (a1, a2) and the matching components of the shifted vertices
__device__ __forceinline__ bool vox_edge_separates(double a1, double a2, double p0c1, double p0c2, double p1c1, double p1c2, double p2c1,
                                                   double p2c2, double h) {
    const double p0 = a1 * p0c1 + a2 * p0c2, p1 = a1 * p1c1 + a2 * p1c2, p2 = a1 * p2c1 + a2 * p2c2;
    const double r = h * (fabs(a1) + fabs(a2));
    return fmin(p0, fmin(p1, p2)) > r || fmax(p0, fmax(p1, p2)) < -r;
}

// the closed triangle-box test of the rule: true when no axis separates the face from the cell of centre c, half-width h
__device__ __forceinline__ bool vox_overlaps(const VoxTri& T, double cx, double cy, double cz, double h) {
    const double c[3] = {cx, cy, cz};
    double p[3][3];
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int a = 0; a < 3; a++) p[k][a] = T.v[k][a] - c[a];
#pragma unroll
    for (int a = 0; a < 3; a++)
        if (fmin(p[0][a], fmin(p[1][a], p[2][a])) > h || fmax(p[0][a], fmax(p[1][a], p[2][a])) < -h) return false;
    double e[3][3];      // e0 = v1 - v0, e1 = v2 - v1, e2 = v0 - v2
#pragma unroll
    for (int a = 0; a < 3; a++) {
        e[0][a] = T.v[1][a] - T.v[0][a];
        e[1][a] = T.v[2][a] - T.v[1][a];
        e[2][a] = T.v[0][a] - T.v[2][a];
    }
    const double nx = e[0][1] * e[1][2] - e[0][2] * e[1][1], ny = e[0][2] * e[1][0] - e[0][0] * e[1][2], nz = e[0][0] * e[1][1] - e[0][1] * e[1][0];
    const double d = (nx * p[0][0] + ny * p[0][1]) + nz * p[0][2];
    if (fabs(d) > h * ((fabs(nx) + fabs(ny)) + fabs(nz))) return false;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        // u_0 x e = (0, -ez, ey);  u_1 x e = (ez, 0, -ex);  u_2 x e = (-ey, ex, 0)
        if (vox_edge_separates(-e[j][2], e[j][1], p[0][1], p[0][2], p[1][1], p[1][2], p[2][1], p[2][2], h)) return false;
        if (vox_edge_separates(e[j][2], -e[j][0], p[0][0], p[0][2], p[1][0], p[1][2], p[2][0], p[2][2], h)) return false;
        if (vox_edge_separates(-e[j][1], e[j][0], p[0][0], p[0][1], p[1][0], p[1][1], p[2][0], p[2][1], h)) return false;
    }
    return true;
}

__global__ void __launch_bounds__(kVoxBlock) k_voxel_count(const float* __restrict__ vertices, uint32_t V, const int32_t* __restrict__ faces,
                                                           uint32_t F, ngp_voxel_box B, uint8_t* __restrict__ map,
                                                           int32_t* __restrict__ counts) {
    const uint32_t f = blockIdx.x * kVoxBlock + threadIdx.x;
    if (f >= F) return;
    VoxTri T;
    if (!vox_load(vertices, V, faces, f, B, T)) {
        counts[f] = 0;
        return;
    }
    const VoxRange R = vox_range(T, B);
    counts[f] = (int32_t)(R.n[0] * R.n[1] * R.n[2]);      // <= X Y Z < 2^31
    // rule (b): the cells of the vertices, GridBox.indices' floor
#pragma unroll
    for (int k = 0; k < 3; k++) {
        double idx[3];
        bool inside = true;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            idx[a] = floor((T.v[k][a] - B.start[a]) * B.granularity);
            inside = inside && idx[a] >= 0.0 && idx[a] <= (double)(B.shape[a] - 1);
        }
        if (inside) map[((size_t)(uint32_t)idx[0] * B.shape[1] + (uint32_t)idx[1]) * B.shape[2] + (uint32_t)idx[2]] = 1;
    }
}

__global__ void __launch_bounds__(kVoxBlock) k_voxel_mark(const float* __restrict__ vertices, uint32_t V, const int32_t* __restrict__ faces,
                                                          uint32_t F, ngp_voxel_box B, const int64_t* __restrict__ ends, int64_t pair_base,
                                                          uint32_t n_pairs, uint8_t* __restrict__ map) {
    const uint32_t t = blockIdx.x * kVoxBlock + threadIdx.x;
    if (t >= n_pairs) return;
    const int64_t pair = pair_base + (int64_t)t;
    // the face of this pair: the first f with ends[f] > pair (faces without candidates are never found)
    uint32_t lo = 0, hi = F - 1;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (ends[mid] > pair) hi = mid;
        else lo = mid + 1;
    }
    const uint32_t f = lo;
    const int64_t first = f ? ends[f - 1] : 0;
    if (pair < first || pair >= ends[f]) return;           // (the caller's scan does not describe this pair: write nothing)
    VoxTri T;
    if (!vox_load(vertices, V, faces, f, B, T)) return;
    const VoxRange R = vox_range(T, B);
    const uint64_t j = (uint64_t)(pair - first);
    if (j >= (uint64_t)R.n[0] * R.n[1] * R.n[2]) return;   // (nor do these counts: every cell index below is inside the box)
    const uint32_t jj = (uint32_t)j, nyz = R.n[1] * R.n[2];
    const uint32_t ix = R.lo[0] + jj / nyz, iy = R.lo[1] + (jj % nyz) / R.n[2], iz = R.lo[2] + jj % R.n[2];
    const double cx = B.start[0] + ((double)ix + 0.5) / B.granularity, cy = B.start[1] + ((double)iy + 0.5) / B.granularity,
                 cz = B.start[2] + ((double)iz + 0.5) / B.granularity;
    if (vox_overlaps(T, cx, cy, cz, 0.5 / B.granularity)) map[((size_t)ix * B.shape[1] + iy) * B.shape[2] + iz] = 1;
}

static int vox_check(const char* what, const ngp_voxel_box* B, uint32_t V, uint32_t F) {
    NGP_REQUIRE(B, "%s: null box", what);
    NGP_REQUIRE(B->granularity > 0.0 && B->granularity <= 1.7e308, "%s: the granularity must be positive and finite", what);
    uint32_t seen = 0;
    for (int a = 0; a < 3; a++) {
        NGP_REQUIRE(B->start[a] - B->start[a] == 0.0, "%s: the box's start must be finite", what);
        NGP_REQUIRE(B->shape[a] >= 1, "%s: every axis of the box has at least one cell", what);
        NGP_REQUIRE(B->axis[a] >= 0 && B->axis[a] <= 2 && (B->sign[a] == 1 || B->sign[a] == -1),
                    "%s: world axis %d must be plus or minus one of the mesh's axes", what, a);
        seen |= 1u << B->axis[a];
    }
    NGP_REQUIRE(seen == 7u, "%s: the three world axes must take three different axes of the mesh", what);
    NGP_REQUIRE((uint64_t)B->shape[0] * B->shape[1] * B->shape[2] < ((uint64_t)1 << 31), "%s: X * Y * Z must be < 2^31", what);
    NGP_REQUIRE(V >= 1 && V < (1u << 31) && F >= 1 && F < (1u << 31), "%s: 1 <= V, F < 2^31 (got %u, %u)", what, V, F);
    return NGP_OK;
}

}  // namespace ngp

using namespace ngp;

extern "C" {

int ngp_voxelize_count(const float* vertices, uint32_t V, const int32_t* faces, uint32_t F, const ngp_voxel_box* box, uint8_t* map,
                       int32_t* counts, ngp_stream_t stream) {
    int rc = vox_check("voxelize_count", box, V, F);
    if (rc) return rc;
    NGP_REQUIRE(vertices && faces && map && counts, "voxelize_count: null pointer");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("voxelize_count", s, (double)F);
    const size_t cells = (size_t)box->shape[0] * box->shape[1] * box->shape[2];
    if (hipMemsetAsync(map, 0, cells, s) != hipSuccess) return check_launch("voxelize_count (memset)");
    k_voxel_count<<<div_up(F, kVoxBlock), kVoxBlock, 0, s>>>(vertices, V, faces, F, *box, map, counts);
    return check_launch("voxelize_count");
}

int ngp_voxelize_mark(const float* vertices, uint32_t V, const int32_t* faces, uint32_t F, const ngp_voxel_box* box, const int64_t* ends,
                      uint64_t pair_base, uint64_t n_pairs, uint8_t* map, ngp_stream_t stream) {
    int rc = vox_check("voxelize_mark", box, V, F);
    if (rc) return rc;
    NGP_REQUIRE(n_pairs < ((uint64_t)1 << 31), "voxelize_mark: at most 2^31 - 1 pairs per call (got %llu)", (unsigned long long)n_pairs);
    NGP_REQUIRE(pair_base < ((uint64_t)1 << 62), "voxelize_mark: pair_base must be < 2^62");
    if (n_pairs == 0) return NGP_OK;
    NGP_REQUIRE(vertices && faces && ends && map, "voxelize_mark: null pointer");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("voxelize_mark", s, (double)n_pairs);
    k_voxel_mark<<<div_up((uint32_t)n_pairs, kVoxBlock), kVoxBlock, 0, s>>>(vertices, V, faces, F, *box, ends, (int64_t)pair_base,
                                                                            (uint32_t)n_pairs, map);
    return check_launch("voxelize_mark");
}

}  // extern "C"
