// mesh.hip -- the isosurface of a scalar lattice as an indexed triangle mesh (nerfsafetyvalidation_amd/mesh.py): the device form of
// the step the reference leaves to mcubes in extract_geometry (nerf/utils.py:170-182), by marching tetrahedra on the Kuhn split.
//
// Rule (DESIGN.md "Mesh export"; mesh.py's numpy path is the same rule in the same order):
//   * a lattice point of the C-order field u [X,Y,Z] is INSIDE iff u > threshold (strict; NaN is outside);
//   * every cell is cut into the six tetrahedra around its (0,0,0)-(1,1,1) diagonal: for the permutation (a,b,c) of the axes, in
//     lexicographic order, tetrahedron k is { corner, +e_a, +e_a+e_b, +(1,1,1) }.  Corner offsets are 3-bit codes, bit 0 = x,
//     bit 1 = y, bit 2 = z;
//   * the edges of those tetrahedra are the 7 lattice edges with offset in {0,1}^3 \ 0, owned by their lower end:
//     type 0..6 = +x, +y, +z, +xy, +xz, +yz, +xyz.  An edge whose ends differ carries ONE vertex, at
//     t = (thr - ua) / (ub - ua), v = pa + t * (pb - pa) (a the owner; fp32, one IEEE operation per step);
//   * vertices are ordered by (owner in C order, type), faces by (cell in C order, tetrahedron, triangle); normals point from
//     inside to outside.
//
// Kernels (one thread per lattice point, z fastest, so every load of a wave is a run of one row):
//   k_iso_flags   u -> one inside byte per point (each point is classified once)
//   k_iso_count   the 7-bit mask of crossing edges a point owns and the triangle count of the cell it is the corner of, from the
//                 flag bytes of its 8 cell corners (four coalesced rows, the +z neighbour the same row shifted by one: the re-reads
//                 are L1/L2 hits).  The block-exclusive prefixes of both counts -- ballot + popcount per bit plane inside a
//                 wave64, wave totals through LDS -- go out as uint16 next to the counts, the block totals as uint64.
//   k_iso_scan    one workgroup turns the block totals into exclusive block offsets (64-bit) and the grand totals V, F: a second
//                 launch, no workgroup waits for another, no atomics.
//   k_iso_emit    vertices [V,3] fp32 and faces [F,3] int32: a vertex id is its owner's offset (block offset + prefix) plus the
//                 popcount of the owner's mask below the edge's bit.
//
// The 16-case tetrahedron table is derived at compile time (make_iso_tables) from the geometry itself: the cut of a tetrahedron
// with corners at their lattice offsets and crossings at edge midpoints, each triangle turned so that its normal has a positive
// component from the inside corners' centroid to the outside corners'.  Nothing is typed in.
#include "ngp_common.hpp"

namespace ngp {

constexpr uint32_t kIsoBlock = 256;          // points per workgroup of k_iso_count / k_iso_emit: the granule of the block offsets
constexpr uint32_t kIsoScanBlock = 1024;

struct IsoTables {
    uint8_t tet[6][4];        // corner offset codes of tetrahedron k's four vertices
    uint8_t ntri[16];         // triangles of a case (bit i = vertex i inside)
    uint8_t tri[6][16][6];    // up to two triangles x three vertices: (owner corner code) | (edge type << 3)
    uint8_t type_of[8];       // edge type of an offset code
    uint8_t off_of[8];        // offset code of an edge type (entry 7 unused)
};

constexpr IsoTables make_iso_tables() {
    IsoTables T{};
    // type 0..6 = +x, +y, +z, +xy, +xz, +yz, +xyz  <->  offset codes 1, 2, 4, 3, 5, 6, 7
    const uint8_t off_of[7] = {1, 2, 4, 3, 5, 6, 7};
    for (int t = 0; t < 7; t++) {
        T.off_of[t] = off_of[t];
        T.type_of[off_of[t]] = (uint8_t)t;
    }
    const int perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    for (int c = 0; c < 16; c++) {
        const int n = (c & 1) + ((c >> 1) & 1) + ((c >> 2) & 1) + ((c >> 3) & 1);
        T.ntri[c] = (uint8_t)(n == 2 ? 2 : (n == 1 || n == 3) ? 1 : 0);
    }
    for (int k = 0; k < 6; k++) {
        const int a = perms[k][0], b = perms[k][1];
        T.tet[k][0] = 0;
        T.tet[k][1] = (uint8_t)(1 << a);
        T.tet[k][2] = (uint8_t)((1 << a) | (1 << b));
        T.tet[k][3] = 7;
        int P[4][3] = {};
        for (int i = 0; i < 4; i++)
            for (int d = 0; d < 3; d++) P[i][d] = (T.tet[k][i] >> d) & 1;
        for (int c = 1; c < 15; c++) {
            int in[4] = {}, out[4] = {}, n_in = 0, n_out = 0;
            for (int i = 0; i < 4; i++) {
                if ((c >> i) & 1) in[n_in++] = i;
                else out[n_out++] = i;
            }
            // cut edges (pairs of tetrahedron vertices) in a fixed order, then the orientation test
            int e[6][2] = {};      // up to 2 triangles x 3 vertices
            int nt = 1;
            if (n_in == 1) {
                for (int j = 0; j < 3; j++) { e[j][0] = in[0]; e[j][1] = out[j]; }
            } else if (n_in == 3) {
                for (int j = 0; j < 3; j++) { e[j][0] = out[0]; e[j][1] = in[j]; }
            } else {
                // the quad (i0 o0) (i0 o1) (i1 o1) (i1 o0), cut along (i0 o0)-(i1 o1)
                nt = 2;
                e[0][0] = in[0]; e[0][1] = out[0];
                e[1][0] = in[0]; e[1][1] = out[1];
                e[2][0] = in[1]; e[2][1] = out[1];
                e[3][0] = in[0]; e[3][1] = out[0];
                e[4][0] = in[1]; e[4][1] = out[1];
                e[5][0] = in[1]; e[5][1] = out[0];
            }
            // n_in * sum(outside corners) - n_out * sum(inside corners): the inside -> outside direction, scaled
            int dir[3] = {};
            for (int d = 0; d < 3; d++) {
                int so = 0, si = 0;
                for (int i = 0; i < n_out; i++) so += P[out[i]][d];
                for (int i = 0; i < n_in; i++) si += P[in[i]][d];
                dir[d] = n_in * so - n_out * si;
            }
            for (int t = 0; t < nt; t++) {
                int m[3][3] = {};   // twice the edge midpoints
                for (int j = 0; j < 3; j++)
                    for (int d = 0; d < 3; d++) m[j][d] = P[e[3 * t + j][0]][d] + P[e[3 * t + j][1]][d];
                int p[3] = {}, q[3] = {};
                for (int d = 0; d < 3; d++) { p[d] = m[1][d] - m[0][d]; q[d] = m[2][d] - m[0][d]; }
                const int nx = p[1] * q[2] - p[2] * q[1], ny = p[2] * q[0] - p[0] * q[2], nz = p[0] * q[1] - p[1] * q[0];
                if (nx * dir[0] + ny * dir[1] + nz * dir[2] < 0) {
                    const int s0 = e[3 * t + 1][0], s1 = e[3 * t + 1][1];
                    e[3 * t + 1][0] = e[3 * t + 2][0]; e[3 * t + 1][1] = e[3 * t + 2][1];
                    e[3 * t + 2][0] = s0; e[3 * t + 2][1] = s1;
                }
                for (int j = 0; j < 3; j++) {
                    // the tetrahedron's corner codes form a chain under inclusion: the lower end of an edge is the AND of its ends
                    const int oa = T.tet[k][e[3 * t + j][0]], ob = T.tet[k][e[3 * t + j][1]];
                    T.tri[k][c][3 * t + j] = (uint8_t)((oa & ob) | (T.type_of[oa ^ ob] << 3));
                }
            }
        }
    }
    return T;
}

__constant__ IsoTables c_iso = make_iso_tables();

struct IsoDims {
    uint32_t X, Y, Z, N, YZ;
};

__device__ __forceinline__ uint32_t iso_flat_offset(uint32_t code, const IsoDims& D) {
    return (code & 1u) * D.YZ + ((code >> 1) & 1u) * D.Z + ((code >> 2) & 1u);
}

// exclusive prefix over the lanes of a wave64 of a value below 2^BITS, one ballot per bit plane; `total` = the wave's sum
template <int BITS>
__device__ __forceinline__ uint32_t iso_wave_prefix(uint32_t v, uint32_t& total) {
    const unsigned long long below = (1ull << (threadIdx.x & 63u)) - 1ull;
    uint32_t pre = 0, tot = 0;
#pragma unroll
    for (int b = 0; b < BITS; b++) {
        const unsigned long long m = __ballot((v >> b) & 1u);
        pre += (uint32_t)__popcll(m & below) << b;
        tot += (uint32_t)__popcll(m) << b;
    }
    total = tot;
    return pre;
}

// block-exclusive prefixes of two per-thread counts (BLOCK / 64 waves, totals through LDS); every thread of the block must call it
template <int BITS_A, int BITS_B, uint32_t BLOCK>
__device__ __forceinline__ void iso_block_prefix(uint32_t a, uint32_t b, uint32_t& pre_a, uint32_t& pre_b, uint32_t& tot_a, uint32_t& tot_b) {
    constexpr uint32_t kWaves = BLOCK / 64;
    __shared__ uint32_t s_tot[2][kWaves];
    uint32_t wa, wb;
    pre_a = iso_wave_prefix<BITS_A>(a, wa);
    pre_b = iso_wave_prefix<BITS_B>(b, wb);
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) {
        s_tot[0][wave] = wa;
        s_tot[1][wave] = wb;
    }
    __syncthreads();
    tot_a = 0;
    tot_b = 0;
    for (uint32_t w = 0; w < kWaves; w++) {
        const uint32_t ta = s_tot[0][w], tb = s_tot[1][w];
        if (w < wave) { pre_a += ta; pre_b += tb; }
        tot_a += ta;
        tot_b += tb;
    }
    __syncthreads();          // s_tot may be written again by the caller's next round
}

__global__ void __launch_bounds__(kIsoBlock) k_iso_flags(const float* __restrict__ u, uint32_t N, float thr, uint8_t* __restrict__ flags) {
    const uint32_t p = blockIdx.x * kIsoBlock + threadIdx.x;
    if (p < N) flags[p] = u[p] > thr ? 1 : 0;
}

// corner configuration of the cell whose low corner is p (bit o = corner with offset code o inside); the cell must exist
__device__ __forceinline__ uint32_t iso_cell_config(const uint8_t* __restrict__ flags, uint32_t p, const IsoDims& D) {
    uint32_t cfg = 0;
#pragma unroll
    for (uint32_t o = 0; o < 8; o++) cfg |= (uint32_t)flags[p + iso_flat_offset(o, D)] << o;
    return cfg;
}

__device__ __forceinline__ uint32_t iso_tet_case(uint32_t cfg, int k) {
    return ((cfg >> c_iso.tet[k][0]) & 1u) | (((cfg >> c_iso.tet[k][1]) & 1u) << 1) | (((cfg >> c_iso.tet[k][2]) & 1u) << 2) |
           (((cfg >> c_iso.tet[k][3]) & 1u) << 3);
}

__global__ void __launch_bounds__(kIsoBlock) k_iso_count(const uint8_t* __restrict__ flags, IsoDims D, uint8_t* __restrict__ mask_out,
                                                         uint8_t* __restrict__ ntri_out, uint16_t* __restrict__ vpre, uint16_t* __restrict__ fpre,
                                                         unsigned long long* __restrict__ block_tot) {
    const uint32_t p = blockIdx.x * kIsoBlock + threadIdx.x;
    uint32_t mask = 0, nt = 0;
    if (p < D.N) {
        const uint32_t z = p % D.Z, y = (p / D.Z) % D.Y, x = p / D.YZ;
        const bool hx = x + 1 < D.X, hy = y + 1 < D.Y, hz = z + 1 < D.Z;
        const uint32_t f0 = flags[p];
#pragma unroll
        for (uint32_t t = 0; t < 7; t++) {
            const uint32_t o = c_iso.off_of[t];
            const bool exists = (hx || !(o & 1u)) && (hy || !(o & 2u)) && (hz || !(o & 4u));
            if (exists && flags[p + iso_flat_offset(o, D)] != f0) mask |= 1u << t;
        }
        if (hx && hy && hz) {
            const uint32_t cfg = iso_cell_config(flags, p, D);
            if (cfg != 0 && cfg != 255) {
#pragma unroll
                for (int k = 0; k < 6; k++) nt += c_iso.ntri[iso_tet_case(cfg, k)];
            }
        }
        mask_out[p] = (uint8_t)mask;
        ntri_out[p] = (uint8_t)nt;
    }
    uint32_t pv, pf, tv, tf;
    iso_block_prefix<3, 4, kIsoBlock>((uint32_t)__popc(mask), nt, pv, pf, tv, tf);     // <= 7 vertices, <= 12 triangles per point
    if (p < D.N) {
        vpre[p] = (uint16_t)pv;       // <= 255 * 7
        fpre[p] = (uint16_t)pf;       // <= 255 * 12
    }
    if (threadIdx.x == 0) {
        block_tot[2 * (size_t)blockIdx.x] = tv;
        block_tot[2 * (size_t)blockIdx.x + 1] = tf;
    }
}

// block totals (<= 256 * 7 and <= 256 * 12) -> exclusive block offsets in place, grand totals to totals[0..1].  One workgroup.
__global__ void __launch_bounds__(kIsoScanBlock) k_iso_scan(unsigned long long* __restrict__ block_tot, uint32_t n_blocks,
                                                            unsigned long long* __restrict__ totals) {
    unsigned long long carry_v = 0, carry_f = 0;
    for (uint32_t b0 = 0; b0 < n_blocks; b0 += kIsoScanBlock) {
        const uint32_t b = b0 + threadIdx.x;
        uint32_t v = 0, f = 0;
        if (b < n_blocks) {
            v = (uint32_t)block_tot[2 * (size_t)b];
            f = (uint32_t)block_tot[2 * (size_t)b + 1];
        }
        uint32_t pv, pf, tv, tf;
        iso_block_prefix<11, 12, kIsoScanBlock>(v, f, pv, pf, tv, tf);
        if (b < n_blocks) {
            block_tot[2 * (size_t)b] = carry_v + pv;
            block_tot[2 * (size_t)b + 1] = carry_f + pf;
        }
        carry_v += tv;
        carry_f += tf;
    }
    if (threadIdx.x == 0) {
        totals[0] = carry_v;
        totals[1] = carry_f;
    }
}

__device__ __forceinline__ uint32_t iso_vertex_id(uint32_t owner, uint32_t type, const uint8_t* __restrict__ mask, const uint16_t* __restrict__ vpre,
                                                  const unsigned long long* __restrict__ block_off) {
    return (uint32_t)block_off[2 * (size_t)(owner / kIsoBlock)] + vpre[owner] + (uint32_t)__popc(mask[owner] & ((1u << type) - 1u));
}

__global__ void __launch_bounds__(kIsoBlock) k_iso_emit(const float* __restrict__ u, const uint8_t* __restrict__ flags, IsoDims D, float thr,
                                                        const uint8_t* __restrict__ mask, const uint8_t* __restrict__ ntri,
                                                        const uint16_t* __restrict__ vpre, const uint16_t* __restrict__ fpre,
                                                        const unsigned long long* __restrict__ block_off, uint32_t V, uint32_t F,
                                                        float* __restrict__ vertices, int32_t* __restrict__ faces) {
    const uint32_t p = blockIdx.x * kIsoBlock + threadIdx.x;
    if (p >= D.N) return;
    // (the existence tests repeat k_iso_count's: a workspace that is not this lattice's must not steer a load past the field)
    const uint32_t z = p % D.Z, y = (p / D.Z) % D.Y, x = p / D.YZ;
    const bool hx = x + 1 < D.X, hy = y + 1 < D.Y, hz = z + 1 < D.Z;
    uint32_t exist = 0;
#pragma unroll
    for (uint32_t t = 0; t < 7; t++) {
        const uint32_t o = c_iso.off_of[t];
        if ((hx || !(o & 1u)) && (hy || !(o & 2u)) && (hz || !(o & 4u))) exist |= 1u << t;
    }
    const uint32_t m = mask[p] & exist;
    if (m) {
        const float fx = (float)x, fy = (float)y, fz = (float)z;
        const float ua = u[p];
        uint32_t id = (uint32_t)block_off[2 * (size_t)blockIdx.x] + vpre[p];
#pragma unroll
        for (uint32_t t = 0; t < 7; t++) {
            if (!((m >> t) & 1u)) continue;
            const uint32_t o = c_iso.off_of[t];
            const float ub = u[p + iso_flat_offset(o, D)];
            const float s = (thr - ua) / (ub - ua);
            if (id < V) {       // (V, F are the caller's: never write past what they describe)
                vertices[3 * (size_t)id + 0] = fx + s * (float)(o & 1u);
                vertices[3 * (size_t)id + 1] = fy + s * (float)((o >> 1) & 1u);
                vertices[3 * (size_t)id + 2] = fz + s * (float)((o >> 2) & 1u);
            }
            id++;
        }
    }
    if (ntri[p] && hx && hy && hz) {
        const uint32_t cfg = iso_cell_config(flags, p, D);
        uint32_t f = (uint32_t)block_off[2 * (size_t)blockIdx.x + 1] + fpre[p];
        for (int k = 0; k < 6; k++) {
            const uint32_t c = iso_tet_case(cfg, k);
            const uint32_t n = c_iso.ntri[c];
            for (uint32_t j = 0; j < n; j++, f++) {
                if (f >= F) continue;
#pragma unroll
                for (uint32_t i = 0; i < 3; i++) {
                    const uint32_t code = c_iso.tri[k][c][3 * j + i];
                    const uint32_t owner = p + iso_flat_offset(code & 7u, D);
                    faces[3 * (size_t)f + i] = (int32_t)iso_vertex_id(owner, code >> 3, mask, vpre, block_off);
                }
            }
        }
    }
}

struct IsoWorkspace {
    unsigned long long* block_tot;     // [n_blocks][2]: totals, then exclusive offsets (vertices, faces)
    uint16_t *vpre, *fpre;             // [N] block-exclusive prefixes
    uint8_t *flags, *mask, *ntri;      // [N]
    uint32_t n_blocks;
};

static IsoWorkspace iso_layout(Carver& c, uint32_t N) {
    IsoWorkspace w;
    w.n_blocks = div_up(N, kIsoBlock);
    w.block_tot = c.take<unsigned long long>((size_t)w.n_blocks * 2);
    w.vpre = c.take<uint16_t>(N, 8);
    w.fpre = c.take<uint16_t>(N, 8);
    w.flags = c.take<uint8_t>(N, 8);
    w.mask = c.take<uint8_t>(N);
    w.ntri = c.take<uint8_t>(N);
    c.pad(64);      // no kernel touches it: kept so that the size stays what it was
    return w;
}

static int iso_check_dims(const char* what, uint32_t X, uint32_t Y, uint32_t Z) {
    NGP_REQUIRE(X >= 2 && Y >= 2 && Z >= 2, "%s: every axis needs at least 2 lattice points (got %u x %u x %u)", what, X, Y, Z);
    const uint64_t xy = (uint64_t)X * Y, lim = (uint64_t)1 << 31;      // xy < 2^31 keeps xy * Z below 2^63
    NGP_REQUIRE(xy < lim && xy * Z < lim, "%s: X * Y * Z must be < 2^31 (got %u x %u x %u)", what, X, Y, Z);
    return NGP_OK;
}

}  // namespace ngp

using namespace ngp;

extern "C" {

size_t ngp_isosurface_workspace(uint32_t X, uint32_t Y, uint32_t Z) {
    if (iso_check_dims("isosurface_workspace", X, Y, Z) != NGP_OK) return 0;
    Carver c; iso_layout(c, X * Y * Z); return c.bytes();
}

int ngp_isosurface_count(const float* u, uint32_t X, uint32_t Y, uint32_t Z, float threshold, void* workspace, size_t workspace_bytes,
                         uint64_t* totals, ngp_stream_t stream) {
    int rc = iso_check_dims("isosurface_count", X, Y, Z);
    if (rc) return rc;
    NGP_REQUIRE(u && totals, "isosurface_count: null pointer");
    NGP_REQUIRE(((uintptr_t)totals & 7) == 0, "isosurface_count: totals must be 8-byte aligned");
    rc = check_workspace("isosurface_count", workspace, workspace_bytes, ngp_isosurface_workspace(X, Y, Z), 8);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const IsoDims D{X, Y, Z, X * Y * Z, Y * Z};
    Carver c(workspace);
    const IsoWorkspace w = iso_layout(c, D.N);
    {
        ProfScope prof("isosurface_count", s, (double)D.N);
        k_iso_flags<<<w.n_blocks, kIsoBlock, 0, s>>>(u, D.N, threshold, w.flags);
        k_iso_count<<<w.n_blocks, kIsoBlock, 0, s>>>(w.flags, D, w.mask, w.ntri, w.vpre, w.fpre, w.block_tot);
    }
    {
        ProfScope prof("isosurface_scan", s, (double)w.n_blocks);
        k_iso_scan<<<1, kIsoScanBlock, 0, s>>>(w.block_tot, w.n_blocks, reinterpret_cast<unsigned long long*>(totals));
    }
    return check_launch("isosurface_count");
}

int ngp_isosurface_emit(const float* u, uint32_t X, uint32_t Y, uint32_t Z, float threshold, const void* workspace, size_t workspace_bytes,
                        uint64_t V, uint64_t F, float* vertices, int32_t* faces, ngp_stream_t stream) {
    int rc = iso_check_dims("isosurface_emit", X, Y, Z);
    if (rc) return rc;
    NGP_REQUIRE(V < ((uint64_t)1 << 31) && F < ((uint64_t)1 << 31), "isosurface_emit: V and F must be < 2^31 (got V = %llu, F = %llu)",
                (unsigned long long)V, (unsigned long long)F);
    NGP_REQUIRE(u, "isosurface_emit: null pointer");
    NGP_REQUIRE((V == 0 || vertices) && (F == 0 || faces), "isosurface_emit: null output for a non-empty mesh");
    rc = check_workspace("isosurface_emit", workspace, workspace_bytes, ngp_isosurface_workspace(X, Y, Z), 8);
    if (rc) return rc;
    if (V == 0 && F == 0) return NGP_OK;
    hipStream_t s = (hipStream_t)stream;
    const IsoDims D{X, Y, Z, X * Y * Z, Y * Z};
    Carver c(const_cast<void*>(workspace));      // (read only here: ngp_isosurface_count filled it)
    const IsoWorkspace w = iso_layout(c, D.N);
    ProfScope prof("isosurface_emit", s, (double)D.N);
    k_iso_emit<<<w.n_blocks, kIsoBlock, 0, s>>>(u, w.flags, D, threshold, w.mask, w.ntri, w.vpre, w.fpre, w.block_tot, (uint32_t)V, (uint32_t)F,
                                                vertices, faces);
    return check_launch("isosurface_emit");
}

}  // extern "C"
