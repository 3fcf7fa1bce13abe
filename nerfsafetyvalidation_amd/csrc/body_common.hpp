// body_common.hpp -- what the units that judge the drone's body share (body.hip: the verdict; clearance.hip: the distance): the box
// table's row, the way into the box's frame, the box's world extent, the two closed overlap tests of world.py's "The body rule" and
// the outward float32 rounding of the box's bounds.  float64, one IEEE rounding per operation: a unit that includes this is compiled
// with -ffp-contract=off and holds no fma.
#pragma once
#include "cast_common.hpp"

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

// the closed box-triangle test of the rule: p[k][a] the triangle's vertices in the box's frame (body_tri_overlaps: w[k][a] its world
// vertices); true when no axis separates
__device__ __forceinline__ bool body_tri_overlaps_frame(const BodyBox& B, const double p[3][3]) {
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
__device__ __forceinline__ bool body_tri_overlaps(const BodyBox& B, const double w[3][3]) {
    double p[3][3];
#pragma unroll
    for (int k = 0; k < 3; k++) body_to_frame(B, w[k], p[k]);
    return body_tri_overlaps_frame(B, p);
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

}  // namespace ngp
