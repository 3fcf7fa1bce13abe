// freq_math.hpp -- sin and cos of 2^f x for the frequency encoder (freqencoder.hip), host and device.
//
// The argument 2^f x is an exact float (a scaling by a power of two), so the only errors are the range reduction's and the
// polynomials'.  The reduction is done ONCE per input value, in double, in quarter turns:
//     t = x * (2 / pi)                    two roundings of 2^-53: relative 2^-52
//     u_f = 2^f t                         exact (a doubling per frequency)
//     q = rint(u_f),  r = u_f - q         exact;  |r| <= 1/2 quarter turn
//     a = float(r * (pi / 2))             |a| <= pi / 4
// For |x| <= kFreqFastMax = 1024 and f <= 15, |u_f| < 2^25 and its error is below 2^25 2^-52 = 2^-27 quarter turns = 1.2e-8 rad;
// rounding a to float adds at most 2^-25 (pi/4) = 2.4e-8.  sin a and cos a come from two polynomials in a^2 (least-squares fits on
// Chebyshev nodes of [0, (pi/4)^2], truncation below 3e-9) evaluated with fmaf, and q mod 4 picks and signs them.  Measured on the
// host against float64 (DESIGN.md "Frequency encoder"): 9.3e-8 worst at every degree up to 16, for |x| < 2 and for |x| < 1024 alike
// (a correctly rounded float result is within 3e-8).  Larger or non-finite x takes the library's sincosf on ldexpf(x, f)
// (freqencoder.hip).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define NGP_HD __host__ __device__ __forceinline__
#else
#define NGP_HD inline
#endif

namespace ngp {

constexpr float kFreqFastMax = 1024.0f;
constexpr uint32_t kFreqMaxDegree = 16;

// x in quarter turns (the `t` above)
NGP_HD double freq_quarter_turns(float x) { return (double)x * 0.63661977236758134308; }

// sin and cos of (pi/2) u, u in quarter turns with |u| < 2^31
NGP_HD void freq_sincos_quarter(double u, float& s, float& c) {
    const double q = rint(u);
    const float a = (float)((u - q) * 1.57079632679489661923);
    const int32_t qi = (int32_t)q;
    const float z = a * a;
    float p = fmaf(z, 0x1.6c4bf2p-19f, -0x1.a00ceep-13f);
    p = fmaf(z, p, 0x1.111104p-7f);
    p = fmaf(z, p, -0x1.555556p-3f);
    const float sn = fmaf(a * z, p, a);                    // a + a^3 P(a^2)
    float k = fmaf(z, -0x1.23fed2p-22f, 0x1.a01044p-16f);
    k = fmaf(z, k, -0x1.6c16b8p-10f);
    k = fmaf(z, k, 0x1.555556p-5f);
    const float cs = fmaf(z * z, k, fmaf(z, -0.5f, 1.0f));  // 1 - a^2/2 + a^4 Q(a^2)
    // q = 0: (sn, cs)   1: (cs, -sn)   2: (-sn, -cs)   3: (-cs, sn)
    const bool swap = (qi & 1) != 0;
    const float s0 = swap ? cs : sn, c0 = swap ? sn : cs;
    s = (qi & 2) ? -s0 : s0;
    c = ((qi + 1) & 2) ? -c0 : c0;
}

}  // namespace ngp
