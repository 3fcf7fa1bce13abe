// launch_plan.hpp -- the arithmetic of "several reference iterations per launch" (render_fused.hip, struct Ctl): how many iterations the
// next launch covers and whether a finished launch was equivalent to the reference's iterations.  Plain integer code, host and
// device: k_render_compact and tests/test_launch_plan_cpu.py (compiled with a host compiler) share this one copy.
#ifndef NGP_LAUNCH_PLAN_HPP
#define NGP_LAUNCH_PLAN_HPP
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define NGP_PLAN_HD __host__ __device__ __forceinline__
#else
#define NGP_PLAN_HD inline
#endif

namespace ngp {

constexpr uint32_t kSpecK = 8;            // most reference iterations per launch
constexpr uint32_t kSpecSafetyX2 = 1;     // later launches: sized for kSpecSafetyX2 / 2 x the recent death rate (+ 4 sigma + 16 rays).  1.5 x until
                                          // a failed launch came to be replayed as its verified prefix: a wrong guess now costs the discarded
                                          // launch only, and the larger launches win (bound-2 frame: 49.5 -> 41.8 launches, 4.80 -> 4.48 ms)
constexpr uint32_t kForecastBuckets = 8;  // saturation forecast: rays expected to saturate after 1 .. 8 further samples (k_render_iter, step 4)

// the reference's schedule: n_step = clamp(N // n_alive, 1, 8) (renderer.py:347-373)
NGP_PLAN_HD uint32_t schedule_n_step(uint32_t N, uint32_t n_alive) {
    const uint32_t ns = n_alive ? N / n_alive : 8u;
    return ns < 1u ? 1u : (ns > 8u ? 8u : ns);
}

// VERDICT on a finished launch of K iterations of q samples: n_alive(j) = n_alive - deaths before j.  Each iteration after the first
// must have been run with n_step = clamp(N // n_alive, 1, 8) == q, and the loop would have stopped at the first empty list.
// `keep`: the iterations before the first violation.  They WERE the reference's (every ray was processed exactly as the reference
// processes it up to there, so their death counts are the true ones): a launch of just those verifies for certain.
// own_last: the last iteration of the loop must run on its own (the caller wants its tensors), so a launch in which the last ray
// dies is a violation too.
struct LaunchVerdict { uint32_t bad, keep; };
NGP_PLAN_HD LaunchVerdict launch_verdict(uint32_t N, uint32_t n_alive, uint32_t q, uint32_t K, const uint32_t* deaths, bool own_last) {
    LaunchVerdict v = {0u, K};
    uint32_t alive = n_alive;
    for (uint32_t j = 0; j < K; j++) {
        if (alive == 0) break;                            // the reference stops here; the rest of the launch had no ray to touch
        if (j > 0 && schedule_n_step(N, alive) != q) { v.bad = 1; v.keep = j; break; }
        alive -= deaths[j] < alive ? deaths[j] : alive;
        if (own_last && alive == 0) { v.bad = 1; v.keep = j; break; }
    }
    return v;
}

// floor(sqrt(x)): a float estimate put right by at most a step or two (the planning thread of k_render_compact asks for it up to
// eight times per launch, for counts of 10^5: counting up from zero was microseconds on the loop's critical path)
NGP_PLAN_HD uint32_t isqrt_floor(uint32_t x) {
    unsigned long long sq = (unsigned long long)sqrtf((float)x);
    while (sq * sq > x) sq--;
    while ((sq + 1) * (sq + 1) <= x) sq++;
    return (uint32_t)sq;
}
// four standard deviations of a count that size, and 16 rays
NGP_PLAN_HD uint32_t death_allowance(uint32_t count) { return 4u * isqrt_floor(count) + 16u; }

// PLAN of the next launch: K iterations of q = clamp(N // n_alive, 1, 8) samples, for n_alive rays of which `recent` died per
// iteration lately.  Two guesses of the deaths inside the launch, and the smaller K wins (the larger guess, P = max(D, R)):
//   R  the recent death rate: as many iterations as kSpecSafetyX2 / 2 x (recent + allowance) leaves room for above the n_alive at
//      which the reference's n_step changes (N // n_alive == q  <=>  n_alive > N / (q + 1));
//   D  the saturation forecast: forecast[s - 1] rays will have T < 1e-4 after s further samples if their last opacity persists
//      (NULL: no forecast).  D(j) = rays with s <= j q die within the first j iterations; iteration j is verified against the
//      deaths of iterations 0 .. j-1 (launch_verdict), so K iterations need D(j) + allowance(D(j)) <= headroom for j = 1 .. K-1.
// Caps: at most 8 samples per ray and launch while n_step is small, cap_mid_max for n_step 2..4, cap_hi in the n_step >= 5 regimes
// (few rays, every launch latency-bound); at most `room` iterations (what max_steps leaves).  With n_step = 8 the guess cannot fail.
// K < 2: the next launch is an ordinary one.
struct LaunchPlan {
    uint32_t K;            // iterations of the next launch, after the caps and `room`
    uint32_t K_rate;       // ... as the death rate alone would have it (after the same caps)
    uint32_t headroom;     // rays that may die before N // n_alive changes
    uint32_t rate;         // recent + allowance: the per-iteration guess R is sized from
    uint32_t forecast;     // D(K - 1) of the chosen K: forecast deaths before its last verified iteration
};
NGP_PLAN_HD LaunchPlan plan_launch(uint32_t N, uint32_t n_alive, uint32_t q, uint32_t recent, const uint32_t* forecast, uint32_t room,
                                   uint32_t cap_mid_max, uint32_t cap_hi, bool own_last) {
    LaunchPlan p = {};
    p.headroom = n_alive - (q == 8u ? 0u : N / (q + 1u)) - 1u;
    const unsigned long long rate = (unsigned long long)recent + 4ull * isqrt_floor(recent) + 16ull;
    p.rate = (uint32_t)rate;
    uint32_t K = (uint32_t)((unsigned long long)p.headroom * 2u / (kSpecSafetyX2 * rate));
    const uint32_t cap_mid = 8u * q < cap_mid_max ? 8u * q : cap_mid_max;      // (n_alive <= N / q: at most 8 N samples per launch)
    const uint32_t cap_samples = q == 1u ? 8u : (q <= 4u ? cap_mid : cap_hi);
    const uint32_t capK = cap_samples / q < kSpecK ? cap_samples / q : kSpecK;
    K = (q == 8u && !own_last) ? capK : (K < capK ? K : capK);
    K = K < room ? K : room;
    p.K_rate = K;
    if (forecast && !(q == 8u && !own_last)) {
        uint32_t Kf = 1, D = 0, s = 0;
        for (uint32_t j = 1; j < K; j++) {               // may iteration j be part of the launch?
            for (; s < kForecastBuckets && s + 1u <= j * q; s++) D += forecast[s];
            if ((unsigned long long)D + death_allowance(D) > p.headroom) break;
            Kf = j + 1u;
            p.forecast = D;
        }
        K = K < Kf ? K : Kf;
    }
    p.K = K;
    return p;
}

}  // namespace ngp
#endif
