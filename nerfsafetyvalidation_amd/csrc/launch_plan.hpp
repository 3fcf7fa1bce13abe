// launch_plan.hpp -- the schedule of the fused render loop (render_fused.hip) as one integer state machine, Ctl -> Ctl: the state a
// call starts from (loop_begin), the cut of a launch that cannot verify (truncate_launch), the verdict on a finished launch
// (launch_verdict), the state after it (finish_launch, which sizes the next launch with plan_launch) and the words that carry a
// state to the host (pack_status / pack_fin and their inverses).  Plain integer code with no pointer into a device buffer, host and
// device: the kernels and tests/test_launch_plan_cpu.py (compiled with a host compiler, where it runs whole loops against the
// reference's) share this one copy.
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
constexpr uint32_t kSpecMarginDiv = 16;   // first launch: entered only if n_alive - N/2 > N / kSpecMarginDiv
// largest q for which a launch covers several iterations (K * q <= 8 samples per ray and launch, K >= 2)
constexpr uint32_t kSpecMaxQ = 8;
constexpr uint32_t kSpecMaxSamples = 32;  // samples per ray and launch in the n_step >= 5 regimes (plan_launch's cap_hi)
constexpr uint32_t kSpecMidSamples = 8;   // ... and in the n_step 2..4 regimes (its cap_mid_max)

// the switches of the schedule, one word per render call (composed by ngp_render_rays)
constexpr uint32_t kPlanMulti = 1;        // launches may cover several reference iterations
constexpr uint32_t kPlanOwnLast = 2;      // the loop's last iteration runs on its own (the caller wants its tensors)
constexpr uint32_t kPlanReplayOne = 4;    // diagnostics: a failed launch is replayed as ONE iteration, not as its verified prefix
constexpr uint32_t kPlanNoForecast = 8;   // diagnostics: launches are sized by the death rate alone, not by the saturation forecast

// device-side loop state (ping-pong pair)
struct Ctl {
    uint32_t n_alive, n_step, step, done;
    uint32_t iters, last_n_alive, last_n_step, pad;
    unsigned long long samples_marched, samples_slots;
    uint32_t spec, rollbacks, backoff, rsv;   // see "several reference iterations per launch" below
    // schedule diagnostics (ngp_render_ctx_schedule_stats): accumulated by finish_launch, nothing in the loop reads them back
    unsigned long long discarded;             // network samples of the launches that were rolled back
    uint32_t fc_sized, spec_launches;         // launches the saturation forecast made smaller; multi-iteration launches run
    uint32_t fc_pred, fc_actual;              // last multi-iteration launch: deaths forecast / counted before its last verified iteration
    uint32_t plan_pred, plan_headroom, plan_rate, plan_k_rate;   // the plan of the launch this state starts (trace, fc_pred)
};

// Several reference iterations per launch.  While more than half of the N rays are alive the reference's schedule is
// n_step = clamp(N // n_alive, 1, 8) = 1: one sample per ray and iteration, for dozens of iterations (50 of the 56 of an 800x800
// Stonehenge frame), each paying a launch, the per-ray state round trip and a compaction for a single sample.  A launch with
// `spec` = q set covers K = n_step / q consecutive reference iterations of q samples each: per ray it emulates the iteration
// boundaries exactly (march restarts from the re-accumulated rays_t, raymarching.cu:727,848) and the per-iteration death
// counts give the n_alive sequence, so iterations / samples_slots / step are the reference's.  That is valid only if
// N // n_alive stays q through the K iterations.  K is GUESSED from the recent death rate and the launch is VERIFIED afterwards
// by k_render_compact: on a violation every ray gets back the state the launch started from (each wave saves it when it
// loads it), the alive list is handed on unchanged and the iteration is run again on its own -- a wrong guess costs one
// launch, never a result.  Not used with perturb (the jitter of an iteration is seeded with the ray's index in that
// iteration's list).

// the reference's schedule: n_step = clamp(N // n_alive, 1, 8) (renderer.py:347-373)
NGP_PLAN_HD uint32_t schedule_n_step(uint32_t N, uint32_t n_alive) {
    const uint32_t ns = n_alive ? N / n_alive : 8u;
    return ns < 1u ? 1u : (ns > 8u ? 8u : ns);
}

// BEGIN: the state a call of N rays starts from.  Its first launch covers several iterations of one sample when more than
// N/2 + N/kSpecMarginDiv rays are alive (all N are) and max_steps leaves room for two.
NGP_PLAN_HD Ctl loop_begin(uint32_t N, uint32_t max_steps, uint32_t flags) {
    Ctl c = {};
    c.n_alive = N;
    c.n_step = 1;  // clamp(N // N, 1, 8)
    c.done = (N == 0 || max_steps == 0) ? 1 : 0;
    const uint32_t room = (flags & kPlanOwnLast) ? (max_steps ? max_steps - 1 : 0) : max_steps;   // the last iteration runs on its own
    if ((flags & kPlanMulti) && !c.done && N > N / 2 + N / kSpecMarginDiv && room >= 2) {
        c.spec = 1;
        c.n_step = room < kSpecK ? room : kSpecK;
    }
    return c;
}

// A multi-iteration launch that cannot pass its verification is cut short BEFORE the network runs.  k_march_ahead knows, for every
// ray, in which of the launch's iterations its march runs out of samples (the ray dies there at the latest): those counts are a lower
// bound of the deaths per iteration, and N // n_alive only grows as rays die, so an iteration whose n_step already differs from q
// under the lower bound differs for certain.  The launch then covers the iterations before it (one iteration: an ordinary launch);
// k_render_iter and k_render_compact both apply this to their copy of the launch's Ctl, from the same counts.  Cameras outside the
// scene box (BASELINE configs[3]) lose most rays in the first iteration: without this the first launch of every frame ran the
// network on up to eight samples per ray, failed its verification and was run again.
// `exhausted[j]`: rays whose march ends in iteration j of the launch (summed over the shards).
NGP_PLAN_HD void truncate_launch(Ctl& c, const uint32_t* exhausted, uint32_t N) {
    if (!c.spec) return;
    const uint32_t q = c.spec, K = c.n_step / q;
    uint32_t alive = c.n_alive, ok = K;
    for (uint32_t j = 0; j < K; j++) {
        if (alive == 0) break;                                    // (the reference stops here: nothing left to violate)
        const uint32_t want_q = N / alive;
        if (j > 0 && (want_q < 1 ? 1u : (want_q > 8 ? 8u : want_q)) != q) { ok = j; break; }
        alive -= exhausted[j] < alive ? exhausted[j] : alive;
    }
    if (ok < K) {
        if (ok <= 1) { c.spec = 0; c.n_step = q; }
        else c.n_step = ok * q;
        c.rsv += 1;                                               // (diagnostics: launches cut short)
    }
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

// TRANSITION: the state after a finished launch.  `c`: the launch's state after truncate_launch; `v`: its launch_verdict (nothing
// to judge for an ordinary launch: bad = 0); deaths[j]: rays that died in its iteration j; `forecast`: the saturation forecast of
// its survivors; `survivors`: the length of the compacted list; `marched`: the network samples of the launch.
//   v.bad  ROLL-BACK: the launch was not equivalent to the reference's iterations and every ray has its state back.  Nothing
//          advances; the next launch runs the iterations before the violation again as one launch, certain to verify (see
//          launch_verdict's `keep`), or, with fewer than two of them (or kPlanReplayOne), the one iteration on its own, and the two
//          launches after that are ordinary ones too (`backoff`).
//   else   COMMIT: iters / samples_slots / step / last_n_* advance by the reference iterations the launch covered, re-derived from
//          the per-iteration deaths (iterations after the list ran empty are the reference's never-run ones), and the next launch
//          may again cover several iterations of q = n_step samples: as many as plan_launch finds room for above the n_alive at
//          which the reference's n_step changes, judged by the recent death rate and by the forecast.
// A state with `spec` set starts a launch that counts deaths per iteration: whoever stores it clears that launch's counters first.
NGP_PLAN_HD Ctl finish_launch(const Ctl& c, LaunchVerdict v, const uint32_t* deaths, const uint32_t* forecast, uint32_t survivors,
                              unsigned long long marched, uint32_t N, uint32_t max_steps, uint32_t flags, uint32_t cap_mid_max,
                              uint32_t cap_hi) {
    Ctl n = c;
    n.plan_pred = 0; n.plan_headroom = 0; n.plan_rate = 0; n.plan_k_rate = 0;   // (the plan of the next launch, if it is a guess)
    if (c.spec) {   // schedule diagnostics: how the launch's forecast compared
        uint32_t before_last = 0;
        for (uint32_t j = 0; j + 1 < c.n_step / c.spec; j++) before_last += deaths[j];
        n.spec_launches = c.spec_launches + 1;
        n.fc_pred = c.plan_pred;
        n.fc_actual = before_last;
    }
    if (v.bad) {
        n.rollbacks = c.rollbacks + 1;
        n.discarded = c.discarded + marched;
        if (v.keep >= 2 && !(flags & kPlanReplayOne)) {
            n.spec = c.spec;
            n.n_step = v.keep * c.spec;
            n.backoff = 0;
        } else {
            n.spec = 0;
            n.n_step = schedule_n_step(N, c.n_alive);
            n.backoff = 2;                                    // the next two iterations run one per launch
        }
        return n;
    }
    n.samples_marched = c.samples_marched + marched;
    n.n_alive = survivors;
    uint32_t recent = c.n_alive - n.n_alive;   // deaths per reference iteration, most recent observation
    if (!c.spec) {
        n.last_n_alive = c.n_alive;
        n.last_n_step = c.n_step;
        n.iters = c.iters + 1;
        n.samples_slots = c.samples_slots + (unsigned long long)c.n_alive * c.n_step;
        n.step = c.step + c.n_step;
    } else {
        const uint32_t q = c.spec, K = c.n_step / q;
        uint32_t alive = c.n_alive, d_last = 0, d_prev = 0;
        unsigned long long slots = c.samples_slots;
        uint32_t it = 0;
        for (uint32_t j = 0; j < K; j++) {
            if (alive == 0) break;                            // iterations the reference does not run
            slots += (unsigned long long)alive * q;
            it++;
            n.last_n_alive = alive;
            n.last_n_step = q;
            alive -= deaths[j];
            d_prev = d_last;
            d_last = deaths[j];
        }
        recent = d_last > d_prev ? d_last : d_prev;            // the launch's last two iterations
        n.iters = c.iters + it;
        n.samples_slots = slots;
        n.step = c.step + it * q;
    }
    n.n_step = schedule_n_step(N, n.n_alive);
    n.done = (n.n_alive == 0 || n.step >= max_steps) ? 1 : 0;
    n.spec = 0;
    if (n.backoff) n.backoff--;
    else if ((flags & kPlanMulti) && !n.done && n.n_step <= kSpecMaxQ && (n.n_step == 8 || n.n_alive > N / (n.n_step + 1))) {
        const uint32_t q = n.n_step;
        const bool own_last = (flags & kPlanOwnLast) != 0;     // the last iteration must not be part of such a launch
        uint32_t room = (max_steps - n.step) / q;
        if (own_last && room) room--;
        const LaunchPlan p = plan_launch(N, n.n_alive, q, recent, (flags & kPlanNoForecast) ? nullptr : forecast, room, cap_mid_max, cap_hi, own_last);
        if (p.K < p.K_rate && p.K_rate >= 2) n.fc_sized = c.fc_sized + 1;
        if (p.K >= 2) {
            n.spec = q; n.n_step = p.K * q;
            n.plan_pred = p.forecast; n.plan_headroom = p.headroom; n.plan_rate = p.rate; n.plan_k_rate = p.K_rate;
        }
    }
    return n;
}

// What the host needs while it enqueues launches ahead -- how many rays are left and whether the loop has ended -- is ONE 64-bit
// word: sequence number << 32 | done << 31 | n_alive.
struct LoopStatus { uint32_t seq, done, n_alive; };
NGP_PLAN_HD unsigned long long pack_status(uint32_t seq, const Ctl& n) {
    return ((unsigned long long)seq << 32) | ((unsigned long long)(n.done ? 1u : 0u) << 31) | (n.n_alive & 0x7FFFFFFFu);
}
NGP_PLAN_HD LoopStatus unpack_status(unsigned long long w) {
    return {(uint32_t)(w >> 32), (uint32_t)((w >> 31) & 1ull), (uint32_t)w & 0x7FFFFFFFu};
}
// The counters of a finished loop (ngp_render_stats) in four words, each carrying in its upper 16 bits a tag that names the render
// CALL (bit 15 + a 15-bit call counter): 48-bit sample counts, 24-bit iters and rollbacks, last_n_alive above an 8-bit last_n_step.
// unpack_fin: false unless all four words carry this call's tag (another call's words, or none yet).
NGP_PLAN_HD void pack_fin(const Ctl& n, uint32_t call_tag, unsigned long long w[4]) {
    const unsigned long long tag = (unsigned long long)(0x8000u | (call_tag & 0x7FFFu)) << 48;
    w[0] = tag | (n.samples_marched & 0xFFFFFFFFFFFFull);
    w[1] = tag | (n.samples_slots & 0xFFFFFFFFFFFFull);
    w[2] = tag | ((unsigned long long)(n.iters & 0xFFFFFFu) << 24) | (n.rollbacks & 0xFFFFFFu);
    w[3] = tag | ((unsigned long long)n.last_n_alive << 8) | (n.last_n_step & 0xFFu);
}
NGP_PLAN_HD bool unpack_fin(const unsigned long long w[4], uint32_t call_tag, Ctl& fin) {
    for (int i = 0; i < 4; i++)
        if ((w[i] >> 48) != (0x8000u | (call_tag & 0x7FFFu))) return false;
    fin.samples_marched = w[0] & 0xFFFFFFFFFFFFull;
    fin.samples_slots = w[1] & 0xFFFFFFFFFFFFull;
    fin.iters = (uint32_t)((w[2] >> 24) & 0xFFFFFFu);
    fin.rollbacks = (uint32_t)(w[2] & 0xFFFFFFu);
    fin.last_n_alive = (uint32_t)((w[3] >> 8) & 0xFFFFFFFFu);
    fin.last_n_step = (uint32_t)(w[3] & 0xFFu);
    return true;
}

}  // namespace ngp
#endif
