"""The schedule of the fused render loop (csrc/launch_plan.hpp: the Ctl state machine and its leaves plan_launch, launch_verdict),
compiled for the host into a small stand-alone program that answers one query per input line.  No GPU: the kernels and this test share
the one copy of the code."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nerfsafetyvalidation_amd", "csrc")
K_MAX, SAFETY_X2 = 8, 1          # kSpecK, kSpecSafetyX2

MAIN = r"""
#include <stdio.h>
#include <vector>
#include "launch_plan.hpp"
using namespace ngp;

struct Rng {   // splitmix64
    unsigned long long s;
    unsigned long long next() { unsigned long long z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
                                z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    unsigned below(unsigned n) { return (unsigned)(next() % n); }
};
// The ray model: M march samples available, saturation after S samples.  One iteration of q samples: the ray takes
// e = min(q, M - used) of them and dies if the march ran out (e < q) or it has saturated (used >= S).
struct Rays { std::vector<unsigned> M, S, used; };
static bool iterate(Rays& r, unsigned ray, unsigned q, unsigned long long& marched) {
    const unsigned left = r.M[ray] - r.used[ray], e = q < left ? q : left;
    r.used[ray] += e;
    marched += e;
    return e < q || r.used[ray] >= r.S[ray];
}
struct Outcome { unsigned long long iters, slots, step, last_n_alive, last_n_step, marched; std::vector<unsigned> alive, used; };

// the reference's loop (renderer.py:347-373): one iteration per pass, n_step from the list's length
static Outcome reference_loop(Rays r, unsigned N, unsigned max_steps) {
    Outcome o = {};
    for (unsigned i = 0; i < N; i++) o.alive.push_back(i);
    while (o.step < max_steps && !o.alive.empty()) {
        const unsigned n_alive = (unsigned)o.alive.size(), q = schedule_n_step(N, n_alive);
        std::vector<unsigned> next;
        for (unsigned ray : o.alive) if (!iterate(r, ray, q, o.marched)) next.push_back(ray);
        o.iters++; o.slots += (unsigned long long)n_alive * q; o.step += q; o.last_n_alive = n_alive; o.last_n_step = q;
        o.alive.swap(next);
    }
    o.used = r.used;
    return o;
}

// the launch loop, from launch_plan.hpp alone: what k_render_init, k_march_ahead, k_render_iter and k_render_compact do with the state
struct Counts { unsigned launches, rollbacks, cut, replay_prefix, replay_one, last_spec, bound_ok; };
static Outcome launch_loop(Rays r, unsigned N, unsigned max_steps, unsigned flags, Rng fc_rng, unsigned fc_shift, Counts& k) {
    Outcome o = {};
    for (unsigned i = 0; i < N; i++) o.alive.push_back(i);
    Ctl c = loop_begin(N, max_steps, flags);
    k = Counts{};
    k.bound_ok = 1;
    while (!c.done) {
        if (++k.launches > 2u * max_steps + 16u) { k.bound_ok = 0; break; }      // ngp_render_rays' "cannot happen"
        unsigned exhausted[kSpecK] = {}, deaths[kSpecK] = {}, forecast[kForecastBuckets];
        if (c.spec)      // k_march_ahead: the iteration of the PLANNED launch in which a ray's march runs out
            for (unsigned ray : o.alive) {
                const unsigned left = r.M[ray] - r.used[ray];
                if (left < c.n_step) exhausted[left / c.spec]++;
            }
        const unsigned rsv = c.rsv;
        truncate_launch(c, exhausted, N);
        k.cut += c.rsv - rsv;
        const unsigned q = c.spec ? c.spec : c.n_step, K = c.spec ? c.n_step / c.spec : 1u;
        const std::vector<unsigned> backup = r.used;
        std::vector<unsigned> next;
        unsigned long long marched = 0;
        for (unsigned ray : o.alive) {
            bool dead = false;
            for (unsigned j = 0; j < K && !dead; j++)
                if ((dead = iterate(r, ray, q, marched))) deaths[j]++;
            if (!dead) next.push_back(ray);
        }
        LaunchVerdict v = {0u, 0u};
        if (c.spec) v = launch_verdict(N, c.n_alive, c.spec, K, deaths, (flags & kPlanOwnLast) != 0);
        if (v.bad) r.used = backup;             // roll-back: every ray's state restored, the list handed on unchanged
        else o.alive.swap(next);
        for (unsigned& f : forecast) f = fc_rng.below((c.n_alive >> fc_shift) + 1u);      // nothing to do with the rays
        const Ctl n = finish_launch(c, v, deaths, forecast, (unsigned)o.alive.size(), marched, N, max_steps, flags, kSpecMidSamples, kSpecMaxSamples);
        if (v.bad) { k.rollbacks++; if (n.spec) k.replay_prefix++; else k.replay_one++; }
        k.last_spec = c.spec;
        c = n;
    }
    o.iters = c.iters; o.slots = c.samples_slots; o.step = c.step; o.last_n_alive = c.last_n_alive; o.last_n_step = c.last_n_step;
    o.marched = c.samples_marched;
    o.used = r.used;
    if (k.rollbacks != c.rollbacks || k.cut != c.rsv) k.bound_ok = 0;      // (the state's own counters say the same)
    return o;
}

int main() {
    static_assert(kSpecK == 8 && kSpecSafetyX2 == 1 && kForecastBuckets == 8, "the test transcribes these");
    static_assert(kSpecMarginDiv == 16 && kSpecMaxQ == 8 && kSpecMaxSamples == 32 && kSpecMidSamples == 8, "the schedule the feasibility run used");
    static_assert(kPlanMulti == 1 && kPlanOwnLast == 2 && kPlanReplayOne == 4 && kPlanNoForecast == 8, "the test draws flag words from these bits");
    char kind;
    while (scanf(" %c", &kind) == 1) {
        unsigned N, n_alive, q, K, flag, a[8];
        if (kind == 'L') {          // one trial: rays drawn from `seed` in one of four lifetime shapes, both loops over them
            unsigned max_steps, shape, fc_shift;
            unsigned long long seed;
            if (scanf("%u %u %u %u %u %llu", &N, &max_steps, &flag, &shape, &fc_shift, &seed) != 6) return 2;
            Rng rng = {seed};
            Rays r;
            for (unsigned i = 0; i < N; i++) {
                const unsigned m = shape == 0 ? rng.below(4) : shape == 1 ? rng.below(300)
                                   : shape == 2 ? (rng.below(3) < 2 ? rng.below(5) : rng.below(400)) : 30 + rng.below(20);
                r.M.push_back(m);
                r.S.push_back(1 + rng.below(shape == 3 ? 60 : 500));
                r.used.push_back(0);
            }
            Counts k;
            const Outcome want = reference_loop(r, N, max_steps), got = launch_loop(r, N, max_steps, flag, Rng{seed ^ 0x5DEECE66Dull}, fc_shift, k);
            printf("%llu %llu %llu %llu %llu %llu  %llu %llu %llu %llu %llu %llu  %d %d  %u %u %u %u %u %u %u\n", want.iters, want.slots, want.step,
                   want.last_n_alive, want.last_n_step, want.marched, got.iters, got.slots, got.step, got.last_n_alive, got.last_n_step, got.marched,
                   (int)(want.alive == got.alive), (int)(want.used == got.used), k.launches, k.rollbacks, k.cut, k.replay_prefix, k.replay_one,
                   k.last_spec, k.bound_ok);
        } else if (kind == 'W') {   // the status word, packed and unpacked
            Ctl c = {};
            unsigned seq;
            if (scanf("%u %u %u", &seq, &c.done, &c.n_alive) != 3) return 2;
            const LoopStatus s = unpack_status(pack_status(seq, c));
            printf("%u %u %u\n", s.seq, s.done, s.n_alive);
        } else if (kind == 'F') {   // the finished loop's words, packed with one call tag and unpacked with it and with another
            Ctl c = {}, back = {}, other = {};
            unsigned tag, other_tag;
            if (scanf("%llu %llu %u %u %u %u %u %u", &c.samples_marched, &c.samples_slots, &c.iters, &c.rollbacks, &c.last_n_alive, &c.last_n_step,
                      &tag, &other_tag) != 8) return 2;
            unsigned long long w[4], none[4] = {0, 0, 0, 0}, mixed[4];
            pack_fin(c, tag, w);
            const bool ok = unpack_fin(w, tag, back), wrong = unpack_fin(w, other_tag, other), empty = unpack_fin(none, tag, other);
            pack_fin(c, other_tag, mixed);
            mixed[0] = w[0]; mixed[1] = w[1]; mixed[2] = w[2];      // three words of this call, the fourth still the other call's
            const bool torn = unpack_fin(mixed, tag, other);
            printf("%d %d %d %d %llu %llu %u %u %u %u\n", (int)ok, (int)wrong, (int)empty, (int)torn, back.samples_marched, back.samples_slots, back.iters,
                   back.rollbacks, back.last_n_alive, back.last_n_step);
        } else if (kind == 'V') {
            if (scanf("%u %u %u %u %u", &N, &n_alive, &q, &K, &flag) != 5) return 2;
            for (int i = 0; i < 8; i++) if (scanf("%u", &a[i]) != 1) return 2;
            const LaunchVerdict v = launch_verdict(N, n_alive, q, K, a, flag != 0);
            printf("%u %u\n", v.bad, v.keep);
        } else if (kind == 'P') {
            unsigned recent, room, cap_mid, cap_hi, own_last, has_fc;
            if (scanf("%u %u %u %u %u %u %u %u %u", &N, &n_alive, &q, &recent, &room, &cap_mid, &cap_hi, &own_last, &has_fc) != 9) return 2;
            for (int i = 0; i < 8; i++) if (scanf("%u", &a[i]) != 1) return 2;
            const LaunchPlan p = plan_launch(N, n_alive, q, recent, has_fc ? a : nullptr, room, cap_mid, cap_hi, own_last != 0);
            printf("%u %u %u %u %u\n", p.K, p.K_rate, p.headroom, p.rate, p.forecast);
        } else if (kind == 'S') {
            if (scanf("%u", &N) != 1) return 2;
            printf("%u\n", isqrt_floor(N));
        } else return 3;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("launch_plan")
    src, exe = d / "main.cpp", d / "launch_plan"
    src.write_text(MAIN)
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), str(src)])

    def run(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
        rows = [[int(v) for v in ln.split()] for ln in out.splitlines()]
        assert len(rows) == len(lines)
        return rows
    return run


def n_step_of(N, alive):
    return min(8, max(1, N // alive)) if alive else 8


def random_launches(rng, n):
    """consistent launches: q is the schedule's n_step at the start, the full death vector never kills more rays than there are"""
    out = []
    for i in range(n):
        N = int(rng.integers(1, 1 << int(rng.integers(1, 21))))
        n_alive = int(rng.integers(1, N + 1))
        q = n_step_of(N, n_alive)
        K = int(rng.integers(2, K_MAX + 1))
        headroom = n_alive - (0 if q == 8 else N // (q + 1)) - 1
        mode = i % 4        # deaths well inside the headroom / around it / most rays / every ray
        budget = [max(headroom // 2, 0), min(n_alive, 2 * headroom + 2), n_alive, n_alive][mode]
        cuts = np.sort(rng.integers(0, budget + 1, size=K))
        full = np.diff(np.concatenate([[0], cuts])).astype(np.int64)
        if mode == 3:
            full[int(rng.integers(0, K))] += n_alive - int(full.sum())        # the last ray dies inside the launch
        full = np.concatenate([full, np.zeros(8 - K, dtype=np.int64)])
        partial = np.array([int(rng.integers(0, f + 1)) for f in full])
        if i % 7 == 0:
            partial = full.copy()
        out.append((N, n_alive, q, K, full, partial))
    return out


def py_verdict(N, n_alive, q, K, deaths, own_last):
    """launch_verdict transcribed: the first iteration j > 0 whose n_step = clamp(N // n_alive, 1, 8) differs from q, or (own_last) the
    iteration in which the list runs empty"""
    alive = n_alive
    for j in range(K):
        if alive == 0:
            break
        if j > 0 and n_step_of(N, alive) != q:
            return 1, j
        alive -= min(int(deaths[j]), alive)
        if own_last and alive == 0:
            return 1, j
    return 0, K


def test_verdict_on_random_launches_and_on_partial_counts(ask):
    """10 000 random launches: the verdict equals its transcription; and with partial death vectors (element-wise <= the full one) of a
    launch that some ray survives, a violation under the partial counts is a violation under the full ones, no later (deaths only
    grow, and N // n_alive only grows as rays die).  When every ray dies inside the launch that does not hold: the reference stops
    at the empty list, and the example below is a launch that is fine although 60 of its 100 deaths look like a violation."""
    rng = np.random.default_rng(20240607)
    cases = random_launches(rng, 10000)
    lines = []
    for N, n_alive, q, K, full, partial in cases:
        for own_last in (0, 1):
            lines.append(f"V {N} {n_alive} {q} {K} {own_last} " + " ".join(map(str, full)))
            lines.append(f"V {N} {n_alive} {q} {K} {own_last} " + " ".join(map(str, partial)))
    rows = ask(lines)
    n_bad = n_pbad = 0
    for i, (N, n_alive, q, K, full, partial) in enumerate(cases):
        survivors = n_alive - int(full[:K].sum())
        for own_last in (0, 1):
            (bad, keep), (pbad, pkeep) = rows[4 * i + 2 * own_last:4 * i + 2 * own_last + 2]
            assert (bad, keep) == py_verdict(N, n_alive, q, K, full, own_last), (cases[i], own_last)
            assert keep <= K and pkeep <= K
            if pbad and (survivors > 0 or own_last):
                assert bad and keep <= pkeep, (cases[i], own_last)
                n_pbad += 1
            n_bad += bad
    assert 4000 < n_bad < 18000 and n_pbad > 1000      # the cases exercise both outcomes
    (bad, keep), (pbad, pkeep) = ask(["V 100 100 1 4 0 100 0 0 0 0 0 0 0", "V 100 100 1 4 0 60 0 0 0 0 0 0 0"])
    assert (bad, keep) == (0, 4) and (pbad, pkeep) == (1, 1)


def isqrt(x):
    s = 0
    while (s + 1) * (s + 1) <= x:
        s += 1
    return s


def parent_plan(N, n_alive, q, recent, room, cap_mid_max, cap_hi, own_last):
    """the sizing of k_render_compact before launch_plan.hpp existed, transcribed: K from the recent death rate, the caps, room"""
    headroom = n_alive - (0 if q == 8 else N // (q + 1)) - 1
    rate = recent + 4 * isqrt(recent) + 16
    K = headroom * 2 // (SAFETY_X2 * rate)
    cap_mid = min(8 * q, cap_mid_max)
    cap_samples = 8 if q == 1 else (cap_mid if q <= 4 else cap_hi)
    capK = min(cap_samples // q, K_MAX)
    K = capK if (q == 8 and not own_last) else min(K, capK)
    return min(K, room), capK, headroom


def test_plan_respects_caps_and_equals_the_rate_formula_without_a_forecast(ask):
    rng = np.random.default_rng(7)
    lines, meta = [], []
    for i in range(10000):
        N = int(rng.integers(2, 1 << int(rng.integers(2, 21))))
        q = int(rng.integers(1, 9))
        lo, hi = (0 if q == 8 else N // (q + 1)) + 1, N // q              # n_alive with clamp(N // n_alive, 1, 8) == q (k_render_compact's entry condition)
        if hi < lo:
            continue
        n_alive = int(rng.integers(lo, hi + 1))
        recent = int(rng.integers(0, max(n_alive // int(rng.integers(1, 64)), 1) + 1))
        room = int(rng.integers(0, 40))
        own_last = int(rng.integers(0, 2))
        kind = i % 3              # no forecast / all-zero forecast / a forecast of the order of the headroom
        headroom = n_alive - (0 if q == 8 else N // (q + 1)) - 1
        fc = np.zeros(8, dtype=np.int64) if kind < 2 else rng.integers(0, headroom // int(rng.integers(1, 9)) + 2, size=8)
        lines.append(f"P {N} {n_alive} {q} {recent} {room} 8 32 {own_last} {int(kind > 0)} " + " ".join(map(str, fc)))
        meta.append((N, n_alive, q, recent, room, own_last, kind, fc))
    rows = ask(lines)
    shrunk = 0
    for (N, n_alive, q, recent, room, own_last, kind, fc), (K, K_rate, headroom, rate, forecast) in zip(meta, rows):
        want, capK, hr = parent_plan(N, n_alive, q, recent, room, 8, 32, own_last)
        assert headroom == hr and rate == recent + 4 * isqrt(recent) + 16
        assert K_rate == want                                  # the death rate alone: the formula as it was
        assert K <= K_rate and K <= room and K <= capK and K <= K_MAX and K * q <= 32
        if kind < 2:
            # (an all-zero forecast could bind only below the 16-ray allowance, where the rate formula gives K < 2 anyway)
            assert K == want and forecast == 0, (N, n_alive, q, recent, room)
        else:
            # every verified iteration j = 1 .. K-1 sees forecast deaths D(j) + 4 sqrt(D(j)) + 16 within the headroom, and K is the largest such
            def fits(j):
                D = int(fc[:min(8, j * q)].sum())
                return D + 4 * isqrt(D) + 16 <= headroom
            if not (q == 8 and not own_last):
                assert all(fits(j) for j in range(1, K))
                assert K == K_rate or K < 1 or not fits(K)
                shrunk += K < K_rate
            else:
                assert K == K_rate
    assert shrunk > 300


def test_integer_square_root_is_exact(ask):
    """floor(sqrt(x)) around every kind of edge: small values, perfect squares and their neighbours up to 2^32 - 1, random values"""
    import math
    rng = np.random.default_rng(3)
    xs = list(range(0, 300)) + [v for r in (255, 256, 4095, 4096, 46340, 46341, 65535) for v in (r * r - 1, r * r, r * r + 1)]
    xs += [2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 31, 2 ** 32 - 1] + [int(v) for v in rng.integers(0, 2 ** 32, size=3000)]
    xs = [x for x in xs if 0 <= x < 2 ** 32]
    rows = ask([f"S {x}" for x in xs])
    assert [r[0] for r in rows] == [math.isqrt(x) for x in xs]


OWN_LAST = 2          # kPlanOwnLast


def test_launch_loop_equals_the_reference_loop_on_random_rays(ask):
    """3000 random trials, each the reference's loop (one iteration per pass) and the launch loop (loop_begin, then per launch
    truncate_launch / launch_verdict / finish_launch, as the kernels call them) over the same rays: a ray has M march samples and
    saturates after S.  The two end with the same schedule statistics, the same alive list and the same samples consumed per ray,
    whatever the flag word (0: one iteration per launch) and although the saturation forecast is noise; the launches stay within the
    host's bound; with the own-last flag the loop's last iteration is an ordinary launch.  The lower bounds on roll-backs and cut
    launches keep the trials from passing vacuously."""
    rng = np.random.default_rng(20241021)
    trials = []
    for i in range(3000):
        N = int(rng.integers(0, 1 << int(rng.integers(0, 15))))      # uniform below a random power of two <= 2^14
        max_steps = int(rng.integers(1, 201))
        flags = int(rng.integers(0, 16)) | int(rng.integers(0, 4) > 0)      # any word; multi-iteration launches allowed in 7 of 8
        shape = i % 4                                                # lifetimes: M < 4 / M < 300 / two thirds M < 5, the rest < 400 / M in 30..49, S <= 60
        trials.append((N, max_steps, flags, shape, int(rng.integers(0, 16)), int(rng.integers(0, 2 ** 62))))
    rows = ask(["L " + " ".join(map(str, t)) for t in trials])
    rollbacks = cut = prefix = one = 0
    for (N, max_steps, flags, *_), row in zip(trials, rows):
        want, got, (same_alive, same_used, launches, n_rb, n_cut, n_prefix, n_one, last_spec, ok) = row[:6], row[6:12], row[12:]
        assert got == want, (N, max_steps, flags, want, got)          # iters, samples_slots, step, last_n_alive, last_n_step, samples marched
        assert same_alive and same_used and ok, (N, max_steps, flags)
        assert launches <= 2 * max_steps + 16
        if flags & OWN_LAST:
            assert last_spec == 0, (N, max_steps, flags)
        if flags & 4:
            assert n_prefix == 0
        rollbacks, cut, prefix, one = rollbacks + n_rb, cut + n_cut, prefix + n_prefix, one + n_one
    assert rollbacks >= 100 and cut >= 500 and prefix > 0 and one > 0, (rollbacks, cut, prefix, one)
    seen = {t[2] for t in trials}
    assert 0 in seen and all({bool(f & b) for f in seen} == {False, True} for b in (1, 2, 4, 8))


def test_status_and_counter_words_round_trip_at_the_field_edges(ask):
    """pack_status / unpack_status and pack_fin / unpack_fin at both ends of every field: n_alive 0 and 2^31 - 1, 48-bit sample counts,
    24-bit iters and rollbacks, a 15-bit call tag; words of another call, no words yet, or a mix of two calls' words are not accepted."""
    status = [(s, d, n) for s in (0, 1, 2 ** 32 - 1) for d in (0, 1) for n in (0, 1, 2 ** 31 - 1)]
    assert ask([f"W {s} {d} {n}" for s, d, n in status]) == [list(t) for t in status]
    big48, big24 = 2 ** 48 - 1, 2 ** 24 - 1
    fins = [(m, sl, it, rb, la, ls, tag) for m, sl in ((0, 0), (big48, 0), (0, big48), (big48, big48), (24245331, 31415926535))
            for it, rb in ((0, 0), (big24, 0), (0, big24), (big24, big24)) for la, ls in ((0, 0), (2 ** 32 - 1, 8), (2 ** 31 - 1, 255))
            for tag in (0, 1, 0x7FFF)]
    rows = ask(["F " + " ".join(map(str, f)) + f" {(f[6] + 1) & 0x7FFF}" for f in fins])
    for f, row in zip(fins, rows):
        assert row == [1, 0, 0, 0] + list(f[:6]), f
