"""The launch arithmetic of the fused render loop (csrc/launch_plan.hpp: plan_launch, launch_verdict), compiled for the
host into a small stand-alone program that answers one query per input line.  No GPU: k_render_compact and this test share the one copy
of the code."""
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
#include "launch_plan.hpp"
using namespace ngp;
int main() {
    static_assert(kSpecK == 8 && kSpecSafetyX2 == 1 && kForecastBuckets == 8, "the test transcribes these");
    char kind;
    while (scanf(" %c", &kind) == 1) {
        unsigned N, n_alive, q, K, flag, a[8];
        if (kind == 'V') {
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
