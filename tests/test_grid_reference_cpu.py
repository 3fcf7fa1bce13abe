"""tests/grid_reference.py (the grid encoder in NumPy float64) checked without a GPU, and the per-entry comparison shown to have teeth.

Method.  The reference restates the operator independently of oracle/; here the two meet.  Its forward interpolation is compared with
the float32 C oracle on fp32 tables (2^-20 absolute for tables in +-0.5: the oracle rounds eight fp32 multiply-adds per feature), and
its scatter with the oracle's fp32 scatter under the same per-entry fp32 bound the GPU tests use.  Then the comparison itself is
tried on the bursts input of the GPU tests: a legitimate result -- every entry's contributions rounded to half and summed in
np.float16 one at a time in a random order, 2k roundings -- must pass on every entry, and each of five single-contribution mutations
must fail for at least the share of ALL contributions of a level that the GPU tests' launch condition promises (0.85).  The mutations
are applied to every contribution in turn, not to a sample, so the shares are exact.
"""
import functools

import numpy as np
import pytest

import grid_reference as GR
import helpers as Hh
from oracle import oracle as O

EDGE = 5


def _points(B, D, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, (B, D)).astype(np.float32)
    x[0] = 0.0
    x[1] = 1.0            # exactly 1 is in range
    x[2, 0] = 1.0000001   # out of range -> zeros
    x[3, 1] = -1e-7
    x[4] = 0.5
    return x


@pytest.mark.parametrize("align", [False, True], ids=["cell_centres", "align_corners"])
@pytest.mark.parametrize("gridtype", [0, 1], ids=["hash", "tiled"])
@pytest.mark.parametrize("D", [2, 3])
def test_reference_forward_matches_the_oracle(D, gridtype, align):
    L, log2T = (16, 19) if D == 3 else (12, 17)
    offsets, pls = GR.level_table(D, L, log2T, align_corners=align)
    o2, p2 = Hh.grid_offsets(input_dim=D, num_levels=L, log2_hashmap_size=log2T, desired_resolution=2048, align_corners=align)
    assert np.array_equal(offsets, o2) and pls == p2
    scale, res = GR.level_geometry(L, pls)
    for l in (0, 1, L // 2, L - 1):
        s, r = O.level_geometry(l, float(np.log2(pls)), 16)
        assert (np.float32(s), int(r)) == (scale[l], res[l])
    rng = np.random.default_rng(40 + D)
    emb = rng.uniform(-0.5, 0.5, (offsets[-1], 2)).astype(np.float32)
    x = _points(4000, D, seed=41)
    want, _ = Hh.oracle_grid_encode(x, emb, offsets, pls, gridtype=gridtype, align_corners=align)
    got = GR.forward(x, emb, offsets, pls, gridtype=gridtype, align_corners=align)
    err = np.abs(got - want.astype(np.float64)).reshape(len(x), L, 2).max(axis=(0, 2))
    print("worst |reference - oracle| per level:", " ".join(f"{e:.1e}" for e in err))
    assert err.max() <= 2.0 ** -20
    assert np.all(got[2] == 0) and np.all(got[3] == 0) and np.abs(got[:EDGE]).max() > 0.1


@pytest.mark.parametrize("D,gridtype,align", [(3, 0, False), (3, 1, True), (2, 0, True), (2, 1, False)])
def test_reference_scatter_matches_the_oracle(D, gridtype, align):
    L, log2T, C = (16, 19, 2) if D == 3 else (12, 17, 4)
    offsets, pls = GR.level_table(D, L, log2T, align_corners=align)
    x = GR.ray_points(60, 50, D, seed=50 + D)                   # ray order: the coarse levels' entries collect long runs
    x[:EDGE] = _points(EDGE, D, seed=0)
    B = len(x)
    rng = np.random.default_rng(51)
    g = rng.normal(size=(L, B, C)).astype(np.float32)
    g[:, 100:140] = 0                                           # points without a gradient emit nothing
    got = np.zeros((offsets[-1], C), np.float32)
    O.grid_encode_backward(g, x, np.zeros((offsets[-1], C), np.float32), offsets, got, B, D, C, L, float(np.log2(pls)), 16, False,
                           np.zeros((B, L * D * C), np.float32), np.zeros((B, D), np.float32), gridtype, align)
    E, W, inb = GR.corners(x, offsets, pls, gridtype=gridtype, align_corners=align)
    assert not inb[2] and not inb[3] and inb[:2].all()
    want, A, k, _ = GR.expected(E, W, inb, g, offsets)
    res = GR.compare_levels(got, want, A, k, offsets, np.float32)
    print("worst error / bound per level:", " ".join(f"{r[0]:.3f}" for r in res))
    for l, (ratio, bad, stray) in enumerate(res):
        assert len(bad) == 0 and len(stray) == 0 and ratio <= 1.0, (l, ratio, bad[:5], stray[:5])
    assert (k > 0).sum() > 10000 and k.max() > 50


# ---------------------------------------------------------------------------------------------------------------------------------
# the comparison has teeth
# ---------------------------------------------------------------------------------------------------------------------------------
BURSTS = ("bursts400", "bursts4000")
L_NERF, C_NERF = GR.NERF_LEVELS, GR.NERF_FEATURES


@functools.lru_cache(maxsize=None)
def _bursts(name):
    """the contributions of a bursts input of tests/test_grid_scatter_gpu.py, per level: (e [n], c [n, C], want, A, k, legit fp16 result)"""
    offsets, pls = GR.level_table(3, L_NERF, GR.NERF_LOG2_T)
    x = GR.nerf_points()
    g = GR.nerf_gradient(name)
    on = (g[0] != 0).any(axis=1)
    assert np.array_equal(on, (g != 0).any(axis=(0, 2)))
    E, W, inb = GR.corners(x[on], offsets, pls)                 # (a point's corners do not depend on the other points)
    g = g[:, on]
    rng = np.random.default_rng(7)
    levels = []
    for l in range(L_NERF):
        size = int(offsets[l + 1] - offsets[l])
        want, A, k = GR.scatter(E[l], W[l], inb, g[l], size)
        live = GR.live_points(inb, g[l])
        e = E[l][live].ravel()
        c = (W[l][live][:, :, None] * g[l][live].astype(np.float64)[:, None, :]).reshape(-1, C_NERF)
        # a legitimate fp16 result: each contribution rounded to half, added one at a time in a random order
        order = rng.permutation(len(e))
        order = order[np.argsort(e[order], kind="stable")]
        es, cs = e[order], c[order].astype(np.float16)
        rank = np.arange(len(es)) - np.searchsorted(es, es, side="left")
        legit = np.zeros((size, C_NERF), np.float16)
        for r in range(int(rank.max()) + 1):
            sel = rank == r
            legit[es[sel]] = legit[es[sel]] + cs[sel]           # (one contribution per entry and round: no duplicate indices)
        share = GR.detectable_share(E[l], W[l], inb, g[l], A, k, np.float16)
        levels.append(dict(e=e, c=c, want=want, A=A, k=k, legit=legit, share=share, size=size))
    return levels


def test_a_legitimate_fp16_sum_passes():
    for name in BURSTS:
        ratios = []
        for l, lv in enumerate(_bursts(name)):
            ratio, bad, stray = GR.compare(lv["legit"], lv["want"], lv["A"], lv["k"], np.float16)
            ratios.append(ratio)
            assert len(bad) == 0 and len(stray) == 0, (name, l, bad[:5], stray[:5])
        print(name, "worst error / bound per level:", " ".join(f"{r:.3f}" for r in ratios))
        assert 0 < max(ratios) <= 1.0


def _fails(lv, rows, values):
    """does the comparison fail on entries `rows` [n] when they read `values` [n, C] (float64)?  -> bool [n]"""
    bd = GR.bound(lv["A"], lv["k"], np.float16)[rows]
    over = (np.abs(values - lv["want"][rows]) > bd).any(axis=1)
    return over | ((lv["k"][rows] == 0) & (values != 0).any(axis=1))


MUTATIONS = ["dropped", "doubled", "moved_to_the_next_entry", "channels_swapped"]


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_one_wrong_contribution_fails(mutation):
    """every contribution of every level mutated in turn; per level, on the bursts input that serves it best, at least 0.85 must fail"""
    best = []
    for l in range(L_NERF):
        rates = {}
        for name in BURSTS:
            lv = _bursts(name)[l]
            e, c, got = lv["e"], lv["c"], lv["legit"].astype(np.float64)
            if mutation == "dropped":
                fails = _fails(lv, e, got[e] - c)
            elif mutation == "doubled":
                fails = _fails(lv, e, got[e] + c)
            elif mutation == "channels_swapped":
                fails = _fails(lv, e, got[e] - c + c[:, ::-1])
            else:
                nxt = (e + 1) % lv["size"]
                fails = _fails(lv, e, got[e] - c) | _fails(lv, nxt, got[nxt] + c)
            rates[name] = (float(fails.mean()), lv["share"])
        best.append(max(rates.values()))
    print(mutation, "failing share per level:", " ".join(f"{r:.2f}" for r, _ in best))
    print(mutation, "detectable share per level:", " ".join(f"{s:.2f}" for _, s in best))
    for l, (rate, share) in enumerate(best):
        assert rate >= 0.85, (mutation, l, rate)
        if mutation != "channels_swapped":                      # (a swap changes an entry by c0 - c1, not by c)
            assert rate >= share, (mutation, l, rate, share)    # |c| > 2 bound is sufficient, so no fewer than that share fail


def test_a_write_into_an_untouched_entry_fails():
    for name in BURSTS:
        for l, lv in enumerate(_bursts(name)):
            idle = np.flatnonzero(lv["k"] == 0)
            assert len(idle) > 0
            got = lv["legit"].copy()
            got[idle[len(idle) // 2], 1] = 2.0 ** -10
            ratio, bad, stray = GR.compare(got, lv["want"], lv["A"], lv["k"], np.float16)
            assert list(stray) == [idle[len(idle) // 2]], (name, l)


def test_the_launch_condition_of_the_gpu_tests_holds():
    """over the bursts inputs taken together every level has a detectable share of at least 0.85 (the dense input's share needs the
    whole batch and is checked where it is used, in tests/test_grid_scatter_gpu.py)"""
    shares = [max(_bursts(name)[l]["share"] for name in BURSTS) for l in range(L_NERF)]
    print("detectable share per level, best bursts input:", " ".join(f"{s:.2f}" for s in shares))
    assert min(shares) >= 0.85
