"""The table gradient of the grid encoder (grid_encode_backward, csrc/gridencoder.hip) per entry against a float64 scatter, on every
route an update can take: the LDS level, the binned scatter with the plain and the merging first pass, region overflow, the bin
reduce, and the run-combining atomics.

Method.  tests/grid_reference.py restates the operator in NumPy float64 and gives, per table entry, the exact sum `want`, the sum of
magnitudes A and the number of contributions k.  Every entry of every level must satisfy

    |got - want| <= R(k) u A + R(k) tiny,      R = 3k + 2, u = 2^-11, tiny = 2^-14 (fp16);  R = 2k + 6, u = 2^-24, tiny = 2^-126 (fp32)

with R read off the kernels (derivation in grid_reference's docstring), and an entry with k = 0 must read back as zero bits.  Nothing
is fitted to the kernels' output.  Each case prints the worst error / bound per level with the route that level took.

A lost, doubled or misfiled contribution c is certain to fail where |c| > 2 bound, which needs a small k.  So the inputs are a dense
gradient (every sample of 640 rays x 256 samples: few contributions per entry on the fine, hashed levels only) and two bursts
gradients (non-zero on isolated runs of 1 to 5 consecutive samples, one run per 400 and per 4000 samples: few contributions per entry
on every level, and zero gradients on both sides of each run for the run heads and tails of combine_runs and merge_cell_rows).  A
fourth input, runs of 6 to 16 samples (one per 4000), makes same-cell chains long enough for all four rounds of the segmented sums
of merge_cell_rows and most of combine_runs', which no run of five can reach.
Before a case launches anything it checks, from the reference alone, that on every level at least one bursts input has a detectable
share of 0.85 or more, and the dense input 0.75 or more on levels 10 and above.

The workspace decides the route: cases call ngp_grid_encode_backward through ctypes with a workspace of their own; cases where the
workspace is not the point go through the grid_encode wrapper.  NaN, inf and overflowing gradients are not in this module
(test_ops_gpu.py::test_grid_encode_backward_ray_ordered_batch has them).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import grid_reference as GR

pytestmark = pytest.mark.gpu

H = 16
KINDS = tuple(GR.NERF_KINDS)
SMALL_MAX_FLOATS, BIN_MIN_POINTS, BIN_MAX_ENTRIES, MERGE_MAX_RES = 15 * 1024, 128 * 1024, 128 * 4096, 1024


def _t(a, device):
    return torch.from_numpy(np.array(a, order="C")).to(device)       # a copy: the cached arrays are read-only


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _routes(offsets, res, B, C, dtype, binned, merging):
    """the route of each level as plan_grid_backward chooses it (for the printed table only)"""
    out = []
    for l in range(len(offsets) - 1):
        size = int(offsets[l + 1] - offsets[l])
        if size * C <= SMALL_MAX_FLOATS and B * 8 >= size * C * 16:
            out.append("lds")
        elif binned and dtype == np.float16 and C == 2 and B >= BIN_MIN_POINTS and size <= BIN_MAX_ENTRIES:
            out.append("bin-merge" if merging and res[l] <= MERGE_MAX_RES else "bin-plain")
        else:
            out.append("atomics")
    return out


def _report(name, got, want, A, k, offsets, dtype, routes):
    res = GR.compare_levels(got, want, A, k, offsets, dtype)
    print(f"{name}: worst error / bound per level: " + " ".join(f"{l}:{rt}:{r[0]:.3f}" for l, (rt, r) in enumerate(zip(routes, res))))
    worst = {}
    for rt, r in zip(routes, res):
        worst[rt] = max(worst.get(rt, 0.0), r[0])
    print(f"{name}: worst per route: " + " ".join(f"{rt}={v:.3f}" for rt, v in sorted(worst.items())))
    for l, (ratio, bad, stray) in enumerate(res):
        lo = int(offsets[l])
        assert len(stray) == 0, f"{name}: level {l} ({routes[l]}): untouched entries written, first {stray[:5]}: {got[lo + stray[:5]]}"
        assert len(bad) == 0 and ratio <= 1.0, (f"{name}: level {l} ({routes[l]}): {len(bad)} entries beyond the bound, worst ratio {ratio:.3f}; "
                                                f"first {bad[:5]} got {got[lo + bad[:5]]} want {want[lo + bad[:5]]} k {k[lo + bad[:5]]}")
    return res


def _backward(device, x, g, offsets, pls, dtype, gridtype=0, align=False, workspace="full"):
    """ngp_grid_encode_backward through ctypes.  x [B, D] f32, g [L, B, C].  workspace: "full", None (NULL) or a number of bytes.
    -> (table gradient as numpy [n, C], full workspace size)"""
    from nerfsafetyvalidation_amd import _lib
    lib = _lib.lib()
    L, B, C = g.shape
    D = x.shape[1]
    td = torch.float16 if dtype == np.float16 else torch.float32
    code = _lib.NGP_F16 if dtype == np.float16 else _lib.NGP_F32
    x_t, g_t = _t(x, device), _t(g, device).to(td)
    ge = torch.zeros(int(offsets[-1]), C, dtype=td, device=device)
    host = (ctypes.c_int32 * len(offsets))(*[int(o) for o in offsets])
    full = lib.ngp_grid_encode_backward_workspace(B, D, C, L, code)
    nbytes = full if workspace == "full" else (0 if workspace is None else int(workspace))
    work = torch.empty(nbytes, dtype=torch.uint8, device=device) if nbytes else None
    _lib.check(lib.ngp_grid_encode_backward(_lib.ptr(g_t), _lib.ptr(x_t), _lib.ptr(ge), host, _lib.ptr(ge), B, D, C, L, float(np.log2(pls)), H, 0,
                                            None, None, gridtype, int(align), code, _lib.ptr(work), nbytes, _lib.stream()), "grid_encode_backward")
    torch.cuda.synchronize()
    return ge.cpu().numpy(), full


def _through_wrapper(device, x, g, offsets, pls, dtype, gridtype=0, align=False):
    """the same through grid_encode's autograd function (its own workspace)"""
    from nerfsafetyvalidation_amd.gridencoder import grid_encode
    L, B, C = g.shape
    td = torch.float16 if dtype == np.float16 else torch.float32
    emb = torch.zeros(int(offsets[-1]), C, dtype=td, device=device, requires_grad=True)
    rows = _t(g.transpose(1, 0, 2), device).reshape(B, L * C).to(td)
    out = grid_encode(_t(x, device), emb, _t(np.asarray(offsets, np.int32), device), pls, H, False, gridtype, align)
    out.backward(rows)
    return emb.grad.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------------------
# the NeRF shape: D = 3, C = 2, L = 16, T = 2^19
# ---------------------------------------------------------------------------------------------------------------------------------
L3, C3 = GR.NERF_LEVELS, GR.NERF_FEATURES
B3 = GR.NERF_RAYS * GR.NERF_SAMPLES


@functools.lru_cache(maxsize=None)
def _nerf():
    offsets, pls = GR.level_table(3, L3, GR.NERF_LOG2_T)
    x = GR.nerf_points()
    E, W, inb = GR.corners(x, offsets, pls)
    assert 0 < (~inb).sum() < 1000                              # the far ends of a few rays leave [0, 1]
    _ro(x, E, W, inb, offsets)
    return dict(offsets=offsets, pls=pls, x=x, E=E, W=W, inb=inb, res=GR.level_geometry(L3, pls)[1])


@functools.lru_cache(maxsize=None)
def _nerf_gradient(kind):
    return _ro(GR.nerf_gradient(kind))[0]


@functools.lru_cache(maxsize=6)
def _nerf_expected(kind, B):
    """(want, A, k) over the whole table for the first B points"""
    n = _nerf()
    return _ro(*GR.expected(n["E"][:, :B], n["W"][:, :B], n["inb"][:B], _nerf_gradient(kind)[:, :B], n["offsets"])[:3])


@functools.lru_cache(maxsize=None)
def _nerf_shares(kind, B, dtype):
    n = _nerf()
    _, A, k = _nerf_expected(kind, B)
    g = _nerf_gradient(kind)
    off = n["offsets"]
    return [GR.detectable_share(n["E"][l, :B], n["W"][l, :B], n["inb"][:B], g[l, :B], A[off[l]:off[l + 1]], k[off[l]:off[l + 1]], dtype)
            for l in range(L3)]


def _launch_condition(B, dtype):
    """computed from the reference alone, before anything runs on the device"""
    sh = {kind: _nerf_shares(kind, B, dtype) for kind in KINDS}
    for kind in KINDS:
        print(f"detectable share per level, {kind}, B = {B}: " + " ".join(f"{s:.2f}" for s in sh[kind]))
    bursts = [max(sh["bursts400"][l], sh["bursts4000"][l]) for l in range(L3)]
    assert min(bursts) >= 0.85, bursts
    assert min(sh["dense"][10:]) >= 0.75, sh["dense"]
    # runs4000 is there for chains of neighbouring samples in one cell that are longer than a bursts input can make them
    n = _nerf()
    live = GR.live_points(n["inb"][:B], _nerf_gradient("runs4000")[0, :B])
    same = live[1:] & live[:-1] & (n["E"][0, 1:B] == n["E"][0, :B - 1]).all(axis=1)
    edges = np.flatnonzero(np.diff(np.concatenate(([0], same.astype(np.int8), [0]))))
    assert (edges[1::2] - edges[::2]).max() + 1 >= 12


def _run_nerf(device, name, B, dtype, workspace, binned, merging, wrapper=False):
    n = _nerf()
    _launch_condition(B, dtype)
    routes = _routes(n["offsets"], n["res"], B, C3, dtype, binned, merging)
    for kind in KINDS:
        g = _nerf_gradient(kind)[:, :B].astype(dtype)
        if wrapper:
            got = _through_wrapper(device, n["x"][:B], g, n["offsets"], n["pls"], dtype)
        else:
            ws = workspace(B) if callable(workspace) else workspace
            got, _ = _backward(device, n["x"][:B], g, n["offsets"], n["pls"], dtype, workspace=ws)
        _report(f"{name}/{kind}", got, *_nerf_expected(kind, B), n["offsets"], dtype, routes)
    return routes


def _per_level(B):
    from nerfsafetyvalidation_amd import _lib
    full = _lib.lib().ngp_grid_encode_backward_workspace(B, 3, C3, L3, _lib.NGP_F16)
    assert full > 0 and full % L3 == 0
    return full // L3


def _env(monkeypatch, merging, fill_pct=None):
    monkeypatch.delenv("NGP_GRID_MERGE_MIN", raising=False)
    monkeypatch.delenv("NGP_GRID_BIN_FILL_PCT", raising=False)
    if merging:
        monkeypatch.setenv("NGP_GRID_MERGE_MIN", "0")
    if fill_pct is not None:
        monkeypatch.setenv("NGP_GRID_BIN_FILL_PCT", str(fill_pct))


@pytest.mark.parametrize("merging", [False, True], ids=["plain_first_pass", "merging_first_pass"])
def test_full_workspace(device, monkeypatch, merging):
    """every level but the LDS one through the bins in one group"""
    _env(monkeypatch, merging)
    routes = _run_nerf(device, "full", B3, np.float16, "full", True, merging)
    assert routes[0] == "lds" and routes[1] != "lds" and "atomics" not in routes
    assert ("bin-merge" in routes) == merging and "bin-plain" in routes


@pytest.mark.parametrize("merging", [False, True], ids=["plain_first_pass", "merging_first_pass"])
def test_regions_sized_for_a_fifth_of_the_updates(device, monkeypatch, merging):
    """NGP_GRID_BIN_FILL_PCT=20: the dense input's records exceed the regions and the excess goes straight to the table"""
    _env(monkeypatch, merging, fill_pct=20)
    n = _nerf()
    # A workgroup of the first pass (1024 consecutive points) emits at least one record per entry it touches, merging or not; the
    # regions of a level hold at most level_records = (workspace of a level - its fill counters) / 8 of them.
    level_records = (_per_level(B3) - 128 * 32 * 32 * 4) // 8
    assert 0 < level_records < B3 * 8 * 0.7
    live = GR.live_points(n["inb"], _nerf_gradient("dense")[L3 - 1].astype(np.float32))
    wg = (np.flatnonzero(live) // 1024).astype(np.int64)
    pairs = np.unique(wg[:, None] * (1 << 20) + n["E"][L3 - 1][live].astype(np.int64))
    print(f"finest level: at least {len(pairs)} records for regions of {level_records}")
    assert len(pairs) > level_records
    _run_nerf(device, "fill20", B3, np.float16, "full", True, merging)


@pytest.mark.parametrize("levels,merging", [(1, False), (3, False), (4, False), (3, True), (2, True)],
                         ids=["one_level", "three_levels", "four_levels", "three_levels_merging", "two_levels_merging"])
def test_smaller_workspace_takes_the_levels_in_groups(device, monkeypatch, levels, merging):
    """15 binned levels (12 of them merging when that is forced) in groups of 1, 3, 4 and 2: even and uneven splits, and a group never
    mixes the two variants of the first pass"""
    _env(monkeypatch, merging)
    routes = _run_nerf(device, f"{levels}-level workspace", B3, np.float16, lambda B: levels * _per_level(B), True, merging)
    assert routes.count("bin-merge") == (12 if merging else 0) and routes.count("bin-plain") == (3 if merging else 15)


@pytest.mark.parametrize("workspace", ["one_byte_short_of_a_level", "null"])
def test_without_a_usable_workspace_every_level_takes_the_atomics(device, monkeypatch, workspace):
    _env(monkeypatch, False)
    ws = (lambda B: _per_level(B) - 1) if workspace != "null" else None
    routes = _run_nerf(device, workspace, B3, np.float16, ws, False, False)
    assert routes == ["lds"] + ["atomics"] * 15


def test_fp32_table_lds_level_and_float_atomics(device, monkeypatch):
    _env(monkeypatch, False)
    routes = _run_nerf(device, "fp32", B3, np.float32, None, False, False, wrapper=True)
    assert routes == ["lds"] + ["atomics"] * 15


@pytest.mark.parametrize("B", [131071, 131072, 131072 + 513])
def test_batch_sizes_around_the_switch_to_the_bins(device, monkeypatch, B):
    """B = 128 k switches the binned scatter on; neither 131071 nor 131585 fills its last workgroup (1024, 256 or 64 lanes)"""
    _env(monkeypatch, False)
    from nerfsafetyvalidation_amd import _lib
    full = _lib.lib().ngp_grid_encode_backward_workspace(B, 3, C3, L3, _lib.NGP_F16)
    assert (full > 0) == (B >= BIN_MIN_POINTS)
    _run_nerf(device, f"B={B}", B, np.float16, "full", full > 0, False)


# ---------------------------------------------------------------------------------------------------------------------------------
# small batches: no LDS level, no bins
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float16, np.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("B", [1, 63, 65, 1000])
def test_small_batches(device, monkeypatch, dtype, B):
    _env(monkeypatch, False)
    offsets, pls = GR.level_table(3, L3, 19)
    rng = np.random.default_rng(77)
    x = rng.uniform(0, 1, (1000, 3)).astype(np.float32)
    x[5] = (0.5, 1.5, 0.5)           # outside [0, 1]
    x[7] = 1.0                       # exactly 1: in range
    x[61, 2] = -1e-7
    x = x[:B]
    g = GR.dense_gradient(1000, L3, C3, seed=78)[:, :B].astype(dtype)
    E, W, inb = GR.corners(x, offsets, pls)
    want, A, k, shares = GR.expected(E, W, inb, g, offsets, dtype)
    print("detectable share per level:", " ".join(f"{s:.2f}" for s in shares))
    assert B == 1 or min(shares) >= 0.85                    # (a single point has eight contributions per level: shares in eighths)
    routes = _routes(offsets, GR.level_geometry(L3, pls)[1], B, C3, dtype, False, False)
    assert routes == ["atomics"] * L3
    got = _through_wrapper(device, x, g, offsets, pls, dtype)
    _report(f"B={B}", got, want, A, k, offsets, dtype, routes)
    assert (k > 0).sum() > 0 and np.abs(got).max() > 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 2-D grids: several LDS levels for every C, both grid types, align_corners with a point at exactly 1
# ---------------------------------------------------------------------------------------------------------------------------------
L2, B2 = 12, 700 * 200


@functools.lru_cache(maxsize=2)
def _plane(gridtype, align):
    offsets, pls = GR.level_table(2, L2, 17, align_corners=align)
    x = GR.ray_points(700, 200, 2, seed=202, t_max=0.3)
    x[5] = 1.0                       # in range; with align_corners it indexes grid point `resolution`, which only the modulo brings back
    x[9] = (0.25, 1.5)
    E, W, inb = GR.corners(x, offsets, pls, gridtype=gridtype, align_corners=align)
    assert inb[5] and not inb[9]
    _ro(x, E, W, inb, offsets)
    return dict(offsets=offsets, pls=pls, x=x, E=E, W=W, inb=inb, res=GR.level_geometry(L2, pls)[1])


@pytest.mark.parametrize("dtype,C,gridtype,align", [(np.float16, 2, 0, False), (np.float16, 2, 1, True), (np.float16, 4, 0, True), (np.float16, 4, 1, False),
                                                    (np.float16, 8, 0, False), (np.float16, 8, 1, True), (np.float32, 2, 0, True), (np.float32, 2, 1, False)])
def test_two_dimensional_grids(device, monkeypatch, dtype, C, gridtype, align):
    _env(monkeypatch, False)
    p = _plane(gridtype, align)
    assert B2 >= BIN_MIN_POINTS
    routes = _routes(p["offsets"], p["res"], B2, C, dtype, True, False)
    assert routes.count("lds") >= 3, routes
    gradients = (("dense", GR.dense_gradient(B2, L2, C, seed=5)), ("bursts400", GR.burst_gradient(B2, L2, C, B2 // 400, seed=6)),
                 ("bursts4000", GR.burst_gradient(B2, L2, C, B2 // 4000, seed=7)))
    ref = {kind: GR.expected(p["E"], p["W"], p["inb"], g.astype(dtype), p["offsets"], dtype) for kind, g in gradients}
    for kind, _ in gradients:
        print(f"detectable share per level, {kind}: " + " ".join(f"{s:.2f}" for s in ref[kind][3]))
    # (level 0 holds 289 entries: 35 runs already leave some of them with a dozen contributions; levels 1 and 2 are LDS levels for every C)
    assert routes[2] == "lds" and min(max(ref["bursts400"][3][l], ref["bursts4000"][3][l]) for l in range(1, L2)) >= 0.85
    for kind, g in gradients:
        got = _through_wrapper(device, p["x"], g.astype(dtype), p["offsets"], p["pls"], dtype, gridtype, align)
        _report(f"2-D/{kind}", got, *ref[kind][:3], p["offsets"], dtype, routes)


# ---------------------------------------------------------------------------------------------------------------------------------
# one exact case
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["full_plain", "full_merging", "three_levels", "null"])
def test_exactly_representable_sums_are_exact_on_every_route(device, monkeypatch, route):
    """L = 8 up to resolution 2048: per_level_scale is exactly 2, every scale an integer, and (0.5, 0.5, 0.5) a grid vertex of every
    level: all the weight of a point falls on one entry.  The gradient is +-2^-3 on 64 of 200 000 points (in different workgroups) and
    zero elsewhere, so every partial sum on every route is exactly representable: the table gradient must equal the float64 sum bit
    for bit, and the seven other corners of the cell, which receive updates of value zero, must stay zero."""
    _env(monkeypatch, route == "full_merging")
    L, B = 8, 200_000
    offsets, pls = GR.level_table(3, L, 19)
    assert pls == 2.0
    x = np.full((B, 3), 0.5, np.float32)
    rng = np.random.default_rng(9)
    at = np.arange(64) * (B // 64) + rng.integers(0, 1024, 64)
    assert len(np.unique(at // 1024)) == 64 and at.max() < B
    g = np.zeros((L, B, C3), np.float16)
    g[:, at] = rng.choice([-0.125, 0.125], (L, 64, C3))
    E, W, inb = GR.corners(x[at], offsets, pls)
    assert np.all(W[:, :, 0] == 1.0) and np.all(W[:, :, 1:] == 0.0) and len(np.unique(E[:, 0], axis=0)) == L
    want, A, k, _ = GR.expected(E, W, inb, g[:, at], offsets)
    assert (k > 0).sum() == 8 * L and (want != 0).any(axis=1).sum() <= L and np.all(want * 8 == np.round(want * 8))
    full_per_level = None
    if route == "three_levels":
        from nerfsafetyvalidation_amd import _lib
        full = _lib.lib().ngp_grid_encode_backward_workspace(B, 3, C3, L, _lib.NGP_F16)
        assert full % L == 0
        full_per_level = 3 * (full // L)
    ws = {"full_plain": "full", "full_merging": "full", "three_levels": full_per_level, "null": None}[route]
    got, _ = _backward(device, x, g, offsets, pls, np.float16, workspace=ws)
    assert got.dtype == np.float16
    diff = np.flatnonzero((got.view(np.uint16) != want.astype(np.float16).view(np.uint16)).any(axis=1))
    assert len(diff) == 0, (route, diff[:8], got[diff[:8]], want[diff[:8]])
    assert np.array_equal(got.astype(np.float64), want) and (got != 0).any()
