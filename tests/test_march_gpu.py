"""The occupancy march (csrc/occupancy.hpp: march_rays, march_rays_train and, through the shared header, the render loop) against the
CPU oracle's plain cell walk on the hand-built grids, bounds and rays of march_cases.py.  Every comparison is on uint32 views and exact:
there is no tolerance in this file.  test_march_cases_cpu.py checks, on the oracle alone, that these cases take samples in every ray
family, fill step budgets and cross cascade surfaces inside cells, so that equality here is not vacuous.

march_rays_train picks one of four kernel forms (ngp_march_rays_train): with lin = N >= 1024 and the grid has derived copies
(ngp_occupancy_lin_bytes > 0, bitfield 8-byte aligned), trace = lin and N <= 16384 and max_steps <= 1024,
    kPlain  not lin                         kLin    lin, no trace
    kWave   trace and dt_gamma == 0         kTraced trace and dt_gamma != 0
The 2048 rays of the table's rows take (FORMS, in the order of march_cases.CONFIGS):
    (1, 1, 128, 1024, 0)        kWave       (2, 2, 128, 1024, 1/128)    kTraced     (4, 3, 128, 512, 0)     kPlain (above the coarse cap)
    (8, 4, 64, 1024, 0)         kWave       (16, 5, 64, 1024, 1/256)    kTraced     (1.5, 2, 64, 256, 0)    kWave
    (3, 3, 32, 128, 0)          kWave       (1, 1, 16, 64, 0)           kWave       (8, 8, 8, 128, 0)       kWave
    (1, 1, 8, 64, 0)            kPlain (512 cells: no copies)           (2, 2, 64, 1100, 0)     kLin (max_steps > 1024)
and every row again with 1000 of the rays (kPlain whatever the grid), two rows with the bitfield at an odd address (kPlain).
march_rays takes the derived-copy kernel when the grid has copies and the bitfield is aligned (USE_OCCUPANCY_LIN), else the plain one.
"""
import numpy as np
import pytest
import torch

import march_cases as MC
from nerfsafetyvalidation_amd import _lib

pytestmark = pytest.mark.gpu

CONFIG_IDS = [MC.config_id(c) for c in MC.CONFIGS]
FORMS = ("kWave", "kTraced", "kPlain", "kWave", "kTraced", "kWave", "kWave", "kWave", "kWave", "kPlain", "kLin")
GRID_SHAPES = sorted({(c.C, c.H) for c in MC.CONFIGS})
NGP_EINVAL = -1


def _t(x, device):
    return torch.from_numpy(np.array(x, order="C")).to(device)          # (a copy: the cases are read-only arrays)


def _np(t):
    return MC.bits(t.cpu().numpy())


def train_form(lin_bytes, aligned, N, max_steps, dt_gamma):
    """the dispatch rule of ngp_march_rays_train"""
    lin = N >= 1024 and lin_bytes > 0 and aligned
    trace = lin and N <= 16384 and max_steps <= 1024
    return "kPlain" if not lin else ("kLin" if not trace else ("kWave" if dt_gamma == 0 else "kTraced"))


# ---------------------------------------------------------------------------------------------------------------- derived copies
def test_occupancy_lin_bytes(device):
    """0 exactly for the grids without copies: above the coarse cap (3, 128), fewer than 4096 cells (1, 8), H below 8, C above 8"""
    L = _lib.lib()
    for C, H in GRID_SHAPES + [(1, 4), (8, 4), (9, 8), (9, 64), (2, 8), (8, 128), (1, 256), (2, 256), (4, 128), (1, 48), (2, 100), (1, 1024)]:
        assert L.ngp_occupancy_lin_bytes(C, H) == MC.lin_bytes(C, H), (C, H)
    assert [s for s in GRID_SHAPES if MC.lin_bytes(*s) == 0] == [(1, 8), (3, 128)]
    assert MC.lin_bytes(1, 4) == 0 and MC.lin_bytes(9, 8) == 0 and MC.lin_bytes(9, 64) == 0
    assert MC.lin_bytes(2, 128) == 512 * 1024 + 8192 and MC.lin_bytes(1, 16) == 512 + 8 and MC.lin_bytes(8, 8) == 512 + 8


def _build_lin(device, bitfield, C, H):
    """ngp_build_occupancy_lin into a buffer pre-filled with 0xAA -> (linear copy, the bytes between, coarse copy) as uint8 arrays"""
    L = _lib.lib()
    nbytes = L.ngp_occupancy_lin_bytes(C, H)
    cells = C * H ** 3
    assert nbytes == MC.ceil256(cells // 8) + cells // 512
    out = torch.full((nbytes + 256,), 0xAA, dtype=torch.uint8, device=device)
    bf = _t(bitfield, device)
    assert bf.data_ptr() % 8 == 0 and out.data_ptr() % 256 == 0
    _lib.check(L.ngp_build_occupancy_lin(_lib.ptr(bf), C, H, _lib.ptr(out), nbytes, _lib.stream()), "build_occupancy_lin")
    got = out.cpu().numpy()
    assert (got[nbytes:] == 0xAA).all()                                      # nothing past the size the library states
    return got[:cells // 8], got[cells // 8:MC.ceil256(cells // 8)], got[MC.ceil256(cells // 8):nbytes]


@pytest.mark.parametrize("C,H", GRID_SHAPES, ids=lambda v: str(v))
def test_derived_copies_hold_the_bitfields_cells(device, C, H):
    """linear bit (level, z, y, x) == bitfield bit level * H^3 + morton3D(x, y, z) for every cell; coarse bit (level, bz, by, bx), at
    byte ceil256(C H^3 / 8), == any cell of the 4x4x4 block set.  A wrong coarse bit would make the march skip occupied space."""
    L = _lib.lib()
    if MC.lin_bytes(C, H) == 0:
        out = torch.full((4096,), 0xAA, dtype=torch.uint8, device=device)
        bf = _t(MC.grid("random", C, H)[1], device)
        assert L.ngp_build_occupancy_lin(_lib.ptr(bf), C, H, _lib.ptr(out), 4096, _lib.stream()) == NGP_EINVAL
        assert (out.cpu().numpy() == 0xAA).all()
        return
    for g in MC.GRIDS:
        occ, bitfield = MC.grid(g, C, H)
        lin, gap, coarse = _build_lin(device, bitfield, C, H)
        want_lin, want_coarse = MC.lin_reference(occ)
        assert np.array_equal(lin, want_lin), g
        assert np.array_equal(coarse, want_coarse), g
        assert (gap == 0xAA).all()
    B = H // 4
    for cell in MC.corner_cells(C, H):                                       # one cell set: one bit in each copy, at the stated place
        level, x, y, z = cell
        lin, _, coarse = _build_lin(device, MC.single_bit(C, H, cell)[1], C, H)
        fine = level * H ** 3 + (z * H + y) * H + x
        block = level * B ** 3 + ((z // 4) * B + y // 4) * B + x // 4
        assert np.flatnonzero(lin).tolist() == [fine // 8] and lin[fine // 8] == 1 << (fine % 8), cell
        assert np.flatnonzero(coarse).tolist() == [block // 8] and coarse[block // 8] == 1 << (block % 8), cell


# ---------------------------------------------------------------------------------------------------------------- march_rays
def _march_rays_case(device, cfg, bitfield_dev, bitfield, forms, n_steps, monkeypatch):
    """three consecutive march_rays calls per n_step, the oracle's composite_rays (zero density) moving rays_t in between: the
    second and third calls resume mid-ray.  Every row is compared, the zero-filled tails included.
    -> n_step: the oracle's samples per call"""
    from nerfsafetyvalidation_amd import raymarching
    from nerfsafetyvalidation_amd.raymarching import raymarching as rm
    r = MC.rays(cfg.bound, cfg.H)
    dev = [_t(a, device) for a in (r.rays_o, r.rays_d, r.nears, r.fars)]
    seen = {}
    for n_step in n_steps:
        seen[n_step] = []
        alive = np.random.default_rng(7).permutation(MC.N_RAYS)[:MC.N_RAYS // 2].astype(np.int32)      # a shuffled half
        rays_t = r.nears.copy()
        for call in range(3):
            n_alive = alive.shape[0]
            if n_alive == 0:
                break
            want = MC.oracle_march(cfg, bitfield, r, alive, rays_t, n_step)
            seen[n_step].append(int((want[2][:, 0] > 0).sum()))
            for lin in forms:
                monkeypatch.setattr(rm, "USE_OCCUPANCY_LIN", lin)
                got = raymarching.march_rays(n_alive, n_step, _t(alive, device), _t(rays_t, device), dev[0], dev[1], cfg.bound, bitfield_dev,
                                             cfg.C, cfg.H, dev[2], dev[3], 128, cfg.perturb, cfg.dt_gamma, cfg.max_steps)
                for name, g, w in zip(("xyzs", "dirs", "deltas"), got, want):
                    assert g.shape == w.shape
                    g = _np(g)
                    if not np.array_equal(g, MC.bits(w)):
                        row = int(np.flatnonzero((g != MC.bits(w)).any(-1))[0])
                        ray = int(alive[row // n_step]) if row < n_alive * n_step else -1
                        raise AssertionError("%s differs (derived copies: %s, n_step %d, call %d): first at row %d = sample %d of ray %d; "
                                             "got %r, oracle %r; oracle xyz %r dt %r, rays_t %r"
                                             % (name, lin, n_step, call, row, row % n_step, ray, got[("xyzs", "dirs", "deltas").index(name)][row]
                                                .cpu().numpy(), w[row], want[0][row], want[2][row], rays_t[ray] if ray >= 0 else None))
            alive, rays_t = MC.oracle_advance(alive, rays_t, want[2], n_step)
    return seen


@pytest.mark.parametrize("grid_name", MC.GRIDS)
@pytest.mark.parametrize("ci", range(len(MC.CONFIGS)), ids=CONFIG_IDS)
def test_march_rays_equals_the_cell_walk(device, ci, grid_name, monkeypatch):
    from nerfsafetyvalidation_amd.raymarching import raymarching as rm
    cfg = MC.CONFIGS[ci]
    bitfield = MC.grid(grid_name, cfg.C, cfg.H)[1]
    bf = _t(bitfield, device)
    has_copies = _lib.lib().ngp_occupancy_lin_bytes(cfg.C, cfg.H) > 0
    assert has_copies == (MC.lin_bytes(cfg.C, cfg.H) > 0) and bf.data_ptr() % 8 == 0
    assert (rm._occupancy_lin(bf, cfg.C, cfg.H) is not None) == has_copies          # which kernel USE_OCCUPANCY_LIN = True selects
    seen = _march_rays_case(device, cfg, bf, bitfield, (True, False), (1, 3, 64), monkeypatch)
    print("%s %s: samples per call %s" % (MC.config_id(cfg), grid_name, seen))
    if grid_name in ("random", "blocks"):                                            # the resumed calls take samples too
        assert len(seen[1]) == 3 and len(seen[3]) == 3 and min(seen[1] + seen[3]) > 100 and seen[64][0] > 100


# ---------------------------------------------------------------------------------------------------------------- march_rays_train
def _train_case(device, cfg, bitfield_dev, rays_o, rays_d, nears, fars, want):
    from nerfsafetyvalidation_amd import raymarching
    N = rays_o.shape[0]
    counter = torch.zeros(2, dtype=torch.int32, device=device)
    gx, gd, gdl, grays = raymarching.march_rays_train(_t(rays_o, device), _t(rays_d, device), cfg.bound, bitfield_dev, cfg.C, cfg.H,
                                                      _t(nears, device), _t(fars, device), counter, -1, bool(cfg.perturb), 128, True,
                                                      cfg.dt_gamma, cfg.max_steps)
    assert np.array_equal(counter.cpu().numpy(), want.counter), (counter.cpu().numpy(), want.counter)
    table = grays.cpu().numpy()
    if not np.array_equal(table, want.rays):
        n = int(np.flatnonzero((table != want.rays).any(-1))[0])
        raise AssertionError("rays table differs first at ray %d: got %r, oracle %r" % (n, table[n], want.rays[n]))
    m = int(want.counter[0])
    m_pad = MC.padded(m)
    assert gx.shape == (m_pad, 3) and gd.shape == (m_pad, 3) and gdl.shape == (m_pad, 2)
    owner = np.repeat(want.rays[:, 0], want.rays[:, 2])
    for name, g, w in (("xyzs", gx, want.xyzs), ("dirs", gd, want.dirs), ("deltas", gdl, want.deltas)):
        g = _np(g)
        assert not g[m:].any(), name                                                 # the padding rows read zero
        if not np.array_equal(g[:m], MC.bits(w)):
            row = int(np.flatnonzero((g[:m] != MC.bits(w)).any(-1))[0])
            n = int(owner[row])
            raise AssertionError("%s differs first at row %d = sample %d of ray %d (%d samples): got %r, oracle %r; oracle xyz %r deltas %r"
                                 % (name, row, row - want.rays[n, 1], n, want.rays[n, 2], g[row].view(np.float32), w[row], want.xyzs[row],
                                    want.deltas[row]))
    assert N == want.rays.shape[0]


@pytest.mark.parametrize("grid_name", MC.GRIDS)
@pytest.mark.parametrize("ci", range(len(MC.CONFIGS)), ids=CONFIG_IDS)
def test_march_rays_train_equals_the_cell_walk(device, ci, grid_name):
    cfg = MC.CONFIGS[ci]
    L = _lib.lib()
    bitfield = MC.grid(grid_name, cfg.C, cfg.H)[1]
    bf = _t(bitfield, device)
    r = MC.rays(cfg.bound, cfg.H)
    # the inputs of the dispatch rule, and the form they select
    lin_bytes = L.ngp_occupancy_lin_bytes(cfg.C, cfg.H)
    assert lin_bytes == MC.lin_bytes(cfg.C, cfg.H) and bf.data_ptr() % 8 == 0 and MC.N_RAYS == 2048
    assert train_form(lin_bytes, True, MC.N_RAYS, cfg.max_steps, cfg.dt_gamma) == FORMS[ci]
    _train_case(device, cfg, bf, r.rays_o, r.rays_d, r.nears, r.fars, MC.train_reference(ci, grid_name))
    # 1000 of the same rays (every other one): below 1024, the plain form whatever the grid
    sub = MC.subset(r, np.arange(0, MC.N_RAYS, 2)[:1000])
    assert train_form(lin_bytes, True, 1000, cfg.max_steps, cfg.dt_gamma) == "kPlain"
    want = MC.oracle_train(cfg, bitfield, *sub)
    if grid_name in ("random", "blocks"):
        assert want.counter[0] > 5000
    _train_case(device, cfg, bf, *sub, want)


@pytest.mark.parametrize("ci", [3, 5], ids=[CONFIG_IDS[3], CONFIG_IDS[5]])
def test_bitfield_at_an_odd_address_takes_the_plain_kernels(device, ci, monkeypatch):
    """the derived copies are built with 8-byte loads of the bitfield: a bitfield that is not 8-byte aligned has none, in both operators"""
    from nerfsafetyvalidation_amd.raymarching import raymarching as rm
    cfg = MC.CONFIGS[ci]
    bitfield = MC.grid("random", cfg.C, cfg.H)[1]
    big = torch.zeros(bitfield.shape[0] + 16, dtype=torch.uint8, device=device)
    bf = big[1:1 + bitfield.shape[0]]
    bf.copy_(_t(bitfield, device))
    assert bf.data_ptr() % 8 == 1 and bf.is_contiguous()
    lin_bytes = _lib.lib().ngp_occupancy_lin_bytes(cfg.C, cfg.H)
    assert lin_bytes > 0 and FORMS[ci] == "kWave" and train_form(lin_bytes, False, MC.N_RAYS, cfg.max_steps, cfg.dt_gamma) == "kPlain"
    assert rm._occupancy_lin(bf, cfg.C, cfg.H) is None
    r = MC.rays(cfg.bound, cfg.H)
    _train_case(device, cfg, bf, r.rays_o, r.rays_d, r.nears, r.fars, MC.train_reference(ci, "random"))
    seen = _march_rays_case(device, cfg, bf, bitfield, (True,), (3,), monkeypatch)
    assert len(seen[3]) == 3 and min(seen[3]) > 100
    assert not big[0].item() and not big[1 + bitfield.shape[0]:].any().item()


# ---------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("H", [48, 100])
def test_a_grid_size_that_is_no_power_of_two_is_refused_on_the_host(device, H):
    """morton3D(x, y, z) exceeds H^3 for such an H (march_cases.pack refuses it too): the march would read, and mark_untrained_grid
    write, past the grid.  Every entry point returns NGP_EINVAL before it launches anything, names the grid size, and leaves its
    outputs as they were.  (All buffers are full size all the same.)"""
    L = _lib.lib()
    C, N, n_step, max_steps = 2, 64, 2, 64
    cells = C * H ** 3
    assert cells % 8 == 0 and int(MC.morton3D(H - 1, H - 1, H - 1)) >= H ** 3
    s = _lib.stream()
    f = lambda *shape: torch.full(shape, 7.0, dtype=torch.float32, device=device)      # noqa: E731
    untouched = lambda *ts: all(bool((t == 7).all()) for t in ts)                      # noqa: E731

    def refused(rc, what):
        msg = L.ngp_last_error().decode()
        assert rc == NGP_EINVAL, (what, rc)
        assert what in msg and "H=%d" % H in msg and "power of two" in msg and "morton3D" in msg, msg

    bitfield = torch.zeros(cells // 8, dtype=torch.uint8, device=device)
    rays_o, rays_d = torch.zeros(N, 3, device=device), torch.ones(N, 3, device=device)
    nears, fars = torch.full((N,), 0.1, device=device), torch.full((N,), 1.0, device=device)
    alive = torch.arange(N, dtype=torch.int32, device=device)
    xyzs, dirs, deltas = f(N * max_steps, 3), f(N * max_steps, 3), f(N * max_steps, 2)
    M_padded = N * n_step
    refused(L.ngp_march_rays(N, n_step, _lib.ptr(alive), _lib.ptr(nears), _lib.ptr(rays_o), _lib.ptr(rays_d), 1.0, 0.0, max_steps, C, H,
                             _lib.ptr(bitfield), _lib.ptr(nears), _lib.ptr(fars), _lib.ptr(xyzs), _lib.ptr(dirs), _lib.ptr(deltas), 0, M_padded,
                             s), "march_rays")
    lin = torch.zeros(1 << 20, dtype=torch.uint8, device=device)
    refused(L.ngp_march_rays_lin(N, n_step, _lib.ptr(alive), _lib.ptr(nears), _lib.ptr(rays_o), _lib.ptr(rays_d), 1.0, 0.0, max_steps, C, H,
                                 _lib.ptr(bitfield), _lib.ptr(nears), _lib.ptr(fars), _lib.ptr(xyzs), _lib.ptr(dirs), _lib.ptr(deltas), 0,
                                 M_padded, _lib.ptr(lin), s), "march_rays")
    table = torch.full((N, 3), 7, dtype=torch.int32, device=device)
    counter = torch.full((2,), 7, dtype=torch.int32, device=device)
    ws_bytes = L.ngp_march_rays_train_workspace(N)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
    refused(L.ngp_march_rays_train(_lib.ptr(rays_o), _lib.ptr(rays_d), _lib.ptr(bitfield), 1.0, 0.0, max_steps, N, C, H, N * max_steps,
                                   _lib.ptr(nears), _lib.ptr(fars), _lib.ptr(xyzs), _lib.ptr(dirs), _lib.ptr(deltas), _lib.ptr(table),
                                   _lib.ptr(counter), 0, _lib.ptr(ws), ws_bytes, s), "march_rays_train")
    assert untouched(xyzs, dirs, deltas, table, counter)
    assert L.ngp_occupancy_lin_bytes(C, H) == 0

    grid = f(C, H ** 3)
    pose = torch.eye(4, device=device)[None].contiguous()
    refused(L.ngp_mark_untrained_grid(_lib.ptr(pose), 1, 50.0, 50.0, 24.0, 24.0, 1.0, C, H, _lib.ptr(grid), None, 0, s), "mark_untrained_grid")
    dws_bytes = L.ngp_density_grid_workspace(C, H)
    dws = torch.empty(dws_bytes, dtype=torch.uint8, device=device)
    cells_i = torch.zeros(16, dtype=torch.int32, device=device)
    sigmas = torch.ones(16, device=device)
    refused(L.ngp_density_grid_update(_lib.ptr(grid), C, H, 0, _lib.ptr(cells_i), _lib.ptr(sigmas), 16, 1.0, 0.95, _lib.ptr(dws), dws_bytes, s),
            "density_grid_update")
    mean_thresh = f(2)
    bits_out = torch.full((cells // 8,), 7, dtype=torch.uint8, device=device)
    refused(L.ngp_density_grid_finish(_lib.ptr(grid), C, H, 0.01, _lib.ptr(mean_thresh), _lib.ptr(bits_out), _lib.ptr(dws), dws_bytes, s),
            "density_grid_finish")
    assert untouched(grid, mean_thresh, bits_out)
    # the Python operators raise with the same message
    from nerfsafetyvalidation_amd import raymarching
    with pytest.raises(RuntimeError, match="H=%d.*power of two" % H):
        raymarching.march_rays(N, n_step, alive, nears, rays_o, rays_d, 1.0, bitfield, C, H, nears, fars, 128, False, 0.0, max_steps)
    with pytest.raises(RuntimeError, match="H=%d.*power of two" % H):
        raymarching.march_rays_train(rays_o, rays_d, 1.0, bitfield, C, H, nears, fars, None, -1, False, 128, True, 0.0, max_steps)
    torch.cuda.synchronize()
