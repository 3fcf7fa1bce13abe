"""The cases of march_cases.py, judged on the CPU oracle alone: the conditions that keep test_march_gpu.py from passing vacuously.
Every test prints the counts it measured (pytest -s shows them)."""
import numpy as np
import pytest

import march_cases as MC
from oracle import oracle as O

CONFIG_IDS = [MC.config_id(c) for c in MC.CONFIGS]


def test_packer_round_trips_against_the_oracle():
    """bit level * H^3 + morton3D(x, y, z), LSB first: O.morton3D gives the index, O.packbits the bytes"""
    rng = np.random.default_rng(5)
    for C, H in ((1, 8), (3, 16), (2, 32)):
        occ = rng.random((C, H, H, H)) < 0.4
        coords = np.stack(np.meshgrid(np.arange(H), np.arange(H), np.arange(H), indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
        idx = np.empty(H ** 3, np.int32)
        O.morton3D(coords, H ** 3, idx)
        assert np.array_equal(MC.cell_bit_index(C, H)[0].ravel(), idx.astype(np.uint32))
        assert sorted(idx.tolist()) == list(range(H ** 3))
        dense = np.zeros((C, H ** 3), np.float32)
        for level in range(C):
            dense[level, idx] = occ[level].ravel()
        want = np.empty(C * H ** 3 // 8, np.uint8)
        O.packbits(dense, C * H ** 3 // 8, 0.5, want)
        got = MC.pack(occ)
        assert got.dtype == np.uint8 and np.array_equal(got, want)
        assert np.array_equal(MC.unpack(got, C, H), occ)
    # one cell -> one bit
    occ, bf = MC.single_bit(2, 8, (1, 7, 0, 7))
    bit = 512 + int(MC.morton3D(7, 0, 7))
    assert bit == 512 + 0b101101101 and bf[bit // 8] == 1 << (bit % 8) and int(np.unpackbits(bf).sum()) == 1


@pytest.mark.parametrize("H", [48, 100, 6])
def test_packer_refuses_a_grid_size_that_is_no_power_of_two(H):
    """morton3D(H-1, H-1, H-1) >= H^3 there (233 471 against 110 592 cells for H = 48): the bit would lie past the level"""
    assert int(MC.morton3D(H - 1, H - 1, H - 1)) >= H ** 3
    with pytest.raises(ValueError, match="power of two"):
        MC.pack(np.zeros((1, H, H, H), bool))


def test_grids_are_what_they_claim():
    for C, H in sorted({(c.C, c.H) for c in MC.CONFIGS}):
        rnd, blocks, corners, shell = (MC.grid(g, C, H)[0] for g in MC.GRIDS)
        assert abs(rnd.mean() - 0.3) < 4 * np.sqrt(0.3 * 0.7 / rnd.size)          # four standard deviations of the fraction
        assert blocks.mean() == 0.5
        b = blocks.reshape(C, H // 4, 4, H // 4, 4, H // 4, 4)
        assert (b.any(axis=(2, 4, 6)) == b.all(axis=(2, 4, 6))).all()          # whole blocks
        assert corners.sum() == 3 * C and corners[:, 0, 0, 0].all() and corners[:, H - 1, H - 1, H - 1].all()
        assert shell.any(axis=(1, 2, 3)).all() and not shell[:, 0, 0, 0].any() and not shell[:, H // 2, H // 2, H // 2].any()
        for g in MC.GRIDS:
            occ, bf = MC.grid(g, C, H)
            assert bf.shape == (C * H ** 3 // 8,) and np.array_equal(MC.unpack(bf, C, H), occ)


def test_rays_are_what_they_claim():
    for bound, H in sorted({(c.bound, c.H) for c in MC.CONFIGS}):
        r = MC.rays(bound, H)
        assert r.rays_o.shape == (MC.N_RAYS, 3) and MC.N_RAYS == 2048 and r.miss.sum() == 4 * MC.MISSES
        for a in (r.rays_o, r.rays_d, r.nears, r.fars):
            assert a.dtype == np.float32
        assert not np.isnan(r.rays_o).any() and not np.isnan(r.rays_d).any()
        # an axis ray that runs IN a face of the box has a slab of 0 * inf = NaN, which the reference's comparisons let through into
        # near or far: such a ray takes no sample (`t < far` is false).  Nowhere else.
        in_face = (np.abs(r.rays_o) == np.float32(bound)).any(-1)
        nan = np.isnan(r.nears) | np.isnan(r.fars)
        assert not nan[~in_face].any() and (np.flatnonzero(nan) // MC.PER_FAMILY == MC.FAMILIES.index("axis")).all()
        print("bound %g H %d: %d axis rays lie in a face of the box, %d of them with a NaN near or far" % (bound, H, in_face.sum(), nan.sum()))
        assert np.abs(np.linalg.norm(r.rays_d.astype(np.float64), axis=-1) - 1).max() < 1e-6
        for name in MC.FAMILIES:
            assert r.miss[r.family[name]].sum() == MC.MISSES            # 16 misses in every family
        assert (r.nears[r.miss] == MC.FLT_MAX).all() and (r.fars[r.miss] == MC.FLT_MAX).all()
        hit = ~r.miss & ~nan
        assert (r.nears[hit] >= np.float32(MC.MIN_NEAR)).all()
        # (a lattice ray along an edge of the box, or a diagonal through one of its corners, may graze it or miss it by a rounding)
        assert (r.fars[hit] < MC.FLT_MAX).mean() > 0.95 and (r.fars[hit] > r.nears[hit]).mean() > 0.95
        o, d = r.rays_o[r.family["inside"]][:-MC.MISSES], r.rays_d[r.family["inside"]][:-MC.MISSES]
        assert np.abs(o).max() <= 0.9 * bound
        o, d = r.rays_o[r.family["axis"]], r.rays_d[r.family["axis"]]
        assert ((d != 0).sum(-1) == 1).all() and (np.abs(d).max(-1) == 1).all()
        assert np.signbit(d[d == 0]).any() and not np.signbit(d[d == 0]).all()      # both zeros
        k = np.abs(d).argmax(-1)
        other = np.ones_like(o, bool)
        other[np.arange(len(o)), k] = False
        j = (o[:-MC.MISSES][other[:-MC.MISSES]].astype(np.float64) + 1) * H / 2
        assert (j == np.round(j)).all() and j.min() == 0 and j.max() == H           # on the lattice, the box faces of level 0 included
        d = r.rays_d[r.family["diagonal"]]
        assert (np.abs(d) == np.float32(1 / np.sqrt(3.0))).all()


@pytest.mark.parametrize("ci", range(len(MC.CONFIGS)), ids=CONFIG_IDS)
def test_every_family_takes_samples(ci):
    cfg = MC.CONFIGS[ci]
    r = MC.rays(cfg.bound, cfg.H)
    for g in MC.GRIDS:
        t = MC.train_reference(ci, g)
        counts = MC.samples_per_ray(t)
        for a in (t.xyzs, t.dirs, t.deltas):
            assert not np.isnan(a).any()
        assert t.counter[1] == MC.N_RAYS and t.counter[0] == counts.sum() == t.xyzs.shape[0]
        assert t.counter[0] <= 2_100_000
        assert (counts[r.miss] == 0).all()
        with_samples = {f: int((counts[r.family[f]] > 0).sum()) for f in MC.FAMILIES}
        full = int((counts == cfg.max_steps).sum())
        print("%s %-8s samples %8d  rays with samples %s  budget filled %d" % (MC.config_id(cfg), g, t.counter[0], with_samples, full))
        if g in ("random", "blocks"):
            for f in MC.FAMILIES:
                assert with_samples[f] >= MC.PER_FAMILY // 2, (g, f, with_samples[f])
        if g == "corners":
            assert with_samples["diagonal"] >= 100
        if g == "shell":
            assert sum(with_samples.values()) >= 100


@pytest.mark.parametrize("key", [(4.0, 3, 128), (8.0, 4, 64), (8.0, 8, 8)], ids=str)
def test_budget_is_filled(key):
    ci = [i for i, c in enumerate(MC.CONFIGS) if (c.bound, c.C, c.H) == key]
    assert len(ci) == 1
    cfg = MC.CONFIGS[ci[0]]
    full = int((MC.samples_per_ray(MC.train_reference(ci[0], "blocks")) == cfg.max_steps).sum())
    print("%s blocks: %d rays fill the budget of %d steps" % (MC.config_id(cfg), full, cfg.max_steps))
    assert full >= 50


@pytest.mark.parametrize("key", [(1.5, 2, 64, 256), (3.0, 3, 32, 128)], ids=str)
def test_boundary_crossings_inside_a_top_level_cell(key):
    ci = [i for i, c in enumerate(MC.CONFIGS) if (c.bound, c.C, c.H, c.max_steps) == key]
    assert len(ci) == 1
    cfg = MC.CONFIGS[ci[0]]
    assert cfg.dt_gamma == 0 and cfg.bound != 2 ** (cfg.C - 1) and 2 ** (cfg.C - 2) < cfg.bound < 2 ** (cfg.C - 1)
    occ = MC.grid("random", cfg.C, cfg.H)[0]
    r = MC.rays(cfg.bound, cfg.H)
    crossing = MC.boundary_crossings(cfg, occ, r, MC.train_reference(ci[0], "random"))
    print("%s random: %d of %d rays step across the lower level's cube surface inside one top-level cell into an empty cell"
          % (MC.config_id(cfg), int(crossing.sum()), MC.N_RAYS))
    assert crossing.sum() >= 100


def test_resumed_marches_take_samples():
    """the three consecutive march_rays calls of the GPU test: the second and third resume mid-ray and still find samples"""
    for ci in (0, 5, 8):
        cfg = MC.CONFIGS[ci]
        r = MC.rays(cfg.bound, cfg.H)
        bf = MC.grid("random", cfg.C, cfg.H)[1]
        alive = np.arange(0, MC.N_RAYS, 2, dtype=np.int32)
        rays_t = r.nears.copy()
        taken = []
        for _ in range(3):
            xyzs, dirs, deltas = MC.oracle_march(cfg, bf, r, alive, rays_t, 3)
            assert not np.isnan(xyzs).any() and not np.isnan(deltas).any()
            taken.append(int((deltas[:, 0] > 0).sum()))
            alive, rays_t = MC.oracle_advance(alive, rays_t, deltas, 3)
        print("%s random, n_step 3: samples per call %s, %d rays alive after" % (MC.config_id(cfg), taken, alive.shape[0]))
        assert min(taken) > 500 and alive.shape[0] > 100
