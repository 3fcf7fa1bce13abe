"""csrc/raycast.hip against world.py's numpy path: EXACT equality (prim equal; t, u, v bit for bit) on every ray of raycast_cases, on
every mesh, for the grids (1,1,1), (4,4,4), (16,7,3) and the automatic one, with and without frame_width, on a non-default stream.  The
arithmetic per (ray, triangle) is fixed, so any difference is a coverage or an ordering bug; the (1,1,1) grid separates arithmetic bugs
from traversal bugs."""
import numpy as np
import pytest
import torch

import raycast_cases as RC
from nerfsafetyvalidation_amd import world as WO

pytestmark = pytest.mark.gpu
HAND_WIDTH = 10


def make_world(name, resolution, device, colors=True):
    v, f, c = RC.mesh(name)
    return WO.MeshWorld(torch.from_numpy(v).to(device), torch.from_numpy(f).to(device),
                        torch.from_numpy(c).to(device) if colors and c is not None else None, resolution=resolution)


def assert_identical(got, ref, rows=slice(None), what=""):
    got = {k: a.cpu().numpy().reshape(-1) for k, a in got.items()}
    prim = ref["prim"][rows]
    diff = np.flatnonzero(got["prim"] != prim)
    assert diff.size == 0, f"{what}: prim differs on {diff.size} rays, first {diff[:5]}: {got['prim'][diff[:5]]} != {prim[diff[:5]]}"
    for k in ("t", "u", "v"):
        diff = np.flatnonzero(RC.bits(got[k]) != RC.bits(ref[k][rows]))
        assert diff.size == 0, f"{what}: {k} differs on {diff.size} rays, first {diff[:5]}"
    assert got["prim"].dtype == np.int32 and got["t"].dtype == np.float32


@pytest.mark.parametrize("resolution", RC.RESOLUTIONS, ids=lambda r: "auto" if r is None else "x".join(map(str, r)))
@pytest.mark.parametrize("name", RC.MESHES)
def test_cast_is_identical_to_the_numpy_path(device, name, resolution):
    world = make_world(name, resolution, device)
    if resolution is not None:
        assert world.dims == resolution
    o, d, sections, _ = RC.rays(name)
    ref = RC.reference(name)
    to, td = torch.tensor(o, device=device), torch.tensor(d, device=device)
    assert_identical(world.cast(to, td), ref, what="row-major")
    frames = slice(0, sections["hand"].start)
    assert_identical(world.cast(to[frames], td[frames], frame_width=RC.FRAME), ref, frames, "8 x 8 tiles, frames")
    hand = sections["hand"]
    assert (hand.stop - hand.start) % HAND_WIDTH == 0
    assert_identical(world.cast(to[hand], td[hand], frame_width=HAND_WIDTH), ref, hand, "8 x 8 tiles, hand rays")
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        got = world.cast(to, td, frame_width=1)
    side.synchronize()
    assert_identical(got, ref, what="side stream")
    for n in RC.N_TAILS:
        rows = slice(hand.start, hand.start + n)
        assert_identical(world.cast(to[rows], td[rows]), ref, rows, f"N = {n}")
        assert_identical(world.cast(to[rows], td[rows], frame_width=n), ref, rows, f"N = {n}, one row")


@pytest.mark.parametrize("name", RC.MESHES)
def test_windowed_cast_and_binning_match_numpy(device, name):
    o, d, sections, _ = RC.rays(name)
    hand = sections["hand"]
    size = float(np.ptp(RC.mesh(name)[0], axis=0).max())
    world = make_world(name, None, device)
    cell_start, pair_tri = WO.bin_triangles_numpy(RC.tri_data(name), world.grid)
    assert np.array_equal(world.cell_start.cpu().numpy(), cell_start) and np.array_equal(world.pair_tri.cpu().numpy(), pair_tri)
    assert np.array_equal(world.tri_data.cpu().numpy(), RC.tri_data(name))
    for t_min, t_max in ((0.0, 1.2 * size), (0.9 * size, float("inf")), (-float("inf"), 0.0)):
        want = WO.cast_numpy(o[hand], d[hand], RC.tri_data(name), t_min, t_max)
        got = world.cast(torch.tensor(o[hand], device=device), torch.tensor(d[hand], device=device), t_min=t_min, t_max=t_max)
        assert_identical(got, want, what=f"t in ({t_min}, {t_max})")


@pytest.mark.parametrize("name", RC.MESHES)
def test_shading_matches_the_numpy_path(device, name):
    v, f, c = RC.mesh(name)
    world = make_world(name, None, device)
    o, d, sections, _ = RC.rays(name)
    ref = RC.reference(name)
    bg = np.array([0.125, 0.5, 0.875], np.float32)
    hit = {k: torch.from_numpy(np.array(a)).to(device) for k, a in ref.items()}
    image, u8 = world.shade(torch.tensor(d, device=device), hit, bg_color=bg, ambient=0.3)
    want, want_u8 = WO.shade_numpy(d, ref["prim"], ref["u"], ref["v"], RC.tri_data(name), f, c, bg, 0.3)
    image, u8 = image.cpu().numpy(), u8.cpu().numpy()
    ok = np.isfinite(d).all(1)
    assert image.dtype == np.float32 and u8.dtype == np.uint8 and image.shape == want.shape
    # about ten float32 operations on values in [0, 1] at half an ulp each
    assert np.abs(image[ok] - want[ok]).max() <= 2e-6
    assert np.abs(u8[ok].astype(np.int64) - want_u8[ok].astype(np.int64)).max() <= 1
    miss = ref["prim"] < 0
    assert miss.any() and (image[miss] == bg).all() and (u8[miss] == (bg * np.float32(255)).astype(np.uint8)).all()
    assert (image >= 0).all() and (image <= 1).all()


def test_invalid_inputs_raise_and_empty_batches_are_empty(device):
    v, f, _ = RC.mesh("cube")
    tv, tf = torch.from_numpy(v).to(device), torch.from_numpy(f).to(device)
    with pytest.raises(ValueError):
        WO.MeshWorld(tv, tf, resolution=(257, 2, 2))
    bad = tf.clone()
    bad[5, 2] = 8
    with pytest.raises(ValueError):
        WO.MeshWorld(tv, bad)
    with pytest.raises(ValueError):
        WO.MeshWorld(tv, tf[:0])
    with pytest.raises(ValueError):
        WO.MeshWorld(tv[:0], tf[:0])
    world = WO.MeshWorld(tv, tf)
    out = world.cast(torch.zeros(0, 3, device=device), torch.zeros(0, 3, device=device))
    assert all(a.shape == (0,) and a.device.type == "cuda" for a in out.values()) and out["prim"].dtype == torch.int32
    image, u8 = world.shade(torch.zeros(0, 3, device=device), out)
    assert image.shape == (0, 3) and u8.shape == (0, 3)
    with pytest.raises(ValueError):
        world.cast(torch.zeros(6, 3, device=device), torch.ones(6, 3, device=device), frame_width=4)
    with pytest.raises(ValueError):
        world.cast(torch.zeros(6, 3, device=device), torch.ones(6, 3, device=device), t_max=float("nan"))
    with pytest.raises(ValueError):
        world.cast(torch.zeros(6, 3, device=device), torch.ones(5, 3, device=device))
