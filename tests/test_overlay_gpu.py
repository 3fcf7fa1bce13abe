"""csrc/overlay.hip against the numpy path of the same rule (world.cast_overlay_numpy / shade_overlay_numpy), bit for bit: t, prim,
normal, and the shaded image / image_u8 -- over primitive counts that straddle the LDS chunk of 256 records, ray counts that straddle
a wave and a workgroup, per-ray far limits that mask every lane, none, or some of a wave, and MeshWorld.render_scene."""
import numpy as np
import pytest
import torch

import overlay_cases as OC
import raycast_cases as RC
from nerfsafetyvalidation_amd import _lib
from nerfsafetyvalidation_amd import scene as SC
from nerfsafetyvalidation_amd import world as WO

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def world(device):
    v, f, _ = RC.mesh("cube")
    return WO.MeshWorld(torch.from_numpy(v).to(device), torch.from_numpy(f).to(device))


def same(got, want):
    """a HIP result (tensors) equals a numpy result in every bit"""
    assert np.array_equal(got["prim"].cpu().numpy(), want["prim"])
    assert np.array_equal(OC.bits(got["t"].cpu().numpy()), OC.bits(want["t"]))
    assert np.array_equal(OC.bits(got["normal"].cpu().numpy()), OC.bits(want["normal"]))


def test_the_fixed_frames_equal_numpy_with_and_without_tiles(world, device):
    for which in ("close", "far"):
        o, d = [torch.from_numpy(np.array(a)).to(device) for a in OC.frame(which)]
        want = OC.reference(which)
        rowmajor = world.cast_overlay(o, d, OC.prims())
        tiled = world.cast_overlay(o, d, OC.prims(), frame_width=OC.W)
        same(rowmajor, want)
        same(tiled, want)
        for k in rowmajor:
            assert torch.equal(rowmajor[k].view(torch.int32), tiled[k].view(torch.int32))
        assert (want["prim"] >= 0).sum() > 300
        # the shaded frame over a world frame: bit for bit, untouched pixels keep their bits
        N = o.shape[0]
        image, u8 = torch.full((N, 3), 0.25, device=device), torch.full((N, 3), 63, dtype=torch.uint8, device=device)
        img, q8 = world.shade_overlay(d, tiled, OC.COLORS, image, u8, ambient=0.3)
        want_img, want_u8 = WO.shade_overlay_numpy(OC.frame(which)[1], want["prim"], want["normal"], OC.COLORS, 0.3, image.cpu().numpy(), u8.cpu().numpy())
        assert np.array_equal(OC.bits(img.cpu().numpy()), OC.bits(want_img)) and np.array_equal(q8.cpu().numpy(), want_u8)
        assert (image == 0.25).all() and (u8 == 63).all()


@pytest.mark.parametrize("P", [0, 1, 255, 256, 257, 2 * 256 + 3])
def test_primitive_counts_around_the_lds_chunk(P, world, device):
    q = OC.straddling_prims(P)
    o, d = OC.frame("close")
    want = WO.cast_overlay_numpy(o, d, q)
    got = world.cast_overlay(torch.from_numpy(np.array(o)).to(device), torch.from_numpy(np.array(d)).to(device), q, frame_width=OC.W)
    same(got, want)
    seen = set(np.unique(want["prim"]).tolist())
    if P == 0:
        assert seen == {-1}
    for i in (255, 256, 511, 512):                  # the last record of a chunk and the first of the next are hit
        if i < P:
            assert i in seen
    assert len(np.unique(q, axis=0)) == P


@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_ray_counts_around_a_wave_and_a_workgroup(N, world, device):
    o, d = OC.frame("close")
    pick = np.nonzero(OC.reference("close")["prim"] >= 0)[0]
    idx = np.concatenate([pick[:(N + 1) // 2], np.arange(N - (N + 1) // 2)])          # half of them hit
    q = OC.straddling_prims(257)
    q[:10] = OC.prims()
    want = WO.cast_overlay_numpy(o[idx], d[idx], q)
    got = world.cast_overlay(torch.from_numpy(o[idx]).to(device), torch.from_numpy(d[idx]).to(device), q)
    same(got, want)
    assert (want["prim"] >= 0).any() and got["t"].shape == (N,)


def test_far_limits_mask_lanes_without_losing_them(world, device):
    o, d = OC.frame("close")
    to, td = torch.from_numpy(np.array(o)).to(device), torch.from_numpy(np.array(d)).to(device)
    q = OC.straddling_prims(257)
    q[:10] = OC.prims()
    N = o.shape[0]
    free = WO.cast_overlay_numpy(o, d, q)
    limits = {"open": np.full(N, np.inf, f32),
              "shut": np.zeros(N, f32),                                                   # every lane masked from the start
              "mixed": np.where(np.arange(N) % 3 == 0, f32(0), np.where(np.arange(N) % 3 == 1, f32(0.45), f32(np.inf))).astype(f32)}
    for name, far in limits.items():
        want = WO.cast_overlay_numpy(o, d, q, t_max=far)
        for width in (None, OC.W, 35):      # (35: the last tile of every tile row holds lanes without a ray)
            same(world.cast_overlay(to, td, q, t_max=torch.from_numpy(far).to(device), frame_width=width), want)
        if name == "open":
            assert np.array_equal(want["prim"], free["prim"])
        if name == "shut":
            assert (want["prim"] == -1).all() and np.isposinf(want["t"]).all()
        if name == "mixed":
            assert (want["prim"][0::3] == -1).all() and (want["prim"][2::3] >= 0).any() and (want["prim"][1::3] != free["prim"][1::3]).any()
    # t_min above every hit: masked too; zero and non-finite rays
    same(world.cast_overlay(to, td, q, t_min=50.0), WO.cast_overlay_numpy(o, d, q, t_min=50.0))
    bo, bd = np.array(o[:8]), np.array(d[:8])
    bd[1] = 0
    bd[2, 0] = np.nan
    bo[3, 1] = np.inf
    same(world.cast_overlay(torch.from_numpy(bo).to(device), torch.from_numpy(bd).to(device), q), WO.cast_overlay_numpy(bo, bd, q))


def test_render_scene(device):
    v, f, c = SC.henge_mesh(24)
    world = WO.MeshWorld(torch.from_numpy(v).to(device), torch.from_numpy(f).to(device), torch.from_numpy(c).to(device))
    H, W = 40, 56
    pose = torch.from_numpy(SC.look_at_poses(np.array([[1.4, 1.1, -1.9]]))[0]).float()
    K = SC.intrinsics(H, W)
    plain = world.render(pose, K, H, W)
    empty = world.render_scene(pose, K, H, W)
    for k in plain:
        assert torch.equal(plain[k].view(torch.uint8), empty[k].view(torch.uint8)), k
    assert (empty["overlay_prim"] == -1).all()
    line = np.stack([np.linspace(-0.8, 0.8, 7), np.full(7, 0.45), np.linspace(0.5, -0.6, 7)], 1).astype(f32)      # above the stones
    under = line - f32([0, 1.2, 0])                                                                               # below the ground slab
    tubes = [(line, 0.03, (0.9, 0.1, 0.1)), (under, 0.03, (0.1, 0.1, 0.9))]
    boxes = [(line[::2] + f32([0, 0.1, 0]), (0.04, 0.04, 0.04), (0.1, 0.8, 0.1))]
    scene = world.render_scene(pose, K, H, W, tubes=tubes, boxes=boxes)
    over = scene["overlay_prim"]
    assert (over >= 0).sum() > 40 and (over == -1).sum() > 1000
    seen = set(np.unique(over.cpu().numpy()).tolist())
    assert seen & set(range(6)) and seen & set(range(12, 16)) and not seen & set(range(6, 12))          # the tube under the ground is hidden
    keep = over < 0
    for k in ("image", "image_u8", "depth"):
        assert torch.equal(scene[k][keep].view(torch.uint8), plain[k][keep].view(torch.uint8)), k
    assert torch.equal(scene["prim"], plain["prim"])
    assert (scene["depth"][~keep] < plain["depth"][~keep]).all() and not torch.equal(scene["image_u8"][~keep], plain["image_u8"][~keep])
    # the CPU world draws the same picture: the same bits where the overlay shows (the mesh's own shading agrees to 2e-6, test_world_gpu.py)
    cpu = WO.MeshWorld(v, f, c).render_scene(pose, K, H, W, tubes=tubes, boxes=boxes)
    assert np.array_equal(cpu["overlay_prim"].numpy(), over.cpu().numpy())
    assert np.array_equal(OC.bits(cpu["image"].numpy()[~keep.cpu().numpy()]), OC.bits(scene["image"].cpu().numpy()[~keep.cpu().numpy()]))
    assert np.array_equal(cpu["image_u8"].numpy()[~keep.cpu().numpy()], scene["image_u8"].cpu().numpy()[~keep.cpu().numpy()])


def test_a_bad_table_is_refused_before_any_launch(world, device):
    lib = _lib.lib()
    o, d = [torch.from_numpy(np.array(a[:64])).to(device) for a in OC.frame("close")]
    t = torch.full((64,), 7.0, device=device)
    prim = torch.full((64,), 7, dtype=torch.int32, device=device)
    normal = torch.full((64, 3), 7.0, device=device)
    for col, value, word in ((0, 2.0, b"kind"), (0, 0.5, b"kind"), (7, 0.0, b"r ="), (7, -1.0, b"r ="), (3, np.nan, b"non-finite"), (5, np.inf, b"non-finite"),
                             (7, np.nan, b"non-finite")):
        q = np.array(OC.prims())
        q[4, col] = value
        q_dev = torch.from_numpy(q).to(device)
        rc = lib.ngp_overlay_cast(_lib.ptr(o), _lib.ptr(d), 64, q.ctypes.data, _lib.ptr(q_dev), q.shape[0], 0.0, None, 0, _lib.ptr(t), _lib.ptr(prim),
                                  _lib.ptr(normal), _lib.stream())
        assert rc == -1 and word in lib.ngp_last_error() and b"primitive 4" in lib.ngp_last_error()
        with pytest.raises(ValueError):
            world.cast_overlay(o, d, q)
    torch.cuda.synchronize()
    assert (t == 7.0).all() and (prim == 7).all() and (normal == 7.0).all()                  # nothing was launched
    with pytest.raises(ValueError):
        world.cast_overlay(o, d, OC.prims(), frame_width=7)
    with pytest.raises(ValueError):
        world.cast_overlay(o, d, OC.prims(), t_max=torch.zeros(3))
