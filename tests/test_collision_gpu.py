"""The collision field's GPU kernels (collision.hip ngp_edt_sq, fused_query.hip ngp_cell_max_density) and the rollout with a field:
the distance transform against brute force and scipy, the reference's own createSDF.py output (tests/golden/sdf_henge.npz, made by
make_golden_sdf.py), the cell density against ngp_network_density bit for bit, and a GPU rollout looked up in the henge field."""
import hashlib
import os

import numpy as np
import pytest
import torch

from nerfsafetyvalidation_amd import _lib
from nerfsafetyvalidation_amd import collision as CO

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _brute_d2(occ):
    idx = np.argwhere(occ)
    if len(idx) == 0:
        return np.full(occ.shape, _lib.NGP_EDT_INF, np.int64)
    grid = np.indices(occ.shape).reshape(3, -1).T
    best = np.full(grid.shape[0], np.iinfo(np.int64).max)
    for i in range(0, len(idx), 256):
        best = np.minimum(best, ((grid[:, None, :] - idx[None, i:i + 256]) ** 2).sum(-1).min(1))
    return best.reshape(occ.shape)


@pytest.mark.parametrize("shape,p", [((7, 5, 3), 0.1), ((13, 11, 17), 0.02), ((1, 29, 4), 0.2), ((31, 1, 1), 0.3), ((3, 37, 67), 0.01),
                                     ((2, 3, 130), 0.004), ((23, 19, 1), 0.05)])
def test_edt_against_brute_force(device, shape, p):
    occ = np.random.default_rng(sum(shape)).random(shape) < p
    occ.reshape(-1)[0] = True
    got = CO.edt_sq(torch.from_numpy(occ).to(device)).cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, _brute_d2(occ))


def test_edt_corner_cases(device):
    one = np.zeros((9, 8, 7), bool)
    one[4, 0, 6] = True                                       # a single voxel
    assert np.array_equal(CO.edt_sq(torch.from_numpy(one).to(device)).cpu().numpy(), _brute_d2(one))
    full = np.ones((5, 6, 7), bool)
    assert (CO.edt_sq(torch.from_numpy(full).to(device)).cpu().numpy() == 0).all()
    empty = np.zeros((5, 6, 7), bool)
    assert (CO.edt_sq(torch.from_numpy(empty).to(device)).cpu().numpy() == _lib.NGP_EDT_INF).all()
    sdf = CO.SignedDistanceField.from_occupancy(torch.from_numpy(empty), CO.GridBox((0, 0, 0), 40, empty.shape))
    assert np.isposinf(sdf.values).all()                      # no occupied cell: +inf (scipy's phantom background is not copied)
    assert CO.edt_sq(torch.ones(1, 1, 1, dtype=torch.bool, device=device)).item() == 0


def test_edt_workspace_and_limits(device):
    lib = _lib.lib()
    m = torch.zeros(4, 5, 6, dtype=torch.uint8, device=device)
    d2 = torch.empty(4, 5, 6, dtype=torch.int32, device=device)
    need = lib.ngp_edt_sq_workspace(4, 5, 6)
    ws = torch.empty(need, dtype=torch.uint8, device=device)
    assert lib.ngp_edt_sq(_lib.ptr(m), 4, 5, 6, _lib.ptr(d2), _lib.ptr(ws), need - 1, _lib.stream()) == -3     # NGP_EWORKSPACE
    assert lib.ngp_edt_sq(_lib.ptr(m), 4, 16385, 1, _lib.ptr(d2), _lib.ptr(ws), need, _lib.stream()) == -1      # dimension limit
    assert lib.ngp_edt_sq(_lib.ptr(m), 0, 5, 6, _lib.ptr(d2), _lib.ptr(ws), need, _lib.stream()) == -1


def test_edt_against_scipy(device):
    nd = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(1)
    for shape, p in [((72, 96, 56), 0.002), ((61, 200, 130), 0.0005), ((150, 40, 97), 0.3)]:
        occ = rng.random(shape) < p
        sdf = CO.SignedDistanceField.from_occupancy(torch.from_numpy(occ), CO.GridBox((0, 0, 0), 40, shape))
        want = nd.distance_transform_edt(~occ) / 40
        assert np.array_equal(sdf.values, want), shape


def test_field_equals_the_reference_create_sdf(device, tmp_path):
    """tests/golden/sdf_henge.npz: createSDF.py's own sdf.npy for the henge map, bit for bit (file hash and sampled values)"""
    f = np.load(os.path.join(G, "sdf_henge.npz"), allow_pickle=False)
    shape = tuple(int(v) for v in f["shape"])
    box = CO.GridBox(f["start"], float(f["granularity"]), shape)
    assert box == CO.collision_map_box()
    occ = np.unpackbits(f["occupancy_bits"])[:int(np.prod(shape))].astype(bool).reshape(shape)
    assert np.array_equal(occ, CO.occupancy_from_fn(CO.henge_fn, box, 2).numpy())
    sdf = CO.SignedDistanceField.from_occupancy(torch.from_numpy(occ).to(device), box)
    assert np.array_equal(sdf.values.reshape(-1)[f["sample_index"]], f["sample_value"])
    path = str(tmp_path / "sdf.npy")
    sdf.save(path)
    assert hashlib.sha256(open(path, "rb").read()).hexdigest() == str(f["sdf_npy_sha256"])


def _models(device):
    from nerfsafetyvalidation_amd.scene import StonehengeScene
    sc = StonehengeScene(H=8, W=8, bound=2)
    lin = sc.build_model(device, backbone="linear", cuda_ray=False, fp16_table=False)
    ff = sc.build_model(device, cuda_ray=False)
    return [("f32", lin, False), ("f16", ff, True)]


@pytest.mark.parametrize("s", [1, 2, 3])
def test_cell_max_density_is_the_max_of_network_density(device, s):
    """every precision: max over the s^3 points of ngp_network_density on the same fp32 points, bit for bit, on a box whose start and
    granularity fit no grid, with PLANNER_ROT and with a general rotation"""
    box = CO.GridBox((-0.83, -0.61, -0.27), 37.3, (11, 9, 7))
    c, sn = np.cos(0.7), np.sin(0.7)
    turn = [[c, -sn, 0.0], [sn, c, 0.0], [0.0, 0.0, 1.0]]
    for name, model, autocast in _models(device):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
            fm = model.fused_model()
            assert fm is not None and fm.f32 == (name == "f32")
            for rot in (CO.PLANNER_ROT, turn):
                got = CO.cell_max_density(model, box, s, rot)
                want = None
                for a in range(s):
                    for b in range(s):
                        for cc in range(s):
                            x = CO.to_nerf(box.sample_points(a, b, cc, s, device), rot)
                            sig = fm.network_density(x.reshape(-1, 3).contiguous()).reshape(box.shape)
                            want = sig if want is None else torch.maximum(want, sig)
                assert got.shape == box.shape and torch.equal(got, want), (name, rot)
                assert (got > 0).all()


def test_occupancy_from_density_thresholds_the_max(device):
    box = CO.GridBox((-1.2, -1.2, -0.22), 40, (72, 96, 56))
    for name, model, autocast in _models(device):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
            sig = CO.cell_max_density(model, box, 2)
            thresh = float(sig.median())
            occ = CO.occupancy_from_density(model, box, thresh, 2)
        assert occ.dtype == torch.bool and torch.equal(occ, sig > thresh) and 0 < int(occ.sum()) < occ.numel(), name


def test_rollout_with_the_henge_field(device):
    from nerfsafetyvalidation_amd import rollout as RO
    from nerfsafetyvalidation_amd.scene import StonehengeScene
    occ = CO.occupancy_from_fn(CO.henge_fn, CO.collision_map_box(), 2)
    sdf = CO.SignedDistanceField.from_array(CO.SignedDistanceField.from_occupancy(occ, CO.collision_map_box()).values, CO.reference_box())
    H = W = 32
    sc = StonehengeScene(H=H, W=W, bound=2)
    model = sc.build_model(device, cuda_ray=False)
    kw = dict(num_steps=32, upsample_steps=0, max_ray_batch=1024)
    run = lambda **a: RO.run_rollout(model, sc.intrinsics, H, W, 3, 6, seed=5, in_flight=2, render_kwargs=kw, **a)[0]   # noqa: E731
    rows = run(sdf=sdf)
    assert np.array_equal(rows, run(sdf=sdf))                 # two runs, the same bits
    assert (rows[:, 14] < 9999).any()
    for r in rows:
        collided, value = sdf.lookup(r[15:18])
        if value is not None:
            assert r[14] == value and r[22] == float(collided)
    # the batched gather agrees with the host lookup
    vals, ok = sdf.query(torch.from_numpy(rows[:, 15:18]).to(device))
    for r, v, o in zip(rows, vals.cpu().numpy(), ok.cpu().numpy()):
        lk = sdf.lookup(r[15:18])[1]
        assert o == (lk is not None) and (lk is None or v == lk)
    assert np.array_equal(run(sdf=None), run())
