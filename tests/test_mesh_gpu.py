"""ngp_isosurface_count / ngp_isosurface_emit (csrc/mesh.hip) against mesh.py's numpy path, and save_mesh on a model.

The kernels run one thread per lattice point in workgroups of 256 (four wave64s); the block totals are scanned by one workgroup of
1024 threads, 1024 totals per round.  The build has -ffp-contract=off and both paths take one IEEE fp32 operation per step, so
vertices are compared bit for bit (stricter than the 2 * max(X, Y, Z) * 2^-23 the coordinates' ulp would allow)."""
import os

import numpy as np
import pytest
import torch

import mesh_fields as MF
from nerfsafetyvalidation_amd import _lib
from nerfsafetyvalidation_amd import mesh as M

pytestmark = pytest.mark.gpu


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _check(u, thr, device):
    want_v, want_f = M.isosurface(u, thr)
    v, f = M.isosurface(torch.from_numpy(u).to(device), thr)
    assert v.is_cuda and f.is_cuda and v.dtype == torch.float32 and f.dtype == torch.int32
    v, f = v.cpu().numpy(), f.cpu().numpy()
    assert v.shape == want_v.shape and f.shape == want_f.shape
    assert np.array_equal(f, want_f)
    if len(v):
        print(u.shape, "V", len(v), "F", len(f), "max |dv|", np.abs(v.astype(np.float64) - want_v).max())
    assert _same_bits(v, want_v)
    return v, f


# (65,33,17): 36465 points = 143 workgroups; rows of 17 and planes of 561 points are no multiple of 64 or 256, so waves and
#             workgroups start and end inside rows, and every neighbour offset (1, 17, 561 and their sums) crosses both
# (3,4,300):  one row is longer than a wave AND a workgroup (300 > 256): the +z neighbour of a wave's / workgroup's last lane
#             belongs to the next one, and the 15 block totals carry into each other
# (96,96,96): 884736 points = 3456 block totals > 1024: the scan of the block totals takes four rounds with a carry, and V and F
#             exceed what 1024 workgroups can hold (1024 * 256 * 7)
@pytest.mark.parametrize("shape,seed", [((2, 2, 2), 1), ((2, 5, 3), 3), ((5, 7, 9), 4), ((65, 33, 17), 6), ((3, 4, 300), 7)])
def test_random_fields_match_the_cpu_path(device, shape, seed):
    v, f = _check(MF.random_field(shape, seed), 0.0, device)
    assert len(v) > 0 and len(f) > 0


def test_all_corner_configurations_match_the_cpu_path(device):
    u = MF.random_field(MF.ALL_CONFIG_SHAPE, MF.ALL_CONFIG_SEED)
    assert len(np.unique(MF.corner_configurations(u, 0.0))) == 256
    _check(u, 0.0, device)


def test_smooth_field_beyond_one_round_of_block_totals(device):
    u = MF.smooth_field((96, 96, 96))
    assert u.size // 256 > 1024
    v, f = _check(u, 0.1, device)
    assert len(v) > 1024 and len(f) > 1024


def test_empty_nan_inf_and_non_contiguous(device):
    for value in (-1.0, 1.0, 0.0):
        v, f = M.isosurface(torch.full((4, 5, 6), value, device=device), 0.0)
        assert v.shape == (0, 3) and f.shape == (0, 3) and v.dtype == torch.float32 and f.dtype == torch.int32
    u = MF.sphere()
    u[5, 9, 9] = np.nan
    want_v, want_f = M.isosurface(u, 0.0)
    v, f = M.isosurface(torch.from_numpy(u).to(device), 0.0)
    assert np.array_equal(f.cpu().numpy(), want_f) and np.array_equal(v.cpu().numpy(), want_v, equal_nan=True)
    u[5, 9, 9] = np.inf
    with pytest.raises(ValueError):
        M.isosurface(torch.from_numpy(u).to(device), 0.0)
    # a transposed view and a strided slice: made contiguous, never misread
    r = MF.random_field((9, 7, 5), 8)
    want_v, want_f = M.isosurface(r, 0.0)
    t = torch.from_numpy(np.ascontiguousarray(r.transpose(2, 0, 1))).to(device).permute(1, 2, 0)
    wide = torch.zeros(9, 7, 10, device=device)
    wide[:, :, ::2] = torch.from_numpy(r).to(device)
    for view in (t, wide[:, :, ::2]):
        assert not view.is_contiguous()
        v, f = M.isosurface(view, 0.0)
        assert np.array_equal(f.cpu().numpy(), want_f) and _same_bits(v.cpu().numpy(), want_v)


def test_c_abi_refuses_bad_sizes(device):
    lib = _lib.lib()
    assert lib.ngp_isosurface_workspace(1, 8, 8) == 0 and lib.ngp_isosurface_workspace(2048, 1024, 1024) == 0
    assert lib.ngp_isosurface_workspace(65535, 65535, 65535) == 0          # no overflow on the way to the answer
    u = torch.zeros(8, 8, 8, device=device)
    nbytes = lib.ngp_isosurface_workspace(8, 8, 8)
    assert nbytes >= 7 * 512
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    tot = torch.zeros(2, dtype=torch.int64, device=device)
    args = (_lib.ptr(ws), nbytes, _lib.ptr(tot), _lib.stream())
    assert lib.ngp_isosurface_count(_lib.ptr(u), 1, 8, 8, 0.0, *args) == -1 and b"at least 2" in lib.ngp_last_error()
    assert lib.ngp_isosurface_count(_lib.ptr(u), 2048, 1024, 1024, 0.0, *args) == -1 and b"2^31" in lib.ngp_last_error()
    assert lib.ngp_isosurface_count(_lib.ptr(u), 8, 8, 8, 0.0, _lib.ptr(ws), nbytes - 1, _lib.ptr(tot), _lib.stream()) == -3
    assert lib.ngp_isosurface_emit(_lib.ptr(u), 8, 8, 8, 0.0, _lib.ptr(ws), nbytes, 1 << 31, 6, _lib.ptr(ws), _lib.ptr(ws), _lib.stream()) == -1
    assert b"V and F" in lib.ngp_last_error()
    torch.cuda.synchronize()


def test_two_streams_give_the_serial_results(device):
    fields = [torch.from_numpy(MF.smooth_field((40, 48, 56))).to(device), torch.from_numpy(MF.random_field((33, 31, 65), 9)).to(device)]
    serial = [M.isosurface(u, 0.05) for u in fields]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device), torch.cuda.Stream(device)]
    out = [None, None]
    for _ in range(2):
        for i in (0, 1):
            streams[i].wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(streams[i]):
                out[i] = M.isosurface(fields[i], 0.05)
    torch.cuda.synchronize()
    for (v, f), (sv, sf) in zip(out, serial):
        assert torch.equal(f, sf) and _same_bits(v.cpu().numpy(), sv.cpu().numpy())


def test_two_streams_count_then_emit_interleaved(device):
    """both counts in flight on their own streams and workspaces before either emit"""
    lib = _lib.lib()
    fields = [torch.from_numpy(MF.smooth_field((40, 48, 56))).to(device), torch.from_numpy(MF.random_field((33, 31, 65), 9)).to(device)]
    serial = [M.isosurface(u, 0.05) for u in fields]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device), torch.cuda.Stream(device)]
    ws, tot = [], []
    for u in fields:
        n = lib.ngp_isosurface_workspace(*u.shape)
        ws.append(torch.empty(n, dtype=torch.uint8, device=device))
        tot.append(torch.zeros(2, dtype=torch.int64, device=device))
    torch.cuda.synchronize()
    for i, u in enumerate(fields):
        _lib.check(lib.ngp_isosurface_count(_lib.ptr(u), *u.shape, 0.05, _lib.ptr(ws[i]), ws[i].numel(), _lib.ptr(tot[i]), streams[i].cuda_stream))
    torch.cuda.synchronize()
    out = []
    for i, u in enumerate(fields):
        V, F = tot[i].tolist()
        v = torch.empty(V, 3, dtype=torch.float32, device=device)
        f = torch.empty(F, 3, dtype=torch.int32, device=device)
        _lib.check(lib.ngp_isosurface_emit(_lib.ptr(u), *u.shape, 0.05, _lib.ptr(ws[i]), ws[i].numel(), V, F, _lib.ptr(v), _lib.ptr(f),
                                           streams[i].cuda_stream))
        out.append((v, f))
    torch.cuda.synchronize()
    for (v, f), (sv, sf) in zip(out, serial):
        assert torch.equal(f, sf) and _same_bits(v.cpu().numpy(), sv.cpu().numpy())


# ------------------------------------------------------------------ save_mesh on the synthetic henge model
def _models(device):
    from nerfsafetyvalidation_amd.scene import StonehengeScene
    sc = StonehengeScene(H=8, W=8, bound=2)
    return {"f32": (sc.build_model(device, backbone="linear", cuda_ray=False, fp16_table=False), False),
            "f16": (sc.build_model(device, cuda_ray=False), True)}


@pytest.mark.parametrize("name", ["f32", "f16"])
def test_save_mesh_on_the_henge_model(device, tmp_path, name):
    """the field is model.density on the lattice points, bit for bit; the mesh is the CPU path's on that field; it is open only at the
    lattice boundary; and every vertex sits on a lattice edge whose two ends, re-queried from the model, have the threshold between
    their densities (one > threshold, the other not).  The threshold is the field's median, so that the surface runs everywhere."""
    model, fp16 = _models(device)[name]
    model.eval()
    R = 48
    lo, hi = model.aabb_infer[:3], model.aabb_infer[3:]

    def query(pts):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=fp16):
            return model.density(pts.to(device))["sigma"]

    axes = [torch.linspace(float(lo[d]), float(hi[d]), R) for d in range(3)]
    pts = torch.stack(torch.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    direct = query(pts).float().reshape(R, R, R)
    u = M.extract_fields(lo, hi, R, query, S=32)              # 2 x 2 x 2 chunks of 32 and 16
    assert u.is_cuda and u.dtype == torch.float32 and torch.equal(u, direct)
    assert torch.equal(M.extract_fields(lo, hi, R, query), direct)
    thr = float(direct.median())

    path = os.path.join(tmp_path, "meshes", "henge.ply")
    verts, tris = M.save_mesh(model, path, resolution=R, threshold=thr, fp16=fp16)
    assert os.path.getsize(path) > 12 * len(verts) + 13 * len(tris)
    un = direct.cpu().numpy()
    want_v, want_f = M.isosurface(un, thr)
    assert len(want_v) > 1000 and np.array_equal(tris, want_f)
    b_min, b_max = lo.cpu().numpy(), hi.cpu().numpy()
    assert np.array_equal(verts, want_v.astype(np.float64) / (R - 1.0) * (b_max - b_min)[None, :] + b_min[None, :])

    owners, types = M.vertex_edges(un, thr)
    MF.assert_open_only_at_the_boundary(un.shape, owners, types, tris, M.EDGE_OFFSETS)
    other = owners + np.asarray(M.EDGE_OFFSETS)[types]
    assert ((want_v >= owners) & (want_v <= other)).all()
    ends = []
    for idx in (owners, other):
        p = torch.stack([axes[d][torch.from_numpy(idx[:, d])] for d in range(3)], -1)
        ends.append(query(p).float().cpu().numpy())
    assert ((ends[0] > np.float32(thr)) != (ends[1] > np.float32(thr))).all()
