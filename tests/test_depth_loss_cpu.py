"""Depth supervision without a GPU: the float64 helper (depth_cases.py) against finite differences, loss.depth_loss's torch form against
the helper, the dataset's depth files from the writer through NeRFDataset.collate, make_mesh_dataset --depth against the world's own
cast, the Trainer's part with a stub model, and the entry point's flags."""
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import depth_cases as DC
from nerfsafetyvalidation_amd import loss as LS
from nerfsafetyvalidation_amd import main_nerf
from nerfsafetyvalidation_amd.nerf import provider as P
from nerfsafetyvalidation_amd.nerf import targets as TG
from nerfsafetyvalidation_amd.nerf import trainer as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, B = 0.7, 0.3


@pytest.fixture(scope="module")
def fx():
    return DC.load()


@pytest.fixture(scope="module")
def cases(fx):
    target, names = DC.make_targets(fx)
    return target, names


def test_every_target_case_occurs(fx, cases):
    target, names = cases
    assert set(names) == set(DC.CASES)
    slots = fx["rays"][:, 0]
    for n, name in enumerate(names):
        z = target[slots[n]]
        assert (name in DC.NO_MEASUREMENT) == (not z > 0) and (name == "inf") == bool(np.isposinf(z))
    long_rays = [names[n] for n in range(len(names)) if fx["n_live"][n] > 128]
    assert any(name.startswith("mid") for name in long_rays)             # a surface inside a ray of more than two chunks


def test_helper_gradient_is_the_derivative_of_its_loss(fx, cases):
    """central differences in float64 on every live sample of a few rays, the sample that stops the ray included"""
    target, names = cases
    want = DC.packed64(fx, target, fx["scale"], a=A, b=B)
    checked = 0
    for n in (1, 2, 5, 13, 15, 16, 31):           # one and two samples, 65 (mid63), the rays that stop at 63 (mid0) and 40 (inf), beyond
        slot, rows, n_live, takes_part = DC.ray_rows(fx, n)
        assert takes_part and names[n] not in DC.NO_MEASUREMENT
        sigma = fx["sigmas"][rows].astype(np.float64)
        z, s = float(target[slot]), float(fx["scale"][slot])
        for i in range(n_live):
            h = 1e-6 * max(1.0, sigma[i])
            up, down = sigma.copy(), sigma.copy()
            up[i] += h
            down[i] -= h
            fd = (DC.ray_loss_of_sigma64(fx, n, up, z, s, DC.MARGIN, A, B) - DC.ray_loss_of_sigma64(fx, n, down, z, s, DC.MARGIN, A, B)) / (2 * h)
            got = want["grad_sigma"][rows.start + i]
            scale = np.abs(want["grad_sigma"][rows.start:rows.start + n_live]).max()
            # (truncation 1e-6 of the ray's largest gradient; the difference of two losses rounded to 2^-52 each, divided by 2 h)
            assert abs(fd - got) <= 1e-6 * scale + 4 * 2.0 ** -52 * max(want["loss_rays"][slot], 1.0) / h, (n, i, fd, got)
            checked += 1
        assert (want["grad_sigma"][rows.start + n_live:rows.stop] == 0).all()
    assert checked > 200


def _dense(fx, cases, dtype):
    """the fixture's rays as dense [37, 1024] float64 weights and distances (zero weights behind the stop and in the padding), with
    their targets and scales in table-row order"""
    target, _ = cases
    N = fx["rays"].shape[0]
    w, t = np.zeros((N, 1024)), np.zeros((N, 1024))
    for n in range(N):
        _, rows, n_live, _ = DC.ray_rows(fx, n)
        count = rows.stop - rows.start
        if count:
            w[n, :count], t[n, :count], _ = DC.weights64(fx["sigmas"][rows], fx["deltas"][rows, 0], fx["deltas"][rows, 1], n_live)
    slots = fx["rays"][:, 0]
    return w.astype(dtype), t.astype(dtype), target[slots], fx["scale"][slots]


@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-12), (np.float32, 2e-5)])
def test_torch_form_matches_the_helper(fx, cases, dtype, tol):
    """float32 bound: d and A are sums of up to 1024 non-negative products, each rounded once and added pairwise, (log2(1024) + 2) *
    2^-24 = 7e-7 of their value; the squared miss (d - z)^2 and the gradient's 2 (d - z) t magnify d's error by at most 2 d / |d - z|,
    below 30 for these targets (asserted): 30 * 7e-7 = 2e-5.  What was observed is printed."""
    w, t, z, s = _dense(fx, cases, dtype)
    for scale in (s, None):
        wt = torch.from_numpy(w).requires_grad_(True)
        loss = LS.depth_loss(wt, torch.from_numpy(t), torch.from_numpy(z), DC.MARGIN, None if scale is None else torch.from_numpy(scale), A, B)
        loss.backward()
        want_loss, want_g = DC.dense64(w, t, z, scale, a=A, b=B)
        surface = np.isfinite(z) & (z > 0)
        d64 = (w.astype(np.float64) * t).sum(axis=1)
        assert (2 * d64[surface] <= 30 * np.abs(d64 - z)[surface]).all()
        err = abs(float(loss.detach()) - want_loss.sum() / len(z)) / (want_loss.sum() / len(z))
        got = wt.grad.double().numpy() * len(z)
        gmax = np.abs(want_g).max(axis=1, keepdims=True)
        err_g = np.max(np.abs(got - want_g) / np.where(gmax > 0, gmax, 1))
        print(f"depth_loss torch form {np.dtype(dtype).name}: loss {err:.2e}, grad_w {err_g:.2e}")
        assert loss.shape == () and err <= tol and err_g <= tol
        nothing = ~(z > 0)
        assert nothing.sum() >= 9 and (got[nothing] == 0).all()                 # no measurement: every gradient row exactly 0
        empty = np.isposinf(z)
        assert empty.sum() >= 3 and np.abs(got[empty] - B).max() <= 4 * 2.0 ** -24                      # known empty: only the free-space term


def test_torch_form_autograd_is_the_analytic_gradient():
    g = torch.Generator().manual_seed(3)
    w = (torch.rand(2, 3, 9, generator=g, dtype=torch.float64) * 0.1).requires_grad_(True)
    t = torch.sort(torch.rand(2, 3, 9, generator=g, dtype=torch.float64), dim=-1).values
    z = torch.tensor([[0.5, float("inf"), 0.0], [float("nan"), 0.3, -1.0]], dtype=torch.float64)
    s = torch.rand(2, 3, generator=g, dtype=torch.float64) + 0.5
    loss = LS.depth_loss(w, t, z, 0.05, s, A, B)
    loss.backward()
    want_loss, want_g = DC.dense64(w.detach().reshape(6, 9).numpy(), t.reshape(6, 9).numpy(), z.reshape(6).numpy(), s.reshape(6).numpy(), 0.05, A, B)
    assert abs(loss.item() - want_loss.sum() / 6) <= 1e-14
    assert np.abs(w.grad.reshape(6, 9).numpy() * 6 - want_g).max() <= 1e-14
    flat = LS.depth_loss(w.detach().reshape(6, 9), t.reshape(6, 9), z.reshape(6), 0.05, s.reshape(6), A, B)
    assert torch.equal(flat, loss.detach())


# ------------------------------------------------------------------------------------------------ dataset
H5, W7 = 5, 7
INTR = dict(fl_x=6.5, fl_y=5.25, cx=3.1, cy=2.8)


def _options(path, **extra):
    opt = dict(preload=False, bound=2, fp16=False, num_rays=12, rand_pose=-1, error_map=False, color_space="srgb", path=path, scale=0.8,
               offset=[0.1, -0.2, 0.05])
    opt.update(extra)
    return SimpleNamespace(**opt)


def _write_small(root, with_depth=True, ids=None):
    """two 5 x 7 frames with off-centre, anisotropic intrinsics; the second frame has no depth_path"""
    from nerfsafetyvalidation_amd.scene import orbit_poses
    rng = np.random.default_rng(4)
    images = rng.integers(0, 256, (2, H5, W7, 4), dtype=np.uint8)
    depths = rng.uniform(0.4, 3.0, (2, H5, W7))
    depths[0, 0, :4] = [np.nan, -1.0, 0.0, np.inf]
    ids = 3.0 / 65534 if ids is None else ids
    depths[0, 1, 0], depths[0, 1, 1], depths[0, 1, 2] = 1e-9, 65534 * ids, 100.0          # codes 1, 65534 and 65534 (clipped)
    P.write_blender_dataset(root, orbit_poses()[[3, 90]], images, 0.7, "train", scale=0.8, offset=(0.1, -0.2, 0.05),
                            depths=depths if with_depth else None, integer_depth_scale=ids if with_depth else None)
    path = os.path.join(root, "transforms_train.json")
    meta = json.load(open(path))
    meta.update(INTR, w=W7, h=H5)
    if with_depth:
        del meta["frames"][1]["depth_path"]
    json.dump(meta, open(path, "w"))
    return depths, ids


def test_writer_and_dataset_round_trip(tmp_path):
    root = str(tmp_path / "d")
    depths, ids = _write_small(root)
    meta = json.load(open(os.path.join(root, "transforms_train.json")))
    assert meta["integer_depth_scale"] == ids and meta["frames"][0]["depth_path"] == "./train/r_0_depth.png"
    d = P.NeRFDataset(_options(root, lambda_depth=0.1), "cpu", type="train")
    assert d.depths.data.dtype == torch.int16 and tuple(d.depths.data.shape) == (2, H5 * W7)
    codes = d.depths.codes([0, 1]).numpy().reshape(2, H5, W7)
    assert codes[0, 0, :4].tolist() == [0, 0, 0, 65535] and codes[0, 1, :3].tolist() == [1, 65534, 65534]      # the four special codes survive
    assert (codes[1] == 0).all()                                                                             # no depth_path: all zero
    assert np.array_equal(codes[0], TG.encode_depth(depths[0], ids))
    assert abs(d.depths.unit - np.float32(ids * 0.8)) <= 2.0 ** -24 * ids

    torch.manual_seed(0)
    batch = d.collate([0])
    got = batch["depth"]
    assert got.dtype == torch.float32 and tuple(got.shape) == (1, 12)
    # the same pixels again (collate draws them): seed, draw, compare with the float64 formula
    torch.manual_seed(0)
    pix = torch.randint(0, H5 * W7, size=[12]).numpy()
    i, j = pix % W7, pix // W7
    length = np.sqrt(((i + 0.5 - INTR["cx"]) / INTR["fl_x"]) ** 2 + ((j + 0.5 - INTR["cy"]) / INTR["fl_y"]) ** 2 + 1.0)
    z = depths[0].reshape(-1)[pix]
    for k in range(12):
        g = float(got[0, k])
        if np.isposinf(z[k]):
            assert g == np.inf
        elif not z[k] > 0:
            assert g == 0.0
        else:
            want = min(max(z[k], ids), 65534 * ids) * 0.8 * length[k]
            assert abs(g - want) <= 0.5 * ids * 0.8 * length[k] + 8 * 2.0 ** -24 * want, (k, g, want)
    # the direction get_rays forms before it normalises it has z component 1: the ray distance is z-depth times its length
    import shutil
    shutil.copy(os.path.join(root, "transforms_train.json"), os.path.join(root, "transforms_val.json"))
    full = P.NeRFDataset(_options(root, lambda_free=0.1), "cpu", type="val").collate([0])["depth"]
    assert tuple(full.shape) == (1, H5 * W7) and float(full[0, 3]) == np.inf and float(full[0, 0]) == 0.0


def test_depth_files_are_not_read_when_the_terms_are_off(tmp_path):
    a, b = str(tmp_path / "with"), str(tmp_path / "without")
    _write_small(a, True)
    _write_small(b, False)
    for extra in (dict(), dict(lambda_depth=0, lambda_free=0)):
        da, db = P.NeRFDataset(_options(a, **extra), "cpu", type="train"), P.NeRFDataset(_options(b, **extra), "cpu", type="train")
        assert da.depths is None
        torch.manual_seed(1)
        ba = da.collate([1])
        torch.manual_seed(1)
        bb = db.collate([1])
        assert list(ba) == list(bb) and "depth" not in ba
        for k in ba:
            assert torch.equal(ba[k], bb[k]) if torch.is_tensor(ba[k]) else ba[k] == bb[k], k
    # a dataset WITHOUT depth files and the term on: all-zero maps, no measurement anywhere
    dz = P.NeRFDataset(_options(b, lambda_depth=1.0), "cpu", type="train")
    assert (dz.collate([0])["depth"] == 0).all()


def test_downscale_with_depth_raises(tmp_path):
    root = str(tmp_path / "d")
    _write_small(root)
    with pytest.raises(NotImplementedError):
        P.NeRFDataset(_options(root, lambda_depth=0.1), "cpu", type="train", downscale=2)
    P.NeRFDataset(_options(root), "cpu", type="train", downscale=2)                  # the term off: loads as before


def test_make_mesh_dataset_writes_the_worlds_depth(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import make_mesh_dataset as MD
    finally:
        sys.path.pop(0)
    from nerfsafetyvalidation_amd import scene as SC
    from nerfsafetyvalidation_amd import world as WO
    from nerfsafetyvalidation_amd.nerf.utils import get_rays
    out = MD.make(str(tmp_path / "ds"), size=16, n_train=2, n_val=1, n_test=1, device="cpu", resolution=16, depth=True)
    opt = _options(out, scale=1.0, offset=[0, 0, 0], lambda_depth=1.0, lambda_free=1.0)
    d = P.NeRFDataset(opt, "cpu", type="val")
    ids = json.load(open(os.path.join(out, "transforms_val.json")))["integer_depth_scale"]
    got = d.collate([0])["depth"][0].numpy()
    v, f, c = SC.henge_mesh(16)
    world = WO.MeshWorld(torch.from_numpy(v), torch.from_numpy(f), None if c is None else torch.from_numpy(c))
    rays = get_rays(d.poses[:1], d.intrinsics, 16, 16)
    want = world.cast(rays["rays_o"].reshape(-1, 3), rays["rays_d"].reshape(-1, 3))["t"].numpy().astype(np.float64)
    miss = np.isposinf(want)
    assert 0 < miss.sum() < miss.size and np.array_equal(np.isposinf(got), miss)
    fx_, fy_, cx_, cy_ = d.intrinsics
    i, j = np.arange(256) % 16, np.arange(256) // 16
    length = np.sqrt(((i + 0.5 - cx_) / fx_) ** 2 + ((j + 0.5 - cy_) / fy_) ** 2 + 1.0)
    bound = 0.5 * ids * length + 16 * 2.0 ** -24 * np.where(miss, 0, want)
    assert (np.abs(got[~miss] - want[~miss]) <= bound[~miss]).all(), np.abs(got[~miss] - want[~miss]).max()
    assert (got[~miss] > 0).all()


# ------------------------------------------------------------------------------------------------ Trainer and entry point
class StubModel(torch.nn.Module):
    """what train_step needs of a model; `render` records its keyword arguments and returns the depth term only when it got a target"""
    bg_radius, cuda_ray = -1, False

    def __init__(self):
        super().__init__()
        self.color = torch.nn.Parameter(torch.tensor([0.1, -0.2, 0.3]))
        self.term = torch.nn.Parameter(torch.tensor(0.25))
        self.calls = []

    def invalidate_fused(self):
        pass

    def render(self, rays_o, rays_d, staged=False, bg_color=None, perturb=False, **kwargs):
        self.calls.append(kwargs)
        out = {"image": torch.sigmoid(self.color).expand(1, rays_o.shape[1], 3) + 0 * rays_d}
        if kwargs.get("depth_target") is not None:
            out["loss_depth"] = self.term * self.term
            out["loss_depth_parts"] = torch.tensor([0.5, 0.25])
        return out


def trainer_with(tmp_path, model, **extra):
    opt = SimpleNamespace(color_space="srgb", rand_pose=-1, update_extra_interval=16, fp16=False, num_rays=16, error_map=False, **extra)
    return T.Trainer("ngp", opt, model, device="cpu", workspace=str(tmp_path), criterion=torch.nn.MSELoss(reduction="none"), mute=True,
                     use_tensorboardX=False, use_checkpoint="scratch")


def batch(with_depth):
    g = torch.Generator().manual_seed(2)
    data = {"rays_o": torch.zeros(1, 9, 3), "rays_d": torch.zeros(1, 9, 3), "images": torch.rand(1, 9, 3, generator=g)}
    if with_depth:
        data["depth"] = torch.rand(1, 9, generator=g) + 0.5
    return data


def test_train_step_adds_the_depth_term(tmp_path):
    plain = trainer_with(tmp_path / "a", StubModel()).train_step(batch(False))[2]
    model = StubModel()
    trainer = trainer_with(tmp_path / "b", model, lambda_depth=0.5, lambda_free=0.0, depth_margin=0.03)
    data = batch(True)
    loss = trainer.train_step(data)[2]
    call = model.calls[0]
    assert call["lambda_depth"] == 0.5 and call["lambda_free"] == 0.0 and call["depth_margin"] == 0.03
    assert torch.equal(call["depth_target"], data["depth"])
    assert abs(loss.item() - (plain.item() + 0.25 ** 2)) <= 1e-7           # the renderer's term is already weighted
    assert trainer.last_loss_depth is not None and abs(trainer.last_loss_depth.item() - 0.0625) <= 1e-8
    assert trainer.last_loss_depth_parts.tolist() == [0.5, 0.25]
    loss.backward()
    assert abs(model.term.grad.item() - 2 * 0.25) <= 1e-7


@pytest.mark.parametrize("extra", [dict(), dict(lambda_depth=0, lambda_free=0)])
def test_train_step_without_the_term_is_unchanged(tmp_path, extra):
    plain = trainer_with(tmp_path / "a", StubModel()).train_step(batch(False))[2]
    model = StubModel()
    trainer = trainer_with(tmp_path / "b", model, **extra)
    loss = trainer.train_step(batch(True))[2]                               # a batch that carries depth, the term off
    assert "depth_target" not in model.calls[0] and torch.equal(loss, plain) and trainer.last_loss_depth is None
    # the term on, a batch without depth (a dataset of another kind): nothing to add
    model = StubModel()
    trainer = trainer_with(tmp_path / "c", model, lambda_free=0.2)
    assert torch.equal(trainer.train_step(batch(False))[2], plain) and trainer.last_loss_depth is None


def test_parser_knows_the_depth_flags():
    opt = main_nerf.parse_args(["data"])
    assert opt.lambda_depth == 0 and opt.lambda_free == 0 and opt.depth_margin == 0.02
    opt = main_nerf.parse_args(["data", "--lambda_depth", "0.1", "--lambda_free", "1e-2", "--depth_margin", "0.05"])
    assert (opt.lambda_depth, opt.lambda_free, opt.depth_margin) == (0.1, 1e-2, 0.05)
