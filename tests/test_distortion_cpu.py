"""nerfsafetyvalidation_amd/loss.py on the CPU against the reference's own loss.py (tests/golden/distortion.npz, float64), and the
distortion term's way through Trainer.train_step and main_nerf's parser.  No GPU."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from nerfsafetyvalidation_amd import loss as LS
from nerfsafetyvalidation_amd import main_nerf
from nerfsafetyvalidation_amd.nerf import trainer as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
T_PAD = 1024
# float64 results of the same formula in another order of operations: a few hundred roundings of 1.1e-16 on sums of up to 1024 terms
F64_TOL = 1e-12


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "distortion.npz")))


def dense_of(fx, tag, dtype=np.float64):
    """the fixture's packed per-sample arrays as [N, 1024] padded with zeros, rows in table order"""
    rays = fx["rays"]
    out = {k: np.zeros((rays.shape[0], T_PAD), dtype=dtype) for k in ("w", "m", "interval", "grad_w64")}
    for n, (_, offset, count) in enumerate(rays):
        for k in out:
            out[k][n, :count] = fx[f"dense_{k}_{tag}"][offset:offset + count]
    return out


def test_mape_and_huber_match_the_reference(fx):
    pred, target = torch.from_numpy(fx["pair_pred"]), torch.from_numpy(fx["pair_target"])
    assert np.allclose(LS.mape_loss(pred, target).numpy(), fx["mape_mean"], rtol=1e-14, atol=0)
    assert np.allclose(LS.mape_loss(pred, target, reduction="none").numpy(), fx["mape_none"], rtol=1e-14, atol=0)
    assert np.allclose(LS.huber_loss(pred, target).numpy(), fx["huber_mean"], rtol=1e-14, atol=0)
    none = LS.huber_loss(pred, target, reduction="none").numpy()
    assert none.shape == (7, 3) and np.allclose(none, fx["huber_none"], rtol=1e-14, atol=0)
    assert np.allclose(LS.huber_loss(pred, target, delta=0.3).numpy(), fx["huber_delta03_mean"], rtol=1e-14, atol=0)
    r = np.abs(fx["pair_pred"] - fx["pair_target"])
    assert (r > 0.1).any() and (r < 0.1).any()            # both branches of the Huber loss are in the fixture


@pytest.mark.parametrize("tag", ["s", "1"])
def test_eff_distloss_cpu_matches_the_reference_per_ray(fx, tag):
    d = dense_of(fx, tag)
    w = torch.from_numpy(d["w"]).requires_grad_(True)
    loss = LS.eff_distloss(w, torch.from_numpy(d["m"]), torch.from_numpy(d["interval"]))
    want = fx[f"dense_loss64_{tag}"]
    assert abs(loss.item() - want.sum() / len(want)) <= F64_TOL * want.sum() / len(want)          # [B, N]: the mean over the B rays
    loss.backward()
    got = w.grad.numpy() * len(want)                                                              # the fixture's gradients are per ray (/ 1)
    gmax = np.abs(d["grad_w64"]).max(axis=1, keepdims=True)
    real = np.arange(T_PAD)[None, :] < fx["rays"][:, 2:3]                                         # (the padding has gradients too; the fixture holds the rays')
    assert (np.abs(got - d["grad_w64"])[real] <= (F64_TOL * np.broadcast_to(gmax, got.shape))[real]).all()
    # one ray at a time: the per-ray losses
    for n in (1, 5, 10, 14, 36):
        one = LS.eff_distloss(torch.from_numpy(d["w"][n]), torch.from_numpy(d["m"][n]), torch.from_numpy(d["interval"][n]))
        assert abs(one.item() - want[n]) <= F64_TOL * want[n]


def test_eff_distloss_cpu_scalar_interval_and_leading_shapes(fx):
    for name, interval in (("scalar", float(fx["small_interval_scalar"])), ("tensor", torch.from_numpy(fx["small_interval"]).double())):
        w = torch.from_numpy(fx["small_w"]).double().requires_grad_(True)
        loss = LS.eff_distloss(w, torch.from_numpy(fx["small_m"]).double(), interval)
        assert abs(loss.item() - float(fx[f"small_{name}_loss64"])) <= F64_TOL * float(fx[f"small_{name}_loss64"])
        loss.backward()
        want = fx[f"small_{name}_grad_w64"]
        assert np.abs(w.grad.numpy() - want).max() <= F64_TOL * np.abs(want).max()
    w = torch.from_numpy(fx["lead_w"]).requires_grad_(True)                                        # [2, 3, N]: six rays
    m, interval = torch.from_numpy(fx["lead_m"]).requires_grad_(True), torch.from_numpy(fx["lead_interval"])
    loss = LS.eff_distloss(w, m, interval)
    assert abs(loss.item() - float(fx["lead_loss"])) <= F64_TOL * float(fx["lead_loss"])
    loss.backward()
    assert np.abs(w.grad.numpy() - fx["lead_grad_w"]).max() <= F64_TOL * np.abs(fx["lead_grad_w"]).max()
    assert m.grad is None                                                                          # as in the reference: w only
    # the same six rays as [6, N] give the same number
    flat = LS.eff_distloss(w.detach().reshape(6, -1), m.detach().reshape(6, -1), interval.reshape(6, -1))
    assert abs(flat.item() - loss.item()) <= F64_TOL * loss.item()


def test_eff_distloss_is_the_pairwise_definition():
    """sum_ij w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 delta_i, written out, for sorted m"""
    g = torch.Generator().manual_seed(1)
    w, delta = torch.rand(3, 17, generator=g, dtype=torch.float64), torch.rand(3, 17, generator=g, dtype=torch.float64)
    m = torch.sort(torch.rand(3, 17, generator=g, dtype=torch.float64), dim=-1).values
    pairs = (w[:, :, None] * w[:, None, :] * (m[:, :, None] - m[:, None, :]).abs()).sum((1, 2)) + (w * w * delta).sum(1) / 3
    assert abs(LS.eff_distloss(w, m, delta).item() - pairs.mean().item()) <= F64_TOL * pairs.mean().item()


class StubModel(torch.nn.Module):
    """what train_step needs of a model; `render` records its keyword arguments and returns a distortion term only when told to"""
    bg_radius, cuda_ray = -1, False

    def __init__(self, with_term):
        super().__init__()
        self.color = torch.nn.Parameter(torch.tensor([0.1, -0.2, 0.3]))
        self.term = torch.nn.Parameter(torch.tensor(0.25))
        self.with_term, self.calls = with_term, []

    def invalidate_fused(self):
        pass

    def render(self, rays_o, rays_d, staged=False, bg_color=None, perturb=False, **kwargs):
        self.calls.append(kwargs)
        out = {"image": torch.sigmoid(self.color).expand(1, rays_o.shape[1], 3) + 0 * rays_d}
        if self.with_term:
            out["loss_distort"] = self.term * self.term
        return out


def trainer_with(tmp_path, model, **extra):
    opt = SimpleNamespace(color_space="srgb", rand_pose=-1, update_extra_interval=16, fp16=False, num_rays=16, error_map=False, **extra)
    return T.Trainer("ngp", opt, model, device="cpu", workspace=str(tmp_path), criterion=torch.nn.MSELoss(reduction="none"), mute=True,
                     use_tensorboardX=False, use_checkpoint="scratch")


def batch():
    g = torch.Generator().manual_seed(2)
    return {"rays_o": torch.zeros(1, 9, 3), "rays_d": torch.zeros(1, 9, 3), "images": torch.rand(1, 9, 3, generator=g)}


def test_train_step_adds_the_weighted_term(tmp_path):
    plain = trainer_with(tmp_path / "a", StubModel(with_term=False)).train_step(batch())[2]
    model = StubModel(with_term=True)
    trainer = trainer_with(tmp_path / "b", model, lambda_distort=0.5)
    loss = trainer.train_step(batch())[2]
    assert model.calls[0]["lambda_distort"] == 0.5                                  # reaches the renderer through vars(opt)
    assert abs(loss.item() - (plain.item() + 0.5 * 0.25 ** 2)) <= 1e-7
    loss.backward()
    assert abs(model.term.grad.item() - 0.5 * 2 * 0.25) <= 1e-7 and model.color.grad.abs().max() > 0


@pytest.mark.parametrize("extra", [dict(lambda_distort=0), dict()])
def test_train_step_without_the_term_is_unchanged(tmp_path, extra):
    plain = trainer_with(tmp_path / "a", StubModel(with_term=False)).train_step(batch())[2]
    # a render that returns NO loss_distort: a train_step that read the key would raise
    loss = trainer_with(tmp_path / "b", StubModel(with_term=False), **extra).train_step(batch())[2]
    assert torch.equal(loss, plain)
    model = StubModel(with_term=True)
    loss = trainer_with(tmp_path / "c", model, **extra).train_step(batch())[2]
    assert torch.equal(loss, plain)
    loss.backward()
    assert model.term.grad is None


def test_parser_knows_lambda_distort():
    assert main_nerf.parse_args(["data"]).lambda_distort == 0
    assert main_nerf.parse_args(["data", "--lambda_distort", "1e-3"]).lambda_distort == 1e-3
