#!/usr/bin/env python3
"""Generates tests/golden/distortion.npz by running the REFERENCE's own loss.py (eff_distloss, mape_loss, huber_loss) on CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_distortion.py

The reference module is imported from /root/reference unmodified.  The fixture is a set of 37 rays in march_rays_train's packed
layout (sigmas [M], deltas [M,2] = (dt, gap), rays int32 [N,3] = (index, offset, count), scale [N] per slot) and the same rays padded
to 1024 samples with zero weights, which contribute nothing.  Per ray, in TABLE-ROW order (ray n's slot is rays[n, 0]), it records, from
the reference's function evaluated on ONE ray at a time (so that its "/ n_rays" is "/ 1"):

    loss                  float64, and the same evaluated in float32 on the CPU
    grad_sigma            [M], packed rows: autograd through w(sigma) (this script's statement of composite_rays_train's forward rule:
                          alpha = 1 - exp(-sigma dt), T the exclusive cumprod of 1 - alpha, the ray ending behind the first sample with
                          T_{i+1} < 1e-4) and the reference's function, float64 and float32
    dense_w / _m / _interval   [M], packed rows: the float32 w, m = scale * cumsum(gap), scale * dt of every ray (the last, which the
                          packed operator drops, included) -- the inputs of the dense case, which a test pads to [N, 1024]
    dense_loss, dense_grad_w   the reference's forward and its OWN backward on those float32 arrays, float64 and float32

each with scale = the random per-ray factor ("_s") and with scale = 1 ("_1").  err_* are the worst float32-versus-float64 errors over
the rays -- loss relative to the ray's float64 loss, gradients relative to the ray's max |gradient| -- the yardstick the GPU tests'
tolerance is formed from.  mape_* / huber_* are the other two losses on a small random pair, both reductions.  Arrays only.

Condition on the inputs, asserted here in float64: no T_{i+1} of any ray lies within a relative 1e-3 of 1e-4, so every order of
forming T picks the same stopping sample."""
import importlib.util
import os
import sys

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

import numpy as np  # noqa: E402
import torch  # noqa: E402

SEED = 20
T_PAD = 1024
STOP = 1e-4
COUNTS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 200, 1024]
N_RAYS = 37
GAP_BEFORE, GAP = 20, 7


def build_rays(rng):
    """-> list of dicts(sigma, dt, gap) in table-row order, with the special rays the tests name"""
    rays = []

    def plain(count, density=None):
        dt = rng.uniform(0.002, 0.01, count)
        gap = dt + (rng.uniform(0, 1, count) < 0.2) * rng.uniform(0.0, 0.05, count)      # a jump over empty space now and then
        peak = rng.uniform(5.0, 40.0) if density is None else density
        sigma = peak * rng.uniform(0, 1, count) ** 2
        return dict(sigma=sigma, dt=dt, gap=gap)

    for c in COUNTS:
        # (an optical depth of about 3 over the whole ray: every sample of these lengths stays live)
        rays.append(plain(c, density=min(200.0, 1500.0 / max(c, 1))))
    zero = plain(70)
    zero["sigma"][:] = 0.0
    rays.append(dict(zero, tag="zero_sigma"))
    rep = plain(90, density=6.0)
    rep["gap"][rng.uniform(0, 1, 90) < 0.3] = 0.0                                          # repeated depths
    rays.append(dict(rep, tag="repeat"))
    for count, stop_at, tag in ((100, 63, "stop63"), (130, 64, "stop64"), (150, 40, "stop40")):
        r = plain(count, density=2.0)
        r["sigma"][stop_at + 1:] = rng.uniform(5, 50, count - stop_at - 1)                 # dead samples with density: they must not count
        # place the crossing: after stop_at - 1 samples T is far above 1e-4; the stopping sample takes it to 0.3e-4
        od = float(np.sum(r["sigma"][:stop_at] * r["dt"][:stop_at]))
        r["sigma"][stop_at] = (-np.log(0.3 * STOP) - od) / r["dt"][stop_at]
        rays.append(dict(r, tag=tag, stop_at=stop_at))
    while len(rays) < N_RAYS - 1:
        rays.append(plain(int(rng.integers(1, 180))))
    rays.append(dict(plain(33), tag="dropped"))                                            # the last rows of the arrays: offset + count == M
    assert len(rays) == N_RAYS
    return rays


def live_count(sigma, dt):
    """float64: the number of live samples and the margin of every T_{i+1} from the threshold"""
    T = np.cumprod(np.exp(-sigma * dt))
    margin = np.min(np.abs(T / STOP - 1.0)) if len(T) else np.inf
    hit = np.nonzero(T < STOP)[0]
    return (int(hit[0]) + 1 if len(hit) else len(T)), margin


def weights_of(sigma, dt, n_live):
    """torch, differentiable: w_i = alpha_i T_i for i < n_live, 0 beyond"""
    alpha = 1 - torch.exp(-sigma * dt)
    T = torch.cat([torch.ones(1, dtype=sigma.dtype), torch.cumprod(1 - alpha, 0)[:-1]])
    keep = (torch.arange(sigma.shape[0]) < n_live).to(sigma.dtype)
    return alpha * T * keep


def evaluate(ref, ray, scale, n_live, dtype):
    """one ray through the reference, padded to T_PAD -> (loss, grad_w [count], grad_sigma [count])"""
    count = len(ray["sigma"])
    sigma = torch.tensor(ray["sigma"], dtype=dtype, requires_grad=True)
    dt, gap = torch.tensor(ray["dt"], dtype=dtype), torch.tensor(ray["gap"], dtype=dtype)
    s = torch.tensor(scale, dtype=dtype)
    w = weights_of(sigma, dt, n_live)
    m, delta = s * torch.cumsum(gap, 0), s * dt
    pad = torch.zeros(T_PAD - count, dtype=dtype)
    w_leaf = torch.cat([w.detach(), pad]).requires_grad_(True)
    m_pad, d_pad = torch.cat([m, pad]), torch.cat([delta, pad])
    loss = ref.eff_distloss(w_leaf[None], m_pad[None], d_pad[None])
    loss.backward()
    grad_w = w_leaf.grad[:count].clone()
    ref.eff_distloss(torch.cat([w, pad])[None], m_pad[None], d_pad[None]).backward()
    return loss.detach(), grad_w, sigma.grad.clone(), (w.detach(), m, delta)


def main():
    spec = importlib.util.spec_from_file_location("ref_loss", os.path.join(REF, "loss.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    rng = np.random.default_rng(SEED)
    rays = build_rays(rng)
    # float32 inputs are THE inputs: everything below starts from their exact values
    for r in rays:
        for k in ("sigma", "dt", "gap"):
            r[k] = r[k].astype(np.float32)
    for r in rays:                       # the constructed crossings, re-placed on the rounded values
        if "stop_at" in r:
            k = r["stop_at"]
            od = float(np.sum(r["sigma"][:k].astype(np.float64) * r["dt"][:k].astype(np.float64)))
            r["sigma"][k] = np.float32((-np.log(0.3 * STOP) - od) / float(r["dt"][k]))
    N = len(rays)
    index = rng.permutation(N).astype(np.int32)
    assert not np.array_equal(index, np.arange(N))
    scale = rng.uniform(0.2, 0.7, N).astype(np.float32)                 # indexed by slot

    counts = np.array([len(r["sigma"]) for r in rays], dtype=np.int32)
    # GAP rows that no ray owns lie before ray GAP_BEFORE (march_rays_train leaves none, a hand-built table may): they hold values, not zeros
    offsets = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int32)
    offsets[GAP_BEFORE:] += GAP
    M = int(counts.sum()) + GAP
    assert offsets[-1] + counts[-1] == M and rays[-1]["tag"] == "dropped"
    sigmas = rng.uniform(1, 30, M).astype(np.float32)
    deltas = rng.uniform(0.002, 0.01, (M, 2)).astype(np.float32)
    owned = np.zeros(M, dtype=bool)
    for r, o, c in zip(rays, offsets, counts):
        sigmas[o:o + c], deltas[o:o + c, 0], deltas[o:o + c, 1] = r["sigma"], r["dt"], r["gap"]
        owned[o:o + c] = True
    assert (~owned).sum() == GAP
    table = np.stack([index, offsets, counts], axis=1).astype(np.int32)

    n_live = np.zeros(N, dtype=np.int32)        # per table row
    margins = []
    for n, r in enumerate(rays):
        n_live[n], margin = live_count(r["sigma"].astype(np.float64), r["dt"].astype(np.float64))
        margins.append(margin)
        assert margin > 1e-3, (n, margin)
        if "stop_at" in r:
            assert n_live[n] == r["stop_at"] + 1 and margin > 0.5, (r["tag"], n_live[n], margin)
        elif n < len(COUNTS):
            assert n_live[n] == counts[n], (n, n_live[n], counts[n])     # the rays of the named lengths keep every sample
    dropped = np.zeros(N, dtype=bool)
    dropped[-1] = True

    out = dict(sigmas=sigmas, deltas=deltas, rays=table, scale=scale, n_live=n_live, dropped=dropped, owned=owned, M=np.int64(M),
               stop_margin_min=np.float64(min(margins)))
    err = {}

    def dense_eval(w32, m32, d32, dtype):
        """the float32 arrays are the inputs of the dense case: the reference on them, padded with zero weights"""
        pad = torch.zeros(T_PAD - w32.shape[0], dtype=dtype)
        w = torch.cat([w32.to(dtype), pad]).requires_grad_(True)
        loss = ref.eff_distloss(w[None], torch.cat([m32.to(dtype), pad])[None], torch.cat([d32.to(dtype), pad])[None])
        loss.backward()
        return float(loss.detach()), w.grad[:w32.shape[0]].numpy()

    # per-ray results are in TABLE-ROW order (the operator writes ray n's loss to slot rays[n, 0]); per-sample results in packed-row order
    for tag, use_scale in (("s", True), ("1", False)):
        f = {k: np.zeros(M, dtype=np.float64) for k in ("grad_sigma64", "grad_sigma32", "dense_grad_w64", "dense_grad_w32")}
        dense = {k: np.zeros(M, dtype=np.float32) for k in ("w", "m", "interval")}
        loss64, loss32, dl64, dl32 = np.zeros(N), np.zeros(N), np.zeros(N), np.zeros(N)
        e = dict(loss=0.0, grad_sigma=0.0, dense_loss=0.0, dense_grad_w=0.0)
        for n, r in enumerate(rays):
            slot, count, at = int(index[n]), int(counts[n]), slice(int(offsets[n]), int(offsets[n]) + int(counts[n]))
            if count == 0:
                continue
            sc = float(scale[slot]) if use_scale else 1.0
            l64, _, gs64, _ = evaluate(ref, r, sc, int(n_live[n]), torch.float64)
            l32, _, gs32, (w32, m32, d32) = evaluate(ref, r, sc, int(n_live[n]), torch.float32)
            if not dropped[n]:
                loss64[n], loss32[n] = float(l64), float(l32)
                f["grad_sigma64"][at], f["grad_sigma32"][at] = gs64.numpy(), gs32.numpy()
                if float(l64) > 0:
                    e["loss"] = max(e["loss"], abs(float(l32) - float(l64)) / float(l64))
                    e["grad_sigma"] = max(e["grad_sigma"], float((gs32.double() - gs64).abs().max() / gs64.abs().max()))
            dense["w"][at], dense["m"][at], dense["interval"][at] = w32.numpy(), m32.numpy(), d32.numpy()
            dl64[n], g64 = dense_eval(w32, m32, d32, torch.float64)
            dl32[n], g32 = dense_eval(w32, m32, d32, torch.float32)
            f["dense_grad_w64"][at], f["dense_grad_w32"][at] = g64, g32
            if dl64[n] > 0:
                e["dense_loss"] = max(e["dense_loss"], abs(dl32[n] - dl64[n]) / dl64[n])
                e["dense_grad_w"] = max(e["dense_grad_w"], float(np.abs(g32 - g64).max() / np.abs(g64).max()))
        err.update({f"err_{k}_{tag}": v for k, v in e.items()})
        out.update({f"loss64_{tag}": loss64, f"loss32_{tag}": loss32.astype(np.float32), f"dense_loss64_{tag}": dl64,
                    f"dense_loss32_{tag}": dl32.astype(np.float32),
                    f"grad_sigma64_{tag}": f["grad_sigma64"], f"grad_sigma32_{tag}": f["grad_sigma32"].astype(np.float32),
                    f"dense_grad_w64_{tag}": f["dense_grad_w64"], f"dense_grad_w32_{tag}": f["dense_grad_w32"].astype(np.float32),
                    f"dense_w_{tag}": dense["w"], f"dense_m_{tag}": dense["m"], f"dense_interval_{tag}": dense["interval"]})
    out.update({k: np.float64(v) for k, v in err.items()})

    # a small dense case with one interval for every sample (a number), and with leading shape [2, 3, N]
    g = torch.Generator().manual_seed(SEED)
    w_small = torch.rand(5, 65, generator=g) * 0.03
    m_small = torch.sort(torch.rand(5, 65, generator=g), dim=-1).values
    iv = 1.0 / 65
    for name, interval in (("scalar", iv), ("tensor", torch.rand(5, 65, generator=g) * 0.02)):
        for dtype, tag in ((torch.float64, "64"), (torch.float32, "32")):
            w = w_small.detach().clone().to(dtype).requires_grad_(True)
            loss = ref.eff_distloss(w, m_small.to(dtype), interval if name == "scalar" else interval.to(dtype))
            loss.backward()
            out[f"small_{name}_loss{tag}"], out[f"small_{name}_grad_w{tag}"] = loss.detach().numpy(), w.grad.numpy()
        if name == "tensor":
            out["small_interval"] = interval.numpy()
    out["small_w"], out["small_m"], out["small_interval_scalar"] = w_small.numpy(), m_small.numpy(), np.float64(iv)
    w6 = torch.rand(2, 3, 40, generator=g, dtype=torch.float64).requires_grad_(True)
    m6 = torch.sort(torch.rand(2, 3, 40, generator=g, dtype=torch.float64), dim=-1).values
    i6 = torch.rand(2, 3, 40, generator=g, dtype=torch.float64) * 0.05
    loss = ref.eff_distloss(w6, m6, i6)
    loss.backward()
    out.update(lead_w=w6.detach().numpy(), lead_m=m6.numpy(), lead_interval=i6.numpy(), lead_loss=loss.detach().numpy(), lead_grad_w=w6.grad.numpy())

    pred = torch.randn(7, 3, generator=g, dtype=torch.float64) * 0.3
    target = torch.randn(7, 3, generator=g, dtype=torch.float64) * 0.3
    out.update(pair_pred=pred.numpy(), pair_target=target.numpy(),
               mape_mean=ref.mape_loss(pred, target).numpy(), mape_none=ref.mape_loss(pred, target, reduction="none").numpy(),
               huber_mean=ref.huber_loss(pred, target).numpy(), huber_none=ref.huber_loss(pred, target, reduction="none").numpy(),
               huber_delta03_mean=ref.huber_loss(pred, target, delta=0.3).numpy())

    path = os.path.join(HERE, "distortion.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes); M = {M}, min stop margin {min(margins):.3g}")
    for k, v in err.items():
        print(k, f"{v:.3e}")


if __name__ == "__main__":
    main()
