"""Depth supervision in float64 numpy, from the definitions of DESIGN.md "Depth supervision" (this file's own code), on the packed rays
of tests/golden/distortion.npz: 37 rays with counts {0, 1, 2, 63, 64, 65, 127, 128, 129, 200, 1024, ...}, a dropped ray, rows no ray
owns and a shuffled `index` column.  The fixture's `n_live` is the live length of every ray, so that float64 does not re-decide a stop
that float32 made.

Targets are assigned to the table's rows by a fixed rule (`CASES`, row n takes case n mod 11; a ray too short for a midpoint case takes
the midpoint of its first two samples, a ray of one sample `beyond`) so that every case occurs:

    zero, nan, neg   no measurement                     inf      known empty
    before           z - margin before the first sample (empty front set)
    beyond           z - margin behind the last live sample (all front)
    mid<j>           z - margin at the midpoint between samples j and j + 1, j in {0, 62, 63, 64, 127}

Condition, asserted here in float64 on the float32 targets the tests use: no live t_i lies closer to z - margin than a quarter of the
local gap (the distance between the two samples that bracket z - margin; the first gap, the last gap at the ends), and that gap is
positive.  A float32 kernel then cannot land on the other side of the indicator.  A midpoint that violates it (two samples at the same
depth) is replaced by the next bracket behind it that passes."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MARGIN = float(np.float32(0.02))
CASES = ["zero", "before", "mid0", "nan", "inf", "mid63", "mid62", "mid64", "neg", "beyond", "mid127"]
NO_MEASUREMENT = ("zero", "nan", "neg")


def load():
    return dict(np.load(os.path.join(GOLDEN, "distortion.npz")))


def ray_rows(fx, n):
    """table row n -> (slot, slice of its packed rows, live samples, takes part)"""
    slot, offset, count = [int(v) for v in fx["rays"][n]]
    return slot, slice(offset, offset + count), int(fx["n_live"][n]), count > 0 and not bool(fx["dropped"][n])


def weights64(sigma, dt, gap, n_live):
    """-> w, t, T_next of one ray; w is 0 behind the stop"""
    sigma, dt, gap = [np.asarray(a, dtype=np.float64) for a in (sigma, dt, gap)]
    alpha = 1.0 - np.exp(-sigma * dt)
    T_next = np.cumprod(1.0 - alpha)
    T = np.concatenate([[1.0], T_next[:-1]])
    w = alpha * T
    w[n_live:] = 0.0
    return w, np.cumsum(gap), T_next


def _bracket_ok(t_live, lo):
    """the midpoint between live samples lo and lo + 1 -> (threshold, passes the quarter-gap condition)"""
    gap = t_live[lo + 1] - t_live[lo]
    return 0.5 * (t_live[lo] + t_live[lo + 1]), gap > 0


def make_targets(fx, margin=MARGIN):
    """-> (target float32 [N] by SLOT, case name per table row).  Asserts that every case occurs and the condition of the module
    docstring on every finite target."""
    N = fx["rays"].shape[0]
    target = np.zeros(N, dtype=np.float32)
    names = []
    for n in range(N):
        slot, rows, n_live, _ = ray_rows(fx, n)
        case = CASES[n % len(CASES)]
        t = np.cumsum(fx["deltas"][rows, 1].astype(np.float64))[:n_live]
        if case.startswith("mid") and n_live < int(case[3:]) + 2:
            case = "mid0" if n_live >= 2 else "beyond"
        if n_live == 0:
            case = "zero"
        if case == "zero":
            z = 0.0
        elif case == "nan":
            z = np.nan
        elif case == "neg":
            z = -1.5
        elif case == "inf":
            z = np.inf
        elif case == "before":
            z = 0.5 * t[0] + margin
        elif case == "beyond":
            z = t[-1] + 0.5 * max(t[-1] - (t[-2] if n_live > 1 else 0.0), 1e-3) + margin
        else:
            lo = int(case[3:])
            thr, ok = _bracket_ok(t, lo)
            while not ok:                      # (two samples at one depth: the next bracket behind it)
                lo += 1
                thr, ok = _bracket_ok(t, lo)
            z = thr + margin
        target[slot] = np.float32(z)
        names.append(case)
        if np.isfinite(target[slot]) and target[slot] > 0:
            thr = float(target[slot]) - float(np.float32(margin))
            behind = int(np.searchsorted(t, thr))                  # live samples in front of the threshold
            if behind == 0:
                local = t[0]
            elif behind == n_live:
                local = t[-1] - t[-2] if n_live > 1 else t[-1]
            else:
                local = t[behind] - t[behind - 1]
            assert local > 0 and np.min(np.abs(t - thr)) >= 0.25 * local, (n, case, local, np.min(np.abs(t - thr)))
            assert np.min(np.abs(t - thr)) > 64 * 2.0 ** -24 * max(1.0, t[-1]), (n, case)
    assert set(names) == set(CASES), sorted(set(CASES) - set(names))
    return target, names


def ray_loss64(w, t, z, margin, scale, a, b):
    """one ray from its weights -> (L_ray, d, A, g [len(w)])"""
    w, t = np.asarray(w, dtype=np.float64), np.asarray(t, dtype=np.float64)
    if not z > 0:
        return 0.0, 0.0, 0.0, np.zeros_like(w)
    front = (t < z - margin).astype(np.float64)
    d, A = float(np.sum(w * t)), float(np.sum(w * front))
    if np.isinf(z):
        return b * A, d, A, b * front
    return a * (scale * (d - z)) ** 2 + b * A, d, A, 2 * a * scale ** 2 * (d - z) * t + b * front


def packed64(fx, target, scale=None, margin=MARGIN, a=1.0, b=1.0):
    """the packed operator in float64 -> dict(loss_rays [N] by SLOT, parts [N,2] by SLOT, grad_sigma [M] of sum(L_ray), live [M] bool,
    mean)"""
    N, M = fx["rays"].shape[0], int(fx["M"])
    out = dict(loss_rays=np.zeros(N), parts=np.zeros((N, 2)), grad_sigma=np.zeros(M), live=np.zeros(M, dtype=bool))
    margin = float(np.float32(margin))
    for n in range(N):
        slot, rows, n_live, takes_part = ray_rows(fx, n)
        if not takes_part:
            continue
        z = float(target[slot])
        s = 1.0 if scale is None else float(scale[slot])
        w, t, T_next = weights64(fx["sigmas"][rows], fx["deltas"][rows, 0], fx["deltas"][rows, 1], n_live)
        L, d, A, g = ray_loss64(w[:n_live], t[:n_live], z, margin, s, a, b)
        out["loss_rays"][slot], out["parts"][slot] = L, (d, A)
        out["live"][rows.start:rows.start + n_live] = True
        gw = g * w[:n_live]
        after = np.concatenate([np.cumsum(gw[::-1])[::-1][1:], [0.0]])              # sum_{k>i, live} g_k w_k
        dt = fx["deltas"][rows, 0].astype(np.float64)[:n_live]
        out["grad_sigma"][rows.start:rows.start + n_live] = dt * (T_next[:n_live] * g - after)
    out["mean"] = out["loss_rays"].sum() / N
    return out


def ray_loss_of_sigma64(fx, n, sigma, z, s, margin, a, b):
    """L_ray of table row n with its densities replaced by `sigma` (the live length stays the fixture's): for finite differences"""
    _, rows, n_live, _ = ray_rows(fx, n)
    w, t, _ = weights64(sigma, fx["deltas"][rows, 0], fx["deltas"][rows, 1], n_live)
    return ray_loss64(w[:n_live], t[:n_live], z, float(np.float32(margin)), s, a, b)[0]


def torch_chain(fx, target, scale, dtype, margin=MARGIN, a=1.0, b=1.0):
    """The same computation as a torch chain on the CPU in `dtype` (sigma -> alpha -> cumprod -> w, cumsum -> t, the loss, autograd):
    the float32 yardstick of the GPU tests.  -> dict like packed64's."""
    N, M = fx["rays"].shape[0], int(fx["M"])
    out = dict(loss_rays=np.zeros(N), parts=np.zeros((N, 2)), grad_sigma=np.zeros(M))
    mg = torch.tensor(float(np.float32(margin)), dtype=dtype)
    for n in range(N):
        slot, rows, n_live, takes_part = ray_rows(fx, n)
        z = torch.tensor(float(target[slot]), dtype=dtype)
        if not takes_part or not bool(z > 0):
            continue
        s = torch.tensor(1.0 if scale is None else float(scale[slot]), dtype=dtype)
        sigma = torch.tensor(fx["sigmas"][rows], dtype=dtype, requires_grad=True)
        dt, gap = torch.tensor(fx["deltas"][rows, 0], dtype=dtype), torch.tensor(fx["deltas"][rows, 1], dtype=dtype)
        alpha = 1 - torch.exp(-sigma * dt)
        T = torch.cat([torch.ones(1, dtype=dtype), torch.cumprod(1 - alpha, 0)[:-1]])
        w = (alpha * T)[:n_live]
        t = torch.cumsum(gap, 0)[:n_live]
        d, A = (w * t).sum(), (w * (t < z - mg).to(dtype)).sum()
        L = b * A if bool(torch.isinf(z)) else a * (s * (d - z)) ** 2 + b * A
        L.backward()
        out["loss_rays"][slot], out["parts"][slot] = float(L.detach()), (float(d.detach()), float(A.detach()))
        out["grad_sigma"][rows] = sigma.grad.double().numpy()
    return out


def errors(fx, got, want):
    """worst errors over the rays that take part: loss_rays and parts relative to the ray's float64 value (where that is not 0),
    grad_sigma relative to the ray's max |gradient| -> dict(loss, d, A, grad)"""
    e = dict(loss=0.0, d=0.0, A=0.0, grad=0.0)
    for n in range(fx["rays"].shape[0]):
        slot, rows, n_live, takes_part = ray_rows(fx, n)
        if not takes_part:
            continue
        for key, g, w in (("loss", got["loss_rays"][slot], want["loss_rays"][slot]), ("d", got["parts"][slot, 0], want["parts"][slot, 0]),
                          ("A", got["parts"][slot, 1], want["parts"][slot, 1])):
            if w != 0:
                e[key] = max(e[key], abs(float(g) - w) / abs(w))
        live = slice(rows.start, rows.start + n_live)
        gmax = np.abs(want["grad_sigma"][live]).max()
        if gmax > 0:
            e["grad"] = max(e["grad"], float(np.abs(got["grad_sigma"][live] - want["grad_sigma"][live]).max() / gmax))
    return e


def dense64(w, t, target, scale=None, margin=MARGIN, a=1.0, b=1.0):
    """dense [B,T] weights -> (loss_rays [B], g [B,T] = d sum(L_ray) / dw)"""
    w, t = np.asarray(w, dtype=np.float64), np.asarray(t, dtype=np.float64)
    loss, g = np.zeros(w.shape[0]), np.zeros_like(w)
    for r in range(w.shape[0]):
        loss[r], _, _, g[r] = ray_loss64(w[r], t[r], float(target[r]), float(np.float32(margin)), 1.0 if scale is None else float(scale[r]), a, b)
    return loss, g
