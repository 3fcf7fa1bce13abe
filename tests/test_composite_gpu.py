"""The ray-compositing kernels (k_composite_train_fwd / k_composite_train_bwd / k_composite_rays, csrc/raymarching.hip) and the other
per-ray reduction (ngp_uq_stats, csrc/capi.hip) on hand-built ray tables.

Every reference is written here: float64 numpy recurrences for the forward sums, torch.float64 autograd on the CPU for the gradient of
rays that never stop, and the reference's stop rule restated in float64 for rays that do.  None of them groups steps or fuses
multiply-adds.  Tolerances are not chosen: the float32 CPU oracle is measured against the float64 reference on the very same table and the
kernel is allowed 4x that error (it differs from the oracle by the device's expf against glibc's and by nothing else: both use the
same explicit fmaf calls).  Each test prints the oracle's measured error and the kernel's before it asserts.

Threshold condition: the tables are built so that no transmittance a kernel compares with 1e-4 lies within a factor 1 +- 1e-3 of it
(checked in float64 at build time), so float32 and float64 take the same branch on every step of every ray and no ray is excused.
"""
import functools
import os
import re

import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu

THRESH = 1e-4
MARGIN = 1e-3      # no compared transmittance within THRESH * (1 +- MARGIN)
SENTINEL = 7.0
ORACLE_FACTOR = 4.0


def _t(x, device):
    return torch.from_numpy(np.array(x, order="C")).to(device)      # a copy: the cached tables are read-only


def _clear_of_threshold(T):
    T = np.asarray(T, np.float64)
    return not np.any((T > THRESH * (1 - MARGIN)) & (T < THRESH * (1 + MARGIN)))


def _errs(got, ref):
    """largest absolute and largest relative error of got against the float64 ref"""
    got, ref = np.asarray(got, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    d = np.abs(got - ref)
    nz = ref != 0
    return float(d.max(initial=0.0)), float((d[nz] / np.abs(ref[nz])).max(initial=0.0))


def _within(name, kernel, oracle):
    """kernel error <= 4 x the oracle's error, for each of (absolute, relative); prints both"""
    print(f"{name}: oracle abs {oracle[0]:.3e} rel {oracle[1]:.3e} | kernel abs {kernel[0]:.3e} rel {kernel[1]:.3e}")
    assert kernel[0] <= ORACLE_FACTOR * oracle[0], f"{name}: absolute error {kernel[0]:.3e} > 4 x oracle's {oracle[0]:.3e}"
    assert kernel[1] <= ORACLE_FACTOR * oracle[1], f"{name}: relative error {kernel[1]:.3e} > 4 x oracle's {oracle[1]:.3e}"


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the ray-table builder
# ---------------------------------------------------------------------------------------------------------------------------------
def _train_cases():
    """(num_steps, stop_at): stop_at None = never below 1e-4, else the step whose update takes T below it."""
    cases = []
    for ns in (0, 1, 2, 3, 4, 5, 7, 8, 9, 64, 257):
        stops = sorted({s for s in (0, 1, 2, 3, 4, 5, ns - 1) if 0 <= s < ns})
        cases += [(ns, None)] + [(ns, s) for s in stops]
    # a second zero-step ray, and a stop at every position of the last full group / the group before a one-step tail
    cases += [(0, None), (64, 60), (64, 61), (64, 62), (257, 253), (257, 254), (257, 255)]
    return cases


DROPPED = (5, None)     # laid last: its slab ends exactly at M, so offset + num_steps >= M drops it


def build_ray_table(cases, lead=0, seed=0):
    """rays [N,3] int32 (index, offset, num_steps), sigmas [M], rgbs [M,3], deltas [M,2] and M from (num_steps, stop_at) per ray.
    Slabs lie end to end behind `lead` padding rows, in a shuffled order, so offsets are arbitrary modulo 4; index is a permutation
    without fixed points; the last ray (DROPPED) is the only one with offset + num_steps >= M."""
    rng = np.random.default_rng(seed)
    specs = [cases[i] for i in rng.permutation(len(cases))] + [DROPPED]
    N = len(specs)
    p = rng.permutation(N)
    index = np.empty(N, np.int64)
    index[p] = np.roll(p, -1)                   # one N-cycle: index[n] != n for every n
    assert sorted(index) == list(range(N)) and not np.any(index == np.arange(N))
    rays = np.zeros((N, 3), np.int32)
    off = lead
    for n, (ns, _) in enumerate(specs):
        rays[n] = (index[n], off, ns)
        off += ns
    M = off
    over = rays[:, 1] + rays[:, 2] >= M
    assert over[-1] and not over[:-1].any()
    assert M < 10000

    deltas = np.stack([rng.uniform(0.003, 0.03, M), rng.uniform(0.003, 0.05, M)], axis=1).astype(np.float32)
    rgbs = rng.uniform(0, 1, (M, 3)).astype(np.float32)
    sigmas = rng.uniform(5, 200, M).astype(np.float32)      # what padding, the dropped ray and the steps after a stop keep
    dt = deltas[:, 0].astype(np.float64)
    for n, (ns, stop) in enumerate(specs[:-1]):
        o = int(rays[n, 1])
        if ns == 0:
            continue
        scale = 1.0
        for _ in range(50):
            pre = ns if stop is None else stop
            budget = (8.0 if stop is None else 6.0) * scale      # optical depth of the steps that must not stop the ray (ln 1e4 = 9.2)
            tau = rng.uniform(0.2, 1.0, pre) * budget / max(pre, 1)
            sigmas[o:o + pre] = (tau / dt[o:o + pre]).astype(np.float32)
            if stop is not None:
                T_before = np.prod(np.exp(-sigmas[o:o + pre].astype(np.float64) * dt[o:o + pre]))
                target = THRESH * rng.uniform(0.2, 0.6)
                sigmas[o + stop] = np.float32(np.log(T_before / target) / dt[o + stop])
            T = np.cumprod(1.0 - (1.0 - np.exp(-sigmas[o:o + ns].astype(np.float64) * dt[o:o + ns])))
            crossed = np.flatnonzero(T < THRESH)
            ok = _clear_of_threshold(T) and (len(crossed) == 0 if stop is None else (len(crossed) > 0 and crossed[0] == stop))
            if ok:
                break
            scale *= 0.9        # another sigma scale for this ray (and fresh draws); never an exclusion
        assert ok, f"ray ({ns}, {stop}) cannot be kept clear of the threshold"
    return {"rays": rays, "sigmas": sigmas, "rgbs": rgbs, "deltas": deltas, "M": M, "N": N, "specs": specs, "lead": lead}


def _ref_train_forward(tb):
    """float64 recurrence: the step that takes T below 1e-4 still contributes, then the ray stops.  Also the number of steps whose
    gradient exists (all of them, or those before the stopping step)."""
    N, M, rays = tb["N"], tb["M"], tb["rays"]
    sg, rg, dl = tb["sigmas"].astype(np.float64), tb["rgbs"].astype(np.float64), tb["deltas"].astype(np.float64)
    ws, depth, image = np.zeros(N), np.zeros(N), np.zeros((N, 3))
    n_grad = np.zeros(N, np.int64)
    live = np.zeros(N, bool)
    for n in range(N):
        idx, o, ns = (int(v) for v in rays[n])
        if ns == 0 or o + ns >= M:
            continue
        live[n] = True
        T, t = 1.0, 0.0
        n_grad[n] = ns
        for k in range(o, o + ns):
            alpha = 1.0 - np.exp(-sg[k] * dl[k, 0])
            w = alpha * T
            image[idx] += w * rg[k]
            t += dl[k, 1]
            depth[idx] += w * t
            ws[idx] += w
            T *= 1.0 - alpha
            if T < THRESH:
                n_grad[n] = k - o
                break
    return ws, depth, image, n_grad, live


def _ref_train_backward(tb, ref, g_ws, g_im):
    """The reference's rule in float64: its gradient formula for the steps before the stopping step, nothing from it on.  `written`
    marks the rows that receive a gradient."""
    N, M, rays = tb["N"], tb["M"], tb["rays"]
    sg, rg, dl = tb["sigmas"].astype(np.float64), tb["rgbs"].astype(np.float64), tb["deltas"].astype(np.float64)
    ws_f, _, im_f, n_grad, live = ref
    gs, gr = np.zeros(M), np.zeros((M, 3))
    written = np.zeros(M, bool)
    for n in range(N):
        idx, o, ns = (int(v) for v in rays[n])
        if not live[n]:
            continue
        T, acc = 1.0, np.zeros(3)
        for k in range(o, o + int(n_grad[n])):
            alpha = 1.0 - np.exp(-sg[k] * dl[k, 0])
            w = alpha * T
            acc += w * rg[k]
            T *= 1.0 - alpha
            gr[k] = g_im[idx] * w
            gs[k] = dl[k, 0] * (np.dot(g_im[idx], T * rg[k] - (im_f[idx] - acc)) + g_ws[idx] * (1.0 - ws_f[idx]))
            written[k] = True
    return gs, gr, written


def _autograd_train_backward(tb, g_ws, g_im):
    """d(sum(g_ws * ws) + sum(g_im * image)) / d(sigmas, rgbs) by torch.autograd in float64 over a plain loop of the forward, for the
    rays that never stop.  Independent of the gradient formula."""
    rays, specs = tb["rays"], tb["specs"]
    sg = torch.tensor(tb["sigmas"].astype(np.float64), requires_grad=True)
    rg = torch.tensor(tb["rgbs"].astype(np.float64), requires_grad=True)
    dl = torch.tensor(tb["deltas"].astype(np.float64))
    gw, gi = torch.tensor(g_ws.astype(np.float64)), torch.tensor(g_im.astype(np.float64))
    loss = torch.zeros((), dtype=torch.float64)
    rows = np.zeros(tb["M"], bool)
    for n, (ns, stop) in enumerate(specs[:-1]):
        if stop is not None or ns == 0:
            continue
        idx, o = int(rays[n, 0]), int(rays[n, 1])
        T, ws, im = torch.ones((), dtype=torch.float64), torch.zeros((), dtype=torch.float64), torch.zeros(3, dtype=torch.float64)
        for k in range(o, o + ns):
            alpha = 1.0 - torch.exp(-sg[k] * dl[k, 0])
            w = alpha * T
            im = im + w * rg[k]
            ws = ws + w
            T = T * (1.0 - alpha)
        loss = loss + gw[idx] * ws + (gi[idx] * im).sum()
        rows[o:o + ns] = True
    loss.backward()
    return sg.grad.numpy(), rg.grad.numpy(), rows


def _per_ray_err(tb, got, ref, rows):
    """largest over the rays of max|got - ref| / max|ref| within the ray's rows selected by `rows` (the `final - accumulated`
    subtraction of the sigma gradient cancels near the end of long rays, so single elements have no relative accuracy)"""
    worst = 0.0
    for n in range(tb["N"]):
        o, ns = int(tb["rays"][n, 1]), int(tb["rays"][n, 2])
        sel = np.flatnonzero(rows[o:o + ns]) + o
        if len(sel):
            scale = np.abs(ref[sel]).max()
            assert scale > 0
            worst = max(worst, float(np.abs(np.asarray(got, np.float64)[sel] - ref[sel]).max() / scale))
    return worst


@functools.lru_cache(maxsize=None)
def _train_table(lead):
    """The table, its float64 references and the oracle's measured errors: computed once per lead, shared, never modified."""
    tb = build_ray_table(_train_cases(), lead=lead, seed=100 + lead)
    N, M = tb["N"], tb["M"]
    rng = np.random.default_rng(7 + lead)
    g_ws, g_dp, g_im = (rng.normal(size=N).astype(np.float32), rng.normal(size=N).astype(np.float32),
                        rng.normal(size=(N, 3)).astype(np.float32))
    ref = _ref_train_forward(tb)
    ws, depth, image, n_grad, live = ref
    stops = [s for _, s in tb["specs"][:-1]]
    for n, (ns, stop) in enumerate(tb["specs"][:-1]):       # the table does what its specification says
        assert live[n] == (ns > 0) and n_grad[n] == (ns if stop is None else stop)
    assert not live[-1]
    o_ws, o_dp, o_im = np.full(N, SENTINEL, np.float32), np.full(N, SENTINEL, np.float32), np.full((N, 3), SENTINEL, np.float32)
    O.composite_rays_train_forward(tb["sigmas"], tb["rgbs"], tb["deltas"], tb["rays"], M, N, o_ws, o_dp, o_im)
    sel = tb["rays"][live, 0]
    fwd_err = {"weights_sum": _errs(o_ws[sel], ws[sel]), "depth": _errs(o_dp[sel], depth[sel]), "image": _errs(o_im[sel], image[sel])}
    gs, gr, written = _ref_train_backward(tb, ref, g_ws.astype(np.float64), g_im.astype(np.float64))
    o_gs, o_gr = np.full(M, SENTINEL, np.float32), np.full((M, 3), SENTINEL, np.float32)
    O.composite_rays_train_backward(g_ws, g_im, tb["sigmas"], tb["rgbs"], tb["deltas"], tb["rays"], o_ws, o_im, M, N, o_gs, o_gr)
    assert np.all(o_gs[~written] == SENTINEL) and np.all(o_gr[~written] == SENTINEL)        # the oracle follows the same stop rule
    a_gs, a_gr, a_rows = _autograd_train_backward(tb, g_ws, g_im)
    # the restated formula IS the derivative where no step stops the ray (float64 against float64)
    assert np.abs(a_gs[a_rows] - gs[a_rows]).max() <= 1e-12 * np.abs(gs[a_rows]).max()
    assert np.abs(a_gr[a_rows] - gr[a_rows]).max() <= 1e-12 * np.abs(gr[a_rows]).max()
    assert not np.any(a_gs[~a_rows]) and not np.any(a_gr[~a_rows])
    bwd_err = {
        "grad_sigmas": _errs(o_gs[written], gs[written]),
        "grad_rgbs": _errs(o_gr[written], gr[written]),
        "grad_sigmas/autograd": (_errs(o_gs[a_rows], a_gs[a_rows])[0], _per_ray_err(tb, o_gs, a_gs, a_rows)),
        "grad_rgbs/autograd": (_errs(o_gr[a_rows], a_gr[a_rows])[0], _per_ray_err(tb, o_gr, a_gr, a_rows)),
    }
    out = dict(tb=tb, g_ws=g_ws, g_dp=g_dp, g_im=g_im, ref=ref, stops=stops, fwd_err=fwd_err, gs=gs, gr=gr, written=written,
               a_gs=a_gs, a_gr=a_gr, a_rows=a_rows, bwd_err=bwd_err)
    for v in list(out.values()) + list(tb.values()) + list(ref):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _raw_train_forward(tb, dev, device):
    from nerfsafetyvalidation_amd import _lib
    N, M = tb["N"], tb["M"]
    ws = torch.full((N,), SENTINEL, dtype=torch.float32, device=device)
    depth = torch.full((N,), SENTINEL, dtype=torch.float32, device=device)
    image = torch.full((N, 3), SENTINEL, dtype=torch.float32, device=device)
    _lib.check(_lib.lib().ngp_composite_rays_train_forward(_lib.ptr(dev["sigmas"]), _lib.ptr(dev["rgbs"]), _lib.ptr(dev["deltas"]),
                                                           _lib.ptr(dev["rays"]), M, N, _lib.ptr(ws), _lib.ptr(depth), _lib.ptr(image),
                                                           _lib.stream()), "composite_rays_train_forward")
    torch.cuda.synchronize()
    return ws, depth, image


def _device_table(tb, device):
    return {k: _t(tb[k], device) for k in ("sigmas", "rgbs", "deltas", "rays")}


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. composite_rays_train forward
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_composite_train_forward(device, lead):
    """Every (num_steps, stop_at) of _train_cases at slab offsets shifted by `lead`, through the operator and through the raw entry
    point with outputs prefilled with 7.0: all five values of every ray are written, zero-step rays and the dropped ray are exactly
    0, every other ray equals the float64 recurrence within 4x the float32 oracle's own error on this table."""
    from nerfsafetyvalidation_amd import raymarching
    c = _train_table(lead)
    tb = c["tb"]
    ws, depth, image, _, live = c["ref"]
    dev = _device_table(tb, device)
    via_op = [x.cpu().numpy() for x in raymarching.composite_rays_train(dev["sigmas"], dev["rgbs"], dev["deltas"], dev["rays"])]
    via_raw = [x.cpu().numpy() for x in _raw_train_forward(tb, dev, device)]
    sel, dead = tb["rays"][live, 0], tb["rays"][~live, 0]
    assert len(dead) >= 3       # two zero-step rays and the dropped one
    for how, (k_ws, k_dp, k_im) in (("operator", via_op), ("raw", via_raw)):
        for name, k in (("weights_sum", k_ws), ("depth", k_dp), ("image", k_im)):
            assert not np.any(k == SENTINEL), f"{how} {name}: a ray was left unwritten"
            assert np.all(k[dead].view(np.uint32) == 0), f"{how} {name}: skipped rays are not exactly +0"
        # measured on MI355X over the four leads (largest abs / rel error against float64):
        #   weights_sum  oracle 5.3e-7..7.5e-7 / 5.3e-7..7.5e-7   kernel 4.1e-7..7.5e-7 / 4.1e-7..7.5e-7   (<= 1.00 x the oracle's)
        #   depth        oracle 7.0e-7..1.1e-6 / 3.9e-7..7.5e-7   kernel 7.1e-7..1.2e-6 / 5.1e-7..6.7e-7   (<= 1.68 x)
        #   image        oracle 2.9e-7..3.4e-7 / 5.2e-7..6.8e-7   kernel 2.7e-7..4.0e-7 / 5.7e-7..7.9e-7   (<= 1.41 x)
        _within(f"lead {lead} {how} weights_sum", _errs(k_ws[sel], ws[sel]), c["fwd_err"]["weights_sum"])
        _within(f"lead {lead} {how} depth", _errs(k_dp[sel], depth[sel]), c["fwd_err"]["depth"])
        _within(f"lead {lead} {how} image", _errs(k_im[sel], image[sel]), c["fwd_err"]["image"])
    for a, b in zip(via_op, via_raw):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. composite_rays_train backward
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_composite_train_backward(device, lead):
    """(a) rays that never stop: the kernel's gradient against float64 autograd of the forward, relative to the ray's largest
    gradient; a non-zero grad_depth changes nothing.  (b) rays that stop: the formula before the stopping step; at and after it the
    operator returns exactly 0.0 and the raw entry point leaves the 7.0 it was handed, as it does in the rows of the dropped ray and
    the padding."""
    from nerfsafetyvalidation_amd import _lib, raymarching
    c = _train_table(lead)
    tb, written, a_rows = c["tb"], c["written"], c["a_rows"]
    N, M = tb["N"], tb["M"]
    dev = _device_table(tb, device)
    g_ws, g_dp, g_im = _t(c["g_ws"], device), _t(c["g_dp"], device), _t(c["g_im"], device)
    assert written.sum() > 1000 and (~written).sum() > 1000 and (~written)[:tb["lead"]].all()

    ts, tr = dev["sigmas"].clone().requires_grad_(True), dev["rgbs"].clone().requires_grad_(True)
    k_ws, k_dp, k_im = raymarching.composite_rays_train(ts, tr, dev["deltas"], dev["rays"])
    loss = (k_ws * g_ws).sum() + (k_im * g_im).sum()
    op_gs, op_gr = torch.autograd.grad(loss, (ts, tr), retain_graph=True)
    dp_gs, dp_gr = torch.autograd.grad(loss + (k_dp * g_dp).sum(), (ts, tr))
    assert torch.equal(op_gs.view(torch.int32), dp_gs.view(torch.int32)) and torch.equal(op_gr.view(torch.int32), dp_gr.view(torch.int32))
    op_gs, op_gr = op_gs.cpu().numpy(), op_gr.cpu().numpy()
    assert op_gs.shape == (M,) and op_gr.shape == (M, 3)
    # the pattern, exactly: no gradient at or after the stopping step, in skipped rays or in padding
    assert np.all(op_gs[~written].view(np.uint32) == 0) and np.all(op_gr[~written].view(np.uint32) == 0)

    raw_gs = torch.full((M,), SENTINEL, dtype=torch.float32, device=device)
    raw_gr = torch.full((M, 3), SENTINEL, dtype=torch.float32, device=device)
    k_ws, k_im = k_ws.detach().contiguous(), k_im.detach().contiguous()
    _lib.check(_lib.lib().ngp_composite_rays_train_backward(_lib.ptr(g_ws), _lib.ptr(g_im), _lib.ptr(dev["sigmas"]), _lib.ptr(dev["rgbs"]),
                                                            _lib.ptr(dev["deltas"]), _lib.ptr(dev["rays"]), _lib.ptr(k_ws), _lib.ptr(k_im),
                                                            M, N, _lib.ptr(raw_gs), _lib.ptr(raw_gr), _lib.stream()),
               "composite_rays_train_backward")
    torch.cuda.synchronize()
    raw_gs, raw_gr = raw_gs.cpu().numpy(), raw_gr.cpu().numpy()
    assert np.all(raw_gs[~written] == SENTINEL) and np.all(raw_gr[~written] == SENTINEL), "a row without a gradient was written"
    assert np.array_equal(raw_gs[written].view(np.uint32), op_gs[written].view(np.uint32))
    assert np.array_equal(raw_gr[written].view(np.uint32), op_gr[written].view(np.uint32))

    # measured on MI355X over the four leads (largest abs / rel error against float64; for (a) rel is per ray, against its largest gradient):
    #   (b) grad_sigmas  oracle 1.7e-8..2.6e-8 / 3.4e-3..9.3e-3   kernel 1.4e-8..2.5e-8 / 4.0e-3..8.9e-3   (<= 1.28 x the oracle's; the
    #                    elementwise relative error is that of the most cancelled `final - accumulated` element)
    #   (b) grad_rgbs    oracle 9.3e-8..1.9e-7 / 5.7e-6..6.1e-6   kernel 9.0e-8..1.9e-7 / 5.6e-6..6.0e-6   (<= 1.00 x)
    #   (a) grad_sigmas  oracle 7.4e-9..2.1e-8 / 1.3e-6..1.6e-5   kernel 5.9e-9..2.0e-8 / 1.6e-6..1.6e-5   (<= 1.21 x)
    #   (a) grad_rgbs    oracle 5.3e-8..9.2e-8 / 7.8e-7..1.2e-6   kernel 5.5e-8..9.2e-8 / 7.8e-7..1.2e-6   (<= 1.38 x)
    e = c["bwd_err"]
    _within(f"lead {lead} (b) grad_sigmas", _errs(op_gs[written], c["gs"][written]), e["grad_sigmas"])
    _within(f"lead {lead} (b) grad_rgbs", _errs(op_gr[written], c["gr"][written]), e["grad_rgbs"])
    _within(f"lead {lead} (a) grad_sigmas [rel = per ray]", (_errs(op_gs[a_rows], c["a_gs"][a_rows])[0], _per_ray_err(tb, op_gs, c["a_gs"], a_rows)),
            e["grad_sigmas/autograd"])
    _within(f"lead {lead} (a) grad_rgbs [rel = per ray]", (_errs(op_gr[a_rows], c["a_gr"][a_rows])[0], _per_ray_err(tb, op_gr, c["a_gr"], a_rows)),
            e["grad_rgbs/autograd"])


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. composite_rays (inference, in place)
# ---------------------------------------------------------------------------------------------------------------------------------
INFER_N = 400
INFER_STEPS = (1, 2, 3, 4, 8)
INFER_ALIVE = (1, 63, 64, 65, 300)
_STATE = ("rays_t", "ws", "depth", "image")


def _ref_composite_rays(n_alive, n_step, alive, state, sig, rgb, deltas, trace=None):
    """float64 restatement of one launch: a deltas[.,0] == 0 marker ends the ray without a contribution; a step that starts with
    T = 1 - weights_sum < 1e-4 contributes and ends it.  Ended rays get -1 and keep rays_t."""
    alive = alive.copy()
    st = {k: v.astype(np.float64) for k, v in state.items()}
    finished = np.zeros(n_alive, bool)
    for n in range(n_alive):
        i = int(alive[n])
        t, ws, d, c = st["rays_t"][i], st["ws"][i], st["depth"][i], st["image"][i].copy()
        step = 0
        while step < n_step:
            k = n * n_step + step
            if deltas[k, 0] == 0:
                break
            alpha = 1.0 - np.exp(-np.float64(sig[k]) * np.float64(deltas[k, 0]))
            T = 1.0 - ws
            if trace is not None:
                trace.append(T)
            w = alpha * T
            ws += w
            t += np.float64(deltas[k, 1])
            d += w * t
            c += w * rgb[k].astype(np.float64)
            if T < THRESH:
                break
            step += 1
        if step < n_step:
            alive[n] = -1
        else:
            st["rays_t"][i] = t
            finished[n] = True
            if trace is not None:
                trace.append(1.0 - ws)       # what the next launch would compare first
        st["ws"][i], st["depth"][i], st["image"][i] = ws, d, c
    return alive, st, finished


def build_launch(n_step, n_alive, seed):
    """One composite_rays launch over INFER_N rays: an unsorted subset alive, n_step sample slots each (padded as march_rays pads:
    to the next multiple of 128, zero deltas), and per slot one of: finishes all steps; finishes with T taken below 1e-4 by its
    last step; a deltas == 0 marker at position p; a T < 1e-4 exit at position p (p = 0: the incoming weights_sum is already above
    1 - 1e-4), for every p in 0..n_step-1."""
    rng = np.random.default_rng(seed)
    N = INFER_N
    alive = rng.permutation(N)[:n_alive].astype(np.int32)
    assert n_alive < 3 or np.any(np.diff(alive) < 0)
    M = n_alive * n_step
    M += 128 - M % 128
    state = dict(rays_t=rng.uniform(0.2, 3, N).astype(np.float32), ws=rng.uniform(0, 0.9, N).astype(np.float32),
                 depth=rng.uniform(0, 1, N).astype(np.float32), image=rng.uniform(0, 1, (N, 3)).astype(np.float32))
    rest = np.setdiff1d(np.arange(N), alive)
    # rays that are not alive: finished ones (weights_sum above 1 - 1e-4) and bit patterns that arithmetic would not preserve
    state["ws"][rest[0::5]] = (1 - THRESH * rng.uniform(0.01, 0.9, len(rest[0::5]))).astype(np.float32)
    state["depth"][rest[1::7]] = np.float32(-0.0)
    state["image"][rest[2::7], 1] = np.uint32(0x7FC12345).view(np.float32)      # a NaN with a payload
    state["rays_t"][rest[3::7]] = np.float32(np.inf)
    sig = rng.uniform(5, 200, M).astype(np.float32)
    rgb = rng.uniform(0, 1, (M, 3)).astype(np.float32)
    deltas = np.stack([rng.uniform(0.003, 0.03, M), rng.uniform(0.003, 0.05, M)], axis=1).astype(np.float32)
    deltas[n_alive * n_step:] = 0
    plans = [("full", 0), ("cross_last", 0)] + [("marker", p) for p in range(n_step)] + [("texit", p) for p in range(n_step)]
    plan_of = []
    for n in range(n_alive):
        kind, p = plans[(n + seed) % len(plans)]
        plan_of.append((kind, p))
        i, o = int(alive[n]), n * n_step
        dt = deltas[o:o + n_step, 0].astype(np.float64)
        cross = {"full": None, "marker": None, "cross_last": n_step - 1, "texit": p - 1}[kind]     # the step that takes T below 1e-4
        scale = 1.0
        for _ in range(50):
            if cross == -1:
                state["ws"][i] = np.float32(1 - THRESH * rng.uniform(0.1, 0.5))
            tau = rng.uniform(0.05, 0.6, n_step) * scale
            sig[o:o + n_step] = (tau / dt).astype(np.float32)
            if cross is not None and cross >= 0:
                T_before = (1.0 - np.float64(state["ws"][i])) * np.prod(np.exp(-sig[o:o + cross].astype(np.float64) * dt[:cross]))
                sig[o + cross] = np.float32(np.log(T_before / (THRESH * rng.uniform(0.1, 0.5))) / dt[cross])
            if kind == "marker":
                deltas[o + p] = 0
            trace = []
            got, _, fin = _ref_composite_rays(1, n_step, alive[n:n + 1], state, sig[o:o + n_step], rgb[o:o + n_step], deltas[o:o + n_step],
                                              trace)
            if kind == "marker":
                ok = got[0] == -1 and len(trace) == p
            elif kind == "texit":
                ok = got[0] == -1 and len(trace) == p + 1 and trace[-1] < THRESH
            else:
                ok = bool(fin[0]) and (trace[-1] < THRESH) == (kind == "cross_last")
            ok = ok and _clear_of_threshold(trace)
            if ok:
                break
            scale *= 0.9
        assert ok, f"slot {n} ({kind}, {p}) cannot be kept clear of the threshold"
    return dict(n_step=n_step, n_alive=n_alive, alive=alive, state=state, sig=sig, rgb=rgb, deltas=deltas, plans=plan_of, M=M)


@functools.lru_cache(maxsize=None)
def _launch(n_step, n_alive):
    L = build_launch(n_step, n_alive, seed=1000 + 17 * n_step + n_alive)
    trace = []
    L["want_alive"], L["want"], L["finished"] = _ref_composite_rays(n_alive, n_step, L["alive"], L["state"], L["sig"], L["rgb"], L["deltas"],
                                                                    trace)
    assert _clear_of_threshold(trace)
    o_alive, o = L["alive"].copy(), {k: v.copy() for k, v in L["state"].items()}
    O.composite_rays(n_alive, n_step, o_alive, o["rays_t"], L["sig"], L["rgb"], L["deltas"], o["ws"], o["depth"], o["image"])
    assert np.array_equal(o_alive, L["want_alive"])
    L["oracle"] = o
    for v in list(L.values()) + list(L["state"].values()) + list(L["want"].values()) + list(o.values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return L


@functools.lru_cache(maxsize=None)
def _inference_oracle_err():
    """The float32 oracle's largest (absolute, relative) error against float64 per state array, over all 25 launches (a launch of one
    ray and one step has too few roundings to measure anything on its own)."""
    worst = {k: (0.0, 0.0) for k in _STATE}
    kinds = set()
    for n_step in INFER_STEPS:
        for n_alive in INFER_ALIVE:
            L = _launch(n_step, n_alive)
            kinds |= set(L["plans"])
            for k in _STATE:
                sel = L["alive"] if k != "rays_t" else L["alive"][L["finished"]]
                e = _errs(L["oracle"][k][sel], L["want"][k][sel])
                worst[k] = (max(worst[k][0], e[0]), max(worst[k][1], e[1]))
    # every exit at every position of the longest launch, both ways of finishing
    assert kinds >= {("full", 0), ("cross_last", 0)} | {(kind, p) for kind in ("marker", "texit") for p in range(max(INFER_STEPS))}
    return worst


@pytest.mark.parametrize("n_alive", INFER_ALIVE)
@pytest.mark.parametrize("n_step", INFER_STEPS)
def test_composite_rays_exits_and_untouched_state(device, n_step, n_alive):
    """rays_alive equals the float64 reference's exactly, no ray excused; rays_t moves only for rays that took all n_step steps; rays
    outside rays_alive keep every bit of their state; the sums are within 4x the float32 oracle's error."""
    from nerfsafetyvalidation_amd import raymarching
    L = _launch(n_step, n_alive)
    tol = _inference_oracle_err()
    N = INFER_N
    g_alive = _t(L["alive"], device)
    g = {k: _t(v, device) for k, v in L["state"].items()}
    ret = raymarching.composite_rays(n_alive, n_step, g_alive, g["rays_t"], _t(L["sig"], device), _t(L["rgb"], device),
                                     _t(L["deltas"], device), g["ws"], g["depth"], g["image"])
    assert ret == tuple()
    got_alive = g_alive.cpu().numpy()
    got = {k: v.cpu().numpy() for k, v in g.items()}
    assert np.array_equal(got_alive, L["want_alive"])
    if n_alive >= 63:
        assert (got_alive == -1).sum() > 10 and (got_alive >= 0).sum() >= 3
    outside = np.setdiff1d(np.arange(N), L["alive"])
    for k in _STATE:
        assert np.array_equal(got[k][outside].view(np.uint32), L["state"][k][outside].view(np.uint32)), f"{k} of a ray not alive changed"
    ended = L["alive"][~L["finished"]]
    assert np.array_equal(got["rays_t"][ended].view(np.uint32), L["state"]["rays_t"][ended].view(np.uint32))
    for k in _STATE:
        sel = L["alive"] if k != "rays_t" else L["alive"][L["finished"]]
        # measured on MI355X (abs / rel; the oracle's over all 25 launches, the kernel's largest in any one launch):
        #   rays_t  oracle 4.1e-7 / 1.8e-7   kernel 4.1e-7 / 1.8e-7 (the same float32 additions)
        #   ws      oracle 1.1e-7 / 1.8e-7   kernel 1.1e-7 / 1.8e-7
        #   depth   oracle 4.4e-7 / 5.3e-7   kernel 3.9e-7 / 5.3e-7
        #   image   oracle 2.7e-7 / 3.3e-7   kernel 2.7e-7 / 3.3e-7
        _within(f"n_step {n_step} n_alive {n_alive} {k}", _errs(got[k][sel], L["want"][k][sel]), tol[k])


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. ngp_uq_stats
# ---------------------------------------------------------------------------------------------------------------------------------
def _uq_constants():
    import nerfsafetyvalidation_amd
    src = open(os.path.join(os.path.dirname(nerfsafetyvalidation_amd.__file__), "csrc", "capi.hip")).read()
    m = re.search(r"constexpr\s+uint32_t\s+kUqBlocks\s*=\s*(\d+)\s*,\s*kUqThreads\s*=\s*(\d+)\s*;", src)
    assert m, "kUqBlocks / kUqThreads not found in capi.hip"
    return int(m.group(1)), int(m.group(2))


def _uq_call(c, d, r, device):
    from nerfsafetyvalidation_amd import _lib
    lib = _lib.lib()
    wbytes = lib.ngp_uq_stats_workspace()
    work = torch.empty(wbytes // 8, dtype=torch.float64, device=device)
    stats = torch.full((8,), SENTINEL, dtype=torch.float64, device=device)
    _lib.check(lib.ngp_uq_stats(_lib.ptr(c), 1 if c.dtype == torch.float16 else 0, _lib.ptr(d), d.numel(), _lib.ptr(r), r.numel(),
                                _lib.ptr(stats), _lib.ptr(work), wbytes, _lib.stream()), "uq_stats")
    return stats.cpu().numpy()


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, "grid+17"])
def test_uq_stats_sums_and_counts(device, n, dtype):
    """The five sums and the two counts against float64 numpy (terms and sums in extended precision), for sample counts around a
    wave and past one pass of the grid (kUqBlocks * kUqThreads + 17), rendered-colour counts m that differ from n, signed d, fp32
    and fp16 colours.  The kernel accumulates in double: per sum, count * 2^-52 * sum|terms|, times 8 for the tree order.  Two
    calls give the same bits."""
    blocks, threads = _uq_constants()
    if n == "grid+17":
        n = blocks * threads + 17
        assert n == 256 * 512 + 17
    rng = np.random.default_rng(n % 1000 + (7 if dtype == np.float16 else 0))
    c = rng.uniform(0, 1, (n, 3)).astype(np.float32).astype(dtype)
    d = (rng.normal(size=n) * 30).astype(np.float32)
    assert n < 2 or (d.min() < 0 < d.max())
    cl, dl_ = c.astype(np.longdouble), d.astype(np.longdouble)
    sc, sc2 = cl.sum(axis=1), (cl * cl).sum(axis=1)
    tc, td = _t(c, device), _t(d, device)
    for m in sorted({0, 5, n, 3 * n + 1}):
        r = rng.uniform(-0.2, 1, m).astype(np.float32)
        terms = {0: sc2 * dl_ * dl_, 1: sc * dl_, 2: r.astype(np.longdouble), 4: dl_, 5: dl_ * dl_}
        tr = _t(r, device)
        stats = _uq_call(tc, td, tr, device)
        assert stats[3] == m and stats[6] == n and stats[7] == 0
        for slot, t in terms.items():
            want = t.sum(dtype=np.longdouble) if len(t) else np.longdouble(0)
            bound = 8 * len(t) * 2.0 ** -52 * float(np.abs(t).sum(dtype=np.longdouble)) if len(t) else 0.0
            err = abs(float(np.longdouble(stats[slot]) - want))
            if m in (0, 3 * n + 1):
                print(f"uq n {n} m {m} {np.dtype(dtype).name} stats[{slot}]: error {err:.3e}, bound {bound:.3e}")
            # measured on MI355X: the largest error is 0.05 x its bound (n = 1, fp16 colours, stats[0]: 1.1e-14 against 2.3e-13);
            # at n = 256 * 512 + 17 the errors are below 1e-5 x their bounds
            assert err <= bound, f"stats[{slot}] n={n} m={m}: {stats[slot]!r} vs {float(want)!r}, error {err:.3e} > {bound:.3e}"
        again = _uq_call(tc, td, tr, device)
        assert np.array_equal(stats.view(np.uint64), again.view(np.uint64))
