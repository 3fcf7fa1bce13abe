"""The frequency encoder's HIP kernels (csrc/freqencoder.hip) against float64, and the networks that use the encoder.

Forward tolerance: every sin / cos element within 4 ulp of 1.0 = 4 * 2^-23 = 4.77e-7 of numpy's float64 sin / cos of the exact argument
ldexp(x, f) -- the OpenCL bound for a full-precision float sine.  The kernel's arithmetic evaluated on the host measures 9.3e-8
(DESIGN.md "Frequency encoder"); the reference's phase-shifted fast sine is 6.4e-7 off at degree 4 and 4.8e-4 at degree 16, so the bound
tells the two apart.  Backward tolerance per element: 2e-6 * M, M = |g_x| + sum_f 2^f (|g_sin| + |g_cos|): 4 ulp on each sin / cos
(4.8e-7), two roundings per product and an fmaf (1.8e-7), and a float32 sum of at most 2 * 16 + 1 terms, each partial sum below M
(33 * 6e-8 = 2e-6 in the worst case of every rounding going one way; the three parts do not reach their worst together).
Each test prints the worst error it saw."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FWD_TOL = 4 * 2.0 ** -23
BWD_TOL = 2e-6
PI_2, PI = np.float32(np.pi / 2), np.float32(np.pi)
UP, DOWN = np.float32(np.inf), np.float32(-np.inf)
SPECIAL = np.array([0.0, -0.0, 1, -1, 2, -2, 2.0 ** -20, -2.0 ** -20, 1e-38, -1e-38,
                    np.nextafter(PI_2, DOWN), PI_2, np.nextafter(PI_2, UP), np.nextafter(PI, DOWN), PI, np.nextafter(PI, UP)], dtype=np.float32)
BATCHES = (1, 63, 64, 65, 257, 4099)


def _inputs(B, D, seed):
    """uniform in [-2, 2) with the fixed values written over the first entries (from a place that moves with the shape, so that the
    one-row shapes see different ones)"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-2, 2, size=B * D).astype(np.float32)
    x[x >= 2] = np.float32(-2)                                   # (the rounding to float32 may reach 2)
    n = min(len(SPECIAL), B * D)
    x[:n] = np.roll(SPECIAL, seed)[:n]
    return x.reshape(B, D)


def _ref_forward(x, deg):
    """float64 [B, C] in the reference's column order: [x | sin(2^0 x) | cos(2^0 x) | sin(2^1 x) | ...], D columns each; the argument
    is the float32 ldexp(x, f) -- exact, unless it overflows to inf, whose sine is nan"""
    cols = [x.astype(np.float64)]
    with np.errstate(invalid="ignore", over="ignore"):
        for f in range(deg):
            a = np.ldexp(x, f).astype(np.float64)
            cols += [np.sin(a), np.cos(a)]
    return np.concatenate(cols, axis=1)


def _ref_backward(x, g, deg):
    """float64 grad_inputs and the magnitude M of the tolerance"""
    D = x.shape[1]
    g64 = g.astype(np.float64)
    out, M = g64[:, :D].copy(), np.abs(g64[:, :D])
    with np.errstate(invalid="ignore", over="ignore"):
        for f in range(deg):
            gs, gc = g64[:, D + 2 * f * D:D + (2 * f + 1) * D], g64[:, D + (2 * f + 1) * D:D + (2 * f + 2) * D]
            a = np.ldexp(x, f).astype(np.float64)
            out += 2.0 ** f * (gs * np.cos(a) - gc * np.sin(a))
            M += 2.0 ** f * (np.abs(gs) + np.abs(gc))
    return out, M


def _run(x, g, deg, device):
    """the operator on numpy inputs -> (outputs, grad_inputs) as numpy"""
    from nerfsafetyvalidation_amd.freqencoder import freq_encode
    B, D = x.shape
    xt = torch.from_numpy(x).to(device).requires_grad_(True)
    out = freq_encode(xt, deg, D + 2 * D * deg)
    out.backward(torch.from_numpy(g).to(device))
    return out.detach().cpu().numpy(), xt.grad.cpu().numpy()


def _check(x, deg, device, seed):
    """forward, backward and a second run of both on inputs x; nan (the sine of a non-finite argument) must sit where float64 has it"""
    B, D = x.shape
    C = D + 2 * D * deg
    g = np.random.default_rng(seed + 1).standard_normal((B, C)).astype(np.float32)
    out, gin = _run(x, g, deg, device)
    assert out.shape == (B, C) and out.dtype == np.float32 and gin.shape == (B, D) and gin.dtype == np.float32
    assert np.array_equal(out[:, :D].view(np.int32), x.view(np.int32))             # bit copies: -0.0 and the subnormals included
    want = _ref_forward(x, deg)
    assert np.array_equal(np.isnan(out), np.isnan(want))
    ok = np.isfinite(want)                                                          # (an infinite x is in the bit copies above)
    err_f = np.abs(out[ok].astype(np.float64) - want[ok]).max()
    want_g, M = _ref_backward(x, g, deg)
    ok = ~np.isnan(want_g)
    assert np.array_equal(np.isnan(gin), ~ok)
    err_b = (np.abs(gin[ok].astype(np.float64) - want_g[ok]) / M[ok]).max()
    assert err_f <= FWD_TOL, (B, D, deg, err_f)
    assert err_b <= BWD_TOL, (B, D, deg, err_b)
    out2, gin2 = _run(x, g, deg, device)                                            # the same bits on a second run
    same = lambda a, b: np.array_equal(a.view(np.int32)[~np.isnan(a)], b.view(np.int32)[~np.isnan(a)]) and np.array_equal(np.isnan(a), np.isnan(b))
    assert same(out, out2) and same(gin, gin2)
    return err_f, err_b, out


@pytest.mark.parametrize("deg", [0, 1, 4, 6, 10, 16])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_operator_matches_float64(device, D, deg):
    worst_f = worst_b = 0.0
    for B in BATCHES:
        x = _inputs(B, D, seed=B + 7 * D + 31 * deg)
        err_f, err_b, _ = _check(x, deg, device, seed=B)
        worst_f, worst_b = max(worst_f, err_f), max(worst_b, err_b)
    print(f"freq_encode D={D} deg={deg}: forward {worst_f:.2e} (bound {FWD_TOL:.2e}), backward / M {worst_b:.2e} (bound {BWD_TOL:.0e})")


def test_every_fixed_value_at_the_highest_degree(device):
    """the shapes above put the fixed values in front of random ones; here they are the whole input, every one in every column"""
    for D in (1, 2, 3):
        x = np.stack([np.roll(SPECIAL, k) for k in range(D)], axis=1).copy()
        err_f, err_b, out = _check(x, 16, device, seed=D)
        assert out[0, D] == 0 and out[0, 2 * D] == 1                                # sin 0, cos 0
        print(f"freq_encode fixed values D={D} deg=16: forward {err_f:.2e}, backward / M {err_b:.2e}")


def test_large_and_non_finite_inputs_take_the_library_path(device):
    """|x| > 1024 leaves the shared range reduction for the device library's sincosf of the exact argument (its own test: bounded random
    inputs never get there); inf and nan give nan in their sin / cos columns and keep their bits in the first D"""
    rng = np.random.default_rng(5)
    B, D, deg = 300, 3, 6
    x = (np.exp(rng.uniform(np.log(1024.0), np.log(1e6), size=(B, D))) * rng.choice([-1.0, 1.0], size=(B, D))).astype(np.float32)
    x[0] = [1024.0, np.nextafter(np.float32(1024), UP), -np.nextafter(np.float32(1024), UP)]       # the last value of the fast path, the first of the other
    x[1, 1], x[2, 0], x[3, 2] = np.inf, -np.inf, np.nan
    x[4] = [1e30, -3e38, 1e-3]                                                                    # 2^f x overflows from f = 1 on in one column
    err_f, err_b, out = _check(x, deg, device, seed=9)
    print(f"freq_encode |x| in [1024, 1e6]: forward {err_f:.2e} (bound {FWD_TOL:.2e}), backward / M {err_b:.2e}")
    bad = np.isnan(out)
    assert bad[1, 1::D].sum() == 2 * deg and bad[2, 0::D].sum() == 2 * deg and bad[3, 2::D].sum() == 2 * deg + 1       # (inf, -inf: x stays; nan: x too)
    assert bad[4, 1::D].sum() == 2 * (deg - 1) and bad.sum() == 3 * 2 * deg + 1 + 2 * (deg - 1)


@pytest.mark.parametrize("D", [77, 155, 156])
def test_rows_at_and_past_the_staging_buffer(device, D):
    """C = 33 D: 2541 words go two rows to a workgroup's 5120-word staging buffer, 5115 one row, 5148 do not fit (rows written
    straight to memory)"""
    x = _inputs(3, D, seed=D)
    err_f, err_b, _ = _check(x, 16, device, seed=D)
    print(f"freq_encode D={D} deg=16 (C={33 * D}): forward {err_f:.2e}, backward / M {err_b:.2e}")


def test_no_backward_without_an_input_gradient(device, monkeypatch):
    from nerfsafetyvalidation_amd import _lib
    from nerfsafetyvalidation_amd.freqencoder import FreqEncoder
    lib = _lib.lib()
    real, calls = lib.ngp_freq_encode_backward, []
    monkeypatch.setattr(lib, "ngp_freq_encode_backward", lambda *a: calls.append(1) or real(*a))
    enc = FreqEncoder(3, 4)
    x = torch.rand(65, 3, device=device)
    w = torch.ones(27, device=device, requires_grad=True)
    assert not enc(x).requires_grad
    (enc(x) * w).sum().backward()
    assert calls == [] and x.grad is None and w.grad is not None
    x.requires_grad_(True)
    (enc(x) * w).sum().backward()
    assert calls == [1] and x.grad.shape == (65, 3)


def test_shapes_strides_autocast_and_empty(device):
    from nerfsafetyvalidation_amd.freqencoder import FreqEncoder
    enc = FreqEncoder(3, 5)
    g = torch.Generator().manual_seed(3)
    wide = (torch.rand(5, 7, 6, generator=g) * 4 - 2).to(device)
    x = wide[..., ::2]                                                              # [5, 7, 3], not contiguous
    assert not x.is_contiguous()
    out = enc(x, bound=2, size=3)                                                   # both ignored: no normalisation
    flat = enc(x.reshape(-1, 3).contiguous())
    assert out.shape == (5, 7, 33) and torch.equal(out.reshape(-1, 33), flat)
    assert torch.equal(out[..., :3], x)
    want = _ref_forward(x.reshape(-1, 3).cpu().numpy(), 5)
    assert np.abs(flat.cpu().numpy() - want).max() <= FWD_TOL
    xg = x.detach().clone().requires_grad_(True)                                    # gradient back through the reshape of a strided view
    base = wide.detach().clone().requires_grad_(True)
    enc(base[..., ::2]).sum().backward()
    enc(xg).sum().backward()
    assert torch.equal(base.grad[..., ::2], xg.grad) and (base.grad[..., 1::2] == 0).all()
    half = x.half()
    with torch.autocast("cuda", dtype=torch.float16):
        o16 = enc(half)
    assert o16.dtype == torch.float32 and torch.equal(o16, enc(half.float()))
    e = torch.empty(0, 3, device=device, requires_grad=True)
    o = enc(e)
    assert o.shape == (0, 33) and o.dtype == torch.float32
    o.sum().backward()
    assert e.grad.shape == (0, 3)
    assert enc(torch.empty(4, 0, 3, device=device)).shape == (4, 0, 33)


def test_element_index_past_32_bits(device):
    """B * C > 2^32 (the reference's uint32 element index wraps there): rows on both sides of the 2^32-th element and the last rows,
    forward and backward.  17 GB of outputs, which also serve as the incoming gradient."""
    from nerfsafetyvalidation_amd import _lib
    D, deg, C = 3, 6, 39
    B = 2 ** 32 // C + 4099 + 5000
    need = 4 * B * (C + 2 * D) + (1 << 30)
    if torch.cuda.mem_get_info(device)[0] < need:
        pytest.skip(f"needs {need / 2 ** 30:.0f} GiB of free device memory")
    x = torch.rand(B, D, device=device) * 4 - 2
    out = torch.empty(B, C, device=device)
    lib = _lib.lib()
    _lib.check(lib.ngp_freq_encode_forward(_lib.ptr(x), _lib.ptr(out), B, D, deg, _lib.stream()), "freq_encode_forward")
    gin = torch.empty(B, D, device=device)
    _lib.check(lib.ngp_freq_encode_backward(_lib.ptr(out), _lib.ptr(x), B, D, deg, _lib.ptr(gin), _lib.stream()), "freq_encode_backward")
    edge = 2 ** 32 // C
    worst_f = worst_b = 0.0
    for rows in (slice(0, 300), slice(edge - 300, edge + 300), slice(2 ** 31 // C - 100, 2 ** 31 // C + 100), slice(B - 4099, B)):
        xs, os_, gs = x[rows].cpu().numpy(), out[rows].cpu().numpy(), gin[rows].cpu().numpy()
        assert np.array_equal(os_[:, :D].view(np.int32), xs.view(np.int32))
        worst_f = max(worst_f, np.abs(os_ - _ref_forward(xs, deg)).max())
        want_g, M = _ref_backward(xs, os_, deg)
        worst_b = max(worst_b, (np.abs(gs - want_g) / M).max())
    print(f"freq_encode B={B} (B*C = 2^32 + {B * C - 2 ** 32}): forward {worst_f:.2e}, backward / M {worst_b:.2e}")
    assert worst_f <= FWD_TOL and worst_b <= BWD_TOL


# ---------------------------------------------------------------------------------------------------------------- through the networks
def _compose(x, deg):
    """the encoding as torch operators, in x's precision"""
    return torch.cat([x] + [fn(x * 2.0 ** f) for f in range(deg) for fn in (torch.sin, torch.cos)], dim=-1)


def _mlp(layers, h):
    for i, layer in enumerate(layers):
        h = torch.nn.functional.linear(h, layer.weight)
        if i != len(layers) - 1:
            h = torch.relu(h)
    return h


def _network(device, **kw):
    from nerfsafetyvalidation_amd.nerf.network import NeRFNetwork
    torch.manual_seed(0)
    net = NeRFNetwork(bound=1, density_scale=1, min_near=0.2, density_thresh=0.01, **kw)
    if hasattr(net.encoder, "embeddings"):
        g = torch.Generator().manual_seed(5)
        net.encoder.embeddings.data.copy_(torch.rand(net.encoder.embeddings.shape, generator=g) - 0.5)
    return net.to(device).eval()


def _points(device, n=64):
    g = torch.Generator().manual_seed(11)
    x = (torch.rand(n, 3, generator=g) * 2 - 1).to(device)
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1).to(device)
    return x, d


def _frame(device, side=16):
    """a side x side pinhole frame from (0.1, -0.2, 2.2) looking down -z at the unit box"""
    u = (torch.arange(side, dtype=torch.float32) + 0.5) / side - 0.5
    dirs = torch.stack([u[None, :].expand(side, side), -u[:, None].expand(side, side), -torch.ones(side, side)], dim=-1)
    rays_d = torch.nn.functional.normalize(dirs.reshape(1, -1, 3), dim=-1).to(device)
    rays_o = torch.tensor([0.1, -0.2, 2.2]).expand(1, side * side, 3).contiguous().to(device)
    return rays_o, rays_d


def test_network_with_frequency_encoded_directions(device):
    """forward equals the same layers on the torch-composed encoding; d colour / d direction through the operator's backward equals
    float64 autograd of the composition, (a) for the very gradient the operator received, within the operator's own bound, and (b)
    end to end against the float64 network, where the float32 layers add their own error: at most gamma = (54 + 64 + 64 + 3) 2^-24 =
    1.1e-5 of the gradient's absolute-value propagation through the layers (twice: the forward's error reaches sigmoid')"""
    net = _network(device, encoding_dir="frequency")
    x, d = _points(device)
    with torch.no_grad():
        sigma, rgb = net(x, d)
        geo = _mlp(net.sigma_net, net.encoder(x, bound=net.bound))
        want = torch.sigmoid(_mlp(net.color_net, torch.cat([_compose(d, 6), geo[..., 1:]], dim=-1)))
        assert sigma.shape == (64,) and rgb.shape == (64, 3) and torch.allclose(sigma, torch.exp(geo[..., 0]), rtol=1e-5, atol=0)
    err = (rgb - want).abs().max().item()
    print(f"NeRFNetwork(encoding_dir=frequency) forward vs the torch composition: {err:.2e}")
    assert err <= 1e-5
    assert net.fused_model() is None
    with torch.autocast("cuda", dtype=torch.float16):
        assert net.fused_model() is None

    # the gradient to the directions
    got = {}

    def keep(module, args, output):
        output.retain_grad()
        got["enc"] = output

    hook = net.encoder_dir.register_forward_hook(keep)
    dg = d.clone().requires_grad_(True)
    w = torch.tensor([0.7, -1.1, 0.4], device=device)                              # a colour direction: d (w . rgb) / d d
    (net(x, dg)[1] * w).sum().backward()
    hook.remove()
    g32 = got["enc"].grad
    # (a) float64 autograd of the composition, fed the gradient the operator was handed
    d64 = d.double().requires_grad_(True)
    _compose(d64, 6).backward(g32.double())
    _, M = _ref_backward(d.cpu().numpy(), g32.cpu().numpy(), 6)
    ratio = ((dg.grad.double() - d64.grad).abs().cpu().numpy() / M).max()
    # (b) the whole float64 network
    d64b = d.double().requires_grad_(True)
    e64 = _compose(d64b, 6)
    e64.retain_grad()
    layers = [l.weight.double() for l in net.color_net]
    h1 = torch.cat([e64, geo[..., 1:].double()], dim=-1) @ layers[0].t()
    h2 = torch.relu(h1) @ layers[1].t()
    rgb64 = torch.sigmoid(torch.relu(h2) @ layers[2].t())
    (rgb64 * w.double()).sum().backward()
    with torch.no_grad():                                                          # |gradient| carried back through |weights|
        top = (rgb64 * (1 - rgb64) * w.double()).abs()
        gabs = ((((top @ layers[2].abs()) * (h2 > 0)) @ layers[1].abs()) * (h1 > 0)) @ layers[0].abs()
    _, M64 = _ref_backward(d.cpu().numpy(), e64.grad.cpu().numpy(), 6)
    _, Mabs = _ref_backward(d.cpu().numpy(), gabs[:, :39].cpu().numpy(), 6)
    gamma = (54 + 64 + 64 + 3) * 2.0 ** -24
    bound = BWD_TOL * M64 + 2 * gamma * Mabs
    diff = (dg.grad.double() - d64b.grad).abs().cpu().numpy()
    gmax = d64b.grad.abs().max().item()
    print(f"d colour / d direction: operator part {ratio:.2e} of M (bound {BWD_TOL:.0e}); end to end {diff.max() / gmax:.2e} of max |gradient| "
          f"(bound {bound.max() / gmax:.2e})")
    assert ratio <= BWD_TOL
    assert (diff <= bound).all()


@pytest.mark.parametrize("cuda_ray", [False, True])
def test_render_with_frequency_encoded_directions(device, cuda_ray):
    net = _network(device, encoding_dir="frequency", cuda_ray=cuda_ray)
    rays_o, rays_d = _frame(device)
    kw = dict(staged=True, bg_color=1, perturb=False, num_steps=16, upsample_steps=0, max_steps=32)
    images = []
    with torch.no_grad():
        if cuda_ray:
            net.update_extra_state()
            assert net.density_bitfield.any()
        for fused in (True, False):
            net.fused = fused
            assert net.fused_model() is None
            out = net.render(rays_o, rays_d, **kw)
            assert out["image"].shape == (1, 256, 3) and out["depth"].shape == (1, 256)
            assert torch.isfinite(out["image"]).all() and torch.isfinite(out["depth"]).all()
            images.append((out["image"].clone(), out["depth"].clone()))
    assert torch.equal(images[0][0], images[1][0]) and torch.equal(images[0][1], images[1][1])       # both take the operators
    assert (images[0][0] - 1).abs().max().item() > 1e-3                                              # something was rendered in front of the white backdrop


def test_frequency_encoded_background(device):
    net = _network(device, bg_radius=1, encoding_bg="frequency")
    _, d = _points(device)
    g = torch.Generator().manual_seed(12)
    uv = (torch.rand(64, 2, generator=g) * 2 - 1).to(device)
    with torch.no_grad():
        got = net.background(uv, d)
        want = torch.sigmoid(_mlp(net.bg_net, torch.cat([net.encoder_dir(d), _compose(uv, 6)], dim=-1)))
    err = (got - want).abs().max().item()
    print(f"NeRFNetwork(encoding_bg=frequency) background vs the torch composition: {err:.2e}")
    assert got.shape == (64, 3) and err <= 1e-5
    assert net.fused_model() is None


def test_frequency_encoded_positions(device):
    net = _network(device, encoding="frequency", cuda_ray=True)
    x, _ = _points(device)
    with torch.no_grad():
        got = net.density(x)
        h = _mlp(net.sigma_net, _compose(x, 6))
        err = (got["sigma"] - torch.exp(h[..., 0])).abs().max().item()
        err_geo = (got["geo_feat"] - h[..., 1:]).abs().max().item()
        print(f"NeRFNetwork(encoding=frequency) density vs the torch composition: sigma {err:.2e}, geo_feat {err_geo:.2e}")
        assert got["sigma"].shape == (64,) and got["geo_feat"].shape == (64, 15) and err <= 1e-5 and err_geo <= 1e-5
        assert net.fused_model() is None
        net.update_extra_state()
        assert net.iter_density == 1 and torch.isfinite(net.density_grid).all() and net.mean_density > 0


def test_training_step_under_autocast(device):
    """training mode, occupancy-grid path, fp16 autocast: the encoder stays float32, the colour network's gradients arrive"""
    net = _network(device, encoding_dir="frequency", cuda_ray=True)
    rays_o, rays_d = _frame(device)
    with torch.no_grad():
        net.update_extra_state()
    net.train()
    with torch.autocast("cuda", dtype=torch.float16):
        assert net.encoder_dir(rays_d[0].half()).dtype == torch.float32
        out = net.render(rays_o, rays_d, staged=False, bg_color=1, perturb=True, force_all_rays=True, max_steps=32)
    out["image"].float().square().mean().backward()
    grads = [layer.weight.grad for layer in net.color_net]
    assert all(g is not None and torch.isfinite(g).all() for g in grads) and grads[0][:, :39].abs().max().item() > 0
    assert net.encoder.embeddings.grad is not None and torch.isfinite(net.encoder.embeddings.grad).all()


def test_operator_inside_a_captured_graph(device):
    """forward and backward launch on the current stream without a host synchronisation: a captured graph replays them on new inputs"""
    from nerfsafetyvalidation_amd.freqencoder import freq_encode
    g = torch.Generator().manual_seed(21)
    first, second = [(torch.rand(257, 3, generator=g) * 4 - 2).to(device) for _ in range(2)]
    grad = torch.randn(257, 39, generator=g).to(device)
    x = first.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):                                                         # warm-up outside the capture
            freq_encode(x, 6, 39).backward(grad)
            x.grad = None
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = freq_encode(x, 6, 39)
        out.backward(grad)
    for value in (second, first):
        with torch.no_grad():
            x.copy_(value)
        graph.replay()
        torch.cuda.synchronize()
        eager = value.clone().requires_grad_(True)
        want = freq_encode(eager, 6, 39)
        want.backward(grad)
        assert torch.equal(out, want) and torch.equal(x.grad, eager.grad)
